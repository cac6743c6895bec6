"""The split-bf16 (bf16x6) arithmetic of the Winograd transform-domain GEMMs (be_wino.hip, k_wino_gemm_ps).

CPU: the three-piece split x = hi + mid + lo (each piece a bf16 rounded to nearest-even from what is left) is exact, on the same
operation sequence as the kernel's split8.  GPU: the six LocalStage Winograd layer shapes against float64 and against the fp32 GEMMs
(BE_WINO_F32=1, in a child process: the knob is read once per process), the three batch regimes on equal bits, non-finite inputs."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import relmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LAYERS = [(96, 256), (256, 256), (256, 384), (384, 384), (384, 256), (256, 256)]   # LocalStage layers 1-3, conv1 / conv2 each


def bf16_rne(x):
    """float32 -> the float32 value of its bf16 (round to nearest even; what v_cvt_pk_bf16_f32 computes for finite x)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    r = (x - hi).astype(np.float32)
    mid = bf16_rne(r)
    lo = bf16_rne((r - mid).astype(np.float32))
    return hi, mid, lo


def test_split_is_exact_on_random_and_edge_values():
    rng = np.random.default_rng(7)
    rnd = np.concatenate([rng.standard_normal(200000), rng.standard_normal(50000) * 1e6, rng.standard_normal(50000) * 1e-20])
    p2 = np.ldexp(1.0, np.arange(-100, 120))
    edge = np.concatenate([p2, -p2, p2 * (1 + 2.0 ** -8), p2 * (2 - 2.0 ** -23), p2 * (1 + 2.0 ** -9 + 2.0 ** -23),   # round up a binade
                           p2 * (1 + 2.0 ** -8 + 2.0 ** -16 + 2.0 ** -23), [0.0, -0.0, 1e-30, -3e-31, 3.0e38]])
    x = np.concatenate([rnd, edge]).astype(np.float32)
    hi, mid, lo = split3(x)
    for piece in (hi, mid, lo):                                     # every piece is a bf16 value
        assert np.all(piece.view(np.uint32) & 0xFFFF == 0)
    s = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(s, x.astype(np.float64))                 # exact
    ax = np.abs(x.astype(np.float64))
    assert np.all(np.abs(mid) <= 2.0 ** -8 * ax) and np.all(np.abs(lo) <= 2.0 ** -16 * ax)
    # rounding up a binade: 2 - 2^-23 -> hi = 2, mid = -2^-23 (negative pieces carry the rest)
    h, m, lw = split3(np.float32(2 - 2.0 ** -23))
    assert (float(h), float(m) + float(lw)) == (2.0, -2.0 ** -23)


def test_split_below_the_bf16_normal_range_loses_only_subnormal_bits():
    """|x| < ~2^-110: lo falls under 2^-126 and is rounded to the bf16 subnormal grid (2^-133); the loss stays below that grid."""
    x = (np.ldexp(1.0, -118) * (1 + np.arange(1, 2000) * 2.0 ** -23)).astype(np.float32)
    hi, mid, lo = split3(x)
    err = np.abs(hi.astype(np.float64) + mid + lo - x.astype(np.float64))
    assert err.max() <= 2.0 ** -134 and err.max() > 0


# ---------------------------------------------------------------------------------------------------------------------- GPU

_CHILD = r'''
import os, sys
import numpy as np, torch
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd")]
sys.path.insert(0, os.path.join(os.environ["BE_ROOT"], "tests"))
import test_wino_split_bf16 as t
np.savez(os.environ["BE_OUT"], **t.run_cases())
'''


def _inputs(n, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 6, 6, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * np.sqrt(2.0 / (9 * cin))
    b = 0.1 * torch.randn(cout, generator=g)
    return x, w, b


def run_cases():
    """Outputs of the Winograd layers on fixed inputs (this process's arithmetic: bf16x6, or fp32 under BE_WINO_F32=1)."""
    from be_hip import native
    out = {}
    for i, (cin, cout) in enumerate(LAYERS):
        x, w, b = _inputs(700, cin, cout, 100 + i)
        uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
        y, _ = native.wino_conv3x3(x.to(DEV), uw, ub, cout)
        out[f"layer{i}"] = y.cpu().numpy()
    x, w, b = _inputs(64, 256, 256, 7)
    x[3, 2, 2, 5] = float("inf")
    x[9, 0, 4, 17] = float("-inf")
    x[20, 5, 5, 100] = float("nan")
    uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
    y, _ = native.wino_conv3x3(x.to(DEV), uw, ub, 256)
    out["nonfinite"] = y.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.fixture(scope="module")
def fp32_outputs():
    """The same cases through the fp32 GEMMs (BE_WINO_F32=1) in a fresh child process."""
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, "f32.npz"), BE_WINO_F32="1")
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, "f32.npz")))


@pytest.mark.gpu
def test_split_bf16_layers_vs_fp64_and_the_fp32_gemms(native, fp32_outputs):
    """Each of the six layer shapes: bf16x6 within the Winograd layer bound of the fp64 result (1.5e-5) and no worse than 2x the
    fp32 GEMMs' error on the same data.  (The two differ from each other by about as much as each differs from fp64: the rounding of
    the transform-domain sums dominates both, and it is uncorrelated between the two arithmetics.)"""
    new = run_cases()
    for i, (cin, cout) in enumerate(LAYERS):
        x, w, b = _inputs(700, cin, cout, 100 + i)
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).numpy()
        e64, e32 = relmax(new[f"layer{i}"], ref), relmax(new[f"layer{i}"], fp32_outputs[f"layer{i}"])
        e64_f32 = relmax(fp32_outputs[f"layer{i}"], ref)
        print(f"{cin}->{cout}: bf16x6 vs fp64 {e64:.2e} (fp32 GEMMs {e64_f32:.2e}), vs fp32 GEMMs {e32:.2e}")
        assert e64 <= 1.5e-5 and e64 <= 2.0 * e64_f32


@pytest.mark.gpu
def test_nonfinite_inputs_stay_nonfinite(native, fp32_outputs):
    """Inf / NaN in a patch: its outputs are non-finite where the fp32 GEMMs' are, and the other patches keep the clean run's bits."""
    new = run_cases()["nonfinite"]
    old = fp32_outputs["nonfinite"]
    bad = ~np.isfinite(old)
    assert bad.any() and np.array_equal(~np.isfinite(new), bad)
    x, w, b = _inputs(64, 256, 256, 7)
    uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
    clean, _ = native.wino_conv3x3(x.to(DEV), uw, ub, 256)
    keep = np.setdiff1d(np.arange(64), [3, 9, 20])
    assert np.array_equal(new[keep], clean.cpu().numpy()[keep])


@pytest.mark.gpu
def test_three_batch_regimes_give_equal_bits(native):
    """700 patches (plane-major buffers), 1501 (tile-major, a partly empty last row tile), 4096 (tile-major, full tiles: the
    fp32 GEMMs' weight-stationary regime): the first 700 patches' outputs are bit-identical in all three."""
    x, w, b = _inputs(4096, 256, 384, 11)
    uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
    xd = x.to(DEV)
    ys = [native.wino_conv3x3(xd[:n].contiguous(), uw, ub, 384, act=1)[0][:700] for n in (700, 1501, 4096)]
    assert torch.isfinite(ys[0]).all()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
