"""The split-bf16 (bf16x6) row GEMMs of LocalStage's eval path (be_wino.hip: k_wino_gemm_ps<EPI, 1> on pre-split weights): the 1x1
downsamples of layers 1-3 and fc.1.

CPU: the size of the planes.  GPU: the planes are the round-to-nearest-even split of the packed fp32 matrix in the block layout of the
Winograd planes; the row GEMM at the four LocalStage shapes gives a row the same bits in a large call and in a small one, and against a
float64 product errs at most 2 x what the fp32 path (native.conv_nhwc) errs on the same operands - the rule of the Winograd layers
(test_wino_split_bf16.py); non-finite inputs; and LocalStage's logits in child processes (the knobs are read once per process): inside
an arm (default / BE_ROWS_F32=1) a patch's bits depend on neither batch nor chunk, and the two arms differ by at most the logits'
tolerance."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import relmax
from test_wino_split_bf16 import split3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
# (K, N, [M ...]): the downsamples of layers 1-3 on 36 n rows, fc.1 on n rows
DOWN = [(96, 256), (256, 384), (384, 256)]
CASES = [(k, n, [36 * p for p in (1, 100, 1031, 4096)]) for k, n in DOWN] + [(2304, 1024, [1, 5, 1000, 4100])]
ODD = [(64, 100), (32, 164)]             # cout_pad32 = 128 / 192: a partly empty N tile, N tiles past cout_pad32 (zero rows of the planes)


def _lib():
    from be_hip import native
    return native.lib()


def test_packed_size_is_three_bf16_planes_of_cout_padded_to_128():
    lib = _lib()
    for cin, cout in DOWN + ODD + [(2304, 1024), (16, 4), (48, 130)]:
        assert lib.be_gemm_rows_bf6_packed_floats(cout, cin) == (cout + 127) // 128 * 128 * cin * 3 // 2, (cout, cin)
    assert lib.be_gemm_rows_bf6_packed_floats(64, 40) == 0
    assert lib.be_gemm_rows_bf6_packed_floats(64, 8) == 0


# ---------------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


def _operands(m, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) * np.sqrt(2.0 / k)
    b = 0.1 * torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    return x, w, b, res


def _smish64(v):
    return v * np.tanh(np.log1p(1.0 / (1.0 + np.exp(-v))))


@pytest.mark.gpu
def test_planes_are_the_rne_split_of_the_packed_matrix_in_block_layout(native):
    for i, (cin, cout) in enumerate(DOWN + ODD + [(2304, 1024)]):
        g = torch.Generator().manual_seed(400 + i)
        w = torch.randn(cout, cin, generator=g) * np.sqrt(2.0 / cin)
        pw, _ = native.conv_pack(w.to(DEV), None)
        planes = native.gemm_rows_bf6_pack(pw, cout, cin).cpu().numpy()
        cp32, nt, kc = (cout + 31) // 32 * 32, (cout + 127) // 128, cin // 16
        u = np.zeros((nt * 128, cin), np.float32)
        u[:cp32] = pw.cpu().numpy().reshape(cp32, cin)
        assert np.array_equal(u[:cout], w.numpy()) and np.all(u[cout:] == 0)
        # expected: [N tile][K chunk][plane][row][half][8] with the halves of rows 8-15, 24-31, ... swapped
        pieces = np.stack([p.view(np.uint32) >> 16 for p in split3(u)]).astype(np.uint16)        # [3][rows][cin]
        e = pieces.reshape(3, nt, 128, kc, 2, 8).transpose(1, 3, 0, 2, 4, 5).copy()
        swap = ((np.arange(128) >> 3) & 1).astype(bool)
        e[:, :, :, swap] = e[:, :, :, swap][..., ::-1, :]
        got = planes.view(np.uint16).reshape(nt, kc, 3, 128, 2, 8)
        assert np.array_equal(got, e), (cin, cout)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,ms", CASES, ids=[f"{k}x{n}" for k, n, _ in CASES])
def test_row_gemm_bits_do_not_depend_on_the_call_and_error_vs_fp64(native, k, n, ms):
    """bias + Smish + residual.  Rows of the largest call against the same rows in every smaller call: bit for bit.  Every call against
    float64: at most 2 x the fp32 path's error on the same operands (normal-distributed operands: the CPU emulation of the two
    arithmetics, lab/wino_split_bf16_error.py, gives 0.41-0.70 for the raw products)."""
    x, w, b, res = _operands(max(ms), k, n, 500 + k)
    pw, pb = native.conv_pack(w.to(DEV), b.to(DEV))
    planes = native.gemm_rows_bf6_pack(pw, n, k)
    xd, rd = x.to(DEV), res.to(DEV)
    big = native.gemm_rows_bf6(xd, planes, n, pb, rd, act=1)
    assert torch.isfinite(big).all()
    ref = _smish64(x.double().numpy() @ w.double().numpy().T + b.double().numpy() + res.double().numpy())
    for m in ms:
        y = native.gemm_rows_bf6(xd[:m].contiguous(), planes, n, pb, rd[:m].contiguous(), act=1)
        assert torch.equal(y, big[:m]), (k, n, m)
        y32 = native.conv_nhwc(xd[:m].reshape(m, 1, 1, k).contiguous(), pw, pb, n, 1, 1, residual=rd[:m].contiguous()).reshape(m, n)
        e64, e64_f32 = relmax(y.cpu().numpy(), ref[:m]), relmax(y32.cpu().numpy(), ref[:m])
        print(f"K {k} N {n} M {m}: bf16x6 vs fp64 {e64:.2e}, fp32 path vs fp64 {e64_f32:.2e}, ratio {e64 / e64_f32:.2f}")
        assert e64 <= 2.0 * e64_f32, (k, n, m, e64, e64_f32)
    # the raw-store form (no bias, residual, activation: the downsamples) and a row stride wider than N
    raw = native.gemm_rows_bf6(xd, planes, n)
    m = ms[1]
    out = torch.full((m, n + 8), 7.0, device=DEV)
    native.gemm_rows_bf6(xd[:m].contiguous(), planes, n, out=out)
    assert torch.equal(out[:, :n], raw[:m]) and bool((out[:, n:] == 7.0).all())
    raw64 = x.double().numpy() @ w.double().numpy().T
    y32 = native.conv_nhwc(xd.reshape(-1, 1, 1, k), pw, torch.zeros_like(pb), n, 1, 0).reshape(-1, n)
    e64, e64_f32 = relmax(raw.cpu().numpy(), raw64), relmax(y32.cpu().numpy(), raw64)
    print(f"K {k} N {n} M {max(ms)} raw: bf16x6 vs fp64 {e64:.2e}, fp32 path vs fp64 {e64_f32:.2e}, ratio {e64 / e64_f32:.2f}")
    assert e64 <= 2.0 * e64_f32


@pytest.mark.gpu
def test_nonfinite_inputs_stay_nonfinite_in_their_rows_only(native):
    for k, n, m in [(256, 384, 36 * 64), (2304, 1024, 300), (96, 256, 128 * 9 * 4)]:
        x, w, b, res = _operands(m, k, n, 600 + k)
        pw, pb = native.conv_pack(w.to(DEV), b.to(DEV))
        planes = native.gemm_rows_bf6_pack(pw, n, k)
        clean = native.gemm_rows_bf6(x.to(DEV), planes, n, pb, res.to(DEV), act=0)
        assert torch.isfinite(clean).all()
        rows = [3, 129, m - 1]
        x[3, 5] = float("inf")
        x[129, k - 1] = float("-inf")
        x[m - 1, 17] = float("nan")
        y = native.gemm_rows_bf6(x.to(DEV), planes, n, pb, res.to(DEV), act=0).cpu().numpy()
        assert not np.isfinite(y[rows]).any()
        keep = np.setdiff1d(np.arange(m), rows)
        assert np.array_equal(y[keep], clean.cpu().numpy()[keep])


BATCHES = (3, 700, 4096, 8492)
CHUNKS = (0, 1000, 4096)


def _logits():
    """LocalStage logits (Winograd path) of the first n patches of one seeded batch, for every batch size and chunk."""
    import models
    from be_hip import synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(BATCHES), name="rows_bf6"), dtype=np.float32)).to(DEV)
    out = {}
    with torch.no_grad():
        for n in BATCHES:
            for chunk in CHUNKS:
                m.chunk = chunk
                out[f"n{n}_c{chunk}"] = m(x[:n].contiguous()).cpu().numpy().copy()
    return out


_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_rows_split_bf16 as t
np.savez(os.environ["BE_OUT"], **t._logits())
'''


@pytest.mark.gpu
def test_local_stage_logits_per_arm_are_batch_and_chunk_independent_and_the_arms_agree(native):
    def arm(d, name, **knobs):
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"))
        for k in ("BE_WINO_F32", "BE_ROWS_F32"):
            env.pop(k, None)
        env.update(knobs)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, name + ".npz")))

    with tempfile.TemporaryDirectory() as d:
        arms = {"default": arm(d, "default"), "rows_f32": arm(d, "rows_f32", BE_ROWS_F32="1")}
    for name, a in arms.items():
        full = a[f"n{max(BATCHES)}_c0"]
        assert np.isfinite(full).all()
        for n in BATCHES:
            for chunk in CHUNKS:
                assert a[f"n{n}_c{chunk}"].tobytes() == full[:n].tobytes(), (name, n, chunk)
    new, old = arms["default"][f"n{max(BATCHES)}_c0"], arms["rows_f32"][f"n{max(BATCHES)}_c0"]
    assert new.tobytes() != old.tobytes()                            # the knob reaches the kernels
    e = relmax(new, old)
    print(f"default vs BE_ROWS_F32=1 logits: relmax {e:.2e}")
    assert e <= 1e-5
