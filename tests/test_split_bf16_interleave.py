"""The two-set, interleaved K loop of the split-bf16 kernels (be_wino.hip: k_wino_gemm_ps; be_conv_pm_bf6.hip: k_conv_pm_bf6): chunk c's
MFMAs read register set c & 1 while chunk c + 1's fragments are read and split into the other set between them.

What such a loop can get wrong, at the smallest shapes that reach it: a stale or swapped set, an odd chunk total (the loop walks two
chunks per trip), a loop shorter than the three-chunk DMA prologue, a problem boundary right behind the first chunk, a partial row tile.

Exact-product tests: operands chosen so that every partial sum of every product of pieces is an fp32 value, so that ANY order of exact
operations gives the float64 product exactly - a wrong or stale piece cannot hide in a tolerance.  With x = s (1 + 2^-9 + 2^-17),
s in {+-1, +-2, +-3}: hi = s, mid = s 2^-9, lo = s 2^-17 (all three pieces carry bits); the other operand is in {0, +-1, +-2} with at
most 20 (rows) / 16 (layer0) non-zeros along K, so every partial sum is T_hi + T_mid 2^-9 + T_lo 2^-17 with integers |T| <= 120: a
multiple of 2^-17 below 2^7, 24 bits.  Then the Winograd layers against float64 (the bound of test_wino_split_bf16.py), run-to-run, and
non-finite inputs in an odd chunk (the second register set)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from conftest import relmax
from test_layer0_split_bf16 import COUT, _pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
C3 = 1.0 + 2.0 ** -9 + 2.0 ** -17
# row GEMMs: K = 16 / 48 / 96 is 1 / 3 / 6 chunks (the smallest K, an odd and an even count); M = 1, 130 (a partial second tile),
# 1152 (nine full tiles), and 66560 = 520 full tiles at N = 100: more workgroups than two rounds of the CUs, so that the launch walks
# several tiles per workgroup - problem boundaries behind chunk 1 (K = 16) and behind an odd chunk (K = 48)
ROW_KS = (16, 48, 96)
ROW_MNS = [(m, n) for m in (1, 130, 1152) for n in (100, 256)] + [(66560, 100)]
# layer0 (n, h, w, cin, cin2): 8 chunks per corner pixel ... 19 per interior pixel with the 1x1 behind; both parities
L0_SHAPES = [(3, 3, 3, 32, 0), (130, 3, 3, 32, 16), (3, 5, 9, 64, 64)]
WINO_LAYERS = [(32, 164), (64, 100), (96, 256)]          # 2 / 4 / 6 chunks per problem; partly empty and zero N tiles
WINO_NS = (1, 3, 65)


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


def _three_piece(shape, rng):
    s = rng.choice(np.array([-3, -2, -1, 1, 2, 3], np.float64), size=shape)
    v = s * C3
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return v


def _sparse_rows(rows, k, nnz, rng):
    """[rows][k] in {0, +-1, +-2} with at most nnz non-zeros per row"""
    v = np.zeros((rows, k))
    for r in range(rows):
        idx = rng.choice(k, size=min(nnz, k), replace=False)
        v[r, idx] = rng.choice(np.array([-2, -1, 1, 2], np.float64), size=idx.size)
    return v


def _sparse_rows_fast(rows, k, nnz, rng):
    """the same for many rows: non-zeros at nnz drawn columns per row (repeats merge: at most nnz)"""
    v = np.zeros((rows, k))
    idx = rng.integers(0, k, size=(rows, nnz))
    v[np.arange(rows)[:, None], idx] = rng.choice(np.array([-2, -1, 1, 2], np.float64), size=(rows, nnz))
    return v


def _packed(w):
    """the packed fp32 matrix [cout_pad32][K] of a 1x1 weight (zero rows past cout): what gemm_rows_bf6_pack splits (any K % 16 == 0)"""
    n, k = w.shape
    pw = torch.zeros((n + 31) // 32 * 32, k)
    pw[:n] = torch.as_tensor(w, dtype=torch.float32)
    return pw.reshape(-1).to(DEV)


def _exact_f32(ref):
    """the condition of an exact-product test: the float64 result is an fp32 value"""
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    return ref.astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", ROW_KS)
@pytest.mark.parametrize("pieces_in", ["a", "b"])
def test_row_gemm_exact_products(native, k, pieces_in):
    rng = np.random.default_rng(1200 + k + (pieces_in == "b"))
    m_max = max(m for m, _ in ROW_MNS)
    if pieces_in == "a":
        x, w = _three_piece((m_max, k), rng), _sparse_rows(256, k, 20, rng)
    else:
        x, w = _sparse_rows_fast(m_max, k, 20, rng), _three_piece((256, k), rng)
    xd = torch.from_numpy(x.astype(np.float32)).to(DEV)
    for n in (100, 256):
        wn = w[:n]
        ref = _exact_f32(x @ wn.T)
        assert (np.abs(x) @ np.abs(wn).T).max() < 128.0             # every partial sum stays below 2^7
        planes = native.gemm_rows_bf6_pack(_packed(wn), n, k)
        for m in [m for m, nn in ROW_MNS if nn == n]:
            y = native.gemm_rows_bf6(xd[:m].contiguous(), planes, n).cpu().numpy()
            bad = np.argwhere(y != ref[:m])
            assert bad.size == 0, (k, pieces_in, m, n, len(bad), bad[:4].tolist())


def _l0_ref(x, wt, x2, w2):
    y = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), padding=1)
    if w2 is not None:
        y = y + torch.nn.functional.conv2d(torch.from_numpy(x2).permute(0, 3, 1, 2), torch.from_numpy(w2))
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cin2", L0_SHAPES, ids=[f"n{s[0]}_{s[1]}x{s[2]}_c{s[3]}_x{s[4]}" for s in L0_SHAPES])
@pytest.mark.parametrize("pieces_in", ["a", "b"])
def test_layer0_exact_products(native, n, h, w, cin, cin2, pieces_in):
    rng = np.random.default_rng(1300 + n + cin2 + (pieces_in == "b"))
    ktot = 9 * cin + cin2
    if pieces_in == "a":
        # every output channel: at most 16 non-zero weights among its 9 cin + cin2
        x = _three_piece((n, h, w, cin), rng)
        x2 = _three_piece((n, h, w, cin2), rng) if cin2 else None
        wall = _sparse_rows(COUT, ktot, 16, rng)
    else:
        # every image: 10 non-zeros in x and 6 in x2, so that a window sees at most 16
        # (here the operand the kernel splits, x, is mostly zero: this case checks B's mid / lo planes; a stale or swapped A set is
        # case "a"'s to catch, where x is dense and carries all three pieces)
        x = _sparse_rows(n, h * w * cin, 10, rng).reshape(n, h, w, cin)
        x2 = _sparse_rows(n, h * w * cin2, 6, rng).reshape(n, h, w, cin2) if cin2 else None
        wall = _three_piece((COUT, ktot), rng)
    wt = wall[:, :9 * cin].reshape(COUT, cin, 3, 3).copy()
    w2 = wall[:, 9 * cin:].reshape(COUT, cin2, 1, 1).copy() if cin2 else None
    ref = _exact_f32(_l0_ref(x, wt, x2, w2))
    f32 = lambda a: None if a is None else torch.from_numpy(a.astype(np.float32))
    _, pb, planes, _ = _pack(native, f32(wt), torch.zeros(COUT), f32(w2))
    y = native.conv3x3_pm_bf6(f32(x).to(DEV), planes, pb, COUT, act=0, x2=f32(x2).to(DEV) if cin2 else None).cpu().numpy()
    bad = np.argwhere(y != ref)
    assert bad.size == 0, (pieces_in, len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------------------------------------------- Winograd layers

def _wino_inputs(cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(max(WINO_NS), 6, 6, cin, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * np.sqrt(2.0 / (9 * cin))
    b = 0.1 * torch.randn(cout, generator=g)
    return x, w, b


def _poisoned(x):
    """an inf and a NaN in channels 16-31: the second 16-deep chunk of the K loop, multiplied out of the second register set"""
    x = x.clone()
    x[3, 2, 2, 17] = float("inf")
    x[20, 5, 5, 19] = float("nan")
    return x


def run_cases():
    """Outputs of the Winograd layers (this process's arithmetic: bf16x6, or the fp32 GEMMs under BE_WINO_F32=1)."""
    from be_hip import native
    out = {}
    for i, (cin, cout) in enumerate(WINO_LAYERS):
        x, w, b = _wino_inputs(cin, cout, 1400 + i)
        uw, ub = native.wino_pack(w.to(DEV), b.to(DEV))
        for n in WINO_NS:
            out[f"l{i}_n{n}"] = native.wino_conv3x3(x[:n].contiguous().to(DEV), uw, ub, cout)[0].cpu().numpy()
        out[f"l{i}_nonfinite"] = native.wino_conv3x3(_poisoned(x).to(DEV), uw, ub, cout)[0].cpu().numpy()
    return out


_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_split_bf16_interleave as t
np.savez(os.environ["BE_OUT"], **t.run_cases())
'''


@pytest.fixture(scope="module")
def wino_outputs(native):
    return run_cases()


@pytest.fixture(scope="module")
def wino_fp32_outputs():
    """The same cases through the fp32 GEMMs (BE_WINO_F32=1: read once per process, hence the one child process of this module)."""
    with tempfile.TemporaryDirectory() as d:
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, "f32.npz"), BE_WINO_F32="1")
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, "f32.npz")))


@pytest.mark.gpu
def test_wino_layers_vs_fp64_and_patch_bits_do_not_depend_on_the_batch(wino_outputs, wino_fp32_outputs):
    """The bound of test_wino_split_bf16.py for the same kernel: within 1.5e-5 of float64 and at most 2 x the fp32 GEMMs' error."""
    for i, (cin, cout) in enumerate(WINO_LAYERS):
        x, w, b = _wino_inputs(cin, cout, 1400 + i)
        ref = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).numpy()
        for n in WINO_NS:
            y, y32 = wino_outputs[f"l{i}_n{n}"], wino_fp32_outputs[f"l{i}_n{n}"]
            e64, e64_f32 = relmax(y, ref[:n]), relmax(y32, ref[:n])
            print(f"{cin}->{cout} n {n}: bf16x6 vs fp64 {e64:.2e}, fp32 GEMMs vs fp64 {e64_f32:.2e}")
            assert e64 <= 1.5e-5 and e64 <= 2.0 * e64_f32, (cin, cout, n, e64, e64_f32)
            assert np.array_equal(y[0], wino_outputs[f"l{i}_n{max(WINO_NS)}"][0]), (cin, cout, n)


@pytest.mark.gpu
def test_wino_nonfinite_in_an_odd_chunk_stays_in_its_patches(wino_outputs, wino_fp32_outputs):
    for i, (cin, cout) in enumerate(WINO_LAYERS):
        new, old = wino_outputs[f"l{i}_nonfinite"], wino_fp32_outputs[f"l{i}_nonfinite"]
        bad = ~np.isfinite(old)
        assert bad.any() and np.array_equal(~np.isfinite(new), bad), (cin, cout)
        keep = np.setdiff1d(np.arange(max(WINO_NS)), [3, 20])
        assert np.array_equal(new[keep], wino_outputs[f"l{i}_n{max(WINO_NS)}"][keep]), (cin, cout)


def _rand_rows(m, k, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) * np.sqrt(2.0 / k)


@pytest.mark.gpu
def test_row_gemm_nonfinite_in_an_odd_chunk_stays_in_its_rows(native):
    for m, k, n in [(1152, 96, 256), (130, 48, 100)]:
        x, w = _rand_rows(m, k, n, 1500 + k)
        planes = native.gemm_rows_bf6_pack(_packed(w), n, k)
        clean = native.gemm_rows_bf6(x.to(DEV), planes, n).cpu().numpy()
        assert np.isfinite(clean).all()
        rows = [3, 129]
        x[3, 17] = float("inf")                        # k = 16 .. 31: chunk 1
        x[129, 16 + 5] = float("nan")
        y = native.gemm_rows_bf6(x.to(DEV), planes, n).cpu().numpy()
        assert not np.isfinite(y[rows]).any()
        keep = np.setdiff1d(np.arange(m), rows)
        assert np.array_equal(y[keep], clean[keep])


def _l0_rand(n, h, w, cin, cin2, seed):
    g = torch.Generator().manual_seed(seed)
    k = 9 * cin + cin2
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(COUT, cin, 3, 3, generator=g) * np.sqrt(2.0 / k)
    b = 0.1 * torch.randn(COUT, generator=g)
    x2 = torch.randn(n, h, w, cin2, generator=g)
    w2 = torch.randn(COUT, cin2, 1, 1, generator=g) * np.sqrt(2.0 / k)
    return x, wt, b, x2, w2


@pytest.mark.gpu
def test_layer0_nonfinite_in_an_odd_chunk_stays_under_its_taps(native):
    n, h, w, cin, cin2 = 130, 5, 9, 32, 16
    x, wt, b, x2, w2 = _l0_rand(n, h, w, cin, cin2, 1600)
    _, pb, planes, _ = _pack(native, wt, b, w2)
    clean = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=1, x2=x2.to(DEV)).cpu().numpy()
    assert np.isfinite(clean).all()
    # channels 16-31 of a 32-channel group: the second half of a tap, an odd chunk of the walk
    poison = [(0, 2, 4, 17, float("inf")), (129, 0, 0, 31, float("nan"))]
    for i, py, px, c, v in poison:
        x[i, py, px, c] = v
    y = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=1, x2=x2.to(DEV)).cpu().numpy()
    hit = np.zeros((n, h, w), bool)
    for i, py, px, _, _ in poison:
        hit[i, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    assert not np.isfinite(y[hit]).any()
    assert np.array_equal(y[~hit], clean[~hit])


@pytest.mark.gpu
def test_ten_runs_are_bit_identical(native):
    """A set read before its split is complete, or a chunk multiplied before its DMA has landed, shows here."""
    x, wt, b, x2, w2 = _l0_rand(130, 5, 9, 64, 64, 1700)
    _, pb, planes, _ = _pack(native, wt, b, w2)
    xd, x2d = x.to(DEV), x2.to(DEV)
    first = native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d)
    assert torch.isfinite(first).all()
    for _ in range(9):
        assert torch.equal(native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d), first)
    cin, cout = WINO_LAYERS[2]
    xw, w, bw = _wino_inputs(cin, cout, 1402)
    uw, ub = native.wino_pack(w.to(DEV), bw.to(DEV))
    xwd = xw.to(DEV)
    first, ws = native.wino_conv3x3(xwd, uw, ub, cout)
    first = first.clone()
    assert torch.isfinite(first).all()
    for _ in range(9):
        assert torch.equal(native.wino_conv3x3(xwd, uw, ub, cout, workspace=ws)[0], first)
