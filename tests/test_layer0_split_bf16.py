"""LocalStage's layer0 in split-bf16 (bf16x6) arithmetic (be_conv_pm_bf6.hip: k_conv_pm_bf6 on pre-split weights): the pixel-major 3x3
convolution 64 -> 96 and the fused 3x3 96 -> 96 + 1x1 64 -> 96 on the 11x11 maps.

CPU: the size of the planes.  GPU: the planes are the round-to-nearest-even split of the packed fp32 matrix in the block layout of the
row GEMMs' planes, one 12-KB block per 16-deep chunk of the pixel-major K walk; an image gets the same bits in a large call and in a
small one; against a float64 convolution the kernel errs at most 2 x what the fp32 path (native.conv_nhwc / conv_nhwc_fused2) errs on
the same operands - the rule of the Winograd layers and the row GEMMs; non-finite inputs; run-to-run; bad arguments; and LocalStage's
logits in child processes (the knobs are read once per process): inside an arm (default / BE_L0_F32=1) a patch's bits depend on neither
batch nor chunk, and the two arms differ by at most the logits' tolerance."""
import ctypes as C
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
COUT = 96
# (n, h, w, cin, cin2): layer0's two launches, then every pixel on the border, a non-square map, the fused form with one and four x2 chunks
L0_PLAIN, L0_FUSED = (300, 11, 11, 64, 0), (300, 11, 11, 96, 64)
SHAPES = [L0_PLAIN, L0_FUSED, (300, 3, 3, 64, 0), (257, 5, 9, 32, 0), (300, 7, 7, 32, 16), (300, 7, 7, 32, 64)]


def _lib():
    from be_hip import native
    return native.lib()


def test_packed_size_is_three_bf16_planes_of_128_rows_per_k_column():
    lib = _lib()
    for cin, cin2 in [(64, 0), (96, 64), (32, 0), (32, 16), (32, 64)]:
        for cout in (96, 65, 80):
            assert lib.be_conv3x3_pm_bf6_packed_floats(cout, cin, cin2) == 128 * (9 * cin + cin2) * 3 // 2, (cout, cin, cin2)
            assert lib.be_conv3x3_pm_bf6_packed_floats(cout, cin, cin2) == lib.be_gemm_rows_bf6_packed_floats(cout, 9 * cin + cin2)
    for cout, cin, cin2 in [(64, 64, 0), (128, 64, 0), (97, 64, 0), (0, 64, 0), (96, 48, 0), (96, 16, 0), (96, 0, 0), (96, 64, 8), (96, 64, -16)]:
        assert lib.be_conv3x3_pm_bf6_packed_floats(cout, cin, cin2) == 0, (cout, cin, cin2)


# ---------------------------------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


def _operands(n, h, w, cin, cin2, seed):
    g = torch.Generator().manual_seed(seed)
    k = 9 * cin + cin2
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(COUT, cin, 3, 3, generator=g) * np.sqrt(2.0 / k)
    b = 0.1 * torch.randn(COUT, generator=g)
    x2 = torch.randn(n, h, w, cin2, generator=g) if cin2 else None
    w2 = torch.randn(COUT, cin2, 1, 1, generator=g) * np.sqrt(2.0 / k) if cin2 else None
    return x, wt, b, x2, w2


def _pack(native, wt, b, w2):
    """-> (packed fp32 matrix for the fp32 path, packed bias, planes, zero channels the fp32 path needs behind x2).  The fp32 fused
    path packs cin2 % 32 == 0 only: at cin2 = 16 it gets w2 and x2 with 16 zero channels appended (they add exactly 0: the same
    operands), and the planes come from the first 9 cin + 16 columns of that packed matrix."""
    cin, cin2 = wt.shape[1], (w2.shape[1] if w2 is not None else 0)
    pad = -cin2 % 32
    if w2 is None:
        pw, pb = native.conv_pack(wt.to(DEV), b.to(DEV))
    else:
        pw, pb = native.conv_pack_fused2(wt.to(DEV), b.to(DEV), None, torch.nn.functional.pad(w2, (0, 0, 0, 0, 0, pad)).to(DEV), None, None)
    m = pw if not pad else pw.reshape(COUT, 9 * cin + cin2 + pad)[:, :9 * cin + cin2].contiguous().reshape(-1)
    return pw, pb, native.conv3x3_pm_bf6_pack(m, COUT, cin, cin2), pad


def _smish64(v):
    return v * np.tanh(np.log1p(1.0 / (1.0 + np.exp(-v))))


def _ref64(x, wt, b, x2, w2):
    """float64 on the CPU: conv2d (+ the 1x1 on x2) + bias, Smish; NHWC like the kernel's output"""
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), b.double(), padding=1)
    if w2 is not None:
        y = y + torch.nn.functional.conv2d(x2.double().permute(0, 3, 1, 2), w2.double())
    return _smish64(y.permute(0, 2, 3, 1).numpy())


@pytest.mark.gpu
def test_planes_are_the_rne_split_of_the_packed_matrix_one_block_per_walk_chunk(native):
    for i, (cin, cin2) in enumerate([(64, 0), (96, 64)]):
        _, wt, b, _, w2 = _operands(1, 3, 3, cin, cin2, 700 + i)
        pw, _, planes, _ = _pack(native, wt, b, w2)
        ktot, kc = 9 * cin + cin2, (9 * cin + cin2) // 16
        assert ktot == (576, 928)[i]
        m = pw.cpu().numpy().reshape(COUT, ktot)
        # the packed matrix's K order is the pixel-major K walk's: (32-channel chunk, tap, channel), the 1x1 behind ncc * 9 * 32
        main = m[:, :9 * cin].reshape(COUT, cin // 32, 9, 32)
        assert np.array_equal(main, wt.numpy().reshape(COUT, cin // 32, 32, 9).transpose(0, 1, 3, 2))
        if cin2:
            assert np.array_equal(m[:, 9 * cin:], w2.numpy().reshape(COUT, cin2))
        u = np.zeros((128, ktot), np.float32)
        u[:COUT] = m
        # expected: [K chunk][plane][row][half][8] with the halves of rows 8-15, 24-31, ... swapped
        pieces = np.stack([p.view(np.uint32) >> 16 for p in split3(u)]).astype(np.uint16)        # [3][128][ktot]
        e = pieces.reshape(3, 128, kc, 2, 8).transpose(2, 0, 1, 3, 4).copy()
        swap = ((np.arange(128) >> 3) & 1).astype(bool)
        e[:, :, swap] = e[:, :, swap][..., ::-1, :]
        got = planes.cpu().numpy().view(np.uint16).reshape(kc, 3, 128, 2, 8)
        assert np.array_equal(got, e), (cin, cin2)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cin2", [(64, 0), (96, 64)], ids=["conv1", "conv2_fused"])
def test_bits_do_not_depend_on_the_call(native, cin, cin2):
    """bias + Smish.  The images of an n = 600 call against the same images run as n = 1, 3, 255, 257 (with the kernel's 128-image tiles: partly filled tiles,
    two tiles less one image, two tiles plus one, a ragged multi-tile batch): bit for bit;
    and a row stride wider than cout with the sentinel columns untouched."""
    x, wt, b, x2, w2 = _operands(600, 11, 11, cin, cin2, 710 + cin)
    _, pb, planes, _ = _pack(native, wt, b, w2)
    xd, x2d = x.to(DEV), (x2.to(DEV) if cin2 else None)
    big = native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d)
    assert torch.isfinite(big).all()
    for n in (1, 3, 255, 257):
        y = native.conv3x3_pm_bf6(xd[:n].contiguous(), planes, pb, COUT, act=1, x2=x2d[:n].contiguous() if cin2 else None)
        assert torch.equal(y, big[:n]), (cin, cin2, n)
    # the same images at another position of the batch (another row of another tile)
    y = native.conv3x3_pm_bf6(xd[130:400].contiguous(), planes, pb, COUT, act=1, x2=x2d[130:400].contiguous() if cin2 else None)
    assert torch.equal(y, big[130:400])
    n = 257
    out = torch.full((n, 11, 11, COUT + 8), 7.0, device=DEV)
    native.conv3x3_pm_bf6(xd[:n].contiguous(), planes, pb, COUT, act=1, x2=x2d[:n].contiguous() if cin2 else None, out=out)
    assert torch.equal(out[..., :COUT], big[:n]) and bool((out[..., COUT:] == 7.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cin2", SHAPES, ids=[f"n{s[0]}_{s[1]}x{s[2]}_c{s[3]}_x{s[4]}" for s in SHAPES])
def test_error_vs_fp64_at_most_twice_the_fp32_paths(native, n, h, w, cin, cin2):
    """Normal-distributed operands, weights scaled by sqrt(2 / K); float64 conv2d + Smish on the CPU.  The rule of the two earlier
    split-bf16 changes (ratio measured there 0.55-1.06): relmax <= 2 x the fp32 path's relmax on the same operands."""
    x, wt, b, x2, w2 = _operands(n, h, w, cin, cin2, 720 + h * w + cin2)
    pw, pb, planes, pad = _pack(native, wt, b, w2)
    xd, x2d = x.to(DEV), (x2.to(DEV) if cin2 else None)
    y = native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d)
    y32 = native.conv_nhwc_fused2(xd, torch.nn.functional.pad(x2d, (0, pad)).contiguous(), pw, pb, COUT, 3, 1) if cin2 else native.conv_nhwc(xd, pw, pb, COUT, 3, 1)
    ref = _ref64(x, wt, b, x2, w2)
    assert torch.isfinite(y).all()
    e64, e64_f32 = relmax(y.cpu().numpy(), ref), relmax(y32.cpu().numpy(), ref)
    print(f"n {n} {h}x{w} cin {cin} cin2 {cin2}: bf16x6 vs fp64 {e64:.2e}, fp32 path vs fp64 {e64_f32:.2e}, ratio {e64 / e64_f32:.2f}")
    assert e64 <= 2.0 * e64_f32, (n, h, w, cin, cin2, e64, e64_f32)


@pytest.mark.gpu
def test_nonfinite_inputs_stay_nonfinite_under_their_taps_only(native):
    n, h, w, cin, _ = L0_PLAIN
    x, wt, b, _, _ = _operands(n, h, w, cin, 0, 730)
    _, pb, planes, _ = _pack(native, wt, b, None)
    clean = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=1).cpu().numpy()
    assert np.isfinite(clean).all()
    # (image, y, x, channel): the first row of a tile, the first row of the next tile (128 | 256 rows), the last image
    poison = [(0, 5, 5, 7, float("inf")), (128, 0, 0, 63, float("-inf")), (256, 3, 10, 31, float("nan")), (n - 1, 10, 4, 17, float("nan"))]
    for i, py, px, c, v in poison:
        x[i, py, px, c] = v
    y = native.conv3x3_pm_bf6(x.to(DEV), planes, pb, COUT, act=1).cpu().numpy()
    hit = np.zeros((n, h, w), bool)
    for i, py, px, _, _ in poison:
        hit[i, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True
    assert not np.isfinite(y[hit]).any()
    assert np.array_equal(y[~hit], clean[~hit])          # every other image, and every other pixel of the poisoned ones


@pytest.mark.gpu
def test_ten_runs_of_the_fused_form_are_bit_identical(native):
    """The hand-counted vmcnt waits are the reason for this test: a chunk multiplied before its DMA has landed shows here."""
    x, wt, b, x2, w2 = _operands(600, 11, 11, 96, 64, 740)
    _, pb, planes, _ = _pack(native, wt, b, w2)
    xd, x2d = x.to(DEV), x2.to(DEV)
    first = native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d)
    for _ in range(9):
        assert torch.equal(native.conv3x3_pm_bf6(xd, planes, pb, COUT, act=1, x2=x2d), first)


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(native):
    lib = native.lib()
    x = torch.randn(4, 11, 11, 64, device=DEV)
    x48 = torch.randn(4, 11, 11, 48, device=DEV)
    planes = torch.zeros(lib.be_conv3x3_pm_bf6_packed_floats(96, 64, 0) + 4, device=DEV)
    pb = torch.zeros(96, device=DEV)
    y = torch.full((4, 11, 11, 96), 7.0, device=DEV)
    s = native.stream_ptr(x.device)

    def call(d, xp, plp, x2p=None, cin2=0):
        return lib.be_conv3x3_pm_bf6_f32(C.byref(d), xp, x2p, cin2, plp, C.c_void_p(pb.data_ptr()), C.c_void_p(y.data_ptr()), 96, s)

    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    good = native.ConvDesc(4, 11, 11, 64, 96, 3, 1)
    assert call(good, None, P(planes)) != 0                                              # null pointer
    assert call(good, P(x), None) != 0
    assert call(native.ConvDesc(4, 11, 11, 64, 64, 3, 1), P(x), P(planes)) != 0          # cout_pad32 != 96
    assert call(native.ConvDesc(4, 11, 11, 48, 96, 3, 1), P(x48), P(planes)) != 0        # cin % 32
    assert call(native.ConvDesc(4, 2, 11, 64, 96, 3, 1), P(x), P(planes)) != 0           # h < 3
    assert call(native.ConvDesc(4, 11, 2, 64, 96, 3, 1), P(x), P(planes)) != 0           # w < 3
    assert call(good, P(x, 4), P(planes)) != 0                                           # misaligned pointers
    assert call(good, P(x), P(planes, 4)) != 0
    assert call(good, P(x), P(planes), P(x), 8) != 0                                     # cin2 % 16
    assert call(native.ConvDesc(4, 11, 11, 64, 96, 1, 1), P(x), P(planes)) != 0          # not a 3x3
    with pytest.raises(RuntimeError):
        native.conv3x3_pm_bf6_pack(torch.zeros(64 * 576, device=DEV), 64, 64)
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                                                         # nothing was launched
    assert call(good, P(x), P(planes)) == 0                                               # and the good call is taken
    torch.cuda.synchronize()
    assert bool((y != 7.0).all())


BATCHES = (3, 300, 700)
CHUNKS = (0, 256)


def _logits():
    """LocalStage logits (Winograd path) of the first n patches of one seeded batch, for every batch size and chunk."""
    import models
    from be_hip import synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(BATCHES), name="l0_bf6"), dtype=np.float32)).to(DEV)
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
import test_layer0_split_bf16 as t
np.savez(os.environ["BE_OUT"], **t._logits())
'''


@pytest.mark.gpu
def test_local_stage_logits_per_arm_are_batch_and_chunk_independent_and_the_arms_agree(native):
    def arm(d, name, **knobs):
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"))
        for k in ("BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32"):
            env.pop(k, None)
        env.update(knobs)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, name + ".npz")))

    with tempfile.TemporaryDirectory() as d:
        arms = {"default": arm(d, "default"), "l0_f32": arm(d, "l0_f32", BE_L0_F32="1"),
                "l0_f32_rows_bf6": arm(d, "l0_f32_rows_bf6", BE_L0_F32="1", BE_ROWS_F32="0")}
    for name, a in arms.items():
        full = a[f"n{max(BATCHES)}_c0"]
        assert np.isfinite(full).all()
        for n in BATCHES:
            for chunk in CHUNKS:
                assert a[f"n{n}_c{chunk}"].tobytes() == full[:n].tobytes(), (name, n, chunk)
    new, old = arms["default"][f"n{max(BATCHES)}_c0"], arms["l0_f32"][f"n{max(BATCHES)}_c0"]
    assert new.tobytes() != old.tobytes()                            # the knob reaches the kernel
    e = relmax(new, old)
    print(f"default vs BE_L0_F32=1 logits: relmax {e:.2e}")
    assert e <= 1e-5
    assert old.tobytes() == arms["l0_f32_rows_bf6"][f"n{max(BATCHES)}_c0"].tobytes()     # no other knob is disturbed
