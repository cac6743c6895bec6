"""LocalStage's head in split-bf16 (bf16x6) arithmetic (be_conv1_pool_bf6.hip: k_conv1_pool_bf6, the image pre-split to bf16 planes in
LDS, the weights split once per wave in registers): conv1 7x7 + folded BatchNorm + Smish + MaxPool2d(3, 2, 1) in one image-major launch.

GPU: an image gets the same bits whatever call, workgroup and position it is computed in; against a float64 Conv2d + BatchNorm (eval) +
Smish + MaxPool2d the kernel errs at most 2 x what the fp32 kernel (be_conv7x7_pool_nhwc4p_f32) errs on the same operands - the rule
of every split-bf16 kernel here; a non-finite pixel disturbs only the pooled cells within its 7 x 7 taps' reach; run-to-run; bad
arguments; and LocalStage's logits in child processes (the knobs are read once per process): inside an arm (default / BE_C1_F32=1) a
patch's bits depend on neither batch nor chunk, the two arms differ by at most the logits' tolerance, and BE_WINO_F32=1 is not
disturbed by BE_C1_F32."""
import ctypes as C
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
N = 1031                     # ragged: with two workgroups per CU (512 on 256 CUs) two or three images per workgroup
R, OR = 21, 11


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.fixture(scope="module")
def ops(native):
    """Inputs and weights of test_hip_parity's conv1-pool test at n = 1031: (rand - 0.3) * 3, BatchNorm folded into the pack; the
    padded staging; the n = 1031 run every other call is compared with; the float64 reference of the first 8 images."""
    g = torch.Generator().manual_seed(100 + N)
    x = (torch.rand(N, 3, R, R, generator=g) - 0.3) * 3.0
    w = (torch.rand(64, 3, 7, 7, generator=g) - 0.5) * 0.4
    b = torch.rand(64, generator=g) - 0.5
    bn = (0.5 + torch.rand(64, generator=g), torch.rand(64, generator=g) - 0.5, torch.rand(64, generator=g) - 0.5,
          0.5 + torch.rand(64, generator=g))
    pw, pb = native.conv_pack(w.to(DEV), b.to(DEV), bn=tuple(t.to(DEV) for t in bn))
    xp = native.nchw3_to_nhwc4p(x.to(DEV))
    big = native.conv7x7_pool_bf6_nhwc4p(xp, pw, pb)
    assert big.shape == (N, OR, OR, 64) and bool(torch.isfinite(big).all())

    def ref64(xs):
        y = torch.nn.functional.conv2d(xs.double(), w.double(), b.double(), padding=3)
        ga, be_, mu, var = (t.double()[None, :, None, None] for t in bn)
        y = (y - mu) / torch.sqrt(var + 1e-5) * ga + be_
        y = y * torch.tanh(torch.log(1 + torch.sigmoid(y)))
        return torch.nn.functional.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).numpy()

    return dict(x=x, xp=xp, pw=pw, pb=pb, big=big, ref64=ref64)


@pytest.mark.gpu
def test_bits_do_not_depend_on_the_call(native, ops):
    """n = 1031 exercises the buffer hand-over and the cell reset (2-3 images per workgroup); the first 1, 3, 255 and 600 images and
    images [130:400] as calls of their own (other workgroups, other positions in a workgroup's sequence): bit for bit."""
    xp, pw, pb, big = ops["xp"], ops["pw"], ops["pb"], ops["big"]
    for n in (1, 3, 255, 600):
        assert torch.equal(native.conv7x7_pool_bf6_nhwc4p(xp[:n].contiguous(), pw, pb), big[:n]), n
    assert torch.equal(native.conv7x7_pool_bf6_nhwc4p(xp[130:400].contiguous(), pw, pb), big[130:400])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["wide", "unit"])
def test_error_vs_fp64_at_most_twice_the_fp32_kernels(native, ops, which):
    """The first 8 images against float64 Conv2d + BatchNorm (eval) + Smish + MaxPool2d: relmax <= 2 x the fp32 kernel's relmax on the
    same operands.  `wide`: the (rand - 0.3) * 3 input; `unit`: pixels in [0, 1]."""
    pw, pb = ops["pw"], ops["pb"]
    if which == "wide":
        x = ops["x"][:8]
    else:
        x = torch.rand(8, 3, R, R, generator=torch.Generator().manual_seed(1869))
    xp = native.nchw3_to_nhwc4p(x.to(DEV))
    ref = ops["ref64"](x)
    y = native.conv7x7_pool_bf6_nhwc4p(xp, pw, pb)
    y32 = native.conv7x7_pool_nhwc4p(xp, pw, pb)
    assert torch.isfinite(y).all()
    e, e32 = relmax(y.cpu().numpy(), ref), relmax(y32.cpu().numpy(), ref)
    print(f"{which}: bf16x6 vs fp64 {e:.3e}, fp32 kernel vs fp64 {e32:.3e}, ratio {e / e32:.2f}")
    assert e <= 2.0 * e32, (which, e, e32)


@pytest.mark.gpu
def test_nonfinite_pixels_disturb_only_the_cells_in_their_reach(native, ops):
    """+inf, -inf and NaN at single pixels of the first image, of an image that is a workgroup's second, and of the last.  Every other
    image, and every pooled cell of those three whose 3 x 3 window holds no conv output within 3 pixels of the poisoned pixel, keeps
    the clean run's bits.  Nothing is asserted about the cells inside that reach (the maxima drop NaN: be_conv1_pool_bf6.hip)."""
    pw, pb, clean = ops["pw"], ops["pb"], ops["big"].cpu().numpy()
    grid = min(N, 2 * torch.cuda.get_device_properties(0).multi_processor_count)
    second = grid + 5 if grid + 5 < N - 1 else N // 2
    poison = [(0, 1, 10, 10, float("inf")), (second, 0, 0, 0, float("-inf")), (N - 1, 2, 20, 17, float("nan"))]
    x = ops["x"].clone()
    for i, c, py, px, v in poison:
        x[i, c, py, px] = v
    y = native.conv7x7_pool_bf6_nhwc4p(native.nchw3_to_nhwc4p(x.to(DEV)), pw, pb).cpu().numpy()
    keep = np.ones((N, OR, OR), bool)
    for i, _, py, px, _ in poison:
        for a in range(OR):
            for b in range(OR):
                rows = [r for r in (2 * a - 1, 2 * a, 2 * a + 1) if 0 <= r < R]
                cols = [c for c in (2 * b - 1, 2 * b, 2 * b + 1) if 0 <= c < R]
                if any(abs(r - py) <= 3 for r in rows) and any(abs(c - px) <= 3 for c in cols):
                    keep[i, a, b] = False
    assert keep.sum() < keep.size and keep[[p[0] for p in poison]].any(axis=(1, 2)).all()
    assert np.array_equal(y[keep], clean[keep])


@pytest.mark.gpu
def test_ten_runs_are_bit_identical(native, ops):
    """A racy LDS hand-over (the image buffer is refilled while the pooled map is written) shows here."""
    xp, pw, pb = ops["xp"][:600].contiguous(), ops["pw"], ops["pb"]
    for _ in range(10):
        assert torch.equal(native.conv7x7_pool_bf6_nhwc4p(xp, pw, pb), ops["big"][:600])


@pytest.mark.gpu
def test_bad_arguments_are_refused_before_any_launch(native, ops):
    lib = native.lib()
    xp, pw, pb = ops["xp"][:4].contiguous(), ops["pw"], ops["pb"]
    y = torch.full((4 * OR * OR * 64 + 4,), 7.0, device=DEV)
    s = native.stream_ptr(xp.device)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

    def call(xq, n, wq, yq):
        return lib.be_conv7x7_pool_bf6_nhwc4p_f32(xq, n, wq, P(pb), yq, s)

    assert call(None, 4, P(pw), P(y)) != 0                  # null pointers
    assert call(P(xp), 4, None, P(y)) != 0
    assert call(P(xp), 4, P(pw), None) != 0
    assert call(P(xp, 4), 3, P(pw), P(y)) != 0              # misaligned pointers
    assert call(P(xp), 4, P(pw, 4), P(y)) != 0
    assert call(P(xp), 4, P(pw), P(y, 4)) != 0
    assert call(P(xp), 0, P(pw), P(y)) != 0                 # n <= 0
    assert call(P(xp), -1, P(pw), P(y)) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                           # nothing was launched
    assert call(P(xp), 4, P(pw), P(y)) == 0                 # and the good call is taken
    torch.cuda.synchronize()
    assert torch.equal(y[:4 * OR * OR * 64].reshape(4, OR, OR, 64), ops["big"][:4]) and bool((y[4 * OR * OR * 64:] == 7.0).all())


BATCHES = (3, 300, 700)
CHUNKS = (0, 256)
KNOBS = ("BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32", "BE_C1_F32", "BE_NO_CONV_PM", "BE_NO_CONV1_POOL")


def _logits():
    """LocalStage logits (Winograd path) of the first n patches of one seeded batch, for every batch size and chunk."""
    import models
    from be_hip import synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(BATCHES), name="c1_bf6"), dtype=np.float32)).to(DEV)
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
import test_conv1_pool_split_bf16 as t
np.savez(os.environ["BE_OUT"], **t._logits())
'''


@pytest.mark.gpu
def test_local_stage_logits_per_arm_are_batch_and_chunk_independent_and_the_arms_agree(native):
    def arm(d, name, **knobs):
        env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"))
        for k in KNOBS:
            env.pop(k, None)
        env.update(knobs)
        r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return dict(np.load(os.path.join(d, name + ".npz")))

    with tempfile.TemporaryDirectory() as d:
        arms = {"default": arm(d, "default"), "c1_f32": arm(d, "c1_f32", BE_C1_F32="1"),
                "wino_f32": arm(d, "wino_f32", BE_WINO_F32="1"), "wino_f32_c1_f32": arm(d, "wino_f32_c1_f32", BE_WINO_F32="1", BE_C1_F32="1")}
    top = f"n{max(BATCHES)}_c0"
    for name in ("default", "c1_f32"):
        full = arms[name][top]
        assert np.isfinite(full).all()
        for n in BATCHES:
            for chunk in CHUNKS:
                assert arms[name][f"n{n}_c{chunk}"].tobytes() == full[:n].tobytes(), (name, n, chunk)
    new, old = arms["default"][top], arms["c1_f32"][top]
    assert new.tobytes() != old.tobytes()                            # the knob reaches the kernel
    e = relmax(new, old)
    print(f"default vs BE_C1_F32=1 logits: relmax {e:.2e}")
    assert e <= 1e-5
    for k in arms["wino_f32"]:                                       # BE_WINO_F32=1 already means fp32 everywhere
        assert arms["wino_f32"][k].tobytes() == arms["wino_f32_c1_f32"][k].tobytes(), k
