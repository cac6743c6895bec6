"""The Winograd blocks of LocalStage chained through one workspace (be_wino.hip, round 13): a block's last launch
(k_wino_out_res_in) writes y AND the next block's input transform, the max-pool in front of layer1 (k_pool_wino_in) writes the
pooled map AND layer1's input transform, and a block told `x_in_v` starts from that transform without reading x again.

The change moves no bit, so every comparison is on the raw bits (torch.equal of the int32 views: NaNs compare too): chained blocks
against the same blocks through wino_conv3x3_pair, the pool kernel against maxpool_nhwc and a following block, a refused chain, and
LocalStage's logits with the chain against BE_WINO_NO_CHAIN=1 (child processes: the knobs are read once per process)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu

# (cin, cmid = cout of block one, cmid = cout of block two).  At n = 1024 a layer with 128 outputs is tile-major, others are
# plane-major: (32, 128, 96) has tile-major M and plane-major V', (64, 128, 128) both tile-major; small n: both plane-major
SHAPES = [(32, 64, 64), (32, 128, 96), (64, 128, 128)]
BATCHES = [1, 3, 65, 1024]


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


def biteq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _conv(g, cout, cin, native, zero_out=0):
    w = torch.randn(cout, cin, 3, 3, generator=g) * float(np.sqrt(2.0 / (9 * cin)))
    b = 0.1 * torch.randn(cout, generator=g)
    if zero_out:                                             # output channels whose convolution result is an exact zero
        w[:zero_out] = 0.0
        b[:zero_out] = 0.0
    return native.wino_pack(w.to(DEV), b.to(DEV))


_PACKS = {}


def packs(native, shape):
    """The four packed convolutions of a two-block chain, once per shape (block one's conv2 has four all-zero output channels)."""
    if shape not in _PACKS:
        cin, c1, c2 = shape
        g = torch.Generator().manual_seed(1300 + cin + 7 * c1 + 13 * c2)
        _PACKS[shape] = (_conv(g, c1, cin, native), _conv(g, c1, c1, native, zero_out=4), _conv(g, c2, c1, native), _conv(g, c2, c2, native))
    return _PACKS[shape]


def two_blocks(native, shape, x, res, act1, act2, chained):
    """-> (y of block one, output of block two).  chained: block one leaves block two's input transform in the shared workspace and
    block two is handed zeros for x, so its result can only come from that transform."""
    cin, c1, c2 = shape
    (u1, b1), (u2, b2), (u3, b3), (u4, b4) = packs(native, shape)
    n = x.shape[0]
    if not chained:
        y1, _ = native.wino_conv3x3_pair(x, u1, b1, c1, u2, b2, c1, act1=act1, act2=act2, residual=res)
        y2, _ = native.wino_conv3x3_pair(y1, u3, b3, c2, u4, b4, c2, act1=1, act2=1)
        return y1, y2
    lib = native.lib()
    need = max(lib.be_wino_pair_workspace_floats(n, cin, c1, c1), lib.be_wino_pair_workspace_floats(n, c1, c2, c2))
    ws = torch.full((need,), float("nan"), dtype=torch.float32, device=DEV)
    y1 = native.wino_conv3x3_pair_chain(x, u1, b1, c1, u2, b2, c1, ws, act1=act1, act2=act2, residual=res, next_cmid=c2)
    y2 = native.wino_conv3x3_pair_chain(torch.zeros_like(y1), u3, b3, c2, u4, b4, c2, ws, act1=1, act2=1, x_in_v=True)
    return y1, y2


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_chained_blocks_equal_the_unchained_pair(native, shape, n):
    cin, c1, c2 = shape
    g = torch.Generator().manual_seed(17 * n + c1)
    x = torch.randn(n, 6, 6, cin, generator=g).to(DEV)
    r = torch.randn(n, 6, 6, c1, generator=g).to(DEV)
    for res in (None, r):
        for act in (0, 1, 2):
            y1, y2 = two_blocks(native, shape, x, res, 1, act, chained=True)
            ry1, ry2 = two_blocks(native, shape, x, res, 1, act, chained=False)
            assert bool(torch.isfinite(ry2).all())
            assert biteq(y1, ry1), (shape, n, res is not None, act, "y of block one")
            assert biteq(y2, ry2), (shape, n, res is not None, act, "output of block two")


@pytest.mark.parametrize("n", [3, 1024])
@pytest.mark.parametrize("act", [0, 1])
def test_chained_blocks_carry_signed_zeros_infinities_and_nans(native, n, act):
    """Block one's conv2 has four zero output channels (weights and bias), so there y = act(0 + res): the residual puts the special
    values in.  Without activation y = res: +-inf, NaN, +0.  Smish: a very negative value gives -0 (x * 0), +inf stays, -inf and
    NaN give NaN, +0 stays.  Image 0 carries them; the other images stay finite."""
    shape = (32, 128, 96)
    g = torch.Generator().manual_seed(91 + n)
    x = torch.randn(n, 6, 6, 32, generator=g).to(DEV)
    r = torch.randn(n, 6, 6, 128, generator=g)
    r[0, :, :, :4] = 0.0
    r[0, 0, 0, 0], r[0, 0, 1, 1], r[0, 2, 3, 2], r[0, 5, 5, 3] = float("inf"), float("-inf"), float("nan"), -1000.0
    r[0, 3, 3, 0], r[0, 4, 1, 1] = -0.0, -1.0e30
    r[0, 1, 4, 77], r[0, 4, 4, 100] = float("inf"), float("nan")          # and in channels with ordinary weights
    r = r.to(DEV)
    y1, y2 = two_blocks(native, shape, x, r, 1, act, chained=True)
    ry1, ry2 = two_blocks(native, shape, x, r, 1, act, chained=False)
    bits = ry1[0, :, :, :4].contiguous().view(torch.int32)
    has = lambda v: bool((bits == int(np.float32(v).view(np.int32))).any())
    assert has(0.0) and has(np.inf) and bool(torch.isnan(ry1[0]).any())
    assert has(-np.inf) if act == 0 else has(-0.0)
    assert bool(torch.isfinite(ry1[1:]).all()) and bool(torch.isfinite(ry2[1:]).all())
    assert biteq(y1, ry1) and biteq(y2, ry2)


def test_a_chain_that_would_reach_m_is_refused_before_any_launch(native):
    lib = native.lib()
    n, cin, cmid, cout = 5, 32, 32, 128                     # V' = 80 n 128 floats, M starts at 100 n 32
    g = torch.Generator().manual_seed(5)
    (u1, b1), (u2, b2) = _conv(g, cmid, cin, native), _conv(g, cout, cmid, native)
    x = torch.randn(n, 6, 6, cin, generator=g).to(DEV)
    y = torch.full((n, 6, 6, cout), 7.0, device=DEV)
    ws = torch.full((lib.be_wino_pair_workspace_floats(n, cin, cmid, cout),), 7.0, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())

    def call(x_in_v, next_cmid):
        return lib.be_wino_conv3x3_pair_chain_6x6_f32(P(x), P(u1), P(b1), 1, P(u2), P(b2), None, 1, P(y), n, cin, cmid, cout, P(ws),
                                                      ws.numel(), native.stream_ptr(x.device), x_in_v, next_cmid)

    assert call(0, 64) != 0
    assert call(1, 64) != 0
    assert call(0, -1) != 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((ws == 7.0).all())           # nothing was launched
    assert call(0, 0) == 0                                               # unchained, the same call is taken
    torch.cuda.synchronize()
    ref, _ = native.wino_conv3x3_pair(x, u1, b1, cmid, u2, b2, cout)
    assert biteq(y, ref)


def _pool_input(n, c):
    """[n,11,11,c] with, in image 0: an all-NaN corner (output (0,0) sees only NaNs), a window of zeros of both signs, a window of
    -inf with one NaN, a window with +inf, -inf, NaN and ordinary values, and specials sprinkled over the rest; images 1.. finite."""
    g = torch.Generator().manual_seed(1000 * c + n)
    x = torch.randn(n, 11, 11, c, generator=g)
    pick = torch.rand(11, 11, c, generator=g)
    x0 = x[0]
    for lo, v in ((0.00, float("nan")), (0.06, float("inf")), (0.09, float("-inf")), (0.12, 0.0), (0.16, -0.0)):
        x0[(pick >= lo) & (pick < lo + 0.03)] = v
    x0[0:3, 0:3, :] = float("nan")                          # output (0,0): rows 0-1, columns 0-1
    x0[5:8, 5:8, :] = -0.0                                  # output (3,3): rows 5-7, columns 5-7
    x0[6, 6, ::2] = 0.0
    x0[5, 7, 1::4] = 0.0
    x0[9:11, 9:11, :] = float("-inf")                       # output (5,5): rows 9-10, columns 9-10
    x0[10, 9, :] = float("nan")
    x0[1:4, 7:10, :] = torch.randn(3, 3, c, generator=g)    # output (1,4): rows 1-3, columns 7-9
    x0[1, 7, :], x0[2, 8, :], x0[3, 9, :] = float("inf"), float("-inf"), float("nan")
    return x.to(DEV)


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("c", [32, 96])
def test_pool_kernel_equals_the_max_pool_and_feeds_the_next_block(native, c, n):
    cmid = 128                                              # tile-major at n = 1024
    g = torch.Generator().manual_seed(7 + c)
    (u1, b1), (u2, b2) = _conv(g, cmid, c, native), _conv(g, cmid, cmid, native)
    x = _pool_input(n, c)
    ref = native.maxpool_nhwc(x, 3, 2, 1)
    ws = torch.full((native.lib().be_wino_pair_workspace_floats(n, c, cmid, cmid),), float("nan"), dtype=torch.float32, device=DEV)
    pooled = native.maxpool_wino_in(x, cmid, ws)
    assert biteq(pooled, ref)
    assert bool(torch.isinf(ref[0, 0, 0]).all()) and bool((ref[0, 0, 0] < 0).all())          # the all-NaN window: the fold's -inf
    assert bool((ref[0, 3, 3] == 0).all()) and bool(torch.isinf(ref[0, 5, 5]).all()) and bool(torch.isinf(ref[0, 1, 4]).all())
    y = native.wino_conv3x3_pair_chain(torch.zeros_like(pooled), u1, b1, cmid, u2, b2, cmid, ws, x_in_v=True)
    ry, _ = native.wino_conv3x3_pair(ref, u1, b1, cmid, u2, b2, cmid)
    assert biteq(y, ry)
    if n > 1:
        assert bool(torch.isfinite(ry[1:]).all())


# ---------------------------------------------------------------------------------------------------- whole LocalStage
LS_BATCHES = (1, 65, 1100)                                  # 1100 crosses the tile-major threshold (1024 maps)
KNOBS = ("BE_WINO_NO_CHAIN", "BE_WINO_F32", "BE_ROWS_F32", "BE_L0_F32", "BE_C1_F32", "BE_NO_CONV_PM", "BE_NO_CONV1_POOL",
         "BE_WINO_NO_PERSIST", "BE_WINOGRAD")


def _logits():
    """LocalStage logits (Winograd path) of the first n patches of one seeded batch, twice each, and the profiler's launch counts of
    one 65-patch forward: [Winograd transform launches, k_maxpool_nhwc launches]."""
    import models
    from be_hip import native, synth
    m = models.LocalStage()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.local_stage_state_dict().items()})
    m = m.to(DEV).eval()
    assert m.winograd is True
    x = torch.from_numpy(np.asarray(synth.uniform_patches(max(LS_BATCHES), name="wino_chain"), dtype=np.float32)).to(DEV)
    out = {}
    with torch.no_grad():
        for n in LS_BATCHES:
            for run in (0, 1):
                out[f"n{n}_r{run}"] = m(x[:n].contiguous()).cpu().numpy().copy()
        native.profile_enable(256)
        native.profile_reset()
        m(x[:65].contiguous())
        torch.cuda.synchronize()
        ids = [r[0] for r in native.profile_read(256)]
    out["launches"] = np.array([ids.count(8), ids.count(9)])
    return out


_CHILD = r'''
import os, sys
import numpy as np
sys.path[:0] = [os.environ["BE_ROOT"], os.path.join(os.environ["BE_ROOT"], "blurry-edges_amd"), os.path.join(os.environ["BE_ROOT"], "tests")]
import test_wino_chain as t
np.savez(os.environ["BE_OUT"], **t._logits())
'''


@pytest.mark.parametrize("arm", ["bf16x6", "f32"])
def test_local_stage_logits_with_and_without_the_chain_are_the_same_bits(native, arm):
    """Per arithmetic arm (the default split-bf16, BE_WINO_F32=1) two fresh processes, one after the other: the chain, and
    BE_WINO_NO_CHAIN=1.  Each prints what it got before anything is asserted."""
    base = {"BE_WINO_F32": "1"} if arm == "f32" else {}
    got = {}
    with tempfile.TemporaryDirectory() as d:
        for name, knobs in (("chain", base), ("no_chain", dict(base, BE_WINO_NO_CHAIN="1"))):
            env = dict(os.environ, BE_ROOT=ROOT, BE_OUT=os.path.join(d, name + ".npz"))
            for k in KNOBS:
                env.pop(k, None)
            env.update(knobs)
            r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (name, r.stdout[-2000:] + r.stderr[-4000:])
            got[name] = dict(np.load(os.path.join(d, name + ".npz")))
    for name, a in got.items():
        print(arm, name, {k: (zlib.crc32(v.tobytes()) if k != "launches" else v.tolist()) for k, v in sorted(a.items())})
    for name, a in got.items():
        for n in LS_BATCHES:
            assert a[f"n{n}_r0"].shape == (n, 10) and np.isfinite(a[f"n{n}_r0"]).all()
            assert a[f"n{n}_r0"].tobytes() == a[f"n{n}_r1"].tobytes(), (arm, name, n, "run to run")
    for n in LS_BATCHES:
        assert got["chain"][f"n{n}_r0"].tobytes() == got["no_chain"][f"n{n}_r0"].tobytes(), (arm, n)
    # the chain is on in both arithmetic arms and off under the knob: per forward the pool kernel, three k_wino_out_in, two
    # k_wino_out_res_in and k_wino_out_pool2 (7 transform launches) against a k_wino_in, k_wino_out_in and k_wino_out(_pool2) per
    # block (9) and one more k_maxpool_nhwc - three launches fewer.  The arm is what it says: at 65 patches the split-bf16 head pools
    # inside its conv1 kernel, the fp32 head of a small batch with k_maxpool_nhwc
    assert got["chain"]["launches"].tolist() == [7, 1 if arm == "f32" else 0], got["chain"]["launches"]
    assert got["no_chain"]["launches"].tolist() == [9, 2 if arm == "f32" else 1], got["no_chain"]["launches"]
