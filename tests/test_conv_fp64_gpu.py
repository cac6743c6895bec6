"""The fp32 convolution against float64 on every planned route (tests/conv_fp64_oracle.py: ref, mag and the derived per-element
bound |y - ref| <= (K + 16) 2^-24 mag).  tests/test_conv_routes_gpu.py pins each route's bits to a recording; this file holds the
same cases, and the shapes that file does not have, to what the convolution IS:

  a. every element inside the bound, the kernel ids the case names, and - y given a row stride of cout + 4, pre-filled with the
     bit pattern 0x7fc0beef - the four padding columns untouched (residuals are [.., :cout] views of a tensor of the same stride)
  b. rms(y - ref) <= 8 x rms(y32 - ref), y32 = conv2d in float32 on the CPU: catches a precision downgrade (a split that keeps two
     or three bf16 pieces is >= 64 x worse) that the worst-case bound is too coarse for.  8 = three bits: the MFMA chains add K
     sequentially where the CPU adds in blocks, which can account for a factor 2 at K up to 2304
  c. cout that is no multiple of 32 (ldy = cout: unaligned stores, a partly empty last N tile), images smaller than the kernel,
     ragged pixel-major and flat tiles, BatchNorm folded in the pack (eps 1e-5 and 1e-3 at variances down to 1e-3; fc.1's
     (C,H,W) flatten), split K against float64
  d. ReLU = max(y_act0, 0) bit for bit; Smish inside its own bound against smish64 of the GPU's act = 0 output; the whole domain
     of be::smish through the real epilogue
  e. +inf, -inf and NaN stay inside their receptive fields: non-finite exactly there, every other element bit-identical
  f. each batch of the batched launch against its own reference, and bit-identical to the single launch

Every case runs at act = 0 unless the test is about the activation.  The shapes of (c) were planned on the CPU first
(be_conv_plan_debug; tests/test_conv_fp64_cpu.py holds every case of this file to its kernel id, route, tile and pixmaj mode
there, and shows that ldy = cout + 4 changes no case's plan)."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_fp64_oracle as oracle
from test_conv_routes_gpu import CASES as ROUTE_CASES, IDS as ROUTE_IDS, _operands as route_operands
from test_conv_routes_gpu import K128, K96, K64, K32, KROW8, KSMALL, KROWS

DEV = "cuda:0"
PAD = 4
FILL = 0x7fc0beef                                   # a quiet NaN with a payload: any write into the padding columns shows
ROWS, PM, IGEMM = 0, 1, 2                           # be_conv_plan_debug's routes
S64, S128x32, S64_UNI, T128, T96, T64, T32, TROW8 = range(8)       # ... and tiles


def _case(key, shape, kernels, plan, res=False, cin2=0, nbatch=1, scratch=None, bn=False, eps=1e-5, chw_hw=0, pad=PAD):
    """shape = (n, h, w, cin, cout, ks); kernels = the kernel ids of its launches; plan = (route, tile, pixmaj) as planned on the
    CPU; pad: ldy - cout"""
    return dict(key=key, shape=shape, kernels=kernels, plan=plan, res=res, cin2=cin2, nbatch=nbatch, scratch=scratch, bn=bn, eps=eps,
                chw_hw=chw_hw, pad=pad)


# every case of the routes file at ldy = cout + 4: none of their routes depends on ldy in a way that changes (the pixel-major
# LDS-DMA kernel needs ldy % 4 == 0, which cout + 4 = 100 satisfies) - tests/test_conv_fp64_cpu.py shows it on the planner
CASES = [dict(c, plan=None, bn=False, eps=1e-5, chw_hw=0, pad=PAD) for c in ROUTE_CASES]
N_ROUTE = len(CASES)
CASES += [
    # cout no multiple of 32, ldy = cout
    _case("c14_small_128x32", (8, 6, 6, 32, 14, 3), [KSMALL], (IGEMM, S128x32, 0), pad=0),
    _case("c100_1x1_small", (8, 6, 6, 32, 100, 1), [KSMALL], (IGEMM, S64, 0), pad=0),
    _case("c40_large_128x64", (48, 32, 32, 32, 40, 3), [K64], (IGEMM, T64, 0), pad=0),
    # 25088 rows in 196 tiles of 128 and one 128-wide column of tiles: "few tiles" for the planner, which gives 512 = 8 x 64 images
    # the uniform pixel-major 64 x 64 tiles (not the 128-row pixel-major implicit GEMM)
    _case("c100_n512_pm2", (512, 7, 7, 32, 100, 3), [KSMALL], (IGEMM, S64_UNI, 2), pad=0),
    # ldy = 90, no multiple of 4, keeps 640 images of 9x9 off the LDS-DMA kernel: the pixel-major implicit GEMM, unaligned stores
    _case("c90_pm_igemm", (640, 9, 9, 32, 90, 3), [K96], (IGEMM, T96, 1), pad=0),
    # images smaller than the kernel: at n = 64 the uniform pixel-major small tiles, most taps in the padding.  (1x1 at n = 64 is the
    # case that found the pixel-major tile order counting (H - 2)(W - 2) = 1 interior pixel on a 1 x 1 image: the tile computed the
    # pixel (1, 1), read the rows two images back and wrote two rows down - the first two rows never, two rows past the end of y)
    *[_case(f"tiny_{h}x{w}_n{n}", (n, h, w, 32, 64, 3), [KSMALL], (IGEMM, S64_UNI if n == 64 else S64, 2 if n == 64 else 0))
      for h, w in ((1, 1), (1, 5), (5, 1), (2, 2)) for n in (8, 64)],
    # ragged tiles.  577 images of 9x9 onto 96 channels are 366 row tiles, "few": flat 128 x 32 tiles, the last one 17 rows;
    _case("ragged_577_flat", (577, 9, 9, 32, 96, 3), [KSMALL], (IGEMM, S128x32, 0), res=True),
    # onto 192 channels (two columns of tiles) they are the 128-image pixel-major tiles, the last one holding 65 images
    _case("ragged_577_pm128", (577, 7, 7, 32, 192, 3), [K96], (IGEMM, T96, 1), res=True),
    _case("ragged_700_lds_dma", (700, 9, 9, 32, 96, 3), [K96], (PM, T96, 1)),            # 256-image tiles, the last one 188 images
    _case("ragged_130_flat", (130, 6, 6, 32, 64, 3), [KSMALL], (IGEMM, S64, 0)),         # M = 4680 = 73 x 64 + 8
    # BatchNorm folded in the pack, one per route; var in [1e-3, 4], gamma in +-[0.5, 2]
    _case("bn_small", (8, 6, 6, 32, 64, 3), [KSMALL], (IGEMM, S64, 0), bn=True, eps=1e-3),
    _case("bn_large", (48, 32, 32, 32, 64, 3), [K64], (IGEMM, T64, 0), bn=True, eps=1e-5),
    _case("bn_lds_dma", (640, 9, 9, 32, 96, 3), [K96], (PM, T96, 1), bn=True, eps=1e-3),
    _case("bn_rows", (16384, 1, 1, 32, 128, 1), [KROWS], (ROWS, T128, 0), bn=True, eps=1e-5),
    _case("bn_row8", (2, 21, 21, 4, 64, 7), [KROW8], (IGEMM, TROW8, 0), bn=True, eps=1e-3),
    _case("fc1_chw_flatten", (8, 1, 1, 288, 64, 1), [KSMALL], (IGEMM, S64, 0), chw_hw=9),
    # split K against float64 (scratch for 8 slices, a residual); 27 chunks of 32 channels x taps: no slice count divides them
    _case("splitk_cin256", (64, 6, 6, 256, 384, 3), [KSMALL], (IGEMM, S64_UNI, 2), res=True, scratch=8),
    _case("splitk_27_chunks", (64, 6, 6, 96, 256, 3), [KSMALL], (IGEMM, S64_UNI, 2), res=True, scratch=8),
]
IDS = [c["key"] for c in CASES]
BY_KEY = dict(zip(IDS, CASES))

# one case per route for the activation and the non-finite tests
ACT_KEYS = ["small_flat_64x64", "small_pm2_uniform", "tiles_384_128x64", "pm_lds_dma", "pm_lds_dma_x2", "rows_first_rule", "row8_flat",
            "ragged_577_pm128", "splitk_12_chunk_rule"]
NONFINITE_KEYS = ["small_flat_64x64", "small_pm2_uniform", "tiny_2x2_n64", "tiles_384_128x64", "ragged_577_pm128", "ragged_700_lds_dma",
                  "rows_first_rule", "row8_flat", "row8_pixel_major"]
KEEP = set(ACT_KEYS) | set(NONFINITE_KEYS) | {"batched_small", "batched_large"}


def operands(c):
    """-> dict of float32 numpy: x [nbatch,n,h,w,cin], wt [nbatch,cout,cin_w,ks,ks], bias, x2, w2, res (None where absent), bn =
    (gamma, beta, mean, var) | None.  The routes file's cases are its own draws; the others follow the same scheme from their own
    seeds.  Weights with an exact zero (they would hide a non-finite input) are drawn again, never masked"""
    redraw = 0
    while True:
        ops = _draw(c, redraw)
        if ops["wt"].all() and (ops["w2"] is None or ops["w2"].all()):
            return ops
        redraw += 1


def _draw(c, redraw):
    idx = IDS.index(c["key"])
    if idx < N_ROUTE and not redraw:
        x, wt, bias, x2, w2, res = route_operands(ROUTE_CASES[idx])
    else:
        n, h, w, cin, cout, ks = c["shape"]
        rng = np.random.default_rng(1900 + idx + 1000 * redraw)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        nb, cin_w = c["nbatch"], (3 if ks == 7 else cin)
        x = f(nb, n, h, w, cin)
        if ks == 7:
            x[..., 3] = 0.0                              # the NHWC4 staging: the fourth channel is padding
        wt = f(nb, cout, cin_w, ks, ks) * np.float32(np.sqrt(2.0 / (cin_w * ks * ks)))
        bias = f(cout) * np.float32(0.1)
        x2 = f(n, h, w, c["cin2"]) if c["cin2"] else None
        w2 = f(cout, c["cin2"], 1, 1) * np.float32(np.sqrt(2.0 / c["cin2"])) if c["cin2"] else None
        res = f(n, h, w, cout) if c["res"] else None
    bn = None
    if c["bn"]:
        cout = c["shape"][4]
        rng = np.random.default_rng(7900 + idx)
        gamma = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(np.float32)
        bn = (gamma, (rng.standard_normal(cout) * 0.1).astype(np.float32), (rng.standard_normal(cout) * 0.1).astype(np.float32),
              rng.uniform(1e-3, 4.0, cout).astype(np.float32))
    return dict(x=x, wt=wt, bias=bias, x2=x2, w2=w2, res=res, bn=bn)


def run(native, c, ops, act=0, x=None):
    """the case through the entry point it belongs to, y's row stride cout + pad and pre-filled
    -> y [nbatch,n,h,w,cout + pad] (float32 numpy, the padding columns included), the kernel ids of the launches"""
    n, h, w, cin, cout, ks = c["shape"]
    nb, ld = c["nbatch"], cout + c["pad"]
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    xd, bd, x2d = t(ops["x"] if x is None else x), t(ops["bias"]), t(ops["x2"])
    bn = None if ops["bn"] is None else tuple(t(v) for v in ops["bn"])
    if c["cin2"]:
        pw, pb = native.conv_pack_fused2(t(ops["wt"][0]), bd, None, t(ops["w2"]), None, None)
    else:
        packs = [native.conv_pack(t(ops["wt"][b]), bd, bn=bn, eps=c["eps"], chw_hw=c["chw_hw"]) for b in range(nb)]
        pw, pb = torch.stack([p[0] for p in packs]), packs[0][1]
    y = torch.full((nb, n, h, w, ld), FILL, dtype=torch.int32, device=DEV).view(torch.float32)
    resd = None
    if ops["res"] is not None:                           # the residual has y's row stride: a view of a [n,h,w,ld] tensor
        buf = torch.full((n, h, w, ld), 1.0e30, dtype=torch.float32, device=DEV)
        buf[..., :cout] = t(ops["res"])
        resd = buf[..., :cout]
    scratch = None
    if c["scratch"]:
        scratch = torch.empty(c["scratch"] * n * h * w * ((cout + 31) // 32 * 32), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    native.profile_enable(8)
    native.profile_reset()
    if c["cin2"]:
        native.conv_nhwc_fused2(xd[0], x2d, pw, pb, cout, ks, act, out=y[0])
    elif nb > 1:
        d = native.ConvDesc(n, h, w, cin, cout, ks, act)
        native.check(native.lib().be_conv_nhwc_batched_f32(C.byref(d), native.dptr(xd), native.dptr(pw), native.dptr(pb), native.dptr(y), ld,
                                                           nb, xd[0].numel(), pw[0].numel(), y[0].numel(),
                                                           native.stream_ptr(xd.device)), "be_conv_nhwc_batched_f32")
    else:
        native.conv_nhwc(xd[0], pw[0], pb, cout, ks, act, residual=resd, out=y[0], scratch=scratch)
    torch.cuda.synchronize()
    recs = native.profile_read(8)
    native.profile_enable(0)
    return y.cpu().numpy(), [r[0] for r in recs]


def padding_untouched(c, y):
    return bool((y[..., c["shape"][4]:].view(np.uint32) == FILL).all())


def reference(c, ops, b=0):
    """-> ref, mag, y32 of batch b"""
    n, h, w, cin, cout, ks = c["shape"]
    x = ops["x"][b]
    if c["chw_hw"]:                                      # the reference flattens (C,H,W); the activations here are (H,W,C)
        hw = c["chw_hw"]
        x = x.reshape(n, hw, cin // hw).transpose(0, 2, 1).reshape(n, 1, 1, cin)
    kw = dict(bn=ops["bn"], eps=c["eps"], x2=ops["x2"], w2=ops["w2"], res=ops["res"])
    ref, mag = oracle.conv_ref(x, ops["wt"][b], ops["bias"], ks, **kw)
    return ref, mag, oracle.conv_f32(x, ops["wt"][b], ops["bias"], ks, **kw)


_DONE = {}


def evaluate(native, c):
    """the case at act = 0, once per session: kernel ids, padding, max |y - ref| / bound and the rms ratio against the CPU's
    float32 evaluation (over all batches); y itself is kept only for the cases other tests come back to"""
    if c["key"] not in _DONE:
        n, h, w, cin, cout, ks = c["shape"]
        ops = operands(c)
        y, ids = run(native, c, ops)
        K = oracle.products(cin, ks, c["cin2"])
        worst, e_gpu, e_cpu, count = [], 0.0, 0.0, 0
        for b in range(c["nbatch"]):
            ref, mag, y32 = reference(c, ops, b)
            worst.append(oracle.worst(y[b, ..., :cout], ref, mag, K))
            e_gpu += float(np.sum((y[b, ..., :cout].astype(np.float64) - ref) ** 2))
            e_cpu += float(np.sum((y32.astype(np.float64) - ref) ** 2))
        r = dict(ids=ids, padding=padding_untouched(c, y), worst=worst, ratio=float(np.sqrt(e_gpu / e_cpu)), K=K,
                 y=y if c["key"] in KEEP else None)
        print(f"\n{c['key']}: K {K}  max |y - ref| / bound = {max(worst):.4f}  rms(y - ref) / rms(y32 - ref) = {r['ratio']:.3f}")
        _DONE[c["key"]] = r
    return _DONE[c["key"]]


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native as n
    n.lib()
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_element_is_inside_the_float64_bound(native, c):
    """a. (and c., f.: the same assertions on their shapes; every batch of a batched launch against its own reference)"""
    r = evaluate(native, c)
    assert r["ids"] == c["kernels"]                      # the wider ldy must not move the case off its route
    assert max(r["worst"]) <= 1.0, r["worst"]
    assert r["padding"]                                  # nothing is written outside the cout columns


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_rms_error_is_that_of_float32_arithmetic(native, c):
    """b. against conv2d in float32 on the CPU - the reference, never the library"""
    r = evaluate(native, c)
    assert r["ratio"] <= 8.0


@pytest.mark.gpu
@pytest.mark.parametrize("key", ACT_KEYS)
def test_activations_apart_from_the_accumulation(native, key):
    """d. ReLU is max(y_act0, 0) bit for bit; Smish meets its bound against smish64 of the GPU's own pre-activation"""
    c = BY_KEY[key]
    cout, ops, y0 = c["shape"][4], operands(c), evaluate(native, c)["y"][..., :c["shape"][4]]
    relu, ids = run(native, c, ops, act=2)
    assert ids == c["kernels"] and padding_untouched(c, relu)
    assert np.array_equal(relu[..., :cout].view(np.uint32), np.maximum(y0, np.float32(0)).view(np.uint32))
    smish, ids = run(native, c, ops, act=1)
    assert ids == c["kernels"] and padding_untouched(c, smish)
    worst = oracle.smish_worst(smish[..., :cout], y0)
    print(f"\n{key}: max |smish - smish64| / bound = {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.gpu
def test_smish_over_its_whole_domain_through_the_epilogue(native):
    """d. 2048 values covering +-[2^-20, 100] with 0 and -0 through a 1x1 convolution with identity weights"""
    c = _case("smish_sweep", (64, 1, 1, 32, 32, 1), [KSMALL], None)
    v = np.geomspace(2.0 ** -20, 100.0, 1023)
    x = np.concatenate([v, -v, [0.0, -0.0]]).astype(np.float32).reshape(1, 64, 1, 1, 32)
    ops = dict(x=x, wt=np.eye(32, dtype=np.float32).reshape(1, 32, 32, 1, 1), bias=np.zeros(32, np.float32), x2=None, w2=None, res=None, bn=None)
    y0, ids = run(native, c, ops)
    assert ids == c["kernels"] and padding_untouched(c, y0)
    assert np.array_equal(y0[..., :32], x)                                       # x * 1 + zeros: the pre-activation is x itself
    y1, _ = run(native, c, ops, act=1)
    worst = oracle.smish_worst(y1[..., :32], x)
    print(f"\nsmish sweep: max |smish - smish64| / bound = {worst:.4f}")
    assert worst <= 1.0 and padding_untouched(c, y1)
    y2, _ = run(native, c, ops, act=2)
    assert np.array_equal(y2[..., :32], np.maximum(x, np.float32(0)))


@pytest.mark.gpu
@pytest.mark.parametrize("key", NONFINITE_KEYS)
def test_non_finite_values_stay_in_their_receptive_field(native, key):
    """e. +inf, -inf and NaN at three (image, pixel, channel) positions - the last image's last corner, the first image's first
    corner, the middle - make exactly the outputs within ks // 2 of them non-finite, over all cout; every other element keeps
    the bits of the clean run.  (The 7x7 row mode stages eight pixels per kernel row for seven taps; before the eighth was zeroed
    at the load its zero weights turned a non-finite pixel into NaN four columns to its left: the two row8 cases found that.)"""
    c = BY_KEY[key]
    n, h, w, cin, cout, ks = c["shape"]
    ops = operands(c)                                                            # (no weight is an exact zero: see there)
    clean = evaluate(native, c)["y"]
    x, r = ops["x"].copy(), ks // 2
    want = np.zeros((n, h, w), bool)
    for (img, py, px, ch), v in zip(((n - 1, h - 1, w - 1, 0), (0, 0, 0, 1), (n // 2, h // 2, w // 2, 2)), (np.inf, np.nan, -np.inf)):
        x[0, img, py, px, ch] = v
        want[img, max(0, py - r):py + r + 1, max(0, px - r):px + r + 1] = True
    y, ids = run(native, c, ops, x=x)
    assert ids == c["kernels"] and padding_untouched(c, y)
    bad = ~np.isfinite(y[0, ..., :cout])
    leaked = np.argwhere(bad.any(-1) & ~want)
    assert leaked.size == 0, f"non-finite outputs outside the receptive fields at (image, y, x) {leaked[:8].tolist()}"
    assert bad[want].all()                                                       # inside: every channel
    assert np.array_equal(y[0][~want].view(np.uint32), clean[0][~want].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["batched_small", "batched_large"])
def test_each_batch_of_the_batched_launch_is_the_single_launch(native, key):
    """f. (each batch against its own float64 reference: test_every_element_is_inside_the_float64_bound, over all batches)"""
    c = BY_KEY[key]
    r, ops = evaluate(native, c), operands(c)
    assert len(r["worst"]) == c["nbatch"] == 3 and max(r["worst"]) <= 1.0
    for b in range(c["nbatch"]):
        one = dict(ops, x=ops["x"][b:b + 1], wt=ops["wt"][b:b + 1])
        y, ids = run(native, dict(c, nbatch=1), one)
        assert ids == c["kernels"]
        assert np.array_equal(y[0].view(np.uint32), r["y"][b].view(np.uint32)), b
