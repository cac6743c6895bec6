"""tests/conv_fp64_oracle.py can fail: a plain float32 evaluation of the convolution (numpy, taps and 32-channel chunks accumulated
in that order) lies inside the derived bound everywhere, and each of eight subtly wrong evaluations leaves it in at least one
element.  A mutant that stays inside would mean the oracle is too loose - the cure is then the oracle's constant or inputs, never
this list.  Also here, because it is a check on shapes alone: native.conv_nhwc refuses a residual whose row stride is not y's."""
import numpy as np
import pytest
import torch

import conv_fp64_oracle as oracle

F = np.float32


def _case(ks):
    """the 3x3 case (n 4, 5x6, cin 32, cout 40, BN and a residual of row stride cout + 4) and the 1x1 case (cin 64, cout 96)"""
    rng = np.random.default_rng(77 + ks)
    f = lambda *s: rng.standard_normal(s).astype(F)
    n, h, w = 4, 5, 6
    cin, cout = (32, 40) if ks == 3 else (64, 96)
    c = dict(ks=ks, x=f(n, h, w, cin), weight=f(cout, cin, ks, ks) * F(np.sqrt(2.0 / (cin * ks * ks))), bias=f(cout) * F(0.1),
             bn=None, eps=1e-5, res=None, res_buf=None)
    if ks == 3:
        gamma = (rng.uniform(0.5, 2.0, cout) * rng.choice([-1.0, 1.0], cout)).astype(F)
        c["bn"] = (gamma, f(cout) * F(0.1), f(cout) * F(0.1), rng.uniform(1e-3, 4.0, cout).astype(F))
        c["eps"] = 1e-3
        c["res_buf"] = f(n, h, w, cout + 4)                            # the residual lives in a tensor of row stride cout + 4
        c["res"] = c["res_buf"][..., :cout]
    return c


def _round_mantissa(a, bits):
    """float32 rounded to nearest even at `bits` explicit mantissa bits (7: bf16, 10: tf32-like)"""
    drop = 23 - bits
    u = np.ascontiguousarray(a, dtype=F).view(np.uint32).astype(np.uint64)
    u = (u + ((1 << (drop - 1)) - 1) + ((u >> drop) & 1)) >> drop << drop
    return u.astype(np.uint32).view(F)


def _conv_f32(c, mutant=None):
    """the pre-activation in float32: BN folded into the weights as the pack does, then for each tap, for each 32-channel chunk,
    acc += x_chunk . w_chunk; then the folded bias and the residual"""
    x, wt, ks = c["x"], c["weight"], c["ks"]
    n, h, w, cin = x.shape
    cout, r = wt.shape[0], ks // 2
    if c["bn"] is not None:
        gamma, beta, mean, var = c["bn"]
        scale = (gamma / np.sqrt(var + F(c["eps"]))).astype(F)
        wf, bf = (wt * scale[:, None, None, None]).astype(F), ((c["bias"] - mean) * scale + beta).astype(F)
    else:
        wf, bf = wt, c["bias"].copy()
    if mutant in ("bf16", "tf32"):
        bits = 7 if mutant == "bf16" else 10
        x, wf = _round_mantissa(x, bits), _round_mantissa(wf, bits)
    if mutant == "bias":
        bf[cout - 1] = 0
    flat = x.reshape(n, h * w, cin)
    acc = np.zeros((n, h, w, cout), F)
    for dy in range(ks):
        for dx in range(ks):
            src = np.zeros((n, h, w, cin), F)                            # the tap's input, zero outside the image
            for py in range(h):
                for px in range(w):
                    sy, sx = py + dy - r, px + dx - r
                    if 0 <= sy < h and 0 <= sx < w:
                        src[:, py, px] = x[:, sy, sx]
                    elif mutant == "wrap" and 0 <= sy < h and sx == -1 and sy * w + sx >= 0:
                        src[:, py, px] = flat[:, sy * w + sx]            # the left border reads the end of the previous row
            for cc in range(cin // 32):
                if mutant == "chunk" and cc == cin // 32 - 1:
                    continue
                part = (src[..., cc * 32:(cc + 1) * 32] @ wf[:, cc * 32:(cc + 1) * 32, dy, dx].T).astype(F)
                if mutant == "tap" and (dy, dx) == (r, ks - 1) and cc == 0:
                    part[n - 1, 0, 0] = 0                                # one tap (the right neighbour; 1x1: the only one), one corner pixel
                acc += part
    y = acc + bf
    if c["res"] is not None:
        if mutant == "res_stride":                                       # row stride cout on a tensor whose stride is cout + 4
            y = y + c["res_buf"].reshape(-1)[:n * h * w * cout].reshape(n, h, w, cout)
        else:
            y = y + c["res"]
    return y.astype(F)


def _smish_f32(v, mutant=False):
    """be::smish in float32 numpy: x * num / den in t = exp(-|x|); the mutant takes the x >= 0 coefficients everywhere"""
    v = np.asarray(v, F)
    t = np.exp(-np.abs(v)).astype(F)
    pos = (v >= 0) | mutant
    n2, n0, d2, d0 = (np.where(pos, F(a), F(b)) for a, b in ((0, 3), (3, 0), (2, 5), (5, 2)))
    num, den = t * (n2 * t + F(2)) + n0, t * (d2 * t + F(6)) + d0
    return (v * (num / den)).astype(F)


def _ref(c):
    ref, mag = oracle.conv_ref(c["x"], c["weight"], c["bias"], c["ks"], bn=c["bn"], eps=c["eps"], res=c["res"])
    return ref, mag, oracle.products(c["x"].shape[-1], c["ks"])


@pytest.mark.parametrize("ks", [3, 1])
def test_plain_float32_evaluation_lies_inside_the_bound(ks):
    c = _case(ks)
    ref, mag, K = _ref(c)
    y = _conv_f32(c)
    worst = oracle.worst(y, ref, mag, K)
    print(f"ks {ks}: K {K}  max |y - ref| / bound = {worst:.3f}")
    assert worst <= 1.0
    assert oracle.smish_worst(_smish_f32(y), y) <= 1.0
    sweep = np.concatenate([s * np.geomspace(2.0 ** -20, 100.0, 512) for s in (1, -1)] + [[0.0, -0.0]]).astype(F)
    assert oracle.smish_worst(_smish_f32(sweep), sweep) <= 1.0


MUTANTS = {3: ("tap", "chunk", "wrap", "bf16", "tf32", "bias", "res_stride"), 1: ("tap", "chunk", "bf16", "tf32", "bias")}


@pytest.mark.parametrize("ks,mutant", [(ks, m) for ks, ms in MUTANTS.items() for m in ms])
def test_each_wrong_evaluation_leaves_the_bound(ks, mutant):
    """(the 1x1 case has no left neighbour to wrap and no residual: those two mutants are the 3x3 case's)"""
    c = _case(ks)
    ref, mag, K = _ref(c)
    worst = oracle.worst(_conv_f32(c, mutant), ref, mag, K)
    print(f"ks {ks} mutant {mutant}: max |y - ref| / bound = {worst:.1f}: caught")
    assert worst > 1.0, f"the oracle is too loose: mutant {mutant} stays inside the bound"


@pytest.mark.parametrize("ks", [3, 1])
def test_smish_with_the_positive_coefficients_for_negative_x_leaves_the_bound(ks):
    v = _conv_f32(_case(ks))
    worst = oracle.smish_worst(_smish_f32(v, mutant=True), v)
    print(f"ks {ks} mutant smish: max |smish - smish64| / bound = {worst:.1f}: caught")
    assert (v < 0).any() and worst > 1.0


def _plan(c, ldy):
    """be_conv_plan_debug (host only) -> (route, tile, kernel id, pixmaj, K slices)"""
    import ctypes as C
    from be_hip import native
    n, h, w, cin, cout, ks = c["shape"]
    d, out, fe = native.ConvDesc(n, h, w, cin, cout, ks, 0), (C.c_int * 16)(), C.c_double()
    scratch = (c["scratch"] or 0) * n * h * w * ((cout + 31) // 32 * 32) * 4
    rc = native.lib().be_conv_plan_debug(C.byref(d), c["cin2"], int(c["res"]), ldy, c["nbatch"], scratch, 0, out, C.byref(fe))
    assert rc == 0, (c["key"], native.lib().be_last_error().decode())
    return out[0], out[1], out[3], out[4], out[10]


def test_every_case_of_the_gpu_file_is_planned_as_it_says():
    """the planner on the CPU: each case of tests/test_conv_fp64_gpu.py takes the kernel id it names and - the shapes the routes file
    does not have - the route, tile and pixmaj mode its comment says; and giving y a row stride of cout + 4 changes no plan (so
    no case has to stay at ldy = cout for its route's sake; those that do are there for their unaligned stores)"""
    from test_conv_fp64_gpu import CASES, PAD
    for c in CASES:
        cout = c["shape"][4]
        route, tile, kernel, pixmaj, S = _plan(c, cout + c["pad"])
        assert [kernel] == c["kernels"], (c["key"], kernel)
        if c["plan"] is not None:
            assert (route, tile, pixmaj) == c["plan"], (c["key"], route, tile, pixmaj)
        if c["pad"] == PAD:
            assert _plan(c, cout) == (route, tile, kernel, pixmaj, S), c["key"]
        if c["scratch"]:
            assert S > 1, c["key"]
        print(f"{c['key']}: route {route} tile {tile} kernel {kernel} pixmaj {pixmaj} S {S}")
    by = {c["key"]: c for c in CASES}
    assert _plan(by["splitk_cin256"], 388)[4] == 4 and _plan(by["splitk_27_chunks"], 260)[4] == 4      # 27 chunks over 4 slices
    # the one route that does look at ldy: 640 images of 9x9 onto 90 channels would take the LDS-DMA kernel at a stride of 92
    assert _plan(by["c90_pm_igemm"], 92)[0] == 1 and _plan(by["c90_pm_igemm"], 90)[0] == 2


def test_conv_nhwc_refuses_a_residual_that_has_not_ys_row_stride():
    """every route reads residual[m * ldy + c]: a contiguous [N,H,W,cout] residual beside a wider out would be read at the wrong
    stride and past its end.  The refusal is a shape check that comes before any pointer is taken (CPU tensors reach it)."""
    from be_hip import native
    n, h, w, cin, cout = 2, 3, 3, 32, 40
    x, pw, pb = torch.zeros(n, h, w, cin), torch.zeros(1), torch.zeros(64)
    wide, tight = torch.zeros(n, h, w, cout + 4), torch.zeros(n, h, w, cout)
    bad = [(tight, wide),                                              # the case of the issue: row stride cout beside ldy = cout + 4
           (wide, None),                                               # row stride cout + 4 beside a fresh y of row stride cout
           (wide[..., :cout], None),
           (torch.zeros(n, h, w, cout - 8), None),                     # another channel count
           (tight[:1], None),                                          # too few rows
           (torch.zeros(n, h, w, 2 * cout)[..., ::2], None),           # channels not adjacent
           (torch.zeros(n, h, 2 * w, cout + 4)[:, :, ::2, :cout], wide)]   # rows not ldy apart
    for res, out in bad:
        with pytest.raises(RuntimeError, match="read with y's row stride"):
            native.conv_nhwc(x, pw, pb, cout, 3, 0, residual=res, out=out)
    # what the kernels do read correctly passes the check and stops at the next one: these are not GPU tensors
    for res, out in ((tight, None), (wide, wide.clone()), (wide[..., :cout], wide.clone()), (tight.view(n * h * w, cout), None)):
        with pytest.raises(RuntimeError, match="expected a tensor on the GPU"):
            native.conv_nhwc(x, pw, pb, cout, 3, 0, residual=res, out=out)
    with pytest.raises(RuntimeError, match="read with y's row stride"):
        native.linear(torch.zeros(18, 32), pw, pb, cout, residual=torch.zeros(18, cout + 4)[:, :cout])
