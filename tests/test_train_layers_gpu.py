"""The training kernels layer by layer against float64 autograd (tests/train_layers_oracle.py), element by element, at the smallest
shape that reaches each launch path.

Every stage is checked at equal inputs: its float64 reference is computed from the float32 tensors the HIP stage read (the HIP y, mean,
invstd, ds, dy, ...), never from the previous reference stage.  Contractions (class A) are held to the derived fp32 summation bound
(K + 2) 2^-24 S + 2^-24 |ref| per element, elementwise / statistics outputs (class B) to four times the error of torch's float32
evaluation per tensor and channel.  Every output is allocated with 64 guard elements behind it, output and guard filled with a NaN
sentinel: none may survive inside the output, the guard stays untouched.  The units run twice - through train._unit_fwd / _unit_bwd
(the binding native.ops() selects) with dW / db / dgamma / dbeta as adjacent views of ONE flat buffer, as backward_train lays them out,
and through the C entry points with every output guarded on its own (the only way to see dy); the second run is compared with
float64, the first with the second bit for bit.

Worst observed error / bound on an MI355X (printed by the tests as `ratio <quantity> <path> <worst>` lines; A = class A, B = class B):
  the units (UNIT_CASES / PAIR_CASES)   A: y     dgamma dbeta  dW     db     dx    | B: mean  invstd run_m  run_v  s_in   out    ds     dy
  flat64_v1           (3,5,7,32,32,3)   0.019  0.002  0.001  0.024  0.000  0.018 |    0.205  0.220  0.219  0.244  0.346  0.397  0.551  0.250
  flat64_v0_splitk    (3,5,7,64,96,3)   0.007  0.004  0.002  0.030  0.000  0.003 |    0.231  0.234  0.201  0.245  0.365  0.544  0.566  0.449
  uniform_1x1         (16,2,2,64,64,1)  0.050  0.005  0.004  0.027  0.000  0.037 |    0.217  0.227  0.220  0.232    -    0.425  exact  0.250
  pm64                (32,3,3,32,96,3)  0.040  0.001  0.000  0.012  0.000  0.004 |    0.229  0.200  0.224  0.227    -    0.384  exact  0.250
  flat128_3x3 (/no_dx) (8,6,6,128,128,3) 0.002 0.001  0.001  0.010  0.000  0.002 |    0.217  0.221  0.242  0.236  0.489  0.541  0.565  0.250
  flat128_1x1         (8,6,6,128,128,1) 0.033  0.001  0.000  0.006  0.000  0.041 |    0.220  0.235  0.232  0.247  0.363  0.543  0.475  0.287
  pm128               (16,4,4,128,128,3) 0.003 0.001  0.001  0.014  0.000  0.002 |    0.237  0.210  0.226  0.235  0.322  0.509  0.578  0.250
  balanced_1grp       (64,3,3,64,96,3)  0.009  0.000  0.000  0.010  0.000  0.005 |    0.219  0.198  0.206  0.241  0.331  0.452  0.512  0.279
  balanced_2grp       (128,3,3,64,64,3) 0.008  0.000  0.000  0.003  0.000  0.010 |    0.235  0.200  0.225  0.232  0.353  0.431  0.500  0.282
  fc1_balanced        (64,1,1,576,64,1) 0.002  0.006  0.003  0.059  0.000  0.062 |    0.229  0.232  0.235  0.234  0.379  0.519  0.534  0.250
  fc1_ragged          (24,1,1,576,64,1) 0.002  0.026  0.011  0.149  0.000  0.058 |    0.216  0.232  0.242  0.242  0.306  0.618  0.558  0.621
  conv1_n2            (2,21,21,4,64,7)  0.052  0.000  0.000  0.001  0.000    -   |    0.207  0.236  0.206  0.233  0.395  0.362  0.487  0.348
  conv1_n3            (3,21,21,4,64,7)  0.070  0.000  0.000  0.001  0.000    -   |    0.204  0.228  0.197  0.232  0.358  0.441  0.456  0.335
  pair_ragged   3x3   (24,3,3,64,96)    0.006  0.002  0.001  0.018  0.000  0.006 |    0.214  0.196  0.223  0.240  0.367  0.533  0.474  0.335
  pair_ragged   1x1                     0.053  0.001  0.001  0.006  0.000  (sum) |    0.233  0.233  0.233  0.237    -    0.399  exact  0.496
  pair_balanced 3x3   (64,3,3,64,96)    0.011  0.000  0.000  0.007  0.000  0.004 |    0.236  0.198  0.239  0.242  0.433  0.584  0.486  0.250
  pair_balanced 1x1                     0.066  0.000  0.000  0.001  0.000  (sum) |    0.235  0.227  0.223  0.232    -    0.359  exact  0.250
  be_conv_wgrad_f32, dW (A): (3,5,7,8,12,3) 0.015  (2,6,6,68,100,1) 0.024  (5,1,1,32,32,3) 0.224  (4,2,2,32,32,3) 0.311  (5,1,1,72,32,1 chw 9) 0.293
                             (3,9,9,4,8,7) 0.004  (2,21,21,4,64,7) 0.001  (1,3,11,4,4,3: two slices, the last of one row) 0.068
  be_bn_train_fwd / bwd, be_col_sum, worst over res / act on and off and both consecutive calls:
    (M, C)       A: dgamma dbeta  col_sum | B: mean  invstd run_m  run_v  s_in   out    ds     dy
    (2, 4)          0.284  0.133  0.112   |    0.162  0.170  0.218  0.200  0.307  0.307  0.445  0.250
    (105, 100)      0.005  0.002  0.006   |    0.217  0.234  0.221  0.241  0.392  0.530  0.676  0.325
    (2304, 96)      0.000  0.000  0.000   |    0.224  0.240  0.241  0.244  0.339  0.477  0.520  0.299
  be_linear_small_fwd / bwd (A)   y      dx     dw     db        be_linear_param_grads_f32 (A)   dw     db
    (1, 4, 1)                     0.037  0.071  0.189  0.000       (256, 128, 128)                 0.015  0.000
    (3, 1024, 10)                 0.000  0.201  0.370  0.100       (300, 128, 256)                 0.014  0.000
    (64, 1024, 10)                0.000  0.249  0.055  0.012       (600, 256, 128: 304 + 296 rows) 0.004  0.000
    (5, 64, 256)                  0.014  0.006  0.312  0.202
Class A sits at a few per cent of its bound wherever K is large (the bound is the worst case of K roundings, the kernels' errors add
like a random walk, and the column sums are accumulated in double: their ratios round to 0.000); the largest ratios belong to the
shortest sums (K <= 5), where the bound is a few ulps.  The statistics are formed in double and rounded once - half an ulp against a
floor of two: 0.25 at most.  No class-B quantity needed more than 0.68 of its bound, the planted Smish extremes included (be::smish
is a rational form in exp(-|x|) and keeps full relative accuracy at -20 and -100, where torch's float32 log(1 + sigmoid(x)) returns 0).
Max-pool y, the decoded winner and both backward kernels' dx equal torch's bit for bit in every case, ties and all-negative included.
"""
import ctypes as C

import pytest
import torch

import train_layers_oracle as tl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FA5C3D2                                        # a NaN pattern no kernel arithmetic produces
GUARD = 64
ID_ROW8, ID_SMALL, ID_GEMMS = 4, 5, 12                       # native.KERNEL_NAMES: conv1's row-gather tiles, small-M tiles, k_unit_gemms(_sk)
FWD_IDS = {"row8": [ID_ROW8], "small": [ID_SMALL], "balanced": [ID_GEMMS]}
BWD_IDS = {"conv1": [], "wgrad_alone": [], "balanced": [ID_GEMMS], "merged_v0": [ID_GEMMS], "merged_v1": [ID_GEMMS], "merged_v2": [ID_GEMMS]}


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from be_hip import native, train
    native.lib()
    scratch = train._Scratch.get(torch.device(DEV))          # the 112 MB scratch: once per module
    return dict(native=native, train=train, lib=native.lib(), sc=scratch, sc_bytes=scratch.numel() * 4, stream=lambda: native.stream_ptr(torch.device(DEV)))


class Guarded:
    """an output of `shape` with GUARD elements behind it, all filled with the sentinel"""

    def __init__(self, *shape, dtype=torch.float32):
        self.n = 1
        for s in shape:
            self.n *= s
        self.byte = dtype == torch.uint8
        self.buf = (torch.full((self.n + GUARD,), 0xEE, dtype=torch.uint8, device=DEV) if self.byte
                    else torch.full((self.n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32))
        self.t = self.buf[:self.n].view(*shape)

    def check(self, name):
        raw = self.buf if self.byte else self.buf.view(torch.int32)
        mark = 0xEE if self.byte else SENTINEL
        left = int((raw[:self.n] == mark).sum())
        assert left == 0, f"{name}: {left} of {self.n} output elements were never written"
        assert bool((raw[self.n:] == mark).all()), f"{name}: the guard behind the output was written"
        return self.t


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def cpu(t):
    return None if t is None else t.detach().cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


def report(kind, quantity, path, ratio):
    w = float(ratio.max())
    print(f"ratio {quantity} {path} {w:.3f}" + ("" if kind == "A" else " (class B)"))
    return w


def profiled(env, fn):
    """kernel ids of the profiled launches fn() makes"""
    native = env["native"]
    native.profile_enable(64)
    try:
        fn()
        torch.cuda.synchronize()
        return [r[0] for r in native.profile_read(64)]
    finally:
        native.profile_enable(0)


# ------------------------------------------------------------------------------------------------------------------ be_conv_wgrad_f32
@pytest.mark.parametrize("case", tl.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_wgrad_vs_float64(env, case):
    """flat k_wgrad + k_sum_splits (ks 1 | 3), k_wgrad_conv1 from NHWC4 (ks 7), fc.1's (C,H,W) column gather (chw 9)"""
    n, h, w, cin, cout, ks, chw = case
    d = tl.conv_inputs(40 + n + cin, n, h, w, cin, cout, ks)
    dw = Guarded(cout, 3 if ks == 7 else cin, ks, ks)
    x, dy = dev(d["x"]), dev(d["dy"])
    env["native"].check(env["lib"].be_conv_wgrad_f32(env["native"].dptr(x), env["native"].dptr(dy), env["native"].dptr(dw.t), n, h, w, cin, cout, ks, chw,
                                                     env["native"].dptr(env["sc"]), env["sc_bytes"], env["stream"]()), "be_conv_wgrad_f32")
    torch.cuda.synchronize()
    ref = tl.wgrad_ref(d["x"], d["dy"], ks, chw)
    got = cpu(dw.check("dW"))
    assert report("A", "dW", f"be_conv_wgrad_f32{case}", tl.ratio_a(got, ref)) <= 1.0
    if ks == 3 and h * w == 1:
        assert int((ref["K"] == 0).sum()) > 0 and bool((got[ref["K"] == 0] == 0).all())      # taps never inside the map: exactly 0


# ------------------------------------------------------------------------------------------------------------------ BatchNorm, column sums
@pytest.mark.parametrize("with_res,act", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("M,C", tl.BN_CASES)
def test_bn_train_fwd_bwd_and_col_sum_vs_float64(env, M, C, with_res, act):
    """be_bn_train_fwd_f32 twice in a row (running statistics after two calls), be_bn_train_bwd_f32, be_col_sum_f32"""
    native, lib = env["native"], env["lib"]
    dp = native.dptr
    d = tl.bn_inputs(7, M, C)
    res = d["res"] if with_res else None
    y, gamma, beta, res_d, dout = dev(d["y"]), dev(d["gamma"]), dev(d["beta"]), dev(res), dev(d["dout"])
    rm, rv = dev(d["rm"]), dev(d["rv"])
    path = f"bn({M},{C},res={int(with_res)},act={int(act)})"
    worst_a, worst_b = [], []
    for call in (1, 2):
        rm0, rv0 = cpu(rm), cpu(rv)
        o = dict(mean=Guarded(C), invstd=Guarded(C), out=Guarded(M, C))
        if act:
            o["s_in"] = Guarded(M, C)
        native.check(lib.be_bn_train_fwd_f32(dp(y), dp(gamma), dp(beta), dp(res_d), tl.BN_EPS, tl.BN_MOMENTUM, dp(rm), dp(rv), dp(o["mean"].t),
                                             dp(o["invstd"].t), dp(o["s_in"].t) if act else None, dp(o["out"].t), M, C, int(act), dp(env["sc"]),
                                             env["sc_bytes"], env["stream"]()), "be_bn_train_fwd_f32")
        torch.cuda.synchronize()
        g = {k: cpu(v.check(k)) for k, v in o.items()}
        g["run_mean"], g["run_var"] = cpu(rm), cpu(rv)
        st64, st32 = tl.both(tl.bn_stats, d["y"], rm0, rv0)
        for k in ("mean", "invstd", "run_mean", "run_var"):
            worst_b.append(report("B", f"{k}#{call}", path, tl.ratio_b(g[k], st64[k], st32[k])))
        z = tl.both(tl.bn_apply, d["y"], g["mean"], g["invstd"], d["gamma"], d["beta"], res)
        if act:
            worst_b.append(report("B", "s_in", path, tl.ratio_b(g["s_in"], *z)))
            worst_b.append(report("B", "out", path, tl.ratio_b(g["out"], *tl.both(tl.smish_fwd, g["s_in"]))))
            if with_res:                                     # the planted extremes are where they were planted
                assert float((g["s_in"][0] - tl.plant_smish(g["s_in"])).abs().max()) <= 1e-3
        else:
            worst_b.append(report("B", "out", path, tl.ratio_b(g["out"], *z)))
    b = dict(ds=Guarded(M, C), dy=Guarded(M, C), dgamma=Guarded(C), dbeta=Guarded(C))
    s_in = dev(g["s_in"]) if act else None
    mean, invstd = dev(g["mean"]), dev(g["invstd"])
    native.check(lib.be_bn_train_bwd_f32(dp(dout), dp(s_in), dp(y), dp(mean), dp(invstd), dp(gamma), dp(b["ds"].t), dp(b["dy"].t), dp(b["dgamma"].t),
                                         dp(b["dbeta"].t), M, C, dp(env["sc"]), env["sc_bytes"], env["stream"]()), "be_bn_train_bwd_f32")
    cs = Guarded(C)
    native.check(lib.be_col_sum_f32(dp(y), dp(cs.t), M, C, dp(env["sc"]), env["sc_bytes"], env["stream"]()), "be_col_sum_f32")
    torch.cuda.synchronize()
    gb = {k: cpu(v.check(k)) for k, v in b.items()}
    if act:
        worst_b.append(report("B", "ds", path, tl.ratio_b(gb["ds"], *tl.both(tl.smish_bwd, d["dout"], g["s_in"]))))
    else:
        assert torch.equal(bits(gb["ds"]), bits(d["dout"]))
    worst_a.append(report("A", "dgamma", path, tl.ratio_a(gb["dgamma"], tl.dgamma_ref(gb["ds"], d["y"], g["mean"], g["invstd"]))))
    worst_a.append(report("A", "dbeta", path, tl.ratio_a(gb["dbeta"], tl.col_sum_ref(gb["ds"]))))
    worst_b.append(report("B", "dy", path, tl.ratio_b(gb["dy"], *tl.both(tl.bn_bwd_dy, gb["ds"], d["y"], g["mean"], g["invstd"], d["gamma"],
                                                                         gb["dgamma"], gb["dbeta"]))))
    worst_a.append(report("A", "col_sum", path, tl.ratio_a(cpu(cs.check("col_sum")), tl.col_sum_ref(d["y"]))))
    assert max(worst_a) <= 1.0 and max(worst_b) <= 1.0, (worst_a, worst_b)


# ------------------------------------------------------------------------------------------------------------------ max-pool
def _pool_case(env, x, dout, k, s, p, what):
    native, lib, train = env["native"], env["lib"], env["train"]
    dp = native.dptr
    n, h, w, c = x.shape
    oh, ow = dout.shape[1], dout.shape[2]
    y_ref, idx_ref, dx_ref = tl.pool_ref(x, dout, k, s, p)
    xd, dd = dev(x), dev(dout)
    y, idx, dx_i, dx_s = Guarded(n, oh, ow, c), Guarded(n, oh, ow, c, dtype=torch.uint8), Guarded(n, h, w, c), Guarded(n, h, w, c)
    native.check(lib.be_maxpool_nhwc_fwd_idx_f32(dp(xd), dp(y.t), dp(idx.t, "idx", (torch.uint8,)), n, h, w, c, k, s, p, env["stream"]()), "fwd_idx")
    native.check(lib.be_maxpool_nhwc_bwd_idx_f32(dp(idx.t, "idx", (torch.uint8,)), dp(dd), dp(dx_i.t), n, h, w, c, k, s, p, env["stream"]()), "bwd_idx")
    native.check(lib.be_maxpool_nhwc_bwd_f32(dp(xd), dp(dd), dp(dx_s.t), n, h, w, c, k, s, p, env["stream"]()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(cpu(y.check("y")), y_ref), what
    assert torch.equal(tl.pool_decode(idx.check("idx"), w, k, s, p), idx_ref), what
    assert torch.equal(cpu(dx_i.check("dx (idx)")), dx_ref), what
    assert torch.equal(cpu(dx_s.check("dx (scan)")), dx_ref), what
    # the wrappers of the step (the binding native.ops() selects): the same bits
    y2, saved = train._pool_fwd_idx(xd, k, s, p)
    assert torch.equal(y2, y.t) and torch.equal(saved[0], idx.t) and torch.equal(train._pool_bwd_idx(saved, dd, k, s, p), dx_i.t), what
    return dx_ref


@pytest.mark.parametrize("c", tl.POOL_CHANNELS)
@pytest.mark.parametrize("case", tl.POOL_CASES, ids=lambda v: "x".join(map(str, v)))
def test_maxpool_forward_winner_and_both_backwards_equal_torch(env, case, c):
    """distinct integers per plane and an integer dout: y, the decoded winner and dx are exact"""
    h, w, k, s, p = case
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    x = tl.pool_input(3, tl.POOL_N, h, w, c)
    dx = _pool_case(env, x, tl.pool_dout(4, tl.POOL_N, oh, ow, c), k, s, p, (case, c))
    if (h, w, k) == (5, 5, 2):                                # the last row and column belong to no window
        assert bool((dx[:, 4] == 0).all()) and bool((dx[:, :, 4] == 0).all())


@pytest.mark.parametrize("kind", ["negative", "ties"])
@pytest.mark.parametrize("case", [(11, 11, 3, 2, 1), (5, 7, 3, 2, 1), (6, 6, 2, 2, 0)], ids=lambda v: "x".join(map(str, v)))
def test_maxpool_all_negative_input_and_ties(env, case, kind):
    """all-negative: the padding must not win; ties (constant 4x4 patches, two alternating values): the first maximum in scan order"""
    h, w, k, s, p = case
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    _pool_case(env, tl.pool_input(5, tl.POOL_N, h, w, 12, kind), tl.pool_dout(6, tl.POOL_N, oh, ow, 12), k, s, p, (case, kind))


# ------------------------------------------------------------------------------------------------------------------ linears
def _linear_inputs(M, K, J, seed=5):
    g = tl.gen(seed)
    return tl.normal(g, M, K), tl.normal(g, J, K, scale=K ** -0.5), tl.normal(g, J, scale=0.1), tl.normal(g, M, J)


@pytest.mark.parametrize("M,K,J", tl.LINEAR_SMALL_CASES)
def test_linear_small_fwd_bwd_vs_float64(env, M, K, J):
    native, lib = env["native"], env["lib"]
    dp = native.dptr
    x, w, b, dy = _linear_inputs(M, K, J)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    o = dict(y=Guarded(M, J), dx=Guarded(M, K), dw=Guarded(J, K), db=Guarded(J))
    native.check(lib.be_linear_small_fwd_f32(dp(xd), dp(wd), dp(bd), dp(o["y"].t), M, K, J, env["stream"]()), "be_linear_small_fwd_f32")
    native.check(lib.be_linear_small_bwd_f32(dp(xd), dp(wd), dp(dyd), dp(o["dx"].t), dp(o["dw"].t), dp(o["db"].t), M, K, J, env["stream"]()),
                 "be_linear_small_bwd_f32")
    torch.cuda.synchronize()
    refs = dict(tl.linear_bwd_ref(x, w, dy), y=tl.linear_fwd_ref(x, w, b))
    worst = [report("A", k, f"linear_small({M},{K},{J})", tl.ratio_a(cpu(o[k].check(k)), refs[k])) for k in ("y", "dx", "dw", "db")]
    assert max(worst) <= 1.0, worst


@pytest.mark.parametrize("M,cin,cout", tl.LINEAR_GRAD_CASES)
def test_linear_param_grads_vs_float64(env, M, cin, cout):
    """k_lin_grads + k_bwd_post: 600 rows give two slices, 304 and 296 rows"""
    native, lib = env["native"], env["lib"]
    dp = native.dptr
    x, w, _, dy = _linear_inputs(M, cin, cout)
    xd, dyd = dev(x), dev(dy)
    o = dict(dw=Guarded(cout, cin), db=Guarded(cout))
    native.check(lib.be_linear_param_grads_f32(dp(xd), dp(dyd), dp(o["dw"].t), dp(o["db"].t), M, cin, cout, dp(env["sc"]), env["sc_bytes"],
                                               env["stream"]()), "be_linear_param_grads_f32")
    torch.cuda.synchronize()
    refs = tl.linear_bwd_ref(x, w, dy)
    worst = [report("A", k, f"linear_param_grads({M},{cin},{cout})", tl.ratio_a(cpu(o[k].check(k)), refs[k])) for k in ("dw", "db")]
    assert max(worst) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------ the units
FWD_OUT = ("y", "mean", "invstd", "out", "s_in")
BWD_OUT = ("ds", "dy", "dgamma", "dbeta", "dw", "db", "dx")


class Unit:
    """inputs of one unit on the CPU (d) and on the GPU (g), its packs, and the planted residual"""

    def __init__(self, env, seed, shape, chw=0, res=False, act=True, dx_add=False, want_dx=True, x=None):
        native, lib, train = env["native"], env["lib"], env["train"]
        n, h, w, cin, cout, ks = shape
        self.shape, self.chw, self.act, self.want_dx = shape, chw, act, want_dx
        d = tl.conv_inputs(seed, n, h, w, cin, cout, ks, want_res=res, want_add=dx_add)
        if x is not None:
            d["x"] = x
        if res and act:                                       # Smish extremes in the first row of the pre-activation
            d["res"] = tl.plant_res(tl.conv_fwd(d["x"], d["w"], d["b"], ks, chw), d["gamma"], d["beta"], d["res"])
        self.d = d
        self.g = {k: dev(v) for k, v in d.items()}
        self.fwd_pack = native.conv_pack(self.g["w"], self.g["b"], bn=None, chw_hw=chw)
        self.dg_pack = None
        if ks != 7:
            nd = lib.be_conv_dgrad_packed_floats(cout, cin, ks)
            pw, pb = train._new(nd, DEV), train._new((cin + 31) // 32 * 32, DEV)
            native.check(lib.be_conv_pack_dgrad_f32(native.dptr(self.g["w"]), cout, cin, ks, chw, native.dptr(pw), native.dptr(pb), env["stream"]()), "pack dgrad")
            self.dg_pack = (pw, pb)

    def packs(self, wi=0):
        class P:
            fwd, dg = {wi: self.fwd_pack}, ({wi: self.dg_pack} if self.dg_pack is not None else {})
        return P

    def fwd_bufs(self):
        n, h, w, _, cout, _ = self.shape
        o = dict(y=Guarded(n, h, w, cout), mean=Guarded(cout), invstd=Guarded(cout), out=Guarded(n, h, w, cout))
        if self.act:
            o["s_in"] = Guarded(n, h, w, cout)
        return o

    def bwd_bufs(self, want_dx=None):
        n, h, w, cin, cout, ks = self.shape
        o = dict(ds=Guarded(n, h, w, cout), dy=Guarded(n, h, w, cout), dgamma=Guarded(cout), dbeta=Guarded(cout),
                 dw=Guarded(cout, 3 if ks == 7 else cin, ks, ks), db=Guarded(cout))
        if self.want_dx if want_dx is None else want_dx:
            o["dx"] = Guarded(n, h, w, cin)
        return o

    def flat_grads(self):
        """dW, db, dgamma, dbeta as adjacent views of one guarded flat buffer (backward_train's layout)"""
        _, _, _, cin, cout, ks = self.shape
        nw = cout * (3 if ks == 7 else cin) * ks * ks
        flat = Guarded(nw + 3 * cout)
        v = flat.t
        return flat, dict(dw=v[:nw].view(cout, -1, ks, ks), db=v[nw:nw + cout], dgamma=v[nw + cout:nw + 2 * cout], dbeta=v[nw + 2 * cout:])

    def fwd_struct(self, env, o, rm, rv):
        native, g = env["native"], self.g
        dp = native.dptr
        return native.TrainUnitFwd(native.ConvDesc(*self.shape, 0), dp(g["x"]), dp(self.fwd_pack[0]), dp(self.fwd_pack[1]), dp(g["gamma"]), dp(g["beta"]),
                                   dp(g["res"]), dp(rm), dp(rv), dp(o["y"].t), dp(o["mean"].t), dp(o["invstd"].t),
                                   dp(o["s_in"].t) if self.act else None, dp(o["out"].t), int(self.act))

    def bwd_struct(self, env, f, b, with_add=True):
        native, g = env["native"], self.g
        dp = native.dptr
        pw, pb = self.dg_pack if "dx" in b else (None, None)
        return native.TrainUnitBwd(native.ConvDesc(*self.shape, 0), dp(g["x"]), dp(g["dout"]), dp(f["s_in"].t) if self.act else None, dp(f["y"].t),
                                   dp(f["mean"].t), dp(f["invstd"].t), dp(g["gamma"]), dp(pw), dp(pb), dp(g["dx_add"]) if with_add else None, int(self.chw),
                                   dp(b["ds"].t), dp(b["dy"].t), dp(b["dgamma"].t), dp(b["dbeta"].t), dp(b["dw"].t), dp(b["db"].t),
                                   dp(b["dx"].t) if "dx" in b else None)


def check_unit(u, path, f, b, rm0, rv0, rm1, rv1, dx_ref=None, dx_unwritten=False):
    """one unit's outputs (f, b: name -> CPU tensor, from the guarded run) stage by stage against float64 -> (worst class A, worst class B)"""
    d, (n, h, w, cin, cout, ks) = u.d, u.shape
    A, B = [], []
    A.append(report("A", "y", path, tl.ratio_a(f["y"], tl.conv_fwd_ref(d["x"], d["w"], d["b"], ks, u.chw))))
    st64, st32 = tl.both(tl.bn_stats, f["y"], rm0, rv0)
    got = dict(mean=f["mean"], invstd=f["invstd"], run_mean=rm1, run_var=rv1)
    for k in ("mean", "invstd", "run_mean", "run_var"):
        B.append(report("B", k, path, tl.ratio_b(got[k], st64[k], st32[k])))
    z = tl.both(tl.bn_apply, f["y"], f["mean"], f["invstd"], d["gamma"], d["beta"], d["res"])
    if u.act:
        B.append(report("B", "s_in", path, tl.ratio_b(f["s_in"], *z)))
        B.append(report("B", "out", path, tl.ratio_b(f["out"], *tl.both(tl.smish_fwd, f["s_in"]))))
        B.append(report("B", "ds", path, tl.ratio_b(b["ds"], *tl.both(tl.smish_bwd, d["dout"], f["s_in"]))))
        if d["res"] is not None:
            assert float((f["s_in"].reshape(-1, cout)[0] - tl.plant_smish(f["s_in"])).abs().max()) <= 1e-3
    else:
        B.append(report("B", "out", path, tl.ratio_b(f["out"], *z)))
        assert torch.equal(bits(b["ds"]), bits(d["dout"]))
    A.append(report("A", "dgamma", path, tl.ratio_a(b["dgamma"], tl.dgamma_ref(b["ds"], f["y"], f["mean"], f["invstd"]))))
    A.append(report("A", "dbeta", path, tl.ratio_a(b["dbeta"], tl.col_sum_ref(b["ds"]))))
    B.append(report("B", "dy", path, tl.ratio_b(b["dy"], *tl.both(tl.bn_bwd_dy, b["ds"], f["y"], f["mean"], f["invstd"], d["gamma"], b["dgamma"], b["dbeta"]))))
    A.append(report("A", "dW", path, tl.ratio_a(b["dw"], tl.wgrad_ref(d["x"], b["dy"], ks, u.chw))))
    A.append(report("A", "db", path, tl.ratio_a(b["db"], tl.col_sum_ref(b["dy"]))))
    if "dx" in b and not dx_unwritten:
        ref = dx_ref if dx_ref is not None else tl.dgrad_ref(b["dy"], d["w"], ks, u.chw, d["dx_add"])
        A.append(report("A", "dx", path, tl.ratio_a(b["dx"], ref)))
    return max(A), max(B)


def collect(bufs, skip=()):
    return {k: cpu(v.check(k)) if k not in skip else cpu(v.t) for k, v in bufs.items()}


@pytest.mark.parametrize("name", list(tl.UNIT_CASES))
def test_training_unit_stage_by_stage_vs_float64(env, name):
    """_unit_fwd + _unit_bwd at one shape per launch path (train_layers_oracle.UNIT_CASES says which host-code condition sends each
    there; test_train_layers_cpu.py holds that table against the conditions)"""
    native, lib, train = env["native"], env["lib"], env["train"]
    c = tl.UNIT_CASES[name]
    n, h, w, cin, cout, ks = c["shape"]
    u = Unit(env, 50 + n + cin, c["shape"], c["chw"], c["res"], c["act"], c["dx_add"], c["want_dx"])
    g, dp = u.g, native.dptr
    # ---- the C entry points, every output guarded on its own
    rm, rv = g["rm"].clone(), g["rv"].clone()
    fo, bo = u.fwd_bufs(), u.bwd_bufs()
    fs = u.fwd_struct(env, fo, rm, rv)
    ids_f = profiled(env, lambda: native.check(lib.be_train_unit_fwd_f32(
        C.byref(fs.desc), fs.x, fs.packed_w, fs.packed_bias, fs.gamma, fs.beta, fs.res, tl.BN_EPS, tl.BN_MOMENTUM, fs.run_mean, fs.run_var, fs.y, fs.mean,
        fs.invstd, fs.s_in, fs.out, fs.act, dp(env["sc"]), env["sc_bytes"], env["stream"]()), "be_train_unit_fwd_f32"))
    f = collect(fo)
    bs = u.bwd_struct(env, fo, bo)
    ids_b = profiled(env, lambda: native.check(lib.be_train_unit_bwd_f32(
        C.byref(bs.desc), bs.x, bs.dout, bs.s_in, bs.y, bs.mean, bs.invstd, bs.gamma, bs.dgrad_packed_w, bs.dgrad_packed_bias, bs.dx_add, bs.layout_chw_hw,
        bs.ds, bs.dy, bs.dgamma, bs.dbeta, bs.dw, bs.db, bs.dx, dp(env["sc"]), env["sc_bytes"], env["stream"]()), "be_train_unit_bwd_f32"))
    b = collect(bo)
    worst_a, worst_b = check_unit(u, name, f, b, u.d["rm"], u.d["rv"], cpu(rm), cpu(rv))
    # ---- the step's wrappers, parameter gradients as adjacent views of one flat buffer: the same bits
    rm2, rv2 = g["rm"].clone(), g["rv"].clone()
    out2, saved2 = train._unit_fwd(g["x"], u.packs(), 0, cout, ks, g["gamma"], g["beta"], rm2, rv2, g["res"], c["act"])
    flat, v = u.flat_grads()
    ds2, dx2 = train._unit_bwd(g["x"], g["dout"], saved2, g["gamma"], u.dg_pack if c["want_dx"] else None, g["dx_add"], ks, c["chw"], v["dgamma"],
                               v["dbeta"], v["dw"], v["db"])
    torch.cuda.synchronize()
    flat.check("flat gradient buffer")
    pairs = dict(out=(out2, fo["out"].t), y=(saved2[0], fo["y"].t), mean=(saved2[1], fo["mean"].t), invstd=(saved2[2], fo["invstd"].t),
                 run_mean=(rm2, rm), run_var=(rv2, rv), ds=(ds2, bo["ds"].t), **{k: (v[k], bo[k].t) for k in v})
    if c["act"]:
        pairs["s_in"] = (saved2[3], fo["s_in"].t)
    if c["want_dx"]:
        pairs["dx"] = (dx2, bo["dx"].t)
    else:
        assert dx2 is None
    for k, (p, q) in pairs.items():
        assert torch.equal(bits(p), bits(q.reshape(p.shape))), (name, k)
    # the path taken, where it has a profile kernel id (the merged backward-GEMMs launch and the balanced launch share id 12)
    assert ids_f == FWD_IDS[c["path"][0]], (name, ids_f)
    assert ids_b == BWD_IDS[c["path"][2]], (name, ids_b)
    assert worst_a <= 1.0 and worst_b <= 1.0, (name, worst_a, worst_b)


@pytest.mark.parametrize("name", list(tl.PAIR_CASES))
def test_unit_pair_stage_by_stage_vs_float64(env, name):
    """_unit_pair_fwd + _unit_pair_bwd: a 3x3 unit with Smish and a 1x1 downsample on one input; dx is the sum of both branches.
    24 images: outside the balanced launch (k_unit_gemms forward and backward); 64: inside it."""
    native, lib, train = env["native"], env["lib"], env["train"]
    n, h, w, cin, cout = tl.PAIR_CASES[name]
    ua = Unit(env, 70 + n, (n, h, w, cin, cout, 3), act=True)
    ub = Unit(env, 71 + n, (n, h, w, cin, cout, 1), act=False, x=ua.d["x"])
    ub.g["x"] = ua.g["x"]                                     # the pair shares the input tensor
    units = (ua, ub)
    dp = native.dptr
    rms = [(u.g["rm"].clone(), u.g["rv"].clone()) for u in units]
    fos, bos = [u.fwd_bufs() for u in units], [u.bwd_bufs() for u in units]
    fs = [u.fwd_struct(env, fo, *r) for u, fo, r in zip(units, fos, rms)]
    ids_f = profiled(env, lambda: native.check(lib.be_train_unit_pair_fwd_f32(C.byref(fs[0]), C.byref(fs[1]), tl.BN_EPS, tl.BN_MOMENTUM, dp(env["sc"]),
                                                                              env["sc_bytes"], env["stream"]()), "be_train_unit_pair_fwd_f32"))
    fl = [collect(fo) for fo in fos]
    bs = [u.bwd_struct(env, fo, bo, with_add=False) for u, fo, bo in zip(units, fos, bos)]
    ids_b = profiled(env, lambda: native.check(lib.be_train_unit_pair_bwd_f32(C.byref(bs[0]), C.byref(bs[1]), dp(env["sc"]), env["sc_bytes"], env["stream"]()),
                                               "be_train_unit_pair_bwd_f32"))
    bl = [collect(bos[0]), collect(bos[1], skip=("dx",))]     # b's dx is working space: its guard is checked, its content is not
    raw = bos[1]["dx"].buf.view(torch.int32)
    assert bool((raw[bos[1]["dx"].n:] == SENTINEL).all()), "the guard behind b's dx working space was written"
    dx_ref = tl.add_contractions(tl.dgrad_ref(bl[0]["dy"], ua.d["w"], 3), tl.dgrad_ref(bl[1]["dy"], ub.d["w"], 1))
    wa = check_unit(ua, name + ".conv3x3", fl[0], bl[0], ua.d["rm"], ua.d["rv"], cpu(rms[0][0]), cpu(rms[0][1]), dx_ref=dx_ref)
    wb = check_unit(ub, name + ".ds1x1", fl[1], bl[1], ub.d["rm"], ub.d["rv"], cpu(rms[1][0]), cpu(rms[1][1]), dx_unwritten=True)
    # ---- the step's wrappers with the gradients in one flat buffer per unit: the same bits
    rm2 = [(u.g["rm"].clone(), u.g["rv"].clone()) for u in units]

    class P:
        fwd, dg = {0: ua.fwd_pack, 6: ub.fwd_pack}, {0: ua.dg_pack, 6: ub.dg_pack}
    a_, b_ = [(wi, cout, ks, u.g["gamma"], u.g["beta"], *r, act) for wi, ks, u, r, act in ((0, 3, ua, rm2[0], True), (6, 1, ub, rm2[1], False))]
    (out_a, sv_a), (out_b, sv_b) = train._unit_pair_fwd(ua.g["x"], P, a_, b_)
    flats = [u.flat_grads() for u in units]
    a_, b_ = [(u.g["dout"], sv, u.g["gamma"], P.dg[wi], ks, fv[1]["dgamma"], fv[1]["dbeta"], fv[1]["dw"], fv[1]["db"])
              for wi, ks, u, sv, fv in ((0, 3, ua, sv_a, flats[0]), (6, 1, ub, sv_b, flats[1]))]
    ds_a, ds_b, dx = train._unit_pair_bwd(ua.g["x"], a_, b_)
    torch.cuda.synchronize()
    for j, (fo, bo, out, sv, ds, (flat, v), r, r2) in enumerate(zip(fos, bos, (out_a, out_b), (sv_a, sv_b), (ds_a, ds_b), flats, rms, rm2)):
        flat.check(f"flat gradient buffer {j}")
        pairs = dict(out=(out, fo["out"].t), y=(sv[0], fo["y"].t), mean=(sv[1], fo["mean"].t), invstd=(sv[2], fo["invstd"].t), ds=(ds, bo["ds"].t),
                     run_mean=(r2[0], r[0]), run_var=(r2[1], r[1]), **{k: (v[k], bo[k].t) for k in v})
        if j == 0:
            pairs["s_in"], pairs["dx"] = (sv[3], fo["s_in"].t), (dx, bo["dx"].t)
        for k, (p, q) in pairs.items():
            assert torch.equal(bits(p), bits(q.reshape(p.shape))), (name, j, k)
    assert ids_f == [ID_GEMMS] and ids_b == [ID_GEMMS], (ids_f, ids_b)
    assert max(wa[0], wb[0]) <= 1.0 and max(wa[1], wb[1]) <= 1.0, (name, wa, wb)
