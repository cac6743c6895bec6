"""Float64 reference, inputs and bounds for the layer-level tests of the training kernels (test_train_layers_cpu.py checks this
helper, test_train_layers_gpu.py compares the HIP kernels with it).  CPU only, plain torch, nothing from be_hip.

Layouts are the kernels': activations NHWC float32 ([n,h,w,c]; conv1 reads the NHWC4 staging, 3 channels + one of padding),
weights [cout,cin,k,k] as the state dict has them; fc.1 (`chw` > 0) reads features flattened in (h,w,c) order while its weight's
columns run (c,h,w).  Every reference is computed in float64 from the float32 tensors the stage under test READ (stage-wise teacher
forcing): no stage's rounding has to be allowed for in the next.

Two kinds of bound, both elementwise:
  A  contractions (conv y, dW, dx, db, column sums, dgamma, dbeta, linears):  |got - ref| <= (K + 2) 2^-24 S + 2^-24 |ref|, S the same
     contraction over the operands' absolute values in float64 and K its number of terms (taps inside the image only): the worst-case
     forward error of an fp32 sum of K products in ANY order, plus the rounding of the stored result.  Derived, not measured.
  B  elementwise / statistics outputs (mean, invstd, running statistics, s_in, out, ds, the BatchNorm backward's dy): four times the
     worst error, per tensor and channel, of torch's own float32 evaluation of the same stage from the same inputs, with a floor of
     4 * 2^-24 of the channel's largest reference magnitude.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.local_stage import smish

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
BN_EPS, BN_MOMENTUM = float(np.float32(1e-5)), float(np.float32(0.1))       # the float32 values the kernels receive
SMISH_PLANT = (-100.0, -20.0, -1.0, 0.0, 1.0, 20.0, 100.0)

# ------------------------------------------------------------------------------------------------------------------ cases
# be_conv_wgrad_f32 alone: (n, h, w, cin, cout, ks, chw).  ks = 7: cin = 4 is the NHWC4 staging, dW has 3 input channels.
WGRAD_CASES = [(3, 5, 7, 8, 12, 3, 0),          # rectangular, M = 105 (no multiple of 32), one ragged 64-tile each way
               (2, 6, 6, 68, 100, 1, 0),        # two tiles each way, the second nearly empty
               (5, 1, 1, 32, 32, 3, 0),         # every tap but the centre falls outside: those dW entries are exactly 0
               (4, 2, 2, 32, 32, 3, 0),
               (5, 1, 1, 72, 32, 1, 9),         # fc.1's (C,H,W) column gather
               (3, 9, 9, 4, 8, 7, 0), (2, 21, 21, 4, 64, 7, 0),
               (1, 3, 11, 4, 4, 3, 0)]          # M = 33: the smallest M at which pick_splits gives S = 2 with a ragged (1-row) last slice
BN_CASES = [(2, 4), (105, 100), (2304, 96)]
# (h, w, k, stride, pad)
POOL_CASES = [(21, 21, 3, 2, 1), (11, 11, 3, 2, 1), (6, 6, 3, 2, 1), (5, 7, 3, 2, 1), (6, 6, 2, 2, 0), (5, 5, 2, 2, 0)]
POOL_CHANNELS, POOL_N = (4, 12), 3
LINEAR_SMALL_CASES = [(1, 4, 1), (3, 1024, 10), (64, 1024, 10), (5, 64, 256)]
LINEAR_GRAD_CASES = [(256, 128, 128), (300, 128, 256), (600, 256, 128)]
# the units: name -> dict(shape = (n, h, w, cin, cout, ks), chw, res, act, dx_add, want_dx, path).  `path` = (forward, weight gradient,
# backward launch) as the host code decides them (unit_fwd_one / sk_fwd_eligible, plan_wgrad, unit_bwd_one / sk_eligible /
# conv_plan); expected_path() below re-derives it from the shape, and the CPU test holds the two together.
UNIT_CASES = {
    # n = 3: no 64-image group -> not the balanced launch; cout 32: 64-wide flat tiles (n % 32 != 0); dgrad onto cp = 32 -> 128x32 (variant 1)
    "flat64_v1": dict(shape=(3, 5, 7, 32, 32, 3), chw=0, res=True, act=True, dx_add=True, want_dx=True, path=("small", "flat64", "merged_v1")),
    # dgrad onto 64 channels -> 64x64 tiles (variant 0), 2 tiles x 54 half-chunks -> 4 K slices; 96 outputs: second 64-tile half empty
    "flat64_v0_splitk": dict(shape=(3, 5, 7, 64, 96, 3), chw=0, res=False, act=True, dx_add=False, want_dx=True, path=("small", "flat64", "merged_v0")),
    # 1x1, M = 64: uniform tiles (variant 2)
    "uniform_1x1": dict(shape=(16, 2, 2, 64, 64, 1), chw=0, res=False, act=False, dx_add=True, want_dx=True, path=("small", "flat64", "merged_v2")),
    # n % 32 == 0, 3x3: pixel-major 64-wide weight gradient
    "pm64": dict(shape=(32, 3, 3, 32, 96, 3), chw=0, res=True, act=False, dx_add=False, want_dx=True, path=("small", "pm64", "merged_v1")),
    # 128-wide: cin, cout % 128 == 0 and M = 288 >= 256; n % 16 != 0 -> flat
    "flat128_3x3": dict(shape=(8, 6, 6, 128, 128, 3), chw=0, res=False, act=True, dx_add=True, want_dx=True, path=("small", "flat128", "merged_v0")),
    "flat128_1x1": dict(shape=(8, 6, 6, 128, 128, 1), chw=0, res=True, act=True, dx_add=False, want_dx=True, path=("small", "flat128", "merged_v0")),
    # the same with the input gradient not wanted: k_wgrad128 launched on its own
    "flat128_no_dx": dict(shape=(8, 6, 6, 128, 128, 3), chw=0, res=False, act=True, dx_add=False, want_dx=False, path=("small", "flat128", "wgrad_alone")),
    # n % 16 == 0, M = 256: 128-wide pixel-major
    "pm128": dict(shape=(16, 4, 4, 128, 128, 3), chw=0, res=False, act=True, dx_add=False, want_dx=True, path=("small", "pm128", "merged_v0")),
    # whole 64-image groups on a 3x3 map: the balanced launch, one and two groups
    "balanced_1grp": dict(shape=(64, 3, 3, 64, 96, 3), chw=0, res=True, act=True, dx_add=True, want_dx=True, path=("balanced", "balanced", "balanced")),
    "balanced_2grp": dict(shape=(128, 3, 3, 64, 64, 3), chw=0, res=False, act=True, dx_add=False, want_dx=True, path=("balanced", "balanced", "balanced")),
    "fc1_balanced": dict(shape=(64, 1, 1, 576, 64, 1), chw=9, res=False, act=True, dx_add=False, want_dx=True, path=("balanced", "balanced", "balanced")),
    # 24 rows: 1x1 with M % 64 != 0 -> 64x64 bordered tiles (variant 0)
    "fc1_ragged": dict(shape=(24, 1, 1, 576, 64, 1), chw=9, res=False, act=True, dx_add=False, want_dx=True, path=("small", "flat64", "merged_v0")),
    # conv1: 7x7 from NHWC4, no input gradient; M = 882 / 1323 ragged against k_wgrad_conv1_mfma's 32-row blocks
    "conv1_n2": dict(shape=(2, 21, 21, 4, 64, 7), chw=0, res=False, act=True, dx_add=False, want_dx=False, path=("row8", "conv1_mfma", "conv1")),
    "conv1_n3": dict(shape=(3, 21, 21, 4, 64, 7), chw=0, res=False, act=True, dx_add=False, want_dx=False, path=("row8", "conv1_mfma", "conv1")),
}
PAIR_CASES = {"pair_ragged": (24, 3, 3, 64, 96), "pair_balanced": (64, 3, 3, 64, 96)}     # 3x3 + Smish and 1x1 downsample on one input
MAX_HW_BALANCED = 121            # be_sk::MAX_HW: maps of at most 11 x 11


def pick_splits(M, col_blocks, max_splits, target_blocks=1024):
    """be_train.hip's pick_splits"""
    max_splits = min(max_splits, 512)
    s = min((target_blocks + col_blocks - 1) // col_blocks, (M + 31) // 32, max_splits)
    return max(s, 1)


def wgrad_slices(n, h, w, cin, cout, ks):
    """(S, rows per slice, rows of the last slice) of be_conv_wgrad_f32's flat k_wgrad launch"""
    M = n * h * w
    S = pick_splits(M, ((cout + 63) // 64) * ((cin + 63) // 64) * ks * ks, 64, 512)
    rows = ((M + S - 1) // S + 31) // 32 * 32
    S = (M + rows - 1) // rows
    return S, rows, M - (S - 1) * rows


def expected_path(shape, chw, want_dx):
    """(forward, weight gradient, backward launch) from the host code's conditions (be_train.hip unit_fwd_one / plan_wgrad /
    unit_bwd_one, be_train_sk.hip sk_eligible / sk_fwd_eligible, be_conv.hip conv_plan's small-M branch)."""
    n, h, w, cin, cout, ks = shape
    M = n * h * w
    if ks == 7:
        return ("row8", "conv1_mfma", "conv1")
    groups = n >= 64 and n % 64 == 0 and h * w <= MAX_HW_BALANCED and (ks == 1 or (h >= 3 and w >= 3))
    fwd = "balanced" if groups and cout % 32 == 0 and cout >= 64 and cin % 32 == 0 else "small"
    bal = (groups and cout % 32 == 0 and cin % 32 == 0 and cout >= 64 and cin >= 64 and want_dx
           and (not chw or (ks == 1 and h * w == 1 and cin % chw == 0)))
    if bal:
        return (fwd, "balanced", "balanced")
    if not chw and cout % 128 == 0 and cin % 128 == 0 and M >= 256:
        wg = "pm128" if ks == 3 and n % 16 == 0 else "flat128"
    else:
        wg = "pm64" if ks == 3 and n % 32 == 0 and not chw else "flat64"
    if not want_dx:
        return (fwd, wg, "wgrad_alone")
    cp = (cin + 31) // 32 * 32                                       # the data gradient's output channels
    pixmaj = ks > 1 and n >= 64 and n % 64 == 0
    pad64 = cp % 64 == 32 and cp > 64 and (pixmaj or (ks == 1 and M % 64 == 0))
    t64 = cp % 64 == 0 or pad64
    uni = t64 and (pixmaj or (ks == 1 and M % 64 == 0))
    return (fwd, wg, "merged_v2" if uni else ("merged_v0" if t64 else "merged_v1"))


# ------------------------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def normal(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g, dtype=F64) * scale).to(F32)


def conv_inputs(seed, n, h, w, cin, cout, ks, want_res=False, want_add=False):
    """x (NHWC, NHWC4 with a zero fourth channel for ks = 7), w [cout, cin or 3, ks, ks], b, gamma, beta, dout, res, dx_add"""
    g = gen(seed)
    cw = 3 if ks == 7 else cin
    x = normal(g, n, h, w, cin)
    if ks == 7:
        x[..., 3] = 0.0
    d = dict(x=x, w=normal(g, cout, cw, ks, ks, scale=(cw * ks * ks) ** -0.5), b=normal(g, cout, scale=0.1),
             gamma=(1.0 + 0.1 * torch.randn(cout, generator=g, dtype=F64)).to(F32), beta=normal(g, cout, scale=0.1),
             dout=normal(g, n, h, w, cout), dy=normal(g, n, h, w, cout))
    d["rm"], d["rv"] = normal(g, cout, scale=0.1), (1.0 + 0.1 * torch.rand(cout, generator=g, dtype=F64)).to(F32)
    d["res"] = normal(g, n, h, w, cout) if want_res else None
    d["dx_add"] = normal(g, n, h, w, cin) if want_add else None
    return d


def bn_inputs(seed, M, C):
    """y [M, C]: channels c % 4 == 1 carry mean / std ~ 1e3 (a one-pass float32 variance loses them); the first row of the
    pre-activation s_in = (y - mean) invstd gamma + beta + res is planted with the Smish extremes through res."""
    g = gen(seed)
    y = normal(g, M, C)
    y[:, 1::4] = y[:, 1::4] * 0.5 + 500.0
    d = dict(y=y, gamma=(1.0 + 0.1 * torch.randn(C, generator=g, dtype=F64)).to(F32), beta=normal(g, C, scale=0.1),
             res=normal(g, M, C), dout=normal(g, M, C), rm=normal(g, C, scale=0.1), rv=(1.0 + 0.1 * torch.rand(C, generator=g, dtype=F64)).to(F32))
    d["res"] = plant_res(y, d["gamma"], d["beta"], d["res"])
    return d


def plant_smish(s_in):
    """the planted Smish pre-activations, cycled over the channels of s_in's first row"""
    C = s_in.shape[-1]
    return torch.tensor([SMISH_PLANT[c % len(SMISH_PLANT)] for c in range(C)], dtype=F32)


def plant_res(y, gamma, beta, res):
    """res with its first row changed so that the first row of s_in = (y - mean) invstd gamma + beta + res lands on the planted
    extremes (to the rounding of the kernel's own y, mean and invstd).  y: the stage's input in float64 or float32."""
    C = y.shape[-1]
    st = bn_stats(y, torch.zeros(C), torch.ones(C))
    z0 = bn_apply(y, st["mean"], st["invstd"], gamma, beta).reshape(-1, C)[0]
    res = res.clone()
    res.reshape(-1, C)[0] = (plant_smish(res).to(F64) - z0).to(F32)
    return res


def pool_input(seed, n, h, w, c, kind="perm"):
    """NHWC float32.  perm: every (image, channel) plane a permutation of distinct integers (exact in fp32, no ties);
    negative: the same minus h w + 5 (all below 0: padding must not win); ties: constant 4x4 patches / two alternating values."""
    g = gen(seed)
    if kind == "ties":
        x = torch.zeros(n, c, h, w, dtype=F32)
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        x[:, 0::2] = ((yy // 4) * 7 + (xx // 4) * 3).to(F32) % 5            # constant 4x4 patches
        x[:, 1::2] = ((yy + xx) % 2).to(F32) * 2.0 - 1.0                    # a plane of two alternating values
        return x.permute(0, 2, 3, 1).contiguous()
    planes = torch.stack([torch.randperm(h * w, generator=g) for _ in range(n * c)]).view(n, c, h, w).to(F32)
    if kind == "negative":
        planes = planes - float(h * w + 5)
    return planes.permute(0, 2, 3, 1).contiguous()


def pool_dout(seed, n, oh, ow, c):
    return torch.randint(-8, 9, (n, oh, ow, c), generator=gen(seed)).to(F32)


# ------------------------------------------------------------------------------------------------------------------ layouts
def nchw(t, dtype=F64):
    return t.permute(0, 3, 1, 2).to(dtype).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_operands(x, w, ks, chw, dtype):
    """kernel-layout x, w -> the NCHW operands of F.conv2d in `dtype`"""
    if ks == 7:
        return nchw(x[..., :3], dtype), w.to(dtype)
    if chw:                                                          # x [n,1,1,(hw,c)] -> columns (c,hw), the weight's order
        n, cin = x.shape[0], x.shape[-1]
        xc = x.reshape(n, chw, cin // chw).permute(0, 2, 1).reshape(n, cin, 1, 1)
        return xc.to(dtype).contiguous(), w.to(dtype)
    return nchw(x, dtype), w.to(dtype)


def x_grad_to_kernel_layout(gx, ks, chw):
    """gradient w.r.t. conv_operands' x -> the kernel's NHWC layout"""
    if chw:
        n, cin = gx.shape[0], gx.shape[1]
        return gx.reshape(n, cin // chw, chw).permute(0, 2, 1).reshape(n, 1, 1, cin).contiguous()
    return nhwc(gx)


# ------------------------------------------------------------------------------------------------------------------ class A
def contraction(ref, S, K):
    return dict(ref=ref, S=S, K=K if torch.is_tensor(K) else torch.full_like(ref, float(K)))


def bound_a(r):
    return (r["K"] + 2.0) * U * r["S"] + U * r["ref"].abs()


def ratio_a(got, r):
    """elementwise |got - ref| / bound; where the bound is 0 (no term inside the image) got must be exactly 0"""
    got = got.detach().cpu().to(F64).reshape(r["ref"].shape)
    err, b = (got - r["ref"]).abs(), bound_a(r)
    ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.nan_to_num(ratio, nan=float("inf"))


def worst(ratio):
    return float(ratio.max())


def _conv(x, w, b, ks):
    return F.conv2d(x, w, b, padding=ks // 2)


def conv_fwd(x, w, b, ks, chw=0, dtype=F64):
    """y NHWC = conv(x, w) + b"""
    xo, wo = conv_operands(x, w, ks, chw, dtype)
    return nhwc(_conv(xo, wo, b.to(dtype), ks))


def conv_fwd_ref(x, w, b, ks, chw=0):
    xo, wo = conv_operands(x, w, ks, chw, F64)
    S = nhwc(_conv(xo.abs(), wo.abs(), b.to(F64).abs(), ks))
    ones = torch.ones(1, 1, xo.shape[2], xo.shape[3], dtype=F64)
    K = nhwc(_conv(ones, torch.ones(1, 1, ks, ks, dtype=F64), None, ks)) * wo.shape[1] + 1.0      # taps inside x channels + bias
    return contraction(conv_fwd(x, w, b, ks, chw), S, K.expand(S.shape).contiguous())


def _wgrad(xo, dyo, wshape, ks):
    wz = torch.zeros(wshape, dtype=xo.dtype, requires_grad=True)
    return torch.autograd.grad(_conv(xo, wz, None, ks), wz, dyo)[0]


def wgrad(x, dy, ks, chw=0, dtype=F64):
    """dW [cout, cin (3 for ks 7), ks, ks]"""
    xo, _ = conv_operands(x, torch.zeros(1), ks, chw, dtype)
    return _wgrad(xo, nchw(dy, dtype), (dy.shape[-1], xo.shape[1], ks, ks), ks)


def wgrad_ref(x, dy, ks, chw=0):
    xo, _ = conv_operands(x, torch.zeros(1), ks, chw, F64)
    dyo = nchw(dy)
    shape = (dyo.shape[1], xo.shape[1], ks, ks)
    S = _wgrad(xo.abs(), dyo.abs(), shape, ks)
    n, _, h, w = xo.shape
    K = _wgrad(torch.ones(n, 1, h, w, dtype=F64), torch.ones(n, 1, h, w, dtype=F64), (1, 1, ks, ks), ks)   # pixels with the tap inside
    return contraction(_wgrad(xo, dyo, shape, ks), S, K.expand(shape).contiguous())


def _dgrad(dyo, wo, xshape, ks):
    xz = torch.zeros(xshape, dtype=dyo.dtype, requires_grad=True)
    return torch.autograd.grad(_conv(xz, wo, None, ks), xz, dyo)[0]


def dgrad(dy, w, ks, chw=0, dx_add=None, dtype=F64):
    """dx in the kernel's layout (+ dx_add)"""
    n, h, ww, _ = dy.shape
    gx = x_grad_to_kernel_layout(_dgrad(nchw(dy, dtype), w.to(dtype), (n, w.shape[1], h, ww), ks), ks, chw)
    return gx if dx_add is None else gx + dx_add.to(dtype)


def dgrad_ref(dy, w, ks, chw=0, dx_add=None):
    n, h, ww, cout = dy.shape
    shape = (n, w.shape[1], h, ww)
    S = x_grad_to_kernel_layout(_dgrad(nchw(dy).abs(), w.to(F64).abs(), shape, ks), ks, chw)
    K = nhwc(_dgrad(torch.ones(1, 1, h, ww, dtype=F64), torch.ones(1, 1, ks, ks, dtype=F64), (1, 1, h, ww), ks)) * cout
    K = K.expand(S.shape).contiguous()
    if dx_add is not None:
        S, K = S + dx_add.to(F64).abs(), K + 1.0
    return contraction(dgrad(dy, w, ks, chw, dx_add), S, K)


def add_contractions(a, b):
    """the sum of two contractions (a pair's dx): terms and magnitudes add"""
    return dict(ref=a["ref"] + b["ref"], S=a["S"] + b["S"], K=a["K"] + b["K"])


def col_sum(a, dtype=F64):
    return a.reshape(-1, a.shape[-1]).to(dtype).sum(0)


def col_sum_ref(a):
    a2 = a.reshape(-1, a.shape[-1]).to(F64)
    return contraction(a2.sum(0), a2.abs().sum(0), a2.shape[0])


def xhat(y, mean, invstd, dtype=F64):
    return (y.to(dtype) - mean.to(dtype)) * invstd.to(dtype)


def dgamma(ds, y, mean, invstd, dtype=F64):
    return col_sum(ds.to(dtype) * xhat(y, mean, invstd, dtype), dtype)


def dgamma_ref(ds, y, mean, invstd):
    """sum_m ds xhat with xhat = (y - mean) invstd from the float32 mean / invstd the kernel read.  The two roundings of xhat take the
    place of the product's in the (K + 2) count."""
    t = ds.to(F64) * xhat(y, mean, invstd)
    return col_sum_ref(t)


def linear_fwd(x, w, b, dtype=F64):
    return F.linear(x.to(dtype), w.to(dtype), b.to(dtype))


def linear_fwd_ref(x, w, b):
    S = F.linear(x.to(F64).abs(), w.to(F64).abs(), b.to(F64).abs())
    return contraction(linear_fwd(x, w, b), S, x.shape[1] + 1)


def linear_bwd(x, w, dy, dtype=F64):
    """(dx, dw, db) of y = x w^T + b"""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    return dy @ w, dy.t() @ x, dy.sum(0)


def linear_bwd_ref(x, w, dy):
    dx, dw, db = linear_bwd(x, w, dy)
    sx, sw, sb = linear_bwd(x.abs(), w.abs(), dy.abs())
    return dict(dx=contraction(dx, sx, w.shape[0]), dw=contraction(dw, sw, x.shape[0]), db=contraction(db, sb, x.shape[0]))


# ------------------------------------------------------------------------------------------------------------------ class B
def ratio_b(got, ref64, ref32):
    """per channel (last dimension): |got - ref| against max(4 x the float32 run's worst error, 4 * 2^-24 max |ref|) of the channel"""
    C = ref64.shape[-1]
    r64 = ref64.reshape(-1, C)
    got = got.detach().cpu().to(F64).reshape(-1, C)
    e32 = (ref32.to(F64).reshape(-1, C) - r64).abs().amax(0)
    b = torch.maximum(4.0 * e32, 4.0 * U * r64.abs().amax(0))
    ratio = (got - r64).abs().amax(0) / b.clamp_min(1e-300)
    return torch.nan_to_num(ratio, nan=float("inf"))


def both(fn, *a, **k):
    """(float64, float32) evaluations of fn(..., dtype=)"""
    return fn(*a, dtype=F64, **k), fn(*a, dtype=F32, **k)


def bn_stats(y, rm, rv, dtype=F64, eps=BN_EPS, momentum=BN_MOMENTUM):
    """mean, invstd, new running mean, new running variance (unbiased, M / (M - 1)) of y [.., C]"""
    y2 = y.reshape(-1, y.shape[-1]).to(dtype)
    M = y2.shape[0]
    var, mean = torch.var_mean(y2, 0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    unb = var * (M / (M - 1.0)) if M > 1 else var
    return dict(mean=mean, invstd=invstd, run_mean=(1.0 - momentum) * rm.to(dtype) + momentum * mean,
                run_var=(1.0 - momentum) * rv.to(dtype) + momentum * unb)


def bn_apply(y, mean, invstd, gamma, beta, res=None, dtype=F64):
    """s_in = (y - mean) invstd gamma + beta (+ res) from the float32 mean / invstd the kernel read"""
    z = xhat(y, mean, invstd, dtype) * gamma.to(dtype) + beta.to(dtype)
    return z if res is None else z + res.to(dtype)


def smish_fwd(s_in, dtype=F64):
    return smish(s_in.to(dtype))


def smish_bwd(dout, s_in, dtype=F64):
    """ds = dout smish'(s_in) by autograd"""
    s = s_in.to(dtype).clone().requires_grad_(True)
    return torch.autograd.grad(smish(s), s, dout.to(dtype))[0]


def bn_bwd_dy(ds, y, mean, invstd, gamma, dgam, dbet, dtype=F64):
    """dy = gamma invstd (ds - dbeta / M - xhat dgamma / M) from the dgamma / dbeta the kernel read"""
    M = y.numel() // y.shape[-1]
    xh = xhat(y, mean, invstd, dtype)
    return gamma.to(dtype) * invstd.to(dtype) * (ds.to(dtype) - dbet.to(dtype) / M - xh * dgam.to(dtype) / M)


# ------------------------------------------------------------------------------------------------------------------ max-pool
def pool_ref(x, dout, k, stride, pad):
    """x NHWC float32 -> (y NHWC, winner flat index y * w + x per [n,oh,ow,c], dx NHWC) of F.max_pool2d in float64"""
    xo = nchw(x).requires_grad_(True)
    y, idx = F.max_pool2d(xo, k, stride, pad, return_indices=True)
    dx = torch.autograd.grad(y, xo, nchw(dout))[0]
    return nhwc(y.detach()).to(F32), nhwc(idx), nhwc(dx).to(F32)


def pool_decode(idx, w, k, stride, pad):
    """the kernels' idx byte (dy * k + dx of the winner, [n,oh,ow,c]) -> flat index y * w + x"""
    idx = idx.cpu().long()
    oh, ow = idx.shape[1], idx.shape[2]
    oy = torch.arange(oh).view(1, oh, 1, 1) * stride - pad
    ox = torch.arange(ow).view(1, 1, ow, 1) * stride - pad
    return (oy + idx // k) * w + (ox + idx % k)


def pool_unique_max(x, k, stride, pad):
    """True when every window of x (NHWC) has a single maximum (padding = -inf)"""
    xo = F.pad(nchw(x), (pad, pad, pad, pad), value=float("-inf"))
    win = xo.unfold(2, k, stride).unfold(3, k, stride).reshape(*xo.shape[:2], -1, k * k)
    top = win.topk(2, dim=-1).values
    return bool((top[..., 0] > top[..., 1]).all())


# ------------------------------------------------------------------------------------------------------------------ defects
# A float32 CPU implementation of the contractions written the way a kernel walks them (flat pixel index + tap offset, a GEMM over
# K rows), with one defect planted: what the class-A bound has to flag.
DEFECTS = ("drop_row", "double_row", "wrong_neighbour", "swap_hw", "zero_column", "hwc_columns")


def im2col(a, ks, defect=None, mirror=False):
    """a NHWC float32 -> [M, taps, C]: row m = (img, y, x), tap (ty, tx) reads pixel m + tdy W + tdx when inside the image"""
    n, h, w, c = a.shape
    H, W = (w, h) if defect == "swap_hw" else (h, w)                  # swap_hw: the map decoded as w x h
    flat = a.reshape(n * h * w, c)
    m = torch.arange(n * h * w)
    y, x = (m % (H * W)) // W, m % W
    half = ks // 2
    out = torch.zeros(n * h * w, ks * ks, c, dtype=a.dtype)
    for ty in range(ks):
        for tx in range(ks):
            tdy, tdx = (half - ty, half - tx) if mirror else (ty - half, tx - half)
            ok = (y + tdy >= 0) & (y + tdy < H) & (x + tdx >= 0) & (x + tdx < W)
            off = torch.full_like(m, tdy * W + tdx)
            if defect == "wrong_neighbour" and tdy == 1 and tdx == 0:
                last = int(m[ok][-1])                                # the last row that has this tap: its offset computed with H
                off[last] = tdy * h + tdx if W == w and h != w else tdy * W + tdx + 1
            src = (m + off).clamp(0, n * h * w - 1)
            out[:, ty * ks + tx] = torch.where(ok[:, None], flat[src], torch.zeros((), dtype=a.dtype))
    return out


def gemm_kt(P, Q, defect=None, row=None):
    """P [K, I], Q [K, J] -> P^T Q [I, J] in float32; drop_row / double_row: K row `row` left out / taken twice; zero_column: the
    last output column (of the ragged last tile) left at zero"""
    out = P.t() @ Q
    if defect in ("drop_row", "double_row"):
        term = P[row][:, None] * Q[row][None, :]
        out = out - term if defect == "drop_row" else out + term
    if defect == "zero_column":
        out[:, -1] = 0.0
    return out


def kernel_like(kind, d, ks, chw=0, defect=None):
    """float32 CPU evaluation of contraction `kind` (conv_fwd | wgrad | dgrad) from the inputs d, NHWC results in the kernels' layout"""
    x, w, dy = d["x"], d["w"], d["dy"]
    n, h, ww, cin = x.shape
    cout, taps = w.shape[0], ks * ks
    M = n * h * ww
    row = min(32, M - 1)                                             # a K-slice boundary of the row-split kernels
    geo = defect if defect in ("wrong_neighbour", "swap_hw") else None
    red = defect if defect in ("drop_row", "double_row", "zero_column") else None
    wk = w
    if chw and defect != "hwc_columns":                              # weight columns (c, hw) -> the activations' (hw, c)
        wk = w.reshape(cout, cin // chw, chw).permute(0, 2, 1).reshape(cout, cin, 1, 1)
    wmat = wk.permute(2, 3, 1, 0).reshape(taps * cin, cout)          # [(tap, ci), co]
    if kind == "conv_fwd":
        A = im2col(x, ks, geo).reshape(M, taps * cin)
        return (gemm_kt(A.t().contiguous(), wmat, red, row=min(32, taps * cin - 1)) + d["b"]).reshape(n, h, ww, cout)
    if kind == "wgrad":
        A = im2col(x, ks, geo).reshape(M, taps * cin)
        dw = gemm_kt(dy.reshape(M, cout), A, red, row=row).reshape(cout, ks, ks, cin).permute(0, 3, 1, 2)
        if chw and defect != "hwc_columns":                          # back to the weight's (c, hw) column order
            dw = dw.reshape(cout, chw, cin // chw).permute(0, 2, 1).reshape(cout, cin, 1, 1)
        return dw.contiguous()
    if kind == "dgrad":
        A = im2col(dy, ks, geo, mirror=True).reshape(M, taps * cout)
        wt = wk.permute(2, 3, 0, 1).reshape(taps * cout, cin)        # [(tap, co), ci]
        return gemm_kt(A.t().contiguous(), wt, red, row=min(32, taps * cout - 1)).reshape(n, h, ww, cin)
    raise ValueError(kind)
