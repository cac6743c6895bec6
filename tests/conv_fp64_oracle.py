"""The fp32 convolution (be_conv.hip, be_conv_pm.hip and the row GEMM it routes to) in float64, with a DERIVED per-element bound.
CPU only, no library.

    ref  the convolution evaluated in float64 from the float32 operands: conv2d with padding ks // 2, then - where BatchNorm is
         given - BN unfused, (conv + b - mean) * gamma / sqrt(var + eps) + beta, plus conv1x1(x2, w2), plus the residual
    mag  the same expression with every operand replaced by its absolute value and every subtraction by an addition:
         conv2d(|x|, |w * scale|) + (|b| + |mean|) * |scale| + |beta| + conv1x1(|x2|, |w2|) + |res|

The bound:  |y - ref| <= (K + 16) * 2**-24 * mag,   K = cin_real * ks * ks + cin2 real products per output (cin_real = 3 at 7x7).
That is the standard gamma_n bound for a sum of K fp32 products in any order, with or without FMA, with or without K slices; the 16
covers the fold of BN into the weights (gamma / sqrtf(var + eps), one multiply per weight, the bias fold), the bias add, the residual
add and the slice sum of split K.  With N(0,1) inputs and He-scaled weights it is about 2e-4 absolute on outputs of size 1.4: a
dropped tap or channel chunk exceeds it by two orders of magnitude, operands rounded to tf32 or bf16 several times over.

Smish:  smish64(v) = v * tanh(log1p(sigmoid(v))), and |smish_gpu(v) - smish64(v)| <= (|v| + 16) * 2**-24 * |smish64(v)| + 2**-120
for v the float32 pre-activation.  be::smish is x * num / den with num and den sums of positive terms in t = __expf(-|x|), so
nothing cancels; t's relative error is about |x| ulp (the fp32 product with log2(e)) plus 1 ulp each for v_exp_f32 and v_rcp_f32,
the 16 holds the fmaf chains with room to spare, and the absolute term covers results flushed below the normal range."""
import numpy as np
import torch

U = 2.0 ** -24                     # the unit roundoff of float32
SLACK = 16


def _nchw64(a):
    """[N,H,W,C] float32 numpy -> [N,C,H,W] float64 torch"""
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def products(cin, ks, cin2=0):
    """K: the real products per output element (the 7x7 convolution reads 3 real channels of its 4)"""
    return (3 if ks == 7 else cin) * ks * ks + cin2


def conv_ref(x, weight, bias, ks, bn=None, eps=1e-5, x2=None, w2=None, res=None):
    """x [N,H,W,cin], weight [cout,cin_w,ks,ks] (cin_w = 3 at ks 7: the fourth staged channel is padding), bias [cout] | None,
    bn = (gamma, beta, mean, var) | None, x2 [N,H,W,cin2] with w2 [cout,cin2,1,1], res [N,H,W,cout] (any strides): float32 numpy.
    -> ref, mag: [N,H,W,cout] float64 numpy"""
    conv = torch.nn.functional.conv2d
    w64 = torch.from_numpy(np.ascontiguousarray(weight)).double()
    cout, cin_w = w64.shape[0], w64.shape[1]
    w64 = w64.reshape(cout, cin_w, ks, ks)
    x64 = _nchw64(x[..., :cin_w])
    b64 = torch.zeros(cout, dtype=torch.float64) if bias is None else torch.from_numpy(np.asarray(bias)).double()
    c = lambda v: v.view(1, cout, 1, 1)
    ref = conv(x64, w64, padding=ks // 2) + c(b64)
    if bn is not None:
        gamma, beta, mean, var = (torch.from_numpy(np.asarray(t)).double() for t in bn)
        scale = gamma / torch.sqrt(var + float(eps))
        ref = (ref - c(mean)) * c(scale) + c(beta)
        mag = conv(x64.abs(), (w64 * scale.view(cout, 1, 1, 1)).abs(), padding=ks // 2) + c((b64.abs() + mean.abs()) * scale.abs() + beta.abs())
    else:
        mag = conv(x64.abs(), w64.abs(), padding=ks // 2) + c(b64.abs())
    if x2 is not None:
        w2_64 = torch.from_numpy(np.ascontiguousarray(w2)).double().reshape(cout, -1, 1, 1)
        ref = ref + conv(_nchw64(x2), w2_64)
        mag = mag + conv(_nchw64(x2).abs(), w2_64.abs())
    if res is not None:
        r64 = _nchw64(res)
        ref, mag = ref + r64, mag + r64.abs()
    return ref.permute(0, 2, 3, 1).contiguous().numpy(), mag.permute(0, 2, 3, 1).contiguous().numpy()


def conv_f32(x, weight, bias, ks, bn=None, eps=1e-5, x2=None, w2=None, res=None):
    """the same expression by conv2d in float32 on the CPU (BN unfused, as in conv_ref): what an honest fp32 evaluation errs
    against ref - the yardstick of the rms check, never the library"""
    conv = torch.nn.functional.conv2d
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()
    nchw = lambda a: f(a).permute(0, 3, 1, 2)
    w = f(weight)
    cout, cin_w = w.shape[0], w.shape[1]
    y = conv(nchw(x[..., :cin_w]), w.reshape(cout, cin_w, ks, ks), None if bias is None else f(bias), padding=ks // 2)
    if bn is not None:
        gamma, beta, mean, var = (f(t).view(1, cout, 1, 1) for t in bn)
        y = (y - mean) * (gamma / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))) + beta
    if x2 is not None:
        y = y + conv(nchw(x2), f(w2).reshape(cout, -1, 1, 1))
    if res is not None:
        y = y + nchw(res)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def bound(mag, K):
    return (K + SLACK) * U * mag


def worst(y, ref, mag, K):
    """max over the elements of |y - ref| / bound (a non-finite y counts as infinitely far; 0 / 0 as inside)"""
    err = np.abs(np.asarray(y, dtype=np.float64) - ref)
    with np.errstate(invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / np.maximum(bound(mag, K), 1e-300))
    return float(np.where(np.isfinite(err), ratio, np.inf).max())


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))


def smish64(v):
    v = np.asarray(v, dtype=np.float64)
    sig = np.where(v >= 0, 1.0 / (1.0 + np.exp(-np.abs(v))), np.exp(-np.abs(v)) / (1.0 + np.exp(-np.abs(v))))
    return v * np.tanh(np.log1p(sig))


def smish_bound(v):
    """for v the float32 pre-activation"""
    v = np.asarray(v, dtype=np.float64)
    return (np.abs(v) + SLACK) * U * np.abs(smish64(v)) + 2.0 ** -120


def smish_worst(y, v):
    err = np.abs(np.asarray(y, dtype=np.float64) - smish64(v))
    return float(np.where(np.isfinite(err), err / smish_bound(v), np.inf).max())
