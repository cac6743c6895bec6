"""Go / no-go of folding the Winograd blocks' 1x1 downsample into conv2's transform-domain GEMMs, emulated on the CPU (numpy / torch;
nothing in the product uses it).

Today a block of layers 1-3 computes  y = act((A^T M2 A + (b2 + b_ds)) + x W_ds)  with the 1x1 downsample as a split-bf16 row GEMM over
the 36 pixels, added behind conv2's output transform.  A 1x1 convolution is a 3x3 with only the centre tap, whose kernel transform
G[:,1] (x) G'[:,1] W_ds is non-zero at 6 x 3 = 18 of the 40 positions of the 8x5 tiles, so conv2's GEMMs can take it as a second K
segment there:  M2[z] = V_h[z] U2[z] + V_x[z] U_ds[z]  (V_x: the block's own input transform).  The downsample term then passes
through B^T . B, the split-bf16 GEMM and A^T . A instead of being added nearly exactly, so rounding changes.  This script emulates both
forms with the kernels' arithmetic - be_wino_math.h's operation order for the three transforms (every fmaf as one rounding), the
weight pack's (G along the rows in double rounded once, along the columns in fp32), split8's pieces, six bf16 MFMAs per 16-deep chunk
with one fp32 rounding each, V_h chunks ascending then V_x chunks ascending from a zero accumulator - on
  blocks      the three residual blocks 96->256, 256->384, 384->256 alone, against the float64 block (L-inf / L-inf);
  LocalStage  the whole eval forward against the float64 oracle (layers 1-3 and fc.1 emulated; conv1, the pools, layer0 and fc.4 in
              torch float32, the same in both arms), on the synthetic weights (two seeds), the five stressed cases of
              tests/test_hip_parity.py and the trained checkpoint where checkpoints/pretrained_local_stage.pth exists.
Bounds (the project's own): a Winograd layer within 1.5e-5 of float64 (tests/test_hip_parity.py, tests/test_wino_split_bf16.py), the
logits within 1e-5 and, at the default synthetic weights on uniform_patches(16), within 6e-6
(test_local_stage_logits_vs_golden_and_oracle).  Measured figures: profiles/HISTORY.md, Round 24.
    python lab/wino_ds_fold_error.py [patches]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "blurry-edges_amd")]
from be_hip import synth                                   # noqa: E402
from oracle import local_stage as ols                      # noqa: E402

f32, f64 = np.float32, np.float64


def fma(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, one rounding to float32 (the double rounding is below 2^-53)"""
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


# ---- be_wino_math.h, operation for operation (float32 arrays; the vector index is the leading axis of d / m) -------------------------
def bt5(d):
    o0 = fma(-2.0, d[2], fma(2.0, d[0], -d[1])) + d[3]
    o1 = fma(-2.0, d[1], d[3]) - d[2]
    o2 = fma(2.0, d[1], fma(-3.0, d[2], d[3]))
    o3 = d[3] - d[1]
    o4 = fma(-2.0, d[3], fma(2.0, d[1], -d[2])) + d[4]
    return np.stack([o0, o1, o2, o3, o4])


def bt8(d):
    o0 = fma(5.25, d[4] - d[2], d[0] - d[6])
    o7 = fma(5.25, d[3] - d[5], d[7] - d[1])
    e1, f1 = fma(-4.25, d[4], d[2] + d[6]), fma(-4.25, d[3], d[1] + d[5])
    e2, f2 = fma(0.25, d[2], fma(-1.25, d[4], d[6])), fma(0.5, d[1], fma(-2.5, d[3], f32(2.0) * d[5]))
    e3, f3 = fma(4.0, d[2], fma(-5.0, d[4], d[6])), fma(2.0, d[1], fma(-2.5, d[3], f32(0.5) * d[5]))
    return np.stack([o0, e1 + f1, e1 - f1, e2 + f2, e2 - f2, e3 + f3, e3 - f3, o7])


def at5(m):
    return np.stack([((m[0] + m[1]) + m[2]) + m[3], fma(2.0, m[3], m[1] - m[2]), fma(4.0, m[3], m[1] + m[2]) + m[4]])


def at8(m):
    s12, d12, s34, d34, s56, d56 = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4], m[5] + m[6], m[5] - m[6]
    return np.stack([((m[0] + s12) + s34) + s56, fma(0.5, d56, fma(2.0, d34, d12)), fma(0.25, s56, fma(4.0, s34, s12)),
                     fma(0.125, d56, fma(8.0, d34, d12)), fma(0.0625, s56, fma(16.0, s34, s12)),
                     fma(0.03125, d56, fma(32.0, d34, d12)) + m[7]])


def g_rows(a, b, c):
    A, B, C = a.astype(f64), b.astype(f64), c.astype(f64)
    return np.stack([a, (-(A + B + C) * (2.0 / 9.0)).astype(f32), (-(A - B + C) * (2.0 / 9.0)).astype(f32),
                     ((A + 2.0 * B + 4.0 * C) * (1.0 / 90.0)).astype(f32), ((A - 2.0 * B + 4.0 * C) * (1.0 / 90.0)).astype(f32),
                     ((A + 0.5 * B + 0.25 * C) * (32.0 / 45.0)).astype(f32), ((A - 0.5 * B + 0.25 * C) * (32.0 / 45.0)).astype(f32), c])


def g5(a, b, c):
    sixth = f32(1.0) / f32(6.0)
    return np.stack([f32(0.5) * a, f32(-0.5) * (a + b + c), -(a - b + c) * sixth, (a + f32(2.0) * b + f32(4.0) * c) * sixth, c])


def wino_in(x):
    """x [n,6,6,C] float32 -> V [40][2n][C]: columns first (B^T of the 8 window rows), then the 5-point transform of each row"""
    n, _, _, C = x.shape
    xp = np.zeros((n, 8, 8, C), f32)
    xp[:, 1:7, 1:7] = x
    d = np.stack([xp[:, :, 3 * tx:3 * tx + 5] for tx in range(2)], 1).reshape(2 * n, 8, 5, C)      # tile = 2 img + tx
    t = bt8(d.transpose(1, 0, 2, 3))                                                              # [8][2n][5][C]
    v = bt5(t.transpose(2, 1, 0, 3))                                                              # [5 c][2n][8 r][C]
    return v.transpose(2, 0, 1, 3).reshape(40, 2 * n, C)                                          # z = 5 r + c


def wino_out(M):
    """M [40][2n][C] -> y [n,6,6,C] without bias: columns first (A^T 3x5 of each transform row), then A^T 6x8"""
    _, tn, C = M.shape
    m = M.reshape(8, 5, tn, C)
    t = at5(m.transpose(1, 0, 2, 3))                                                              # [3 c][8 r][2n][C]
    o = at8(t.transpose(1, 0, 2, 3))                                                              # [6 r][3 c][2n][C]
    return o.reshape(6, 3, tn // 2, 2, C).transpose(2, 0, 3, 1, 4).reshape(tn // 2, 6, 6, C)


def fold_bn(sd, p):
    scale = (sd[p + ".1.weight"] / np.sqrt(sd[p + ".1.running_var"] + f32(ols.BN_EPS))).astype(f32)
    bias = ((sd[p + ".0.bias"] - sd[p + ".1.running_mean"]) * scale + sd[p + ".1.bias"]).astype(f32)
    return scale, bias


def pack3x3(w, scale):
    """k_wino_pack: [cout,cin,3,3] * scale -> U [40][cin][cout]"""
    g = (w * scale[:, None, None, None]).astype(f32)
    t = np.stack([g_rows(g[:, :, 0, c], g[:, :, 1, c], g[:, :, 2, c]) for c in range(3)])         # [3 c][8 r][cout][cin]
    u = g5(t[0], t[1], t[2])                                                                      # [5 c][8 r][cout][cin]
    return u.transpose(1, 0, 3, 2).reshape(40, w.shape[1], w.shape[0])


def pack_ds(w, scale):
    """the BN-folded 1x1 matrix as a 3x3 with only the centre tap, through the same arithmetic"""
    w3 = np.zeros(w.shape[:2] + (3, 3), f32)
    w3[:, :, 1, 1] = w[:, :, 0, 0]
    return pack3x3(w3, scale)


# ---- split-bf16 GEMM (lab/wino_split_bf16_error.py) -----------------------------------------------------------------------------------
def bf16_rne(x):
    u = np.asarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(f32)


def split3(x):
    hi = bf16_rne(x)
    r = (x - hi).astype(f32)
    mid = bf16_rne(r)
    return [p.astype(f64) for p in (hi, mid, bf16_rne((r - mid).astype(f32)))]


ORDER = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]                                           # lo.hi hi.lo mid.mid mid.hi hi.mid hi.hi


def gemm_bf16x6(a, b, acc=None):
    """acc (+)= a [rows,K] b [K,N]: six bf16 MFMAs per 16-deep chunk, K ascending, one fp32 rounding per MFMA"""
    pa, pb = split3(a), split3(b)
    acc = np.zeros((a.shape[0], b.shape[1]), f32) if acc is None else acc
    for k0 in range(0, a.shape[1], 16):
        for i, j in ORDER:
            acc = (pa[i][:, k0:k0 + 16] @ pb[j][k0:k0 + 16] + acc).astype(f32)
    return acc


def smish(x):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t * torch.tanh(torch.log(1 + torch.sigmoid(t)))).numpy()


def block(sd, p, x, fold):
    """one residual block of layers 1-3 on x [n,6,6,cin] float32 -> [n,6,6,cout] float32"""
    s1, b1 = fold_bn(sd, p + ".conv1")
    s2, b2 = fold_bn(sd, p + ".conv2")
    sd_, bd = fold_bn(sd, p + ".downsample")
    U1, U2 = pack3x3(sd[p + ".conv1.0.weight"], s1), pack3x3(sd[p + ".conv2.0.weight"], s2)
    wd = sd[p + ".downsample.0.weight"]
    bias2 = (b2 + bd).astype(f32)
    Vx = wino_in(x)
    M1 = np.stack([gemm_bf16x6(Vx[z], U1[z]) for z in range(40)])
    h = smish((wino_out(M1) + b1).astype(f32))
    Vh = wino_in(h)
    if fold:
        Ud = pack_ds(wd, sd_)
        live = [z for z in range(40) if np.any(Ud[z])]
        assert len(live) == 18 and all(z // 5 not in (0, 7) and z % 5 in (1, 2, 3) for z in live), live
        M2 = np.stack([gemm_bf16x6(Vx[z], Ud[z], gemm_bf16x6(Vh[z], U2[z])) if z in live else gemm_bf16x6(Vh[z], U2[z])
                       for z in range(40)])
        y = (wino_out(M2) + bias2).astype(f32)
    else:
        M2 = np.stack([gemm_bf16x6(Vh[z], U2[z]) for z in range(40)])
        wds = (wd[:, :, 0, 0] * sd_[:, None]).astype(f32)
        r = gemm_bf16x6(x.reshape(-1, x.shape[-1]), np.ascontiguousarray(wds.T)).reshape(x.shape[:3] + (-1,))
        y = ((wino_out(M2) + bias2).astype(f32) + r).astype(f32)
    return smish(y)


def block64(sd64, p, x):
    return ols.residual_block(torch.from_numpy(x).double().permute(0, 3, 1, 2), sd64, p).permute(0, 2, 3, 1).numpy()


def relmax(a, ref):
    return float(np.abs(np.asarray(a, f64) - ref).max() / np.abs(ref).max())


def local_stage(sd, x, fold):
    """eval forward, x [n,3,21,21] float32 -> logits [n,10] float32"""
    F = torch.nn.functional
    t = ols.to_torch_sd(sd)
    with torch.no_grad():
        h = F.max_pool2d(ols.smish(ols.conv_bn(torch.from_numpy(x), t, "conv1", 3)), 3, 2, 1)
        h = F.max_pool2d(ols.residual_block(h, t, "layer0.0"), 3, 2, 1)
    h = np.ascontiguousarray(h.permute(0, 2, 3, 1).numpy())
    for p in ("layer1.0", "layer2.0", "layer3.0"):
        h = block(sd, p, h, fold)
    with torch.no_grad():
        h = F.max_pool2d(torch.from_numpy(h).permute(0, 3, 1, 2), 2, 2).flatten(1).numpy()         # (C,H,W) order
        s = (sd["fc.2.weight"] / np.sqrt(sd["fc.2.running_var"] + f32(ols.BN_EPS))).astype(f32)
        w = (sd["fc.1.weight"] * s[:, None]).astype(f32)
        b = ((sd["fc.1.bias"] - sd["fc.2.running_mean"]) * s + sd["fc.2.bias"]).astype(f32)
        f1 = smish((gemm_bf16x6(h, np.ascontiguousarray(w.T)) + b).astype(f32))
        return F.linear(torch.from_numpy(f1), t["fc.4.weight"], t["fc.4.bias"]).numpy()


def stressed(case):
    """tests/test_hip_parity.py: test_winograd_and_direct_logits_at_stressed_weights_vs_fp64_oracle"""
    S = 4242
    sd = synth.local_stage_state_dict(seed=S)
    bn = [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]
    convs = [k for k in sd if k.endswith(".0.weight") and sd[k].ndim == 4]
    if case in ("gamma", "all"):
        for p in bn:
            sd[p + ".weight"] = synth.f32(0.5 + 9.5 * synth.hash_uniform(S, p + ".stress_gamma", sd[p + ".weight"].shape))
    if case in ("running_var", "all"):
        for p in bn:
            sd[p + ".running_var"] = synth.f32(10.0 ** (-3.0 + 5.0 * synth.hash_uniform(S, p + ".stress_var", sd[p + ".running_var"].shape)))
    if case in ("weights_x8", "weights_x8_consistent_stats", "all"):
        for k in convs:
            sd[k] = synth.f32(8.0 * sd[k])
    if case == "weights_x8_consistent_stats":
        for p in bn:
            if p != "fc.2":
                sd[p + ".running_var"] = synth.f32(64.0 * sd[p + ".running_var"])
                sd[p + ".running_mean"] = synth.f32(8.0 * sd[p + ".running_mean"])
    return sd


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    cases = [("synthetic", synth.local_stage_state_dict(), synth.uniform_patches(16)[:n], 6e-6),
             ("synthetic seed 7", synth.local_stage_state_dict(seed=7), synth.uniform_patches(16)[:n], 1e-5)]
    for c in ("gamma", "running_var", "weights_x8", "weights_x8_consistent_stats", "all"):
        cases.append(("stressed " + c, stressed(c), synth.synthetic_patch_pairs(96, seed=78)[0][:n], 1e-5))
    ck = os.path.join(ROOT, "checkpoints", "pretrained_local_stage.pth")
    if os.path.exists(ck):
        sd = {k: v.numpy() for k, v in torch.load(ck, map_location="cpu").items()}
        cases.append(("trained checkpoint", sd, synth.synthetic_patch_pairs(96, seed=77)[0][:n], 1e-5))
    else:
        print("(no checkpoints/pretrained_local_stage.pth in this tree: the trained case is left out)")
    go = True
    for name, sd, x, bound in cases:
        sd = {k: np.asarray(v) for k, v in sd.items()}
        x = np.ascontiguousarray(x, dtype=f32)
        sd64 = ols.to_torch_sd(sd, torch.float64)
        taps = {}
        with torch.no_grad():
            ref = ols.local_stage_forward(sd64, torch.from_numpy(x).double(), taps=taps).numpy()
        for p, src in (("layer1.0", "pool2"), ("layer2.0", "layer1"), ("layer3.0", "layer2")):      # each block on its float64 input, rounded
            xin = np.ascontiguousarray(taps[src].permute(0, 2, 3, 1).numpy().astype(f32))
            with torch.no_grad():
                r64 = block64(sd64, p, xin)
            e = [relmax(block(sd, p, xin, fold), r64) for fold in (False, True)]
            go &= e[1] <= 1.5e-5
            print(f"{name:36s} block {p[:6]} {xin.shape[-1]:3d}->{r64.shape[-1]:3d}: separate {e[0]:.2e}  folded {e[1]:.2e}  (bound 1.5e-5)")
        e = [relmax(local_stage(sd, x, fold), ref) for fold in (False, True)]
        go &= e[1] <= bound
        print(f"{name:36s} logits vs float64: separate {e[0]:.2e}  folded {e[1]:.2e}  (bound {bound:.0e})")
    print("GO: the fold stays inside the project's bounds" if go else "NO-GO: the fold leaves the project's bounds")
    return 0 if go else 1


if __name__ == "__main__":
    sys.exit(main())
