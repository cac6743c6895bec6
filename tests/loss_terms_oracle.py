"""Float64 per-patch, per-term references of the two fused loss kernels (be_local_loss_f32, be_global_loss_f32), with the seeded
inputs their tests share.  A helper of test_loss_terms_cpu.py / test_local_loss_terms_gpu.py / test_global_loss_terms_gpu.py, not
collected as a test.

Both references are built from the oracle's primitives (oracle.render: params2dists, params2etas, dists2indicators, ridge_colors,
composite, boundary_map, image_derivative, depth_mask; oracle.depth.etas2depth; oracle.global_loss.restore_params;
oracle.tiling.unfold_patches) under torch autograd in float64, on the float32 inputs cast up.  They return what the kernels keep
apart and the trusted oracles (oracle.render.local_loss, oracle.global_loss.global_loss) only return summed: one value per patch
and per term, and one gradient tensor per term.  test_loss_terms_cpu.py ties their weighted sums to the two trusted oracles.

The global reference takes the folded maps G, Gd, Gb as INPUTS (the reference detaches them and the kernel reads them as data);
`folded_maps` computes them the way oracle.global_loss does, for the tie and for the host-side test.

Every hard decision the kernels and the oracle take on float64 values is listed by `near_*`: a patch with a pixel or parameter
within NEAR of such a threshold may be left out of the per-patch comparisons (never more than MAX_EXCLUDED of a case).
"""
import math

import numpy as np
import torch

from oracle import depth as odepth, global_loss as ogl, render as orr, tiling as ot

NEAR = 1e-6
MAX_EXCLUDED = 0.01
LOCAL_TERMS = ("color", "bndry_loc", "smthns")                                                    # columns of the local partial [n,3]
GLOBAL_TERMS = ("color", "color_cons", "bndry_cons", "smthns", "smthns_cons", "bndry_loc")       # columns 0..5 of the global [B*P,8]
COL_DEPTH, COL_COUNT = 6, 7                                                                       # depth numerator, mask count
N_LOCAL = 1031
LOCAL_SIZES_WORKGROUP = (1, 3, 64, 1024)          # k_local_loss<WAVES>: a workgroup per patch
LOCAL_SIZES_WAVE = (1025, 1026, 1027, 1031)       # k_local_loss<1>: a wave per patch; last workgroups with 1, 2, 3, 3 live waves
# name -> (B, H, W, stride): hp x wp = 3 x 5 and 3 x 2
GLOBAL_CASES = {"b3_25x29_s2": (3, 25, 29, 2), "b2_27x24_s3": (2, 27, 24, 3)}
HOST_CASE = (2, 33, 35, 2)                        # utils.global_loss through autograd: 7 x 8 patches per image
GAMMA_DISTINCT6 = (0.1, 0.05, 0.02, 0.002, 0.003, 0.0001)
GAMMA_DISTINCT7 = dict(color=0.1, color_cons=0.05, bndry_cons=0.02, smthns=0.002, smthns_cons=0.003, bndry_loc=0.0001, depth=0.5)


def D(a):
    """float64 CPU tensor of an array or tensor"""
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double()
    return torch.from_numpy(np.asarray(a)).double()


def term_bound(ref):
    """The per-patch bound of one term: 1e-5 |ref| + 1e-6 (largest per-patch value of that term in the case).  The floor is there
    for the boundary terms: exp(-d^2 / delta^2) reaches 1e-63 in some patches, where a float32 exponential has no relative accuracy."""
    ref = np.asarray(ref, dtype=np.float64)
    return 1e-5 * np.abs(ref) + 1e-6 * np.max(np.abs(ref))


# ------------------------------------------------------------------------------------------------ decisions near their threshold
def near_distance_branch(dists):
    """[N] bool: a pixel within NEAR of `d2 >= 0` or, where that falls to the other side, of `|d1| < |d2|` (boundary_distance)"""
    d1, d2 = dists[:, 0], dists[:, 1]
    hit = (d2.abs() < NEAR) | ((d2 < NEAR) & ((d1.abs() - d2.abs()).abs() < NEAR))
    return hit.flatten(1).any(dim=1)


def near_angle_branch(phi):
    """phi [N,2] wrapped to [0, 2 pi): within NEAR of where `phi < pi` changes (pi, and the wrap at 0 / 2 pi)"""
    hit = ((phi - math.pi).abs() < NEAR) | (phi < NEAR) | (2 * math.pi - phi < NEAR)
    return hit.any(dim=1)


def near_mask_threshold(dists):
    """[N] bool: a pixel whose normalized_gaussian(d1) or (d2) is within NEAR of the 0.5 of depth_mask"""
    return ((orr.normalized_gaussian(dists) - 0.5).abs() < NEAR).flatten(1).any(dim=1)


def depth_branch_values(c, eta1, eta2):
    """c1, c2, c3 of oracle.depth.etas2depth (utils/depth_etas.py:23-28) stacked on the last axis"""
    I = c.intercept
    return torch.stack([-c.sin_w * eta1 + c.cos_w * (eta2 - I), -c.sin_m * (eta1 - I) + c.cos_m * eta2,
                        -c.sin_w * (eta1 - I) + c.cos_w * eta2], dim=-1)


def near_depth_branch(c, etas):
    """etas [N,4]: c1, c2 or c3 of either wedge depth within NEAR of 0"""
    v = torch.cat([depth_branch_values(c, etas[:, 0], etas[:, 2]), depth_branch_values(c, etas[:, 1], etas[:, 3])], dim=1)
    return (v.abs() < NEAR).any(dim=1)


# ------------------------------------------------------------------------------------------------ local loss
def local_inputs(n=N_LOCAL):
    """One seeded set of patches; a smaller case takes its first rows.  float32 numpy arrays in the kernel's layouts."""
    from be_hip import synth
    S = synth.SEED_DEFAULT
    u = lambda name, shape: synth.hash_uniform(S, name, shape)
    return dict(est=synth.plausible_params10(N_LOCAL, name="loss_terms_params")[:n],
                img_fit=synth.f32(u("terms_img", (N_LOCAL, 21, 21, 3)))[:n], gt=synth.f32(u("terms_gt", (N_LOCAL, 21, 21, 3)))[:n],
                bdist=synth.f32(5.0 * u("terms_bd", (N_LOCAL, 21, 21)))[:n], deri=synth.f32(u("terms_deri", (N_LOCAL, 19, 19, 3)))[:n])


def local_reference(est, img_fit, gt, bdist, deri, inverse="cayley"):
    """est [n,10], img_fit / gt [n,21,21,3], bdist [n,21,21], deri [n,19,19,3] (local_training.py:32-52) ->
    partial [n,3]: sum_px sum_c (gt - patch)^2, sum_px (bdist B)^2, sum_q sum_c (deri - Sobel(patch))^2, un-weighted;
    grads: three [n,10], d (sum over patches of term k) / d est; patches [n,3,21,21]; boundary [n,21,21];
    near [n]: a decision of the patch is within NEAR of its threshold."""
    est = D(est).requires_grad_(True)
    img_fit, gt, bdist, deri = D(img_fit), D(gt), D(bdist), D(deri)
    p = torch.cat([est[:, :4], torch.remainder(est[:, 4:8], 2 * torch.pi), est[:, 8:]], dim=1)
    dists = orr.params2dists(p[:, :8])
    wedges = orr.dists2indicators(dists, orr.params2etas(p[:, 8:10]))
    colors, _, _ = orr.ridge_colors([wedges], [img_fit.permute(0, 3, 1, 2)], inverse=inverse)
    patches = orr.composite(wedges, colors)
    bnd = orr.boundary_map(dists)
    partial = torch.stack([((gt - patches.permute(0, 2, 3, 1)) ** 2).sum(dim=(1, 2, 3)),
                           ((bdist * bnd) ** 2).sum(dim=(1, 2)),
                           ((deri.permute(0, 3, 1, 2) - orr.image_derivative(patches)) ** 2).sum(dim=(1, 2, 3))], dim=1)
    grads = [torch.autograd.grad(partial[:, k].sum(), est, retain_graph=True)[0] for k in range(3)]
    near = near_distance_branch(dists.detach()) | near_angle_branch(p.detach()[:, [5, 7]])
    return dict(partial=partial.detach(), grads=grads, patches=patches.detach(), boundary=bnd.detach(), near=near)


def local_loss_from_partial(partial, beta_b, beta_s):
    """the documented weights: S0 / (441 n) + beta_b S1 / (441 n) + beta_s S2 / (361 n)"""
    n = partial.shape[0]
    s = D(partial).sum(dim=0)
    return s[0] / (441 * n) + beta_b * s[1] / (441 * n) + beta_s * s[2] / (361 * n)


def local_weighted_grad(grads, beta_b, beta_s):
    """what `grad * n * 441` of the kernel holds: g0 + beta_b g1 + beta_s (441 / 361) g2"""
    return grads[0] + beta_b * grads[1] + beta_s * (441.0 / 361.0) * grads[2]


def balanced_betas(grads):
    """(beta_b, beta_s), rounded to float32 as the kernel's arguments are, that give the three weighted per-term gradient tensors
    the same L-inf norm: no chain contributes less than a third of the total's scale."""
    a0, a1, a2 = (float(g.abs().max()) for g in grads)
    return float(np.float32(a0 / a1)), float(np.float32(a0 * 361.0 / (441.0 * a2)))


# ------------------------------------------------------------------------------------------------ global loss
def global_inputs(B, H, W, stride, name):
    """Seeded inputs of one global case, different data per image, float32 numpy arrays in the kernel's layouts.  G, Gd, Gb are
    independent streams (NOT the fold of this est): the consistency terms then share nothing with the colour terms.  bdepth is
    non-zero on about half the pixels.  est is synth.plausible_global_output with the four eta columns doubled: the wider spread
    of blur radii is what brings all four etas2depth branches into the 24 wedge depths of the smaller case."""
    from be_hip import synth
    S = synth.SEED_DEFAULT
    hp, wp = ot.grid_dims(H, W, stride)
    P = hp * wp
    u = lambda tag, shape: synth.hash_uniform(S, name + "." + tag, shape)
    est = synth.plausible_global_output(B * P, name=name + ".est").reshape(B, P, 12).copy()
    est[..., 8:] *= 2.0
    z = 0.75 + 0.43 * u("bdepth", (B, H, W))
    return dict(est=est, img_fit=synth.f32(u("img_fit", (B, 2, H, W, 3))), img_gt=synth.f32(u("img_gt", (B, 2, H, W, 3))),
                G=synth.f32(u("G", (B, 2, 3, H, W))), Gd=synth.f32(2.0 * u("Gd", (B, 2, 3, H - 2, W - 2))),
                Gb=synth.f32(u("Gb", (B, H, W))), bdist=synth.f32(5.0 * u("bdist", (B, H, W))),
                deri=synth.f32(u("deri", (B, 2, H - 2, W - 2, 3))),
                bdepth=synth.f32(np.where(u("bdepth_on", (B, H, W)) < 0.5, z, 0.0)), hp=hp, wp=wp, stride=stride)


def _render_image(est_b, img_fit_b, stride, inverse):
    """one image of the batch: (dists [P,2,21,21], etas [P,4], pat [2,P,3,21,21], bnd [P,21,21]), as oracle.global_loss:33-41"""
    p8, etas = ogl.restore_params(est_b)
    dists = orr.params2dists(p8)
    w1 = orr.dists2indicators(dists, etas[:, 0:2])
    w2 = orr.dists2indicators(dists, etas[:, 2:4])
    fit = ot.unfold_patches(img_fit_b.permute(0, 3, 1, 2), stride)
    colors, _, _ = orr.ridge_colors([w1, w2], [fit[0], fit[1]], inverse=inverse)
    return p8, dists, etas, torch.stack([orr.composite(w1, colors), orr.composite(w2, colors)]), orr.boundary_map(dists)


def folded_maps(est, img_fit, stride, inverse="cayley"):
    """G [B,2,3,H,W], Gd [B,2,3,H-2,W-2], Gb [B,H,W] of the current estimate, as oracle.global_loss:42-43,49 computes them"""
    est, img_fit = D(est), D(img_fit)
    H, W = img_fit.shape[2:4]
    G, Gb = [], []
    for b in range(est.shape[0]):
        _, _, _, pat, bnd = _render_image(est[b], img_fit[b], stride, inverse)
        G.append(ot.fold_mean(pat, H, W, stride))
        Gb.append(ot.fold_mean(bnd[None, :, None], H, W, stride)[0, 0])
    G = torch.stack(G)
    return G, torch.stack([orr.image_derivative(g) for g in G]), torch.stack(Gb)


def global_reference(c, est, img_fit, img_gt, G, Gd, Gb, bdist, deri, bdepth, stride, inverse="cayley"):
    """The kernel's contract in float64.  est [B,P,12]; img_fit / img_gt [B,2,H,W,3]; G [B,2,3,H,W]; Gd [B,2,3,H-2,W-2]; Gb, bdist,
    bdepth [B,H,W]; deri [B,2,H-2,W-2,3]; c: oracle.depth.depth_consts() ->
    partial [B*P,8] in the kernel's order (GLOBAL_TERMS, depth numerator, mask count), all un-normalised sums over the patch;
    grads: six [B,P,12], d (sum over patches of term k) / d est; gdepth [B*P,4]: d (depth numerator) / d est[..., 8:12];
    branch [B*P,2] (etas2depth branch 0..3 of the two wedge depths), mask [B*P,21,21], sg [B*P,2] (+1 where phi < pi), near [B*P]."""
    est = D(est).requires_grad_(True)
    img_fit, img_gt, G, Gd, Gb, bdist, deri, bdepth = (D(t) for t in (img_fit, img_gt, G, Gd, Gb, bdist, deri, bdepth))
    B, P = est.shape[:2]
    recs, branch, mask, sg, near = [], [], [], [], []
    for b in range(B):
        p8, dists, etas, pat, bnd = _render_image(est[b], img_fit[b], stride, inverse)
        gtp = ot.unfold_patches(img_gt[b].permute(0, 3, 1, 2), stride)                 # [2,P,3,21,21]
        Gp = ot.unfold_patches(G[b], stride)
        Gbp = ot.unfold_patches(Gb[b][None, None], stride)[0, :, 0]                     # [P,21,21]
        pd = orr.image_derivative(pat.reshape(2 * P, 3, 21, 21)).reshape(2, P, 3, 19, 19)
        dgt = ot.unfold_patches(deri[b].permute(0, 3, 1, 2), stride, r=19)
        dG = ot.unfold_patches(Gd[b], stride, r=19)
        lb = ot.unfold_patches(torch.log2(bdist[b] + 1)[None, None], stride)[0, :, 0]
        mk = orr.depth_mask(dists)
        z1, br1 = odepth.etas2depth(c, etas[:, 0], etas[:, 2], return_branch=True)
        z2, br2 = odepth.etas2depth(c, etas[:, 1], etas[:, 3], return_branch=True)
        zmap = torch.where(mk == 1, z1[:, None, None], torch.where(mk == 2, z2[:, None, None], mk.to(z1.dtype)))
        bdp = ot.unfold_patches(bdepth[b][None, None], stride)[0, :, 0]
        m = ((bdp != 0) & (mk != 0)).to(z1.dtype)
        recs.append(torch.stack([((gtp - pat) ** 2).sum(dim=(0, 2, 3, 4)), ((pat - Gp) ** 2).sum(dim=(0, 2, 3, 4)),
                                 ((bnd - Gbp) ** 2).sum(dim=(1, 2)), ((pd - dgt) ** 2).sum(dim=(0, 2, 3, 4)),
                                 ((pd - dG) ** 2).sum(dim=(0, 2, 3, 4)), ((lb * bnd) ** 2).sum(dim=(1, 2)),
                                 (((zmap - bdp) * m) ** 2).sum(dim=(1, 2)), m.sum(dim=(1, 2))], dim=1))
        phi = p8.detach()[:, [5, 7]]
        branch.append(torch.stack([br1, br2], dim=1))
        mask.append(mk)
        sg.append(torch.where(phi < math.pi, 1, -1))
        near.append(near_distance_branch(dists.detach()) | near_angle_branch(phi) | near_mask_threshold(dists.detach())
                    | near_depth_branch(c, etas.detach()))
    partial = torch.cat(recs)
    grads = [torch.autograd.grad(partial[:, k].sum(), est, retain_graph=True)[0] for k in range(6)]
    gdepth = torch.autograd.grad(partial[:, COL_DEPTH].sum(), est)[0][..., 8:12].reshape(B * P, 4)
    return dict(partial=partial.detach(), grads=grads, gdepth=gdepth, branch=torch.cat(branch), mask=torch.cat(mask), sg=torch.cat(sg),
                near=torch.cat(near))


def global_normalisers(B, P):
    """n_k of GLOBAL_TERMS: color / color_cons over 2 apertures x 441 pixels, bndry_* over 441, smthns* over 2 x 361"""
    n1, n3, n4 = B * 2 * 441 * P, B * 441 * P, B * 2 * 361 * P
    return (n1, n1, n3, n4, n4, n3)


def global_loss_from_partial(partial, gamma, B, P):
    """(loss, terms) from the per-patch record and a gamma dict, the combination of oracle.global_loss:62-66"""
    t = D(partial).sum(dim=0)
    terms = {k: t[i] / n for i, (k, n) in enumerate(zip(GLOBAL_TERMS, global_normalisers(B, P)))}
    terms["depth"] = t[COL_DEPTH] / t[COL_COUNT]
    return sum(gamma[k] * terms[k] for k in terms), terms


def check_branch_coverage(ref):
    """The conditions on the inputs of a global case, in the float64 reference: all four etas2depth branches among the 2 B P wedge
    depths, mask values 0, 1, 2, a patch with mask count 0 and one above, both signs of sg1 and of sg2."""
    assert set(ref["branch"].flatten().tolist()) == {0, 1, 2, 3}, "an etas2depth branch is not visited"
    assert set(ref["mask"].flatten().tolist()) == {0, 1, 2}, "a depth-mask value does not occur"
    ms = ref["partial"][:, COL_COUNT]
    assert bool((ms == 0).any()) and bool((ms > 0).any()), "no patch with an empty depth mask, or none with a live one"
    for w in range(2):
        assert set(ref["sg"][:, w].tolist()) == {1, -1}, f"sg{w + 1} takes one sign only"


def kept_patches(near):
    """indices of the patches that the per-patch comparisons keep; at most MAX_EXCLUDED of a case may be left out"""
    near = np.asarray(near, dtype=bool)
    assert near.mean() <= MAX_EXCLUDED, f"{int(near.sum())} of {near.size} patches are within {NEAR} of a branch threshold"
    return np.nonzero(~near)[0]
