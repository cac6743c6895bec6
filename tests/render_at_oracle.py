"""A numpy restatement of the lattice fold (be_fold_records_at_f32, be_fold_refocus_stack_at_f32) from a [P,32] record array, in
a chosen dtype.  A helper of test_render_at_cpu.py / test_render_at_gpu.py, not collected as a test.

It restates, from the record alone: the coverage rule (origin * k <= Y <= (origin + 20) * k), the patch-local coordinate
(lin[q], or lin[q] + (r / k) * (lin[q+1] - lin[q]) from the float32 `lin` values), the wedge distances
(utils/postprocessing_loss.py:26-30,43-86), the indicators (:91-95), the boundary value (blurry_edges_test.py:59-61), both depth
mask rules (:47-54), the fold with its divisions (utils/postprocessing_loss.py:151-173) and - for a focal stack - the refocus
radii through oracle.depth.depth2sigma.  test_render_at_cpu.py ties it to the pinned oracle (oracle.render.render_pass_b +
oracle.tiling.fold_mean) at scale 1.

Patches are visited rows then columns ascending, so in float32 every sample accumulates in the kernel's order.
"""
import numpy as np
import torch

R = 21
DELTA = 0.07                     # oracle.render.DELTA
# the record layout (csrc/be_render_full.hip): x0 y0 x1 y1 s11 c11 s12 c12 s21 c21 s22 c22 sg1 sg2 | rad img1 | rad img2 | rad refoc |
# colours [rgb][wedge] | depth1 depth2 | flags
R_RAD1, R_RAD2, R_RADF, R_COL, R_DEPTH, R_FLAGS = 14, 16, 18, 20, 29, 31
MAPS = ("image", "shpd", "refoc", "bndry", "depth", "conf")


def lin32():
    """The 21 patch coordinates as the reference builds them (float32 linspace, utils/postprocessing_loss.py:15-17)."""
    return torch.linspace(-1.0, 1.0, R).numpy()


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def axis_cover(origin, size_out, first, k):
    """Output samples of one axis covered by the patch at `origin`: (a, b, q, r) - samples a .. b-1 (empty when b <= a), and for
    each its position t = Y - origin * k = q * k + r inside the patch, 0 <= t <= 20 k."""
    Y = first * k + np.arange(size_out)
    ok = np.nonzero((origin * k <= Y) & (Y <= (origin + R - 1) * k))[0]
    if ok.size == 0:
        return 0, 0, ok, ok
    a, b = int(ok[0]), int(ok[-1]) + 1
    assert b - a == ok.size                                            # a contiguous run
    t = Y[a:b] - origin * k
    return a, b, t // k, t % k


def coord(lin, q, r, k, dt):
    """lin: the float32 table.  r == 0: lin[q] (read, lin[q+1] untouched); else lin[q] + (r / k) * (lin[q+1] - lin[q]) in dt."""
    l = lin.astype(dt)
    l0 = l[q]
    l1 = l[np.minimum(q + 1, R - 1)]                                   # r == 0 at q == 20: the value is not used
    frac = (r.astype(dt) / dt(k)).astype(dt)
    return np.where(r == 0, l0, (l0 + frac * (l1 - l0)).astype(dt)).astype(dt)


def _ray(px, py, vx, vy, s, c, w):
    dx, dy = px - vx, py - vy
    edge = -s * dx + c * dy
    axial = c * dx + s * dy
    far = np.sqrt(edge * edge + (axial * w) * (axial * w))
    return np.where(axial < 0, np.where(edge < 0, -far, far), edge)


def wedge_dists(g, px, py, w):
    """g: the record's first 14 values; px [1,n], py [m,1] -> (d1, d2) [m,n]."""
    x0, y0, x1, y1, s11, c11, s12, c12, s21, c21, s22, c22, sg1, sg2 = g
    d11, d12 = _ray(px, py, x0, y0, s11, c11, w), _ray(px, py, x0, y0, s12, c12, w)
    d21, d22 = _ray(px, py, x1, y1, s21, c21, w), _ray(px, py, x1, y1, s22, c22, w)
    in1 = np.where((sg1 * d11 > 0) & (sg1 * d12 < 0), sg1, -sg1)       # strict
    in2 = np.where((sg2 * d21 >= 0) & (sg2 * d22 <= 0), sg2, -sg2)     # closed
    return np.minimum(np.abs(d11), np.abs(d12)) * in1, np.minimum(np.abs(d21), np.abs(d22)) * in2


def indicators(d1, d2, r1, r2, dt):
    h1 = dt(0.5) * (dt(1) + _erf(d1 / r1))
    h2 = dt(0.5) * (dt(1) + _erf(d2 / r2))
    return (dt(1) - h1) * (dt(1) - h2), h1 * (dt(1) - h2), h2


def boundary_value(d1, d2, delta_sq):
    a1, a2 = np.abs(d1), np.abs(d2)
    db = np.where(d2 >= 0, d2, np.where(a1 < a2, a1, a2))
    return np.exp(-(db * db) / delta_sq)


def depth_mask(d1, d2, delta_sq, densify_w):
    if densify_w:
        return np.where(d2 > 0, 2, np.where(d1 > 0, 1, 0))
    m1 = np.exp(-(d1 * d1) / delta_sq) > 0.5
    m2 = np.exp(-(d2 * d2) / delta_sq) > 0.5
    return np.where(m2 | (d2 >= 0), np.where(m2, 2, 0), np.where(m1, 1, 0))


def fold_at(records, ys, xs, H, W, scale=1, window=None, dtype=np.float64, densify_w=False, w=1.0, rho_primes=None, consts=None,
            want=MAPS):
    """records [len(ys)*len(xs),32] (any float dtype; cast to `dtype`), patch (i, j) at pixel (ys[i], xs[j]) -> dict of the maps in
    `want` on the lattice (scale, window) in `dtype`; with rho_primes (and consts = oracle.depth.depth_consts()) also
    "stack" [K,3,Ho,Wo].  A sample under no patch is 0/0."""
    dt = np.dtype(dtype).type
    k = int(scale)
    top, left, h, wd = (0, 0, H, W) if window is None else window
    Ho, Wo = (h - 1) * k + 1, (wd - 1) * k + 1
    rec = np.asarray(records).astype(dt)
    HP, WP = len(ys), len(xs)
    assert rec.shape == (HP * WP, 32)
    lin = lin32()
    delta_sq = dt(DELTA ** 2)
    w = dt(w)
    rs = dt(np.sqrt(np.float32(2))) * dt(1e-4)                         # sharpened: eta = 1e-4, root2 the float32 value of sqrt(2)
    acc = dict(image=np.zeros((6, Ho, Wo), dt), shpd=np.zeros((3, Ho, Wo), dt), refoc=np.zeros((3, Ho, Wo), dt),
               bndry=np.zeros((Ho, Wo), dt), z=np.zeros((Ho, Wo), dt))
    cnt, cntz = np.zeros((Ho, Wo), np.int64), np.zeros((Ho, Wo), np.int64)
    K = 0 if rho_primes is None else len(rho_primes)
    stack = np.zeros((K, 3, Ho, Wo), dt)
    if K:
        from oracle import depth as od
        root2 = dt(np.sqrt(np.float32(2)))
        T = lambda a: torch.from_numpy(np.asarray(a, dtype=dt))
        flags = rec[:, R_FLAGS].astype(np.int64)
        # [K,P,2] refocus radii: sqrt2 * depth2sigma(z, rho') where the wedge owns a mask pixel, sqrt2 * 1e-4 where it does not
        radf = np.stack([np.stack([np.where(flags & (1 << m), od.depth2sigma(consts, T(rec[:, R_DEPTH + m]), float(rho)).numpy().astype(dt),
                                            dt(1e-4)) for m in (0, 1)], axis=1) for rho in rho_primes]).astype(dt) * root2
    ycov = [axis_cover(o, Ho, top, k) for o in ys]
    xcov = [axis_cover(o, Wo, left, k) for o in xs]
    xcoord = [coord(lin, q, r, k, dt)[None, :] if b > a else None for a, b, q, r in xcov]
    want_z = "depth" in want or "conf" in want
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i, (ya, yb, yq, yr) in enumerate(ycov):
            if yb <= ya:
                continue
            py = coord(lin, yq, yr, k, dt)[:, None]
            for j, (xa, xb, _, _) in enumerate(xcov):
                if xb <= xa:
                    continue
                r = rec[i * WP + j]
                d1, d2 = wedge_dists(r[:14], xcoord[j], py, w)
                col = r[R_COL:R_COL + 9].reshape(3, 3)                 # [rgb][wedge]
                sl = (slice(ya, yb), slice(xa, xb))

                def comp(r1, r2):
                    u0, u1, u2 = indicators(d1, d2, r1, r2, dt)
                    return np.stack([u0 * col[c, 0] + u1 * col[c, 1] + u2 * col[c, 2] for c in range(3)])
                if "image" in want:
                    acc["image"][(slice(0, 3),) + sl] += comp(r[R_RAD1], r[R_RAD1 + 1])
                    acc["image"][(slice(3, 6),) + sl] += comp(r[R_RAD2], r[R_RAD2 + 1])
                if "shpd" in want:
                    acc["shpd"][(slice(None),) + sl] += comp(rs, rs)
                if "refoc" in want:
                    acc["refoc"][(slice(None),) + sl] += comp(r[R_RADF], r[R_RADF + 1])
                if "bndry" in want:
                    acc["bndry"][sl] += boundary_value(d1, d2, delta_sq)
                if want_z:
                    m = depth_mask(d1, d2, delta_sq, densify_w)
                    acc["z"][sl] += np.where(m == 1, r[R_DEPTH], np.where(m == 2, r[R_DEPTH + 1], dt(0)))
                    cntz[sl] += m > 0
                for p in range(K):
                    stack[(p, slice(None)) + sl] += comp(radf[p, i * WP + j, 0], radf[p, i * WP + j, 1])
                cnt[sl] += 1
        n = cnt.astype(dt)
        out = {}
        if "image" in want:
            out["image"] = (acc["image"] / n).reshape(2, 3, Ho, Wo)
        for key in ("shpd", "refoc", "bndry"):
            if key in want:
                out[key] = acc[key] / n
        if "depth" in want:
            out["depth"] = acc["z"] / np.where(cntz > 0, cntz, 1).astype(dt)
        if "conf" in want:
            out["conf"] = cntz.astype(dt) / n
        if K:
            out["stack"] = stack / n
    out["count"] = cnt
    return out
