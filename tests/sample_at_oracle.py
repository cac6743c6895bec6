"""A numpy restatement of the point fold (be_fold_records_points_f32, be_fold_refocus_stack_points_f32) from a [P,32] record array,
in a chosen dtype, in GATHER form: for every point, the run of covering patches is found and visited rows then columns
ascending - the kernel's loop - where tests/render_at_oracle.py scatters every patch over the lattice samples it covers.  A
helper of test_sample_at_cpu.py / test_sample_at_gpu.py, not collected as a test.

The wedge distances, indicators, boundary value, depth masks and the `lin` table are the pieces of render_at_oracle; what is
restated here is the covering rule at a real position (yq = floor(y), f = y - yq, origins in [yq + (f > 0) - 20, yq]), the
coordinate lin[q] (f == 0) or lin[q] + f * (lin[q+1] - lin[q]), the closed domain and the division by the patches visited.
test_sample_at_cpu.py ties it to render_at_oracle.fold_at (and so to the pinned oracle) on a k = 4 window, difference exactly 0.
"""
import numpy as np
import torch

import render_at_oracle as rao

R = rao.R
MAPS = rao.MAPS


def random_points(H, W, n, seed):
    """n seeded positions, uniform over the closed domain [0, H-1] x [0, W-1], float32 [n,2] (y, x)."""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2)) * np.array([H - 1, W - 1], np.float64)
    return np.minimum(pts.astype(np.float32), np.array([H - 1, W - 1], np.float32))


def lattice_points(k, window):
    """The lattice of render_at as positions: float32 [Ho,Wo,2], sample (iy, ix) at (top + iy / k, left + ix / k)."""
    top, left, h, w = window
    y = (top + np.arange((h - 1) * k + 1, dtype=np.float64) / k).astype(np.float32)
    x = (left + np.arange((w - 1) * k + 1, dtype=np.float64) / k).astype(np.float32)
    return np.stack(np.broadcast_arrays(y[:, None], x[None, :]), axis=-1).copy()


def valid_points(points, H, W):
    """The kernel's predicate in float32: inside the closed domain; NaN and the infinities are outside."""
    p = np.asarray(points, np.float32)
    with np.errstate(invalid="ignore"):
        return (p[..., 0] >= 0) & (p[..., 0] <= np.float32(H - 1)) & (p[..., 1] >= 0) & (p[..., 1] <= np.float32(W - 1))


def _axis(origins, v):
    """v float32 [n] inside the domain -> (q0 = floor, f float32 = v - q0 exactly, lo, hi): origins[lo..hi] cover v."""
    o = np.asarray(origins, np.int64)
    q0 = np.floor(v).astype(np.int64)
    f = v - q0.astype(np.float32)
    assert f.dtype == np.float32 and np.array_equal(q0.astype(np.float64) + f.astype(np.float64), v.astype(np.float64))
    first = q0 + (f > 0) - (R - 1)
    return q0, f, np.searchsorted(o, first, side="left"), np.searchsorted(o, q0, side="right") - 1


def _coord(lin, q, f, dt):
    l0 = lin[q]
    l1 = lin[np.minimum(q + 1, R - 1)]                                 # f == 0 at q == 20: the value is not used
    return np.where(f == 0, l0, (l0 + f * (l1 - l0)).astype(dt)).astype(dt)


def fold_points(records, ys, xs, H, W, points, dtype=np.float64, densify_w=False, w=1.0, rho_primes=None, consts=None, want=MAPS,
                chunk=65536):
    """records [len(ys)*len(xs),32] (cast to `dtype`), patch (i, j) at pixel (ys[i], xs[j]); points [...,2] float32 (y, x) -> dict
    of the maps in `want` in `dtype`, channel-major with the points' leading shape (image [2,3,*lead]); with rho_primes (and
    consts = oracle.depth.depth_consts()) also "stack" [K,3,*lead]; "count" [*lead] the patches visited and "valid" [*lead].
    A point outside the domain has 0 everywhere; a point inside under no patch is 0/0."""
    dt = np.dtype(dtype).type
    pts = np.asarray(points)
    assert pts.dtype == np.float32 and pts.shape[-1] == 2
    lead = pts.shape[:-1]
    pts = pts.reshape(-1, 2)
    N = pts.shape[0]
    rec = np.asarray(records).astype(dt)
    HP, WP = len(ys), len(xs)
    assert rec.shape == (HP * WP, 32)
    K = 0 if rho_primes is None else len(rho_primes)
    radf = None
    if K:
        from oracle import depth as od
        root2 = dt(np.sqrt(np.float32(2)))
        T = lambda a: torch.from_numpy(np.asarray(a, dtype=dt))
        flags = rec[:, rao.R_FLAGS].astype(np.int64)
        radf = np.stack([np.stack([np.where(flags & (1 << m), od.depth2sigma(consts, T(rec[:, rao.R_DEPTH + m]), float(rho)).numpy().astype(dt),
                                            dt(1e-4)) for m in (0, 1)], axis=1) for rho in rho_primes]).astype(dt) * root2
    valid = valid_points(pts, H, W)
    res = dict(image=np.zeros((6, N), dt), shpd=np.zeros((3, N), dt), refoc=np.zeros((3, N), dt), bndry=np.zeros(N, dt),
               depth=np.zeros(N, dt), conf=np.zeros(N, dt), stack=np.zeros((K, 3, N), dt), count=np.zeros(N, np.int64))
    idx = np.nonzero(valid)[0]
    for c0 in range(0, idx.size, chunk):
        sel = idx[c0:c0 + chunk]
        part = _fold_valid(rec, np.asarray(ys, np.int64), np.asarray(xs, np.int64), pts[sel], dt, densify_w, dt(w), radf, want)
        for k, v in part.items():
            res[k][..., sel] = v
    out = {k: res[k].reshape(res[k].shape[:-1] + lead) for k in MAPS if k in want}
    if "image" in out:
        out["image"] = out["image"].reshape((2, 3) + lead)
    if K:
        out["stack"] = res["stack"].reshape((K, 3) + lead)
    out["count"], out["valid"] = res["count"].reshape(lead), valid.reshape(lead)
    return out


def _fold_valid(rec, ys, xs, pts, dt, densify_w, w, radf, want):
    n = pts.shape[0]
    WP = len(xs)
    lin = rao.lin32().astype(dt)
    delta_sq = dt(rao.DELTA ** 2)
    rs = dt(np.sqrt(np.float32(2))) * dt(1e-4)
    yq, fy, ilo, ihi = _axis(ys, pts[:, 0])
    xq, fx, jlo, jhi = _axis(xs, pts[:, 1])
    fy, fx = fy.astype(dt), fx.astype(dt)
    K = 0 if radf is None else radf.shape[0]
    acc = dict(image=np.zeros((6, n), dt), shpd=np.zeros((3, n), dt), refoc=np.zeros((3, n), dt), bndry=np.zeros(n, dt), z=np.zeros(n, dt),
               stack=np.zeros((K, 3, n), dt))
    cnt, cntz = np.zeros(n, np.int64), np.zeros(n, np.int64)
    want_z = "depth" in want or "conf" in want
    zero = dt(0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for di in range(int((ihi - ilo).max()) + 1 if n else 0):
            i = ilo + di
            on_i = i <= ihi
            ic = np.minimum(i, len(ys) - 1)
            py = _coord(lin, np.clip(yq - ys[ic], 0, R - 1), fy, dt)
            for dj in range(int((jhi - jlo).max()) + 1):
                j = jlo + dj
                on = on_i & (j <= jhi)
                if not on.any():
                    continue
                jc = np.minimum(j, WP - 1)
                px = _coord(lin, np.clip(xq - xs[jc], 0, R - 1), fx, dt)
                p = ic * WP + jc
                r = rec[p]                                             # [n,32]
                d1, d2 = rao.wedge_dists(tuple(r[:, c] for c in range(14)), px, py, w)
                col = r[:, rao.R_COL:rao.R_COL + 9].reshape(n, 3, 3)   # [rgb][wedge]

                def comp(r1, r2):
                    u0, u1, u2 = rao.indicators(d1, d2, r1, r2, dt)
                    return np.where(on, np.stack([u0 * col[:, c, 0] + u1 * col[:, c, 1] + u2 * col[:, c, 2] for c in range(3)]), zero)
                if "image" in want:
                    acc["image"][0:3] += comp(r[:, rao.R_RAD1], r[:, rao.R_RAD1 + 1])
                    acc["image"][3:6] += comp(r[:, rao.R_RAD2], r[:, rao.R_RAD2 + 1])
                if "shpd" in want:
                    acc["shpd"] += comp(rs, rs)
                if "refoc" in want:
                    acc["refoc"] += comp(r[:, rao.R_RADF], r[:, rao.R_RADF + 1])
                if "bndry" in want:
                    acc["bndry"] += np.where(on, rao.boundary_value(d1, d2, delta_sq), zero)
                if want_z:
                    m = np.where(on, rao.depth_mask(d1, d2, delta_sq, densify_w), 0)
                    acc["z"] += np.where(m == 1, r[:, rao.R_DEPTH], np.where(m == 2, r[:, rao.R_DEPTH + 1], zero))
                    cntz += m > 0
                for k in range(K):
                    acc["stack"][k] += comp(radf[k, p, 0], radf[k, p, 1])
                cnt += on
        nn = cnt.astype(dt)
        out = dict(count=cnt)
        for key in ("image", "shpd", "refoc", "bndry"):
            if key in want:
                out[key] = acc[key] / nn
        if "depth" in want:
            out["depth"] = acc["z"] / np.where(cntz > 0, cntz, 1).astype(dt)
        if "conf" in want:
            out["conf"] = cntz.astype(dt) / nn
        if K:
            out["stack"] = acc["stack"] / nn
    return out
