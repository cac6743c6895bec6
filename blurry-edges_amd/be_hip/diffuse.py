"""Host statement of the diffusion depth completion (native.fill_diffuse, DepthPipeline.complete(method="diffuse")): the edge-aware
harmonic fill of the holes of a sparse depth map.  Pure numpy (scipy for the sparse direct solve when it is installed); nothing
here needs a GPU.

The problem.  Seeds are fill.seeds_of(depth, weight); a seed's boundary value b is what fill_nearest copies from it
(its depth at smooth = 0, fill.local_mean at smooth > 0).  With e = min(max(edge, 0), 1) (NaN: 0; edge None: 0) the conductance
between 4-neighbours p, q is c_pq = max(leak, 1 - max(e_p, e_q)); the image border has no neighbour and no term (Neumann).  Every
hole satisfies u_p sum_q c_pq = sum_q c_pq u_q, a neighbouring seed contributing b.  solve_exact is that system solved directly in
float64; fill_diffuse is the pyramid and the red-black sweeps of be_diffuse.hip restated operation by operation (same levels, tiles,
sweeps and order; float32 with one rounding per written operation, as the kernels are compiled without contraction)."""
from __future__ import annotations

import math

import numpy as np

from . import fill

_F = np.float32
TILE, HALO = 96, 16                 # a workgroup relaxes a region of up to 128 x 128: its 96 x 96 tile and 16 more on every side
REGION = TILE + 2 * HALO            # a level of at most 128 x 128 is one region
COARSEST = 4                        # the pyramid stops when the longer side is <= 4
SWEEPS_PER_LAUNCH = 16              # on a level of several tiles: the halo is refreshed every 16 sweeps
MAX_ITERS = 4096
DENSE_MAX_HOLES = 4096              # solve_exact without scipy


# ------------------------------------------------------------------------------------------ the problem
def clamp_edge(edge, H, W):
    """e [H,W] float32 = min(max(edge, 0), 1), NaN -> 0; edge None -> 0."""
    if edge is None:
        return np.zeros((H, W), _F)
    e = np.asarray(edge)
    if e.shape != (H, W):
        raise ValueError(f"diffuse: edge must be [{H},{W}], got {e.shape}")
    e = e.astype(_F)
    with np.errstate(invalid="ignore"):
        return np.where(e > 0, np.minimum(e, _F(1)), _F(0)).astype(_F)      # NaN and negatives fail e > 0


def _check_leak(leak, who):
    try:
        leak = float(leak)
    except (TypeError, ValueError):
        leak = -1.0
    if not 0 < leak <= 1:
        raise ValueError(f"{who}: leak must be a number in (0, 1], got {leak!r}")
    return _F(leak)


def _links(e, leak):
    """e [H,W] float32 -> (ce, cs) float32 [H,W]: the conductance to the east and south neighbour, 0 where there is none."""
    H, W = e.shape
    ce, cs = np.zeros((H, W), _F), np.zeros((H, W), _F)
    ce[:, :-1] = np.maximum(leak, _F(1) - np.maximum(e[:, :-1], e[:, 1:]))
    cs[:-1, :] = np.maximum(leak, _F(1) - np.maximum(e[:-1, :], e[1:, :]))
    return ce, cs


def conductances(edge, H, W, leak=1e-3):
    """-> (ce, cs) float32 [H,W]: c_pq = max(leak, 1 - max(e_p, e_q)) towards the east and the south neighbour, 0 on the last column
    / row, where there is no such neighbour."""
    return _links(clamp_edge(edge, H, W), _check_leak(leak, "conductances"))


def _problem(depth, weight, edge, smooth, sigma_z, leak, who):
    """The argument checks shared by solve_exact and fill_diffuse -> (near: fill.fill_nearest_f32's result, b [H,W] float32: the
    boundary values (0 off the seeds), e [H,W] float32, leak float32)."""
    if isinstance(smooth, bool) or int(smooth) != smooth or not 0 <= smooth <= fill.MAX_SMOOTH:
        raise ValueError(f"{who}: smooth must be an integer in [0, {fill.MAX_SMOOTH}], got {smooth!r}")
    if not 0 < float(sigma_z) < float("inf"):
        raise ValueError(f"{who}: sigma_z must be a finite number > 0")
    leak = _check_leak(leak, who)
    near = fill.fill_nearest_f32(depth, weight, int(smooth), sigma_z)
    H, W = near["depth"].shape
    e = clamp_edge(edge, H, W)
    seeds = near["seeds"]
    z = np.asarray(depth, _F)
    b = fill.local_mean(depth, weight, seeds, int(smooth), sigma_z) if smooth > 0 else np.where(seeds, z, _F(0))
    return near, b.astype(_F), e, leak


def average(u, ce, cs):
    """(sum_q c_pq u_q, sum_q c_pq) of every pixel over its 4-neighbours inside the image, in the dtype of u; the order of the terms
    is north, south, west, east."""
    T = u.dtype.type
    ce, cs = ce.astype(T), cs.astype(T)
    num, den = np.zeros_like(u), np.zeros_like(u)
    num[1:] += cs[:-1] * u[:-1]
    den[1:] += cs[:-1]
    num[:-1] += cs[:-1] * u[1:]
    den[:-1] += cs[:-1]
    num[:, 1:] += ce[:, :-1] * u[:, :-1]
    den[:, 1:] += ce[:, :-1]
    num[:, :-1] += ce[:, :-1] * u[:, 1:]
    den[:, :-1] += ce[:, :-1]
    return num, den


def residual_of(u, seeds, ce, cs):
    """max over the holes of |avg_p - u_p|, avg_p = sum_q c_pq u_q / sum_q c_pq, in the dtype of u; 0 when there is no hole."""
    holes = ~seeds
    if not holes.any() or u.size == 1:
        return u.dtype.type(0)
    num, den = average(u, ce, cs)
    return np.abs(num[holes] / den[holes] - u[holes]).max()


def solve_exact(depth, weight=None, edge=None, smooth=2, sigma_z=0.02, leak=1e-3):
    """The float64 direct solve of the problem -> dict(depth [H,W] float64: the input at seeds, u at holes; u [H,W] float64: the
    boundary values at seeds, u at holes; seeds, index, dist2 as fill.fill_nearest_f32; b [H,W] float32).  No seed: depth 0."""
    near, b, e, leak = _problem(depth, weight, edge, smooth, sigma_z, leak, "solve_exact")
    seeds = near["seeds"]
    H, W = seeds.shape
    z = np.asarray(depth, _F).astype(np.float64)
    u = np.where(seeds, b, 0).astype(np.float64)
    holes = ~seeds
    n = int(holes.sum())
    if seeds.any() and n:
        ce, cs = (c.astype(np.float64) for c in _links(e, leak))
        num = np.full((H, W), -1, np.int64)
        num[holes] = np.arange(n)
        rows, cols, vals = [], [], []
        diag, rhs = np.zeros(n), np.zeros(n)
        for c, a, bb in ((ce[:, :-1], (slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                         (cs[:-1, :], (slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
            for p, q in ((a, bb), (bb, a)):                     # the link seen from either end
                hp = holes[p]
                ip, iq, cc, uq = num[p][hp], num[q][hp], c[hp], u[q][hp]
                np.add.at(diag, ip, cc)
                to_hole = iq >= 0
                rows.append(ip[to_hole]); cols.append(iq[to_hole]); vals.append(-cc[to_hole])
                np.add.at(rhs, ip[~to_hole], (cc * uq)[~to_hole])
        rows.append(np.arange(n)); cols.append(np.arange(n)); vals.append(diag)
        rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
        try:
            from scipy.sparse import csc_matrix
            from scipy.sparse.linalg import spsolve
            x = spsolve(csc_matrix((vals, (rows, cols)), shape=(n, n)), rhs)
        except ImportError:
            if n > DENSE_MAX_HOLES:
                raise RuntimeError(f"solve_exact: {n} holes need scipy (the dense solve stops at {DENSE_MAX_HOLES})") from None
            A = np.zeros((n, n))
            np.add.at(A, (rows, cols), vals)
            x = np.linalg.solve(A, rhs)
        u[holes] = np.atleast_1d(x)
    out = np.where(seeds, z, u) if seeds.any() else np.zeros((H, W))
    return dict(depth=out, u=u, seeds=seeds, index=near["index"], dist2=near["dist2"], b=b)


# ------------------------------------------------------------------------------------------ the pyramid and its schedule
def level_sizes(H, W):
    """[(H, W), (ceil(H/2), ceil(W/2)), ..]: the pyramid, down to the first level whose longer side is <= 4."""
    if not (1 <= H <= fill.MAX_SIDE and 1 <= W <= fill.MAX_SIDE):
        raise ValueError(f"diffuse: H and W must be in [1, {fill.MAX_SIDE}], got {H} x {W}")
    sizes = [(H, W)]
    while max(sizes[-1]) > COARSEST:
        h, w = sizes[-1]
        sizes.append(((h + 1) // 2, (w + 1) // 2))
    return sizes


def tiles_of(H, W):
    """(tiles down, tiles across): one region when the level fits it, 96 x 96 tiles with a halo of 16 otherwise."""
    return (1 if H <= REGION else -(-H // TILE)), (1 if W <= REGION else -(-W // TILE))


def default_sweeps(H, W):
    """The default number of sweeps on a level of H x W: four times its longer side, rounded up to whole launches of 16.  Over-relaxed
    sweeps shrink the error by about (omega - 1) each, exp(-2 pi / side) with omega_of's factor: exp(-8 pi) over the level."""
    return -(-4 * max(H, W) // SWEEPS_PER_LAUNCH) * SWEEPS_PER_LAUNCH


def omega_of(H, W):
    """The over-relaxation factor of a level, float32: 2 / (1 + sin(pi / max(H, W))), the optimum of a path as long as the longer
    side."""
    return _F(2.0 / (1.0 + math.sin(math.pi / max(H, W))))


def schedule(H, W, iters=None):
    """[(H_l, W_l, launches, sweeps per launch, omega)] from the finest level to the coarsest: a function of (H, W, iters) alone.
    iters None: default_sweeps of every level; an int: that many sweeps on every level.  A level of one region runs them in one
    launch, a level of several tiles in launches of 16 sweeps (the last one shorter), the halo refreshed in between."""
    if iters is not None and (isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 1 <= iters <= MAX_ITERS):
        raise ValueError(f"diffuse: iters must be None or an integer in [1, {MAX_ITERS}], got {iters!r}")
    out = []
    for h, w in level_sizes(H, W):
        n = default_sweeps(h, w) if iters is None else int(iters)
        if tiles_of(h, w) == (1, 1):
            out.append((h, w, [n], omega_of(h, w)))
        else:
            out.append((h, w, [SWEEPS_PER_LAUNCH] * (n // SWEEPS_PER_LAUNCH) + ([n % SWEEPS_PER_LAUNCH] if n % SWEEPS_PER_LAUNCH else []),
                        omega_of(h, w)))
    return out


def pool(u, fixed, e):
    """2 x 2 pooling of a level (cells at an odd border hold fewer pixels) -> (u, fixed, e) of the next: fixed = any; u = the mean
    of the cell's fixed pixels where there is one, of all its pixels otherwise (sums in row-major order, then one division);
    e = max."""
    T = u.dtype.type
    H, W = u.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    su, sf, nu, nf = np.zeros((h, w), T), np.zeros((h, w), T), np.zeros((h, w), T), np.zeros((h, w), T)
    ec = np.zeros((h, w), _F)
    for dy in (0, 1):
        for dx in (0, 1):
            a, f, ee = u[dy::2, dx::2], fixed[dy::2, dx::2], e[dy::2, dx::2]
            hh, ww = a.shape
            su[:hh, :ww] += a
            nu[:hh, :ww] += T(1)
            sf[:hh, :ww] += np.where(f, a, T(0))
            nf[:hh, :ww] += f.astype(T)
            ec[:hh, :ww] = np.maximum(ec[:hh, :ww], ee)
    fc = nf > 0
    return np.where(fc, sf / np.where(fc, nf, T(1)), su / nu), fc, ec


def relax_region(u, fixed, ce, cs, parity, sweeps, omega):
    """`sweeps` red-black over-relaxed sweeps in place on one region: u += omega (avg - u) on every pixel that is not fixed, the
    colour (y + x + parity) & 1 == 0 first; avg = wn un + ws us + ww uw + we ue, left to right, with the weights w_q = c_q / (cn +
    cs + cw + ce) formed once per launch.  (Written on differences, wn (un - u) + .., the sweeps stall once an update is under half
    an ulp of u and stop 4 x farther from the direct solve; the rounding of the sums written here is unbiased.)"""
    T = u.dtype.type
    y, x = np.indices(u.shape)
    free = ~fixed
    colour = [free & (((y + x + parity) & 1) == c) for c in (0, 1)]
    ce, cs = ce.astype(T), cs.astype(T)
    cn, cso, cw, ceo = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    cn[1:], cso[:-1], cw[:, 1:], ceo[:, :-1] = cs[:-1], cs[:-1], ce[:, :-1], ce[:, :-1]
    den = ((cn + cso) + cw) + ceo
    den = np.where(den > 0, den, T(1))
    wn, ws, ww, we = cn / den, cso / den, cw / den, ceo / den
    zero = np.zeros_like(u)
    for _ in range(sweeps):
        for c in (0, 1):
            un, us, uw, ue = zero.copy(), zero.copy(), zero.copy(), zero.copy()
            un[1:], us[:-1], uw[:, 1:], ue[:, :-1] = u[:-1], u[1:], u[:, :-1], u[:, 1:]
            avg = ((wn * un + ws * us) + ww * uw) + we * ue
            u[colour[c]] = (u + omega * (avg - u))[colour[c]]


def relax_level(u, fixed, e, leak, launches, omega):
    """The launches of one level: every launch relaxes each tile's region from the level as the launch found it (block-Jacobi
    between tiles, Gauss-Seidel inside) and writes the tile back.  The outermost ring of a region that does not reach the level's
    border stays as loaded."""
    H, W = u.shape
    ty, tx = tiles_of(H, W)
    ce, cs = _links(e, leak)
    omega = u.dtype.type(omega)
    for sweeps in launches:
        new = u.copy()
        for j in range(ty):
            for i in range(tx):
                y0, y1 = (0, H) if ty == 1 else (j * TILE, min(j * TILE + TILE, H))
                x0, x1 = (0, W) if tx == 1 else (i * TILE, min(i * TILE + TILE, W))
                ry0, ry1 = (0, H) if ty == 1 else (max(y0 - HALO, 0), min(y0 - HALO + REGION, H))
                rx0, rx1 = (0, W) if tx == 1 else (max(x0 - HALO, 0), min(x0 - HALO + REGION, W))
                r = (slice(ry0, ry1), slice(rx0, rx1))
                ur, fr = u[r].copy(), fixed[r].copy()
                if ty > 1:                                     # the ring of the 128 x 128 region, where it lies inside the level
                    if y0 - HALO >= 0: fr[0] = True
                    if y0 - HALO + REGION <= H: fr[-1] = True
                if tx > 1:
                    if x0 - HALO >= 0: fr[:, 0] = True
                    if x0 - HALO + REGION <= W: fr[:, -1] = True
                relax_region(ur, fr, ce[r], cs[r], (ry0 + rx0) & 1, sweeps, omega)     # a link that leaves the region starts at a fixed pixel
                new[y0:y1, x0:x1] = ur[y0 - ry0:y1 - ry0, x0 - rx0:x1 - rx0]
        u[...] = new


def fill_diffuse(depth, weight=None, edge=None, smooth=2, sigma_z=0.02, leak=1e-3, iters=None, dtype=np.float32):
    """The statement of be_fill_diffuse_f32 with the float arithmetic in `dtype` -> dict(depth [H,W] of `dtype`: the input at
    seeds, u at holes; index, dist2, seeds as fill.fill_nearest_f32; residual: max over the holes of |avg - u| after the last
    sweep, of `dtype`).  The start is fill_nearest's result pooled down the pyramid; every level is relaxed and handed to the
    holes of the next finer one as their start value (cascadic)."""
    T = np.dtype(dtype).type
    near, b, e, leak = _problem(depth, weight, edge, smooth, sigma_z, leak, "fill_diffuse")
    seeds = near["seeds"]
    H, W = seeds.shape
    plan = schedule(H, W, iters)
    z = np.asarray(depth, _F).astype(T)
    if not seeds.any():
        return dict(depth=np.zeros((H, W), T), index=near["index"], dist2=near["dist2"], seeds=seeds, residual=T(0))
    levels = [(np.where(seeds, b, near["depth"]).astype(T), seeds, e)]
    for _ in plan[1:]:
        levels.append(pool(*levels[-1]))
    for l in range(len(plan) - 1, -1, -1):
        u, fixed, el = levels[l]
        if l + 1 < len(plan):
            up = levels[l + 1][0].repeat(2, 0).repeat(2, 1)[:u.shape[0], :u.shape[1]]
            u = np.where(fixed, u, up)
            levels[l] = (u, fixed, el)
        relax_level(u, fixed, el, leak, plan[l][2], plan[l][3])
    u = levels[0][0]
    ce, cs = _links(e, leak)
    out = np.where(seeds, z, u)
    assert out.dtype == T
    return dict(depth=out, index=near["index"], dist2=near["dist2"], seeds=seeds, residual=residual_of(u, seeds, ce, cs))
