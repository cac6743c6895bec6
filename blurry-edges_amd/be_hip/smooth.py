"""The contract of mesh smoothing (native.mesh_adjacency / mesh_smooth / mesh_normals, DepthPipeline.smooth_mesh) as pure numpy: to
the kernels of csrc/be_mesh_smooth.hip what simplify.py is to be_mesh_simplify.hip.  Nothing here needs a GPU.

Method: Taubin's lambda | mu smoothing.  Every vertex moves towards the mean of its neighbours by a factor lam, then away from the
new mean by a factor mu < -lam, which undoes the shrinkage a plain Laplacian causes; the faces stay as they are.  Positions are
fixed-point integers (2^-30 m) and a vertex's neighbour sum is an integer sum, so a kernel may gather a row in any order and still
has to give these bits.

Inputs: mesh = the dict components.check_mesh accepts.  A vertex is USABLE when its three coordinates are finite and |x| <
2^COORD_MAX_LOG2.  A face is USABLE when its three indices are in [0, V), pairwise distinct, and name usable vertices.  An index
outside [0, V) is refused here, as components._faces refuses it; the kernels cannot without a read-back and ignore such a face.

adjacency(mesh) -> dict(valence [V] int32, boundary [V] bool)
  Every usable face (a, b, c) gives two SLOTS to each corner: a: (b, c), b: (c, a), c: (a, b).  valence[v] = the number of usable
  faces at v, so v has n = 2 valence slots: a neighbour across an interior edge occurs twice, one across a boundary edge once.
  The undirected edge {v, u} has count = the number of usable faces that hold it; boundary[v] = v touches an edge of count exactly
  1.  A face given twice counts twice - documented, not repaired.  An unusable vertex and one no usable face names: 0 and False.

smooth(mesh, iters=10, lam=0.5, mu=-0.53, boundary="fixed", normals="keep")
  A vertex is MOVABLE when n > 0 and (boundary == "free" or not boundary[v]).
  Q0 = (int64) rint((double) x * 2^FRAC_BITS) per coordinate; the product is exact.  Unusable vertices hold 0 and are never read.
  One STEP with factor f (a float64) updates all vertices at once from the previous Q:
    S = the int64 sum of Q[u] over the slots of v (wrapping; exact while n max|Q| < 2^63)
    in float64, one rounding per written operation: d = (double) S / (double) n - (double) Q
    Q' = Q + (int64) rint(f * d) for a movable v, else Q
  An iteration is a step with lam, then a step with mu unless mu == 0 (plain Laplacian smoothing).
  vertices' = the input bits where Q == Q0 on all three axes at the end, else float32((double) Q * 2^-FRAC_BITS): iters=0 returns
  the positions bit for bit.  displacement [V] float32, in float32 without fused multiply-add: sqrtf((dx dx + dy dy) + dz dz) of
  vertices' - vertices, 0 for an unusable vertex (never NaN).
  faces, weight, feat ride along unchanged; edge = None: a moved vertex has left its lattice edge; valence, boundary, displacement
  are new.  normals="keep" passes normal / normal_valid through, "recompute" replaces them by vertex_normals of the result, "drop"
  gives None for both.
  Refused: iters not an integer in [0, 10000], lam not finite in (0, 1], mu not finite in [-2, 0], other boundary / normals.

vertex_normals(mesh) -> dict(normal [V,3] float32, normal_valid [V] bool)
  Per usable face n = cross(b - a, c - a) from the face's OWN corner order, in components.face_area_q's operation order (float32,
  no fused multiply-add); a component that is not finite becomes 0; each is clamped to +-2^12; nq = (int64)(n * 2^NORMAL_BITS),
  the scaling exact, the value truncated.  Per vertex the int64 sum of nq over its usable faces - area weighting -, m =
  float32((double) sum * 2^-NORMAL_BITS), then in float32 l = sqrtf((mx mx + my my) + mz mz), normal = m / l and valid iff 0 < l <
  inf, else +0 and False: mesh.extract's operations.  The winding normal points to free space, as mesh.py states."""
from __future__ import annotations

import numpy as np

from . import components

_F = np.float32
FRAC_BITS = 30                                                          # BE_SMOOTH_FRAC_BITS: Q counts 2^-30 m
COORD_MAX_LOG2 = 16                                                     # BE_SMOOTH_COORD_MAX_LOG2: |x| < 2^16 m
NORMAL_BITS = 40                                                        # BE_SMOOTH_NORMAL_BITS: nq counts 2^-40 m^2
NORMAL_MAX = float(1 << 12)                                             # a face normal's component is clamped to this
MAX_ITERS = 10000
BOUNDARY, NORMALS = ("fixed", "free"), ("keep", "recompute", "drop")


def check_args(who, iters, lam, mu, boundary, normals):
    """What smooth is asked, validated -> (iters int, lam float, mu float, free bool, normals)."""
    try:
        ok = not isinstance(iters, bool) and int(iters) == iters and 0 <= iters <= MAX_ITERS
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: iters must be an integer in [0, {MAX_ITERS}], got {iters!r}")
    try:
        l, m = float(lam), float(mu)
    except (TypeError, ValueError):
        l = m = float("nan")
    if not 0 < l <= 1:                                                  # NaN fails
        raise ValueError(f"{who}: lam must be a finite number in (0, 1], got {lam!r}")
    if not -2 <= m <= 0:
        raise ValueError(f"{who}: mu must be a finite number in [-2, 0], got {mu!r}")
    if not isinstance(boundary, str) or boundary not in BOUNDARY:
        raise ValueError(f"{who}: boundary must be one of {BOUNDARY}, got {boundary!r}")
    if not isinstance(normals, str) or normals not in NORMALS:
        raise ValueError(f"{who}: normals must be one of {NORMALS}, got {normals!r}")
    return int(iters), l, m, boundary == "free", normals


def usable(mesh, who="smooth"):
    """(vertex_usable [V] bool, faces [T,3] int64 in range, face_usable [T] bool) of the head of this module."""
    v = np.asarray(mesh["vertices"], _F).reshape(-1, 3)
    f = components._faces(who, mesh["faces"], len(v))
    with np.errstate(all="ignore"):
        vu = (np.abs(v) < _F(1 << COORD_MAX_LOG2)).all(1)               # NaN and inf fail
    fu = np.zeros(len(f), bool)
    if len(f):
        fu = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) & vu[f].all(1)
    return vu, f, fu


def rows(V, f):
    """The slots of usable faces f [T',3] by vertex -> (neighbour int64 [6 T'], sorted by owner; start int64 [V], the first slot of
    each vertex): a: (b, c), b: (c, a), c: (a, b).  The order inside a row is that of the faces; only sums read it."""
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    owner, nb = np.concatenate([a, a, b, b, c, c]), np.concatenate([b, c, c, a, a, b])
    order = np.argsort(owner, kind="stable")
    count = np.bincount(owner, minlength=V) if len(owner) else np.zeros(V, np.int64)
    return nb[order], np.cumsum(count) - count


def _adjacency(V, f):
    """valence int64 [V], boundary bool [V] of usable faces f."""
    valence = np.bincount(f.ravel(), minlength=V).astype(np.int64) if len(f) else np.zeros(V, np.int64)
    boundary = np.zeros(V, bool)
    if len(f):
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        key = (e.min(1) << 32) | e.max(1)
        uniq, count = np.unique(key, return_counts=True)
        once = uniq[count == 1]
        boundary[once >> 32] = True
        boundary[once & 0xffffffff] = True
    return valence, boundary


def adjacency(mesh):
    """dict(valence [V] int32, boundary [V] bool) of the head of this module."""
    V, _, _ = components.check_mesh("adjacency", mesh)
    _, f, fu = usable(mesh, "adjacency")
    valence, boundary = _adjacency(V, f[fu])
    return dict(valence=valence.astype(np.int32), boundary=boundary)


def quantise(vertices, vu):
    """Q0 [V,3] int64: rint(x * 2^30) in float64 for usable vertices, 0 elsewhere."""
    v = np.asarray(vertices, _F).reshape(-1, 3)
    x = np.where(vu[:, None], v, _F(0)).astype(np.float64)
    return np.rint(x * float(1 << FRAC_BITS)).astype(np.int64)


def step(Q, nb, start, n, movable, f):
    """One step with factor f: Q [V,3] int64 -> Q' (a new array); nb, start = rows(..), n = 2 valence."""
    S = np.zeros_like(Q)
    has = n > 0
    if has.any():
        S[has] = np.add.reduceat(Q[nb], start[has], axis=0)             # int64, wrapping; rows without a slot are skipped
    with np.errstate(all="ignore"):
        d = S.astype(np.float64) / n.astype(np.float64)[:, None] - Q.astype(np.float64)
        move = np.rint(np.float64(f) * d)
    return Q + np.where(movable[:, None], move, 0.0).astype(np.int64)


def vertex_normals(mesh):
    """dict(normal [V,3] float32, normal_valid [V] bool) of the head of this module."""
    V, _, _ = components.check_mesh("vertex_normals", mesh)
    _, f, fu = usable(mesh, "vertex_normals")
    f = f[fu]
    v = np.asarray(mesh["vertices"], _F).reshape(-1, 3)
    total = np.zeros((V, 3), np.int64)
    if len(f):
        a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        with np.errstate(all="ignore"):
            u, w = b - a, c - a
            n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
            assert n.dtype == _F
            n = np.where(np.isfinite(n), n, _F(0))
            n = np.minimum(np.maximum(n, _F(-NORMAL_MAX)), _F(NORMAL_MAX))
            nq = (n * _F(2.0 ** NORMAL_BITS)).astype(np.int64)
        for k in range(3):
            np.add.at(total, f[:, k], nq)
    m = (total.astype(np.float64) * 2.0 ** -NORMAL_BITS).astype(_F)
    with np.errstate(all="ignore"):
        l = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        assert l.dtype == _F
        valid = (l > 0) & (l < np.inf)
        normal = np.where(valid[:, None], m / l[:, None], _F(0)).astype(_F)
    return dict(normal=normal.reshape(V, 3), normal_valid=valid)


def smooth(mesh, iters=10, lam=0.5, mu=-0.53, boundary="fixed", normals="keep"):
    """The smoothed mesh of the head of this module."""
    V, T, C = components.check_mesh("smooth", mesh)
    iters, lam, mu, free, normals = check_args("smooth", iters, lam, mu, boundary, normals)
    vu, f, fu = usable(mesh)
    f = f[fu]
    valence, bnd = _adjacency(V, f)
    nb, start = rows(V, f)
    n = 2 * valence
    movable = (n > 0) & (free | ~bnd)
    v = np.ascontiguousarray(np.asarray(mesh["vertices"], _F).reshape(-1, 3))
    Q0 = quantise(v, vu)
    Q = Q0
    for _ in range(iters):
        Q = step(Q, nb, start, n, movable, lam)
        if mu != 0:
            Q = step(Q, nb, start, n, movable, mu)
    same = (Q == Q0).all(1)
    new = (Q.astype(np.float64) * 2.0 ** -FRAC_BITS).astype(_F)
    out_v = np.where(same[:, None], v.view(np.uint32), new.view(np.uint32)).view(_F).reshape(V, 3)
    with np.errstate(all="ignore"):
        d = out_v - v
        disp = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        assert disp.dtype == _F
    disp = np.where(vu, disp, _F(0)).astype(_F)
    out = dict(vertices=out_v, faces=mesh["faces"], weight=mesh.get("weight"), feat=mesh.get("feat"), normal=None, normal_valid=None, edge=None,
               valence=valence.astype(np.int32), boundary=bnd, displacement=disp)
    if normals == "keep":
        out.update(normal=mesh.get("normal"), normal_valid=mesh.get("normal_valid"))
    elif normals == "recompute":
        out.update(vertex_normals(out))
    return out
