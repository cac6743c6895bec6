"""The contract of mesh simplification (native.mesh_cluster / mesh_simplify, DepthPipeline.simplify_mesh) as pure numpy: to the
kernels of csrc/be_mesh_simplify.hip what components.py is to be_mesh_components.hip.  Nothing here needs a GPU.

Method: vertex clustering (Rossignac-Borrel).  Every vertex falls into a cell of a regular grid, every occupied cell becomes one
vertex at the weighted mean of its members, every face is re-indexed, and the faces that collapse or repeat are dropped.  Every output
is defined by the mesh and the grid alone - a cluster's label is its LEAST member index, the sums are integers, of equal faces the
LEAST index stays - so a kernel may visit vertices and faces in any order and still has to give these bits.

Inputs: mesh = the dict mesh.extract / components.select return (components.check_mesh): vertices [V,3] float32, faces [T,3] int32,
and optionally (absent or None) weight [V], feat [C,V], normal [V,3], normal_valid [V], edge.  cell = one number or three (cX, cY,
cZ) in metres - per axis, because the voxels are -, origin = (oX, oY, oZ) = a corner of cell (0, 0, 0), flaps = False.
Refused: a cell c for which float32(c) is not a finite number > 0 or for which inv (below) is not finite; an origin that is not
finite as float32; a face index outside [0, V) (the kernels cannot refuse it without a read-back and ignore such a face).

grid(cell, origin), on the host, per axis: c = float32(cell), inv = float32(1.0 / float64(c)), o = float32(origin).

cells(vertices, grid), per vertex and axis, in float32 with one rounding per written operation and no fused multiply-add:
  t = (x - o) * inv,  i = floorf(t),  r = t - i (exact; in [0, 1], and 1 only for a t in (-2^-25, 0), where i = -1),
  q = (int64)(r * 2^24): the scaling is exact, the result truncated, 0 <= q <= 2^24.  No division.
  A vertex is UNUSABLE when for any axis |i| < 2^20 does not hold (NaN and infinite t fail it) or when its quantised weight
  wq = fusion.quantise_weight(weight) = floorf(min(w, 16) * 65536 + 0.5) for w > 0, else 0, is 0; a None weight gives wq = 65536.
  key = ((iX + 2^20) << 42) | ((iY + 2^20) << 21) | (iZ + 2^20), 63 bits, for a usable vertex.

cluster(mesh, cell, origin)
  The usable vertices with equal (iX, iY, iZ) form a cluster; an unusable vertex belongs to none.
  label [V] int32    the least member index of the vertex's cluster, -1 for an unusable vertex; label[v] == v exactly for the ROOT
  cluster [V] int32  the dense id 0..V'-1 of the cluster, numbered in increasing order of label (components.label's rule); -1
  members [V'] int32 the number of vertices in each cluster
  V'                 the number of clusters

simplify(mesh, cell, origin, flaps) -> the simplified mesh.  Per cluster, every sum in int64 over its members (wrapping; exact while
a cell holds fewer than 2^16 members: wq <= 2^20, q <= 2^24, |fq| <= 2^27; that limit is documented, not checked):
  sw = sum wq,  sq_a = sum wq q_a per axis,  sf_c = sum wq fq_c with fq = fusion.quantise_feat(feat_c),
  swn = sum wq and sn_a = sum wq fusion.quantise_feat(normal_a) over the members whose normal_valid is set (all, when it is None).
  In float64 with one rounding per written operation, i the cell index of the cluster (every member's is the same):
  vertices'_a = float32(o + (i + (double) sq_a / (double) sw * 2^-24) * c)        (o, i, c converted exactly)
  weight'     = float32((double) sw / (double) members * 2^-16)                     (None when the mesh holds no weight)
  feat'_c     = float32((double) sf_c / (double) sw * 2^-16)                        (fusion.py finalises channels so; None stays None)
  normal':      m_a = float32((double) sn_a / (double) swn * 2^-16), +0 where swn == 0; then in float32
                l = sqrtf((mX mX + mY mY) + mZ mZ), normal' = m / l and normal_valid' where swn > 0 and 0 < l < inf, else +0 and
                False - mesh.extract's and registration.depth_normals' operations.  A mesh with normals gets normal_valid' even
                when it came without a mask; a mesh without normals keeps None for both.
  edge' = None: an edge id names one vertex of one volume and does not survive clustering.
  cluster [V] int32, members [V'] int32 as above.

Faces.  A face maps corner by corner through cluster.  It is dropped when a corner is unusable or when two corners land in one
cluster.  The other faces are compared up to rotation: with (a, b, c) the face's clusters rotated so that a is the least, its
TRIPLE is (a, min(b, c), max(b, c)) and its WINDING is 0 when b < c, else 1.  Of the faces with one triple and one winding the
LEAST face index stays.  With flaps=False a triple that occurs in BOTH windings loses all its faces: two such faces are a
back-to-back flap of zero volume.  flaps=True keeps the least face index of each winding.  Kept faces stay in their old order with
their old corner order; face_index [T'] int32 gives the old positions.  V' == 0 and T' == 0 are legal."""
from __future__ import annotations

import numpy as np

from . import components, fusion

_F = np.float32
INDEX_BITS = 20                                                         # BE_SIMPLIFY_INDEX_BITS: |i| < 2^20 per axis, 21 bits of the key
FRAC_BITS = 24                                                          # BE_SIMPLIFY_FRAC_BITS: q counts 2^-24 of a cell


def grid(cell, origin=(0.0, 0.0, 0.0), who="simplify"):
    """(c, inv, o), each [3] float32, of the head of this module; refuses what it refuses."""
    try:
        c = np.asarray(cell, np.float64).reshape(-1)
        o = np.asarray(origin, np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: cell must be one number or three and origin three numbers, got {cell!r} and {origin!r}") from None
    if c.size == 1:
        c = np.repeat(c, 3)
    if c.size != 3 or o.size != 3:
        raise ValueError(f"{who}: cell must be one number or three (cX, cY, cZ) and origin three (oX, oY, oZ), got {cell!r} and {origin!r}")
    with np.errstate(all="ignore"):
        c, o = c.astype(_F), o.astype(_F)
        inv = (1.0 / c.astype(np.float64)).astype(_F)
    if not (np.isfinite(c).all() and (c > 0).all() and np.isfinite(inv).all()):
        raise ValueError(f"{who}: cell must be positive and finite (metres per axis), got {cell!r}")
    if not np.isfinite(o).all():
        raise ValueError(f"{who}: origin must be finite, got {origin!r}")
    return c, inv, o


def cells(vertices, g):
    """i [V,3] int64 (0 where not usable), q [V,3] int64, inside [V] bool = |i| < 2^20 on every axis, for g = grid(..)."""
    _, inv, o = g
    v = np.asarray(vertices, _F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        t = (v - o) * inv
        i = np.floor(t)
        r = t - i
        assert t.dtype == _F and r.dtype == _F
        inside = (np.abs(i) < _F(1 << INDEX_BITS)).all(1)              # NaN and inf fail
        q = r * _F(1 << FRAC_BITS)
    keep = inside[:, None]
    return np.where(keep, i, _F(0)).astype(np.int64), np.where(keep, q, _F(0)).astype(np.int64), inside


def keys(i):
    b = i + (1 << INDEX_BITS)
    return (b[:, 0] << (2 * INDEX_BITS + 2)) | (b[:, 1] << (INDEX_BITS + 1)) | b[:, 2]


def _weights(mesh, V):
    w = mesh.get("weight")
    return np.full(V, 65536, np.int64) if w is None else fusion.quantise_weight(np.asarray(w, _F).reshape(V)).astype(np.int64)


def _label(mesh, g):
    """-> (label, cluster int64 [V], V', i, q, wq) - the labelling and what the sums need."""
    V = len(mesh["vertices"])
    i, q, inside = cells(mesh["vertices"], g)
    wq = _weights(mesh, V)
    usable = inside & (wq != 0)
    label = np.full(V, -1, np.int64)
    idx = np.flatnonzero(usable)
    if len(idx):
        _, inv = np.unique(keys(i[idx]), return_inverse=True)
        least = np.full(inv.max() + 1, V, np.int64)
        np.minimum.at(least, inv, idx)
        label[idx] = least[inv]
    root = label == np.arange(V)
    dense = np.cumsum(root) - 1
    cluster = np.where(label >= 0, dense[np.maximum(label, 0)], -1) if V else np.zeros(0, np.int64)
    return label, cluster, int(root.sum()), i, q, wq


def cluster(mesh, cell, origin=(0.0, 0.0, 0.0)):
    """The labelling alone -> dict(label, cluster int32 [V], members int32 [V'], V')."""
    components.check_mesh("cluster", mesh)
    label, cl, V2, _, _, _ = _label(mesh, grid(cell, origin, "cluster"))
    return dict(label=label.astype(np.int32), cluster=cl.astype(np.int32), members=np.bincount(cl[cl >= 0], minlength=V2).astype(np.int32), V=V2)


def face_keep(cl, faces, flaps=False):
    """keep [T] bool of the head of this module, for cluster ids cl [V] (-1: unusable) and faces [T,3] in range."""
    T = len(faces)
    k = cl[faces] if T else np.zeros((0, 3), np.int64)
    ok = (k >= 0).all(1) & (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])
    idx = np.flatnonzero(ok)
    keep = np.zeros(T, bool)
    if not len(idx):
        return keep
    k = k[idx]
    s = np.argmin(k, 1)
    row = np.arange(len(idx))
    a, b, c = k[row, s], k[row, (s + 1) % 3], k[row, (s + 2) % 3]
    wind = (b > c).astype(np.int64)
    _, inv = np.unique(np.stack([a, np.minimum(b, c), np.maximum(b, c)], 1), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    least = np.full((inv.max() + 1, 2), T, np.int64)
    np.minimum.at(least, (inv, wind), idx)
    stays = least[inv, wind] == idx
    if not flaps:
        stays &= least[inv, 1 - wind] == T
    keep[idx] = stays
    return keep


def simplify(mesh, cell, origin=(0.0, 0.0, 0.0), flaps=False):
    """The simplified mesh of the head of this module: components.select's keys without vertex_index (edge = None), and cluster
    [V], members [V'], face_index [T']."""
    V, T, C = components.check_mesh("simplify", mesh)
    g = grid(cell, origin)
    c, _, o = (x.astype(np.float64) for x in g)
    faces = components._faces("simplify", mesh["faces"], V)
    label, cl, V2, i, q, wq = _label(mesh, g)
    used = cl >= 0
    k, wk = cl[used], wq[used]
    members = np.bincount(k, minlength=V2)

    def total(x):
        s = np.zeros(V2, np.int64)
        np.add.at(s, k, x[used])
        return s

    def mean(s, w, scale):
        with np.errstate(all="ignore"):
            return s.astype(np.float64) / w.astype(np.float64) * scale

    sw = total(wq)
    roots = np.flatnonzero(label == np.arange(V))
    vertices = np.stack([(o[a] + (i[roots, a].astype(np.float64) + mean(total(wq * q[:, a]), sw, 2.0 ** -FRAC_BITS)) * c[a]).astype(_F)
                         for a in range(3)], 1).reshape(V2, 3)
    out = dict(vertices=vertices, weight=None, feat=None, normal=None, normal_valid=None, edge=None)
    if mesh.get("weight") is not None:
        out["weight"] = mean(sw, members, 2.0 ** -16).astype(_F)
    if mesh.get("feat") is not None:
        fq = fusion.quantise_feat(np.asarray(mesh["feat"], _F).reshape(C, V))
        out["feat"] = np.stack([mean(total(wq * fq[ch]), sw, 2.0 ** -16).astype(_F) for ch in range(C)]).reshape(C, V2)
    if mesh.get("normal") is not None:
        nv = mesh.get("normal_valid")
        wn = wq if nv is None else wq * np.asarray(nv).reshape(V).astype(bool)
        nq = fusion.quantise_feat(np.asarray(mesh["normal"], _F).reshape(V, 3))
        swn = total(wn)
        m = [np.where(swn > 0, mean(total(wn * nq[:, a]), swn, 2.0 ** -16).astype(_F), _F(0)) for a in range(3)]
        with np.errstate(all="ignore"):
            l = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            assert l.dtype == _F
            valid = (swn > 0) & (l > 0) & (l < np.inf)
            out["normal"] = np.stack([np.where(valid, x / l, _F(0)) for x in m], 1).astype(_F).reshape(V2, 3)
        out["normal_valid"] = valid
    fi = np.flatnonzero(face_keep(cl, faces, flaps))
    out.update(faces=cl[faces[fi]].astype(np.int32).reshape(-1, 3), cluster=cl.astype(np.int32), members=members.astype(np.int32),
               face_index=fi.astype(np.int32))
    return out
