"""The contract of mesh cleaning (native.mesh_components / mesh_select / mesh_clean, DepthPipeline.clean_mesh) as pure numpy: to the
kernels of csrc/be_mesh_components.hip what raster.render is to be_mesh_raster.hip.  Nothing here needs a GPU.

Method: the connected components of an indexed triangle mesh, their sizes, a decision per component, and the compaction of the mesh
to the vertices and faces that stay.  Every output is defined by the mesh alone - a label is the LEAST vertex index of its component,
the sums are integers - so a kernel may visit faces in any order and still has to give these bits.

Inputs: mesh = the dict mesh.extract / read_ply return: vertices [V,3] float32, faces [T,3] int32, and optionally (absent or None)
weight [V], feat [C,V], normal [V,3], normal_valid [V], edge [V] int64.  The statement refuses a face index outside [0, V); the
kernels cannot without a read-back and ignore such a face: it links nothing, counts nowhere, has face_component -1 and is never kept.

label(V, faces)
  Two vertices are connected when a chain of faces joins them, each face joining its three indices: sharing one vertex is enough,
  and a face with repeated indices joins what it names.  A vertex no face names is a component of its own.
  label [V] int32          the least vertex index of the vertex's component; label[v] == v exactly for that vertex, the ROOT
  component [V] int32      the dense id 0..K-1 of the component, numbered in increasing order of label
  face_component [T] int32 component[faces[:, 0]]
  K                        the number of components

stats(mesh, labels), per component, [K]
  triangles int32, vertices int32, area_q int64, area float64 = area_q * 2^-40 (square metres).
  The area of a face with corners a, b, c, in float32 with one rounding per written operation and no fused multiply-add:
    u = b - a, v = c - a, n = (u.y v.z - u.z v.y, u.z v.x - u.x v.z, u.x v.y - u.y v.x)
    A = 0.5f * sqrtf((n.x n.x + n.y n.y) + n.z n.z);  A = 0 when it is not finite;  A = min(A, 2^22)
    q = (int64)(A * 2^40)                                an exact scaling, truncated; at most 2^62
  area_q = the sum of q over the component's faces in int64 (wrapping): fixed point under integer addition, as fusion.py sums.

decide(stats, min_triangles=None, min_area=None, largest=False) -> keep [K] bool
  keep = (triangles >= min_triangles) & (area_q >= area_threshold(min_area)); None asks nothing (0).
  area_threshold(a) = (int64)(float32(a) * 2^40), the product exact (in float64), clamped to 2^63 - 1.
  largest: of the kept components only the one with the most triangles stays, the lowest id on a tie.
  Refused: nothing asked for, a negative or non-finite threshold, min_triangles that is not an integer or is >= 2^31.

select(mesh, vertex_keep [V] bool) -> the compacted mesh
  The kept vertices stay in their order; the faces whose three indices are all in range and kept stay in their order, re-indexed.
  Every per-vertex array the mesh holds is gathered (weight, feat [C,V], normal, normal_valid, edge; None stays None).
  vertex_index [V'] int32 and face_index [T'] int32 give the old positions.  V' == 0 and T' == 0 are legal.

clean(mesh, ...) = label, stats, decide, then select(mesh, keep[component]); the result also holds component [V'] int32 (the OLD
dense ids of the vertices that stay) and components = the stats with keep."""
from __future__ import annotations

import numpy as np

from . import raster

_F = np.float32
AREA_BITS = 40                                                          # BE_COMPONENTS_AREA_BITS: area_q counts 2^-40 m^2
AREA_MAX = float(1 << (62 - AREA_BITS))                                 # 2^22: a face's area is clamped to this many square metres
PER_VERTEX = ("weight", "feat", "normal", "normal_valid", "edge")


def check_mesh(who, mesh):
    """raster.check_mesh, and the edge ids a mesh of mesh.extract carries -> (V, T, C)."""
    V, T, C = raster.check_mesh(who, mesh)
    edge = mesh.get("edge")
    if edge is not None and tuple(getattr(edge, "shape", ())) != (V,):
        raise ValueError(f"{who}: edge must be [{V}] or None, got {tuple(getattr(edge, 'shape', ()))}")
    return V, T, C


def _faces(who, faces, V):
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"{who}: a face index lies outside [0, {V})")
    return faces


def label(V, faces):
    """The components of V vertices under faces [T,3] (the head of this module) -> dict(label, component, face_component, K)."""
    V = int(V)
    if not 0 <= V < 1 << 31:
        raise ValueError(f"label: V must be in [0, 2^31), got {V}")
    f = _faces("label", faces, V)
    lab = np.arange(V, dtype=np.int64)
    # minimum propagation with hooking and pointer jumping to a fixed point: lab[v] is always a vertex of v's component, <= v
    while len(f):
        before = lab
        l = lab[f]
        m = np.repeat(l.min(1), 3)
        lab = lab.copy()
        np.minimum.at(lab, l.ravel(), m)
        np.minimum.at(lab, f.ravel(), m)
        while True:
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt
        if np.array_equal(lab, before):
            break
    root = lab == np.arange(V)
    dense = np.cumsum(root) - 1
    component = dense[lab] if V else np.zeros(0, np.int64)
    fc = component[f[:, 0]] if len(f) else np.zeros(0, np.int64)
    return dict(label=lab.astype(np.int32), component=component.astype(np.int32), face_component=fc.astype(np.int32), K=int(root.sum()))


def face_area_q(vertices, faces):
    """q of the head of this module for every face -> [T] int64."""
    v = np.asarray(vertices, _F).reshape(-1, 3)
    f = _faces("stats", faces, len(v))
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        A = _F(0.5) * np.sqrt((nx * nx + ny * ny) + nz * nz)
        assert A.dtype == _F
        A = np.where(np.isfinite(A), np.minimum(A, _F(AREA_MAX)), _F(0))
        return (A * _F(1 << AREA_BITS)).astype(np.int64)


def stats(mesh, labels):
    """Per component: dict(triangles, vertices int32 [K], area_q int64 [K], area float64 [K])."""
    check_mesh("stats", mesh)
    K = int(labels["K"])
    q = face_area_q(mesh["vertices"], mesh["faces"])
    fc = np.asarray(labels["face_component"], np.int64)
    area_q = np.zeros(K, np.int64)
    np.add.at(area_q, fc, q)
    return dict(triangles=np.bincount(fc, minlength=K).astype(np.int32),
                vertices=np.bincount(np.asarray(labels["component"], np.int64), minlength=K).astype(np.int32),
                area_q=area_q, area=area_q.astype(np.float64) * 2.0 ** -AREA_BITS)


def area_threshold(min_area):
    """(int64)(float32(min_area) * 2^40), clamped to 2^63 - 1; the product of a float32 and 2^40 is exact in float64."""
    return min(int(float(_F(min_area)) * float(1 << AREA_BITS)), (1 << 63) - 1)


def check_decision(who, min_triangles, min_area, largest):
    """What decide is asked, validated -> (min_triangles as an int, min_area as a python float holding a float32, largest)."""
    if min_triangles is None and min_area is None and not largest:
        raise ValueError(f"{who}: nothing asked for; give min_triangles, min_area or largest=True")
    mt = 0
    if min_triangles is not None:
        try:
            ok = not isinstance(min_triangles, bool) and int(min_triangles) == min_triangles and 0 <= min_triangles < 1 << 31
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError(f"{who}: min_triangles must be an integer in [0, 2^31), got {min_triangles!r}")
        mt = int(min_triangles)
    ma = 0.0
    if min_area is not None:
        try:
            ma = float(_F(min_area))
        except (TypeError, ValueError):
            ma = float("nan")
        if not 0 <= ma < float("inf"):                                   # NaN fails
            raise ValueError(f"{who}: min_area must be a finite number >= 0, got {min_area!r}")
    return mt, ma, bool(largest)


def decide(stats, min_triangles=None, min_area=None, largest=False):
    """keep [K] bool of the head of this module."""
    mt, ma, largest = check_decision("decide", min_triangles, min_area, largest)
    tri = np.asarray(stats["triangles"], np.int64)
    keep = (tri >= mt) & (np.asarray(stats["area_q"], np.int64) >= area_threshold(ma))
    if largest and keep.any():
        k = np.flatnonzero(keep)
        best = k[np.argmax(tri[k])]                                      # argmax: the first of equals, the lowest id
        keep = np.zeros_like(keep)
        keep[best] = True
    return keep


def select(mesh, vertex_keep):
    """The compacted mesh of the head of this module."""
    V, T, C = check_mesh("select", mesh)
    vk = np.asarray(vertex_keep)
    if vk.shape != (V,) or vk.dtype != np.bool_:
        raise ValueError(f"select: vertex_keep must be a bool array [{V}], got {vk.dtype} {vk.shape}")
    f = np.asarray(mesh["faces"]).reshape(-1, 3).astype(np.int64)
    inside = ((f >= 0) & (f < V)).all(1)
    fk = inside.copy()
    fk[inside] = vk[f[inside]].all(1)
    new = np.cumsum(vk) - 1
    vi, fi = np.flatnonzero(vk), np.flatnonzero(fk)
    out = dict(vertices=np.asarray(mesh["vertices"], _F).reshape(-1, 3)[vi], faces=new[f[fi]].astype(np.int32).reshape(-1, 3))
    for k in PER_VERTEX:
        a = mesh.get(k)
        out[k] = None if a is None else np.ascontiguousarray(np.asarray(a)[..., vi] if k == "feat" else np.asarray(a)[vi])
    out.update(vertex_index=vi.astype(np.int32), face_index=fi.astype(np.int32))
    return out


def clean(mesh, min_triangles=None, min_area=None, largest=False):
    """label, stats, decide, select -> the mesh that stays, with component [V'] and components (the stats and keep)."""
    V, _, _ = check_mesh("clean", mesh)
    check_decision("clean", min_triangles, min_area, largest)
    lab = label(V, mesh["faces"])
    st = stats(mesh, lab)
    keep = decide(st, min_triangles, min_area, largest)
    out = select(mesh, keep[lab["component"].astype(np.int64)] if V else np.zeros(0, bool))
    out["component"] = lab["component"][out["vertex_index"].astype(np.int64)]
    out["components"] = dict(st, keep=keep)
    return out
