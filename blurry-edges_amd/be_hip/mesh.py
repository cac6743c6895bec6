"""The contract of mesh extraction from a truncated signed distance volume (native.mesh_field / tsdf_mesh, DepthPipeline.extract_mesh)
as pure numpy: to the kernels of csrc/be_tsdf_mesh.hip what volume.raycast is to k_tsdf_raycast.  Nothing here needs a GPU.

Method: marching tetrahedra on the Kuhn (Freudenthal) split of every cell into 6 tetrahedra about the body diagonal 000-111.  Its
case table has 16 entries per tetrahedron and is derived below from an orientation test; it has no ambiguous case; the split is the
same in every cell, so neighbouring cells agree on every face diagonal and the mesh has no cracks; and every mesh vertex lies on a
lattice edge owned by exactly one voxel, which gives an indexed mesh with shared vertices without a hash table or an atomic.

Inputs: D, W [Nz,Ny,Nx] float32 and Fm [C,Nz,Ny,Nx] float32 as volume.mean returns them (x fastest), origin = (X0, Y0, Z0) the
centre of voxel (0, 0, 0) and voxel = (sX, sY, sZ) in metres, min_weight (float32), normals (bool).  A voxel is OBSERVED iff
W > min_weight and POSITIVE iff D > 0 (D == 0 is not positive).  D must be finite wherever a voxel is observed - volume.mean's D
lies in [-1, 1] - and extract refuses a field where it is not; the kernels do not look.

Numbering
  cube corner  k = 4 dz + 2 dy + dx, the order of volume._corners
  edge type    e = 0..6 with the offsets (dx, dy, dz) = (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1); edge (v, e)
               runs from voxel v, its OWNER, to v + offset_e
  tetrahedron  t = 0..5: the permutations (a, b, c) of the axes (x = 0, y = 1, z = 2) in the order of
               itertools.permutations(range(3)); corners p0 = 000, p1 = p0 + e_a, p2 = p1 + e_b, p3 = 111
  tet code     bit i is set when p_i is positive

Cells and edges.  Cell (iz, iy, ix), 0 <= i <= N - 2 per axis, is VALID iff all 8 corners are observed (raycast's rule); only valid
cells emit triangles.  An edge is ACTIVE iff its endpoints differ in positivity and at least one valid cell contains both (up to 4
cells for an axis edge, 2 for a face diagonal, 1 for the body diagonal).  All 19 lattice edges of a cell are edges of its
tetrahedra, so every emitted vertex is referenced by a triangle and every triangle's vertices exist.

Triangles of a tet code (tables(), and nothing else, defines them).  One positive corner, or one non-positive corner, L with the
others o1 < o2 < o3 in tet-corner order: one triangle over the edges (L,o1), (L,o2), (L,o3).  Two and two, positives A < B and
non-positives C < E: the quad cut into (AC, AE, BE) and (AC, BE, BC).  Then every triangle is oriented: with m_i the midpoints of
its three edges in lattice coordinates, the last two are swapped when ((m1 - m0) x (m2 - m0)) . (centroid of the positive corners
- centroid of the others) < 0; it is never 0.  The winding normal (counter-clockwise seen from its tip) therefore points towards
D > 0: free space, the camera's side.

Vertex of an active edge from a (the owner) to b, in `dtype` arithmetic with one rounding per written operation:
  t        = Da / (Da - Db); the signs differ, so the denominator is never 0 and t lies in [0, 1]
  position xa + t * (xb - xa) per axis, xa = X0 + (float) ix * sX and xb = X0 + (float)(ix + off) * sX as k_tsdf_integrate forms
           centres: the volume's frame, metres
  weight   Wa + t * (Wb - Wa); the channels of Fm likewise
Normal (normals=True).  Per endpoint p and axis the gradient of D over the metric spacing s is (D[+1] - D[-1]) * 0.5f / s where
both neighbours exist and are observed, else the one-sided (D[+1] - D[p]) / s or (D[p] - D[-1]) / s towards the one that is.  One
always is: the endpoint is a corner of a valid cell, whose corners are all observed and which holds a neighbour of p along every
axis (asserted below).  Then g = ga + t * (gb - ga), l = sqrtf((gx gx + gy gy) + gz gz), normal = g / l and normal_valid iff
0 < l < inf; otherwise +0 and False.  The gradient of D points towards D > 0, as the winding normals do.

Order.  Vertices in increasing (owner's linear index (iz Ny + iy) Nx + ix, e); triangles in increasing (cell's linear index in the
same voxel numbering, t, the table's order).

Outputs: dict(vertices [V,3] float32 (X, Y, Z), faces [T,3] int32, weight [V] float32, feat [C,V] float32 or None (C == 0),
normal [V,3] float32 and normal_valid [V] bool (None without normals), edge [V] int64 = 7 * owner + e, the vertex's identity).
V == 0 and T == 0 is a legal result: arrays of length 0.  V or T >= 2^31 is refused (check_totals).

Documented, not removed: zero-area triangles.  Where a D is exactly 0 the vertices of all edges that end there coincide (t is 0 or
1), and the triangles between them have no area; they keep the mesh's topology closed and are left in.

write_ply / read_ply: binary little-endian PLY, see there."""
from __future__ import annotations

import itertools

import numpy as np

from . import volume

_F = np.float32
EDGE_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))      # (dx, dy, dz) of edge type e
_E_OF_BITS = {dx + 2 * dy + 4 * dz: e for e, (dx, dy, dz) in enumerate(EDGE_OFFSETS)}               # cube-corner difference -> e
TETS = tuple(itertools.permutations(range(3)))
MAX_TOTAL = 1 << 31

_TABLES = None


def tables():
    """The case table, derived -> dict(corners [6,4] = the cube corner k of tet corner p_i, count [6,16] = triangles of (t, code),
    pairs [6,16,2,3,2] = the tet corners (i < j) of each triangle vertex's edge (-1 where there is no triangle),
    owner [6,16,2,3] = the cube corner that owns that edge and etype [6,16,2,3] = its edge type (-1 likewise),
    cube_count [256] = the triangles of a cell by its cube code (bit k set when corner k is positive))."""
    global _TABLES
    if _TABLES is not None:
        return _TABLES
    corners = np.zeros((6, 4), np.int64)
    count = np.zeros((6, 16), np.int64)
    pairs = np.full((6, 16, 2, 3, 2), -1, np.int64)
    for t, (a, b, c) in enumerate(TETS):
        corners[t] = (0, 1 << a, (1 << a) | (1 << b), 7)
        P = np.array([[(k >> ax) & 1 for ax in range(3)] for k in corners[t]], np.float64)       # lattice (x, y, z) of p_i
        for code in range(1, 15):
            pos = [i for i in range(4) if code >> i & 1]
            neg = [i for i in range(4) if not code >> i & 1]
            if len(pos) == 2:
                (A, B), (C_, E) = pos, neg
                tris = [[(A, C_), (A, E), (B, E)], [(A, C_), (B, E), (B, C_)]]
            else:
                L, others = (pos[0], neg) if len(pos) == 1 else (neg[0], pos)
                tris = [[(L, o) for o in others]]
            towards = P[pos].mean(0) - P[neg].mean(0)
            for s, tri in enumerate(tris):
                tri = [tuple(sorted(p)) for p in tri]
                m = [(P[i] + P[j]) / 2 for i, j in tri]
                d = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), towards))
                assert d != 0.0
                if d < 0:
                    tri[1], tri[2] = tri[2], tri[1]
                pairs[t, code, s] = tri
            count[t, code] = len(tris)
    has = pairs[..., 0] >= 0
    ci = np.where(has, corners[np.arange(6)[:, None, None, None], np.maximum(pairs[..., 0], 0)], 0)
    cj = np.where(has, corners[np.arange(6)[:, None, None, None], np.maximum(pairs[..., 1], 0)], 0)
    etype = np.where(has, np.vectorize(lambda d: _E_OF_BITS.get(int(d), -1))(cj - ci), -1)
    assert (etype[has] >= 0).all() and ((ci & cj) == ci).all()          # the tet's corners are nested: p_j - p_i is an edge offset
    owner = np.where(has, ci, -1)
    cube_count = np.zeros(256, np.int64)
    for cube in range(256):
        for t in range(6):
            cube_count[cube] += count[t, sum((cube >> int(corners[t, i]) & 1) << i for i in range(4))]
    _TABLES = dict(corners=corners, count=count, pairs=pairs, owner=owner, etype=etype, cube_count=cube_count)
    return _TABLES


def table_header():
    """The table as the text of csrc/be_tsdf_mesh_table.h (python -m be_hip.mesh > csrc/be_tsdf_mesh_table.h; test_mesh_cpu.py holds
    the committed file to this text)."""
    tb = tables()
    vert = np.where(tb["owner"] >= 0, tb["owner"] * 8 + tb["etype"], 255)
    row = lambda a: ", ".join(str(int(v)) for v in a)
    out = ["// Generated by `python -m be_hip.mesh` from mesh.tables(), which derives the marching-tetrahedra case table; do not edit.",
           "// kMeshTetCorner[t][i]: the cube corner k = 4 dz + 2 dy + dx of tet corner p_i.  kMeshTriCount[t][code]: triangles of a tet code.",
           "// kMeshTriVert[t][code][s][j]: vertex j of triangle s as (owner cube corner) * 8 + (edge type e), 255 where there is none.",
           "// kMeshCubeCount[cube]: the triangles of a cell whose corner k is positive iff bit k of `cube` is set.",
           "#pragma once", "#include <cstdint>", "",
           "__constant__ uint8_t kMeshTetCorner[6][4] = {" + ", ".join("{" + row(r) + "}" for r in tb["corners"]) + "};",
           "__constant__ uint8_t kMeshTriCount[6][16] = {"]
    out += ["    {" + row(r) + "}," for r in tb["count"]]
    out += ["};", "__constant__ uint8_t kMeshTriVert[6][16][2][3] = {"]
    for t in range(6):
        out.append("    {" + ", ".join("{{" + row(vert[t, c, 0]) + "}, {" + row(vert[t, c, 1]) + "}}" for c in range(16)) + "},")
    out += ["};", "__constant__ uint8_t kMeshCubeCount[256] = {"]
    out += ["    " + row(tb["cube_count"][i:i + 32]) + "," for i in range(0, 256, 32)]
    out += ["};", ""]
    return "\n".join(out)


def check_totals(V, T):
    """The one place that refuses a mesh too large for int32 indices."""
    V, T = int(V), int(T)
    if V < 0 or T < 0 or V >= MAX_TOTAL or T >= MAX_TOTAL:
        raise ValueError(f"mesh: {V} vertices and {T} triangles; both must be below 2^31 (extract a part of the volume at a time)")
    return V, T


def check_field(who, D, W, Fm, origin, voxel, min_weight):
    """Shapes and parameters, validated -> (dims, origin, voxel as python floats holding float32 values, min_weight likewise, C)."""
    shape = tuple(getattr(D, "shape", ()))
    if len(shape) != 3:
        raise ValueError(f"{who}: D must be [Nz,Ny,Nx], got {shape}")
    if tuple(getattr(W, "shape", ())) != shape:
        raise ValueError(f"{who}: W must be {shape} like D, got {tuple(getattr(W, 'shape', ()))}")
    C = 0
    if Fm is not None:
        fs = tuple(getattr(Fm, "shape", ()))
        if len(fs) != 4 or fs[1:] != shape:
            raise ValueError(f"{who}: Fm must be [C,{shape[0]},{shape[1]},{shape[2]}] or None, got {fs}")
        C = fs[0]
    dims, origin, voxel, _, C = volume.check_params(who, shape, origin, voxel, 1.0, C)
    try:
        min_weight = float(_F(min_weight))
    except (TypeError, ValueError):
        min_weight = float("nan")
    if not 0 <= min_weight < float("inf"):                               # NaN fails
        raise ValueError(f"{who}: min_weight must be a finite number >= 0")
    return dims, origin, voxel, min_weight, C


def _shifted(a, dz, dy, dx, fill):
    """a[iz + dz, iy + dy, ix + dx] with `fill` outside, offsets in {-1, 0, 1}."""
    p = np.pad(a, 1, constant_values=fill)
    Nz, Ny, Nx = a.shape
    return p[1 + dz:1 + dz + Nz, 1 + dy:1 + dy + Ny, 1 + dx:1 + dx + Nx]


def extract(D, W, Fm=None, origin=(0.0, 0.0, 0.0), voxel=(1.0, 1.0, 1.0), min_weight=0.0, normals=True, dtype=np.float32):
    """The mesh of the head of this module out of the field (D, W, Fm)."""
    T = np.dtype(dtype).type
    D, W = np.asarray(D, _F), np.asarray(W, _F)
    Fm = None if Fm is None else np.asarray(Fm, _F)
    (Nz, Ny, Nx), origin, voxel, min_weight, C = check_field("extract", D, W, Fm, origin, voxel, min_weight)
    n = Nz * Ny * Nx
    tb = tables()
    with np.errstate(invalid="ignore"):
        obs = W > _F(min_weight)
        pos = D > 0
    if not np.isfinite(D[obs]).all():
        raise ValueError("extract: D must be finite wherever W > min_weight (the kernels do not look: their t would not be a number)")
    # cells, kept on the voxel grid at their origin corner: valid, cube code, triangle count
    valid = np.ones((Nz, Ny, Nx), bool)
    cube = np.zeros((Nz, Ny, Nx), np.int64)
    for k in range(8):
        dx, dy, dz = k & 1, k >> 1 & 1, k >> 2 & 1
        valid &= _shifted(obs, dz, dy, dx, False)
        cube |= _shifted(pos, dz, dy, dx, False).astype(np.int64) << k
    nt = np.where(valid, tb["cube_count"][cube], 0)
    # edges: crossed, and inside a valid cell
    mask = np.zeros((Nz, Ny, Nx, 7), bool)
    for e, (dx, dy, dz) in enumerate(EDGE_OFFSETS):
        inside = np.zeros((Nz, Ny, Nx), bool)
        for cz in ((0,) if dz else (-1, 0)):
            for cy in ((0,) if dy else (-1, 0)):
                for cx in ((0,) if dx else (-1, 0)):
                    inside |= _shifted(valid, cz, cy, cx, False)
        mask[..., e] = inside & (pos != _shifted(pos, dz, dy, dx, False))
    edge = np.flatnonzero(mask.reshape(-1))                             # 7 * owner + e, increasing
    V = edge.size
    cells = np.flatnonzero(nt.reshape(-1) > 0)
    check_totals(V, int(nt.sum()))
    vid = np.cumsum(mask.reshape(-1), dtype=np.int64) - 1               # the vertex of an active edge
    # faces: per cell the 6 x 2 triangle slots of the table in order, those present kept
    corner_lin = np.array([((k >> 2 & 1) * Ny + (k >> 1 & 1)) * Nx + (k & 1) for k in range(8)], np.int64)
    cc = cube.reshape(-1)[cells]
    slots = np.zeros((cells.size, 6, 2, 3), np.int64)
    present = np.zeros((cells.size, 6, 2), bool)
    for t in range(6):
        code = sum(((cc >> int(tb["corners"][t, i])) & 1) << i for i in range(4)) if cells.size else np.zeros(0, np.int64)
        present[:, t] = np.arange(2)[None, :] < tb["count"][t][code][:, None]
        own, et = tb["owner"][t][code], tb["etype"][t][code]            # [cells, 2, 3]
        key = (cells[:, None, None] + corner_lin[np.maximum(own, 0)]) * 7 + np.maximum(et, 0)
        slots[:, t] = np.where(own >= 0, vid[np.minimum(key, n * 7 - 1)], -1)
        assert mask.reshape(-1)[np.minimum(key, n * 7 - 1)][own >= 0].all()      # every triangle's vertices exist
    faces = slots[present].astype(np.int32).reshape(-1, 3)
    assert faces.shape[0] == int(nt.sum())
    # vertices
    a = edge // 7
    e = edge % 7
    off = np.array(EDGE_OFFSETS, np.int64)[e]                           # (dx, dy, dz)
    ax, ay, az = a % Nx, a // Nx % Ny, a // (Nx * Ny)
    b = a + (off[:, 2] * Ny + off[:, 1]) * Nx + off[:, 0]
    Df, Wf = D.reshape(-1), W.reshape(-1)
    with np.errstate(all="ignore"):
        Da, Db = Df[a].astype(T), Df[b].astype(T)
        t = Da / (Da - Db)
        assert t.dtype == T and bool(((t >= 0) & (t <= 1)).all())
        lerp = lambda fa, fb: fa + t * (fb - fa)
        vertices = np.empty((V, 3), _F)
        for axis, (ia, o, x0, s) in enumerate(zip((ax, ay, az), off.T, origin, voxel)):
            xa = T(x0) + ia.astype(T) * T(s)
            xb = T(x0) + (ia + o).astype(T) * T(s)
            vertices[:, axis] = lerp(xa, xb).astype(_F)
        weight = lerp(Wf[a].astype(T), Wf[b].astype(T)).astype(_F)
        feat = None
        if C:
            Ff = Fm.reshape(C, n)
            feat = np.stack([lerp(Ff[c][a].astype(T), Ff[c][b].astype(T)).astype(_F) for c in range(C)])
        normal = normal_valid = None
        if normals:
            def gradient(p):
                pi = (p % Nx, p // Nx % Ny, p // (Nx * Ny))
                g = []
                for axis, (i, N, st, s) in enumerate(zip(pi, (Nx, Ny, Nz), (1, Nx, Nx * Ny), voxel)):
                    hi, lo = np.minimum(p + st, n - 1), np.maximum(p - st, 0)
                    has_hi = (i + 1 < N) & obs.reshape(-1)[hi]
                    has_lo = (i - 1 >= 0) & obs.reshape(-1)[lo]
                    assert bool((has_hi | has_lo).all())                # the endpoint is a corner of a valid cell
                    Dp, Dh, Dl = Df[p].astype(T), Df[hi].astype(T), Df[lo].astype(T)
                    g.append(np.where(has_hi & has_lo, (Dh - Dl) * T(0.5) / T(s), np.where(has_hi, (Dh - Dp) / T(s), (Dp - Dl) / T(s))))
                return g
            ga, gb = gradient(a), gradient(b)
            g = [lerp(u, v) for u, v in zip(ga, gb)]
            l = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            assert l.dtype == T
            normal_valid = (l > 0) & (l < np.inf)
            normal = np.stack([np.where(normal_valid, c / l, T(0)) for c in g], 1).astype(_F).reshape(V, 3)
    return dict(vertices=vertices, faces=faces, weight=weight, feat=feat, normal=normal, normal_valid=normal_valid, edge=edge.astype(np.int64))


def extract_volume(vol, min_weight=0.0, normals=True, dtype=np.float32, field=None):
    """extract on the means of the numpy volume `vol` (field: volume.mean(vol) when the caller already holds it)."""
    D, W, Fm = volume.mean(vol) if field is None else field
    return extract(D, W, Fm if vol.C else None, vol.origin, vol.voxel, min_weight, normals, dtype)


# ---------------------------------------------------------------------------------------------- PLY files
def write_ply(path, mesh, colour=None):
    """Binary little-endian PLY: per vertex x y z float, nx ny nz float when mesh["normal"] is present, red green blue uchar =
    floor(clamp(c, 0, 1) * 255 + 0.5) when colour is a [3,V] array; per face a `uchar int` list of 3 indices."""
    v = np.ascontiguousarray(np.asarray(mesh["vertices"], _F).reshape(-1, 3))
    f = np.asarray(mesh["faces"], np.int32).reshape(-1, 3)
    nrm = mesh.get("normal")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if nrm is not None:
        nrm = np.asarray(nrm, _F)
        if nrm.shape != v.shape:
            raise ValueError(f"write_ply: normal must be {v.shape}, got {nrm.shape}")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colour is not None:
        colour = np.asarray(colour, _F)
        if colour.shape != (3, v.shape[0]):
            raise ValueError(f"write_ply: colour must be [3,{v.shape[0]}], got {colour.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(v.shape[0], np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = v[:, 0], v[:, 1], v[:, 2]
    if nrm is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colour is not None:
        with np.errstate(invalid="ignore"):
            c8 = np.floor(np.clip(np.where(np.isnan(colour), _F(0), colour), _F(0), _F(1)) * _F(255) + _F(0.5)).astype(np.uint8)
        rec["red"], rec["green"], rec["blue"] = c8
    frec = np.zeros(f.shape[0], np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    frec["n"], frec["i"] = 3, f
    names = {"<f4": "float", "u1": "uchar"}
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}"]
    head += [f"property {names[dt]} {name}" for name, dt in fields]
    head += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def read_ply(path):
    """The files write_ply writes -> dict(vertices [V,3] float32, faces [T,3] int32, normal [V,3] float32 or None, colour [3,V]
    uint8 or None)."""
    with open(path, "rb") as fh:
        raw = fh.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"read_ply: {path} is not a PLY file")
    lines = raw[:end].decode("ascii").split("\n")
    body = raw[end + len(b"end_header\n"):]
    if lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"read_ply: {path}: only binary_little_endian 1.0 is read, got {lines[1]!r}")
    types = {"float": "<f4", "uchar": "u1"}
    V = T = 0
    fields, where = [], None
    for ln in lines[2:]:
        w = ln.split()
        if not w or w[0] == "comment":
            continue
        if w[0] == "element":
            where = w[1]
            if where == "vertex":
                V = int(w[2])
            elif where == "face":
                T = int(w[2])
            else:
                raise ValueError(f"read_ply: {path}: unknown element {where!r}")
        elif w[0] == "property" and where == "vertex":
            if w[1] not in types:
                raise ValueError(f"read_ply: {path}: vertex property type {w[1]!r} is not read")
            fields.append((w[2], types[w[1]]))
        elif w[0] == "property" and where == "face":
            if w[1:] != ["list", "uchar", "int", "vertex_indices"]:
                raise ValueError(f"read_ply: {path}: faces must be `list uchar int vertex_indices`")
    vdt = np.dtype(fields)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    if len(body) != V * vdt.itemsize + T * fdt.itemsize:
        raise ValueError(f"read_ply: {path}: {len(body)} bytes of data, the header describes {V * vdt.itemsize + T * fdt.itemsize}")
    rec = np.frombuffer(body, vdt, V)
    frec = np.frombuffer(body, fdt, T, V * vdt.itemsize)
    if T and not (frec["n"] == 3).all():
        raise ValueError(f"read_ply: {path}: only triangles are read")
    names = [n for n, _ in fields]
    col = lambda ks: np.stack([rec[k] for k in ks], 1) if V else np.zeros((0, 3), rec[ks[0]].dtype)
    return dict(vertices=col(("x", "y", "z")).astype(_F), faces=frec["i"].astype(np.int32).reshape(T, 3),
                normal=col(("nx", "ny", "nz")).astype(_F) if "nx" in names else None,
                colour=np.ascontiguousarray(col(("red", "green", "blue")).T) if "red" in names else None)


if __name__ == "__main__":
    import sys
    sys.stdout.write(table_header())
