"""The contract of mesh rasterisation (native.raster_mesh, DepthPipeline.render_mesh) as pure numpy: to the kernels of
csrc/be_mesh_raster.hip what mesh.extract is to be_tsdf_mesh.hip and camera.splat to k_splat_zbuf.  Nothing here needs a GPU.

Method: a z-buffered triangle rasteriser.  Vertices are projected in floating point and snapped to a 1/256 pixel lattice; coverage
is decided on those integers alone, exactly, with the top-left rule, so two triangles that share an edge cover every pixel centre
on it exactly once; depth is interpolated perspective-correctly (1/Z is affine on the image plane) and the nearest fragment wins
under an unsigned minimum of 64-bit keys (depth bits : face index), which does not depend on the order fragments arrive in.

Inputs: mesh = the dict mesh.extract / read_ply return: vertices [V,3] float32 (X, Y, Z in the mesh's frame), faces [T,3] int32,
and optionally (absent or None) feat [C,V], normal [V,3] with normal_valid [V], weight [V].  cam_dst = (fy, fx, cy, cx)
(camera.Pinhole), pose = raycast's: the 12 numbers that map the camera's frame to the mesh's; vertices go through
volume.inverse_pose(pose) = (r0..r8, t0..t2).  size = (Ho, Wo), 1 <= Ho, Wo <= 16384.  All arithmetic below is in `dtype` with one
rounding per written operation; the cameras, the pose and the mesh are the float32 numbers the kernels take whatever dtype is.

Vertex stage, per vertex (X, Y, Z)
  Xc = ((r0 X + r1 Y) + r2 Z) + t0, Yc = ((r3 X + r4 Y) + r5 Z) + t1, Zc = ((r6 X + r7 Y) + r8 Z) + t2   (be_projection.h's grouping)
  u  = (fx Xc) / Zc + cx, v = (fy Yc) / Zc + cy           the column and the row, pixel centres on the integers (camera.py)
  xs = floor(u * 256 + 0.5), ys = floor(v * 256 + 0.5)    the snapped coordinates: 8 sub-pixel bits
  q  = 1 / Zc
  USABLE iff near < Zc < inf and |xs| <= 2^22 and |ys| <= 2^22, tested on the floats before any conversion: NaN fails.
A triangle with a vertex that is not usable is dropped whole.  There is no near-plane and no guard-band clipping: this camera
family sees a few degrees and the meshes it renders lie in front of it; a triangle that crosses the plane Zc = near, or that
reaches further than 2^14 pixels from the origin, is not drawn in part, it is not drawn.  With |xs|, |ys| <= 2^22 and the frame
inside [0, 16384) every edge function below is smaller than 2^48 in magnitude: int64 with room to spare.

Triangle stage, on the integers (int64; x the column, y the row, y down)
  A = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0)
  A == 0: dropped (mesh.extract documents that it emits zero-area triangles).
  The triangle FACES the camera iff A < 0: for Z > 0 the sign of A is the sign of det[p0; p1; p2] = n . p0 with n the winding
  normal (counter-clockwise seen from its tip, mesh.py), which is negative when n points back at the camera.
  cull = "back" drops A > 0, "front" drops A < 0, "none" keeps both.
  A < 0: vertices 1 and 2 are exchanged, and A = -A, for everything that follows; only `bary` is reported in the face's own order.
  E_i(P), the edge function of the edge opposite vertex i, which runs from a = v_(i+1) to b = v_(i+2) (indices mod 3):
    E_i = (xb - xa)(Py - ya) - (yb - ya)(Px - xa) at P = (256 x, 256 y) for the pixel (y, x); E_0 + E_1 + E_2 = A.
  The edge (dx, dy) = (xb - xa, yb - ya) is TOP-LEFT iff dy < 0 or (dy == 0 and dx > 0).
  Pixel (y, x) is INSIDE iff for every i: E_i > 0, or E_i == 0 and edge i is top-left.
  Only the pixels of the bounding box ceil(min xs / 256) .. floor(max xs / 256) (rows likewise), clipped to the frame, are visited.

Depth, per inside pixel
  w_i = (T) E_i / (T) A              int64 -> float rounds to nearest even
  iz  = (w0 q0 + w1 q1) + w2 q2,  z = 1 / iz
  A FRAGMENT exists iff the pixel is inside and 0 < z < inf, z as float32.

Z-buffer: per pixel the minimum over its fragments of (float32 bits of z) << 32 | face index, unsigned.  A positive float orders as
its bits: the nearest surface wins, and the lowest face index where depths are equal.

Resolve, per pixel with a winner, the winner's w_i, q_i and z recomputed by the operations above
  l_i = (w_i q_i) * z                the perspective-correct barycentric coordinates: `bary`
  an attribute a is (l0 a0 + l1 a1) + l2 a2: weight, every channel of feat, every component of normal
  normal: the interpolated (nx, ny, nz) rotated into the camera's frame, mx = (r0 nx + r1 ny) + r2 nz and so on, l = sqrt((mx mx
  + my my) + mz mz), normal = m / l; normal_valid iff all three vertices are normal_valid and 0 < l < inf, else +0 and False.

Outputs: dict(depth [Ho,Wo] float32 (the key's high word), face [Ho,Wo] int32, valid [Ho,Wo] bool, weight [Ho,Wo], feat
[C,Ho,Wo], normal [3,Ho,Wo], normal_valid [Ho,Wo], bary [3,Ho,Wo]); +0 / -1 / False where nothing landed.  What the mesh does not
hold, or `want` (a subset of ("feat", "normal", "weight", "bary")) does not name, is None.  T == 0 and V == 0 are legal.
Refused: a face index outside [0, V), a camera or pose that is not finite, a bad size, near or cull."""
from __future__ import annotations

import numpy as np

from . import camera, volume

_F = np.float32
SUB = 256                                                               # BE_RASTER_SUB: sub-pixel positions per pixel
GUARD = 1 << 22                                                         # BE_RASTER_GUARD: |xs|, |ys| of a usable vertex
MAX_SIZE = 16384                                                        # BE_RASTER_MAX_SIZE
CULL = ("none", "back", "front")                                        # the kernels' 0, 1, 2
WANT = ("feat", "normal", "weight", "bary")
_CHUNK = 1 << 21                                                        # candidate pixels expanded at a time


def check_params(who, size, near, cull, want):
    """size, near, cull and want, validated -> (Ho, Wo, near as a python float holding a float32, the cull code, want as a tuple)."""
    # MAX_SIZE, not the 2^24 of the splatting entries (native.TARGET_MAX_SIDE): the rasteriser's sub-pixel integers bound the image
    Ho, Wo = camera.check_size(who, size, MAX_SIZE, f"size must be (Ho, Wo), integers in [1, {MAX_SIZE}]")
    try:
        near = float(_F(near))
    except (TypeError, ValueError):
        near = float("nan")
    if not 0 <= near < float("inf"):                                     # NaN fails
        raise ValueError(f"{who}: near must be a finite number >= 0")
    if cull not in CULL:
        raise ValueError(f"{who}: cull must be one of {CULL}, got {cull!r}")
    if isinstance(want, str):
        want = (want,)
    try:
        want = tuple(want)
    except TypeError:
        want = (want,)
    if any(k not in WANT for k in want):
        raise ValueError(f"{who}: want must be a subset of {WANT}, got {want!r}")
    return int(Ho), int(Wo), near, CULL.index(cull), want


def check_mesh(who, mesh):
    """The shapes of a mesh dict -> (V, T, C); the optional members may be absent or None."""
    if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
        raise ValueError(f"{who}: mesh must be a dict with vertices [V,3] and faces [T,3] (mesh.extract, read_ply, extract_mesh)")
    shape = lambda a: tuple(getattr(a, "shape", ()))
    vs, fs = shape(mesh["vertices"]), shape(mesh["faces"])
    if len(vs) != 2 or vs[1] != 3:
        raise ValueError(f"{who}: vertices must be [V,3], got {vs}")
    if len(fs) != 2 or fs[1] != 3:
        raise ValueError(f"{who}: faces must be [T,3], got {fs}")
    V, T = vs[0], fs[0]
    if V >= 1 << 31 or T >= 1 << 31:
        raise ValueError(f"{who}: {V} vertices and {T} triangles; both must be below 2^31")
    C = 0
    feat = mesh.get("feat")
    if feat is not None:
        if len(shape(feat)) != 2 or shape(feat)[1] != V:
            raise ValueError(f"{who}: feat must be [C,{V}] or None, got {shape(feat)}")
        C = shape(feat)[0]
        if C > volume.MAX_CHANNELS:
            raise ValueError(f"{who}: feat holds {C} channels, at most {volume.MAX_CHANNELS}")
    if mesh.get("weight") is not None and shape(mesh["weight"]) != (V,):
        raise ValueError(f"{who}: weight must be [{V}] or None, got {shape(mesh['weight'])}")
    nrm, nv = mesh.get("normal"), mesh.get("normal_valid")
    if nrm is not None:
        if shape(nrm) != (V, 3):
            raise ValueError(f"{who}: normal must be [{V},3] or None, got {shape(nrm)}")
        if nv is not None and shape(nv) != (V,):
            raise ValueError(f"{who}: normal_valid must be [{V}] or None, got {shape(nv)}")
    return V, T, C


def vertex_stage(vertices, cam_dst, pose, near=1e-3, dtype=np.float32):
    """The vertex stage -> dict(xs, ys int64 [V] (0 where not usable), q [V] `dtype`, usable [V] bool, Zc [V] `dtype`)."""
    T = np.dtype(dtype).type
    fy, fx, cy, cx = np.asarray(camera.as_pinhole(cam_dst, "render(cam_dst)").f32(), T)
    camera.as_pose(pose, "render(pose)")
    r = np.asarray(volume.inverse_pose(pose), T)
    v = np.asarray(vertices, _F).reshape(-1, 3).astype(T)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        Xc = ((r[0] * X + r[1] * Y) + r[2] * Z) + r[9]
        Yc = ((r[3] * X + r[4] * Y) + r[5] * Z) + r[10]
        Zc = ((r[6] * X + r[7] * Y) + r[8] * Z) + r[11]
        u = (fx * Xc) / Zc + cx
        w = (fy * Yc) / Zc + cy
        xs = np.floor(u * T(SUB) + T(0.5))
        ys = np.floor(w * T(SUB) + T(0.5))
        q = T(1) / Zc
        usable = (Zc > T(_F(near))) & (Zc < T(np.inf)) & (np.abs(xs) <= T(GUARD)) & (np.abs(ys) <= T(GUARD))
    assert xs.dtype == T and q.dtype == T
    return dict(xs=np.where(usable, xs, 0).astype(np.int64), ys=np.where(usable, ys, 0).astype(np.int64), q=q, usable=usable, Zc=Zc)


def _setup(vs, faces, cull, Ho, Wo):
    """The triangle stage for all faces -> dict of [T'] arrays over the faces that are kept and whose clipped box is not empty:
    face (the index), i [3,T'] = the vertex indices in the positive orientation, swapped, A, xlo, xhi, ylo, yhi."""
    f = faces.astype(np.int64)
    keep = vs["usable"][f].all(1) if len(f) else np.zeros(0, bool)
    i0, i1, i2 = f[:, 0], f[:, 1], f[:, 2]
    x, y = vs["xs"], vs["ys"]
    A = (x[i1] - x[i0]) * (y[i2] - y[i0]) - (y[i1] - y[i0]) * (x[i2] - x[i0])
    keep &= A != 0
    if cull == 1:
        keep &= A < 0
    elif cull == 2:
        keep &= A > 0
    swapped = A < 0
    i1, i2 = np.where(swapped, i2, i1), np.where(swapped, i1, i2)
    A = np.abs(A)
    tx, ty = np.stack([x[i0], x[i1], x[i2]]), np.stack([y[i0], y[i1], y[i2]])
    xlo = np.maximum(-((-tx.min(0)) // SUB), 0)
    xhi = np.minimum(tx.max(0) // SUB, Wo - 1)
    ylo = np.maximum(-((-ty.min(0)) // SUB), 0)
    yhi = np.minimum(ty.max(0) // SUB, Ho - 1)
    keep &= (xlo <= xhi) & (ylo <= yhi)
    k = np.flatnonzero(keep)
    return dict(face=k, i=np.stack([i0, i1, i2])[:, k], swapped=swapped[k], A=A[k], xlo=xlo[k], xhi=xhi[k], ylo=ylo[k], yhi=yhi[k])


def _at(vs, tri, sel, px, py, T):
    """Coverage and depth of the pixels (py, px) under the triangles tri[...][sel] -> (inside, w [3], q [3], z, z32)."""
    i = tri["i"][:, sel]
    x, y = vs["xs"][i], vs["ys"][i]                                      # [3,n]
    Px, Py = px * SUB, py * SUB
    E, inside = [], np.ones(px.shape, bool)
    for e in range(3):
        a, b = (e + 1) % 3, (e + 2) % 3
        dx, dy = x[b] - x[a], y[b] - y[a]
        Ee = dx * (Py - y[a]) - dy * (Px - x[a])
        inside &= (Ee > 0) | ((Ee == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))
        E.append(Ee)
    A = tri["A"][sel]
    assert bool((E[0] + E[1] + E[2] == A).all())
    q = vs["q"][i]
    with np.errstate(all="ignore"):
        w = [Ee.astype(T) / A.astype(T) for Ee in E]
        iz = (w[0] * q[0] + w[1] * q[1]) + w[2] * q[2]
        z = T(1) / iz
        z32 = z.astype(_F)
    assert z.dtype == T
    return inside, w, q, z, z32


def fragments(mesh, cam_dst, pose, size, near=1e-3, cull="none", dtype=np.float32):
    """Every fragment of the head of this module, before the z-buffer -> dict(face [n] int64, pixel [n] int64 = y * Wo + x, z [n]
    float32) in the order of (face, row, column)."""
    Ho, Wo, near, cull, _ = check_params("render", size, near, cull, ())
    vs, tri, _ = _prepare(mesh, cam_dst, pose, Ho, Wo, near, cull, dtype)
    face, pixel, z = _fragments(vs, tri, Wo, np.dtype(dtype).type)
    return dict(face=face, pixel=pixel, z=z)


def _prepare(mesh, cam_dst, pose, Ho, Wo, near, cull, dtype):
    V, _, C = check_mesh("render", mesh)
    faces = np.asarray(mesh["faces"]).reshape(-1, 3)
    if faces.size and (faces.min() < 0 or faces.max() >= V):
        raise ValueError(f"render: a face index lies outside [0, {V})")
    vs = vertex_stage(mesh["vertices"], cam_dst, pose, near, dtype)
    return vs, _setup(vs, faces, cull, Ho, Wo), C


def _fragments(vs, tri, Wo, T):
    bw = tri["xhi"] - tri["xlo"] + 1
    n = bw * (tri["yhi"] - tri["ylo"] + 1)
    ends = np.cumsum(n)
    faces, pixels, zs = [], [], []
    start = 0
    while start < len(n):
        stop = max(start + 1, int(np.searchsorted(ends, (ends[start - 1] if start else 0) + _CHUNK, "right")))
        sel = np.repeat(np.arange(start, stop), n[start:stop])
        first = np.repeat(ends[start:stop] - n[start:stop], n[start:stop])
        o = np.arange(sel.size) + (ends[start] - n[start]) - first
        px = tri["xlo"][sel] + o % bw[sel]
        py = tri["ylo"][sel] + o // bw[sel]
        inside, _, _, _, z32 = _at(vs, tri, sel, px, py, T)
        with np.errstate(invalid="ignore"):
            frag = inside & (z32 > 0) & (z32 < _F(np.inf))
        faces.append(tri["face"][sel][frag])
        pixels.append((py * Wo + px)[frag])
        zs.append(z32[frag])
        start = stop
    cat = lambda parts, dt: np.concatenate(parts) if parts else np.zeros(0, dt)
    return cat(faces, np.int64), cat(pixels, np.int64), cat(zs, _F)


def render(mesh, cam_dst, pose, size, near=1e-3, cull="none", want=WANT, dtype=np.float32):
    """The rasteriser of the head of this module."""
    T = np.dtype(dtype).type
    Ho, Wo, near, cull, want = check_params("render", size, near, cull, want)
    vs, tri, C = _prepare(mesh, cam_dst, pose, Ho, Wo, near, cull, dtype)
    face, pixel, z32 = _fragments(vs, tri, Wo, T)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    zbuf = np.full(Ho * Wo, empty, np.uint64)
    np.minimum.at(zbuf, pixel, (np.ascontiguousarray(z32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | face.astype(np.uint64))
    hit = zbuf != empty
    out_face = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, zbuf >> np.uint64(32), 0).astype(np.uint32).view(_F)
    out = dict(depth=depth.reshape(Ho, Wo), face=out_face.reshape(Ho, Wo), valid=hit.reshape(Ho, Wo), weight=None, feat=None, normal=None,
               normal_valid=None, bary=None)
    has = lambda k: mesh.get(k) is not None
    todo = [k for k in want if k == "bary" or has(k)]
    if not todo:
        return out
    # resolve: the winner's arithmetic again
    o = np.flatnonzero(hit)
    where = np.full(int(tri["face"].max()) + 1 if len(tri["face"]) else 0, -1, np.int64)
    where[tri["face"]] = np.arange(len(tri["face"]))
    sel = where[out_face[o]]
    inside, w, q, z, zz = _at(vs, tri, sel, o % Wo, o // Wo, T)
    assert bool(inside.all()) and np.array_equal(zz.view(np.uint32), depth[o].view(np.uint32))
    idx = tri["i"][:, sel]
    with np.errstate(all="ignore"):
        l = [(w[k] * q[k]) * z for k in range(3)]
        mix = lambda a: (l[0] * a[idx[0]].astype(T) + l[1] * a[idx[1]].astype(T)) + l[2] * a[idx[2]].astype(T)

        def full(values, shape, fill=0):
            a = np.full((len(values), Ho * Wo), fill, _F)
            for c, v in enumerate(values):
                a[c, o] = v.astype(_F)
            return a.reshape(shape)

        if "bary" in todo:
            sw = tri["swapped"][sel]
            out["bary"] = full([l[0], np.where(sw, l[2], l[1]), np.where(sw, l[1], l[2])], (3, Ho, Wo))
        if "weight" in todo:
            out["weight"] = full([mix(np.asarray(mesh["weight"], _F))], (Ho, Wo))
        if "feat" in todo:
            f = np.asarray(mesh["feat"], _F).reshape(C, -1)
            out["feat"] = full([mix(f[c]) for c in range(C)], (C, Ho, Wo))
        if "normal" in todo:
            nrm = np.asarray(mesh["normal"], _F).reshape(-1, 3)
            nv = np.ones(len(nrm), bool) if mesh.get("normal_valid") is None else np.asarray(mesh["normal_valid"]).astype(bool)
            n = [mix(nrm[:, c]) for c in range(3)]
            r = np.asarray(volume.inverse_pose(pose), T)
            m = [(r[3 * k] * n[0] + r[3 * k + 1] * n[1]) + r[3 * k + 2] * n[2] for k in range(3)]
            ln = np.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
            assert ln.dtype == T
            ok = nv[idx[0]] & nv[idx[1]] & nv[idx[2]] & (ln > 0) & (ln < T(np.inf))
            out["normal"] = full([np.where(ok, c / ln, T(0)) for c in m], (3, Ho, Wo))
            valid = np.zeros(Ho * Wo, bool)
            valid[o] = ok
            out["normal_valid"] = valid.reshape(Ho, Wo)
    return out
