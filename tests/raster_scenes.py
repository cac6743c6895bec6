"""The meshes, cameras and targets the rasteriser's tests share (test_raster_cpu.py, test_raster_gpu.py): triangles placed by hand
on the pixel lattice, and the meshes of mesh_scenes.py seen by a camera.  A case is dict(mesh, cam, pose, size, kw); CASES names
them all, and reference() renders each with raster.render once.  Everything is numpy and is computed once."""
import numpy as np

from be_hip import camera, raster
import fuse_scenes as fs
import mesh_scenes as ms
import reproject_scenes as rs

_F = np.float32
_CACHE = {}

# under UNIT a vertex (X, Y, 1) lands on column X, row Y exactly
UNIT = camera.Pinhole(1, 1, 0, 0)
# DepthEtas.intrinsics(147, 147) at the default arguments: the pipeline's own camera (test_reproject_cpu.py holds the two equal)
PIPE = camera.Pinhole(4709.897610921502, 4709.897610921502, 73.0, 73.0)


def flat(points, faces, z=1.0, seed=0):
    """A mesh from (x, y) or (x, y, z) points under UNIT: vertex (x z, y z, z) lands on column x, row y.  Two channels, a weight and
    normals (not unit: the resolve normalises) drawn from default_rng(seed) ride along."""
    p = np.asarray(points, np.float64)
    p = p.reshape(len(p), p.shape[1] if p.ndim == 2 else 2)
    zz = p[:, 2] if p.shape[1] == 3 else np.full(len(p), float(z))
    v = np.stack([p[:, 0] * zz, p[:, 1] * zz, zz], 1).astype(_F)
    rng = np.random.default_rng(seed)
    V = len(v)
    return dict(vertices=v, faces=np.asarray(faces, np.int32).reshape(-1, 3), weight=rng.uniform(0.5, 4, V).astype(_F),
                feat=rng.standard_normal((2, V)).astype(_F), normal=rng.standard_normal((V, 3)).astype(_F), normal_valid=np.ones(V, bool))


def case(mesh, cam=UNIT, pose=None, size=(9, 9), **kw):
    return dict(mesh=mesh, cam=cam, pose=pose, size=size, kw=kw)


def flipped(mesh):
    return dict(mesh, faces=np.ascontiguousarray(mesh["faces"][:, [0, 2, 1]]))


# two triangles that share an edge through pixel centres: a diamond about (3, 3) cut along its horizontal and its vertical
# diagonal, and the square [1, 5]^2 cut along the diagonal (1, 1) - (5, 5)
DIAMOND = [(1, 3), (3, 1), (5, 3), (3, 5)]
PAIRS = dict(horizontal=flat(DIAMOND, [(0, 1, 2), (0, 2, 3)]), vertical=flat(DIAMOND, [(1, 2, 3), (1, 3, 0)]),
             diagonal=flat([(1, 1), (5, 1), (5, 5), (1, 5)], [(0, 1, 2), (0, 2, 3)]))
# the pixel centres (row, column) a polygon covers under the top-left rule, by hand: a boundary point counts iff the point just to
# its right (and, on a horizontal edge, just below) is inside
DIAMOND_PIXELS = {(3, 3), (3, 2), (3, 4), (2, 3), (4, 3), (2, 2), (3, 1), (4, 2)}
SQUARE_PIXELS = {(y, x) for y in range(1, 5) for x in range(1, 5)}

BIG_TRI = [(-10000, -10000), (15000, -10000), (-10000, 15000)]


def _dropped():
    """Face 4 is the only one that can be drawn: faces 0-3 and 5 each hold a vertex that is not usable (Zc <= near twice, NaN,
    infinite, beyond the guard band) and face 6 has no area."""
    good = [(1, 1), (7, 1), (1, 7)]
    m = flat(good + [(2, 2), (2, 2), (2, 2), (2, 2), (20000, 2), (4, 4)], [(0, 1, 3), (0, 1, 4), (0, 1, 5), (0, 1, 6), (0, 1, 2), (0, 1, 7), (0, 8, 2)])
    v = m["vertices"]
    v[3] = (0.001, 0.001, 0.0005)                                       # Zc <= near
    v[4] = (2, 2, -1)                                                   # behind the camera
    v[5] = (2, np.nan, 1)
    v[6] = (np.inf, 2, 1)
    m["faces"][6] = (1, 8, 2)                                           # (7, 1), (4, 4), (1, 7): collinear, A == 0
    return m


def _interpenetrating():
    """Two triangles over the same pixels whose depths cross: one rises along x from 1 to 3 m, the other falls."""
    pts = [(-1, -1, 1.0), (9, -1, 3.0), (-1, 9, 1.0), (9, 9, 3.0), (-1, -1, 3.0), (9, -1, 1.0), (-1, 9, 3.0), (9, 9, 1.0)]
    return flat(pts, [(0, 1, 2), (1, 3, 2), (4, 5, 6), (5, 7, 6)])


def _large_edge():
    """Edge functions of about 2^39 units (far above 2^24, where int64 -> float32 rounds) and depths from 1 to 3 m."""
    return flat([(-3000.3, -2000.7, 1.0), (2500.2, -1800.1, 2.0), (-1200.9, 3100.4, 3.0)], [(0, 1, 2)])


def _planted_nan():
    """The ellipsoid with NaN and infinities planted: three vertices, and attributes of others."""
    m = {k: None if v is None else np.array(v) for k, v in ms.reference("ellipsoid", ms.ellipsoid()).items()}
    m["feat"] = np.random.default_rng(8).standard_normal((2, len(m["vertices"]))).astype(_F)
    m["vertices"][[5, 300, 700]] = [(np.nan, 6, 6), (6, np.inf, 6), (6, 6, -np.inf)]
    m["weight"][[10, 400]] = (np.nan, np.inf)
    m["feat"][0, [20, 500]] = (np.inf, np.nan)
    m["normal"][[30, 600]] = [(np.nan, 0, 0), (0, np.inf, 0)]
    m["normal_valid"][[40, 41, 42]] = False
    return m


ELL_CAM, ELL_POSE = camera.Pinhole(27, 27, 20, 20), camera.pose(None, [6.3, 6.6, -20.0])      # the ellipsoid from outside, along +Z
PLANTED_CAM = camera.Pinhole(600, 12, 310.3, 2.1)                       # the planted strip (5 m x 2 cm at 1 m) spread over 41 x 67
TARGETS = ((1, 1), (1, 67), (41, 1), (9, 9), (41, 67))


def _build():
    c = {}
    one = flat([(-1, -1), (2, -1), (-1, 2)], [(0, 1, 2)])
    c["one pixel"] = case(one, size=(1, 1))
    c["vertex on a centre"] = case(flat([(2, 2), (5, 2), (2, 5)], [(0, 1, 2)]))
    for k, m in PAIRS.items():
        c[f"pair {k}"] = case(m)
        c[f"pair {k} reversed"] = case(flipped(m))
    c["no centre"] = case(flat([(0.2, 0.2), (0.8, 0.2), (0.2, 0.8)], [(0, 1, 2)]))
    c["zero area"] = case(flat([(0, 0), (2, 2), (4, 4), (1, 1)], [(0, 1, 2), (3, 3, 0)]))
    c["dropped"] = case(_dropped())
    c["larger than the frame"] = case(flat(BIG_TRI, [(0, 1, 2)]))
    c["large edge functions"] = case(_large_edge(), size=(41, 67))
    sq = [(1, 1), (5, 1), (5, 5), (1, 5)]
    c["coincident"] = case(flat(sq + sq, [(4, 5, 6), (0, 1, 2), (0, 2, 3), (4, 6, 7)]))
    c["interpenetrating"] = case(_interpenetrating())
    facing = flat(sq, [(0, 1, 2), (0, 3, 2)])                           # face 0 has A > 0 (back), face 1 A < 0 (front)
    for cull in raster.CULL:
        c[f"cull {cull}"] = case(facing, cull=cull)
    c["no faces"] = case(dict(one, faces=np.zeros((0, 3), np.int32)))
    c["empty"] = case(flat(np.zeros((0, 2)), np.zeros((0, 3))))
    c["bare"] = case(dict(vertices=one["vertices"], faces=one["faces"]), size=(1, 1))
    ell = lambda: ms.reference("ellipsoid", ms.ellipsoid())
    for cull in ("none", "back"):
        c[f"ellipsoid {cull}"] = lambda cull=cull: case(ell(), ELL_CAM, ELL_POSE, (41, 41), cull=cull)
    c["ellipsoid nan"] = lambda: case(_planted_nan(), ELL_CAM, ELL_POSE, (41, 41))
    c["ellipsoid want"] = lambda: case(ell(), ELL_CAM, ELL_POSE, (41, 41), want=("bary", "normal"))
    c["ellipsoid depth only"] = lambda: case(ell(), ELL_CAM, ELL_POSE, (41, 41), want=())
    for holes in (False, True):
        c[f"planted {holes}"] = lambda holes=holes: case(ms.reference(("planted", holes), ms.planted(holes)), PLANTED_CAM, None, (41, 67))
    c["plane"] = lambda: case(ms.reference("plane", ms.plane()), fs.CAM, None, fs.SIZE)
    for dims in ((5, 7, 9), ms.BIG):
        for V in (1, 3, 8):
            m = lambda dims=dims, V=V: ms.reference(("scene", dims, V, 2), ms.scene_field(dims, V, 2))
            c[f"scene {dims} {V}"] = lambda m=m: case(m(), fs.CAM, None, fs.SIZE)
    big = lambda: ms.reference(("scene", ms.BIG, 8, 2), ms.scene_field(ms.BIG, 8, 2))
    for size in TARGETS:
        c[f"target {size}"] = lambda size=size: case(big(), fs.CAM, None, size)
    c["target pipeline"] = lambda: case(big(), PIPE, None, (147, 147))  # 1 m away a voxel is ~70 pixels: triangles larger than the frame
    c["lattice"] = lambda: case(ms.reference("lattice", ms.lattice_field()), rs.SRC, rs.reference_pose(), fs.SIZE)
    return c


CASES = _build()
HAND = tuple(k for k, v in CASES.items() if isinstance(v, dict))


def get(name):
    if name not in _CACHE:
        c = CASES[name]
        _CACHE[name] = c if isinstance(c, dict) else c()
    return _CACHE[name]


_REFS = {}


def reference(name, dtype=np.float32):
    """raster.render of a case, once; nothing changes it afterwards."""
    key = (name, np.dtype(dtype).name)
    if key not in _REFS:
        c = get(name)
        _REFS[key] = raster.render(c["mesh"], c["cam"], c["pose"], c["size"], dtype=dtype, **c["kw"])
    return _REFS[key]


def fragment_counts(name):
    """The number of fragments per pixel [Ho,Wo], before the z-buffer."""
    c = get(name)
    kw = {k: v for k, v in c["kw"].items() if k != "want"}
    fr = raster.fragments(c["mesh"], c["cam"], c["pose"], c["size"], **kw)
    return np.bincount(fr["pixel"], minlength=c["size"][0] * c["size"][1]).reshape(c["size"])


KEYS = ("depth", "face", "valid", "weight", "feat", "normal", "normal_valid", "bary")


def same(a, b):
    """Two renderings (numpy) are equal in every output: ints and bools as they are, floats as uint32."""
    for k in KEYS:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (k, int((x != y).sum()))
    return True
