"""The fields and volumes the mesh extraction tests share (test_mesh_cpu.py, test_mesh_gpu.py): an ellipsoid, a volume with every
cube code planted, the same with holes, the plane of test_tsdf_cpu.py, the fusion scene's volumes as test_tsdf_gpu.py builds them,
a slanted plane in a volume large enough for the scan's second level, and the score of a mesh against the fusion scene's truth.
Everything is numpy and is computed once."""
import numpy as np

from be_hip import mesh, volume
import fuse_scenes as fs
import reproject_scenes as rs

_F = np.float32
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def field(D, W=None, Fm=None, origin=(0.0, 0.0, 0.0), voxel=(1.0, 1.0, 1.0)):
    D = np.ascontiguousarray(D, _F)
    return dict(D=D, W=np.ones_like(D) if W is None else np.ascontiguousarray(W, _F), Fm=Fm, origin=origin, voxel=voxel)


def ellipsoid():
    """14 x 14 x 14, fully observed: D = sqrt((x - 6.3)^2 + 1.3 (y - 6.6)^2 + 0.8 (z - 6.4)^2) - 4.2 in lattice units: positive outside."""
    def make():
        z, y, x = np.meshgrid(*(np.arange(14.0),) * 3, indexing="ij")
        return field(np.sqrt((x - 6.3) ** 2 + 1.3 * (y - 6.6) ** 2 + 0.8 * (z - 6.4) ** 2) - 4.2)
    return _once("ellipsoid", make)


def planted(holes=False):
    """(2, 2, 512): the cell at ix = 2c has cube code c (corner k = 4 dz + 2 dy + dx positive iff bit k of c), c = 0..255, with
    magnitudes drawn in [0.1, 1] from default_rng(3); the cells at odd ix hold what their neighbours leave them.  Every one of the
    6 x 16 tet cases occurs.  Two channels ride along.  holes: 10 % of W set to 0 by default_rng(4)."""
    def make():
        rng = np.random.default_rng(3)
        D = rng.uniform(0.1, 1.0, (2, 2, 512))
        for c in range(256):
            for k in range(8):
                if not c >> k & 1:
                    D[k >> 2 & 1, k >> 1 & 1, 2 * c + (k & 1)] *= -1
        W = np.ones((2, 2, 512))
        if holes:
            W[np.random.default_rng(4).random((2, 2, 512)) < 0.1] = 0
        Fm = np.random.default_rng(6).standard_normal((2, 2, 2, 512)).astype(_F)
        return field(D, W, Fm, origin=(0.25, -0.5, 1.0), voxel=(0.01, 0.02, 0.03))
    return _once(("planted", holes), make)


# the volume of test_tsdf_cpu.py (the prototype's): 96 x 40 x 56 voxels of (18, 17.5, 6) mm from (-0.5, -0.35, 0.62)
DIMS, ORIGIN, VOXEL, TRUNC = (96, 40, 56), (-0.5, -0.35, 0.62), (0.018, 0.0175, 0.006), 0.04
PLANE_Z = 0.9137


def _of_volume(vol):
    D, W, Fm = volume.mean(vol)
    return field(D, W, Fm if vol.C else None, vol.origin, vol.voxel)


def plane():
    """One identity view of the plane Z = 0.9137 in the prototype's volume at trunc 0.05, as test_tsdf_cpu.py integrates it."""
    def make():
        vol = volume.Volume(DIMS, ORIGIN, VOXEL, 0.05)
        volume.integrate(vol, [dict(depth=np.full(fs.SIZE, PLANE_Z, _F), weight=None, feat=None, cam_src=fs.CAM, pose=None)])
        return _of_volume(vol)
    return _once("plane", make)


def prototype(V):
    """fuse_scenes.scene(V) in the prototype's volume: the volume the ray cast's quality figures come from."""
    return _once(("prototype", V), lambda: _of_volume(volume.integrate(volume.Volume(DIMS, ORIGIN, VOXEL, TRUNC), fs.scene(V), fs.NEAR)))


# (Nz, Ny, Nx) -> trunc, as test_tsdf_gpu.py: every volume spans X in [-0.5, 0.5], Y in [-0.35, 0.35], Z in [0.62, 1.2]
VOLUMES = {(1, 1, 1): 0.5, (1, 5, 5): 0.5, (2, 2, 2): 0.5, (5, 7, 9): 0.2, (33, 40, 65): 0.04}
BIG = (33, 40, 65)


def describe(dims):
    nz, ny, nx = dims
    voxel = (1.0 / nx, 0.7 / ny, 0.58 / nz)
    return dict(dims=dims, origin=(-0.5 + voxel[0] / 2, -0.35 + voxel[1] / 2, 0.62 + voxel[2] / 2), voxel=voxel, trunc=VOLUMES[dims])


def scene_volume(dims, V):
    """fuse_scenes.scene(V, C=2) with its weights in the volume describe(dims) -> the numpy volume."""
    return _once(("scene", dims, V), lambda: volume.integrate(volume.Volume(C=2, **describe(dims)), fs.scene(V, C=2), fs.NEAR))


def scene_field(dims, V, C=2):
    f = _once(("scene field", dims, V), lambda: _of_volume(scene_volume(dims, V)))
    return f if C == 2 else dict(f, Fm=None)


def lattice_views():
    """The rotated reference view of reproject_scenes on the lattices of scale 1, 3 (window origin (5, 7)) and 2, two channels."""
    views = []
    for k in (1, 3, 2):
        scale, win, (Hs, Ws) = rs.LATTICES[k]
        views.append(dict(depth=rs.lattice_depth(k), weight=None, feat=rs.feat_for(Hs, Ws, 2), cam_src=rs.SRC, pose=rs.reference_pose(),
                          scale=scale, window_origin=win[:2]))
    return views


def lattice_field():
    return _once("lattice", lambda: _of_volume(volume.integrate(volume.Volume(C=2, **describe(BIG)), lattice_views(), rs.NEAR)))


SECOND = (5, 230, 230)                                                  # 264500 voxels: past 256 workgroup sums of 1024 elements


def slanted():
    """A plane through a (5, 230, 230) volume, fully observed, slanted so that it crosses every layer: its last layer's voxels lie
    past the 262144 elements one pass of the scan's second level covers."""
    def make():
        z, y, x = np.meshgrid(np.arange(5.0), np.arange(230.0), np.arange(230.0), indexing="ij")
        return field(0.31 * (z - 2.0) + 0.0062 * (x - 115.0) - 0.0011 * (y - 100.0), origin=(-1.0, -1.0, 0.5), voxel=(0.01, 0.01, 0.02))
    return _once("slanted", make)


_MESHES = {}


def reference(name, f, min_weight=0.0, normals=True, dtype=np.float32):
    """mesh.extract once per case; nothing changes it afterwards."""
    key = (name, float(min_weight), bool(normals), np.dtype(dtype).name)
    if key not in _MESHES:
        _MESHES[key] = mesh.extract(f["D"], f["W"], f["Fm"], f["origin"], f["voxel"], min_weight, normals, dtype)
    return _MESHES[key]


def same(a, b):
    """Two meshes (numpy) are equal in every output: ints as ints, floats as uint32."""
    for k in ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge"):
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


# the fusion scene's truth in the frame of view 0: a square at Z = 0.80 over X in (-0.12, 0.10), Y in (-0.08, 0.09), a wall at 1.10
SQUARE, WALL, SQUARE_X, SQUARE_Y = 0.80, 1.10, (-0.12, 0.10), (-0.08, 0.09)
STEP_MARGIN = 0.035                                                     # a pixel at the wall (1.10 / 58 = 19 mm) and a voxel (18 mm) ~


def quality(m):
    """A mesh of the fusion scene scored as fuse_scenes.quality scores a ray cast: the error of a vertex is its Z minus the Z of the
    nearest true surface over its (X, Y) - the wall, or the square where (X, Y) lies under it; vertices within STEP_MARGIN of the
    square's outline in (X, Y) are left out, as quality leaves out the pixels next to the depth step.  -> dict(rmse (metres), wrong =
    the vertices further than 0.15 m from every true surface, vertices = the number scored)."""
    X, Y, Z = (m["vertices"][:, i].astype(np.float64) for i in range(3))
    dx = np.minimum(np.abs(X - SQUARE_X[0]), np.abs(X - SQUARE_X[1]))
    dy = np.minimum(np.abs(Y - SQUARE_Y[0]), np.abs(Y - SQUARE_Y[1]))
    inside = (SQUARE_X[0] < X) & (X < SQUARE_X[1]) & (SQUARE_Y[0] < Y) & (Y < SQUARE_Y[1])
    near_x = (dx < STEP_MARGIN) & (SQUARE_Y[0] - STEP_MARGIN < Y) & (Y < SQUARE_Y[1] + STEP_MARGIN)
    near_y = (dy < STEP_MARGIN) & (SQUARE_X[0] - STEP_MARGIN < X) & (X < SQUARE_X[1] + STEP_MARGIN)
    keep = ~(near_x | near_y)
    e_wall, e_square = Z - WALL, Z - SQUARE
    err = np.where(inside & (np.abs(e_square) < np.abs(e_wall)), e_square, e_wall)[keep]
    return dict(rmse=float(np.sqrt(np.mean(err ** 2))) if err.size else float("nan"), wrong=int((np.abs(err) > 0.15).sum()),
                vertices=int(keep.sum()))
