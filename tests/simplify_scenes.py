"""The meshes and grids the mesh-simplification tests share (test_simplify_cpu.py, test_simplify_gpu.py): cases worked by hand, the
strips and soups of components_scenes under grids chosen for the hash tables' races and the scan's boundaries, a flap mesh for the
face table, and the field meshes of components_scenes / mesh_scenes under cells of 1, 2 and 3 voxels.  Nothing is copied: the
meshes are components_scenes' own.  Everything is numpy and is computed once; nothing changes a mesh or a result afterwards."""
import numpy as np

from be_hip import simplify
import components_scenes as cs
import mesh_scenes as ms

_F = np.float32
_CACHE = {}
KEYS = ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge", "cluster", "members", "face_index")
CLUSTER_KEYS = ("label", "cluster", "members")
H = 0.5                                                                 # the other two coordinates of the hand-worked vertices: mid-cell


def weighted(vertices, faces, weight):
    return dict(cs.bare(vertices, faces), weight=np.asarray(weight, _F))


def _x(*xs):
    """Vertices at the given X, mid-cell in Y and Z."""
    return [(x, H, H) for x in xs]


NAN, INF = float("nan"), float("inf")
BELOW_ONE = float(np.nextafter(_F(1), _F(0)))                            # 1 - 2^-24: r of the last position of cell 0, q = 2^24 - 1

# name -> (mesh, kw of simplify beside cell = 1 and origin = 0, the answer worked by hand: cluster, members, the old indices of the
# faces that stay, and - where they are exact - the new positions)
HAND = {
    "no vertex": (cs.bare(np.zeros((0, 3)), np.zeros((0, 3))), {}, dict(cluster=[], members=[], face_index=[], vertices=[])),
    "three vertices, no face": (cs.bare([(0.5, H, H), (1.5, H, H), (0.25, 0.25, 0.25)], np.zeros((0, 3))), {},
                                dict(cluster=[0, 1, 0], members=[2, 1], face_index=[], vertices=[(0.375, 0.375, 0.375), (1.5, H, H)])),
    "one triangle inside one cell": (cs.bare([(0.125, 0.125, 0.125), (0.875, 0.125, 0.125), (0.125, 0.875, 0.125)], [[0, 1, 2]]), {},
                                     dict(cluster=[0, 0, 0], members=[3], face_index=[])),
    "two triangles across four cells": (cs.bare([(0.5, 0.5, H), (1.5, 0.5, H), (0.5, 1.5, H), (1.5, 1.5, H)], [[0, 1, 2], [2, 1, 3]]), {},
                                        dict(cluster=[0, 1, 2, 3], members=[1, 1, 1, 1], face_index=[0, 1],
                                             vertices=[(0.5, 0.5, H), (1.5, 0.5, H), (0.5, 1.5, H), (1.5, 1.5, H)])),
    # 1.0 is the first position of cell 1 (r = 0), the float32 below it the last of cell 0
    "a vertex on a cell boundary": (cs.bare(_x(1.0, BELOW_ONE, 2.0, 1.5), np.zeros((0, 3))), {},
                                    dict(cluster=[0, 1, 2, 0], members=[2, 1, 1], face_index=[], vertices=_x(1.25, BELOW_ONE, 2.0))),
    # floorf(-0.5) = floorf(-1.0) = -1, floorf(-1.5) = -2: cells reach from their index upwards on the negative side too
    "negative coordinates": (cs.bare([(-0.5, -0.5, -0.5), (-1.0, -0.5, -0.5), (-1.5, -0.5, -0.5)], np.zeros((0, 3))), {},
                             dict(cluster=[0, 0, 1], members=[2, 1], face_index=[], vertices=[(-0.75, -0.5, -0.5), (-1.5, -0.5, -0.5)])),
    # |i| < 2^20: 2^20 is out, 2^20 - 1 in; -2^20 out, -(2^20 - 1) in
    "the last cell index": (cs.bare(_x(1048576.5, 1048575.5, -1048575.5, -1048574.5), [[1, 3, 0], [1, 3, 2]]), {},
                            dict(cluster=[-1, 0, -1, 1], members=[1, 1], face_index=[], vertices=_x(1048575.5, -1048574.5))),
    "positions that are not finite": (cs.bare([(NAN, H, H), (0.5, H, H), (0.5, INF, H), (0.5, H, -INF), (2.5, H, H)], [[0, 1, 4], [1, 4, 2]]), {},
                                      dict(cluster=[-1, 0, -1, -1, 1], members=[1, 1], face_index=[], vertices=_x(0.5, 2.5))),
    # wq = 65536, 0, 0, 0, 2^20 (an infinite weight clamps to 16): X' = (0.25 + 16 * 0.75) / 17, weight' = (1 + 16) / 2
    "weights 0, negative, NaN and infinite": (weighted(_x(0.25, 0.5, 0.5, 0.5, 0.75), np.zeros((0, 3)), [1, 0, -1, NAN, INF]), {},
                                              dict(cluster=[0, -1, -1, -1, 0], members=[2], face_index=[], weight=[8.5])),
    "a repeated index": (cs.bare(_x(0.5, 1.5, 2.5), [[0, 0, 1], [2, 1, 2], [0, 1, 2]]), {},
                         dict(cluster=[0, 1, 2], members=[1, 1, 1], face_index=[2])),
    "five copies of one face": (cs.bare(_x(0.5, 1.5, 2.5), [[1, 2, 0], [0, 1, 2], [2, 0, 1], [0, 1, 2], [1, 2, 0]]), {},
                                dict(cluster=[0, 1, 2], members=[1, 1, 1], face_index=[0])),
    "both windings, no flaps": (cs.bare(_x(0.5, 1.5, 2.5, 3.5), [[0, 1, 2], [0, 2, 1], [2, 1, 0], [1, 2, 0], [1, 2, 3]]), dict(flaps=False),
                                dict(cluster=[0, 1, 2, 3], members=[1, 1, 1, 1], face_index=[4])),
    "both windings, flaps": (cs.bare(_x(0.5, 1.5, 2.5, 3.5), [[0, 1, 2], [0, 2, 1], [2, 1, 0], [1, 2, 0], [1, 2, 3]]), dict(flaps=True),
                             dict(cluster=[0, 1, 2, 3], members=[1, 1, 1, 1], face_index=[0, 1, 4])),
    # cells 7, 3, 5, 7, 9, 5 -> labels 0, 1, 2, 0, 4, 2: the clusters are numbered by their least member, not by their cell
    "labels numbered by the least member": (cs.bare(_x(7.5, 3.5, 5.5, 7.25, 9.5, 5.25), [[0, 1, 2], [3, 4, 5]]), {},
                                            dict(cluster=[0, 1, 2, 0, 3, 2], members=[2, 1, 2, 1], face_index=[0, 1], label=[0, 1, 2, 0, 4, 2],
                                                 vertices=_x(7.375, 3.5, 5.375, 9.5))),
}
# faces 1 and 2 name what is not there: the statement refuses them, the kernels ignore them
OUT_OF_RANGE = cs.bare(_x(0.5, 1.5, 2.5, 3.5), [[0, 1, 2], [0, 1, 4], [3, -1, 2], [1, 2, 3]])
OUT_OF_RANGE_FACES = (1, 2)

FLAPS = 5000


def flap_mesh():
    """FLAPS faces over 30 vertices in three cells, each naming one vertex of every cell, in a winding and at a rotation drawn by
    default_rng(31): every face has the triple (0, 1, 2), and both windings occur thousands of times."""
    def make():
        rng = np.random.default_rng(31)
        cell = np.arange(30) % 3                                        # vertex v lies in cell v % 3
        pos = np.stack([cell + 0.1 + 0.8 * rng.random(30), 0.1 + 0.8 * rng.random(30), 0.1 + 0.8 * rng.random(30)], 1)
        corners = 3 * rng.integers(0, 10, (FLAPS, 3)) + np.arange(3)    # one vertex of cell 0, 1, 2
        flip = rng.random(FLAPS) < 0.5
        corners[flip] = corners[flip][:, ::-1]
        roll = rng.integers(0, 3, FLAPS)
        faces = np.stack([corners[np.arange(FLAPS), (k + roll) % 3] for k in range(3)], 1)
        return cs.bare(pos, faces)
    return cs._once("flap mesh", make)


# the lattice of components_scenes._grid: 37 positions 0.01 apart in X, rows 0.013 apart in Y, Z in [0, 0.008]
_ROW = (0.01, 0.013, 1.0)
_BACK = (-0.005, -0.0065, -0.5)                                          # half a position back: no vertex near a cell boundary
# name -> (the mesh's name in components_scenes, cell, origin)
SYNTHETIC = {
    "strip in one cell": ("strip ascending 1", 100.0, (-1.0, -1.0, -1.0)),
    "strip ascending, cells of four": ("strip ascending 1", (0.04, 0.013, 1.0), _BACK),
    "strip descending, cells of four": ("strip descending 1", (0.04, 0.013, 1.0), _BACK),
    "strip permuted, cells of four": ("strip permuted 1", (0.04, 0.013, 1.0), _BACK),
    "soup, a cell per vertex": ("soup", _ROW, _BACK),
    "soup, cells that join neighbours": ("soup", (0.02, 0.026, 1.0), _BACK),
    "soup joined, cells that join neighbours": ("soup joined", (0.02, 0.026, 1.0), _BACK),
}


def field_of(name):
    """The field a mesh of components_scenes.FIELD_NAMES came out of: its origin and voxel are the grid's."""
    if name in ("ellipsoid", "planted", "lattice", "plane"):
        return dict(ellipsoid=ms.ellipsoid, planted=lambda: ms.planted(True), lattice=ms.lattice_field, plane=ms.plane)[name]()
    kind, dims, V, _, _ = name
    return ms.scene_field(dims, V) if kind == "scene" else cs.outlier_field(dims, V)


def grid_of(name, k, shift=False):
    """(cell, origin) of k voxels of the mesh's field, from the field's origin or half a cell further."""
    f = field_of(name)
    cell = tuple(k * float(v) for v in f["voxel"])
    return cell, tuple(float(o) + (0.5 * c if shift else 0.0) for o, c in zip(f["origin"], cell))


CELLS, SHIFTS = (1, 2, 3), (False, True)


def case(name):
    """(mesh, cell, origin, flaps) of a named case: a hand-worked one, a synthetic one, "flaps" / "flaps kept", or (a field mesh's
    name, voxels per cell, shifted)."""
    if name in HAND:
        m, kw, _ = HAND[name]
        return m, 1.0, (0.0, 0.0, 0.0), kw.get("flaps", False)
    if name in SYNTHETIC:
        src, cell, origin = SYNTHETIC[name]
        return cs.get(src), cell, origin, False
    if name in ("flaps", "flaps kept"):
        return flap_mesh(), 1.0, (0.0, 0.0, 0.0), name == "flaps kept"
    field, k, shift = name
    return (cs.get(field),) + grid_of(field, k, shift) + (False,)


def ref(name):
    """simplify.simplify and simplify.cluster of a named case, once -> the simplified mesh with label beside it."""
    def make():
        m, cell, origin, flaps = case(name)
        out = simplify.simplify(m, cell, origin, flaps)
        lab = simplify.cluster(m, cell, origin)
        assert np.array_equal(lab["cluster"], out["cluster"]) and np.array_equal(lab["members"], out["members"]) and lab["V"] == len(out["vertices"])
        return dict(out, label=lab["label"])
    return cs._once(("simplified", name), make)


FIELD_CASES = [(f, k, s) for f in cs.FIELD_NAMES for k in CELLS for s in SHIFTS]
ALL = list(HAND) + list(SYNTHETIC) + ["flaps", "flaps kept"] + FIELD_CASES
