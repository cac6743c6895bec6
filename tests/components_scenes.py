"""The meshes the mesh-cleaning tests share (test_components_cpu.py, test_components_gpu.py): cases worked by hand, strips and soups
chosen for the union-find's races and the scan's boundaries, the meshes of mesh_scenes, and the fusion scene WITH outliers - the
floaters the feature removes.  Everything is numpy and is computed once; nothing changes a mesh afterwards."""
import numpy as np

from be_hip import components, mesh, volume
import fuse_scenes as fs
import mesh_scenes as ms

_F = np.float32
_CACHE = {}
KEYS = ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge")


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bare(vertices, faces):
    """A mesh of positions and faces alone."""
    return dict(vertices=np.asarray(vertices, _F).reshape(-1, 3), faces=np.asarray(faces, np.int32).reshape(-1, 3), weight=None, feat=None,
                normal=None, normal_valid=None, edge=None)


def _grid(V):
    """V positions with some area between any three of them: a lattice 37 wide, bent."""
    i = np.arange(V)
    return np.stack([(i % 37) * 0.01, (i // 37) * 0.013, 0.002 * ((i * 7) % 5)], 1).astype(_F)


# name -> (mesh, labels worked by hand)
HAND = {
    "no vertex": (bare(np.zeros((0, 3)), np.zeros((0, 3))), []),
    "three vertices, no face": (bare(_grid(3), np.zeros((0, 3))), [0, 1, 2]),
    "one triangle": (bare(_grid(3), [[0, 1, 2]]), [0, 0, 0]),
    "two triangles sharing an edge": (bare(_grid(4), [[0, 1, 2], [2, 1, 3]]), [0, 0, 0, 0]),
    "two triangles sharing a vertex": (bare(_grid(5), [[0, 1, 2], [2, 3, 4]]), [0, 0, 0, 0, 0]),
    "two disjoint triangles": (bare(_grid(7), [[4, 5, 6], [0, 1, 2]]), [0, 0, 0, 3, 4, 4, 4]),
    "a repeated index": (bare(_grid(4), [[1, 1, 3], [2, 2, 2]]), [0, 1, 2, 1]),
}
OUT_OF_RANGE = bare(_grid(6), [[0, 1, 2], [3, 4, 6], [3, -1, 5], [4, 5, 5]])        # faces 1 and 2 name what is not there
OUT_OF_RANGE_FACES = (1, 2)

STRIP = 70000                                                           # triangles; 274 workgroups of 256 faces


def strip(order="ascending", stride=1):
    """STRIP triangles (i, i + s, i + 2 s) over STRIP + 2 s vertices: one component for s = 1, two interleaved ones for s = 2.  order
    renames the vertices: ascending (the identity), descending, or permuted by default_rng(21) - deep trees, and unions that meet
    across waves and workgroups."""
    def make():
        V = STRIP + 2 * stride
        i = np.arange(STRIP)
        faces = np.stack([i, i + stride, i + 2 * stride], 1)
        name = dict(ascending=np.arange(V), descending=np.arange(V)[::-1], permuted=np.random.default_rng(21).permutation(V))[order]
        pos = np.empty((V, 3), _F)
        pos[name] = _grid(V)
        return bare(pos, name[faces])
    return _once(("strip", order, stride), make)


SOUP = 90000                                                            # triangles; 270000 vertices: past the scan's 262144


def soup(joined=False):
    """SOUP disjoint triangles (3 t, 3 t + 1, 3 t + 2); joined: every third triangle also shares a vertex with its neighbour, by a
    further face (3 t + 2, 3 t + 3, 3 t + 3)."""
    def make():
        t = np.arange(SOUP)
        faces = np.stack([3 * t, 3 * t + 1, 3 * t + 2], 1)
        if joined:
            j = t[:-1:3]
            faces = np.concatenate([faces, np.stack([3 * j + 2, 3 * j + 3, 3 * j + 3], 1)])
        return bare(_grid(3 * SOUP), faces)
    return _once(("soup", joined), make)


def twins():
    """Two equal strips of 40 triangles and a third of 39: a tie for the largest."""
    def make():
        faces, base = [], 0
        for n in (40, 40, 39):
            i = np.arange(n) + base
            faces.append(np.stack([i, i + 1, i + 2], 1))
            base += n + 2
        return bare(_grid(base), np.concatenate(faces))
    return _once("twins", make)


def outlier_volume(dims, V):
    """mesh_scenes.scene_volume's volume, integrated from the views WITH outliers: 2 % of each view's samples 0.3 m forward."""
    return _once(("outlier volume", dims, V),
                 lambda: volume.integrate(volume.Volume(C=2, **ms.describe(dims)), fs.scene(V, outliers=True, C=2), fs.NEAR))


def outlier_field(dims, V):
    return _once(("outlier field", dims, V), lambda: ms._of_volume(outlier_volume(dims, V)))


def _extract(f, normals=True):
    return mesh.extract(f["D"], f["W"], f["Fm"], f["origin"], f["voxel"], 0.0, normals)


def field_mesh(name):
    """The meshes out of fields, by name."""
    def make():
        if name == "ellipsoid":
            return _extract(ms.ellipsoid())
        if name == "planted":
            return _extract(ms.planted(True))
        if name == "lattice":
            return _extract(ms.lattice_field())
        if name == "plane":
            return _extract(ms.plane())
        kind, dims, V, C, normals = name
        f = ms.scene_field(dims, V) if kind == "scene" else outlier_field(dims, V)
        return _extract(f if C == 2 else dict(f, Fm=None), normals)
    return _once(("mesh", name), make)


SMALL = (5, 7, 9)
# (kind, dims, views, channels, normals): both volumes with and without outliers at 1 / 5 / 8 views; 0 channels and no normals once each
FIELD_NAMES = ["ellipsoid", "planted", "lattice"] + [(kind, dims, V, 2, True) for kind in ("scene", "outlier") for dims in (SMALL, ms.BIG)
                                                      for V in (1, 5, 8)] + [("outlier", ms.BIG, 5, 0, True), ("outlier", ms.BIG, 8, 2, False)]


def get(name):
    if name in HAND:
        return HAND[name][0]
    if isinstance(name, str) and name.startswith("strip"):
        _, order, stride = name.split()
        return strip(order, int(stride))
    if name in ("soup", "soup joined"):
        return soup(name == "soup joined")
    if name == "twins":
        return twins()
    return field_mesh(name)


SYNTHETIC = ["strip ascending 1", "strip descending 1", "strip permuted 1", "strip permuted 2", "soup", "soup joined", "twins"]
ALL = list(HAND) + SYNTHETIC + FIELD_NAMES
_REF = {}


def labels(name):
    """components.label and stats of a named mesh, once -> dict(label, component, face_component, K, triangles, vertices, area_q, area)."""
    if name not in _REF:
        m = get(name)
        lab = components.label(len(m["vertices"]), m["faces"])
        _REF[name] = dict(lab, **components.stats(m, lab))
    return _REF[name]


def same(a, b, keys):
    """Two results (numpy) are equal in every named output: ints as ints, float32 as uint32, float64 as uint64."""
    for k in keys:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype.kind == "f":
            x, y = x.view(f"u{x.dtype.itemsize}"), y.view(f"u{y.dtype.itemsize}")
        assert np.array_equal(x, y), (k, int((x != y).sum()))
    return True


LABEL_KEYS = ("label", "component", "face_component", "triangles", "vertices", "area_q", "area")
SELECT_KEYS = KEYS + ("vertex_index", "face_index")
