"""CPU tests of the statement of mesh cleaning (be_hip/components.py), which test_components_gpu.py holds the kernels to bit for bit.

They tie the statement to ground: labels worked by hand, a breadth-first search written here, a closed surface that must be one
component, areas against float64, the compaction against itself, and the purpose of the feature - on the fusion scene with outliers
the floaters are the small components, and dropping them removes every wrong vertex while nearly all others stay."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from be_hip import components
import components_scenes as cs
import mesh_scenes as ms

_F = np.float32


def _bfs_labels(V, faces):
    """The least index of every vertex's component by a plain breadth-first search over vertex-to-vertex adjacency."""
    adj = [[] for _ in range(V)]
    for a, b, c in np.asarray(faces).tolist():
        adj[a] += [b, c]
        adj[b] += [a, c]
        adj[c] += [a, b]
    lab = [-1] * V
    for s in range(V):                                                   # in increasing order: s is the least of what it reaches
        if lab[s] >= 0:
            continue
        lab[s], queue = s, [s]
        while queue:
            nxt = []
            for v in queue:
                for w in adj[v]:
                    if lab[w] < 0:
                        lab[w] = s
                        nxt.append(w)
            queue = nxt
    return np.array(lab, np.int32).reshape(V)


# ------------------------------------------------------------------------------------------ 1. labels
def test_the_hand_worked_cases():
    for name, (m, want) in cs.HAND.items():
        got = cs.labels(name)
        assert got["label"].tolist() == want and got["label"].dtype == np.int32, name
        roots = sorted(set(want))
        assert got["K"] == len(roots) and got["component"].tolist() == [roots.index(l) for l in want], name
        assert got["face_component"].tolist() == [roots.index(want[f[0]]) for f in m["faces"].tolist()], name
        assert got["vertices"].tolist() == [want.count(r) for r in roots] and int(got["triangles"].sum()) == len(m["faces"]), name
    assert cs.labels("three vertices, no face")["K"] == 3 and cs.labels("no vertex")["K"] == 0
    assert cs.labels("two triangles sharing an edge")["triangles"].tolist() == [2]
    assert cs.labels("two triangles sharing a vertex")["triangles"].tolist() == [2]
    assert cs.labels("two disjoint triangles")["triangles"].tolist() == [1, 0, 1]
    assert cs.labels("a repeated index")["triangles"].tolist() == [0, 1, 1]
    assert (cs.labels("a repeated index")["area_q"] == 0).all()          # degenerate faces: no area


def test_an_index_out_of_range_is_refused():
    m = cs.OUT_OF_RANGE
    with pytest.raises(ValueError):
        components.label(6, m["faces"])
    with pytest.raises(ValueError):
        components.clean(m, min_triangles=1)
    with pytest.raises(ValueError):
        components.label(-1, np.zeros((0, 3), np.int32))
    got = components.select(m, np.ones(6, bool))                        # select alone drops such a face
    assert got["face_index"].tolist() == [0, 3]


@pytest.mark.parametrize("name", cs.ALL, ids=str)
def test_labels_equal_a_breadth_first_search(name):
    m, got = cs.get(name), cs.labels(name)
    V = len(m["vertices"])
    want = _bfs_labels(V, m["faces"])
    assert np.array_equal(got["label"], want), name
    roots = np.flatnonzero(want == np.arange(V))
    assert got["K"] == len(roots) and np.array_equal(roots[got["component"]], want)
    assert int(got["triangles"].sum()) == len(m["faces"]) and int(got["vertices"].sum()) == V


def test_the_strips_and_soups():
    for order in ("ascending", "descending", "permuted"):
        got = cs.labels(f"strip {order} 1")
        assert got["K"] == 1 and not got["label"].any() and got["triangles"].tolist() == [cs.STRIP]
    two = cs.labels("strip permuted 2")
    assert two["K"] == 2 and two["triangles"].tolist() == [cs.STRIP // 2] * 2
    assert cs.labels("soup")["K"] == cs.SOUP and 3 * cs.SOUP > 262144
    joined = cs.labels("soup joined")
    assert joined["K"] == cs.SOUP - cs.SOUP // 3 and joined["triangles"].max() == 3
    assert cs.labels("twins")["triangles"].tolist() == [40, 40, 39]


def test_the_ellipsoid_is_one_component():
    got = cs.labels("ellipsoid")
    assert got["K"] == 1 and got["triangles"].tolist() == [1972]


# ------------------------------------------------------------------------------------------ 2. areas
def _plane_areas():
    m, got = cs.get("plane"), cs.labels("plane")
    v, f = m["vertices"].astype(np.float64), m["faces"]
    each = 0.5 * np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    return got, each, np.bincount(got["face_component"], each, got["K"])


def test_the_area_of_the_plane():
    """The area of the plane's mesh against the float64 sum of its triangles' areas, within 1e-6 relative.  The plane is one component
    of 11408 faces of 3.94e-5 m^2 on average.  q truncates each face to a multiple of 2^-40 = 9.1e-13 m^2, half of that lost per face
    on average: 1.2e-8 of a face.  The float32 evaluation costs a few 2^-24.  Measured: 7.8e-9 relative low.  (A unit of 2^-30 m^2
    loses 1.2e-5 of such a face, measured 1.03e-5: it cannot meet this bound, which is why the unit is 2^-40.)"""
    got, each, want = _plane_areas()
    print(f"plane: {len(each)} faces of {each.mean():.3e} m^2 in {got['K']} component(s); area {got['area'].max():.8f} against {want.max():.8f} m^2, "
          f"relative error {np.abs(got['area'] - want).max() / want.max():.2e}")
    assert np.abs(got["area"][want > 0] / want[want > 0] - 1).max() < 1e-6


def test_the_area_of_the_plane_within_its_truncation():
    """What the statement's own arithmetic allows: every face loses less than one unit of 2^-40 m^2 to truncation and nothing is ever
    gained by it; the float32 evaluation of a face's area (three differences, six products, an addition of squares, a square root:
    a dozen roundings of 2^-24 each) stays within 1e-6 relative."""
    got, each, want = _plane_areas()
    assert got["area"].dtype == np.float64 and got["area_q"].dtype == np.int64 and got["K"] == 1
    faces, unit = got["triangles"].astype(np.float64), 2.0 ** -components.AREA_BITS
    assert components.AREA_BITS == 40 and components.AREA_MAX == 2.0 ** 22
    assert (got["area"] <= want * (1 + 1e-6)).all() and (got["area"] >= want * (1 - 1e-6) - faces * unit).all()
    assert np.array_equal(got["area"], got["area_q"] * unit)


def test_an_area_that_is_not_finite_counts_as_zero():
    m = cs.bare([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.inf, 0, 0], [3e19, 0, 0], [0, 3e19, 0], [np.nan, 1, 1]],
                [[0, 1, 2], [0, 1, 3], [0, 4, 5], [0, 1, 6]])
    q = components.face_area_q(m["vertices"], m["faces"])
    assert q.tolist() == [1 << 39, 0, 0, 0]                             # 0.5 m^2; inf - inf, an overflowing product, NaN
    big = cs.bare([[0, 0, 0], [1e6, 0, 0], [0, 1e6, 0]], [[0, 1, 2]])
    assert components.face_area_q(big["vertices"], big["faces"]).tolist() == [1 << 62]   # 5e11 m^2, clamped to 2^22


# ------------------------------------------------------------------------------------------ 3. decide
def test_decide():
    st = dict(triangles=np.array([40, 3, 40, 0], np.int32), area_q=np.array([5 << 40, 1 << 30, 9 << 40, 0], np.int64))
    d = components.decide
    assert d(st, min_triangles=1).tolist() == [True, True, True, False]
    assert d(st, min_triangles=0).tolist() == [True] * 4
    assert d(st, min_triangles=4).tolist() == [True, False, True, False]
    assert d(st, min_area=6.0).tolist() == [False, False, True, False]
    assert d(st, min_area=2.0 ** -10).tolist() == [True, True, True, False]
    assert d(st, min_triangles=4, min_area=6).tolist() == [False, False, True, False]
    assert d(st, largest=True).tolist() == [True, False, False, False]  # the tie goes to the lowest id
    assert d(st, min_area=6, largest=True).tolist() == [False, False, True, False]
    assert d(st, min_triangles=41, largest=True).tolist() == [False] * 4
    assert components.area_threshold(1e-3) == int(float(_F(1e-3)) * 2 ** 40) and components.area_threshold(3e38) == 2 ** 63 - 1
    for bad in (dict(), dict(min_triangles=-1), dict(min_triangles=1 << 31), dict(min_triangles=2.5), dict(min_triangles=True),
                dict(min_area=-1e-3), dict(min_area=float("nan")), dict(min_area=float("inf")), dict(min_area="much")):
        with pytest.raises(ValueError):
            d(st, **bad)


# ------------------------------------------------------------------------------------------ 4. select and clean
def test_select_everything_and_nothing():
    for name in ("planted", ("outlier", cs.SMALL, 5, 2, True), "two disjoint triangles", "no vertex"):
        m = cs.get(name)
        V, T = len(m["vertices"]), len(m["faces"])
        got = components.select(m, np.ones(V, bool))
        assert cs.same(got, m, cs.KEYS) and got["vertex_index"].tolist() == list(range(V)) and got["face_index"].tolist() == list(range(T))
        none = components.select(m, np.zeros(V, bool))
        assert none["vertices"].shape == (0, 3) and none["faces"].shape == (0, 3) and none["faces"].dtype == np.int32
        assert none["vertex_index"].shape == (0,) and none["face_index"].shape == (0,)
        for k in components.PER_VERTEX:
            assert (none[k] is None) == (m[k] is None), k
        if m["feat"] is not None:
            assert none["feat"].shape == (2, 0) and none["normal"].shape == (0, 3) and none["edge"].dtype == np.int64
    with pytest.raises(ValueError):
        components.select(cs.get("one triangle"), np.ones(2, bool))
    with pytest.raises(ValueError):
        components.select(cs.get("one triangle"), np.ones(3, np.uint8))


def test_select_gathers_every_array():
    m = cs.get("planted")
    V = len(m["vertices"])
    keep = np.random.default_rng(2).random(V) < 0.7
    got = components.select(m, keep)
    vi, fi = got["vertex_index"], got["face_index"]
    assert np.array_equal(vi, np.flatnonzero(keep)) and np.array_equal(fi, np.flatnonzero(keep[m["faces"]].all(1))) and 0 < len(fi) < len(m["faces"])
    assert np.array_equal(vi[got["faces"]], m["faces"][fi])             # a kept face names the vertices it named
    for k in ("vertices", "weight", "normal", "normal_valid", "edge"):
        assert np.array_equal(got[k], m[k][vi], equal_nan=k != "edge" and k != "normal_valid"), k
    assert np.array_equal(got["feat"], m["feat"][:, vi])


def test_clean_is_idempotent():
    for name, kw in ((("outlier", ms.BIG, 5, 2, True), dict(min_triangles=50)), ("twins", dict(largest=True)),
                     ("soup joined", dict(min_triangles=2, min_area=1e-6))):
        once = components.clean(cs.get(name), **kw)
        twice = components.clean(once, **kw)
        assert cs.same(twice, once, cs.KEYS) and len(once["faces"]) > 0, name
        assert twice["components"]["keep"].all() and twice["components"]["triangles"].sum() == len(once["faces"])
        assert np.array_equal(twice["vertex_index"], np.arange(len(once["vertices"])))
    tw = components.clean(cs.get("twins"), largest=True)
    assert tw["components"]["keep"].tolist() == [True, False, False] and len(tw["faces"]) == 40 and not tw["component"].any()
    with pytest.raises(ValueError):
        components.clean(cs.get("twins"))


# ------------------------------------------------------------------------------------------ 5. what it is for
@pytest.mark.parametrize("views", [5, 8])
def test_the_floaters_are_the_small_components(views):
    """The fusion scene with outliers in the (33, 40, 65) volume: every wrong-surface vertex sits in a component of fewer than 50
    triangles.  Measured: 88 -> 0 wrong vertices, RMSE 2.37 -> 0.53 cm, 98.8 % of the vertices kept at 5 views; 38 -> 0, 1.48 ->
    0.42 cm, 99.5 % at 8."""
    m = cs.get(("outlier", ms.BIG, views, 2, True))
    before = ms.quality(m)
    out = components.clean(m, min_triangles=50)
    after = ms.quality(out)
    tri = np.sort(out["components"]["triangles"])[::-1]
    print(f"{views} views: {len(m['faces'])} triangles in {len(tri)} components {tri[:6].tolist()}; wrong {before['wrong']} -> {after['wrong']}, "
          f"RMSE {100 * before['rmse']:.2f} -> {100 * after['rmse']:.2f} cm, {len(out['vertices'])} of {len(m['vertices'])} vertices kept")
    assert before["wrong"] >= 30 and after["wrong"] == 0
    assert after["rmse"] < 0.006
    assert len(out["vertices"]) >= 0.98 * len(m["vertices"])
    assert int(out["components"]["keep"].sum()) == 2                     # the two true surfaces: the square and the wall
    clean = cs.get(("scene", ms.BIG, views, 2, True))                   # without outliers the same filter changes next to nothing
    assert abs(ms.quality(components.clean(clean, min_triangles=50))["rmse"] - ms.quality(clean)["rmse"]) < 1e-4


# ------------------------------------------------------------------------------------------ 6. the plumbing
def test_the_abi_is_declared_exported_and_refuses_bad_arguments():
    from be_hip import native
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    names = ("be_mesh_components_workspace_bytes", "be_mesh_components_i32", "be_mesh_components_stats", "be_mesh_components_decide",
             "be_mesh_select_workspace_bytes", "be_mesh_select_count", "be_mesh_select_emit")
    for name in names:
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    assert f"#define BE_COMPONENTS_AREA_BITS {components.AREA_BITS}\n" in hdr
    o = native.ops()
    for name in ("mesh_components", "mesh_components_stats", "mesh_components_decide", "mesh_select_count", "mesh_select"):
        assert hasattr(o, name), name
    scan = lib.be_exclusive_scan_workspace_bytes
    assert lib.be_mesh_components_workspace_bytes(10) == 40 + 16 + scan(10) and lib.be_mesh_components_workspace_bytes(0) == scan(0) == 8
    assert lib.be_mesh_components_workspace_bytes(-1) == 0 and lib.be_mesh_components_workspace_bytes(1 << 31) == 0
    assert lib.be_mesh_select_workspace_bytes(10, 3) == 16 + 8 + scan(10) and lib.be_mesh_select_workspace_bytes(3, -1) == 0
    # every refusal below returns before a launch: no GPU is touched
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    assert lib.be_mesh_components_i32(p, -1, 0, p, p, p, p, p, 512, None) != 0
    assert lib.be_mesh_components_i32(p, 4, 1 << 31, p, p, p, p, p, 512, None) != 0
    assert lib.be_mesh_components_i32(p, 4, 1, p, p, p, None, p, 512, None) != 0
    assert lib.be_mesh_components_i32(p, 4, 1, p, p, p, p, odd, 512, None) != 0
    assert lib.be_mesh_components_i32(p, 4, 1, p, p, p, p, p, 8, None) != 0
    assert b"workspace" in lib.be_last_error()
    assert lib.be_mesh_components_stats(p, p, 4, 1, p, 5, p, p, p, None) != 0            # Kcap > V
    assert lib.be_mesh_components_decide(p, p, p, 4, -1, 0.0, 0, p, None, 0, None, p, 8, None) != 0
    assert lib.be_mesh_components_decide(p, p, p, 4, 1, float("nan"), 0, p, None, 0, None, p, 8, None) != 0
    assert lib.be_mesh_components_decide(p, p, p, 4, 1, 0.0, 0, p, None, 3, p, p, 8, None) != 0   # vertex_keep without component
    assert lib.be_mesh_components_decide(p, p, p, 4, 1, 0.0, 0, p, None, 0, None, p, 4, None) != 0
    assert lib.be_mesh_select_count(p, 4, 1, p, p, p, p, p, 8, None) != 0
    emit = lambda **kw: lib.be_mesh_select_emit(*[dict(dict(vertices=p, faces=p, V=4, T=1, weight=None, feat=None, C=0, normal=None, normal_valid=None,
                                                             edge=None, component=None, vertex_keep=p, voff=p, foff=p, V2=2, T2=0, vertices_out=p,
                                                             faces_out=None, weight_out=None, feat_out=None, normal_out=None, normal_valid_out=None,
                                                             edge_out=None, component_out=None, vertex_index=p, face_index=None, stream=None), **kw)[k]
                                                  for k in ("vertices", "faces", "V", "T", "weight", "feat", "C", "normal", "normal_valid", "edge",
                                                            "component", "vertex_keep", "voff", "foff", "V2", "T2", "vertices_out", "faces_out",
                                                            "weight_out", "feat_out", "normal_out", "normal_valid_out", "edge_out", "component_out",
                                                            "vertex_index", "face_index", "stream")])
    for bad in (dict(V2=5), dict(T2=2), dict(C=65), dict(weight=p), dict(edge_out=p), dict(C=1), dict(vertices_out=None), dict(T2=1)):
        assert emit(**bad) != 0, bad


def test_the_wrappers_refuse_what_is_not_on_the_gpu():
    import torch
    from be_hip import native
    m = {k: None if v is None else torch.from_numpy(v) for k, v in cs.get("planted").items()}
    for call in (lambda: native.mesh_components(m), lambda: native.mesh_select(m, torch.ones(len(m["vertices"]), dtype=torch.bool)),
                 lambda: native.mesh_clean(m, min_triangles=1), lambda: native.mesh_components(cs.get("planted")),
                 lambda: native.mesh_clean(m), lambda: native.mesh_components(dict(m, edge=m["edge"][:-1])),
                 lambda: native.mesh_components(dict(m, faces=m["faces"].long())), lambda: native.mesh_components([1])):
        with pytest.raises(ValueError):
            call()
