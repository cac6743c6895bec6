"""CPU tests of the statement of mesh simplification (be_hip/simplify.py), which test_simplify_gpu.py holds the kernels to bit for bit.

They tie the statement to ground: cases worked by hand, a dictionary-based brute force written here, a closed surface that must stay
closed and keep its volume, a plane that must stay a plane, and the purpose of the feature - on the fusion scene the mesh gets many
times coarser while its error against the true surfaces does not grow."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from be_hip import components, fusion, simplify
import components_scenes as cs
import mesh_scenes as ms
import simplify_scenes as ss

_F = np.float32


# ------------------------------------------------------------------------------------------ 1. by hand
@pytest.mark.parametrize("name", list(ss.HAND), ids=str)
def test_the_hand_worked_cases(name):
    m, _, want = ss.HAND[name]
    got = ss.ref(name)
    assert got["cluster"].tolist() == want["cluster"] and got["cluster"].dtype == np.int32
    assert got["members"].tolist() == want["members"] and got["members"].dtype == np.int32
    assert got["face_index"].tolist() == want["face_index"] and got["face_index"].dtype == np.int32
    assert got["vertices"].shape == (len(want["members"]), 3) and got["vertices"].dtype == _F and got["faces"].dtype == np.int32
    assert got["faces"].tolist() == [[want["cluster"][i] for i in m["faces"][f]] for f in want["face_index"]]    # old order, old corner order
    if "vertices" in want:                                              # exact: binary fractions, equal weights
        assert got["vertices"].tolist() == np.asarray(want["vertices"], _F).reshape(-1, 3).tolist()
    if "weight" in want:
        assert got["weight"].tolist() == want["weight"]
    if "label" in want:
        assert got["label"].tolist() == want["label"]
    assert got["edge"] is None and (got["weight"] is None) == (m["weight"] is None) and got["feat"] is None and got["normal"] is None


def test_the_hand_worked_means():
    one = ss.ref("one triangle inside one cell")["vertices"][0]        # (0.125 + 0.875 + 0.125) / 3: within 2^-24 of a cell and a rounding
    assert np.abs(one.astype(np.float64) - [0.375, 0.375, 0.125]).max() <= 2.0 ** -23
    w = ss.ref("weights 0, negative, NaN and infinite")["vertices"][0]
    assert abs(float(w[0]) - (0.25 + 16 * 0.75) / 17) <= 2.0 ** -23 and w[1] == 0.5 and w[2] == 0.5
    flap, kept = ss.ref("flaps"), ss.ref("flaps kept")
    assert len(flap["vertices"]) == 3 and len(flap["faces"]) == 0 and flap["members"].tolist() == [10, 10, 10]
    faces = ss.flap_mesh()["faces"]
    assert kept["face_index"].tolist()[0] == 0 and len(kept["faces"]) == 2
    a, b = (faces[i] % 3 for i in kept["face_index"])                  # the first face and the first of the other winding
    wind = lambda f: (int(f[(np.argmin(f) + 1) % 3]) - int(f[(np.argmin(f) + 2) % 3])) > 0
    assert wind(a) != wind(b) and all(wind(faces[i] % 3) == wind(a) for i in range(kept["face_index"][1]))


def test_an_index_out_of_range_is_refused():
    with pytest.raises(ValueError):
        simplify.simplify(ss.OUT_OF_RANGE, 1.0)
    inside = [i for i in range(4) if i not in ss.OUT_OF_RANGE_FACES]
    got = simplify.simplify(dict(ss.OUT_OF_RANGE, faces=ss.OUT_OF_RANGE["faces"][inside]), 1.0)
    assert got["face_index"].tolist() == [0, 1] and got["cluster"].tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------ 2. against a brute force
def _brute(m, cell, origin, flaps):
    """Clusters and kept faces by dictionaries over python ints; the cell of a vertex by the statement's float32 operations, one
    vertex at a time."""
    c, inv, o = simplify.grid(cell, origin)
    V = len(m["vertices"])
    wq = np.full(V, 65536) if m["weight"] is None else fusion.quantise_weight(m["weight"])
    first, cluster = {}, []
    with np.errstate(all="ignore"):
        for v in range(V):
            i = [np.floor((m["vertices"][v, a] - o[a]) * inv[a]) for a in range(3)]
            if not all(abs(x) < 2 ** 20 for x in i) or wq[v] == 0:
                cluster.append(None)
                continue
            cluster.append(first.setdefault(tuple(int(x) for x in i), v))
    roots = sorted(set(first.values()))
    dense = {r: n for n, r in enumerate(roots)}
    cl = [-1 if l is None else dense[l] for l in cluster]
    seen, order = {}, []
    for f, face in enumerate(m["faces"].tolist()):
        k = [cl[i] for i in face]
        if min(k) < 0 or len(set(k)) < 3:
            continue
        s = k.index(min(k))
        k = (k[s], k[(s + 1) % 3], k[(s + 2) % 3])
        if k not in seen:
            seen[k] = f
            order.append(k)
    keep = sorted(seen[k] for k in order if flaps or (k[0], k[2], k[1]) not in seen)
    return cl, [cluster.count(r) for r in roots], keep


BRUTE = list(ss.HAND) + ["flaps", "flaps kept", "strip permuted, cells of four", "soup joined, cells that join neighbours"] \
    + [(f, k, s) for f in cs.FIELD_NAMES for k, s in ((1, True), (2, False), (3, True))]


@pytest.mark.parametrize("name", BRUTE, ids=str)
def test_clusters_and_faces_equal_a_dictionary(name):
    m, cell, origin, flaps = ss.case(name)
    if len(m["vertices"]) > 20000:                                      # the python loops: the first vertices and the faces among them
        n = 20000
        f = m["faces"][(m["faces"] < n).all(1)]
        m = {k: None if v is None else (v[..., :n] if k == "feat" else v[:n]) for k, v in m.items()}
        m["faces"] = f
        got = simplify.simplify(m, cell, origin, flaps)
    else:
        got = ss.ref(name)
    cl, members, keep = _brute(m, cell, origin, flaps)
    assert got["cluster"].tolist() == cl and got["members"].tolist() == members and got["face_index"].tolist() == keep


def test_the_means_equal_float64():
    """Positions, weights, channels and normals against float64 weighted means over the same members with the same (quantised)
    weights.  A position: q truncates at most 2^-24 of a cell, t carries two float32 roundings of a number below 64 cells (8e-6 of a
    cell of at most 0.06 m: 5e-7 m) and the result one (6e-8 m at 1 m): 2^-22 cell + 5e-7.  A weight <= 16 is one float32 rounding
    of the exact mean: 2^-20.  A channel: fq rounds by 2^-17 and the result once more: 2^-14 for |f| <= 64.  A normal whose members
    agree (the mean's length above half the weight): 2^-17 sqrt(3) / 0.5 = 2.6e-5 and the float32 normalisation: 1e-4."""
    for name in (("scene", ms.BIG, 5, 2, True), ("outlier", ms.BIG, 8, 2, True), "planted"):
        m, cell, origin, _ = ss.case((name, 2, False))
        got = ss.ref((name, 2, False))
        cl = got["cluster"].astype(np.int64)
        used = cl >= 0
        w = fusion.quantise_weight(m["weight"]).astype(np.float64) * 2.0 ** -16
        V2 = len(got["vertices"])
        total = lambda x, sel=used: np.bincount(cl[sel], (w * x)[sel], V2)
        sw = total(np.ones_like(w))
        assert used.sum() > 0 and np.abs(got["weight"] - sw / got["members"]).max() <= 2.0 ** -20
        for a in range(3):
            assert np.abs(got["vertices"][:, a] - total(m["vertices"][:, a].astype(np.float64)) / sw).max() <= 2.0 ** -22 * cell[a] + 5e-7
        for c in range(2):
            assert np.abs(m["feat"][c]).max() <= 64 and np.abs(got["feat"][c] - total(m["feat"][c].astype(np.float64)) / sw).max() <= 2.0 ** -14
        nv = used & m["normal_valid"]
        n = np.stack([total(m["normal"][:, a].astype(np.float64), nv) for a in range(3)], 1)
        l = np.linalg.norm(n, axis=1)
        ok = l > 0.5 * total(np.ones_like(w), nv).clip(1e-30)
        assert ok.sum() > 0.5 * V2 and got["normal_valid"][ok].all() and np.abs(got["normal"][ok] - n[ok] / l[ok, None]).max() <= 1e-4
        assert not got["normal"][~got["normal_valid"]].any()


# ------------------------------------------------------------------------------------------ 3. a closed surface
def _unbalanced(faces):
    """The number of directed edges (a, b) that do not occur as often as (b, a)."""
    f = np.asarray(faces, np.int64)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    count = {}
    for a, b in e.tolist():
        count[(a, b)] = count.get((a, b), 0) + 1
    return sum(1 for (a, b), n in count.items() if count.get((b, a), 0) != n)


def _volume(m):
    v = m["vertices"].astype(np.float64)
    a, b, c = (v[m["faces"][:, k]] for k in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6)


def test_the_ellipsoid_stays_closed_and_keeps_its_volume():
    """The ellipsoid (closed, oriented; 988 vertices, 1972 triangles) at cells of 1, 2 and 3 lattice units from origins 0 and 0.5:
    every directed edge keeps its partner, and at cell 1 the enclosed volume stays within 0.97 of the input's (clustering shrinks a
    convex surface).  Measured: 0 unbalanced edges in all six cases; volume ratios 0.979 / 0.982 at cell 1 (334 / 255 vertices),
    0.876 / 0.874 at cell 2 and 0.751 / 0.708 at cell 3 (origins 0 / 0.5) - the coarser cells are recorded, not bounded."""
    m = cs.get("ellipsoid")
    v0 = abs(_volume(m))
    assert len(m["vertices"]) == 988 and len(m["faces"]) == 1972 and _unbalanced(m["faces"]) == 0 and abs(v0 - 295.4) < 0.1
    for k in (1, 2, 3):
        for origin in (0.0, 0.5):
            out = simplify.simplify(m, float(k), (origin,) * 3)
            ratio = abs(_volume(out)) / v0
            print(f"ellipsoid: cell {k}, origin {origin}: {len(out['vertices'])} vertices, {len(out['faces'])} triangles, volume ratio {ratio:.3f}")
            assert _unbalanced(out["faces"]) == 0 and 0 < len(out["faces"]) < len(m["faces"]), (k, origin)
            assert np.sign(_volume(out)) == np.sign(_volume(m))         # the winding survives
            if k == 1:
                assert ratio >= 0.97, (origin, ratio)


# ------------------------------------------------------------------------------------------ 4. what it is for
def test_the_plane_stays_a_plane():
    """Means of points on a plane stay on it, and the quantisation adds at most cell * 2^-24: max |Z - 0.9137| <= 1e-5, the project's
    plane bound.  Measured: 4.9e-7 m before and after, at cells of 2 and 3 voxels."""
    m = cs.get("plane")
    before = float(np.abs(m["vertices"][:, 2] - ms.PLANE_Z).max())
    for k in (2, 3):
        cell, origin = ss.grid_of("plane", k)
        out = simplify.simplify(m, cell, origin)
        err = float(np.abs(out["vertices"][:, 2] - ms.PLANE_Z).max())
        print(f"plane: cells of {k} voxels: {len(m['vertices'])} -> {len(out['vertices'])} vertices, {len(m['faces'])} -> {len(out['faces'])} triangles, "
              f"max |Z - {ms.PLANE_Z}| {before:.2e} -> {err:.2e} m")
        assert err <= 1e-5 and 0 < len(out["faces"]) < len(m["faces"]) / 3


@pytest.mark.parametrize("views", [1, 5, 8])
def test_the_fusion_scene_gets_coarser_and_no_worse(views):
    """The clean fusion scene in the (33, 40, 65) volume at cells of 2 and 3 voxels from the volume's origin: no wrong-surface
    vertex, and the RMSE at most 1.25 x the input mesh's - a cap, not a measurement.  Measured (vertices / triangles, RMSE in cm):
    1 view   4068 /  5276 0.82 ->  2 voxels 559 /  358 0.93 (x 1.14),  3 voxels 439 / 275 0.66 (x 0.81)
    5 views 12917 / 24716 0.53 ->  2 voxels 806 / 1327 0.56 (x 1.06),  3 voxels 615 / 926 0.41 (x 0.78)
    8 views 12817 / 24758 0.42 ->  2 voxels 776 / 1301 0.38 (x 0.92),  3 voxels 621 / 875 0.35 (x 0.83)"""
    name = ("scene", ms.BIG, views, 2, True)
    m = cs.get(name)
    before = ms.quality(m)
    for k in (2, 3):
        out = ss.ref((name, k, False))
        after = ms.quality(out)
        print(f"{views} views, cells of {k} voxels: {len(m['vertices'])} / {len(m['faces'])} -> {len(out['vertices'])} / {len(out['faces'])}, "
              f"RMSE {100 * before['rmse']:.2f} -> {100 * after['rmse']:.2f} cm (x {after['rmse'] / before['rmse']:.2f}), wrong {after['wrong']}")
        assert after["wrong"] == 0 and before["wrong"] == 0
        assert after["rmse"] <= 1.25 * before["rmse"]
        assert len(out["vertices"]) < len(m["vertices"]) / 2 and 100 < len(out["faces"]) < len(m["faces"])   # a cell holds 8 voxels or 27


def test_simplifying_twice_with_the_same_grid_changes_nothing():
    """Where it must hold: a mean of positions in a cell lies in that cell, so on the same grid every vertex is alone in its cell, no
    face collapses and none repeats.  It must hold where no member lies on a cell's face: a cluster flat on a face has its mean
    there too, and the float32 rounding of that mean may put it on either side.  Marching-tetrahedra vertices lie on the voxel
    lattice's edges, so the grids here start half a VOXEL off the lattice (cells of 1 and 3 voxels shifted by half a cell): a
    member is at least a quarter voxel inside its cell."""
    for name in (("scene", ms.BIG, 8, 2, True), ("outlier", ms.BIG, 5, 2, True), "ellipsoid"):
        for k in (1, 3):
            _, cell, origin, _ = ss.case((name, k, True))
            once = ss.ref((name, k, True))
            twice = simplify.simplify(once, cell, origin)
            n = len(once["vertices"])
            assert np.array_equal(twice["cluster"], np.arange(n)) and (twice["members"] == 1).all(), (name, k)
            assert np.array_equal(twice["faces"], once["faces"]) and np.array_equal(twice["face_index"], np.arange(len(once["faces"]))), (name, k)
            assert np.abs(twice["vertices"] - once["vertices"]).max() <= 2.0 ** -22 * max(cell) + 5e-7


# ------------------------------------------------------------------------------------------ 5. what is refused
def test_refusals():
    m = cs.get("ellipsoid")
    for cell in (0, -1.0, NAN := float("nan"), float("inf"), (1, 1), (1, 0, 1), (1, 1, -2), "a", 1e-46, None):
        with pytest.raises(ValueError):
            simplify.simplify(m, cell)
        with pytest.raises(ValueError):
            simplify.cluster(m, cell)
    for origin in ((0, 0), (0, NAN, 0), (0, 0, float("inf")), 1.0):
        with pytest.raises(ValueError):
            simplify.simplify(m, 1.0, origin)
    for bad in ([1], dict(m, weight=m["weight"][:-1]), dict(m, faces=m["faces"][:, :2]), dict(m, edge=m["edge"][:-1])):
        with pytest.raises(ValueError):
            simplify.simplify(bad, 1.0)
    c, inv, o = simplify.grid(0.03, (1, 2, 3))
    assert c.dtype == inv.dtype == o.dtype == _F and c.tolist() == [float(_F(0.03))] * 3 and o.tolist() == [1, 2, 3]
    assert inv[0] == _F(1.0 / float(_F(0.03)))


# ------------------------------------------------------------------------------------------ 6. the plumbing
def test_the_abi_is_declared_exported_and_refuses_bad_arguments():
    from be_hip import native
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    names = ("be_mesh_cluster_workspace_bytes", "be_mesh_cluster_f32", "be_mesh_simplify_sum_rows", "be_mesh_simplify_workspace_bytes",
             "be_mesh_simplify_count", "be_mesh_simplify_emit")
    for name in names:
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    assert f"#define BE_SIMPLIFY_INDEX_BITS {simplify.INDEX_BITS}\n" in hdr and f"#define BE_SIMPLIFY_FRAC_BITS {simplify.FRAC_BITS}\n" in hdr
    o = native.ops()
    for name in ("mesh_cluster", "mesh_simplify_count", "mesh_simplify"):
        assert hasattr(o, name), name
    scan = lib.be_exclusive_scan_workspace_bytes
    # keys 8 V, a table of 32 slots (the power of two >= 2 V) of 4 bytes, slots 4 V, flags V, ids 4 V, each padded to 8
    assert lib.be_mesh_cluster_workspace_bytes(10) == 80 + 128 + 40 + 16 + 40 + scan(10)
    assert lib.be_mesh_cluster_workspace_bytes(-1) == 0 and lib.be_mesh_cluster_workspace_bytes((1 << 29) + 1) == 0
    assert lib.be_mesh_simplify_workspace_bytes(5) == 64 + 128 + 24 + scan(5) and lib.be_mesh_simplify_workspace_bytes(-1) == 0
    assert lib.be_mesh_simplify_sum_rows(0, 0) == 4 and lib.be_mesh_simplify_sum_rows(3, 1) == 11 and lib.be_mesh_simplify_sum_rows(-1, 0) == 0
    # every refusal below returns before a launch: no GPU is touched
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    f3 = lambda *x: (C.c_float * 3)(*x)
    one, zero = f3(1, 1, 1), f3(0, 0, 0)
    big = 1 << 20
    cl = lambda **kw: lib.be_mesh_cluster_f32(*[dict(dict(vertices=p, weight=None, V=4, cell=one, origin=zero, label=p, cluster=p, members=p, totals=p,
                                                          workspace=p, bytes=big, stream=None), **kw)[k]
                                                for k in ("vertices", "weight", "V", "cell", "origin", "label", "cluster", "members", "totals", "workspace",
                                                          "bytes", "stream")])
    for bad in (dict(V=-1), dict(V=(1 << 29) + 1), dict(cell=f3(1, 0, 1)), dict(cell=f3(1, -1, 1)), dict(cell=f3(float("nan"), 1, 1)),
                dict(cell=f3(float("inf"), 1, 1)), dict(cell=f3(1e-45, 1, 1)), dict(origin=f3(0, float("inf"), 0)), dict(origin=f3(float("nan"), 0, 0)),
                dict(totals=None), dict(label=None), dict(workspace=odd), dict(bytes=8)):
        assert cl(**bad) != 0, bad
    assert b"workspace" in lib.be_last_error()
    count = lambda **kw: lib.be_mesh_simplify_count(*[dict(dict(vertices=p, faces=p, V=4, T=2, weight=None, feat=None, C=0, normal=None, normal_valid=None,
                                                                cell=one, origin=zero, cluster=p, flaps=0, sums=p, fflag=p, foff=p, totals=p, workspace=p,
                                                                bytes=big, stream=None), **kw)[k]
                                                      for k in ("vertices", "faces", "V", "T", "weight", "feat", "C", "normal", "normal_valid", "cell", "origin",
                                                                "cluster", "flaps", "sums", "fflag", "foff", "totals", "workspace", "bytes", "stream")])
    for bad in (dict(T=-1), dict(V=(1 << 29) + 1), dict(C=65), dict(C=1), dict(normal_valid=p), dict(cell=f3(0, 1, 1)), dict(cluster=None), dict(sums=None),
                dict(fflag=None), dict(workspace=odd), dict(bytes=16)):
        assert count(**bad) != 0, bad
    emit = lambda **kw: lib.be_mesh_simplify_emit(*[dict(dict(vertices=p, faces=p, V=4, T=2, cell=one, origin=zero, label=p, cluster=p, members=p, sums=p, C=0,
                                                              normals=0, fflag=p, foff=p, V2=2, T2=1, vertices_out=p, faces_out=p, weight_out=None,
                                                              feat_out=None, normal_out=None, normal_valid_out=None, face_index=p, stream=None), **kw)[k]
                                                    for k in ("vertices", "faces", "V", "T", "cell", "origin", "label", "cluster", "members", "sums", "C",
                                                              "normals", "fflag", "foff", "V2", "T2", "vertices_out", "faces_out", "weight_out", "feat_out",
                                                              "normal_out", "normal_valid_out", "face_index", "stream")])
    for bad in (dict(V2=5), dict(T2=3), dict(C=65), dict(C=1), dict(normals=1), dict(normal_out=p), dict(vertices_out=None), dict(face_index=None),
                dict(label=None), dict(cell=f3(-1, 1, 1))):
        assert emit(**bad) != 0, bad


def test_the_wrappers_refuse_what_is_not_on_the_gpu():
    import torch
    from be_hip import native
    m = {k: None if v is None else torch.from_numpy(v) for k, v in cs.get("planted").items()}
    for call in (lambda: native.mesh_cluster(m, 1.0), lambda: native.mesh_simplify(m, 1.0), lambda: native.mesh_simplify(cs.get("planted"), 1.0),
                 lambda: native.mesh_simplify(m, 0.0), lambda: native.mesh_simplify(m, 1.0, origin=(0, 0)), lambda: native.mesh_cluster([1], 1.0),
                 lambda: native.mesh_simplify(dict(m, faces=m["faces"].long()), 1.0), lambda: native.mesh_cluster(dict(m, weight=m["weight"][:-1]), 1.0)):
        with pytest.raises(ValueError):
            call()


def test_the_workflow_settings(tmp_path):
    from be_hip import workflow as wf
    from be_hip import camera
    base = dict(poses=np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))]), tsdf_dims=(8, 8, 8), tsdf_origin=(0.0, 0.0, 0.5), tsdf_voxel=(0.01, 0.01, 0.01), tsdf_mesh=1)
    path = str(tmp_path / "f.npz")

    def load(**more):
        np.savez(path, **{k: v for k, v in dict(base, **more).items() if v is not None})
        return wf.load_fusion(path)

    assert "mesh_cell" not in load()
    assert load(mesh_cell=0.02)["mesh_cell"] == (float(_F(0.02)),) * 3
    assert load(mesh_cell=(0.02, 0.03, 0.01), tsdf_mesh=None, mesh_render=1)["mesh_cell"] == tuple(float(_F(c)) for c in (0.02, 0.03, 0.01))
    for bad in (dict(mesh_cell=0.0), dict(mesh_cell=-0.01), dict(mesh_cell=(0.02, 0.02)), dict(mesh_cell=float("nan")),
                dict(mesh_cell=0.02, tsdf_mesh=None), dict(mesh_cell=0.02, tsdf_mesh=0)):
        with pytest.raises(ValueError):
            load(**bad)
