"""CPU tests of the statement of mesh smoothing (be_hip/smooth.py), which test_smooth_gpu.py holds the kernels to bit for bit.

They tie the statement to ground: cases worked by hand, a dictionary-based brute force in python integers written here, the same
iteration in float64 without quantisation, a closed surface that must keep its volume, a plane that must stay a plane, and the purpose
of the feature - on the fusion scene the vertices come closer to the true surfaces while none is lost."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from be_hip import smooth
import components_scenes as cs
import mesh_scenes as ms
import smooth_scenes as sm

_F = np.float32
SCENE8 = ("scene", ms.BIG, 8, 2, True)


# ------------------------------------------------------------------------------------------ 1. by hand
@pytest.mark.parametrize("name", list(sm.HAND), ids=str)
def test_the_hand_worked_cases(name):
    m, kw, want = sm.HAND[name]
    got = sm.ref(name)
    V = len(m["vertices"])
    assert got["valence"].tolist() == want["valence"] and got["valence"].dtype == np.int32
    assert got["boundary"].tolist() == [bool(b) for b in want["boundary"]] and got["boundary"].dtype == np.bool_
    adj = sm.adjacency(name)
    assert np.array_equal(adj["valence"], got["valence"]) and np.array_equal(adj["boundary"], got["boundary"]) and set(adj) == set(sm.ADJACENCY_KEYS)
    assert got["vertices"].shape == (V, 3) and got["vertices"].dtype == _F and got["displacement"].shape == (V,) and got["displacement"].dtype == _F
    assert set(got) == set(sm.KEYS) and got["faces"] is m["faces"] and got["edge"] is None and got["weight"] is None and got["normal"] is None
    if "vertices" in want:                                              # exact: binary fractions
        w = np.asarray(want["vertices"], _F).reshape(-1, 3)
        assert np.array_equal(got["vertices"].view(np.uint32), w.view(np.uint32)), got["vertices"].tolist()
        with np.errstate(all="ignore"):
            moved = np.sqrt(((w - m["vertices"]).astype(np.float64) ** 2).sum(1))
        ok = np.isfinite(moved)
        assert np.allclose(got["displacement"][ok], moved[ok], rtol=1e-6, atol=0) and not got["displacement"][~ok].any()
    assert not np.isnan(got["displacement"]).any()


def test_the_tetrahedron_moves_towards_its_centre():
    """Vertex 0 of the tetrahedron: each neighbour twice, the mean (4/3, 4/3, 4/3), one step with lam = 0.5 -> (2/3, 2/3, 2/3) to a
    unit of 2^-30 and a float32 rounding."""
    got = sm.ref("a tetrahedron", iters=1, mu=0.0)
    assert np.abs(got["vertices"][0].astype(np.float64) - 2 / 3).max() <= 2.0 ** -30 + 2.0 ** -25
    assert np.abs(got["displacement"][0] - np.sqrt(3) * 2 / 3) <= 1e-6


def test_an_index_out_of_range_is_refused():
    for call in (smooth.smooth, smooth.adjacency, smooth.vertex_normals):
        with pytest.raises(ValueError):
            call(sm.OUT_OF_RANGE)
    inside = [i for i in range(4) if i not in sm.OUT_OF_RANGE_FACES]
    got = smooth.adjacency(dict(sm.OUT_OF_RANGE, faces=sm.OUT_OF_RANGE["faces"][inside]))
    assert got["valence"].tolist() == [1, 2, 2, 1]


# ------------------------------------------------------------------------------------------ 2. against a brute force
def _brute(m, iters, lam, mu, free):
    """Adjacency by dictionaries and the steps in python integers and python floats (float64, one rounding per operation), one
    vertex at a time -> (valence, boundary, Q [V][3])."""
    v = m["vertices"]
    V = len(v)
    with np.errstate(all="ignore"):
        ok = [bool(all(abs(float(x)) < 65536.0 for x in v[i])) for i in range(V)]
    slots = [[] for _ in range(V)]
    edges = {}
    valence = [0] * V
    for a, b, c in m["faces"].tolist():
        if len({a, b, c}) < 3 or not (ok[a] and ok[b] and ok[c]):
            continue
        slots[a] += [b, c]
        slots[b] += [c, a]
        slots[c] += [a, b]
        for x, y in ((a, b), (b, c), (c, a)):
            edges[(min(x, y), max(x, y))] = edges.get((min(x, y), max(x, y)), 0) + 1
        for x in (a, b, c):
            valence[x] += 1
    boundary = [False] * V
    for (x, y), n in edges.items():
        if n == 1:
            boundary[x] = boundary[y] = True
    Q = [[round(float(x) * 2.0 ** 30) if ok[i] else 0 for x in v[i]] for i in range(V)]
    for f in [lam, mu] * iters:
        if f == 0:
            continue
        new = []
        for i in range(V):
            n = len(slots[i])
            if n == 0 or (boundary[i] and not free):
                new.append(Q[i])
                continue
            row = []
            for a in range(3):
                S = sum(Q[u][a] for u in slots[i])
                d = float(S) / float(n) - float(Q[i][a])
                row.append(Q[i][a] + round(f * d))                      # round: to even on a tie, as rint
            new.append(row)
        Q = new
    return valence, boundary, Q


@pytest.mark.parametrize("name", sm.ALL, ids=str)
def test_adjacency_and_steps_equal_a_dictionary(name):
    """Every scene, two iterations, boundary fixed and free; of a large mesh the first 6000 vertices and the faces among them."""
    m = sm.get(name)
    if len(m["vertices"]) > 6000:
        n = 6000
        m = dict(cs.bare(m["vertices"][:n], m["faces"][(m["faces"] < n).all(1)]))
    kw = sm.HAND[name][1] if name in sm.HAND else {}
    lam, mu = kw.get("lam", 0.5), kw.get("mu", -0.53)
    for free in (False, True):
        got = smooth.smooth(m, iters=2, lam=lam, mu=mu, boundary="free" if free else "fixed")
        valence, boundary, Q = _brute(m, 2, lam, mu, free)
        assert got["valence"].tolist() == valence and got["boundary"].tolist() == boundary
        vu = smooth.usable(m)[0]
        Q0 = smooth.quantise(m["vertices"], vu)
        Q = np.asarray(Q, np.int64).reshape(-1, 3)
        same = (Q == Q0).all(1)
        want = np.where(same[:, None], m["vertices"].view(np.uint32), (Q.astype(np.float64) * 2.0 ** -30).astype(_F).view(np.uint32))
        assert np.array_equal(got["vertices"].view(np.uint32), want), name
        if name == "fan":                                                # cut open: the hub's row is still 2 x 5998 slots long
            assert valence[0] == 6000 - 2


def test_the_synthetic_scenes_are_what_they_are_for():
    f = sm.adjacency("fan")
    assert f["valence"][0] == sm.FAN and f["valence"][1:].tolist() == [2] * sm.FAN and not f["boundary"][0] and f["boundary"][1:].all()
    fixed, free = sm.ref("fan"), sm.ref("fan", boundary="free")
    assert (fixed["displacement"] > 0).tolist() == [True] + [False] * sm.FAN and (free["displacement"] > 0).all()
    s = sm.adjacency("soup")
    assert len(s["valence"]) == 3 * cs.SOUP > 262144 and (s["valence"] == 1).all() and s["boundary"].all()
    assert not sm.ref("soup")["displacement"].any()                     # every vertex is boundary: nothing moves
    # free: every vertex moves but the one in the middle of a collinear, evenly spaced triangle, which components_scenes._grid has
    moved = sm.ref("soup", boundary="free")["displacement"] > 0
    assert 0.9 < moved.mean() < 1
    j = sm.adjacency("soup joined")                                     # the joining faces repeat an index: they are not usable
    assert np.array_equal(j["valence"], s["valence"]) and np.array_equal(j["boundary"], s["boundary"])
    for order in ("ascending", "descending", "permuted"):
        a = sm.adjacency(f"strip {order} 1")
        assert sorted(a["valence"].tolist()) == [1, 1, 2, 2] + [3] * (cs.STRIP - 2) and a["boundary"].all()


# ------------------------------------------------------------------------------------------ 3. against float64
def _float64(m, iters, lam, mu, free):
    """The same iteration on float64 positions, with plain means over the slots: no fixed point, no rounding to 2^-30."""
    V = len(m["vertices"])
    vu, f, fu = smooth.usable(m)
    f = f[fu]
    valence, bnd = smooth._adjacency(V, f)
    nb, start = smooth.rows(V, f)
    n = 2 * valence
    movable = (n > 0) & (free | ~bnd)
    P = m["vertices"].astype(np.float64)
    for fac in [lam, mu] * iters:
        S = np.zeros_like(P)
        S[n > 0] = np.add.reduceat(P[nb], start[n > 0], axis=0)
        P = np.where(movable[:, None], P + fac * (S / np.maximum(n, 1)[:, None] - P), P)
    return P


def test_the_fixed_point_iteration_equals_float64():
    """The 8-view scene in 33 x 40 x 65 voxels, fixed and free, 10 and 20 iterations, against the unquantised iteration: at most 5e-7
    m.  A step rounds a position by 2^-31 m (4.7e-10) and the amplification of lam | mu over 40 steps stays small; the final
    float32 rounding at |x| <= 1.2 m is 6e-8 m.  Measured: 6.3e-8 m in all four cases - the float32 rounding."""
    m = cs.get(SCENE8)
    for free in (False, True):
        for iters in (10, 20):
            got = smooth.smooth(m, iters=iters, boundary="free" if free else "fixed")
            want = _float64(m, iters, 0.5, -0.53, free)
            gap = float(np.abs(got["vertices"].astype(np.float64) - want).max())
            print(f"8 views, {'free' if free else 'fixed'}, {iters} iterations: max |fixed point - float64| = {gap:.2e} m")
            assert gap <= 5e-7


# ------------------------------------------------------------------------------------------ 4. what it is for
@pytest.mark.parametrize("views", [1, 5, 8])
def test_the_fusion_scene_comes_closer_to_the_truth(views):
    """The clean fusion scene in the (33, 40, 65) volume at the defaults (10 iterations, lam 0.5, mu -0.53, boundary held): the RMSE
    against the true surfaces falls, no vertex lands on a wrong surface, no vertex or face is lost.  Measured (cm):
    1 view 0.815 -> 0.790 (x 0.969), 5 views 0.527 -> 0.474 (x 0.899), 8 views 0.420 -> 0.372 (x 0.886)."""
    name = ("scene", ms.BIG, views, 2, True)
    m = cs.get(name)
    out = sm.ref(name)
    before, after = ms.quality(m), ms.quality(out)
    print(f"{views} views: {len(m['vertices'])} / {len(m['faces'])}, RMSE {100 * before['rmse']:.3f} -> {100 * after['rmse']:.3f} cm "
          f"(x {after['rmse'] / before['rmse']:.3f}), wrong {after['wrong']}, moved {int((out['displacement'] > 0).sum())}")
    assert after["rmse"] < before["rmse"] and after["wrong"] == 0 and before["wrong"] == 0
    assert out["vertices"].shape == m["vertices"].shape and out["faces"] is m["faces"] and after["vertices"] > 0
    for k in ("weight", "feat", "normal", "normal_valid"):               # they ride along
        assert out[k] is m[k]


def test_the_outlier_scene_keeps_its_floaters():
    """Smoothing does not remove floaters: the wrong-surface vertices of the outlier scene are recorded, not bounded.  Measured at 8
    views in 33 x 40 x 65 voxels: 38 before, 38 after."""
    name = ("outlier", ms.BIG, 8, 2, True)
    before, after = ms.quality(cs.get(name)), ms.quality(sm.ref(name))
    print(f"outlier scene, 8 views: wrong {before['wrong']} -> {after['wrong']}, RMSE {100 * before['rmse']:.3f} -> {100 * after['rmse']:.3f} cm")
    assert before["wrong"] > 0


# ------------------------------------------------------------------------------------------ 5. a closed surface, a plane
def _unbalanced(faces):
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


def test_the_ellipsoid_keeps_its_volume():
    """The ellipsoid (closed, oriented) has no boundary vertex and every directed edge has its partner; 10 iterations at the defaults
    keep its volume within 1 %, and a plain Laplacian (mu = 0) is further from 1.  Measured: 1.0064 and 0.868."""
    m = cs.get("ellipsoid")
    adj = sm.adjacency("ellipsoid")
    assert not adj["boundary"].any() and adj["valence"].min() >= 3 and _unbalanced(m["faces"]) == 0
    v0 = _volume(m)
    taubin, laplace = _volume(sm.ref("ellipsoid")) / v0, _volume(sm.ref("ellipsoid", mu=0.0)) / v0
    print(f"ellipsoid: volume ratio after 10 iterations: {taubin:.4f} at the defaults, {laplace:.4f} with mu = 0")
    assert abs(taubin - 1) <= 0.01 and abs(laplace - 1) > abs(taubin - 1)


def test_the_plane_stays_a_plane():
    """Means of points on a plane stay on it: max |Z - 0.9137| <= 1e-5 before and after, fixed and free.  Measured: 4.8e-7 m."""
    m = cs.get("plane")
    before = float(np.abs(m["vertices"][:, 2] - ms.PLANE_Z).max())
    assert before <= 1e-5
    for boundary in smooth.BOUNDARY:
        out = smooth.smooth(m, boundary=boundary)
        err = float(np.abs(out["vertices"][:, 2] - ms.PLANE_Z).max())
        print(f"plane, {boundary}: max |Z - {ms.PLANE_Z}| {before:.2e} -> {err:.2e} m, moved {int((out['displacement'] > 0).sum())} of {len(m['vertices'])}")
        assert err <= 1e-5 and (out["displacement"] > 0).any()


# ------------------------------------------------------------------------------------------ 6. vertex normals
def test_vertex_normals_of_the_ellipsoid():
    """Unit length where valid; on the ellipsoid every normal agrees with the float64 area-weighted sum of face normals to 1e-5 (the
    float32 cross products of edges a few units long carry 1e-7 relative, the quantisation 2^-40) and points the same way."""
    m = cs.get("ellipsoid")
    got = sm.normals("ellipsoid")
    assert got["normal"].dtype == _F and got["normal_valid"].dtype == np.bool_ and got["normal_valid"].all()
    assert np.abs(np.linalg.norm(got["normal"].astype(np.float64), axis=1) - 1).max() <= 1e-6
    v = m["vertices"].astype(np.float64)
    a, b, c = (v[m["faces"][:, k]] for k in range(3))
    fn = np.cross(b - a, c - a)
    total = np.zeros_like(v)
    for k in range(3):
        np.add.at(total, m["faces"][:, k], fn)
    want = total / np.linalg.norm(total, axis=1)[:, None]
    assert (np.einsum("ij,ij->i", got["normal"], total) > 0).all() and np.abs(got["normal"] - want).max() <= 1e-5


def test_vertex_normals_by_hand():
    tri = smooth.vertex_normals(sm.get("one triangle, fixed"))           # cross((4, 0, 0), (0, 4, 0)) = (0, 0, 16)
    assert tri["normal"].tolist() == [[0, 0, 1]] * 3 and tri["normal_valid"].all()
    none = smooth.vertex_normals(sm.get("vertices without a face"))
    assert not none["normal"].any() and not none["normal_valid"].any() and not np.signbit(none["normal"]).any()
    nan = smooth.vertex_normals(sm.get("a vertex that is not a number"))
    assert nan["normal_valid"].tolist() == [True, True, True, False] and nan["normal"][3].tolist() == [0, 0, 0]
    flip = smooth.vertex_normals(cs.bare(sm.get("one triangle, fixed")["vertices"], [[0, 2, 1]]))    # the face's own corner order
    assert flip["normal"].tolist() == [[0, 0, -1]] * 3
    both = smooth.vertex_normals(cs.bare(sm.get("one triangle, fixed")["vertices"], [[0, 1, 2], [0, 2, 1]]))
    assert not both["normal_valid"].any() and not both["normal"].any()   # the sums cancel exactly: integers
    out = smooth.smooth(cs.get("planted"), normals="recompute")
    again = smooth.vertex_normals(out)
    assert np.array_equal(out["normal"].view(np.uint32), again["normal"].view(np.uint32)) and np.array_equal(out["normal_valid"], again["normal_valid"])
    assert smooth.smooth(cs.get("planted"), normals="drop")["normal"] is None and smooth.smooth(cs.get("planted"), normals="drop")["normal_valid"] is None


def test_the_normals_the_volume_gives_are_the_better_ones():
    """The median angle to the true normal (0, 0, -1) on the 8-view scene - both true surfaces face the cameras - of the TSDF
    gradient normals the mesh came with, of vertex_normals of the raw mesh and of vertex_normals of the smoothed mesh: recorded,
    not bounded.  Measured: 13.0, 19.2 and 15.9 degrees - which is why normals="keep" is the default."""
    m = cs.get(SCENE8)
    angle = lambda n, ok: float(np.degrees(np.median(np.arccos(np.clip(-n[ok, 2].astype(np.float64), -1, 1)))))
    raw, smoothed = sm.normals(SCENE8), smooth.vertex_normals(sm.ref(SCENE8))
    got = angle(m["normal"], m["normal_valid"]), angle(raw["normal"], raw["normal_valid"]), angle(smoothed["normal"], smoothed["normal_valid"])
    print("8 views: median angle to (0, 0, -1): TSDF normals %.1f, vertex_normals of the raw mesh %.1f, of the smoothed mesh %.1f degrees" % got)
    assert all(np.isfinite(got))


# ------------------------------------------------------------------------------------------ 7. what is refused
def test_refusals():
    m = cs.get("ellipsoid")
    nan = float("nan")
    for kw in (dict(iters=-1), dict(iters=10001), dict(iters=1.5), dict(iters=True), dict(iters="a"), dict(iters=None), dict(lam=0.0), dict(lam=1.5),
               dict(lam=nan), dict(lam=-0.5), dict(lam="a"), dict(lam=float("inf")), dict(mu=0.1), dict(mu=-2.5), dict(mu=nan), dict(mu=None),
               dict(boundary="held"), dict(boundary=None), dict(normals="new"), dict(normals=True)):
        with pytest.raises(ValueError):
            smooth.smooth(m, **kw)
    for bad in ([1], dict(m, weight=m["weight"][:-1]), dict(m, faces=m["faces"][:, :2]), dict(m, edge=m["edge"][:-1])):
        for call in (smooth.smooth, smooth.adjacency, smooth.vertex_normals):
            with pytest.raises(ValueError):
                call(bad)
    assert smooth.check_args("x", np.int64(3), 1, -2, "free", "drop") == (3, 1.0, -2.0, True, "drop")
    assert smooth.check_args("x", 10000, 1e-9, 0, "fixed", "keep") == (10000, 1e-9, 0.0, False, "keep")


# ------------------------------------------------------------------------------------------ 8. the plumbing
def test_the_abi_is_declared_exported_and_refuses_bad_arguments():
    from be_hip import native
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_mesh_smooth_workspace_bytes", "be_mesh_adjacency_f32", "be_mesh_smooth_f32", "be_mesh_normals_f32"):
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    assert f"#define BE_SMOOTH_FRAC_BITS {smooth.FRAC_BITS}\n" in hdr and f"#define BE_SMOOTH_COORD_MAX_LOG2 {smooth.COORD_MAX_LOG2}\n" in hdr
    assert f"#define BE_SMOOTH_NORMAL_BITS {smooth.NORMAL_BITS}\n" in hdr and f"#define BE_SMOOTH_MAX_ITERS {smooth.MAX_ITERS}\n" in hdr
    o = native.ops()
    for name in ("mesh_adjacency", "mesh_smooth", "mesh_normals"):
        assert hasattr(o, name), name
    size = lib.be_mesh_smooth_workspace_bytes
    # two Q buffers of 24 V, a table of 64 slots (the power of two >= 6 T) of 8 + 4 bytes, rows 24 T, offsets and cursors 4 V each, one
    # scan sum per 1024 vertices, flags V and T, each padded to 8
    assert size(10, 9) == 2 * 240 + 64 * 12 + 216 + 2 * 40 + 8 + 16 + 16
    assert size(0, 0) == 2 * 12 and size(1025, 0) == 2 * 24600 + 24 + 2 * 4104 + 8 + 1032
    assert size(-1, 0) == 0 and size(0, -1) == 0 and size((1 << 29) + 1, 0) == 0 and size(0, (1 << 29) + 1) == 0
    # every refusal below returns before a launch: no GPU is touched
    buf = (C.c_int64 * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    big = 1 << 20
    nan, inf = float("nan"), float("inf")
    order = ("vertices", "faces", "V", "T", "iters", "lam", "mu", "free", "vertices_out", "displacement", "valence", "boundary", "workspace", "bytes",
             "stream")
    base = dict(vertices=p, faces=p, V=4, T=2, iters=1, lam=0.5, mu=-0.53, free=0, vertices_out=p, displacement=p, valence=p, boundary=p, workspace=p,
                bytes=big, stream=None)
    run = lambda **kw: lib.be_mesh_smooth_f32(*[dict(base, **kw)[k] for k in order])
    for bad in (dict(V=-1), dict(T=-1), dict(V=(1 << 29) + 1), dict(T=(1 << 29) + 1), dict(iters=-1), dict(iters=10001), dict(lam=0.0), dict(lam=1.25),
                dict(lam=nan), dict(lam=inf), dict(mu=0.25), dict(mu=-2.5), dict(mu=nan), dict(mu=-inf), dict(free=2), dict(free=-1), dict(vertices=None),
                dict(faces=None), dict(vertices_out=None), dict(displacement=None), dict(valence=None), dict(boundary=None), dict(workspace=None),
                dict(workspace=odd), dict(bytes=8)):
        assert run(**bad) != 0, bad
    assert b"workspace" in lib.be_last_error()
    few = ("vertices", "faces", "V", "T", "a", "b", "workspace", "bytes", "stream")
    for fn in (lib.be_mesh_adjacency_f32, lib.be_mesh_normals_f32):
        call = lambda **kw: fn(*[dict(dict(vertices=p, faces=p, V=4, T=2, a=p, b=p, workspace=p, bytes=big, stream=None), **kw)[k] for k in few])
        for bad in (dict(V=-1), dict(T=-1), dict(V=(1 << 29) + 1), dict(vertices=None), dict(faces=None), dict(a=None), dict(b=None),
                    dict(workspace=None), dict(workspace=odd), dict(bytes=8)):
            assert call(**bad) != 0, bad
        assert b"workspace" in lib.be_last_error()
    assert run(V=0, T=0) == 0                                           # nothing to do, nothing launched


def test_the_wrappers_refuse_what_is_not_on_the_gpu():
    import torch
    from be_hip import native
    m = {k: None if v is None else torch.from_numpy(v) for k, v in cs.get("planted").items()}
    for call in (lambda: native.mesh_adjacency(m), lambda: native.mesh_smooth(m), lambda: native.mesh_normals(m), lambda: native.mesh_smooth(cs.get("planted")),
                 lambda: native.mesh_smooth(m, iters=-1), lambda: native.mesh_smooth(m, lam=0), lambda: native.mesh_smooth(m, mu=1),
                 lambda: native.mesh_smooth(m, boundary="x"), lambda: native.mesh_smooth(m, normals="x"), lambda: native.mesh_adjacency([1]),
                 lambda: native.mesh_smooth(dict(m, faces=m["faces"].long())), lambda: native.mesh_normals(dict(m, weight=m["weight"][:-1]))):
        with pytest.raises(ValueError):
            call()


def test_the_workflow_settings(tmp_path):
    from be_hip import workflow as wf
    from be_hip import camera
    base = dict(poses=np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))]), tsdf_dims=(8, 8, 8), tsdf_origin=(0.0, 0.0, 0.5),
                tsdf_voxel=(0.01, 0.01, 0.01), tsdf_mesh=1)
    path = str(tmp_path / "f.npz")

    def load(**more):
        np.savez(path, **{k: v for k, v in dict(base, **more).items() if v is not None})
        return wf.load_fusion(path)

    assert "mesh_smooth" not in load()
    assert load(mesh_smooth=10)["mesh_smooth"] == 10 and load(mesh_smooth=0)["mesh_smooth"] == 0
    assert load(mesh_smooth=3, tsdf_mesh=None, mesh_render=1)["mesh_smooth"] == 3 and load(mesh_smooth=0, tsdf_mesh=None)["mesh_smooth"] == 0
    for bad in (dict(mesh_smooth=-1), dict(mesh_smooth=2.5), dict(mesh_smooth=10001), dict(mesh_smooth=float("nan")), dict(mesh_smooth=5, tsdf_mesh=None),
                dict(mesh_smooth=5, tsdf_mesh=0)):
        with pytest.raises(ValueError):
            load(**bad)
