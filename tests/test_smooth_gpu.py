"""GPU tests of mesh smoothing (be_mesh_adjacency_f32, be_mesh_smooth_f32, be_mesh_normals_f32; native.mesh_adjacency / mesh_smooth /
mesh_normals; DepthPipeline.smooth_mesh; the mesh_smooth key of `workflow eval --fuse`).

One bit contract: every output equals the statement be_hip/smooth.py, ints as ints and floats as their bits, through both bindings;
test_smooth_cpu.py ties that statement to hand-worked cases, a brute force in python integers, the float64 iteration, a closed
surface and the fusion scene.  Beside it: a repeated run and a side stream change no bit, and a mesh whose faces are permuted gives
the same positions - the order inside a row does not matter.

Where the kernels can go wrong, and the cases that go there: one address under every thread of the edge table and the cursor, and a
row far longer than a workgroup - a fan of 70000 triangles around one hub, whose row of 140000 slots the wave sums; the table's
and the cursors' races - a strip of 70000 triangles numbered ascending, descending and at random; the scan's second level - 270000
vertices; V = 0, T = 0, faces and vertices that are not usable, a face that names what is not there."""
import os

import numpy as np
import pytest
import torch

from be_hip import components, smooth
import components_scenes as cs
import mesh_scenes as ms
import smooth_scenes as sm
from test_render_at_gpu import DEV, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
DTYPES = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32, normal_valid=torch.bool,
              valence=torch.int32, boundary=torch.bool, displacement=torch.float32)
_GPU = {}


def _on_gpu(m):
    """A mesh of the scenes on the GPU, uploaded once; nothing writes to it."""
    if id(m) not in _GPU:
        _GPU[id(m)] = (m, {k: None if v is None else G(v) for k, v in m.items() if k in cs.KEYS})
    return _GPU[id(m)][1]


def _host(out, keys):
    """The named outputs as numpy, after the checks every output passes: on the GPU, of its dtype, contiguous."""
    for k in keys:
        assert out[k] is None or (out[k].device == torch.device(DEV) and out[k].dtype == DTYPES[k] and out[k].is_contiguous()), k
    return {k: None if out[k] is None else N(out[k]) for k in keys}


def _same_smoothed(out, ref):
    assert set(out) == set(sm.KEYS) and out["edge"] is None
    return cs.same(_host(out, sm.KEYS), ref, sm.KEYS)


def _run(n, name, **kw):
    g = _on_gpu(sm.get(name))
    ref = sm.ref(name, **kw)
    call = dict(sm.HAND[name][1], **kw) if name in sm.HAND else kw
    assert _same_smoothed(n.mesh_smooth(g, **call), ref), (name, kw)
    return ref


def _adjacency_and_normals(n, name):
    g = _on_gpu(sm.get(name))
    adj, nor = n.mesh_adjacency(g), n.mesh_normals(g)
    assert set(adj) == set(sm.ADJACENCY_KEYS) and set(nor) == set(sm.NORMAL_KEYS)
    assert cs.same(_host(adj, sm.ADJACENCY_KEYS), sm.adjacency(name), sm.ADJACENCY_KEYS), name
    assert cs.same(_host(nor, sm.NORMAL_KEYS), sm.normals(name), sm.NORMAL_KEYS), name


# ------------------------------------------------------------------------------------------ 1. the bit contract
@pytest.mark.parametrize("name", list(sm.HAND), ids=str)
def test_hand_cases_equal_the_statement(env, binding, name):
    _run(env["native"], name)
    _run(env["native"], name, normals="recompute")
    _adjacency_and_normals(env["native"], name)


@pytest.mark.parametrize("name", sm.SYNTHETIC, ids=str)
def test_synthetic_cases_equal_the_statement(env, binding, name):
    """(1 and 10 iterations) x (boundary fixed, free) x (mu -0.53, 0)."""
    n = env["native"]
    for kw in sm.CONFIGS:
        ref = _run(n, name, **kw)
        if name == "fan":                                               # the row of 140000 slots is the hub's, and the hub moves
            assert ref["valence"][0] == sm.FAN and ref["displacement"][0] > 0
    if name == "soup":                                                  # past the scan's second level
        assert len(ref["valence"]) == 3 * cs.SOUP > 262144
    _adjacency_and_normals(n, name)


@pytest.mark.parametrize("field", cs.FIELD_NAMES, ids=str)
def test_field_meshes_equal_the_statement(env, binding, field):
    """At the defaults, and with the boundary free and the normals recomputed."""
    n = env["native"]
    m = sm.get(field)
    for kw in sm.FIELD_CONFIGS:
        ref = _run(n, field, **kw)
        assert (ref["displacement"] > 0).any() and (ref["feat"] is None) == (m["feat"] is None)
    assert ref["normal"] is not None and ref["normal_valid"].any()
    _adjacency_and_normals(n, field)


def test_a_face_out_of_range_is_ignored(env, binding):
    n = env["native"]
    m = sm.OUT_OF_RANGE
    inside = np.array([i not in sm.OUT_OF_RANGE_FACES for i in range(len(m["faces"]))])
    g = {k: None if v is None else G(v) for k, v in m.items()}
    kw = dict(iters=3, boundary="free", normals="recompute")
    want = smooth.smooth(dict(m, faces=m["faces"][inside]), **kw)
    got = n.mesh_smooth(g, **kw)
    assert torch.equal(got["faces"], g["faces"])                        # the faces ride along, the one that is ignored too
    assert _same_smoothed(dict(got, faces=got["faces"][torch.from_numpy(inside).to(DEV)].contiguous()), want) and want["valence"].tolist() == [1, 2, 2, 1]
    assert cs.same(_host(n.mesh_adjacency(g), sm.ADJACENCY_KEYS), want, sm.ADJACENCY_KEYS)


def test_repeats_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    for name, kw in ((("outlier", ms.BIG, 8, 2, True), dict(boundary="free", normals="recompute")), ("strip permuted 1", dict(boundary="free", iters=10, mu=-0.53)),
                     ("fan", dict(boundary="fixed", iters=10, mu=-0.53))):
        g, ref = _on_gpu(sm.get(name)), sm.ref(name, **kw)
        for _ in range(2):
            assert _same_smoothed(n.mesh_smooth(g, **kw), ref)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            out, adj, nor = n.mesh_smooth(g, **kw), n.mesh_adjacency(g), n.mesh_normals(g)
        side.synchronize()
        assert _same_smoothed(out, ref) and cs.same(_host(adj, sm.ADJACENCY_KEYS), sm.adjacency(name), sm.ADJACENCY_KEYS)
        assert cs.same(_host(nor, sm.NORMAL_KEYS), sm.normals(name), sm.NORMAL_KEYS)


def test_the_order_of_the_faces_does_not_matter(env, binding):
    """The faces permuted: other rows in another order, other slots of the table - the same sums, so the same bits."""
    n = env["native"]
    for name in (("scene", ms.BIG, 8, 2, True), "fan"):
        m = sm.get(name)
        perm = np.random.default_rng(5).permutation(len(m["faces"]))
        g = dict(_on_gpu(m), faces=G(np.ascontiguousarray(m["faces"][perm])))
        kw = dict(boundary="free", normals="recompute") if name != "fan" else dict(boundary="fixed", normals="recompute")
        got, ref = n.mesh_smooth(g, **kw), sm.ref(name, **kw)
        keys = ("vertices", "boundary", "valence", "displacement", "normal", "normal_valid")
        assert cs.same(_host(got, keys), ref, keys)


def test_smoothing_twice(env, binding):
    """smooth_mesh(smooth_mesh(m, 5), 5) runs: the result is a mesh and goes straight back in.  It is NOT expected to equal 10
    iterations: between the two calls the positions pass through float32, 2^-24 relative, where one call keeps 2^-30 m."""
    n = env["native"]
    name = ("scene", ms.BIG, 8, 2, True)
    once = n.mesh_smooth(_on_gpu(sm.get(name)), iters=5)
    twice = n.mesh_smooth(once, iters=5)
    assert _same_smoothed(twice, smooth.smooth(sm.ref(name, iters=5), iters=5))
    ten = sm.ref(name)["vertices"]
    assert np.abs(N(twice["vertices"]) - ten).max() < 1e-6 and torch.equal(twice["valence"], once["valence"]) and torch.equal(twice["boundary"], once["boundary"])


# ------------------------------------------------------------------------------------------ 2. what is refused
def test_rejected_inputs(env, binding):
    n = env["native"]
    m = _on_gpu(cs.get("planted"))
    cpu = {k: None if v is None else v.cpu() for k, v in m.items()}
    nan = float("nan")
    for call in (lambda: n.mesh_smooth(cpu), lambda: n.mesh_adjacency(cpu), lambda: n.mesh_normals(cpu), lambda: n.mesh_smooth(cs.get("planted")),
                 lambda: n.mesh_smooth(m, iters=-1), lambda: n.mesh_smooth(m, iters=10001), lambda: n.mesh_smooth(m, iters=2.5), lambda: n.mesh_smooth(m, lam=0.0),
                 lambda: n.mesh_smooth(m, lam=nan), lambda: n.mesh_smooth(m, lam=1.01), lambda: n.mesh_smooth(m, mu=0.01), lambda: n.mesh_smooth(m, mu=-2.01),
                 lambda: n.mesh_smooth(m, mu=nan), lambda: n.mesh_smooth(m, boundary="open"), lambda: n.mesh_smooth(m, normals=None),
                 lambda: n.mesh_smooth(dict(m, faces=m["faces"].long())), lambda: n.mesh_smooth(dict(m, vertices=m["vertices"].double())),
                 lambda: n.mesh_normals(dict(m, faces=m["faces"][:, :2])), lambda: n.mesh_adjacency(dict(m, weight=m["weight"].cpu()))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------ 3. DepthPipeline.smooth_mesh
def test_pipeline_smooth_mesh(env, pipe, binding):
    """extract_mesh -> clean_mesh -> smooth_mesh -> simplify_mesh -> render_mesh -> save_mesh, end to end; the smoothing against the
    statement on the cleaned mesh."""
    from be_hip.pipeline import DepthPipeline
    sc = _scene(env, "g6", None)
    H, W = sc["H"], sc["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"])
    maps = _maps_of(env, sc, p.depth_thres)
    z = maps["depth_map"]
    has = (z > 0) & torch.isfinite(z)
    lo, hi = float(z[has].min()), float(z[has].max())
    cam = env["dcal"].intrinsics(H, W)
    half = 0.55 * W / cam.fx * hi                                        # the volume of test_components_gpu.py's pipeline test
    desc = dict(dims=(48, 32, 32), origin=(-half, -half, lo - 0.06), voxel=(2 * half / 31, 2 * half / 31, (hi - lo + 0.12) / 47), trunc=0.05)
    tri = p.extract_mesh(p.integrate([(maps, None)], want=("shpd",), **desc))
    cleaned = p.clean_mesh(tri, min_triangles=2)                         # the lone triangles go; the mesh of this scene is many small patches
    out = p.smooth_mesh(cleaned)
    assert set(out) == set(cleaned) | {"valence", "boundary", "displacement"} and out["shpd"] is cleaned["shpd"] and out["faces"] is cleaned["faces"]
    assert out["normal"] is cleaned["normal"] and out["vertices"].shape == cleaned["vertices"].shape
    as_mesh = dict(vertices=N(cleaned["vertices"]), faces=N(cleaned["faces"]))
    ref = smooth.smooth(as_mesh)
    for k in ("vertices", "valence", "boundary", "displacement"):
        assert cs.same(dict(a=N(out[k])), dict(a=ref[k]), ("a",)), k
    print(f"pipeline scene: {as_mesh['vertices'].shape[0]} / {as_mesh['faces'].shape[0]}, moved {int((ref['displacement'] > 0).sum())}, "
          f"boundary {int(ref['boundary'].sum())}, largest displacement {float(ref['displacement'].max()):.2e} m")
    assert (ref["displacement"] > 0).any()
    free = p.smooth_mesh(cleaned, iters=3, lam=0.4, mu=0.0, boundary="free", normals="recompute")
    want = smooth.smooth(as_mesh, iters=3, lam=0.4, mu=0.0, boundary="free", normals="recompute")
    for k in ("vertices", "normal", "normal_valid", "displacement"):
        assert cs.same(dict(a=N(free[k])), dict(a=want[k]), ("a",)), k
    dropped = p.smooth_mesh(cleaned, iters=0, normals="drop")
    assert dropped["normal"] is None and dropped["normal_valid"] is None and torch.equal(dropped["vertices"].view(torch.int32), cleaned["vertices"].view(torch.int32))
    # the smoothed mesh goes straight into simplify_mesh, render_mesh, save_mesh, clean_mesh and smooth_mesh again
    cell = tuple(2 * v for v in desc["voxel"])
    coarse = p.simplify_mesh(out, cell, origin=desc["origin"])
    assert set(coarse) == (set(cleaned) - {"component", "components"}) | {"cluster", "members", "face_index"}
    print(f"simplified: {coarse['vertices'].shape[0]} / {coarse['faces'].shape[0]}")
    assert 0 < coarse["vertices"].shape[0] < out["vertices"].shape[0] and coarse["faces"].shape[0] < out["faces"].shape[0]
    assert coarse["shpd"].shape == (3, coarse["vertices"].shape[0])
    assert p.render_mesh(coarse, size=(H, W))["shpd"].shape == (3, H, W)
    assert int(p.render_mesh(out, size=(H, W))["valid"].sum()) > 50
    p.save_mesh(os.devnull, out)
    p.save_mesh(os.devnull, coarse)
    again = p.clean_mesh(out, largest=True)
    assert 0 < again["faces"].shape[0] <= out["faces"].shape[0] and "displacement" not in again
    more = p.smooth_mesh(out, iters=5)
    assert set(more) == set(out) and more["vertices"].shape == out["vertices"].shape
    for bad in (lambda: p.smooth_mesh([1]), lambda: p.smooth_mesh(tri, iters=-1), lambda: p.smooth_mesh(tri, lam=2.0), lambda: p.smooth_mesh(tri, mu=1.0),
                lambda: p.smooth_mesh(tri, boundary="x"), lambda: p.smooth_mesh(tri, normals="x")):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ 4. the workflow settings
def test_workflow_eval_fuse_smooths_the_mesh(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` twice: with mesh_smooth the mesh written and rendered is the
    statement's smooth of the mesh written without it - after the statement's clean, and before its simplify, where those are set."""
    from conftest import ROOT
    from be_hip import camera, datagen_test as dt, simplify, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    tsdf = dict(tsdf_dims=(64, 32, 32), tsdf_origin=(-0.02, -0.02, 0.6), tsdf_voxel=(0.0013, 0.0013, 0.01))
    base = dict(poses=poses, tau=0.03, tsdf_trunc=0.04, tsdf_mesh=1, mesh_render=1, **tsdf)

    def run(tag, **more):
        np.savez(tmp_path / f"{tag}.npz", **base, **more)
        wf.main(["eval", "--fuse", str(tmp_path / f"{tag}.npz"), "--out_path", str(tmp_path / tag), "--model_path", os.path.join(ROOT, "checkpoints"),
                 "--data_path", str(data_dir), "--cuda", DEV])
        assert sorted(os.listdir(tmp_path / tag)) == ["fused_0000.npz", "mesh_0000.npz", "mesh_0000.ply", "mesh_render_0000.npz", "tsdf_0000.npz"]
        return dict(np.load(tmp_path / tag / "mesh_0000.npz")), dict(np.load(tmp_path / tag / "mesh_render_0000.npz"))

    raw, raw_seen = run("raw")
    as_mesh = dict(vertices=raw["vertices"], faces=raw["faces"], weight=raw["weight"], feat=raw["shpd"], normal=raw["normal"], normal_valid=raw["normal_valid"])
    least = int(components.stats(as_mesh, components.label(len(raw["vertices"]), raw["faces"]))["triangles"].max())
    got, seen = run("smoothed", mesh_min_triangles=least, mesh_smooth=4)
    assert set(got) == (set(raw) | {"valence", "boundary", "displacement", "component", "components_triangles"}) and set(seen) == set(raw_seen)
    ref = smooth.smooth(components.clean(as_mesh, min_triangles=least), iters=4)
    for k, r in (("vertices", ref["vertices"]), ("faces", ref["faces"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"]),
                 ("normal_valid", ref["normal_valid"]), ("valence", ref["valence"]), ("boundary", ref["boundary"]), ("displacement", ref["displacement"])):
        assert cs.same(dict(a=got[k]), dict(a=r), ("a",)), k
    print(f"workflow: {len(got['vertices'])} / {len(got['faces'])}, moved {int((got['displacement'] > 0).sum())}")
    assert (got["displacement"] > 0).any() and seen["valid"].sum() > 0
    cell = (0.0026, 0.0039, 0.02)
    both, _ = run("both", mesh_min_triangles=least, mesh_smooth=4, mesh_cell=cell)
    want = simplify.simplify(ref, cell, tsdf["tsdf_origin"])
    assert "displacement" not in both and cs.same(dict(a=both["vertices"], b=both["faces"]), dict(a=want["vertices"], b=want["faces"]), ("a", "b"))
    for bad in (dict(mesh_smooth=-1), dict(mesh_smooth=1.5)):
        np.savez(tmp_path / "bad.npz", **base, **bad)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / "bad.npz"))
