"""GPU tests of mesh simplification (be_mesh_cluster_f32, be_mesh_simplify_*; native.mesh_cluster / mesh_simplify;
DepthPipeline.simplify_mesh; the mesh_cell key of `workflow eval --fuse`).

One bit contract: every output equals the statement be_hip/simplify.py, ints as ints and floats as their bits, through both bindings;
test_simplify_cpu.py ties that statement to hand-worked cases, a dictionary-based brute force, float64 means, a closed surface and the
fusion scene.  Beside it: a repeated run and a side stream change no bit.

Where the kernels can go wrong, and the cases that go there: one address under every thread - a strip of 70000 triangles inside ONE
cell (one slot's atomicMin, one row of sums); the cluster table's races - the same strip in cells four triangles wide, numbered
ascending, descending and at random; the scan's second level and a table with a slot per vertex - 270000 vertices in 270000 cells;
the face table's races - 5000 faces that name three clusters in both windings at random rotations; cell boundaries, negative cells,
the last cell index, positions and weights that are not usable; V = 0, T = 0, a face that names what is not there."""
import os

import numpy as np
import pytest
import torch

from be_hip import components, raster, simplify
import components_scenes as cs
import mesh_scenes as ms
import simplify_scenes as ss
from test_render_at_gpu import DEV, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
DTYPES = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32, normal_valid=torch.bool,
              cluster=torch.int32, members=torch.int32, face_index=torch.int32, label=torch.int32)
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


def _same_simplified(out, ref):
    assert set(out) == set(ss.KEYS) and out["edge"] is None
    got = _host(out, ss.KEYS)
    assert got["vertices"].shape == (len(ref["members"]), 3) and got["faces"].shape == (len(ref["face_index"]), 3)
    return cs.same(got, ref, ss.KEYS)


def _same_clusters(out, ref):
    assert set(out) == set(ss.CLUSTER_KEYS) | {"V"} and isinstance(out["V"], int) and out["V"] == len(ref["members"])
    return cs.same(_host(out, ss.CLUSTER_KEYS), ref, ss.CLUSTER_KEYS)


def _run(n, name):
    m, cell, origin, flaps = ss.case(name)
    g, ref = _on_gpu(m), ss.ref(name)
    assert _same_simplified(n.mesh_simplify(g, cell, origin=origin, flaps=flaps), ref), name
    assert _same_clusters(n.mesh_cluster(g, cell, origin=origin), ref), name
    return ref


# ------------------------------------------------------------------------------------------ 1. the bit contract
@pytest.mark.parametrize("name", list(ss.HAND) + list(ss.SYNTHETIC) + ["flaps", "flaps kept"], ids=str)
def test_simplify_equals_the_statement(env, binding, name):
    ref = _run(env["native"], name)
    if name == "strip in one cell":                                     # one address under every thread
        assert len(ref["vertices"]) == 1 and len(ref["faces"]) == 0 and ref["members"].tolist() == [cs.STRIP + 2]
    if name == "soup, a cell per vertex":                               # past the scan's second level, a slot per vertex
        assert len(ref["vertices"]) == 3 * cs.SOUP > 262144 and len(ref["faces"]) == cs.SOUP
    if name == "flaps":
        assert len(ref["faces"]) == 0
    if name == "flaps kept":
        assert len(ref["faces"]) == 2


@pytest.mark.parametrize("field", cs.FIELD_NAMES, ids=str)
def test_field_meshes_equal_the_statement(env, binding, field):
    """Cells of 1, 2 and 3 voxels, from the volume's origin and half a cell further."""
    for k in ss.CELLS:
        for shift in ss.SHIFTS:
            ref = _run(env["native"], (field, k, shift))
            assert 0 < len(ref["vertices"]) < len(cs.get(field)["vertices"])
    m = cs.get(field)
    assert (ref["feat"] is None) == (m["feat"] is None) and (ref["normal"] is None) == (m["normal"] is None) == (ref["normal_valid"] is None)


def test_a_face_out_of_range_is_ignored(env, binding):
    n = env["native"]
    m = ss.OUT_OF_RANGE
    inside = np.array([i not in ss.OUT_OF_RANGE_FACES for i in range(len(m["faces"]))])
    want = simplify.simplify(dict(m, faces=m["faces"][inside]), 1.0)
    want["face_index"] = np.flatnonzero(inside)[want["face_index"]].astype(np.int32)
    got = n.mesh_simplify({k: None if v is None else G(v) for k, v in m.items()}, 1.0)
    assert _same_simplified(got, want) and N(got["face_index"]).tolist() == [0, 3]


def test_flaps_of_a_real_mesh(env, binding):
    """flaps=True on a mesh where flaps occur: the other branch of the face flags."""
    n = env["native"]
    name = ("outlier", ms.BIG, 8, 2, True)
    cell, origin = ss.grid_of(name, 3)
    ref = simplify.simplify(cs.get(name), cell, origin, flaps=True)
    assert len(ref["faces"]) > len(ss.ref((name, 3, False))["faces"])
    assert _same_simplified(n.mesh_simplify(_on_gpu(cs.get(name)), cell, origin=origin, flaps=True), ref)


def test_repeats_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    for name in ((("outlier", ms.BIG, 8, 2, True), 2, False), "strip permuted, cells of four"):
        m, cell, origin, flaps = ss.case(name)
        g, ref = _on_gpu(m), ss.ref(name)
        for _ in range(2):
            assert _same_simplified(n.mesh_simplify(g, cell, origin=origin), ref) and _same_clusters(n.mesh_cluster(g, cell, origin=origin), ref)
        side = torch.cuda.Stream(DEV)
        side.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(side):
            out, lab = n.mesh_simplify(g, cell, origin=origin), n.mesh_cluster(g, cell, origin=origin)
        side.synchronize()
        assert _same_simplified(out, ref) and _same_clusters(lab, ref)


def test_simplifying_twice_changes_nothing(env, binding):
    n = env["native"]
    name = (("scene", ms.BIG, 8, 2, True), 3, True)
    m, cell, origin, _ = ss.case(name)
    once = n.mesh_simplify(_on_gpu(m), cell, origin=origin)
    twice = n.mesh_simplify(once, cell, origin=origin)                  # the result is a mesh: it goes straight back in
    V2 = once["vertices"].shape[0]
    assert N(twice["cluster"]).tolist() == list(range(V2)) and torch.equal(twice["faces"], once["faces"]) and bool((twice["members"] == 1).all())


# ------------------------------------------------------------------------------------------ 2. what is refused
def test_rejected_inputs(env, binding):
    n = env["native"]
    m = _on_gpu(cs.get("planted"))
    cpu = {k: None if v is None else v.cpu() for k, v in m.items()}
    nan = float("nan")
    for call in (lambda: n.mesh_simplify(cpu, 1.0), lambda: n.mesh_cluster(cpu, 1.0), lambda: n.mesh_simplify(cs.get("planted"), 1.0),
                 lambda: n.mesh_simplify(m, 0.0), lambda: n.mesh_simplify(m, -1.0), lambda: n.mesh_simplify(m, nan), lambda: n.mesh_simplify(m, (1, 1)),
                 lambda: n.mesh_simplify(m, float("inf")), lambda: n.mesh_simplify(m, 1e-45), lambda: n.mesh_cluster(m, (1, 0, 1)),
                 lambda: n.mesh_simplify(m, 1.0, origin=(0, nan, 0)), lambda: n.mesh_cluster(m, 1.0, origin=(0, 0)),
                 lambda: n.mesh_simplify(dict(m, faces=m["faces"].long()), 1.0), lambda: n.mesh_simplify(dict(m, vertices=m["vertices"].double()), 1.0),
                 lambda: n.mesh_simplify(dict(m, weight=m["weight"].cpu()), 1.0), lambda: n.mesh_simplify(dict(m, feat=m["feat"][:, :-1]), 1.0)):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------ 3. DepthPipeline.simplify_mesh
def test_pipeline_simplify_mesh(env, pipe, binding):
    """extract_mesh -> clean_mesh -> simplify_mesh -> render_mesh -> save_mesh, end to end, against the statements in the same order."""
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
    host = {k: N(v) for k, v in tri.items()}
    as_mesh = dict(vertices=host["vertices"], faces=host["faces"], weight=host["weight"], feat=host["shpd"], normal=host["normal"],
                   normal_valid=host["normal_valid"])
    least = int(components.stats(as_mesh, components.label(len(host["vertices"]), host["faces"]))["triangles"].max())
    cell = tuple(2 * v for v in desc["voxel"])
    cleaned = p.clean_mesh(tri, min_triangles=least)
    out = p.simplify_mesh(cleaned, cell, origin=desc["origin"])
    assert set(out) == set(tri) | {"cluster", "members", "face_index"} and out["shpd"].shape == (3, out["vertices"].shape[0])
    ref = simplify.simplify(components.clean(as_mesh, min_triangles=least), cell, desc["origin"])
    for k, r in (("vertices", ref["vertices"]), ("faces", ref["faces"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"]),
                 ("normal_valid", ref["normal_valid"]), ("cluster", ref["cluster"]), ("members", ref["members"]), ("face_index", ref["face_index"])):
        assert cs.same(dict(a=N(out[k])), dict(a=r), ("a",)), k
    print(f"pipeline scene: {len(host['vertices'])} / {len(host['faces'])} -> cleaned {cleaned['vertices'].shape[0]} / {cleaned['faces'].shape[0]} -> "
          f"simplified {len(ref['vertices'])} / {len(ref['faces'])}")
    assert 0 < len(ref["faces"]) < cleaned["faces"].shape[0] / 2
    # the simplified mesh goes straight into render_mesh - and renders as the statement's simplify, then the statement's render -,
    # into save_mesh, and into clean_mesh and simplify_mesh again
    seen = p.render_mesh(out, size=(H, W))
    want = raster.render(ref, cam, None, (H, W), want=("feat", "weight", "normal"))
    for k, r in (("depth", want["depth"]), ("weight", want["weight"]), ("shpd", want["feat"]), ("normal", want["normal"])):
        assert np.array_equal(N(seen[k]).view(np.uint32), r.view(np.uint32)), k
    assert np.array_equal(N(seen["face"]), want["face"]) and want["valid"].sum() > 50
    p.save_mesh(os.devnull, out)
    again = p.clean_mesh(out, largest=True)
    assert set(again) == set(tri) | {"component", "components"} and 0 < again["faces"].shape[0] <= out["faces"].shape[0]
    coarser = p.simplify_mesh(out, tuple(2 * c for c in cell), origin=desc["origin"])
    assert set(coarser) == set(out) and coarser["vertices"].shape[0] < out["vertices"].shape[0] and coarser["cluster"].shape == out["members"].shape
    flaps = p.simplify_mesh(tri, cell, origin=desc["origin"], flaps=True)
    assert flaps["faces"].shape[0] >= p.simplify_mesh(tri, cell, origin=desc["origin"])["faces"].shape[0]
    for bad in (lambda: p.simplify_mesh(tri, 0.0), lambda: p.simplify_mesh([1], 1.0), lambda: p.simplify_mesh(tri, 1.0, origin=(0, 0)),
                lambda: p.simplify_mesh(dict(tri, shpd=tri["shpd"].double()), 1.0)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ 4. the workflow settings
def test_workflow_eval_fuse_simplifies_the_mesh(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` twice: with mesh_cell the mesh written and rendered is the
    statement's simplify of the mesh written without it - after the statement's clean where mesh_min_triangles is set too."""
    from conftest import ROOT
    from be_hip import camera, datagen_test as dt, workflow as wf
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
    sizes = components.stats(as_mesh, components.label(len(raw["vertices"]), raw["faces"]))["triangles"]
    least = int(sizes.max())                                             # only the largest component (and its equals) stays
    cell = (0.0026, 0.0039, 0.02)                                        # 2, 3 and 2 voxels
    got, seen = run("simplified", mesh_min_triangles=least, mesh_cell=cell)
    assert set(got) == (set(raw) | {"cluster", "members", "face_index", "components_triangles"}) and set(seen) == set(raw_seen)
    ref = simplify.simplify(components.clean(as_mesh, min_triangles=least), cell, tsdf["tsdf_origin"])
    for k, r in (("vertices", ref["vertices"]), ("faces", ref["faces"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"]),
                 ("normal_valid", ref["normal_valid"]), ("cluster", ref["cluster"]), ("members", ref["members"]), ("face_index", ref["face_index"])):
        assert cs.same(dict(a=got[k]), dict(a=r), ("a",)), k
    print(f"workflow: {len(raw['vertices'])} / {len(raw['faces'])} -> {len(got['vertices'])} / {len(got['faces'])}")
    assert 0 < len(got["faces"]) < len(raw["faces"]) / 2 and seen["valid"].sum() > 0
    with open(tmp_path / "raw" / "mesh_0000.ply", "rb") as a, open(tmp_path / "simplified" / "mesh_0000.ply", "rb") as b:
        assert len(b.read()) < len(a.read()) / 2
    for bad in (dict(mesh_cell=0.0), dict(mesh_cell=(0.01, 0.01))):
        np.savez(tmp_path / "bad.npz", **base, **bad)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / "bad.npz"))
    np.savez(tmp_path / "bad.npz", **{k: v for k, v in base.items() if k not in ("tsdf_mesh", "mesh_render")}, mesh_cell=0.01)
    with pytest.raises(ValueError):
        wf.load_fusion(str(tmp_path / "bad.npz"))
