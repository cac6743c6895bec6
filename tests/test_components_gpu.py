"""GPU tests of mesh cleaning (be_mesh_components_*, be_mesh_select_*; native.mesh_components / mesh_select / mesh_clean;
DepthPipeline.clean_mesh).

One bit contract: every output equals the statement be_hip/components.py, ints as ints and floats as their bits, through both
bindings; test_components_cpu.py ties that statement to hand-worked labels, a breadth-first search, float64 areas and the floaters of
the fusion scene.  Beside it: the order of the faces, a repeated run and a side stream change no bit.

Where the kernels can go wrong, and the cases that go there: the union-find's races - a strip of 70000 triangles numbered
ascending, descending and at random (deep trees; unions that lose a root to another wave or workgroup and go on), two interleaved
strips; the scan's second level at 262144 root flags - 90000 disjoint triangles on 270000 vertices; waves whose lanes hold one
component, a few, or 64 different ones in the sums; V = 0, T = 0, a face that names what is not there; a tie for the largest."""
import os

import numpy as np
import pytest
import torch

from be_hip import components, raster
import components_scenes as cs
import mesh_scenes as ms
from test_render_at_gpu import DEV, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
DTYPES = dict(label=torch.int32, component=torch.int32, face_component=torch.int32, triangles=torch.int32, vertices=torch.int32,
              area_q=torch.int64, area=torch.float64, keep=torch.bool)
MESH_DTYPES = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32,
                   normal_valid=torch.bool, edge=torch.int64, vertex_index=torch.int32, face_index=torch.int32, component=torch.int32)
_GPU = {}


def _on_gpu(name):
    """A named mesh on the GPU, uploaded once; nothing writes to it."""
    if name not in _GPU:
        _GPU[name] = {k: None if v is None else G(v) for k, v in cs.get(name).items() if k in cs.KEYS}
    return _GPU[name]


def _labels(out):
    assert set(out) == set(cs.LABEL_KEYS) | {"K"} and isinstance(out["K"], int)
    for k in cs.LABEL_KEYS:
        assert out[k].is_cuda and out[k].dtype == DTYPES[k] and out[k].is_contiguous(), k
    return dict({k: N(out[k]) for k in cs.LABEL_KEYS}, K=out["K"])


def _mesh(out, keys=cs.SELECT_KEYS):
    for k in keys:
        assert out[k] is None or (out[k].is_cuda and out[k].dtype == MESH_DTYPES[k] and out[k].is_contiguous()), k
    return {k: None if out[k] is None else N(out[k]) for k in keys}


def _same_labels(got, ref):
    return got["K"] == ref["K"] and cs.same(got, ref, cs.LABEL_KEYS)


_CLEAN = {}


def _clean_ref(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _CLEAN:
        _CLEAN[key] = components.clean(cs.get(name), **kw)
    return _CLEAN[key]


def _same_clean(out, ref):
    got = _mesh(out, cs.SELECT_KEYS + ("component",))
    assert cs.same(got, ref, cs.SELECT_KEYS + ("component",))
    comp = {k: N(out["components"][k]) for k in ("triangles", "vertices", "area_q", "area", "keep")}
    for k, t in out["components"].items():
        assert t.is_cuda and t.dtype == DTYPES[k], k
    return cs.same(comp, ref["components"], ("triangles", "vertices", "area_q", "area", "keep"))


# ------------------------------------------------------------------------------------------ 1. components
@pytest.mark.parametrize("name", cs.ALL, ids=str)
def test_components_equal_the_statement(env, binding, name):
    assert _same_labels(_labels(env["native"].mesh_components(_on_gpu(name))), cs.labels(name)), name


def test_a_face_out_of_range_is_ignored(env, binding):
    n = env["native"]
    m = cs.OUT_OF_RANGE
    inside = np.array([i not in cs.OUT_OF_RANGE_FACES for i in range(len(m["faces"]))])
    ref = components.label(6, m["faces"][inside])
    ref.update(components.stats(dict(m, faces=m["faces"][inside]), ref))
    fc = np.full(len(m["faces"]), -1, np.int32)
    fc[inside] = ref["face_component"]
    g = {k: None if v is None else G(v) for k, v in m.items()}
    assert _same_labels(_labels(n.mesh_components(g)), dict(ref, face_component=fc)) and ref["K"] == 3
    got = _mesh(n.mesh_clean(g, min_triangles=1), cs.SELECT_KEYS + ("component",))
    want = components.clean(dict(m, faces=m["faces"][inside]), min_triangles=1)
    want["face_index"] = np.flatnonzero(inside)[want["face_index"]].astype(np.int32)
    assert cs.same(got, want, cs.SELECT_KEYS + ("component",)) and got["face_index"].tolist() == [0, 3] and got["vertex_index"].tolist() == [0, 1, 2, 4, 5]


def test_the_order_of_the_faces_changes_nothing(env, binding):
    n = env["native"]
    for name in ("strip permuted 1", ("outlier", ms.BIG, 5, 2, True), "soup joined"):
        m, ref = _on_gpu(name), cs.labels(name)
        order = np.random.default_rng(8).permutation(len(cs.get(name)["faces"]))
        got = _labels(n.mesh_components(dict(m, faces=m["faces"][G(order)].contiguous())))
        assert _same_labels(got, dict(ref, face_component=ref["face_component"][order])), name


def test_repeats_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    name = ("outlier", ms.BIG, 8, 2, True)
    m, ref, cref = _on_gpu(name), cs.labels(name), _clean_ref(name, min_triangles=50)
    for _ in range(2):
        assert _same_labels(_labels(n.mesh_components(m)), ref) and _same_clean(n.mesh_clean(m, min_triangles=50), cref)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out, cleaned = n.mesh_components(m), n.mesh_clean(m, min_triangles=50)
    side.synchronize()
    assert _same_labels(_labels(out), ref) and _same_clean(cleaned, cref)


# ------------------------------------------------------------------------------------------ 2. decide and clean
ASKED = (dict(min_triangles=1), dict(min_triangles=50), dict(min_triangles=10 ** 6), dict(min_area=0), dict(min_area=1e-3), dict(largest=True),
         dict(min_triangles=50, min_area=1e-3), dict(min_triangles=1, largest=True), dict(min_area=1e-3, largest=True),
         dict(min_triangles=50, min_area=1e-3, largest=True))
CLEANED = [("outlier", ms.BIG, 1, 2, True), ("outlier", ms.BIG, 5, 2, True), ("outlier", ms.BIG, 5, 0, True), ("outlier", ms.BIG, 8, 2, False),
           ("outlier", cs.SMALL, 5, 2, True), "planted", "twins", "soup joined", "strip permuted 2", "no vertex", "three vertices, no face",
           "a repeated index"]


@pytest.mark.parametrize("name", CLEANED, ids=str)
def test_clean_equals_the_statement(env, binding, name):
    n = env["native"]
    m, lab = _on_gpu(name), cs.labels(name)
    stats = n.mesh_components(m)
    for kw in ASKED:
        ref = _clean_ref(name, **kw)
        assert _same_clean(n.mesh_clean(m, **kw), ref), (name, kw)
        keep = n.mesh_decide(stats, stats["K"], **kw)
        assert keep.dtype == torch.bool and np.array_equal(N(keep), components.decide(lab, **kw)), (name, kw)
    big = _clean_ref(name, min_triangles=10 ** 6)
    assert big["vertices"].shape == (0, 3) and big["faces"].shape == (0, 3)


def test_a_tie_for_the_largest_goes_to_the_lower_id(env, binding):
    out = env["native"].mesh_clean(_on_gpu("twins"), largest=True)
    assert N(out["components"]["keep"]).tolist() == [True, False, False] and N(out["components"]["triangles"]).tolist() == [40, 40, 39]
    assert out["faces"].shape == (40, 3) and not N(out["component"]).any() and N(out["vertex_index"]).tolist() == list(range(42))


def test_cleaning_twice_changes_nothing(env, binding):
    n = env["native"]
    once = n.mesh_clean(_on_gpu(("outlier", ms.BIG, 5, 2, True)), min_triangles=50)
    twice = n.mesh_clean(once, min_triangles=50)
    assert cs.same(_mesh(twice, cs.KEYS), _mesh(once, cs.KEYS), cs.KEYS) and bool(twice["components"]["keep"].all())


# ------------------------------------------------------------------------------------------ 3. select
@pytest.mark.parametrize("name", ["planted", ("outlier", ms.BIG, 5, 2, True), ("outlier", ms.BIG, 8, 2, False), "soup", "one triangle", "no vertex",
                                  "three vertices, no face"], ids=str)
def test_select_equals_the_statement(env, binding, name):
    n = env["native"]
    host, m = cs.get(name), _on_gpu(name)
    V = len(host["vertices"])
    rng = np.random.default_rng(12)
    for keep in (rng.random(V) < 0.5, rng.random(V) < 0.97, np.ones(V, bool), np.zeros(V, bool)):
        got = _mesh(n.mesh_select(m, G(keep)))
        assert cs.same(got, components.select(host, keep), cs.SELECT_KEYS), name
    if name == "planted":                                               # every per-vertex array rode along
        assert all(got[k] is not None for k in cs.KEYS) and got["feat"].shape == (2, 0) and got["edge"].dtype == np.int64


# ------------------------------------------------------------------------------------------ 4. what is refused
def test_rejected_inputs(env, binding):
    n = env["native"]
    m = _on_gpu("planted")
    V = m["vertices"].shape[0]
    keep = torch.ones(V, dtype=torch.bool, device=DEV)
    cpu = {k: None if v is None else v.cpu() for k, v in m.items()}
    for call in (lambda: n.mesh_components(cpu), lambda: n.mesh_clean(cpu, min_triangles=1), lambda: n.mesh_select(cpu, keep.cpu()),
                 lambda: n.mesh_components(dict(m, faces=m["faces"].long())), lambda: n.mesh_components(dict(m, vertices=m["vertices"].double())),
                 lambda: n.mesh_select(dict(m, edge=m["edge"].int()), keep), lambda: n.mesh_select(dict(m, weight=m["weight"].cpu()), keep),
                 lambda: n.mesh_select(m, keep[:-1]), lambda: n.mesh_select(m, keep.to(torch.uint8)), lambda: n.mesh_select(m, keep.cpu()),
                 lambda: n.mesh_select(dict(m, feat=m["feat"][:, :-1]), keep), lambda: n.mesh_clean(m), lambda: n.mesh_clean(m, min_triangles=-1),
                 lambda: n.mesh_clean(m, min_area=float("nan")), lambda: n.mesh_clean(m, min_triangles=1 << 31),
                 lambda: n.mesh_components(cs.get("planted"))):
        with pytest.raises(ValueError):
            call()


# ------------------------------------------------------------------------------------------ 5. DepthPipeline.clean_mesh
def test_pipeline_clean_mesh(env, pipe, binding):
    from be_hip.pipeline import DepthPipeline
    sc = _scene(env, "g6", None)
    H, W = sc["H"], sc["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"])
    maps = _maps_of(env, sc, p.depth_thres)
    z = maps["depth_map"]
    has = (z > 0) & torch.isfinite(z)
    lo, hi = float(z[has].min()), float(z[has].max())
    cam = env["dcal"].intrinsics(H, W)
    half = 0.55 * W / cam.fx * hi                                        # the volume of test_raster_gpu.py's pipeline test
    desc = dict(dims=(48, 32, 32), origin=(-half, -half, lo - 0.06), voxel=(2 * half / 31, 2 * half / 31, (hi - lo + 0.12) / 47), trunc=0.05)
    tri = p.extract_mesh(p.integrate([(maps, None)], want=("shpd",), **desc))
    host = {k: N(v) for k, v in tri.items()}
    as_mesh = dict(vertices=host["vertices"], faces=host["faces"], weight=host["weight"], feat=host["shpd"], normal=host["normal"],
                   normal_valid=host["normal_valid"])
    sizes = np.sort(components.stats(as_mesh, components.label(len(host["vertices"]), host["faces"]))["triangles"])[::-1]
    least = int(sizes[0])                                                # only the largest component (and its equals) stays
    print(f"pipeline scene: {len(host['faces'])} triangles in {len(sizes)} components {sizes[:6].tolist()}; min_triangles = {least}")
    assert len(sizes) > 1                                                # one sparse view: there is something to drop
    out = p.clean_mesh(tri, min_triangles=least)
    assert set(out) == set(tri) | {"component", "components"} and out["shpd"].shape == (3, out["vertices"].shape[0])
    ref = components.clean(as_mesh, min_triangles=least)
    for k, r in (("vertices", ref["vertices"]), ("faces", ref["faces"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"]),
                 ("normal_valid", ref["normal_valid"]), ("component", ref["component"])):
        assert cs.same(dict(a=N(out[k])), dict(a=r), ("a",)), k
    assert np.array_equal(N(out["components"]["keep"]), ref["components"]["keep"]) and 0 < len(ref["faces"]) < len(host["faces"])
    # the cleaned mesh goes straight into render_mesh - and renders as the statement's clean, then the statement's render - and
    # into clean_mesh again
    seen = p.render_mesh(out, size=(H, W))
    want = raster.render(ref, cam, None, (H, W), want=("feat", "weight", "normal"))
    for k, r in (("depth", want["depth"]), ("weight", want["weight"]), ("shpd", want["feat"]), ("normal", want["normal"])):
        assert np.array_equal(N(seen[k]).view(np.uint32), r.view(np.uint32)), k
    assert np.array_equal(N(seen["face"]), want["face"]) and want["valid"].sum() > 50
    again = p.clean_mesh(out, largest=True)
    assert set(again) == set(out) and int(again["components"]["keep"].sum()) == 1 and again["faces"].shape[0] == int(sizes[0])
    p.save_mesh(os.devnull, out)
    for bad in (lambda: p.clean_mesh(tri), lambda: p.clean_mesh([1], min_triangles=1), lambda: p.clean_mesh(tri, min_area=-1.0),
                lambda: p.clean_mesh(dict(tri, shpd=tri["shpd"].double()), min_triangles=1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------ 6. the workflow settings
def test_workflow_eval_fuse_cleans_the_mesh(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` twice: without mesh_min_triangles the files and their keys
    are what they were before the key existed; with it the mesh written and rendered is the statement's clean of that mesh."""
    from conftest import ROOT
    from be_hip import camera, datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    base = dict(poses=poses, tau=0.03, tsdf_dims=(64, 32, 32), tsdf_origin=(-0.02, -0.02, 0.6), tsdf_voxel=(0.0013, 0.0013, 0.01), tsdf_trunc=0.04,
                tsdf_mesh=1, mesh_render=1)

    def run(tag, **more):
        np.savez(tmp_path / f"{tag}.npz", **base, **more)
        wf.main(["eval", "--fuse", str(tmp_path / f"{tag}.npz"), "--out_path", str(tmp_path / tag), "--model_path", os.path.join(ROOT, "checkpoints"),
                 "--data_path", str(data_dir), "--cuda", DEV])
        assert sorted(os.listdir(tmp_path / tag)) == ["fused_0000.npz", "mesh_0000.npz", "mesh_0000.ply", "mesh_render_0000.npz", "tsdf_0000.npz"]
        return dict(np.load(tmp_path / tag / "mesh_0000.npz")), dict(np.load(tmp_path / tag / "mesh_render_0000.npz"))

    raw, raw_seen = run("raw")
    assert set(raw) == {"vertices", "faces", "weight", "shpd", "normal", "normal_valid"} and set(raw_seen) == {"depth", "valid", "face", "normal", "shpd"}
    off, off_seen = run("off", mesh_min_triangles=0)                    # 0 asks for nothing: the same bytes in every array and in the PLY
    assert set(off) == set(raw) and all(off[k].tobytes() == raw[k].tobytes() for k in raw)
    assert all(off_seen[k].tobytes() == raw_seen[k].tobytes() for k in raw_seen)
    with open(tmp_path / "raw" / "mesh_0000.ply", "rb") as a, open(tmp_path / "off" / "mesh_0000.ply", "rb") as b:
        assert a.read() == b.read()
    as_mesh = dict(vertices=raw["vertices"], faces=raw["faces"], weight=raw["weight"], feat=raw["shpd"], normal=raw["normal"], normal_valid=raw["normal_valid"])
    sizes = components.stats(as_mesh, components.label(len(raw["vertices"]), raw["faces"]))["triangles"]
    least = int(np.sort(sizes)[::-1][0])                                 # only the largest component (and its equals) stays
    print(f"workflow: {len(raw['faces'])} triangles in {len(sizes)} components {np.sort(sizes)[::-1][:6].tolist()}")
    got, seen = run("cleaned", mesh_min_triangles=least)
    assert set(got) == set(raw) | {"component", "components_triangles"} and set(seen) == set(raw_seen)
    ref = components.clean(as_mesh, min_triangles=least)
    assert np.array_equal(got["components_triangles"], sizes) and np.array_equal(got["component"], ref["component"])
    for k, r in (("vertices", ref["vertices"]), ("faces", ref["faces"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"]),
                 ("normal_valid", ref["normal_valid"])):
        assert cs.same(dict(a=got[k]), dict(a=r), ("a",)), k
    if len(sizes) > 1:
        assert len(got["faces"]) < len(raw["faces"]) and seen["valid"].sum() <= raw_seen["valid"].sum()
    with open(tmp_path / "raw" / "mesh_0000.ply", "rb") as a, open(tmp_path / "cleaned" / "mesh_0000.ply", "rb") as b:
        assert (a.read() == b.read()) == (len(sizes) == 1)
    for bad in (dict(mesh_min_triangles=-1), dict(mesh_min_triangles=2.5)):
        np.savez(tmp_path / "bad.npz", **base, **bad)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / "bad.npz"))
    np.savez(tmp_path / "bad.npz", **{k: v for k, v in base.items() if k not in ("tsdf_mesh", "mesh_render")}, mesh_min_triangles=5)
    with pytest.raises(ValueError):
        wf.load_fusion(str(tmp_path / "bad.npz"))
