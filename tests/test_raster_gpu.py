"""GPU tests of the mesh rasteriser (be_mesh_raster_f32; native.raster_mesh; DepthPipeline.render_mesh).

One bit contract: every output of native.raster_mesh equals raster.render (be_hip/raster.py), ints as ints and floats as uint32,
through both bindings; test_raster_cpu.py ties that statement to triangles worked by hand, a closed surface, a plane, its own
float64 evaluation and the ray cast.  Beside it: neither a repeated run nor a side stream changes a bit.

The kernel's boundaries and the cases that cross them: k_raster_faces gives a wave to each triangle, four to a workgroup, and walks
the clipped bounding box in 8 x 8 blocks - so 1 x 1, 1 x 67 and 41 x 1 targets (a block cut to one row or column), 9 x 9 (one block
plus one row and one column), 41 x 67, and 147 x 147 under the pipeline's own camera, where a triangle is larger than the frame and
a wave walks hundreds of blocks; meshes of 1, 2 and 4 triangles (a part of a workgroup), of 1972 and of 24758.  The scenes are
those of tests/raster_scenes.py; the pipeline fixtures and scene are those of test_render_at_gpu.py."""
import numpy as np
import pytest
import torch

from be_hip import camera, raster
import fuse_scenes as fs
import mesh_scenes as ms
import raster_scenes as rc
from test_render_at_gpu import DEV, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
_F = np.float32
DTYPES = dict(depth=torch.float32, face=torch.int32, valid=torch.bool, weight=torch.float32, feat=torch.float32, normal=torch.float32,
              normal_valid=torch.bool, bary=torch.float32)


def _on_gpu(mesh):
    return {k: None if v is None else G(v) for k, v in mesh.items() if k in ("vertices", "faces", "weight", "feat", "normal", "normal_valid")}


def _run(n, c, **kw):
    return n.raster_mesh(_on_gpu(c["mesh"]), c["cam"], c["pose"], c["size"], **dict(c["kw"], **kw))


def _host(out):
    assert set(out) == set(rc.KEYS)
    for k, t in out.items():
        if t is not None:
            assert t.is_cuda and t.dtype == DTYPES[k] and t.is_contiguous(), k
    return {k: None if t is None else N(t) for k, t in out.items()}


def _check(n, name):
    ref = rc.reference(name)
    assert rc.same(_host(_run(n, rc.get(name))), ref), name
    return ref


# ------------------------------------------------------------------------------------------ 1. every scene of the CPU file
def test_the_hand_worked_cases(env, binding):
    n = env["native"]
    for name in rc.HAND:
        _check(n, name)
    assert rc.reference("empty")["feat"].shape == (2, 9, 9) and rc.reference("bare")["feat"] is None


def test_the_ellipsoid(env, binding):
    n = env["native"]
    for name in ("ellipsoid none", "ellipsoid back", "ellipsoid want", "ellipsoid depth only", "ellipsoid nan"):
        ref = _check(n, name)
        assert ref["valid"].sum() > 40
    assert not np.isfinite(rc.reference("ellipsoid nan")["feat"]).all()  # the planted attributes reach pixels


@pytest.mark.parametrize("holes", [False, True])
def test_the_planted_volume(env, binding, holes):
    ref = _check(env["native"], f"planted {holes}")
    assert ref["valid"].sum() > 100 and ref["feat"].shape == (2, 41, 67)


@pytest.mark.parametrize("dims", [(5, 7, 9), ms.BIG])
def test_the_fusion_scene(env, binding, dims):
    n = env["native"]
    for V in (1, 3, 8):
        ref = _check(n, f"scene {dims} {V}")
        assert ref["valid"].any()
    c = rc.get(f"scene {dims} 8")
    for cull in ("back", "front"):
        want = raster.render(c["mesh"], c["cam"], c["pose"], c["size"], cull=cull, want=("feat", "bary"))
        assert rc.same(_host(_run(n, c, cull=cull, want=("feat", "bary"))), want)


def test_the_plane_and_the_rotated_views(env, binding):
    n = env["native"]
    assert _check(n, "plane")["valid"].sum() > 1500
    assert _check(n, "lattice")["valid"].sum() > 500


@pytest.mark.parametrize("size", rc.TARGETS + ("pipeline",))
def test_targets(env, binding, size):
    ref = _check(env["native"], f"target {size}")
    assert ref["valid"].any()
    if size == "pipeline":
        assert ref["valid"].all() and len(np.unique(ref["face"])) < 40   # a few triangles, each larger than the 147 x 147 frame


# ------------------------------------------------------------------------------------------ 2. the same bits on every run
def test_repeats_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    name = f"scene {ms.BIG} 8"
    c, ref = rc.get(name), rc.reference(name)
    m = _on_gpu(c["mesh"])
    for _ in range(2):
        assert rc.same(_host(n.raster_mesh(m, c["cam"], c["pose"], c["size"])), ref)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = n.raster_mesh(m, c["cam"], c["pose"], c["size"])
    side.synchronize()
    assert rc.same(_host(out), ref)


def test_rejected_inputs(env, binding):
    n = env["native"]
    c = rc.get("one pixel")
    m = _on_gpu(c["mesh"])
    ok = dict(mesh=m, cam_dst=c["cam"], pose=None, size=(3, 3))
    n.raster_mesh(**ok)
    for bad in (dict(mesh={k: None if v is None else v.cpu() for k, v in m.items()}), dict(mesh=dict(m, faces=m["faces"].long())),
                dict(mesh=dict(m, weight=m["weight"].cpu())), dict(mesh=dict(m, feat=m["feat"][:, :2])), dict(mesh=dict(m, normal=m["normal"].double())),
                dict(mesh=c["mesh"]), dict(size=(0, 3)), dict(size=(3, 16385)), dict(near=float("nan")), dict(cull="both"), dict(want=("depth",)),
                dict(cam_dst=(1, float("nan"), 0, 0)), dict(pose=np.zeros(12))):
        with pytest.raises(ValueError):
            n.raster_mesh(**dict(ok, **bad))
    # a face index outside [0, V): the statement refuses it, the kernels drop the triangle
    faces = torch.tensor([[0, 1, 2], [0, 1, 3], [0, -1, 2]], dtype=torch.int32, device=DEV)
    got, want = _host(n.raster_mesh(dict(m, faces=faces), c["cam"], None, (3, 3))), _host(n.raster_mesh(m, c["cam"], None, (3, 3)))
    assert rc.same(got, want) and want["valid"].any()


# ------------------------------------------------------------------------------------------ 3. DepthPipeline.render_mesh
def test_pipeline_render_mesh(env, pipe, binding):
    from be_hip.pipeline import DepthPipeline
    n = env["native"]
    sc = _scene(env, "g6", None)
    H, W = sc["H"], sc["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"])
    maps = _maps_of(env, sc, p.depth_thres)
    z = maps["depth_map"]
    has = (z > 0) & torch.isfinite(z)
    lo, hi = float(z[has].min()), float(z[has].max())
    cam = env["dcal"].intrinsics(H, W)
    assert cam == rc.PIPE
    half = 0.55 * W / cam.fx * hi                                        # the volume of test_mesh_gpu.py's pipeline test
    desc = dict(dims=(48, 32, 32), origin=(-half, -half, lo - 0.06), voxel=(2 * half / 31, 2 * half / 31, (hi - lo + 0.12) / 47), trunc=0.05)
    vol = p.integrate([(maps, None)], want=("shpd",), **desc)
    tri = p.extract_mesh(vol)
    out = p.render_mesh(tri, size=(H, W))
    assert set(out) == {"depth", "valid", "face", "weight", "shpd", "normal", "normal_valid"}
    assert out["shpd"].shape == (3, H, W) and out["normal"].shape == (3, H, W) and out["face"].dtype == torch.int32
    host = {k: N(v) for k, v in tri.items()}
    ref = raster.render(dict(vertices=host["vertices"], faces=host["faces"], weight=host["weight"], feat=host["shpd"], normal=host["normal"],
                             normal_valid=host["normal_valid"]), cam, None, (H, W), want=("feat", "weight", "normal"))
    print(f"pipeline scene: {int(ref['valid'].sum())} of {H * W} pixels see the mesh of {len(host['faces'])} triangles")
    assert ref["valid"].sum() > 100                                      # one view of the synthetic scene: a sparse volume, a small mesh
    for k, r in (("depth", ref["depth"]), ("weight", ref["weight"]), ("shpd", ref["feat"]), ("normal", ref["normal"])):
        assert np.array_equal(N(out[k]).view(np.uint32), r.view(np.uint32)), k
    assert np.array_equal(N(out["face"]), ref["face"]) and np.array_equal(N(out["valid"]), ref["valid"]) and np.array_equal(N(out["normal_valid"]), ref["normal_valid"])
    # the rendered mesh lies where the ray cast of the same volume does: within a voxel along Z where both see a surface
    cast = p.raycast(vol)
    both = out["valid"] & cast["valid"]
    print(f"pipeline scene: {int(both.sum())} pixels seen by both the mesh and the ray cast")
    assert int(both.sum()) > 20 and float((out["depth"] - cast["depth"])[both].abs().median()) < desc["voxel"][2]
    plain = p.render_mesh(tri, cam_dst=fs.CAM, pose=camera.pose(None, (0.001, 0, 0)), size=(9, 9), want=(), cull="back", normals=False)
    assert set(plain) == {"depth", "valid", "face", "weight", "normal", "normal_valid"} and plain["normal"] is None and plain["depth"].shape == (9, 9)
    for kw in (dict(size=None), dict(want=("colour",)), dict(want=("faces",)), dict(cull="both")):
        with pytest.raises(ValueError):
            p.render_mesh(tri, **dict(dict(size=(H, W)), **kw))
    with pytest.raises(ValueError):
        p.render_mesh([1], size=(H, W))


# ------------------------------------------------------------------------------------------ 4. the workflow settings
def test_workflow_eval_fuse_writes_the_rendered_mesh(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` whose settings hold the tsdf_* keys and mesh_render = 1 (and no
    tsdf_mesh): beside fused_0000.npz and tsdf_0000.npz the group's mesh seen by view 0's camera, mesh_render_0000.npz, which lies
    where the ray cast of the same volume into the same camera does."""
    import os
    from conftest import ROOT
    from be_hip import datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "fuse.npz", poses=poses, tau=0.03, tsdf_dims=(64, 32, 32), tsdf_origin=(-0.02, -0.02, 0.6), tsdf_voxel=(0.0013, 0.0013, 0.01),
             tsdf_trunc=0.04, mesh_render=1)
    out = tmp_path / "fused"
    wf.main(["eval", "--fuse", str(tmp_path / "fuse.npz"), "--out_path", str(out), "--model_path", os.path.join(ROOT, "checkpoints"),
             "--data_path", str(data_dir), "--cuda", DEV])
    assert sorted(os.listdir(out)) == ["fused_0000.npz", "mesh_render_0000.npz", "tsdf_0000.npz"]
    got, cast = dict(np.load(out / "mesh_render_0000.npz")), dict(np.load(out / "tsdf_0000.npz"))
    assert set(got) == {"depth", "valid", "face", "normal", "shpd"}
    assert got["depth"].shape == (147, 147) and got["shpd"].shape == (3, 147, 147) and got["normal"].shape == (3, 147, 147) and got["face"].dtype == np.int32
    both = got["valid"] & cast["valid"]
    print(f"workflow: the mesh is seen on {int(got['valid'].sum())} pixels, the ray cast hits {int(cast['valid'].sum())}, both {int(both.sum())}")
    assert np.array_equal(got["valid"], got["face"] >= 0) and both.sum() > 0.5 * cast["valid"].sum() > 0
    assert np.median(np.abs(got["depth"] - cast["depth"])[both]) < 0.01   # a voxel along Z
