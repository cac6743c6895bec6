"""GPU tests of mesh extraction (be_tsdf_mesh_count_f32, be_tsdf_mesh_emit_f32, be_exclusive_scan_u8_i32; native.mesh_field /
tsdf_mesh / exclusive_scan; DepthPipeline.extract_mesh / save_mesh).

One bit contract: every output of native.mesh_field / tsdf_mesh equals mesh.extract (be_hip/mesh.py), ints as ints and floats as
uint32; test_mesh_cpu.py ties that statement to a cell worked by hand, a closed surface, a plane and its own float64 evaluation.
Beside it: the scan alone against numpy.cumsum, and neither a repeated run nor a side stream changes a bit.

The scan's boundaries (a wave covers 64 x 4 = 256 voxels, a workgroup 1024, one pass of the second level 256 workgroup sums =
262144 voxels) and the volumes that cross them: (5, 7, 9) = 315 voxels crosses a wave inside one workgroup; the planted
(2, 2, 512) = 2048 fills exactly two workgroups; the ellipsoid's 2744 and (33, 40, 65) = 85800 (83 full workgroups and a tail of
808) end in a partial workgroup; no fusion volume reaches the second level's second pass, so mesh_scenes.slanted(),
(5, 230, 230) = 264500 voxels, is the smallest case that does.  The scenes are those of tests/mesh_scenes.py; the pipeline
fixtures and scene are those of test_render_at_gpu.py."""
import numpy as np
import pytest
import torch

from be_hip import camera, mesh, volume
import fuse_scenes as fs
import mesh_scenes as ms
from test_render_at_gpu import DEV, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
_F = np.float32
KEYS = ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge")
DTYPES = dict(vertices=torch.float32, faces=torch.int32, weight=torch.float32, feat=torch.float32, normal=torch.float32,
              normal_valid=torch.bool, edge=torch.int64)


def _run(n, f, min_weight=0.0, normals=True):
    return n.mesh_field(G(f["D"]), G(f["W"]), None if f["Fm"] is None else G(f["Fm"]), f["origin"], f["voxel"], min_weight=min_weight,
                        normals=normals)


def _host(out):
    assert set(out) == set(KEYS)
    for k, t in out.items():
        if t is not None:
            assert t.is_cuda and t.dtype == DTYPES[k] and t.is_contiguous(), k
    return {k: None if t is None else N(t) for k, t in out.items()}


def _check(n, name, f, min_weight=0.0, normals=True):
    ref = ms.reference(name, f, min_weight, normals)
    assert ms.same(_host(_run(n, f, min_weight, normals)), ref), (name, min_weight, normals)
    return ref


# ------------------------------------------------------------------------------------------ 1. the scan alone
SPAN, PASS = 1024, 256 * 1024                                            # BE_SCAN_SPAN, BE_SCAN_SUMS_PER_PASS * BE_SCAN_SPAN
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1, PASS - 1, PASS, PASS + 1)


def test_exclusive_scan_against_cumsum(env, binding):
    n = env["native"]
    draw = np.random.default_rng(12).integers(0, 256, PASS + 1, dtype=np.uint8)
    for length in LENGTHS:
        for name, a in (("zeros", np.zeros(length, np.uint8)), ("sevens", np.full(length, 7, np.uint8)), ("draw", draw[:length])):
            offsets, total = n.exclusive_scan(G(a))
            assert offsets.dtype == torch.int32 and offsets.shape == (length,) and total.dtype == torch.int64 and total.numel() == 1
            incl = np.cumsum(a, dtype=np.int64)
            want = np.concatenate([[0], incl[:-1]]) if length else np.zeros(0, np.int64)
            assert np.array_equal(N(offsets).astype(np.int64), want), (name, length)
            assert int(N(total).reshape(-1)[0]) == (int(incl[-1]) if length else 0), (name, length)
    # a view that does not start on a 4-byte boundary
    offsets, total = n.exclusive_scan(G(draw)[3:5000])
    assert np.array_equal(N(offsets).astype(np.int64), np.concatenate([[0], np.cumsum(draw[3:4999], dtype=np.int64)]))
    assert int(N(total)[0]) == int(draw[3:5000].sum(dtype=np.int64))
    with pytest.raises(ValueError):
        n.exclusive_scan(G(draw[:8]).to(torch.int32))
    with pytest.raises(ValueError):
        n.exclusive_scan(torch.zeros(8, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------ 2. meshes: the host statement
def test_small_volumes_give_empty_meshes_of_the_right_shapes(env, binding):
    n = env["native"]
    for dims in ((1, 1, 1), (1, 5, 5), (2, 2, 2)):
        D = np.where(np.arange(np.prod(dims)).reshape(dims) % 2 == 0, 0.5, -0.5).astype(_F)
        for W in (np.ones(dims, _F), np.zeros(dims, _F)):
            f = ms.field(D, W, np.ones((2,) + dims, _F))
            ref = _check(n, ("small", dims, float(W.sum())), f)
            if dims[0] == 1 or not W.any():
                assert ref["vertices"].shape == (0, 3) and ref["faces"].shape == (0, 3) and ref["feat"].shape == (2, 0)
            else:
                assert len(ref["faces"]) > 0
            out = _run(n, f, normals=False)
            assert out["normal"] is None and out["normal_valid"] is None


@pytest.mark.parametrize("holes", [False, True])
def test_the_planted_volume(env, binding, holes):
    ref = _check(env["native"], ("planted", holes), ms.planted(holes))
    assert len(ref["faces"]) > 500


def test_the_ellipsoid(env, binding):
    ref = _check(env["native"], "ellipsoid", ms.ellipsoid())
    assert ref["faces"].shape == (1972, 3) and ref["vertices"].shape == (988, 3)


@pytest.mark.parametrize("dims", [(5, 7, 9), ms.BIG])
def test_the_fusion_scene(env, binding, dims):
    n = env["native"]
    triangles = 0
    for V in (1, 3, 8):
        for C, normals, min_weight in ((2, True, 0.0), (0, False, 0.0), (2, False, 1.5), (0, True, 1.5)):
            ref = _check(n, ("scene", dims, V, C), ms.scene_field(dims, V, C), min_weight, normals)
            triangles += len(ref["faces"])
    assert triangles > (20000 if dims == ms.BIG else 0)


def test_rotated_views_on_three_lattices(env, binding):
    ref = _check(env["native"], "lattice", ms.lattice_field())
    assert len(ref["faces"]) > 1000


def test_the_second_level_of_the_scan(env, binding):
    f = ms.slanted()
    ref = _check(env["native"], "slanted", f)
    assert int(ref["edge"].max()) // 7 > PASS and len(ref["faces"]) > 50000


def test_tsdf_mesh_of_a_volume_and_the_empty_volume(env, binding):
    n = env["native"]
    views = fs.scene(8, C=2)
    on_gpu = [dict(v, depth=G(v["depth"]), weight=G(v["weight"]), feat=G(v["feat"])) for v in views]
    vol = n.tsdf_integrate(n.tsdf_volume(C=2, device=DEV, **ms.describe(ms.BIG)), on_gpu, near=fs.NEAR)
    ref = ms.reference(("scene", ms.BIG, 8, 2), ms.scene_field(ms.BIG, 8, 2))
    assert ms.same(_host(n.tsdf_mesh(vol)), ref)
    assert ms.same(_host(n.tsdf_mesh(vol, min_weight=1.5, normals=False)), ms.reference(("scene", ms.BIG, 8, 2), ms.scene_field(ms.BIG, 8, 2), 1.5, False))
    empty = _host(n.tsdf_mesh(n.tsdf_volume(C=2, device=DEV, **ms.describe(ms.BIG))))
    assert empty["vertices"].shape == (0, 3) and empty["faces"].shape == (0, 3) and empty["feat"].shape == (2, 0) and empty["edge"].shape == (0,)
    assert empty["normal"].shape == (0, 3) and empty["normal_valid"].shape == (0,)


def test_repeats_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    f = ms.scene_field(ms.BIG, 8, 2)
    ref = ms.reference(("scene", ms.BIG, 8, 2), f)
    D, W, Fm = G(f["D"]), G(f["W"]), G(f["Fm"])
    for _ in range(2):
        assert ms.same(_host(n.mesh_field(D, W, Fm, f["origin"], f["voxel"])), ref)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = n.mesh_field(D, W, Fm, f["origin"], f["voxel"])
    side.synchronize()
    assert ms.same(_host(out), ref)


def test_rejected_inputs(env, binding):
    n = env["native"]
    D = G(np.ones((3, 4, 5), _F))
    n.mesh_field(D, D)
    for bad in (dict(D=D.cpu(), W=D.cpu()), dict(W=D[:2]), dict(W=D.cpu()), dict(D=D.double()), dict(Fm=D), dict(Fm=D[None].cpu()),
                dict(voxel=(1, 0, 1)), dict(origin=(0, 0)), dict(min_weight=-1.0), dict(min_weight=float("nan")), dict(D=N(D))):
        with pytest.raises(ValueError):
            n.mesh_field(**dict(dict(D=D, W=D), **bad))
    with pytest.raises(ValueError):
        n.tsdf_mesh(volume.Volume(C=0, **ms.describe((5, 7, 9))))           # numpy sums: the host statement's volume


# ------------------------------------------------------------------------------------------ 3. DepthPipeline.extract_mesh / save_mesh
def test_pipeline_extract_mesh_and_save_mesh(env, pipe, binding, tmp_path):
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
    half = 0.55 * W / cam.fx * hi                                        # the volume of test_tsdf_gpu.py's pipeline test
    desc = dict(dims=(48, 32, 32), origin=(-half, -half, lo - 0.06), voxel=(2 * half / 31, 2 * half / 31, (hi - lo + 0.12) / 47), trunc=0.05)
    poses = [None, camera.pose(None, (0.0004, -0.0002, 0.001)), camera.pose(None, (-0.0003, 0.0005, -0.002))]
    vol = p.integrate([(maps, q) for q in poses], want=("shpd",), **desc)
    out = p.extract_mesh(vol)
    assert set(out) == {"vertices", "faces", "weight", "shpd", "normal", "normal_valid"}
    V, T = out["vertices"].shape[0], out["faces"].shape[0]
    print(f"pipeline scene: {V} vertices, {T} triangles")
    assert V > 0 and T > 0 and out["shpd"].shape == (3, V) and out["normal"].shape == (V, 3)
    nat = n.tsdf_mesh(vol)
    assert _same_bits(out["shpd"], nat["feat"]) and _same_bits(out["vertices"], nat["vertices"]) and torch.equal(out["faces"], nat["faces"])
    assert ms.same(_host(nat), mesh.extract_volume(vol.numpy()))
    plain = p.extract_mesh(vol, min_weight=0.5, normals=False)
    assert plain["normal"] is None and plain["normal_valid"] is None and plain["vertices"].shape[0] <= V
    path = str(tmp_path / "mesh.ply")
    p.save_mesh(path, out)
    back = mesh.read_ply(path)
    assert np.array_equal(back["vertices"].view(np.uint32), N(out["vertices"]).view(np.uint32)) and np.array_equal(back["faces"], N(out["faces"]))
    assert np.array_equal(back["normal"].view(np.uint32), N(out["normal"]).view(np.uint32))
    assert back["colour"].shape == (3, V) and np.array_equal(back["colour"], np.floor(np.clip(N(out["shpd"]), 0, 1) * _F(255) + _F(0.5)).astype(np.uint8))
    p.save_mesh(path, plain)
    assert mesh.read_ply(path)["normal"] is None


# ------------------------------------------------------------------------------------------ 4. the workflow settings
def test_workflow_eval_fuse_writes_the_mesh(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` whose settings hold the tsdf_* keys and tsdf_mesh = 1: beside
    fused_0000.npz and tsdf_0000.npz the group's mesh, mesh_0000.ply and mesh_0000.npz, which agree."""
    import os
    from conftest import ROOT
    from be_hip import datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "fuse.npz", poses=poses, tau=0.03, tsdf_dims=(64, 32, 32), tsdf_origin=(-0.02, -0.02, 0.6), tsdf_voxel=(0.0013, 0.0013, 0.01),
             tsdf_trunc=0.04, tsdf_mesh=1)
    out = tmp_path / "fused"
    wf.main(["eval", "--fuse", str(tmp_path / "fuse.npz"), "--out_path", str(out), "--model_path", os.path.join(ROOT, "checkpoints"),
             "--data_path", str(data_dir), "--cuda", DEV])
    assert sorted(os.listdir(out)) == ["fused_0000.npz", "mesh_0000.npz", "mesh_0000.ply", "tsdf_0000.npz"]
    got = dict(np.load(out / "mesh_0000.npz"))
    assert set(got) == {"vertices", "faces", "weight", "shpd", "normal", "normal_valid"}
    V = got["vertices"].shape[0]
    print(f"workflow: {V} vertices, {got['faces'].shape[0]} triangles")
    assert V > 0 and got["faces"].shape[0] > 0 and got["faces"].max() < V and got["shpd"].shape == (3, V) and got["faces"].dtype == np.int32
    ply = mesh.read_ply(str(out / "mesh_0000.ply"))
    assert np.array_equal(ply["vertices"], got["vertices"]) and np.array_equal(ply["faces"], got["faces"]) and ply["colour"].shape == (3, V)
