"""GPU tests of the truncated signed distance volume (be_tsdf_integrate_f32, be_tsdf_mean_f32, be_tsdf_raycast_f32; native.tsdf_volume /
tsdf_integrate / tsdf_mean / tsdf_raycast; DepthPipeline.integrate / raycast).

One bit contract: the sums (as integers) and every float output (as uint32) equal the numpy statement of be_hip/volume.py, which
test_tsdf_cpu.py ties to a volume worked by hand, to a plane, to its own float64 evaluation and to the prototype's quality
figures.  Beside it: neither the order of the views, nor their grouping into calls, nor a repeated run, nor a side stream changes
a bit.  The scenes are those of tests/fuse_scenes.py and tests/reproject_scenes.py; the pipeline fixtures and scene are those of
test_render_at_gpu.py."""
import numpy as np
import pytest
import torch

from be_hip import camera, volume
import fuse_scenes as fs
import reproject_scenes as rs
from test_render_at_gpu import DEV, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
_F = np.float32
# (Nz, Ny, Nx) -> trunc: every volume spans X in [-0.5, 0.5], Y in [-0.35, 0.35], Z in [0.62, 1.2] - the scene of fuse_scenes; the
# coarse ones take a truncation of their voxels' size so that voxels take part at all.  33 x 40 x 65 = 85800 voxels: 335 full
# workgroups and a tail of 40 threads, rows of 65 that straddle the waves
VOLUMES = {(1, 1, 1): 0.5, (2, 2, 2): 0.5, (5, 7, 9): 0.2, (33, 40, 65): 0.04}
BIG = (33, 40, 65)
Z_RANGE = (0.65, 1.25)


def _describe(dims):
    nz, ny, nx = dims
    voxel = (1.0 / nx, 0.7 / ny, 0.58 / nz)
    return dict(dims=dims, origin=(-0.5 + voxel[0] / 2, -0.35 + voxel[1] / 2, 0.62 + voxel[2] / 2), voxel=voxel, trunc=VOLUMES[dims])


def _on_gpu(views):
    return [dict(v, depth=G(v["depth"]), weight=None if v.get("weight") is None else G(v["weight"]),
                 feat=None if v.get("feat") is None else G(v["feat"])) for v in views]


def _variant(views, weights, C):
    return [dict(v, weight=v["weight"] if weights else None, feat=v["feat"][:C] if C else None) for v in views]


_REFS = {}


def _ref(key, dims, views, C):
    """volume.integrate once per case: both bindings share the result, and nothing changes it afterwards."""
    if key not in _REFS:
        _REFS[key] = volume.integrate(volume.Volume(C=C, **_describe(dims)), views, fs.NEAR)
    return _REFS[key]


def _same_sums(vol, ref):
    """The GPU volume's sums against a numpy volume's, as integers."""
    for name, dt in (("sw", torch.int32), ("swd", torch.int64), ("swf", torch.int64)):
        t = getattr(vol, name)
        assert t.dtype == dt and t.is_cuda and t.is_contiguous(), name
        a, b = N(t), getattr(ref, name)
        assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (name, int((a != b).sum()))
    return True


def _new(n, dims, C=0):
    return n.tsdf_volume(C=C, device=DEV, **_describe(dims))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_cast(out, ref, C):
    assert set(out) >= {"depth", "valid", "weight", "feat"}
    Ho, Wo = ref["depth"].shape
    for k in ("depth", "weight"):
        assert out[k].shape == (Ho, Wo) and out[k].dtype == torch.float32 and out[k].is_contiguous(), k
        assert np.array_equal(_bits(N(out[k])), _bits(ref[k])), (k, int((_bits(N(out[k])) != _bits(ref[k])).sum()))
    assert out["valid"].dtype == torch.bool and np.array_equal(N(out["valid"]), ref["valid"])
    assert bool(torch.isfinite(out["depth"]).all())
    if C:
        assert out["feat"].shape == (C, Ho, Wo) and np.array_equal(_bits(N(out["feat"])), _bits(ref["feat"]))
    else:
        assert out["feat"] is None and ref["feat"] is None
    return True


# ------------------------------------------------------------------------------------------ 1. integrate: the host statement
@pytest.mark.parametrize("dims", list(VOLUMES))
def test_integrate_equals_the_host_statement(env, binding, dims):
    n = env["native"]
    took_part = 0
    for V in (1, 3, 8):
        scene = fs.scene(V, C=2)
        for weights, C in ((True, 2), (False, 0), (True, 0), (False, 2)):
            views = _variant(scene, weights, C)
            vol = _new(n, dims, C)
            assert n.tsdf_integrate(vol, _on_gpu(views), near=fs.NEAR) is vol
            ref = _ref(("scene", dims, V, weights, C), dims, views, C)
            assert _same_sums(vol, ref), (V, weights, C)
            took_part += int((ref.sw != 0).sum())
    assert took_part > 0                                                 # every volume, the single voxel included, holds something


def _lattice_views(C):
    views = []
    for k in (1, 3, 2):
        scale, win, (Hs, Ws) = rs.LATTICES[k]
        views.append(dict(depth=rs.lattice_depth(k), weight=None, feat=rs.feat_for(Hs, Ws, C) if C else None, cam_src=rs.SRC,
                          pose=rs.reference_pose(), scale=scale, window_origin=win[:2]))
    return views


def test_integrate_rotated_views_on_three_lattices(env, binding):
    """The rotated reference view of reproject_scenes on the lattices of scale 1, 3 (window origin (5, 7)) and 2: each alone, so that
    a slip in one lattice's arithmetic cannot hide behind another's samples, and all three in one volume."""
    n = env["native"]
    views = _lattice_views(2)
    for pick in ((0,), (1,), (2,), (0, 1, 2)):
        sub = [views[i] for i in pick]
        vol = n.tsdf_integrate(_new(n, BIG, 2), _on_gpu(sub), near=rs.NEAR)
        ref = _ref(("lattice", pick), BIG, sub, 2)
        assert int((ref.sw != 0).sum()) > 1000
        assert _same_sums(vol, ref), pick


def _planted():
    """scene(3, C=2) with NaN, infinite, negative and zero depths and weights planted, and NaN and huge channels."""
    views = [dict(v, depth=v["depth"].copy(), weight=v["weight"].copy(), feat=v["feat"].copy()) for v in fs.scene(3, C=2)]
    bad = (np.nan, np.inf, -np.inf, -0.9, 0.0, -0.0)
    for i, v in enumerate(views):
        for j, b in enumerate(bad):
            v["depth"][3 + 4 * j + i, 5:40:3] = b
            v["weight"][4 + 4 * j + i, 7:50:4] = b
        v["weight"][30:33, 10:30] = (1e-4, 30.0, 1e30)[i]               # quantises to 0; clamps to 16; clamps to 16
        v["feat"][0, 8:12, :] = np.nan
        v["feat"][1, 20:24, :] = (1e9, -1e9, np.inf)[i]
    return views


def test_integrate_planted_values(env, binding):
    n = env["native"]
    views = _planted()
    vol = n.tsdf_integrate(_new(n, BIG, 2), _on_gpu(views), near=fs.NEAR)
    ref = _ref("planted", BIG, views, 2)
    clean = _ref(("scene", BIG, 3, True, 2), BIG, _variant(fs.scene(3, C=2), True, 2), 2)
    assert int((ref.sw != clean.sw).sum()) > 100                         # the planted samples did reach voxels
    assert _same_sums(vol, ref)


@pytest.mark.parametrize("t", [(0.0, 0.0, 5.0), (5.0, 0.0, 0.0)], ids=["behind", "outside"])
def test_integrate_nothing_in_view_leaves_the_sums_zero(env, binding, t):
    """A pose 5 m ahead of the volume puts every voxel behind the camera (Z < 0); one 5 m to the side puts every voxel far
    outside the frame."""
    n = env["native"]
    views = [dict(v, pose=camera.pose(None, t)) for v in fs.scene(3, C=2)]
    for dims in VOLUMES:
        vol = n.tsdf_integrate(_new(n, dims, 2), _on_gpu(views), near=fs.NEAR)
        ref = _ref(("nothing", dims, t), dims, views, 2)
        assert not ref.sw.any() and not ref.swd.any() and not ref.swf.any()
        assert _same_sums(vol, ref)


def test_integrate_order_grouping_repeats_and_streams(env, binding):
    n = env["native"]
    views = _variant(fs.scene(8, C=2), True, 2)
    dev = _on_gpu(views)
    ref = _ref(("scene", BIG, 8, True, 2), BIG, views, 2)
    for perm in ((7, 6, 5, 4, 3, 2, 1, 0), (3, 0, 6, 1, 7, 4, 2, 5)):
        assert _same_sums(n.tsdf_integrate(_new(n, BIG, 2), [dev[i] for i in perm], near=fs.NEAR), ref), perm
    vol = _new(n, BIG, 2)
    for v in dev:                                                       # one call per view into the same volume
        n.tsdf_integrate(vol, [v], near=fs.NEAR)
    assert _same_sums(vol, ref)
    vol = n.tsdf_integrate(n.tsdf_integrate(_new(n, BIG, 2), dev[:3], near=fs.NEAR), dev[3:], near=fs.NEAR)
    assert _same_sums(vol, ref)
    assert _same_sums(n.tsdf_integrate(_new(n, BIG, 2), dev, near=fs.NEAR), ref)     # a repeated run
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        vol = n.tsdf_integrate(_new(n, BIG, 2), dev, near=fs.NEAR)
        cast = n.tsdf_raycast(vol, fs.CAM, None, fs.SIZE, Z_RANGE)
    side.synchronize()
    assert _same_sums(vol, ref)
    assert _same_cast(cast, _cast_ref(BIG, "scene", fs.SIZE, None), 2)


# ------------------------------------------------------------------------------------------ 2. mean and ray cast
CAMERAS = {"scene": (fs.CAM, None), "rotated": (rs.DST, rs.reference_pose())}
_CASTS = {}


def _cast_ref(dims, which, size, step, z_range=Z_RANGE):
    key = (dims, which, size, step, z_range)
    if key not in _CASTS:
        views = _variant(fs.scene(8, C=2), True, 2)
        cam, pose = CAMERAS[which]
        _CASTS[key] = volume.raycast(_ref(("scene", dims, 8, True, 2), dims, views, 2), cam, pose, size, z_range, step)
    return _CASTS[key]


@pytest.mark.parametrize("dims", list(VOLUMES))
def test_mean_and_raycast_equal_the_host_statement(env, binding, dims):
    n = env["native"]
    views = _variant(fs.scene(8, C=2), True, 2)
    ref_vol = _ref(("scene", dims, 8, True, 2), dims, views, 2)
    vol = n.tsdf_integrate(_new(n, dims, 2), _on_gpu(views), near=fs.NEAR)
    got, want = n.tsdf_mean(vol), volume.mean(ref_vol)
    for g, w, name in zip(got, want, ("D", "W", "Fm")):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape and np.array_equal(_bits(N(g)), _bits(w)), name
    assert float(got[0].abs().max()) <= 1.0
    hits = 0
    for which, (cam, pose) in CAMERAS.items():
        for size in ((1, 1), (37, 53), (41, 67)):
            for step in (None, VOLUMES[dims]):                          # trunc / 4 and trunc
                out = n.tsdf_raycast(vol, cam, pose, size, Z_RANGE, step=step)
                ref = _cast_ref(dims, which, size, step)
                assert _same_cast(out, ref, 2), (which, size, step)
                assert torch.equal(out["valid"], out["depth"] > 0)
                hits += int(ref["valid"].sum())
    if dims == BIG:
        assert hits > 3000 and int(_cast_ref(dims, "rotated", (41, 67), None)["valid"].sum()) > 500
    elif dims[0] == 1:
        assert hits == 0                                                # no cell of 8 voxels in a single layer


def test_raycast_ranges_without_a_surface_and_the_empty_volume(env, binding):
    n = env["native"]
    views = _variant(fs.scene(8, C=2), True, 2)
    vol = n.tsdf_integrate(_new(n, BIG, 2), _on_gpu(views), near=fs.NEAR)
    # a range that starts inside the wall (3 cm behind its face, within trunc: valid samples, F < 0) and one that ends before the square
    for zr in ((1.13, 1.25), (0.65, 0.74)):
        out, ref = n.tsdf_raycast(vol, fs.CAM, None, fs.SIZE, zr), _cast_ref(BIG, "scene", fs.SIZE, None, zr)
        assert not ref["valid"].any(), zr
        assert _same_cast(out, ref, 2)
        assert not bool(out["depth"].any()) and not bool(out["weight"].any()) and not bool(out["feat"].any()) and not bool(out["valid"].any())
    empty = _new(n, BIG, 2)
    for t in n.tsdf_mean(empty):
        assert not bool(t.view(torch.int32).any())                       # +0 everywhere
    out = n.tsdf_raycast(empty, fs.CAM, None, fs.SIZE, Z_RANGE)
    for k in ("depth", "weight", "feat"):
        assert not bool(out[k].view(torch.int32).any()), k
    assert not bool(out["valid"].any())


def test_raycast_normals_are_depth_normals_of_the_returned_depth(env, binding):
    n = env["native"]
    views = _variant(fs.scene(8), True, 0)
    vol = n.tsdf_integrate(_new(n, BIG), _on_gpu(views), near=fs.NEAR)
    out = n.tsdf_raycast(vol, fs.CAM, None, fs.SIZE, Z_RANGE, normals=True, normals_kw=dict(step=2))
    ref = n.depth_normals(out["depth"], fs.CAM, step=2)
    assert out["normal"].shape == (3,) + fs.SIZE and _same_bits(out["normal"], ref["normal"]) and torch.equal(out["normal_valid"], ref["valid"])
    assert int(out["normal_valid"].sum()) > 1000 and out["feat"] is None
    plain = n.tsdf_raycast(vol, fs.CAM, None, fs.SIZE, Z_RANGE)
    assert "normal" not in plain and _same_bits(plain["depth"], out["depth"])


def test_rejected_inputs(env, binding):
    n = env["native"]
    with pytest.raises(ValueError):
        n.tsdf_volume((0, 4, 4), (0, 0, 0), (0.01, 0.01, 0.01), 0.05, device=DEV)
    with pytest.raises(ValueError):
        n.tsdf_volume((4, 4, 4), (0, 0, 0), (0.01, 0.01, 0.01), 0.05, device="cpu")
    vol = _new(n, (5, 7, 9), 2)
    views = _on_gpu(_variant(fs.scene(1, C=2), True, 2))
    for bad in (dict(views[0], feat=None), dict(views[0], feat=views[0]["feat"][:1]), dict(views[0], depth=views[0]["depth"].cpu()),
                dict(views[0], weight=views[0]["weight"][:5]), dict(views[0], colour=1), dict(views[0], scale=0)):
        with pytest.raises(ValueError):
            n.tsdf_integrate(vol, [bad])
    with pytest.raises(ValueError):
        n.tsdf_integrate(volume.Volume(C=2, **_describe((5, 7, 9))), views)          # numpy sums: the host statement's volume
    assert not bool(vol.sw.any())                                        # nothing was launched
    for kw in (dict(step=0.0), dict(step=1e-6), dict(z_range=(0.0, 1.0)), dict(z_range=(1.0, 0.5)), dict(size=(0, 5)), dict(size=5)):
        with pytest.raises(ValueError):
            n.tsdf_raycast(vol, fs.CAM, None, **dict(dict(size=(3, 3), z_range=Z_RANGE), **kw))


# ------------------------------------------------------------------------------------------ 3. DepthPipeline.integrate / raycast
def test_pipeline_integrate_and_raycast(env, pipe, binding):
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
    # the frame is 147 px of a 4709.9 px focal length: 3 cm across at 1 m.  32 x 32 voxels of 1.1 mm across it, 48 along the depth range
    half = 0.55 * W / cam.fx * hi
    desc = dict(dims=(48, 32, 32), origin=(-half, -half, lo - 0.06), voxel=(2 * half / 31, 2 * half / 31, (hi - lo + 0.12) / 47), trunc=0.05)
    poses = [None, camera.pose(None, (0.0004, -0.0002, 0.001)), camera.pose(None, (-0.0003, 0.0005, -0.002)), camera.pose(None, (0.0, 0.0002, 0.0015))]
    views = [(maps, q) for q in poses]
    vol = p.integrate(views, want=("refoc",), **desc)
    assert isinstance(vol, volume.Volume) and vol.C == 3 and vol.dims == (48, 32, 32) and int((vol.sw != 0).sum()) > 0
    # the native calls on the samples _depth_samples gives, conf as the weights
    src, _ = p._depth_samples("integrate", maps, 1, None, ("refoc", "conf"), None)
    nat = [dict(depth=src["depth_map"], weight=src["conf"], feat=src["refoc"], cam_src=cam, pose=q) for q in poses]
    ref = n.tsdf_integrate(n.tsdf_volume(C=3, device=DEV, **desc), nat)
    for k in ("sw", "swd", "swf"):
        assert torch.equal(getattr(vol, k), getattr(ref, k)), k
    host = volume.integrate(volume.Volume(C=3, **desc), [dict(v, depth=N(v["depth"]), weight=N(v["weight"]), feat=N(v["feat"])) for v in nat])
    assert _same_sums(vol, host)
    # two calls of two views each against one call with all four
    twice = p.integrate(views[2:], volume=p.integrate(views[:2], want=("refoc",), **desc))
    for k in ("sw", "swd", "swf"):
        assert torch.equal(getattr(twice, k), getattr(vol, k)), k
    zr = (lo - 0.05, hi + 0.05)
    out = p.raycast(vol, z_range=zr, normals=True)
    assert set(out) == {"depth", "valid", "weight", "refoc", "normal", "normal_valid"}
    assert out["depth"].shape == (H, W) and out["refoc"].shape == (3, H, W) and out["normal"].shape == (3, H, W)
    nat_out = n.tsdf_raycast(ref, cam, None, (H, W), zr)
    assert _same_bits(out["depth"], nat_out["depth"]) and _same_bits(out["weight"], nat_out["weight"]) and _same_bits(out["refoc"], nat_out["feat"])
    assert torch.equal(out["valid"], nat_out["valid"])
    print(f"pipeline scene: {int((vol.sw != 0).sum())} voxels hold data, {int(out['valid'].sum())} of {H * W} rays hit")
    assert _same_cast(nat_out, volume.raycast(host, cam, None, (H, W), zr), 3)
    nrm = n.depth_normals(out["depth"], cam)
    assert _same_bits(out["normal"], nrm["normal"])
    other = p.raycast(vol, cam_dst=cam, pose=poses[1], size=(40, 50), z_range=zr, step=0.02)
    assert other["depth"].shape == (40, 50) and other["refoc"].shape == (3, 40, 50) and "normal" not in other
    with pytest.raises(ValueError):
        p.integrate(views, volume=vol, **desc)
    with pytest.raises(ValueError):
        p.integrate(views)


# ------------------------------------------------------------------------------------------ 4. the workflow settings
def test_workflow_eval_fuse_with_a_tsdf_volume(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` whose settings hold tsdf_dims / tsdf_origin / tsdf_voxel /
    tsdf_trunc: the group is also integrated and ray-cast into view 0's camera, tsdf_0000.npz with the documented keys."""
    import os
    from conftest import ROOT
    from be_hip import datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "fuse.npz", poses=poses, tau=0.03, tsdf_dims=(64, 32, 32), tsdf_origin=(-0.02, -0.02, 0.6), tsdf_voxel=(0.0013, 0.0013, 0.01),
             tsdf_trunc=0.04)
    cfg = wf.load_fusion(str(tmp_path / "fuse.npz"))
    assert cfg["tsdf"] == dict(dims=(64, 32, 32), origin=tuple(float(_F(v)) for v in (-0.02, -0.02, 0.6)),
                               voxel=tuple(float(_F(v)) for v in (0.0013, 0.0013, 0.01)), trunc=float(_F(0.04)))
    out = tmp_path / "fused"
    wf.main(["eval", "--fuse", str(tmp_path / "fuse.npz"), "--out_path", str(out), "--model_path", os.path.join(ROOT, "checkpoints"),
             "--data_path", str(data_dir), "--cuda", DEV])
    assert sorted(os.listdir(out)) == ["fused_0000.npz", "tsdf_0000.npz"]
    got = dict(np.load(out / "tsdf_0000.npz"))
    assert set(got) == {"depth", "valid", "weight", "normal", "shpd"}
    assert got["depth"].shape == (147, 147) and got["depth"].dtype == np.float32 and got["valid"].dtype == np.bool_
    assert got["normal"].shape == (3, 147, 147) and got["shpd"].shape == (3, 147, 147)
    assert np.isfinite(got["depth"]).all() and np.array_equal(got["valid"], got["depth"] > 0) and (got["weight"][got["valid"]] > 0).all()
    print(f"workflow: {int(got['valid'].sum())} of {got['valid'].size} rays hit")
