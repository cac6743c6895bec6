"""GPU tests of the forward reprojection (be_unproject_f32, be_reproject_f32, native.unproject, native.reproject,
DepthPipeline.point_cloud / reproject, `workflow eval --point_cloud / --reproject`).

Two bit contracts: a warp onto the same camera with the identity pose returns the input wherever the depth is valid, and every
output equals the numpy float32 statement of be_hip/camera.py (project_f32, splat_f32), which test_reproject_cpu.py ties to scenes
worked by hand and to the same function in float64.  The float64 evaluation is checked here too, as a second guard against an
error the kernels and their float32 statement might share.  The scenes are those of tests/reproject_scenes.py; the pipeline
fixtures and scenes are those of test_render_at_gpu.py."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import camera, synth
import reproject_scenes as rs
from test_render_at_gpu import DEV, T, _pixel_fold, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)

pytestmark = pytest.mark.gpu


def G(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_result(out, Ho, Wo, C):
    assert set(out) == {"depth", "index", "valid", "feat"}
    assert out["depth"].shape == (Ho, Wo) and out["depth"].dtype == torch.float32 and out["depth"].is_contiguous()
    assert out["index"].shape == (Ho, Wo) and out["index"].dtype == torch.int32
    assert out["valid"].dtype == torch.bool and torch.equal(out["valid"], out["index"] >= 0)
    if C is None:
        assert out["feat"] is None
    else:
        assert out["feat"].shape == (C, Ho, Wo) and out["feat"].dtype == torch.float32


def _equals_host(out, ref):
    """Every output of native.reproject against camera.splat's, bit for bit."""
    assert np.array_equal(_bits(N(out["depth"])), _bits(ref["depth"]))
    assert np.array_equal(N(out["index"]), ref["index"]) and np.array_equal(N(out["valid"]), ref["valid"])
    if ref["feat"] is not None:
        assert np.array_equal(_bits(N(out["feat"])), _bits(ref["feat"]))


# ------------------------------------------------------------------------------------------ 1. the identity contract
def test_identity_returns_the_input_bit_for_bit(env, binding):
    n = env["native"]
    d = rs.reference_depth()
    feat = rs.feat_for(37, 53)
    out = n.reproject(G(d), rs.SRC, rs.SRC, None, (37, 53), feat=G(feat))
    _check_result(out, 37, 53, 5)
    ok = d > 0
    own = np.arange(37 * 53, dtype=np.int32).reshape(37, 53)
    assert np.array_equal(N(out["valid"]), ok) and 0.15 < 1 - ok.mean() < 0.25
    assert np.array_equal(_bits(N(out["depth"])), _bits(np.where(ok, d, np.float32(0))))
    assert np.array_equal(N(out["index"]), np.where(ok, own, -1))
    assert np.array_equal(_bits(N(out["feat"])), _bits(np.where(ok[None], feat, np.float32(0))))
    # the pipeline's own camera (focal 4709.9 px) on a 147 x 147 image, depths over the working range
    a = env["args"]
    cam = camera.Pinhole.of(a.cam_params, a.mag, 147, 147)
    assert cam == env["dcal"].intrinsics(147, 147)
    d = (0.75 + 0.43 * np.random.default_rng(3).random((147, 147))).astype(np.float32)
    out = n.reproject(G(d), cam, cam, None, (147, 147))
    _check_result(out, 147, 147, None)
    assert bool(out["valid"].all()) and np.array_equal(_bits(N(out["depth"])), _bits(d))
    assert np.array_equal(N(out["index"]).ravel(), np.arange(147 * 147, dtype=np.int32))


# ------------------------------------------------------------------------------------------ 2. the host statement, and float64
@pytest.mark.parametrize("k", [1, 3, 2])
def test_equals_the_host_statement_bit_for_bit(env, binding, k):
    n, c = env["native"], rs.lattice_case(k)
    out = n.reproject(G(c["depth"]), rs.SRC, rs.DST, c["pose"], rs.SIZE, feat=G(c["feat"]), near=rs.NEAR, scale=c["scale"],
                      window_origin=c["origin"])
    _check_result(out, *rs.SIZE, 5)
    ref = c["r32"]
    n_in, filled = int(ref["taking_part"].sum()), int(ref["valid"].sum())
    assert (n_in, filled, n_in - filled) == rs.COUNTS[k]
    _equals_host(out, ref)
    hit = ref["valid"]
    assert np.array_equal(N(out["feat"])[:, hit], c["feat"].reshape(5, -1)[:, ref["index"][hit]])
    # the [C,Ns] form of feat, and no feat at all
    flat = n.reproject(G(c["depth"]), rs.SRC.tuple(), rs.DST.K(), c["pose"], rs.SIZE, feat=G(c["feat"].reshape(5, -1)), near=rs.NEAR,
                       scale=c["scale"], window_origin=c["origin"])
    _equals_host(flat, ref)
    bare = n.reproject(G(c["depth"]), rs.SRC, rs.DST, c["pose"], rs.SIZE, near=rs.NEAR, scale=c["scale"], window_origin=c["origin"])
    _check_result(bare, *rs.SIZE, None)
    _equals_host(bare, dict(ref, feat=None))
    # the float64 evaluation, leaving out the target pixels an ambiguous sample could reach
    rs.check_against_f64(k, N(out["depth"]), N(out["index"]), N(out["valid"]), N(out["feat"]))


# ------------------------------------------------------------------------------------------ 3. the hand-worked scenes
def test_hand_worked_shift_occlusion_and_tie(env, binding):
    n = env["native"]
    out = n.reproject(G(rs.shift_scene()), rs.HAND_CAM, rs.HAND_CAM, rs.HAND_POSE, (9, 12))
    depth, index = rs.expected_shift()
    assert np.array_equal(_bits(N(out["depth"])), _bits(depth)) and np.array_equal(N(out["index"]), index)
    assert not bool(out["valid"][:, :3].any()) and bool(out["valid"][:, 3:].all())
    feat = rs.feat_for(9, 12, 2)
    out = n.reproject(G(rs.occlusion_scene()), rs.HAND_CAM, rs.HAND_CAM, rs.HAND_POSE, (9, 12), feat=G(feat))
    depth, index = rs.expected_occlusion()
    assert np.array_equal(_bits(N(out["depth"])), _bits(depth)) and np.array_equal(N(out["index"]), index)
    assert bool((out["depth"][3:6, 8:11] == 0.5).all())
    assert np.array_equal(N(out["index"])[3:6, 8:11], np.arange(3, 6)[:, None] * 12 + np.arange(2, 5)[None, :])
    hit = index >= 0
    assert np.array_equal(N(out["feat"])[:, hit], feat.reshape(2, -1)[:, index[hit]]) and (N(out["feat"])[:, ~hit] == 0).all()
    out = n.reproject(G(rs.shift_scene()), rs.TIE_SRC, rs.TIE_DST, None, rs.TIE_SIZE)
    assert bool(out["valid"].all()) and bool((out["depth"] == 1.0).all())
    assert np.array_equal(N(out["index"]), rs.expected_tie())


# ------------------------------------------------------------------------------------------ 4. order independence
def test_runs_are_bit_equal_and_one_sample_works(env, binding):
    n = env["native"]
    # 37 * 53 = 1961, 73 * 105 = 7665 = 2501 + 5164 and 41 * 61 = 2501 samples (the first rows and columns of the k = 2 lattice): none
    # a multiple of the 256-thread workgroup, each delivered as one call
    c2 = rs.lattice_case(2)
    crop = dict(c2, depth=np.ascontiguousarray(c2["depth"][:41, :61]), feat=np.ascontiguousarray(c2["feat"][:, :41, :61]))
    for c in (rs.lattice_case(1), c2, crop):
        assert c["depth"].size % 256 != 0 and c["depth"].size in (1961, 7665, 2501)
        d, f = G(c["depth"]), G(c["feat"])
        run = lambda: n.reproject(d, rs.SRC, rs.DST, c["pose"], rs.SIZE, feat=f, near=rs.NEAR, scale=c["scale"], window_origin=c["origin"])
        first = run()
        for _ in range(2):
            again = run()
            for key in ("depth", "feat"):
                assert _same_bits(first[key], again[key]), (c["depth"].shape, key)
            assert torch.equal(first["index"], again["index"]) and torch.equal(first["valid"], again["valid"])
        _equals_host(first, camera.splat_f32(c["depth"], rs.SRC, rs.DST, c["pose"], rs.SIZE, c["feat"], rs.NEAR, c["scale"], c["origin"]))
    # a single sample: the pixel (0, 0) of a camera whose axis goes through it lands on the target's principal point
    one = n.reproject(G(np.full((1, 1), 0.9, np.float32)), (50, 50, 0, 0), (50, 50, 2, 3), None, (4, 5), feat=G(np.full((1, 1, 1), 7, np.float32)))
    _check_result(one, 4, 5, 1)
    want = np.full((4, 5), -1, np.int32)
    want[2, 3] = 0
    assert np.array_equal(N(one["index"]), want) and float(one["depth"][2, 3]) == np.float32(0.9) and float(one["feat"][0, 2, 3]) == 7
    assert int(one["valid"].sum()) == 1 and float(one["depth"].sum()) == np.float32(0.9)


# ------------------------------------------------------------------------------------------ 5. rejected samples
def test_rejected_samples_write_nothing(env, binding):
    n = env["native"]
    d = rs.shift_scene().copy()
    d[0, :4] = [0, -1, np.nan, np.inf]
    d[8, 11] = -np.inf
    feat = rs.feat_for(9, 12, 3)
    out = n.reproject(G(d), rs.HAND_CAM, rs.HAND_CAM, None, (9, 12), feat=G(feat))
    bad = ~(np.isfinite(d) & (d > 0))
    assert bad.sum() == 5
    assert np.array_equal(N(out["valid"]), ~bad) and (N(out["index"])[bad] == -1).all()
    assert (_bits(N(out["depth"]))[bad] == 0).all() and (_bits(N(out["feat"]))[:, bad] == 0).all()
    assert bool(torch.isfinite(out["depth"]).all()) and bool(torch.isfinite(out["feat"]).all())
    _equals_host(out, camera.splat_f32(d, rs.HAND_CAM, rs.HAND_CAM, None, (9, 12), feat=feat))
    # behind near: the plane Z = 1 seen from 0.9995 further along the axis has Zd = 5e-4 < near; a tilted source leaves some in front
    back = camera.pose(None, (0, 0, -0.9995))
    out = n.reproject(G(rs.shift_scene()), rs.HAND_CAM, rs.HAND_CAM, back, (9, 12), near=1e-3)
    assert not bool(out["valid"].any()) and not bool(out["depth"].any()) and bool((out["index"] == -1).all())
    ramp = (1 + 0.0002 * np.arange(12, dtype=np.float32))[None, :].repeat(9, 0)                 # Zd = 5e-4 .. 2.7e-3
    wide = camera.Pinhole(0.064, 0.064, 10, 10)                         # so close to the camera the plane's image is magnified ~ 1000 x
    ref = camera.splat_f32(ramp, rs.HAND_CAM, wide, back, (21, 21), near=1e-3)
    assert 0 < ref["valid"].sum() < 9 * 12 and not ref["taking_part"][:, :3].any() and ref["taking_part"][:, 3:].all()
    out = n.reproject(G(ramp), rs.HAND_CAM, wide, back, (21, 21), near=1e-3)
    _equals_host(out, ref)
    assert bool(torch.isfinite(out["depth"]).all())
    # a finite depth whose Zd overflows to +inf does not take part: every depth written is finite
    big = np.zeros((9, 12), np.float32)
    big[4, 6] = 3e38                                                    # on the optical axis: u = 0 / inf + cx is in frame
    away = camera.pose(None, (0, 0, 3e38))                              # Zd = 3e38 + 3e38 = inf
    p32 = camera.project_f32(big, rs.HAND_CAM, rs.HAND_CAM, away)
    assert np.isinf(p32["xyz"][2][4, 6]) and p32["z_ok"][4, 6] and (p32["fv"][4, 6], p32["fu"][4, 6]) == (4, 6)
    ref = camera.splat(p32, (9, 12))
    assert not ref["taking_part"].any()
    out = n.reproject(G(big), rs.HAND_CAM, rs.HAND_CAM, away, (9, 12))
    _equals_host(out, ref)
    assert not bool(out["valid"].any()) and (_bits(N(out["depth"])) == 0).all()
    # outside the frame on each of the four sides: a 5 x 6 target in the middle of the 9 x 12 plane's image
    crop = camera.Pinhole(64, 64, 4 - 2, 6 - 3)
    out = n.reproject(G(rs.shift_scene()), rs.HAND_CAM, crop, None, (5, 6), feat=G(rs.feat_for(9, 12, 3)))
    assert bool(out["valid"].all())
    assert np.array_equal(N(out["index"]), (np.arange(2, 7)[:, None] * 12 + np.arange(3, 9)[None, :]).astype(np.int32))
    assert np.array_equal(N(out["feat"]), rs.feat_for(9, 12, 3)[:, 2:7, 3:9])
    ref = camera.splat_f32(rs.shift_scene(), rs.HAND_CAM, crop, None, (5, 6))
    part = ref["taking_part"]
    assert part.sum() == 30 and not part[:2].any() and not part[7:].any() and not part[:, :3].any() and not part[:, 9:].any()
    # a target that no sample reaches
    far = n.reproject(G(rs.shift_scene()), rs.HAND_CAM, camera.Pinhole(64, 64, -500, 7000), None, (6, 7), feat=G(rs.feat_for(9, 12, 3)))
    assert not bool(far["valid"].any()) and (_bits(N(far["depth"])) == 0).all() and (_bits(N(far["feat"])) == 0).all()
    # the argument checks
    g = G(rs.shift_scene())
    for kw, match in ((dict(size=(0, 4)), "size"), (dict(size=(3,)), "size"), (dict(scale=0), "scale"), (dict(scale=17), "scale"),
                      (dict(near=-1.0), "near"), (dict(feat=G(np.zeros((2, 9, 11), np.float32))), "feat"),
                      (dict(feat=np.zeros((2, 9, 12), np.float32)), "feat"), (dict(window_origin=(-1, 0)), "window_origin"),
                      (dict(pose=np.diag([1, 1, 2, 1.0])), "rotation"), (dict(cam_dst=(1, 2, 3)), "cam_dst")):
        a = dict(cam_src=rs.HAND_CAM, cam_dst=rs.HAND_CAM, pose=None, size=(9, 12))
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            n.reproject(g, **a)
    with pytest.raises(ValueError, match="GPU"):
        n.reproject(g.cpu(), rs.HAND_CAM, rs.HAND_CAM, None, (9, 12))
    with pytest.raises(ValueError, match="float32"):
        n.reproject(g.double(), rs.HAND_CAM, rs.HAND_CAM, None, (9, 12))
    with pytest.raises(ValueError, match="float32"):
        n.unproject(g[0], rs.HAND_CAM)


# ------------------------------------------------------------------------------------------ 6. unproject
@pytest.mark.parametrize("k", [1, 3, 2])
def test_unproject_equals_the_host_statement(env, binding, k):
    n, c = env["native"], rs.lattice_case(k)
    xyz = n.unproject(G(c["depth"]), rs.SRC, c["pose"], scale=c["scale"], window_origin=c["origin"])
    assert xyz.shape == (3,) + c["depth"].shape and xyz.dtype == torch.float32 and xyz.is_contiguous()
    ref = camera.unproject_f32(c["depth"], rs.SRC, c["pose"], c["scale"], c["origin"])
    assert np.array_equal(_bits(N(xyz)), _bits(ref))
    assert (N(xyz)[:, c["depth"] == 0] == 0).all()
    out = n.reproject(G(c["depth"]), rs.SRC, rs.DST, c["pose"], rs.SIZE, near=rs.NEAR, scale=c["scale"], window_origin=c["origin"])
    hit = out["valid"]
    assert int(hit.sum()) == rs.COUNTS[k][1]
    assert _same_bits(out["depth"][hit], xyz[2].reshape(-1)[out["index"][hit].long()])
    # without a pose the points are in the camera's own frame: Z is the depth itself
    own = n.unproject(G(c["depth"]), rs.SRC, scale=c["scale"], window_origin=c["origin"])
    assert np.array_equal(_bits(N(own[2])), _bits(c["depth"]))


# ------------------------------------------------------------------------------------------ 7. the pipeline
def _maps_of(env, sc, thres):
    """The dict a pipeline entry returns, from the records of a test_render_at_gpu scene (no network runs)."""
    maps = dict(_pixel_fold(env, sc))
    maps["depth_map"] = torch.where(maps["conf"] > thres, maps["depth"], torch.zeros_like(maps["depth"]))
    g = sc["grid"]
    maps.update(records=sc["rec"], grid=dict(H=sc["H"], W=sc["W"], hp=g.get("hp", len(sc["ys"])), wp=g.get("wp", len(sc["xs"])),
                                             stride=g.get("stride", 2), ys=g.get("ys"), xs=g.get("xs")))
    return maps


@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_pipeline_reproject_and_point_cloud(env, pipe, binding, kind, densify):
    from be_hip.pipeline import DepthPipeline
    sc = _scene(env, kind, densify)
    H, W = sc["H"], sc["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify=densify)
    maps = _maps_of(env, sc, p.depth_thres)
    has = maps["depth_map"] > 0
    print(f"{kind}, densify {densify}: {int(has.sum())} of {H * W} pixels have depth")
    assert int(has.sum()) > 0
    # the defaults: the same camera, the identity pose, the same size - the maps themselves wherever there is depth
    out = p.reproject(maps)
    assert set(out) == {"depth", "valid", "index", "lattice", "shpd"}
    assert out["lattice"] == dict(scale=1, window=(0, 0, H, W), Ho=H, Wo=W)
    assert out["depth"].shape == (H, W) and out["shpd"].shape == (3, H, W) and out["index"].dtype == torch.int32
    assert torch.equal(out["valid"], has)
    assert _same_bits(out["depth"][has], maps["depth_map"][has]) and not bool(out["depth"][~has].any())
    assert _same_bits(out["shpd"][:, has], maps["shpd"][:, has]) and not bool(out["shpd"][:, ~has].any())
    assert torch.equal(out["index"][has].long(), torch.arange(H * W, device=DEV).view(H, W)[has])
    # every map rides along, with render_at's channel counts
    full = p.reproject(maps, want=("image", "refoc", "conf"))
    assert full["image"].shape == (2, 3, H, W) and full["refoc"].shape == (3, H, W) and full["conf"].shape == (H, W)
    assert _same_bits(full["image"][..., has], maps["image"][..., has]) and _same_bits(full["conf"][has], maps["conf"][has])
    assert _same_bits(full["refoc"][:, has], maps["refoc"][:, has])
    assert set(p.reproject(maps, want=())) == {"depth", "valid", "index", "lattice"}
    # maps["depth_map"] is the source at the defaults whatever threshold made it (run_big / run_any: 0.05) and whichever maps are held
    other = dict(maps, depth_map=maps["depth_map"].clone())
    other["depth_map"][:, :W // 2] = 0                                  # a depth_map no threshold of render_at reproduces
    del other["refoc"]
    has3 = other["depth_map"] > 0
    assert 0 < int(has3.sum()) < int(has.sum())
    part = p.reproject(other, want=("refoc", "shpd"))
    assert torch.equal(part["valid"], has3) and _same_bits(part["depth"][has3], other["depth_map"][has3])
    assert _same_bits(part["refoc"][:, has3], maps["refoc"][:, has3]) and not bool(part["refoc"][:, ~has3].any())
    # a finer source lattice onto the same camera and size: k^2 samples per pixel, every pixel that had depth still has
    fine = p.reproject(maps, scale=2, depth_thres=p.depth_thres)
    assert fine["lattice"]["scale"] == 2 and fine["depth"].shape == (H, W) and fine["shpd"].shape == (3, H, W)
    assert bool((fine["valid"] | ~has).all()) and bool(torch.isfinite(fine["depth"]).all()) and bool(torch.isfinite(fine["shpd"]).all())
    assert int(fine["index"].max()) < (2 * H - 1) * (2 * W - 1)
    # another camera: half the size, half the focal length, moved 2 mm to the right - against the host statement
    cam = env["dcal"].intrinsics(H, W)
    half = camera.Pinhole(cam.fy / 2, cam.fx / 2, (H // 2 - 1) / 2, (W // 2 - 1) / 2)
    pose = camera.pose(None, (-0.002, 0, 0))
    out = p.reproject(maps, cam_dst=half, pose=pose, size=(H // 2, W // 2), want=("refoc",))
    ref = camera.splat_f32(N(maps["depth_map"]), cam, half, pose, (H // 2, W // 2), feat=N(maps["refoc"]))
    assert 0 < ref["valid"].sum() and np.array_equal(N(out["index"]), ref["index"])
    assert np.array_equal(_bits(N(out["depth"])), _bits(ref["depth"])) and np.array_equal(_bits(N(out["refoc"])), _bits(ref["feat"]))
    # the point cloud: Z is the depth map, the rest the host statement
    pc = p.point_cloud(maps)
    assert set(pc) == {"xyz", "valid", "shpd", "conf", "lattice"} and pc["xyz"].shape == (3, H, W)
    # (k_unproject writes 0 where the depth is not a finite number > 0; depth_map is 0 there already unless a fold went negative)
    assert torch.equal(pc["xyz"][2], torch.where(has, maps["depth_map"], torch.zeros_like(maps["depth_map"]))) and torch.equal(pc["valid"], has)
    print(f"{kind}, densify {densify}: depth_map min {float(maps['depth_map'].min()):.4g} max {float(maps['depth_map'].max()):.4g}")
    assert _same_bits(pc["shpd"], maps["shpd"]) and _same_bits(pc["conf"], maps["conf"])
    assert np.array_equal(_bits(N(pc["xyz"])), _bits(camera.unproject_f32(N(maps["depth_map"]), cam)))
    win = (H - 30, W - 41, 30, 41)
    pcw = p.point_cloud(maps, scale=2, window=win, depth_thres=p.depth_thres)
    assert pcw["xyz"].shape == (3, 59, 81) and pcw["lattice"]["window"] == win
    assert _same_bits(pcw["xyz"][:, ::2, ::2], pc["xyz"][:, H - 30:, W - 41:])


def test_pipeline_reproject_errors_and_densify_pp(env, pipe):
    from be_hip.pipeline import DepthPipeline
    img = T(synth.synthetic_image_pair(147, 147, nshape=8)[0]).to(DEV)
    maps = pipe(img)                                                    # a live pipeline: what __call__ returned
    has = maps["depth_map"] > 0
    out = pipe.reproject(maps)
    assert torch.equal(out["valid"], has) and _same_bits(out["depth"][has], maps["depth_map"][has])
    assert _same_bits(out["shpd"][:, has], maps["shpd"][:, has])
    assert bool(has.any()) and torch.equal(pipe.point_cloud(maps)["xyz"][2], torch.where(has, maps["depth_map"], torch.zeros_like(maps["depth_map"])))
    with pytest.raises(ValueError, match="records"):
        pipe.reproject({k: v for k, v in maps.items() if k != "records"})
    with pytest.raises(ValueError, match="grid"):
        pipe.point_cloud({k: v for k, v in maps.items() if k != "grid"})
    with pytest.raises(ValueError, match="lacks"):
        pipe.reproject(None)
    with pytest.raises(ValueError, match="GPU"):
        pipe.reproject(dict(maps, records=maps["records"].cpu()))
    with pytest.raises(ValueError, match="GPU"):
        pipe.point_cloud(dict(maps, records=maps["records"].cpu()))
    with pytest.raises(ValueError, match="unknown maps"):
        pipe.reproject(maps, want=("depth_map",))
    for size in ((0, 147), (147,), (147.5, 147)):
        with pytest.raises(ValueError, match="size"):
            pipe.reproject(maps, size=size)
    with pytest.raises(ValueError, match="scale"):
        pipe.reproject(maps, scale=17)
    with pytest.raises(ValueError, match="near"):
        pipe.reproject(maps, near=-1)
    with pytest.raises(ValueError, match="rotation"):
        pipe.reproject(maps, pose=np.diag([1.0, 2, 1, 1]))
    # densify == 'pp': depth_map is the U-Net's, defined on the pixels alone (the module is not called here)
    pp = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify="pp", densify_pp_module=torch.nn.Identity())
    dense = dict(maps, depth_map=maps["depth"].abs() + 0.5)
    out = pp.reproject(dense)
    assert bool(out["valid"].all()) and _same_bits(out["depth"], dense["depth_map"]) and _same_bits(out["shpd"], maps["shpd"])
    assert torch.equal(pp.point_cloud(dense)["xyz"][2], dense["depth_map"])
    win = pp.reproject(dense, window=(10, 20, 40, 50), size=(147, 147))
    assert int(win["valid"].sum()) == 40 * 50 and _same_bits(win["depth"][10:50, 20:70], dense["depth_map"][10:50, 20:70])
    with pytest.raises(ValueError, match="pp"):
        pp.reproject(dense, scale=2)
    with pytest.raises(ValueError, match="pp"):
        pp.point_cloud(dense, scale=2)


# ------------------------------------------------------------------------------------------ 8. the workflow flags
def test_workflow_eval_point_cloud_and_reproject_on_a_generated_pair(tmp_path):
    """One datagen_test pair through `workflow eval --point_cloud --reproject CAM.npz` with the shipped checkpoints: one npz of each
    kind whose arrays are DepthPipeline.point_cloud / reproject called directly; no file when the flags are absent."""
    import data
    import models
    import utils
    from be_hip import datagen_test as dt, workflow as wf
    from be_hip.pipeline import DepthPipeline
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 1, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    ckpt = os.path.join(ROOT, "checkpoints")
    args = utils.get_args("eval", argv=["--data_path", str(data_dir), "--model_path", ckpt])
    load = lambda m, name: (m.load_state_dict(torch.load(os.path.join(ckpt, name), map_location=DEV)), m.eval())[1]
    local = load(models.LocalStage().to(DEV), "pretrained_local_stage.pth")
    globl = load(models.GlobalStage(in_parameter_size=38, out_parameter_size=12, device=DEV).to(DEV), "pretrained_global_stage.pth")
    pipe = DepthPipeline(local, globl, utils.PostProcessGlobalBase(args, DEV), utils.DepthEtas(args, DEV), rho_prime=args.rho_prime,
                         stride=args.stride)
    ds = data.TestDataset(DEV, data_path=str(data_dir))
    assert len(ds) == 1
    f = pipe.dcal.focal_px
    R = camera.pose(rs.rot("y", 0.002))[:9].reshape(3, 3)
    np.savez(tmp_path / "cam.npz", K=np.array([[f / 2, 0, 79.5], [0, f / 2, 59.5], [0, 0, 1]]), R=R, t=np.array([-0.01, 0.004, 0.0]),
             size=np.array([120, 160]), scale=2)
    cam = wf.load_camera(str(tmp_path / "cam.npz"))
    assert cam["cam"] == camera.Pinhole(f / 2, f / 2, 59.5, 79.5) and cam["size"] == (120, 160) and cam["scale"] == 2
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    out = tmp_path / "warp"
    res = wf.main(["eval", "--point_cloud", "--reproject", str(tmp_path / "cam.npz"), "--out_path", str(out), *common])
    assert set(res) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
    maps = pipe(ds[0][0].permute(0, 3, 1, 2).contiguous())
    got = dict(np.load(out / "cloud_0000.npz"))
    want = pipe.point_cloud(maps)
    assert set(got) == {"xyz", "valid", "shpd", "conf"}
    assert got["xyz"].shape == (3, 147, 147) and got["xyz"].dtype == np.float32 and got["valid"].dtype == np.bool_
    assert got["valid"].shape == (147, 147) and got["shpd"].shape == (3, 147, 147) and got["conf"].shape == (147, 147)
    for k in got:
        assert np.array_equal(got[k], N(want[k])), k
    assert np.array_equal(got["xyz"][2], N(maps["depth_map"])) and got["valid"].any()
    got = dict(np.load(out / "reproj_0000.npz"))
    want = pipe.reproject(maps, cam_dst=cam["cam"], pose=cam["pose"], size=(120, 160), want=("shpd", "refoc"), scale=2)
    assert set(got) == {"depth", "valid", "index", "shpd", "refoc"}
    assert got["depth"].shape == (120, 160) and got["depth"].dtype == np.float32 and got["index"].dtype == np.int32
    assert got["valid"].dtype == np.bool_ and got["shpd"].shape == (3, 120, 160) and got["refoc"].shape == (3, 120, 160)
    for k in got:
        assert np.array_equal(got[k], N(want[k])) and np.isfinite(got[k]).all(), k
    assert got["valid"].any() and np.array_equal(got["valid"], got["index"] >= 0)
    out = tmp_path / "none"                                             # off by default: no file is written
    wf.main(["eval", "--out_path", str(out), *common])
    assert not out.exists()
    np.savez(tmp_path / "bad.npz", K=np.eye(3))
    with pytest.raises(ValueError, match="size"):
        wf.main(["eval", "--reproject", str(tmp_path / "bad.npz"), "--out_path", str(out), *common])
