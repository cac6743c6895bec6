"""GPU tests of the multi-view depth fusion (be_fuse_views_f32, native.fuse_views, DepthPipeline.fuse, `workflow eval --fuse`).

One bit contract: every output equals the numpy statement of be_hip/fusion.py, which test_fuse_cpu.py ties to the z-buffer of
camera.splat_f32, to a scene worked by hand, to the unquantised float64 mean and to the prototype's quality figures.  Beside it:
tau = 0 with one view is native.reproject, V copies of one view return that view, and neither the order of the views nor a
repeated run changes a bit.  The scenes are those of tests/fuse_scenes.py and tests/reproject_scenes.py; the pipeline fixtures and
scenes are those of test_render_at_gpu.py."""
import itertools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import camera, fusion
import fuse_scenes as fs
import reproject_scenes as rs
from test_render_at_gpu import DEV, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
_F = np.float32
KEYS = ("depth", "valid", "weight", "views", "count", "layer", "feat")


def _on_gpu(views):
    return [dict(v, depth=G(v["depth"]), weight=None if v.get("weight") is None else G(v["weight"]),
                 feat=None if v.get("feat") is None else G(v["feat"])) for v in views]


def _host(out):
    return {k: None if out[k] is None else N(out[k]) for k in KEYS}


def _check_result(out, Ho, Wo, C):
    assert set(out) == set(KEYS)
    for k, dt in (("depth", torch.float32), ("weight", torch.float32), ("views", torch.int32), ("count", torch.int32), ("layer", torch.int32),
                  ("valid", torch.bool)):
        assert out[k].shape == (Ho, Wo) and out[k].dtype == dt and out[k].is_contiguous(), k
    assert torch.equal(out["valid"], out["layer"] >= 0)
    if C:
        assert out["feat"].shape == (C, Ho, Wo) and out["feat"].dtype == torch.float32
    else:
        assert out["feat"] is None


_REFS = {}


def _ref(key, views, dst, size, **kw):
    """fusion.fuse once per case: both bindings share the result."""
    if key not in _REFS:
        _REFS[key] = fusion.fuse(views, dst, size, **kw)
    return _REFS[key]


# ------------------------------------------------------------------------------------------ 1. the host statement, bit for bit
@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("V", [1, 3, 5, 8])
def test_equals_the_host_statement_over_the_parameter_grid(env, binding, V, outliers):
    n = env["native"]
    views = fs.scene(V, outliers=outliers, C=2)
    dev = _on_gpu(views)
    layers = set()
    for recentre, min_views, peel, tau in itertools.product((False, True), (1, 2), (0, 2), (0.0, 0.05)):
        if min_views > V:
            continue
        kw = dict(tau=tau, min_views=min_views, recentre=recentre, peel=peel)
        out = n.fuse_views(dev, fs.CAM, fs.SIZE, **kw)
        _check_result(out, *fs.SIZE, 2)
        ref = _ref(("grid", V, outliers, recentre, min_views, peel, tau), views, fs.CAM, fs.SIZE, **kw)
        assert fs.same(_host(out), ref), kw
        layers |= set(np.unique(ref["layer"]).tolist())
    assert {-1, 0} <= layers and (V < 5 or not outliers or {1, 2} <= layers)


def _variant(pose12, axis, angle, t):
    """pose12 composed with the inverse of a small rigid motion M = (R_m, t_m): the pose of a camera that has moved by M."""
    R, tt = pose12[:9].reshape(3, 3).astype(np.float64), pose12[9:].astype(np.float64)
    Rm = rs.rot(axis, angle)
    Rn = R @ Rm.T
    return camera.pose(Rn, tt - Rn @ np.asarray(t, np.float64))


def _rotated_views(C=5):
    """Three views of the reference scene through rs.SRC, each on another lattice (scale 1; scale 3 with window origin (5, 7);
    scale 2) with its own rotated pose, random weights on the first two."""
    rng = np.random.default_rng(21)
    views = []
    for j, k in enumerate((1, 3, 2)):
        c = rs.lattice_case(k)
        pose = c["pose"] if j == 0 else _variant(c["pose"], "xyz"[j], 0.004 * j, (0.002 * j, -0.003, 0.001 * j))
        w = (0.25 + 0.75 * rng.random(c["depth"].shape)).astype(_F) if j < 2 else None
        views.append(dict(depth=c["depth"], weight=w, feat=c["feat"][:C] if C else None, cam_src=rs.SRC, pose=pose, scale=c["scale"],
                          window_origin=c["origin"]))
    return views


@pytest.mark.parametrize("C", [0, 1, 5])
def test_rotated_views_on_three_lattices(env, binding, C):
    n = env["native"]
    views = _rotated_views(C)
    assert [v["scale"] for v in views] == [1, 3, 2] and views[1]["window_origin"] == (5, 7)
    for kw in (dict(tau=0.05, min_views=1, recentre=True, peel=0), dict(tau=0.02, min_views=2, recentre=False, peel=2)):
        out = n.fuse_views(_on_gpu(views), rs.DST, rs.SIZE, near=rs.NEAR, **kw)
        _check_result(out, *rs.SIZE, C)
        ref = _ref(("rot", C, kw["tau"]), views, rs.DST, rs.SIZE, near=rs.NEAR, **kw)
        assert fs.same(_host(out), ref), kw
        assert ref["valid"].sum() > 1000 and ref["views"].max() == 3 and ref["count"].max() > 3
    if C == 5:
        # feat given as [C,Hs*Ws], cameras as a tuple and a K matrix, poses as 3x4 matrices
        flat = [dict(v, feat=v["feat"].reshape(5, -1), cam_src=rs.SRC.tuple(), pose=np.concatenate([v["pose"][:9].reshape(3, 3), v["pose"][9:, None]], 1))
                for v in views]
        out = n.fuse_views(_on_gpu(flat), rs.DST.K(), rs.SIZE, near=rs.NEAR, tau=0.02, min_views=2, recentre=False, peel=2)
        assert fs.same(_host(out), ref)


@pytest.mark.parametrize("C", [0, 1, 5])
def test_planted_weights_and_depths(env, binding, C):
    """Weights 0, negative, NaN, +inf, above 16 and below the quantum; depths 0, negative, NaN, +-inf and 3e38; NaN, infinite and
    huge channels: a sample that does not take part writes nothing, and every number written is finite."""
    n = env["native"]
    views = [dict(v) for v in fs.scene(3, C=C)]
    w = views[0]["weight"].copy()
    w[5, :8] = [0, -1, np.nan, np.inf, 17, 1000, 2.0 ** -18, -np.inf]
    views[0]["weight"] = w
    d = views[1]["depth"].copy()
    d[7, :7] = [0, -1, np.nan, np.inf, -np.inf, 3e38, -0.0]
    views[1]["depth"] = d
    views[2]["weight"] = None
    if C:
        f = views[2]["feat"].copy()
        f[0, 9, :6] = [np.nan, np.inf, -np.inf, 3000, -1e30, 2047.9999]
        views[2]["feat"] = f
    for kw in (dict(tau=0.05, min_views=1, recentre=True, peel=1), dict(tau=0.05, min_views=2, recentre=False, peel=0)):
        out = n.fuse_views(_on_gpu(views), fs.CAM, fs.SIZE, **kw)
        _check_result(out, *fs.SIZE, C)
        ref = _ref(("planted", C, kw["min_views"]), views, fs.CAM, fs.SIZE, **kw)
        assert fs.same(_host(out), ref), kw
        assert bool(torch.isfinite(out["depth"]).all()) and bool(torch.isfinite(out["weight"]).all())
        assert C == 0 or bool(torch.isfinite(out["feat"]).all())
    # a far pose overflows Zd of the huge depth: it takes no part (reproject's test)
    big = np.zeros((9, 12), _F)
    big[4, 6] = 3e38
    away = camera.pose(None, (0, 0, 3e38))
    out = n.fuse_views(_on_gpu([dict(depth=big, cam_src=rs.HAND_CAM, pose=away)]), rs.HAND_CAM, (9, 12))
    assert not bool(out["valid"].any()) and not bool(out["depth"].view(torch.int32).any())


# ------------------------------------------------------------------------------------------ 2. tau = 0, one view: reproject
@pytest.mark.parametrize("k", [1, 3, 2])
def test_tau_0_with_one_view_is_reproject_bit_for_bit(env, binding, k):
    n, c = env["native"], rs.lattice_case(k)
    d = G(c["depth"])
    warp = n.reproject(d, rs.SRC, rs.DST, c["pose"], rs.SIZE, near=rs.NEAR, scale=c["scale"], window_origin=c["origin"])
    out = n.fuse_views([dict(depth=d, cam_src=rs.SRC, pose=c["pose"], scale=c["scale"], window_origin=c["origin"])], rs.DST, rs.SIZE, tau=0,
                       min_views=1, recentre=False, peel=0, near=rs.NEAR)
    assert int(out["valid"].sum()) == rs.COUNTS[k][1]                    # collisions included
    assert _same_bits(out["depth"], warp["depth"]) and torch.equal(out["valid"], warp["valid"])
    assert int(out["count"].sum()) <= rs.COUNTS[k][0] and bool((out["count"][out["valid"]] >= 1).all())


# ------------------------------------------------------------------------------------------ 3. V copies of one view
@pytest.mark.parametrize("V", [1, 2, 7, 32])
def test_copies_of_one_view_return_that_view(env, binding, V):
    """Under the identity pose Zd = Z: every offset is 0, so without recentring the mean is the input itself, bit for bit, for any
    tau (a recentred pass measures from m - tau, whose offsets are quantised to 2^-20 m: equal to 2^-20 m, not bit for bit - except
    at tau = 0, where it measures from m itself)."""
    n = env["native"]
    v = fs.scene(1, C=2)[0]
    ok = v["depth"] > 0
    wq = fusion.quantise_weight(v["weight"])
    dev = _on_gpu([v]) * V
    for kw in (dict(tau=0.05, recentre=False), dict(tau=0.0, recentre=True)):
        out = n.fuse_views(dev, fs.CAM, fs.SIZE, min_views=V, **kw)
        assert np.array_equal(N(out["valid"]), ok)
        assert np.array_equal(N(out["depth"]).view(np.uint32), np.where(ok, v["depth"], _F(0)).view(np.uint32))
        assert bool((out["views"][out["valid"]] == V).all()) and bool((out["count"][out["valid"]] == V).all())
        assert np.array_equal(N(out["weight"]), np.where(ok, (V * wq).astype(np.float64) / 65536, 0).astype(_F))
        assert np.abs(N(out["feat"]) - v["feat"])[:, ok].max() <= 2.0 ** -16 and not N(out["feat"])[:, ~ok].any()
    near = n.fuse_views(dev, fs.CAM, fs.SIZE, tau=0.05, recentre=True)
    assert np.abs(N(near["depth"]).astype(np.float64) - v["depth"])[ok].max() <= 2.0 ** -20


# ------------------------------------------------------------------------------------------ 4. order independence
def test_view_permutation_and_repeated_runs_are_bit_equal(env, binding):
    n = env["native"]
    views = fs.scene(8, outliers=True, C=2)
    dev = _on_gpu(views)
    kw = dict(tau=0.05, min_views=2, recentre=True, peel=2)
    first = n.fuse_views(dev, fs.CAM, fs.SIZE, **kw)
    assert int((first["layer"] == 1).sum()) > 0 and int(first["count"].max()) >= 8
    for _ in range(2):
        assert fs.same(_host(n.fuse_views(dev, fs.CAM, fs.SIZE, **kw)), _host(first))
    for perm in ([7, 6, 5, 4, 3, 2, 1, 0], [3, 0, 6, 1, 7, 2, 5, 4]):
        assert fs.same(_host(n.fuse_views([dev[i] for i in perm], fs.CAM, fs.SIZE, **kw)), _host(first))


# ------------------------------------------------------------------------------------------ 5. shapes
def test_shapes_one_pixel_nothing_lands_all_invalid_and_more_than_one_block(env, binding):
    n = env["native"]
    # 1 x 1 onto 1 x 1: the pixel on the optical axis
    one = dict(depth=G(np.full((1, 1), 0.9, _F)), weight=G(np.full((1, 1), 0.5, _F)), feat=G(np.full((1, 1, 1), 7, _F)), cam_src=(50, 50, 0, 0))
    out = n.fuse_views([one, one], (50, 50, 0, 0), (1, 1), tau=0.05, recentre=False, min_views=1)
    _check_result(out, 1, 1, 1)
    assert float(out["depth"]) == _F(0.9) and float(out["weight"]) == 1.0 and int(out["views"]) == 2 and int(out["count"]) == 2
    assert int(out["layer"]) == 0 and float(out["feat"]) == 7
    # a target that no sample reaches: every output is the empty value
    views = fs.scene(3, C=2)
    far = n.fuse_views(_on_gpu(views), camera.Pinhole(64, 64, -500, 7000), (6, 7), peel=2)
    _check_result(far, 6, 7, 2)
    for k in ("depth", "weight", "feat"):
        assert not bool(far[k].view(torch.int32).any()), k
    assert not bool(far["valid"].any()) and not bool(far["views"].any()) and not bool(far["count"].any()) and bool((far["layer"] == -1).all())
    # all-invalid depth
    none = n.fuse_views([dict(depth=G(np.zeros(fs.SIZE, _F)), cam_src=fs.CAM), dict(depth=G(np.full(fs.SIZE, np.nan, _F)), cam_src=fs.CAM)],
                        fs.CAM, fs.SIZE, peel=1)
    assert not bool(none["valid"].any()) and not bool(none["depth"].view(torch.int32).any()) and bool((none["layer"] == -1).all())
    # a 147 x 147 pair of views onto 220 x 220: 85 and 190 workgroups, neither count a multiple of 256
    rng = np.random.default_rng(4)
    cam = camera.Pinhole(200, 200, 73, 73)
    big = camera.Pinhole(300, 300, 109.5, 109.5)
    pair = [dict(depth=(0.9 + 0.2 * rng.random((147, 147))).astype(_F), weight=(0.25 + 0.75 * rng.random((147, 147))).astype(_F),
                 feat=rng.standard_normal((1, 147, 147)).astype(_F), cam_src=cam, pose=camera.pose(None, (0.01 * j, 0, 0))) for j in range(2)]
    kw = dict(tau=0.1, min_views=1, recentre=True, peel=1)
    out = n.fuse_views(_on_gpu(pair), big, (220, 220), **kw)
    _check_result(out, 220, 220, 1)
    ref = _ref("big", pair, big, (220, 220), **kw)
    assert fs.same(_host(out), ref) and ref["valid"].sum() > 15000 and (ref["views"] == 2).sum() > 1000


# ------------------------------------------------------------------------------------------ 6. the pipeline
def test_pipeline_fuse(env, pipe, binding):
    from be_hip.pipeline import DepthPipeline
    sc = _scene(env, "g6", None)
    H, W = sc["H"], sc["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"])
    maps = _maps_of(env, sc, p.depth_thres)
    has = (maps["depth_map"] > 0) & torch.isfinite(maps["depth_map"])
    assert int(has.sum()) > 0
    # the same pair twice under the identity pose: depth_map itself, seen by two views
    for kw in (dict(recentre=False), dict(tau=0.0)):
        out = p.fuse([(maps, None), (maps, None)], **kw)
        assert set(out) == {"depth", "valid", "weight", "views", "count", "layer", "shpd"}
        assert out["depth"].shape == (H, W) and out["shpd"].shape == (3, H, W)
        assert torch.equal(out["valid"], has) and _same_bits(out["depth"][has], maps["depth_map"][has]) and not bool(out["depth"][~has].any())
        assert bool((out["views"][has] == 2).all()) and bool((out["count"][has] == 2).all()) and not bool(out["views"][~has].any())
        assert float((out["shpd"][:, has] - maps["shpd"][:, has]).abs().max()) <= 2.0 ** -16
    # a translated second view: native.fuse_views on the samples _depth_samples gives, conf as the weights
    pose = camera.pose(None, (0.0004, -0.0002, 0.001))
    out = p.fuse([(maps, None), (maps, pose)], want=("refoc",), tau=0.02, min_views=1, peel=1)
    src, lat = p._depth_samples("fuse", maps, 1, None, ("refoc", "conf"), None)
    cam = env["dcal"].intrinsics(H, W)
    view = dict(depth=src["depth_map"], weight=src["conf"], feat=src["refoc"], cam_src=cam)
    ref = env["native"].fuse_views([view, dict(view, pose=pose)], cam, (H, W), tau=0.02, min_views=1, peel=1)
    for k in ("depth", "weight"):
        assert _same_bits(out[k], ref[k]), k
    for k in ("valid", "views", "count", "layer"):
        assert torch.equal(out[k], ref[k]), k
    assert _same_bits(out["refoc"], ref["feat"]) and int((out["views"] == 2).sum()) > 0
    host = fusion.fuse([dict(depth=N(src["depth_map"]), weight=N(src["conf"]), feat=N(src["refoc"]), cam_src=cam, pose=q) for q in (None, pose)],
                       cam, (H, W), tau=0.02, min_views=1, peel=1)
    assert fs.same({k: N(ref[k]) for k in KEYS}, host)
    # every map rides along, with reproject's channel counts; another camera and size
    half = camera.Pinhole(cam.fy / 2, cam.fx / 2, (H // 2 - 1) / 2, (W // 2 - 1) / 2)
    full = p.fuse([(maps, None), (maps, pose)], cam_dst=half, size=(H // 2, W // 2), want=("image", "refoc", "conf"), min_views=2)
    assert full["image"].shape == (2, 3, H // 2, W // 2) and full["refoc"].shape == (3, H // 2, W // 2) and full["conf"].shape == (H // 2, W // 2)
    assert full["depth"].shape == (H // 2, W // 2) and bool((full["views"][full["valid"]] == 2).all())
    assert set(p.fuse([(maps, None)], want=())) == {"depth", "valid", "weight", "views", "count", "layer"}
    with pytest.raises(ValueError, match="views"):
        p.fuse([])
    with pytest.raises(ValueError, match="views"):
        p.fuse([maps])
    with pytest.raises(ValueError, match="records"):
        p.fuse([({k: v for k, v in maps.items() if k != "records"}, None)])
    with pytest.raises(ValueError, match="min_views"):
        p.fuse([(maps, None)], min_views=2)


# ------------------------------------------------------------------------------------------ 7. the argument checks
def test_argument_errors_name_the_argument(env, binding):
    n = env["native"]
    views = _on_gpu(fs.scene(3, C=2))
    run = lambda vs=views, **kw: n.fuse_views(vs, fs.CAM, fs.SIZE, **kw)
    with pytest.raises(ValueError, match="views"):
        run([])
    with pytest.raises(ValueError, match="views"):
        run(views * 11)
    for kw, match in ((dict(tau=-0.01), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=4.5), "tau"), (dict(min_views=0), "min_views"),
                      (dict(min_views=4), "min_views"), (dict(peel=-1), "peel"), (dict(peel=9), "peel"), (dict(near=-1.0), "near")):
        with pytest.raises(ValueError, match=match):
            run(**kw)
    with pytest.raises(ValueError, match="feat"):                        # C differs between views
        run([views[0], dict(views[1], feat=views[1]["feat"][:1])])
    with pytest.raises(ValueError, match="feat"):
        run([views[0], dict(views[1], feat=None)])
    with pytest.raises(ValueError, match="GPU"):                         # a CPU tensor
        run([views[0], dict(views[1], depth=views[1]["depth"].cpu())])
    with pytest.raises(ValueError, match="weight"):
        run([dict(views[0], weight=views[0]["weight"].cpu())])
    with pytest.raises(ValueError, match="feat"):                        # a feat of the wrong shape
        run([dict(views[0], feat=views[0]["feat"][:, :, :52])])
    with pytest.raises(ValueError, match="weight"):
        run([dict(views[0], weight=views[0]["weight"][:36])])
    with pytest.raises(ValueError, match="float32"):
        run([dict(views[0], depth=views[0]["depth"].double())])
    with pytest.raises(ValueError, match="size"):
        n.fuse_views(views, fs.CAM, (0, 5))
    with pytest.raises(ValueError, match="cam_dst"):
        n.fuse_views(views, (1, 2, 3), fs.SIZE)
    with pytest.raises(ValueError, match="rotation"):
        run([dict(views[0], pose=np.diag([1, 1, 2, 1.0]))])
    with pytest.raises(ValueError, match="scale"):
        run([dict(views[0], scale=17)])
    with pytest.raises(ValueError, match="unknown keys"):
        run([dict(views[0], wieght=None)])


# ------------------------------------------------------------------------------------------ 8. the workflow flag
def test_workflow_eval_fuse_on_two_generated_pairs(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz` with the shipped checkpoints: one group of two, written as
    fused_0000.npz with the documented keys; no file when the flag is absent."""
    from be_hip import datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    ckpt = os.path.join(ROOT, "checkpoints")
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "fuse.npz", poses=poses, tau=0.03, min_views=1, peel=1, recentre=True)
    cfg = wf.load_fusion(str(tmp_path / "fuse.npz"))
    assert len(cfg["poses"]) == 2 and cfg["cam"] is None and cfg["size"] is None and cfg["scale"] == 1
    assert cfg["kw"] == dict(tau=0.03, min_views=1, peel=1, recentre=True)
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    out = tmp_path / "fused"
    res = wf.main(["eval", "--fuse", str(tmp_path / "fuse.npz"), "--out_path", str(out), *common])
    assert set(res) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
    assert sorted(os.listdir(out)) == ["fused_0000.npz"]
    got = dict(np.load(out / "fused_0000.npz"))
    assert set(got) == {"depth", "valid", "weight", "views", "count", "layer", "shpd"}
    assert got["depth"].shape == (147, 147) and got["depth"].dtype == np.float32 and got["valid"].dtype == np.bool_
    assert got["shpd"].shape == (3, 147, 147) and got["views"].dtype == np.int32 and got["layer"].dtype == np.int32
    assert got["valid"].any() and np.array_equal(got["valid"], got["layer"] >= 0) and got["views"].max() <= 2
    assert np.isfinite(got["depth"]).all() and (got["depth"][got["valid"]] > 0).all() and (got["weight"][got["valid"]] > 0).all()
    np.savez(tmp_path / "bad.npz", K=np.eye(3))
    with pytest.raises(ValueError, match="poses"):
        wf.main(["eval", "--fuse", str(tmp_path / "bad.npz"), "--out_path", str(out), *common])
