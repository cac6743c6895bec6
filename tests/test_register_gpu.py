"""GPU tests of the depth registration (be_depth_normals_f32, be_icp_linearize_f32, native.depth_normals / icp_linearize /
register_depth, DepthPipeline.normals / register, `workflow eval --fuse` with `register`).

One bit contract: normals, rows and the double sums equal the numpy statement of be_hip/registration.py, which
test_register_cpu.py ties to hand-worked normals, to the float64 evaluation and to the true poses of tests/register_scenes.py.
Since the sums are bit-equal and the loop around them is shared host code, every iterate of native.register_depth equals
registration.register's.  The pipeline fixtures and scenes are those of test_render_at_gpu.py; every case runs through both
bindings."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import camera, registration as rg
import register_scenes as sc
from test_register_cpu import normal_cases, sums_bound
from test_render_at_gpu import DEV, _same_bits, _scene, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)
from test_reproject_gpu import G, N, _maps_of

pytestmark = pytest.mark.gpu
_F = np.float32


def _dev(view):
    return dict(view, depth=G(view["depth"]), weight=None if view.get("weight") is None else G(view["weight"]))


_REFS = {}


def _ref(key, fn):
    """A host statement once per case: both bindings share the result."""
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


# ------------------------------------------------------------------------------------------ 1. normals, bit for bit
@functools.lru_cache(None)
def _normal_inputs():
    cases = {k: (d, cam, dict(kw)) for k, (d, cam, kw) in normal_cases().items()}
    noisy = sc.scene("small", noisy=True)
    for step in (1, 3, 8):
        cases[f"dropout_a{step}"] = (noisy["dst"]["depth"], sc.CAM, dict(step=step))
        cases[f"dropout_b{step}"] = (noisy["src"]["depth"], sc.CAM, dict(step=step, max_jump=0.02))
    fine = sc.scene("small", scale=3)["src"]
    assert fine["depth"].shape == (109, 157)
    cases["scale3"] = (fine["depth"], sc.CAM, dict(step=3, scale=3))
    cases["scale3_origin"] = (fine["depth"][:40, :50], sc.CAM, dict(step=2, scale=3, window_origin=(4, 9)))
    rng = np.random.default_rng(8)
    big = (0.9 + 0.2 * rng.random((147, 147))).astype(_F)
    big[rng.random((147, 147)) < 0.2] = 0
    cases["holes147"] = (big, camera.Pinhole(200, 200, 73, 73), dict(step=1, max_jump=0.1))
    return cases


@pytest.mark.parametrize("name", sorted(_normal_inputs()))
def test_depth_normals_equal_the_host_statement(env, binding, name):
    d, cam, kw = _normal_inputs()[name]
    ref = _ref(("n", name), lambda: rg.normals_f32(d, cam, **kw))
    out = env["native"].depth_normals(G(d), cam, **kw)
    assert set(out) == {"normal", "valid"} and out["normal"].shape == (3,) + d.shape and out["normal"].dtype == torch.float32
    assert out["valid"].dtype == torch.bool and out["valid"].shape == d.shape
    assert np.array_equal(sc.bits(N(out["normal"])), sc.bits(ref))
    assert np.array_equal(N(out["valid"]), (ref != 0).any(0))
    if name in ("holes147", "scale3", "dropout_a3"):
        v = (ref != 0).any(0)
        assert 0.2 < v.mean() <= 1 and np.abs(np.sqrt((ref.astype(np.float64) ** 2).sum(0))[v] - 1).max() < 1e-6


# ------------------------------------------------------------------------------------------ 2, 3. rows and sums, bit for bit
def _target(weighted):
    dst = dict(sc.scene("small")["dst"])
    if weighted:
        dst["weight"] = sc.weights(sc.SIZE, 2)
    return dst


@functools.lru_cache(None)
def _linearize_inputs():
    """name -> (src, dst, pose, keywords): the statement's inputs; dst without its normals."""
    pose = camera.pose(*sc.true_pose("small"))
    near = camera.pose(*sc.true_pose("small")[:1], sc.true_pose("small")[1] + [0.004, -0.003, 0.002])       # 5 mm off the truth
    cases = {}
    for n in (1, 63, 64, 65, 255, 256, 257):
        cases[f"row{n}"] = (sc.other_source((1, n)), _target(False), near, dict())
    s = sc.scene("small")
    for ws in (False, True):
        for wd in (False, True):
            src = dict(s["src"], weight=sc.weights(sc.SIZE, 1) if ws else None)
            for huber in (0.0, 0.002):
                cases[f"scene_w{int(ws)}{int(wd)}_h{huber}"] = (src, _target(wd), near, dict(huber=huber))
    cases["scene_maxdist0"] = (s["src"], _target(True), near, dict(max_dist=0.0))
    ident = sc.scene("identity")
    cases["identity_maxdist0"] = (ident["src"], ident["dst"], None, dict(max_dist=0.0))
    cases["scale3"] = (sc.scene("small", scale=3)["src"], _target(True), pose, dict(huber=0.002))
    big = dict(sc.other_source((147, 147)), weight=sc.weights((147, 147), 4))
    cases["src147"] = (big, _target(True), near, dict())
    cases["src147_huber"] = (big, _target(False), near, dict(huber=0.002, max_dist=0.05))
    # planted values on both sides
    src = dict(s["src"], depth=s["src"]["depth"].copy(), weight=sc.weights(sc.SIZE, 1))
    src["depth"][3, :6] = [0, -1, np.nan, np.inf, -np.inf, 3e38]
    src["weight"][9, :7] = [0, -1, np.nan, np.inf, -np.inf, 3e38, 1e-30]
    dst = _target(True)
    dst["depth"] = dst["depth"].copy()
    dst["depth"][20, 10:16] = [0, -1, np.nan, np.inf, -np.inf, 3e38]
    dst["weight"][25, 10:17] = [0, -1, np.nan, np.inf, -np.inf, 3e38, 1e-30]
    cases["planted"] = (src, dst, near, dict(huber=0.002))
    cases["out_of_frame"] = (s["src"], _target(True), camera.pose(None, (5.0, 0, 0)), dict())
    cases["behind"] = (s["src"], _target(False), camera.pose(None, (0, 0, -3.0)), dict())
    return cases


def _statement(name):
    def run():
        src, dst, pose, kw = _linearize_inputs()[name]
        nrm = rg.normals_f32(dst["depth"], dst["cam"])
        return dict(rg.linearize(src, dict(dst, normal=nrm), pose, want_rows=True, **kw), normal=nrm)
    return _ref(("l", name), run)


@pytest.mark.parametrize("name", sorted(_linearize_inputs()))
def test_icp_linearize_equals_the_host_statement(env, binding, name):
    n = env["native"]
    src, dst, pose, kw = _linearize_inputs()[name]
    ref = _statement(name)
    out = n.icp_linearize(_dev(src), _dev(dst), G(ref["normal"]), pose, rows=True, **kw)
    Ns = src["depth"].size
    assert out["sums"].dtype == torch.float64 and out["sums"].shape == (32,) and out["sums"].is_cuda
    assert out["rows"].dtype == torch.float32 and out["rows"].shape == (8, Ns)
    assert np.array_equal(sc.bits(N(out["rows"])), sc.bits(ref["rows"]))
    got = N(out["sums"])
    assert np.array_equal(sc.bits(got), sc.bits(ref["sums"])), (got, ref["sums"])
    plain, bound = sums_bound(ref["rows"], ref["ok"])
    assert (np.abs(got[:30] - plain) <= bound).all() and got[29] == ref["ok"].sum()
    assert n.icp_linearize(_dev(src), _dev(dst), G(ref["normal"]), pose, **kw)["rows"] is None
    count = int(ref["ok"].sum())
    if name in ("out_of_frame", "behind", "scene_maxdist0"):
        assert count == 0 and not sc.bits(got).any()                     # every sum +0.0
    elif name == "identity_maxdist0":
        assert count == 37 * 53 and got[27] == 0 and got[28] == count    # exact hits: D = 0
    elif name.startswith("row"):
        assert count >= 0.6 * Ns
    elif name.startswith("src147"):
        assert Ns == 21609 > 64 * 256 and count > 15000                  # two passes of the grid, 64 partials
    elif name == "planted":
        assert np.isfinite(got).all() and 1000 < count < 1808
    else:
        assert count > 1000
    if "h0.002" in name or name == "planted":
        assert (np.abs(ref["rows"][6]) > 0.002).any()                    # huber acted


# ------------------------------------------------------------------------------------------ 4. the loop, bit for bit
@functools.lru_cache(None)
def _register_inputs():
    return dict(small=(sc.scene("small"), dict()), noisy=(sc.scene("small", noisy=True), dict()), plane=(sc.scene("small", plane=True), dict()),
                weighted=(dict(src=dict(sc.scene("small")["src"], weight=sc.weights(sc.SIZE, 1)), dst=_target(True)),
                          dict(iters=5, step=2, huber=0.01, max_dist=0.2, damping=1e-4)))


@pytest.mark.parametrize("name", sorted(_register_inputs()))
def test_register_depth_equals_the_host_loop_iterate_by_iterate(env, binding, name):
    s, kw = _register_inputs()[name]
    ref = _ref(("r", name), lambda: rg.register(s["src"], s["dst"], **kw))
    out = env["native"].register_depth(_dev(s["src"]), _dev(s["dst"]), **kw)
    assert set(out) == set(ref) == {"pose", "poses", "rms", "count", "A", "cond", "cov", "converged", "iters"}
    assert out["poses"].shape == ref["poses"].shape and len(ref["poses"]) >= 2
    for k in ("pose", "poses", "rms", "A"):
        assert np.array_equal(sc.bits(out[k]), sc.bits(ref[k])), k
    assert np.array_equal(out["count"], ref["count"]) and out["iters"] == ref["iters"] and out["converged"] == ref["converged"]
    assert out["cond"] == ref["cond"] and np.array_equal(out["cov"], ref["cov"])
    if name == "small":
        gap = rg.pose_gap(out["pose"], s["R"], s["t"])
        assert out["converged"] and gap[0] < 0.05 and gap[1] < 5e-4


# ------------------------------------------------------------------------------------------ 5. repeated runs, a side stream
def test_repeated_runs_and_a_side_stream_change_no_bit(env, binding):
    n = env["native"]
    src, dst, pose, kw = _linearize_inputs()["src147"]
    ref = _statement("src147")
    s, d, nrm = _dev(src), _dev(dst), G(ref["normal"])
    first = n.icp_linearize(s, d, nrm, pose, rows=True, **kw)
    nfirst = n.depth_normals(d["depth"], d["cam"])
    for _ in range(2):
        again = n.icp_linearize(s, d, nrm, pose, rows=True, **kw)
        assert torch.equal(again["sums"].view(torch.int64), first["sums"].view(torch.int64)) and _same_bits(again["rows"], first["rows"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again = n.icp_linearize(s, d, nrm, pose, rows=True, **kw)
        nagain = n.depth_normals(d["depth"], d["cam"])
    side.synchronize()
    assert torch.equal(again["sums"].view(torch.int64), first["sums"].view(torch.int64)) and _same_bits(again["rows"], first["rows"])
    assert _same_bits(nagain["normal"], nfirst["normal"]) and np.array_equal(sc.bits(N(nfirst["normal"])), sc.bits(ref["normal"]))


# ------------------------------------------------------------------------------------------ 6. the pipeline
def test_pipeline_normals_and_register(env, pipe, binding):
    from be_hip.pipeline import DepthPipeline
    n = env["native"]
    scn = _scene(env, "g6", None)
    H, W = scn["H"], scn["W"]
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"])
    maps = _maps_of(env, scn, p.depth_thres)
    cam = env["dcal"].intrinsics(H, W)
    # normals of depth_map (the default) and of the completed depth
    out = p.normals(maps)
    assert set(out) == {"normal", "valid", "lattice"} and out["normal"].shape == (3, H, W) and out["lattice"]["scale"] == 1
    by_hand = n.depth_normals(maps["depth_map"], cam)
    assert _same_bits(out["normal"], by_hand["normal"]) and torch.equal(out["valid"], by_hand["valid"])
    done = p.complete(maps)
    dense = p.normals(maps, step=2, source="complete")
    by_hand = n.depth_normals(done["depth_dense"], cam, step=2)
    assert _same_bits(dense["normal"], by_hand["normal"]) and int(dense["valid"].sum()) > int(out["valid"].sum())
    assert np.array_equal(sc.bits(N(dense["normal"])), sc.bits(rg.normals_f32(N(done["depth_dense"]), cam, step=2)))
    fine = p.normals(maps, scale=2, window=(10, 20, 30, 40))
    assert fine["normal"].shape[0] == 3 and fine["lattice"]["scale"] == 2 and fine["normal"].shape[1:] == fine["valid"].shape
    with pytest.raises(ValueError, match="normals"):
        p.normals(maps, source="complete", scale=2)
    with pytest.raises(ValueError, match="source"):
        p.normals(maps, source="dense")
    with pytest.raises(ValueError, match="step"):
        p.normals(maps, step=9)
    # the pair against itself: the identity exactly
    res = p.register(maps, maps)
    assert np.array_equal(res["pose"], camera.pose()) and (res["poses"] == camera.pose()).all()
    assert res["rms"][0] == 0 and res["count"][0] > 0 and res["cond"] > 1
    w = torch.where(done["measured"], maps["conf"].reshape(H, W).to(torch.float32), torch.ones(H, W, device=DEV))
    view = dict(depth=done["depth_dense"], weight=w, cam=cam)
    hand = n.register_depth(view, view)
    for k in ("poses", "rms", "A"):
        assert np.array_equal(sc.bits(res[k]), sc.bits(hand[k])), k
    assert np.array_equal(res["count"], hand["count"]) and res["cond"] == hand["cond"]
    a = p.fuse([(maps, None), (maps, res["pose"])])
    b = p.fuse([(maps, None), (maps, None)])
    for k in a:
        assert torch.equal(a[k], b[k]) if a[k].dtype != torch.float32 else _same_bits(a[k], b[k]), k
    # from a start off the identity, without weights and on depth_map itself
    off = p.register(maps, maps, pose0=camera.pose(None, (0, 0, 0.002)), weights=None, source="depth_map", iters=3)
    assert len(off["rms"]) >= 1 and off["poses"].shape[1] == 12
    with pytest.raises(ValueError, match="weights"):
        p.register(maps, maps, weights="depth")
    with pytest.raises(ValueError, match="source"):
        p.register(maps, maps, source="dense")
    with pytest.raises(ValueError, match="iters"):
        p.register(maps, maps, iters=-1)


# ------------------------------------------------------------------------------------------ 7. the argument checks
def test_argument_errors_name_the_caller(env, binding):
    n = env["native"]
    s = sc.scene("small")
    src, dst = _dev(s["src"]), _dev(s["dst"])
    nrm = n.depth_normals(dst["depth"], dst["cam"])["normal"]
    for kw, match in ((dict(step=0), "step"), (dict(step=9), "step"), (dict(max_jump=-1.0), "max_jump"), (dict(max_jump=float("nan")), "max_jump"),
                      (dict(scale=17), "scale"), (dict(window_origin=(-1, 0)), "window_origin")):
        with pytest.raises(ValueError, match=f"depth_normals.*{match}"):
            n.depth_normals(dst["depth"], sc.CAM, **kw)
    with pytest.raises(ValueError, match="GPU"):
        n.depth_normals(dst["depth"].cpu(), sc.CAM)
    with pytest.raises(ValueError, match="float32"):
        n.depth_normals(dst["depth"].double(), sc.CAM)
    with pytest.raises(ValueError, match=r"depth_normals\(cam\)"):
        n.depth_normals(dst["depth"], (1, 2, 3))
    for kw, match in ((dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("inf")), "max_dist"), (dict(huber=-1.0), "huber"),
                      (dict(huber=float("nan")), "huber"), (dict(near=-1.0), "near")):
        with pytest.raises(ValueError, match=f"icp_linearize: {match}"):
            n.icp_linearize(src, dst, nrm, None, **kw)
    with pytest.raises(ValueError, match="normal_d"):
        n.icp_linearize(src, dst, nrm[:, :36], None)
    with pytest.raises(ValueError, match="normal_d"):
        n.icp_linearize(src, dst, nrm.cpu(), None)
    with pytest.raises(ValueError, match=r"icp_linearize\(dst\).*scale"):
        n.icp_linearize(src, dict(dst, scale=2), nrm, None)
    with pytest.raises(ValueError, match=r"icp_linearize\(src\).*weight"):
        n.icp_linearize(dict(src, weight=src["depth"][:5]), dst, nrm, None)
    with pytest.raises(ValueError, match=r"icp_linearize\(dst\).*weight"):
        n.icp_linearize(src, dict(dst, weight=dst["depth"].cpu()), nrm, None)
    with pytest.raises(ValueError, match="GPU"):
        n.icp_linearize(dict(src, depth=src["depth"].cpu()), dst, nrm, None)
    with pytest.raises(ValueError, match="unknown keys"):
        n.icp_linearize(dict(src, wieght=None), dst, nrm, None)
    with pytest.raises(ValueError, match="rotation"):
        n.icp_linearize(src, dst, nrm, np.diag([1, 1, 2, 1.0]))
    with pytest.raises(ValueError, match="register_depth: step"):
        n.register_depth(src, dst, step=0)
    with pytest.raises(ValueError, match="register_depth: unknown keywords"):
        n.register_depth(src, dst, tau=0.1)
    with pytest.raises(ValueError, match=r"register_depth\(dst\)"):
        n.register_depth(src, dict(depth=dst["depth"]))


# ------------------------------------------------------------------------------------------ 8. the workflow
def test_workflow_eval_fuse_with_register_and_normals(tmp_path):
    """Two datagen_test pairs through `workflow eval --fuse FILE.npz --normals`: with `register: 3` in the settings file the npz
    also holds poses_refined and register_rms; without the key it holds exactly what it held before."""
    from be_hip import datagen_test as dt, workflow as wf
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    ckpt = os.path.join(ROOT, "checkpoints")
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "plain.npz", poses=poses, tau=0.03)
    np.savez(tmp_path / "reg.npz", poses=poses, tau=0.03, register=3)
    assert "register" not in wf.load_fusion(str(tmp_path / "plain.npz")) and wf.load_fusion(str(tmp_path / "reg.npz"))["register"] == 3
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    today = {"depth", "valid", "weight", "views", "count", "layer", "shpd"}
    wf.main(["eval", "--fuse", str(tmp_path / "plain.npz"), "--out_path", str(tmp_path / "a"), *common])
    assert sorted(os.listdir(tmp_path / "a")) == ["fused_0000.npz"]
    assert set(np.load(tmp_path / "a" / "fused_0000.npz").files) == today
    wf.main(["eval", "--fuse", str(tmp_path / "reg.npz"), "--normals", "--out_path", str(tmp_path / "b"), *common])
    assert sorted(os.listdir(tmp_path / "b")) == ["fused_0000.npz", "normals_0000.npz", "normals_0001.npz"]
    got = dict(np.load(tmp_path / "b" / "fused_0000.npz"))
    assert set(got) == today | {"poses_refined", "register_rms"}
    assert got["poses_refined"].shape == (2, 12) and got["poses_refined"].dtype == np.float32 and got["register_rms"].shape == (2,)
    assert np.array_equal(got["poses_refined"][0], poses[0]) and got["register_rms"][0] == 0 and np.isfinite(got["poses_refined"]).all()
    camera.as_pose(got["poses_refined"][1])                              # still a rigid pose
    nrm = dict(np.load(tmp_path / "b" / "normals_0000.npz"))
    assert set(nrm) == {"normal", "valid"} and nrm["normal"].shape == (3, 147, 147) and nrm["valid"].dtype == np.bool_ and nrm["valid"].any()
    np.savez(tmp_path / "bad.npz", poses=poses, register=-2)
    with pytest.raises(ValueError, match="register"):
        wf.load_fusion(str(tmp_path / "bad.npz"))
