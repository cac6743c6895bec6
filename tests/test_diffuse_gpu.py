"""GPU tests of the diffusion depth completion (be_fill_diffuse_f32, native.fill_diffuse, DepthPipeline.complete(method="diffuse"),
`workflow eval --complete --complete_method diffuse`).

The fixed point is the contract: every result lies within 1e-4 m of diffuse.solve_exact, the float64 direct solve, which
test_diffuse_cpu.py ties to the equations.  The kernels are compiled without contraction, so they also equal diffuse.fill_diffuse, the
numpy statement of the same pyramid and sweeps, bit for bit.  The scenes are those of tests/diffuse_scenes.py, the pipeline fixtures
those of test_render_at_gpu.py."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import diffuse, fill, synth
import diffuse_scenes as ds
from test_render_at_gpu import DEV, T, _same_bits, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)

pytestmark = pytest.mark.gpu


def G(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_result(out, H, W):
    assert set(out) == {"depth", "index", "dist2", "residual"}
    assert out["depth"].shape == (H, W) and out["depth"].dtype == torch.float32 and out["depth"].is_contiguous()
    for k in ("index", "dist2"):
        assert out[k].shape == (H, W) and out[k].dtype == torch.int32 and out[k].is_contiguous()
    assert out["residual"].shape == (1,) and out["residual"].dtype == torch.float32 and out["residual"].is_cuda


def _same(a, b):
    return (torch.equal(a["index"], b["index"]) and torch.equal(a["dist2"], b["dist2"]) and _same_bits(a["depth"], b["depth"])
            and _same_bits(a["residual"], b["residual"]))


# ------------------------------------------------------------------------------------------ 1. the direct solve and the statement
@pytest.mark.parametrize("kind", ds.KINDS)
@pytest.mark.parametrize("H,W", ds.SHAPES)
def test_within_the_bound_of_the_direct_solve(env, binding, H, W, kind):
    n = env["native"]
    depth, weight, edge = ds.scene(kind, H, W)
    d, w, e = G(depth), G(weight), G(edge)
    seeds = fill.seeds_of(depth, weight)
    assert seeds.any()
    for r in ds.RADII:
        out = n.fill_diffuse(d, w, e, smooth=r, sigma_z=ds.SIGMA_Z, leak=ds.LEAK)
        _check_result(out, H, W)
        got, res = N(out["depth"]), float(out["residual"])
        ex, ho = ds.exact(kind, H, W, r), ds.host(kind, H, W, r)
        err = np.abs(got.astype(np.float64) - ex["depth"]).max()
        off = np.abs(got - ho["depth"]).max()
        print(f"{kind} {H} x {W} r {r}: {err:.2e} m from the direct solve, {off:.2e} m from the float32 statement, residual {res:.2e}")
        assert err <= ds.TOL, (kind, H, W, r, err)
        near = fill.fill_nearest_f32(depth, weight, r, ds.SIGMA_Z)
        assert np.array_equal(N(out["index"]), near["index"]) and np.array_equal(N(out["dist2"]), near["dist2"])
        assert np.array_equal(_bits(got)[seeds], _bits(depth)[seeds])                                # seeds keep their input bits
        assert np.isfinite(got).all() and (got > 0).all()
        assert np.isfinite(res) and 0 <= res <= 4 * ds.RESIDUAL_CPU[kind], (kind, H, W, r, res)
        # no contraction in the kernels: the numpy statement, bit for bit
        assert np.array_equal(_bits(got), _bits(ho["depth"])) and res == float(ho["residual"]), (kind, H, W, r, off)


def test_defaults_a_weightless_call_and_odd_edge_values(env, binding):
    n = env["native"]
    depth, weight, edge = ds.rooms(24, 31)
    out = n.fill_diffuse(G(depth))                                      # no weight, no edge, smooth=2, sigma_z=0.02, leak=1e-3
    assert np.abs(N(out["depth"]) - diffuse.solve_exact(depth)["depth"]).max() <= ds.TOL
    odd = edge.copy()
    odd[edge == 1] = 7.5                                                # above 1 counts as 1, NaN and negatives as 0
    odd[:, 5] = np.nan
    odd[:, 20] = -3.0
    assert _same(n.fill_diffuse(G(depth), None, G(odd), smooth=0), n.fill_diffuse(G(depth), None, G(edge), smooth=0))
    half = np.where(edge == 1, 0.5, 0).astype(np.float32)               # a fractional edge and another leak
    out = n.fill_diffuse(G(depth), None, G(half), smooth=0, leak=0.25)
    assert np.abs(N(out["depth"]) - diffuse.solve_exact(depth, None, half, 0, leak=0.25)["depth"]).max() <= ds.TOL
    # a non-contiguous view is taken as the image it shows; a bool mask counts as weights 1 / 0
    wide = G(np.concatenate([depth, depth[:, ::-1]], 1))
    mask = depth > 0
    assert _same(n.fill_diffuse(wide[:, :31], G(mask), G(edge)), n.fill_diffuse(G(depth), G(mask.astype(np.float32)), G(edge)))


# ------------------------------------------------------------------------------------------ 2. the ramp and the rooms
@pytest.mark.parametrize("H,W", ds.PLANE_SHAPES)
def test_ramp_and_rooms(env, H, W):
    """The assertions of test_diffuse_cpu.py on the GPU result.  The direct solve is within 1e-6 m of the plane and the GPU result
    within 1e-4 m of the direct solve, so the plane is held to 1e-4 m here; the other bounds are the CPU test's."""
    n = env["native"]
    depth, weight, edge, plane, between = ds.ramp(H, W)
    got = N(n.fill_diffuse(G(depth), None, None, smooth=0)["depth"])
    err = np.abs(got - plane)[between].max()
    near = np.abs(N(n.fill_nearest(G(depth), smooth=0)["depth"]) - plane)[between].max()
    print(f"ramp {H} x {W}: diffuse {err:.2e} m, nearest {100 * near:.1f} cm off the plane")
    assert err <= ds.TOL and near > 0.05
    depth, weight, edge = ds.rooms(H, W)
    left, right = np.s_[:, :W // 2], np.s_[:, W // 2 + 1:]
    got = N(n.fill_diffuse(G(depth), None, G(edge), smooth=0)["depth"])
    assert got[left].max() < ds.NEAR + 0.03 and got[right].min() > ds.FAR - 0.03
    open_ = N(n.fill_diffuse(G(depth), None, None, smooth=0)["depth"])
    print(f"rooms {H} x {W}: left max {got[left].max():.4f} with the edge, {open_[left].max():.4f} without")
    assert open_[left].max() > ds.NEAR + 0.12


# ------------------------------------------------------------------------------------------ 3. repeated calls, iters, the bindings
def test_repeatable_more_sweeps_and_both_bindings(env, monkeypatch):
    n = env["native"]
    for kind, H, W in (("edge", 37, 53), ("rooms", 64, 64), ("sparse", 65, 33), ("dense", 147, 147)):
        depth, weight, edge = ds.scene(kind, H, W)
        d, w, e = G(depth), G(weight), G(edge)
        first = n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z)
        again = n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z)
        assert _same(first, again), kind
        twice = n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z, iters=2 * diffuse.default_sweeps(H, W))
        moved = float((twice["depth"] - first["depth"]).abs().max())
        print(f"{kind} {H} x {W}: iters doubled moves {moved:.2e} m")
        assert moved <= ds.TOL and torch.equal(twice["index"], first["index"])
        single = n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z, iters=24, fuse=False)      # one sweep per launch: the same sweeps where a
        fused = n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z, iters=24)                   # level is one region
        if diffuse.tiles_of(H, W) == (1, 1):
            assert _same(single, fused), kind
        with monkeypatch.context() as m:
            m.setattr(n, "_ops", False)                                 # the ctypes binding
            assert n.ops() is None
            assert _same(n.fill_diffuse(d, w, e, sigma_z=ds.SIGMA_Z), first), kind
        assert n.ops() is not None


def test_argument_checks_no_seed_and_all_seeds(env, binding):
    n = env["native"]
    nothing = ((np.zeros((4, 6), np.float32), None), (np.full((4, 6), np.nan, np.float32), np.ones((4, 6), np.float32)),
               (np.ones((4, 6), np.float32), np.zeros((4, 6), np.float32)), (np.full((37, 53), -np.inf, np.float32), None),
               (np.full((1, 1), np.inf, np.float32), None))
    for d, w in nothing:
        out = n.fill_diffuse(G(d), G(w), G(np.full(d.shape, 0.5, np.float32)))
        _check_result(out, *d.shape)
        assert (_bits(N(out["depth"])) == 0).all() and bool((out["index"] == -1).all()) and bool((out["dist2"] == -1).all())
        assert float(out["residual"]) == 0
    full = np.random.default_rng(3).uniform(0.8, 1.1, (37, 53)).astype(np.float32)
    for r in ds.RADII:
        out = n.fill_diffuse(G(full), smooth=r)
        assert np.array_equal(_bits(N(out["depth"])), _bits(full)) and float(out["residual"]) == 0          # a copy of the input
    g = G(ds.rooms(9, 12)[0])
    for kw, match in ((dict(smooth=9), "smooth"), (dict(smooth=-1), "smooth"), (dict(smooth=1.0), "smooth"), (dict(smooth=True), "smooth"),
                      (dict(sigma_z=0), "sigma_z"), (dict(sigma_z=float("nan")), "sigma_z"), (dict(sigma_z="x"), "sigma_z"),
                      (dict(leak=0), "leak"), (dict(leak=-1e-3), "leak"), (dict(leak=2), "leak"), (dict(leak=float("nan")), "leak"),
                      (dict(leak="x"), "leak"), (dict(iters=0), "iters"), (dict(iters=4097), "iters"), (dict(iters=2.0), "iters"),
                      (dict(iters=True), "iters"),
                      (dict(weight=G(np.ones((9, 11), np.float32))), "weight"), (dict(weight=torch.ones(9, 12)), "weight"),
                      (dict(edge=G(np.ones((9, 11), np.float32))), "edge"), (dict(edge=np.ones((9, 12), np.float32)), "edge"),
                      (dict(edge=torch.ones(9, 12)), "edge"), (dict(edge=torch.ones(9, 12, device=DEV).double()), "edge"),
                      (dict(edge=torch.ones(9, 12, device=DEV) > 0), "edge")):
        with pytest.raises(ValueError, match=match):
            n.fill_diffuse(g, **kw)
    with pytest.raises(ValueError, match="GPU"):
        n.fill_diffuse(g.cpu())
    for bad in (g.double(), g[0], g[None]):
        with pytest.raises(ValueError, match="float32"):
            n.fill_diffuse(bad)


# ------------------------------------------------------------------------------------------ 4. a level of several tiles
def test_edge_scene_at_147(env, binding):
    """147 x 147 is 2 x 2 tiles of 96 with their halos on the finest level, and one region from the next level down."""
    n = env["native"]
    depth, weight, edge = ds.scene("edge", 147, 147)
    out = n.fill_diffuse(G(depth), G(weight), G(edge), sigma_z=ds.SIGMA_Z)
    ex, ho = ds.exact("edge", 147, 147, 2), ds.host("edge", 147, 147, 2)
    err = np.abs(N(out["depth"]).astype(np.float64) - ex["depth"]).max()
    print(f"edge 147 x 147: {err:.2e} m from the direct solve, residual {float(out['residual']):.2e}")
    assert err <= ds.TOL
    assert np.array_equal(_bits(N(out["depth"])), _bits(ho["depth"])) and float(out["residual"]) == float(ho["residual"])


# ------------------------------------------------------------------------------------------ 5. the pipeline
def test_pipeline_complete_diffuse(env, pipe):
    n = env["native"]
    H = W = 147
    img = T(synth.synthetic_image_pair(H, W, nshape=8)[0]).to(DEV)
    maps = pipe(img)
    keys = set(maps)
    out = pipe.complete(maps, method="diffuse")
    near = pipe.complete(maps, method="nearest")
    assert set(out) == {"depth_dense", "measured", "index", "dist", "residual"} and set(maps) == keys
    assert out["depth_dense"].shape == (H, W) and out["depth_dense"].dtype == torch.float32
    assert out["measured"].dtype == torch.bool and out["index"].dtype == torch.int32 and out["dist"].dtype == torch.float32
    assert out["residual"].shape == (1,) and out["residual"].dtype == torch.float32
    for k in ("measured", "index", "dist"):
        assert torch.equal(out[k], near[k]), k
    m = out["measured"]
    assert 0 < int(m.sum()) < H * W
    assert _same_bits(out["depth_dense"][m], maps["depth_map"][m])
    assert bool((out["depth_dense"] > 0).all()) and bool(torch.isfinite(out["depth_dense"]).all())
    bndry = maps["bndry"].reshape(H, W)
    raw = n.fill_diffuse(maps["depth_map"], maps["conf"], bndry)
    assert _same_bits(out["depth_dense"], raw["depth"]) and _same_bits(out["residual"], raw["residual"])
    ex = diffuse.solve_exact(N(maps["depth_map"]), N(maps["conf"]), N(bndry))
    err = np.abs(N(out["depth_dense"]).astype(np.float64) - ex["depth"]).max()
    moved = float((out["depth_dense"] - near["depth_dense"]).abs().max())
    print(f"pipeline 147 x 147: {err:.2e} m from the direct solve, residual {float(out['residual']):.2e}, {moved:.3f} m from nearest")
    # without the edge map, and a bndry with leading dimensions
    flat = pipe.complete(maps, method="diffuse", edges=False)
    assert _same_bits(flat["depth_dense"], n.fill_diffuse(maps["depth_map"], maps["conf"])["depth"])
    lead = pipe.complete(dict(maps, bndry=bndry[None, None]), method="diffuse", smooth=0, leak=0.01, iters=32)
    assert _same_bits(lead["depth_dense"], n.fill_diffuse(maps["depth_map"], maps["conf"], bndry, smooth=0, leak=0.01, iters=32)["depth"])
    # method="nearest" is the call without a method, bit for bit
    plain = pipe.complete(maps)
    assert set(plain) == {"depth_dense", "measured", "index", "dist"} == set(near)
    for k in plain:
        assert _same_bits(plain[k].float(), near[k].float()) and plain[k].dtype == near[k].dtype, k
    with pytest.raises(ValueError, match="method"):
        pipe.complete(maps, method="linear")
    with pytest.raises(ValueError, match="bndry"):
        pipe.complete({k: v for k, v in maps.items() if k != "bndry"}, method="diffuse")
    with pytest.raises(ValueError, match="GPU"):
        pipe.complete(dict(maps, bndry=maps["bndry"].cpu()), method="diffuse")
    with pytest.raises(ValueError, match="bndry"):
        pipe.complete(dict(maps, bndry=bndry[:-1]), method="diffuse")
    assert set(pipe.complete({k: v for k, v in maps.items() if k != "bndry"}, method="diffuse", edges=False)) == set(out)
    with pytest.raises(ValueError, match="leak"):
        pipe.complete(maps, method="diffuse", leak=0)
    with pytest.raises(ValueError, match="iters"):
        pipe.complete(maps, method="diffuse", iters=0)
    # under densify 'w' depth_map is dense already and comes back unchanged
    from be_hip.pipeline import DepthPipeline
    p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify="w", densify_pp_module=torch.nn.Identity())
    same = p.complete(maps, method="diffuse")
    assert same["depth_dense"] is maps["depth_map"] and bool(same["measured"].all()) and not bool(same["dist"].any())
    assert same["residual"].shape == (1,) and float(same["residual"]) == 0
    assert set(p.complete(maps)) == {"depth_dense", "measured", "index", "dist"}


# ------------------------------------------------------------------------------------------ 6. the workflow option
def test_workflow_eval_complete_method_diffuse(tmp_path, capsys):
    """One datagen_test pair through `workflow eval --complete --complete_method diffuse` with the shipped checkpoints: an npz whose
    arrays are DepthPipeline.complete(method="diffuse") called directly, residual among them, and the extra metrics lines."""
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
    p = DepthPipeline(local, globl, utils.PostProcessGlobalBase(args, DEV), utils.DepthEtas(args, DEV), rho_prime=args.rho_prime,
                      stride=args.stride)
    ds_ = data.TestDataset(DEV, data_path=str(data_dir))
    out = tmp_path / "dense"
    capsys.readouterr()
    res = wf.main(["eval", "--complete", "--complete_method", "diffuse", "--out_path", str(out), "--model_path", ckpt, "--data_path",
                   str(data_dir), "--cuda", DEV])
    text = capsys.readouterr().out
    assert set(res["dense"]) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel"}
    assert "Image pair #0 (completed, diffuse): delta1 =" in text
    assert "Average metrics for whole dataset (completed, diffuse): delta1 =" in text
    img, gt = ds_[0]
    maps = p(img.permute(0, 3, 1, 2).contiguous())
    want = p.complete(maps, method="diffuse")
    got = dict(np.load(out / "complete_0000.npz"))
    assert set(got) == {"depth_dense", "measured", "index", "dist", "residual"}
    assert got["residual"].shape == (1,) and got["residual"].dtype == np.float32 and np.isfinite(got["residual"]).all()
    for k in got:
        assert np.array_equal(got[k], N(want[k])) and np.isfinite(got[k]).all(), k
    assert got["measured"].any() and not got["measured"].all() and (got["depth_dense"] > 0).all()
    dense = want["depth_dense"][None]
    m = utils.eval_depth(dense, gt[None].to(dense.dtype), dense, crop=args.crop)
    print("dense (diffuse):", {k: round(v, 4) for k, v in res["dense"].items()}, "residual", got["residual"])
    assert list(res["dense"].values()) == [float(v) for v in m]
