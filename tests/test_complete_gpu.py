"""GPU tests of the nearest-sample flood fill (be_fill_nearest_f32, native.fill_nearest, DepthPipeline.complete,
`workflow eval --complete`).

One bit contract: depth, index and dist2 equal the numpy statement of be_hip/fill.py, which test_complete_cpu.py ties to the
brute-force nearest search, to a window worked by hand and to the same formula in float64 - with the fused tail and without it,
through both bindings.  The scenes are those of tests/complete_scenes.py, the pipeline fixtures those of test_render_at_gpu.py."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import fill, synth
import complete_scenes as cs
from test_render_at_gpu import DEV, T, _same_bits, binding, env, pipe  # noqa: F401  (env, pipe, binding: fixtures)

pytestmark = pytest.mark.gpu


def G(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_result(out, H, W):
    assert set(out) == {"depth", "index", "dist2"}
    assert out["depth"].shape == (H, W) and out["depth"].dtype == torch.float32 and out["depth"].is_contiguous()
    for k in ("index", "dist2"):
        assert out[k].shape == (H, W) and out[k].dtype == torch.int32 and out[k].is_contiguous()


def _equals_host(out, ref, what=None):
    """Every output of native.fill_nearest against fill.fill_nearest_f32's, bit for bit."""
    assert np.array_equal(N(out["index"]), ref["index"]), what
    assert np.array_equal(N(out["dist2"]), ref["dist2"]), what
    assert np.array_equal(_bits(N(out["depth"])), _bits(ref["depth"])), what


def _same(a, b):
    return torch.equal(a["index"], b["index"]) and torch.equal(a["dist2"], b["dist2"]) and _same_bits(a["depth"], b["depth"])


# ------------------------------------------------------------------------------------------ 1. the host statement
@pytest.mark.parametrize("kind", cs.KINDS)
@pytest.mark.parametrize("H,W", cs.SHAPES)
def test_equals_the_host_statement_bit_for_bit(env, binding, H, W, kind):
    n = env["native"]
    depth, weight = cs.scene(kind, H, W)
    d, w = G(depth), G(weight)
    seeds = fill.seeds_of(depth, weight)
    assert seeds.any()
    if kind in ("sparse", "dense", "edge") and min(H, W) > 8:
        assert seeds[0].any() or seeds[-1].any() or seeds[:, 0].any() or seeds[:, -1].any()         # windows clipped at a border
    for r in cs.RADII:
        ref = cs.host(kind, H, W, r)
        out = n.fill_nearest(d, w, smooth=r, sigma_z=cs.SIGMA_Z)
        _check_result(out, H, W)
        _equals_host(out, ref, (kind, H, W, r))
        assert np.array_equal(_bits(N(out["depth"]))[seeds], _bits(depth)[seeds])                   # seeds keep their depth
        assert bool((out["index"] >= 0).all()) and bool(torch.isfinite(out["depth"]).all()) and bool((out["depth"] > 0).all())
        if r == 0:
            assert np.array_equal(_bits(N(out["depth"])), _bits(depth.ravel()[ref["index"]]))       # the seed's depth exactly


def test_defaults_and_a_weightless_call(env, binding):
    n = env["native"]
    depth, weight = cs.scene("edge", 37, 53)
    out = n.fill_nearest(G(depth), G(weight))                           # smooth=2, sigma_z=0.02, fuse=True
    _equals_host(out, fill.fill_nearest_f32(depth, weight, 2, 0.02))
    out = n.fill_nearest(G(depth))
    _equals_host(out, fill.fill_nearest_f32(depth, None, 2, 0.02))
    out = n.fill_nearest(G(depth), G(weight), smooth=3, sigma_z=0.5)
    _equals_host(out, fill.fill_nearest_f32(depth, weight, 3, 0.5))
    # a non-contiguous view is taken as the image it shows
    wide = G(np.concatenate([depth, depth[:, ::-1]], 1))
    _equals_host(n.fill_nearest(wide[:, :53], G(weight)), fill.fill_nearest_f32(depth, weight, 2, 0.02))


# ------------------------------------------------------------------------------------------ 2. the fused tail
@pytest.mark.parametrize("H,W", cs.SHAPES + ((1, 2), (2, 2), (9, 4), (33, 95)))
def test_fused_and_unfused_give_identical_tensors(env, binding, H, W):
    """37 x 53: partial 32 x 32 tiles; 5 x 3, 1 x 7, 1 x 1: an image smaller than the halo; (1, 2), (2, 2), (9, 4): a tail that starts
    at step 1, 1 and 8 with a halo of 1, 1 and 15; 33 x 95: one row and one column of tiles that hold a single pixel row."""
    n = env["native"]
    for kind in cs.KINDS:
        depth, weight = cs.scene(kind, H, W)
        d, w = G(depth), G(weight)
        for r in cs.RADII:
            fused = n.fill_nearest(d, w, smooth=r, sigma_z=cs.SIGMA_Z, fuse=True)
            plain = n.fill_nearest(d, w, smooth=r, sigma_z=cs.SIGMA_Z, fuse=False)
            assert _same(fused, plain), (kind, H, W, r)
            _equals_host(plain, cs.host(kind, H, W, r), (kind, H, W, r))


# ------------------------------------------------------------------------------------------ 3. repeated calls
def test_two_calls_give_identical_results(env, binding):
    n = env["native"]
    for kind, H, W in (("dense", 147, 147), ("edge", 37, 53), ("sparse", 65, 33)):
        depth, weight = cs.scene(kind, H, W)
        d, w = G(depth), G(weight)
        for fuse in (True, False):
            first = n.fill_nearest(d, w, smooth=2, fuse=fuse)
            again = n.fill_nearest(d, w, smooth=2, fuse=fuse)
            assert _same(first, again), (kind, fuse)


# ------------------------------------------------------------------------------------------ 4. every element is written
@pytest.mark.parametrize("fuse", [1, 0])
def test_buffers_filled_with_garbage_are_fully_overwritten(env, fuse):
    """The C entry on caller-owned buffers: outputs and scratch pre-filled with garbage (an index that would be a seed, a NaN
    pattern), twice with different garbage."""
    n = env["native"]
    lib = n.lib()
    for kind, H, W, r in (("edge", 37, 53, 2), ("dense", 5, 3, 8), ("one", 1, 1, 2), ("sparse", 65, 33, 0), ("corners", 64, 64, 2)):
        depth, weight = cs.scene(kind, H, W)
        d, w = G(depth), G(weight)
        ref = cs.host(kind, H, W, r)
        for junk in (0x7FC00001, 5, -7):
            scratch = torch.full((3 if r else 2, H, W), junk, dtype=torch.int32, device=DEV)
            out = torch.full((H, W), junk, dtype=torch.int32, device=DEV).view(torch.float32)
            index = torch.full((H, W), junk, dtype=torch.int32, device=DEV)
            dist2 = torch.full((H, W), junk, dtype=torch.int32, device=DEV)
            n.check(lib.be_fill_nearest_f32(n.dptr(d), n.dptr(w), H, W, r, cs.SIGMA_Z, fuse, n.dptr(scratch), n.dptr(out), n.dptr(index),
                                            n.dptr(dist2), n.stream_ptr(torch.device(DEV))), "be_fill_nearest_f32")
            _equals_host(dict(depth=out, index=index, dist2=dist2), ref, (kind, H, W, r, junk))


# ------------------------------------------------------------------------------------------ 5. no seeds, invalid depths
def test_invalid_depths_and_no_seed_at_all(env, binding):
    n = env["native"]
    depth, weight, want = cs.invalid_depths()
    for r in cs.RADII:
        for fuse in (True, False):
            out = n.fill_nearest(G(depth), G(weight), smooth=r, sigma_z=cs.SIGMA_Z, fuse=fuse)
            _equals_host(out, fill.fill_nearest_f32(depth, weight, r, cs.SIGMA_Z))
            assert np.array_equal(N(out["dist2"]) == 0, want)                           # the seeds, and no other pixel
            assert bool(torch.isfinite(out["depth"]).all()) and bool((out["depth"] > 0).all()) and bool((out["index"] >= 0).all())
            assert want.ravel()[N(out["index"])].all()
    nothing = ((np.zeros((4, 6), np.float32), None), (np.full((4, 6), np.nan, np.float32), np.ones((4, 6), np.float32)),
               (np.ones((4, 6), np.float32), np.zeros((4, 6), np.float32)), (np.full((37, 53), -np.inf, np.float32), None),
               (np.where(want, depth, 0).astype(np.float32), np.where(want, -1, 1).astype(np.float32)),
               (np.full((1, 1), np.inf, np.float32), None))
    for d, w in nothing:
        for fuse in (True, False):
            out = n.fill_nearest(G(d), G(w), fuse=fuse)
            _check_result(out, *d.shape)
            assert (_bits(N(out["depth"])) == 0).all() and bool((out["index"] == -1).all()) and bool((out["dist2"] == -1).all())
            _equals_host(out, fill.fill_nearest_f32(d, w, 2, 0.02))
    # the argument checks
    g = G(depth)
    for kw, match in ((dict(smooth=9), "smooth"), (dict(smooth=-1), "smooth"), (dict(smooth=1.0), "smooth"), (dict(smooth=True), "smooth"),
                      (dict(sigma_z=0), "sigma_z"), (dict(sigma_z=float("nan")), "sigma_z"), (dict(sigma_z="x"), "sigma_z"),
                      (dict(weight=G(np.ones((9, 11), np.float32))), "weight"), (dict(weight=np.ones((9, 12), np.float32)), "weight"),
                      (dict(weight=torch.ones(9, 12)), "weight"), (dict(weight=G(weight).double()), "weight")):
        with pytest.raises(ValueError, match=match):
            n.fill_nearest(g, **kw)
    with pytest.raises(ValueError, match="GPU"):
        n.fill_nearest(g.cpu())
    for bad in (g.double(), g[0], g[None]):
        with pytest.raises(ValueError, match="float32"):
            n.fill_nearest(bad)


# ------------------------------------------------------------------------------------------ 6. the pipeline
@pytest.mark.parametrize("entry,H,W", [("__call__", 147, 147), ("run_any", 200, 262)])
def test_pipeline_complete(env, pipe, entry, H, W):
    n = env["native"]
    img = T(synth.synthetic_image_pair(H, W, nshape=8)[0]).to(DEV)
    maps = (pipe if entry == "__call__" else getattr(pipe, entry))(img)
    keys = set(maps)
    out = pipe.complete(maps)
    assert set(out) == {"depth_dense", "measured", "index", "dist"} and set(maps) == keys
    assert out["depth_dense"].shape == (H, W) and out["depth_dense"].dtype == torch.float32
    assert out["measured"].dtype == torch.bool and out["index"].dtype == torch.int32 and out["dist"].dtype == torch.float32
    raw = n.fill_nearest(maps["depth_map"], maps["conf"])
    assert _same_bits(out["depth_dense"], raw["depth"]) and torch.equal(out["index"], raw["index"])
    assert torch.equal(out["dist"], raw["dist2"].float().sqrt()) and torch.equal(out["measured"], raw["dist2"] == 0)
    has = maps["depth_map"] > 0
    n_meas = int(out["measured"].sum())
    print(f"{entry} {H} x {W}: {int(has.sum())} pixels have depth, {n_meas} measured, farthest hole {float(out['dist'].max()):.1f} px")
    assert 0 < n_meas < H * W                                           # the synthetic weights leave holes to fill
    assert _same_bits(out["depth_dense"][has], maps["depth_map"][has])
    assert torch.equal(out["measured"], has & (maps["conf"] > 0) & torch.isfinite(maps["depth_map"]))
    assert bool((out["depth_dense"] > 0).all()) and bool(torch.isfinite(out["depth_dense"]).all())
    own = torch.arange(H * W, device=DEV, dtype=torch.int32).view(H, W)
    assert torch.equal(out["index"][out["measured"]], own[out["measured"]]) and bool((out["dist"][out["measured"]] == 0).all())
    assert bool(out["measured"].view(-1)[out["index"].view(-1).long()].all()) and bool((out["dist"][~out["measured"]] >= 1).all())
    # the host statement on the pipeline's own maps, and the other radii
    ref = fill.fill_nearest_f32(N(maps["depth_map"]), N(maps["conf"]), 2, 0.02)
    _equals_host(raw, ref)
    r0 = pipe.complete(maps, smooth=0)
    assert torch.equal(r0["index"], out["index"]) and _same_bits(r0["depth_dense"], maps["depth_map"].view(-1)[out["index"].view(-1).long()].view(H, W))
    if entry == "__call__":
        with pytest.raises(ValueError, match="GPU"):
            pipe.complete(dict(maps, depth_map=maps["depth_map"].cpu()))
        with pytest.raises(ValueError, match="GPU"):
            pipe.complete(dict(maps, conf=maps["conf"].cpu()))
        with pytest.raises(ValueError, match="GPU"):
            pipe.complete({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in maps.items()})
        with pytest.raises(ValueError, match="depth_map"):
            pipe.complete({k: v for k, v in maps.items() if k != "depth_map"})
        with pytest.raises(ValueError, match="conf"):
            pipe.complete({k: v for k, v in maps.items() if k != "conf"})
        with pytest.raises(ValueError, match="lacks"):
            pipe.complete(None)
        with pytest.raises(ValueError, match="smooth"):
            pipe.complete(maps, smooth=9)
        with pytest.raises(ValueError, match="sigma_z"):
            pipe.complete(maps, sigma_z=-1)
        # under densify 'w' / 'pp' depth_map is dense already and comes back unchanged (no module is called here)
        from be_hip.pipeline import DepthPipeline
        for mode in ("w", "pp"):
            p = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify=mode, densify_pp_module=torch.nn.Identity())
            same = p.complete(maps)
            assert same["depth_dense"] is maps["depth_map"] and bool(same["measured"].all()) and not bool(same["dist"].any())
            assert torch.equal(same["index"], own)


def test_fill_closes_the_holes_of_a_reprojection(env):
    """native.fill_nearest is general: depth=out["depth"], weight=out["valid"] of a forward warp."""
    import reproject_scenes as rs
    n = env["native"]
    c = rs.lattice_case(1)
    warped = n.reproject(G(c["depth"]), rs.SRC, rs.DST, c["pose"], rs.SIZE, near=rs.NEAR)
    holes = int((~warped["valid"]).sum())
    assert 0 < holes < warped["valid"].numel()
    out = n.fill_nearest(warped["depth"], warped["valid"], smooth=0)             # a bool mask counts as weights 1 / 0
    assert _same(out, n.fill_nearest(warped["depth"], warped["valid"].float(), smooth=0))
    assert bool((out["depth"] > 0).all()) and _same_bits(out["depth"][warped["valid"]], warped["depth"][warped["valid"]])
    _equals_host(out, fill.fill_nearest_f32(N(warped["depth"]), N(warped["valid"]).astype(np.float32), 0, 0.02))


# ------------------------------------------------------------------------------------------ 7. the workflow flag
def test_workflow_eval_complete_on_a_generated_pair(tmp_path, capsys):
    """One datagen_test pair through `workflow eval --complete` with the shipped checkpoints: an npz whose arrays are
    DepthPipeline.complete called directly, one more metrics line and the key `dense`; without the flag none of the three."""
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
    ds = data.TestDataset(DEV, data_path=str(data_dir))
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    out = tmp_path / "none"                                             # off by default: no file, no line, no key
    capsys.readouterr()
    plain = wf.main(["eval", "--out_path", str(out), *common])
    text = capsys.readouterr().out
    assert set(plain) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
    assert not out.exists() and "completed" not in text
    out = tmp_path / "dense"
    res = wf.main(["eval", "--complete", "--out_path", str(out), *common])
    text = capsys.readouterr().out
    assert set(res) == set(plain) | {"dense"} and set(res["dense"]) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel"}
    assert all(res[k] == plain[k] for k in plain if k != "seconds_per_pair")
    assert "Image pair #0 (completed): delta1 =" in text and "Average metrics for whole dataset (completed): delta1 =" in text
    img, gt = ds[0]
    maps = p(img.permute(0, 3, 1, 2).contiguous())
    want = p.complete(maps)
    got = dict(np.load(out / "complete_0000.npz"))
    assert set(got) == {"depth_dense", "measured", "index", "dist"}
    assert got["depth_dense"].shape == (147, 147) and got["depth_dense"].dtype == np.float32 and got["measured"].dtype == np.bool_
    assert got["index"].dtype == np.int32 and got["dist"].dtype == np.float32
    for k in got:
        assert np.array_equal(got[k], N(want[k])) and np.isfinite(got[k]).all(), k
    assert got["measured"].any() and not got["measured"].all() and (got["depth_dense"] > 0).all()
    dense = want["depth_dense"][None]
    m = utils.eval_depth(dense, gt[None].to(dense.dtype), dense, crop=args.crop)
    print("sparse:", {k: round(v, 4) for k, v in plain.items()}, "dense:", {k: round(v, 4) for k, v in res["dense"].items()})
    assert list(res["dense"].values()) == [float(v) for v in m]
