"""GPU tests of the folds at arbitrary positions (be_fold_records_points_f32, be_fold_refocus_stack_points_f32,
native.fold_records_points, native.fold_refocus_stack_points, DepthPipeline.sample_at / render_resized / refocus_stack(points=),
`workflow eval --render_size / --sample_points`).

Bit contracts: a point on a pixel centre is the pixel map; a point of the k = 2, 4, 8, 16 lattice is render_at's sample; every
point is evaluated on its own (permutations, reshapes, halves); plane k of the stack is the refoc map of records rendered at
rho_k.  Points outside the closed domain give zeros.  Off the lattice the maps are held to the float64 gather-form restatement
of tests/sample_at_oracle.py (tied to the pinned oracle by test_sample_at_cpu.py), fed the GPU's own float32 records, at the
bounds of test_render_at_gpu.py.  The scenes, fixtures and bounds are those of test_render_at_gpu.py."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, relmax
from be_hip import synth, tiling
import sample_at_oracle as sao
from test_render_at_gpu import (DEV, F64_BOUNDS, F64_STACK, MAPS, RHO, T, _at, _pixel_fold, _pixel_stack, _same_bits, _scene, _stack_at,
                                binding, env, pipe)  # noqa: F401  (env, pipe, binding: fixtures)

pytestmark = pytest.mark.gpu
R = 21


def P(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _points(env, sc, pts, want=MAPS):
    return env["native"].fold_records_points(sc["opts"], sc["rec"], sc["H"], sc["W"], pts, densify_w=sc["w"], want=want, **sc["grid"])


def _stack_points(env, sc, rhos, pts):
    return env["native"].fold_refocus_stack_points(sc["opts"], env["dcal"].consts, sc["rec"], rhos, sc["H"], sc["W"], pts, **sc["grid"])


def _pixel_points(H, W):
    return np.stack(np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij"), axis=-1)


# ------------------------------------------------------------------------------------------ 1. integer points == the pixel kernels
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_integer_points_equal_the_pixel_folds_bit_for_bit(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    pts = P(_pixel_points(sc["H"], sc["W"]))
    ref, got = _pixel_fold(env, sc), _points(env, sc, pts)
    assert set(got) == set(MAPS)
    for k in MAPS:
        assert got[k].is_contiguous() and _same_bits(got[k], ref[k]), k
    one = _points(env, sc, pts, want=("bndry", "conf"))                  # every map is optional
    assert set(one) == {"bndry", "conf"} and _same_bits(one["bndry"], ref["bndry"]) and _same_bits(one["conf"], ref["conf"])
    st = _stack_points(env, sc, RHO, pts)
    assert st.shape == (len(RHO), 3, sc["H"], sc["W"]) and _same_bits(st, _pixel_stack(env, sc, RHO))
    if kind == "g6":                                                    # uniform tables == the table-free call, off the lattice too
        uni = list(range(0, 147 - R + 1, 2))
        rnd = P(sao.random_points(147, 147, 5000, 3))
        tab = env["native"].fold_records_points(sc["opts"], sc["rec"], 147, 147, rnd, ys=uni, xs=uni, densify_w=sc["w"])
        free = _points(env, sc, rnd)
        for k in MAPS:
            assert _same_bits(tab[k], free[k]), k


# ------------------------------------------------------------------------------------------ 2. dyadic lattice points == render_at
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_dyadic_lattice_points_equal_render_at_bit_for_bit(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    H, W = sc["H"], sc["W"]
    win = (H - 23, W - 31, 23, 31)
    for k in (2, 4, 8, 16):
        for window in (None, win):
            lat = tiling.lattice(H, W, k, window)
            pts = P(tiling.resize_points(H, W, (lat["Ho"], lat["Wo"]), window))
            got, ref = _points(env, sc, pts), _at(env, sc, k, window)
            for m in MAPS:
                assert _same_bits(got[m], ref[m]), (k, window, m)
            if window is not None or k <= 4:
                rhos = RHO[:9]                                          # one full chunk and a short one
                assert _same_bits(_stack_points(env, sc, rhos, pts), _stack_at(env, sc, rhos, k, window)), (k, window)


# ------------------------------------------------------------------------------------------ 3. per-point independence
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_every_point_is_evaluated_on_its_own(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    n = 6000
    base = sao.random_points(sc["H"], sc["W"], n, 5)
    base[::7] = np.round(base[::7])                                     # pixel centres among them
    base[1::7, 0] = np.round(base[1::7, 0])                             # and points integer on one axis only
    pts = P(base)
    got, st = _points(env, sc, pts), _stack_points(env, sc, RHO[:9], pts)
    assert all(torch.isfinite(v).all() for v in got.values()) and torch.isfinite(st).all()
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(DEV)
    gp, sp = _points(env, sc, pts[perm]), _stack_points(env, sc, RHO[:9], pts[perm])
    for m in MAPS:
        assert _same_bits(gp[m], got[m][..., perm]), m
    assert _same_bits(sp, st[..., perm])
    gr, sr = _points(env, sc, pts.view(4, 50, 30, 2)), _stack_points(env, sc, RHO[:9], pts.view(60, 100, 2))
    for m in MAPS:
        assert gr[m].shape == got[m].shape[:-1] + (4, 50, 30) and _same_bits(gr[m].reshape(got[m].shape), got[m]), m
    assert sr.shape == (9, 3, 60, 100) and _same_bits(sr.reshape(st.shape), st)
    cut = 2501                                                          # not a multiple of the workgroup
    ga, gb = _points(env, sc, pts[:cut]), _points(env, sc, pts[cut:])
    for m in MAPS:
        assert _same_bits(torch.cat([ga[m], gb[m]], dim=-1), got[m]), m
    assert _same_bits(torch.cat([_stack_points(env, sc, RHO[:9], pts[:cut]), _stack_points(env, sc, RHO[:9], pts[cut:])], dim=-1), st)
    single = _points(env, sc, pts[17:18])                               # N = 1
    for m in MAPS:
        assert _same_bits(single[m], got[m][..., 17:18]), m


# ------------------------------------------------------------------------------------------ 4. the domain
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_domain_edges_and_points_outside(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    H, W = sc["H"], sc["W"]
    ref, ref_stack = _pixel_fold(env, sc), _pixel_stack(env, sc, RHO[:9])
    inside = np.array([[H - 1, W - 1], [H - 1, 0], [0, W - 1], [0, 0], [H - 1, 30.5], [40.25, W - 1], [57.75, 90.125]], np.float32)
    nan, inf = np.nan, np.inf
    outside = np.array([[-0.25, 10], [10, -0.25], [H - 1 + 1e-3, 10], [10, W - 1 + 1e-3], [nan, 10], [10, nan], [nan, nan], [inf, 10],
                        [10, -inf], [-inf, inf], [-1e-30, 5], [1e30, 5], [H, W]], np.float32)
    assert sao.valid_points(inside, H, W).all() and not sao.valid_points(outside, H, W).any()
    alone = _points(env, sc, P(inside))
    alone_stack = _stack_points(env, sc, RHO[:9], P(inside))
    mixed = np.empty((len(inside) + len(outside), 2), np.float32)       # interleaved: the neighbours of a bad point are unchanged
    where_in = np.arange(len(inside)) * 2
    where_out = np.setdiff1d(np.arange(len(mixed)), where_in)
    mixed[where_in], mixed[where_out] = inside, outside
    assert len(where_out) == len(outside)
    got, st = _points(env, sc, P(mixed)), _stack_points(env, sc, RHO[:9], P(mixed))
    where_in, where_out = torch.from_numpy(where_in).to(DEV), torch.from_numpy(where_out).to(DEV)
    for m in MAPS:
        assert _same_bits(got[m][..., where_in].contiguous(), alone[m]), m
        assert (got[m][..., where_out].contiguous().view(torch.int32) == 0).all(), m    # +0.0, not NaN
        for n, (y, x) in enumerate(((H - 1, W - 1), (H - 1, 0), (0, W - 1), (0, 0))):   # the corners are the last / first pixels
            assert _same_bits(alone[m][..., n], ref[m][..., y, x]), (m, n)
        assert torch.isfinite(alone[m]).all(), m
    assert _same_bits(st[..., where_in].contiguous(), alone_stack) and (st[..., where_out].contiguous().view(torch.int32) == 0).all()
    assert _same_bits(alone_stack[..., 0], ref_stack[..., H - 1, W - 1])
    only_bad = _points(env, sc, P(outside))
    assert all((v.view(torch.int32) == 0).all() for v in only_bad.values())


def test_point_under_no_patch_is_zero_over_zero(env, binding):
    """A uniform grid that stops short of the edge: 150 x 150 with the 64 x 64 stride-2 grid ends at pixel 146, so a point in
    (146, 149] is inside the domain and under no patch - 0/0 as in the pixel fold, not the zeros of an invalid point."""
    n = env["native"]
    sc = _scene(env, "g6", None)
    pts = P(np.array([[146.0, 146.0], [146.5, 30.0], [30.0, 149.0], [149.0, 149.0]], np.float32))
    got = n.fold_records_points(sc["opts"], sc["rec"], 150, 150, pts, hp=64, wp=64, stride=2)
    ref = n.fold_records(sc["opts"], sc["rec"], 64, 64, 150, 150, 2, False)
    for m in ("image", "shpd", "refoc", "bndry", "conf"):
        assert _same_bits(got[m][..., 0], ref[m][..., 146, 146]) and torch.isfinite(got[m][..., 0]).all(), m
        assert torch.isnan(got[m][..., 1:]).all(), m
    assert (got["depth"][1:] == 0).all()                                # depth divides by max(cntz, 1)


def test_stack_point_under_no_patch_is_zero_over_zero(env, binding):
    """The same grid and points through the stack: a short last chunk (K = 9), the covered point equals the pixel stack bit for
    bit, the points under no patch are its 0/0 - NaN bits included where the point is a pixel."""
    n = env["native"]
    sc = _scene(env, "g6", None)
    pts = P(np.array([[146.0, 146.0], [146.5, 30.0], [30.0, 149.0], [149.0, 149.0]], np.float32))
    st = n.fold_refocus_stack_points(sc["opts"], env["dcal"].consts, sc["rec"], RHO[:9], 150, 150, pts, hp=64, wp=64, stride=2)
    ref = n.fold_refocus_stack(sc["opts"], env["dcal"].consts, sc["rec"], RHO[:9], 150, 150, hp=64, wp=64, stride=2)
    assert st.shape == (9, 3, 4)
    assert _same_bits(st[..., 0], ref[..., 146, 146]) and torch.isfinite(st[..., 0]).all()
    assert torch.isnan(st[..., 1:]).all()
    assert _same_bits(st[..., 2], ref[..., 30, 149]) and _same_bits(st[..., 3], ref[..., 149, 149])


# ------------------------------------------------------------------------------------------ 5. stack consistency
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_stack_plane_equals_the_point_fold_of_records_rendered_at_that_power(env, binding, kind):
    n = env["native"]
    sc = _scene(env, kind, None)
    pts = P(np.concatenate([sao.random_points(sc["H"], sc["W"], 8000, 9), _pixel_points(sc["H"], sc["W"])[::5, ::7].reshape(-1, 2)]))
    st = _stack_points(env, sc, RHO, pts)
    for p, rho in enumerate(RHO):
        if kind == "g6":
            img = T(synth.synthetic_image_pair(147, 147)[0]).to(DEV)
            p12 = T(synth.plausible_params12(4096, name="g6_est")).to(DEV)
            rec, _ = n.render_full(sc["opts"], env["dcal"].consts, rho, False, p12, n.view_image_pair(img, 2), pixels=img)
        else:
            img = T(synth.synthetic_image_pair(200, 262, nshape=8)[0]).to(DEV)
            est = T(synth.plausible_params12(91 * 122, name="any_200x262")).to(DEV)
            rec = n.render_full_grid(sc["opts"], env["dcal"].consts, rho, False, est, img, sc["ys"], sc["xs"])
        ref = n.fold_records_points(sc["opts"], rec, sc["H"], sc["W"], pts, want=("refoc",), **sc["grid"])["refoc"]
        assert _same_bits(st[p], ref), (p, rho)
    assert not torch.equal(st[0], st[-1])


# ------------------------------------------------------------------------------------------ 6. against float64
def _hold_to_oracle(tag, got, stack, want, n_rho):
    err = {m: relmax(got[m], want[m]) for m in MAPS}
    flips = np.abs(got["conf"] - want["conf"]) > 1e-6
    share = float(flips.mean())
    serr = [relmax(stack[p], want["stack"][p]) for p in range(n_rho)]
    print(f"\nsample_at {tag}: relmax vs float64 " + "  ".join(f"{m} {err[m]:.2e}" for m in MAPS)
          + f"  conf flip share {share:.2e} of {flips.size}  stack " + " ".join(f"{e:.2e}" for e in serr))
    for m in MAPS:
        assert np.isfinite(got[m]).all(), m
    for m in ("image", "shpd", "refoc", "bndry"):
        assert err[m] <= F64_BOUNDS[m], (m, err[m])
    assert share <= 2e-3, share
    ok = ~flips
    assert relmax(got["conf"][ok], want["conf"][ok]) <= F64_BOUNDS["conf"]
    assert relmax(got["depth"][ok], want["depth"][ok]) <= F64_BOUNDS["depth"]
    for e in serr:
        assert e <= F64_STACK, serr


@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
@pytest.mark.parametrize("what", ["random", "k3"])
def test_points_against_the_float64_restatement(env, kind, densify, what):
    """20 000 seeded random points per scene, and the k = 3 lattice (whose fractions 1/3, 2/3 are rounded in float32), against
    sample_at_oracle.fold_points in float64.  Measured on the MI355X: profiles/HISTORY.md round 13."""
    from oracle import depth as od
    sc = _scene(env, kind, densify)
    H, W = sc["H"], sc["W"]
    pts = sao.random_points(H, W, 20000, 7) if what == "random" else sao.lattice_points(3, (0, 0, H, W))
    rhos = [RHO[0], RHO[8], RHO[10]]
    got = {m: v.double().cpu().numpy() for m, v in _points(env, sc, P(pts)).items()}
    stack = _stack_points(env, sc, rhos, P(pts)).double().cpu().numpy()
    want = sao.fold_points(sc["rec"].cpu().numpy(), sc["ys"], sc["xs"], H, W, pts, np.float64, densify_w=sc["w"], rho_primes=rhos,
                           consts=od.depth_consts())
    assert want["valid"].all() and int(want["count"].min()) >= 1
    _hold_to_oracle(f"{kind} {what} densify={densify}", got, stack, want, len(rhos))
    if what == "k3":                                                    # and next to render_at: the same samples up to the fraction's rounding
        fine = _at(env, sc, 3)
        assert relmax(got["bndry"], fine["bndry"].double().cpu().numpy()) <= 2 * F64_BOUNDS["bndry"]


# ------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("entry,H,W", [("__call__", 147, 147), ("run_big", 235, 323), ("run_any", 200, 262)])
def test_pipeline_sample_at(pipe, entry, H, W):
    img = T(synth.synthetic_image_pair(H, W, nshape=8)[0]).to(DEV)
    run = pipe if entry == "__call__" else getattr(pipe, entry)
    maps = run(img)
    keys = set(maps)
    g = maps["grid"]
    # the pixel grid as points: the maps themselves; array-likes and other dtypes are converted to float32
    pix = _pixel_points(H, W)
    for pts in (pix, torch.from_numpy(pix).double(), torch.from_numpy(pix).to(DEV), pix.astype(np.int64)):
        s = pipe.sample_at(maps, pts)
        assert set(s) == set(MAPS) | {"depth_map", "valid"}
        assert s["valid"].dtype == torch.bool and s["valid"].shape == (H, W) and s["valid"].is_cuda and bool(s["valid"].all())
        for m in MAPS:
            assert s[m].dtype == torch.float32 and _same_bits(s[m], maps[m]), m
    thres = pipe.depth_thres if entry == "__call__" else 0.05
    s = pipe.sample_at(maps, pix, depth_thres=thres)
    assert _same_bits(s["depth_map"], maps["depth_map"])
    # render_resized at a dyadic ratio is render_at; the lattice key
    for k in (2, 4):
        rr = pipe.render_resized(maps, ((H - 1) * k + 1, (W - 1) * k + 1))
        ra = pipe.render_at(maps, scale=k)
        assert set(rr) == set(MAPS) | {"depth_map", "valid", "lattice"}
        assert rr["lattice"] == dict(size=((H - 1) * k + 1, (W - 1) * k + 1), window=(0, 0, H, W))
        for m in MAPS + ("depth_map",):
            assert _same_bits(rr[m], ra[m]), (k, m)
    win = (H - 30, W - 41, 30, 41)
    rr = pipe.render_resized(maps, (117, 161), window=win, want=("bndry", "refoc"))
    ra = pipe.render_at(maps, scale=4, window=win, want=("bndry", "refoc"))
    assert set(rr) == {"bndry", "refoc", "depth_map", "valid", "lattice"} and rr["lattice"]["window"] == win
    assert _same_bits(rr["bndry"], ra["bndry"]) and _same_bits(rr["refoc"], ra["refoc"]) and _same_bits(rr["depth_map"], ra["depth_map"])
    # a non-integer ratio, up and down, against the float64 oracle on the pipeline's own records
    from oracle import depth as od
    ys = list(range(0, g["stride"] * g["hp"], g["stride"])) if g["ys"] is None else g["ys"].cpu().tolist()
    xs = list(range(0, g["stride"] * g["wp"], g["stride"])) if g["xs"] is None else g["xs"].cpu().tolist()
    rhos = [pipe.rho_prime, 9.9054, 10.5964]
    for size in ((220, (W * 3) // 2), (100, 90)):
        rr = pipe.render_resized(maps, size, depth_thres=thres)
        pts = tiling.resize_points(H, W, size)
        assert all(rr[m].shape[-2:] == size for m in MAPS) and rr["image"].shape == (2, 3) + size and bool(rr["valid"].all())
        assert _same_bits(rr["depth_map"], torch.where(rr["conf"] > thres, rr["depth"], torch.zeros_like(rr["depth"])))
        for m in MAPS:                                                  # the corners are the image's corner pixels
            assert _same_bits(rr[m][..., 0, 0], maps[m][..., 0, 0]) and _same_bits(rr[m][..., -1, -1], maps[m][..., -1, -1]), m
        st = pipe.refocus_stack(maps, rho_primes=rhos, points=pts)
        assert st.shape == (3, 3) + size and _same_bits(st[0], rr["refoc"])
        want = sao.fold_points(maps["records"].cpu().numpy(), ys, xs, H, W, pts, np.float64, densify_w=pipe.densify == "w", rho_primes=rhos,
                               consts=od.depth_consts())
        _hold_to_oracle(f"{entry} resized to {size}", {m: rr[m].double().cpu().numpy() for m in MAPS}, st.double().cpu().numpy(), want, 3)
    # keypoints, some of them outside
    kp = np.array([[10.5, 20.25], [H - 1, W - 1], [-1, 5], [5, W], [np.nan, 1], [33.333, 44.444]], np.float32)
    s = pipe.sample_at(maps, kp, want=("depth", "bndry"))
    assert set(s) == {"depth", "bndry", "depth_map", "valid"} and s["valid"].tolist() == [True, True, False, False, False, True]
    assert s["depth"].shape == (6,) and (s["bndry"][2:5] == 0).all() and (s["depth_map"][2:5] == 0).all()
    assert _same_bits(s["bndry"][1], maps["bndry"][H - 1, W - 1])
    st = pipe.refocus_stack(maps, focus_depths=[0.751, 1.0], points=kp)
    assert st.shape == (2, 3, 6) and (st[..., 2:5] == 0).all() and torch.isfinite(st).all()
    assert _same_bits(st[..., 1], pipe.refocus_stack(maps, focus_depths=[0.751, 1.0])[..., H - 1, W - 1])
    # nothing the entry point returns has changed
    again = run(img)
    assert set(again) == keys == set(maps)
    for k, v in maps.items():
        if k != "grid":
            assert _same_bits(v, again[k]), k
    # the error cases, with a live pipeline
    with pytest.raises(ValueError, match="points"):
        pipe.sample_at(maps, np.zeros((5, 3)))
    with pytest.raises(ValueError, match="records"):
        pipe.sample_at({k: v for k, v in maps.items() if k != "records"}, kp)
    with pytest.raises(ValueError, match="GPU"):
        pipe.sample_at(dict(maps, records=maps["records"].cpu()), kp)
    with pytest.raises(ValueError, match="unknown maps"):
        pipe.sample_at(maps, kp, want=("depth_map",))
    with pytest.raises(ValueError, match="size"):
        pipe.render_resized(maps, (0, 10))
    with pytest.raises(ValueError, match="without scale / window"):
        pipe.refocus_stack(maps, rho_primes=rhos, points=kp, scale=2)


def test_sample_at_without_depth_map_under_densify_pp(pipe, env):
    """densify == 'pp': the U-Net is not defined off its native resolution, so there is no depth_map key."""
    import models
    from be_hip.pipeline import DepthPipeline
    unet = models.DepthCompletion()
    unet.load_state_dict({k: T(v) if v.dtype != np.int64 else torch.from_numpy(np.asarray(v)) for k, v in synth.unet_state_dict().items()})
    pp = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify="pp", densify_pp_module=unet.to(DEV).eval())
    img = T(synth.synthetic_image_pair(147, 147, nshape=8)[0]).to(DEV)
    maps = pp(img)
    s = pp.sample_at(maps, _pixel_points(147, 147))
    assert set(s) == set(MAPS) | {"valid"}
    assert _same_bits(s["depth"], maps["depth"])
    only = pp.sample_at(maps, [[3.5, 4.5]], want=("bndry",))
    assert set(only) == {"bndry", "valid"}
    assert set(pp.render_resized(maps, (200, 180))) == set(MAPS) | {"valid", "lattice"}


# ------------------------------------------------------------------------------------------ 8. the workflow flags
def test_workflow_eval_render_size_and_sample_points_on_generated_pairs(tmp_path):
    """Two datagen_test pairs through `workflow eval --render_size 220 200 --sample_points FILE` with the shipped checkpoints, plain
    and --any: per pair one npz of each kind whose arrays are DepthPipeline.render_resized / sample_at called directly; no file
    when the flags are absent."""
    import data
    import models
    import utils
    from be_hip import datagen_test as dt, workflow as wf
    from be_hip.pipeline import DepthPipeline
    data_dir = tmp_path / "set"
    dt.save(dt.generate(dt.ProceduralSource(5), 2, (147, 147), DEV, seed=5, n_interval=40), str(data_dir))
    ckpt = os.path.join(ROOT, "checkpoints")
    args = utils.get_args("eval", argv=["--data_path", str(data_dir), "--model_path", ckpt])
    load = lambda m, name: (m.load_state_dict(torch.load(os.path.join(ckpt, name), map_location=DEV)), m.eval())[1]
    local = load(models.LocalStage().to(DEV), "pretrained_local_stage.pth")
    globl = load(models.GlobalStage(in_parameter_size=38, out_parameter_size=12, device=DEV).to(DEV), "pretrained_global_stage.pth")
    pipe = DepthPipeline(local, globl, utils.PostProcessGlobalBase(args, DEV), utils.DepthEtas(args, DEV), rho_prime=args.rho_prime,
                         stride=args.stride)
    ds = data.TestDataset(DEV, data_path=str(data_dir))
    assert len(ds) == 2
    names = ("shpd", "refoc", "bndry", "depth", "conf", "depth_map")
    kp = np.concatenate([sao.random_points(147, 147, 500, 2), np.array([[146, 146], [-1, 3], [np.nan, 3]], np.float32)]).astype(np.float64)
    np.save(tmp_path / "kp.npy", kp)
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    for mode in ((), ("--any",)):
        out = tmp_path / ("fine" + "".join(mode))
        res = wf.main(["eval", *mode, "--render_size", "220", "200", "--sample_points", str(tmp_path / "kp.npy"), "--out_path", str(out),
                       *common])
        assert set(res) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
        for j in range(2):
            img = ds[j][0].permute(0, 3, 1, 2).contiguous()
            maps = pipe.run_any(img) if mode else pipe(img)
            thres = 0.05 if mode else None
            got = dict(np.load(out / f"render_220x200_{j:04d}.npz"))
            want = pipe.render_resized(maps, (220, 200), depth_thres=thres)
            assert set(got) == set(names)
            for k in names:
                assert got[k].dtype == np.float32 and got[k].shape[-2:] == (220, 200) and np.isfinite(got[k]).all(), (mode, j, k)
                assert np.array_equal(got[k], want[k].cpu().numpy()), (mode, j, k)
            got = dict(np.load(out / f"samples_{j:04d}.npz"))
            want = pipe.sample_at(maps, kp, depth_thres=thres)
            assert set(got) == set(names) | {"valid"}
            assert got["valid"].dtype == np.bool_ and got["valid"].shape == (503,) and got["valid"].tolist() == [True] * 501 + [False] * 2
            for k in names:
                assert got[k].dtype == np.float32 and got[k].shape[-1:] == (503,) and got[k].shape[:-1] == want[k].shape[:-1], (mode, j, k)
                assert np.array_equal(got[k], want[k].cpu().numpy()) and np.all(got[k][..., 501:] == 0), (mode, j, k)
    out = tmp_path / "none"                                             # off by default: no file is written
    wf.main(["eval", "--out_path", str(out), *common])
    assert not out.exists()
    np.save(tmp_path / "bad.npy", np.zeros((4, 3)))
    with pytest.raises(ValueError, match="sample_points"):
        wf.main(["eval", "--sample_points", str(tmp_path / "bad.npy"), "--out_path", str(out), *common])
