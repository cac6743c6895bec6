"""GPU tests of the focal stack (be_fold_refocus_stack_f32, native.fold_refocus_stack, DepthPipeline.refocus_stack, `workflow eval
--refocus_stack`).  Every plane must equal, bit for bit, the refocused map the existing path gives for that optical power
(render_full*(rho_prime) + fold_records*(want=("refoc",))), computed here from the records of ONE render at 10.39; the planes are
also held to the float64 oracle and to the reference's own float64 run (golden g20) at the bound the project holds `refoc` to."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, relmax
from be_hip import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 21
# 9.4928 / 10.1106 / 10.5964 are the planes of golden g20 (focus at 2.30 / 0.95 / 0.65 m); 10.39 is the pipeline's default
RHO = [9.4928, 9.6830, 9.9054, 10.0, 10.0104, 10.1106, 10.2, 10.2344, 10.39, 10.5964, 11.0]
F64_REFOC = 1e-4      # test_fold_maps_vs_golden / F64_BOUNDS["refoc"] of test_any_size_gpu.py: the bound this map is already held to


def T(a, dt=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dt)


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    import utils
    from be_hip import native
    native.lib()
    a = utils.get_args("eval", argv=[])
    return dict(native=native, args=a, helper=utils.PostProcessGlobalBase(a, DEV), dcal=utils.DepthEtas(a, DEV))


@pytest.fixture(scope="module")
def pipe(env):
    import models
    from be_hip.pipeline import DepthPipeline
    lm = models.LocalStage()
    lm.load_state_dict({k: T(v) for k, v in synth.local_stage_state_dict().items()})
    gm = models.GlobalStage(device=DEV)
    gm.load_state_dict({k: T(v) for k, v in synth.global_stage_state_dict().items()})
    return DepthPipeline(lm.to(DEV).eval(), gm.to(DEV).eval(), env["helper"], env["dcal"])


@pytest.fixture(params=["torch_ops", "ctypes"])
def binding(request, env, monkeypatch):
    """Both bindings of the new entry: torch.ops.be.fold_refocus_stack (the default) and the ctypes prototype."""
    n = env["native"]
    assert n.ops() is not None
    if request.param == "ctypes":
        monkeypatch.setattr(n, "_ops", False)
        assert n.ops() is None
    return request.param


def _img(H, W, nshape=6):
    return T(synth.synthetic_image_pair(H, W, nshape=nshape)[0]).to(DEV)


def _g6(env, densify):
    """G6's inputs: (img, params12, opts, densify_w)."""
    img = T(synth.synthetic_image_pair(147, 147)[0]).to(DEV)
    p12 = T(synth.plausible_params12(4096, name="g6_est")).to(DEV)
    return img, p12, env["helper"].render_opts(wrap_angles=False), densify == "w"


def _same_bits(a, b):
    """Equality of two float32 tensors as bit patterns (a record may hold an infinite depth for a wedge that owns no pixel)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _slices():
    from be_hip import native
    kc = native.REFOCUS_STACK_KC
    assert 1 <= kc and kc + 1 <= len(RHO)
    return kc, [RHO, RHO[:1], RHO[:kc], RHO[:kc + 1], RHO[-1:]]


# ------------------------------------------------------------------------------------------ bit for bit, uniform grid
@pytest.mark.parametrize("densify", [None, "w"])
def test_every_plane_equals_render_plus_fold_at_that_power(env, binding, densify):
    n = env["native"]
    img, p12, opts, w = _g6(env, densify)
    view = lambda: n.view_image_pair(img, 2)
    rec, _ = n.render_full(opts, env["dcal"].consts, 10.39, w, p12, view(), pixels=img)        # ONE render, at the default power
    ref = []
    for rho in RHO:
        r, _ = n.render_full(opts, env["dcal"].consts, rho, w, p12, view(), pixels=img)
        ref.append(n.fold_records(opts, r, 64, 64, 147, 147, 2, w, want=("refoc",))["refoc"])
        # nothing of the record but the two refocus radii depends on rho_prime
        assert _same_bits(r[:, :18], rec[:, :18]) and _same_bits(r[:, 20:], rec[:, 20:])
    assert not torch.equal(ref[0], ref[-1])
    kc, slices = _slices()
    for rhos in slices:
        stack = n.fold_refocus_stack(opts, env["dcal"].consts, rec, rhos, 147, 147, hp=64, wp=64, stride=2)
        assert stack.shape == (len(rhos), 3, 147, 147) and stack.dtype == torch.float32 and stack.is_contiguous()
        for k, rho in enumerate(rhos):
            assert torch.equal(stack[k], ref[RHO.index(rho)]), (len(rhos), k, rho)
    # a device float32 tensor of powers is taken as it is; the records of a render at another power give the same stack
    dev_rho = torch.tensor(RHO, dtype=torch.float32, device=DEV)
    stack = n.fold_refocus_stack(opts, env["dcal"].consts, rec, dev_rho, 147, 147, hp=64, wp=64)
    other, _ = n.render_full(opts, env["dcal"].consts, RHO[0], w, p12, view(), pixels=img)
    again = n.fold_refocus_stack(opts, env["dcal"].consts, other, RHO, 147, 147, hp=64, wp=64)
    for k in range(len(RHO)):
        assert torch.equal(stack[k], ref[k]) and torch.equal(again[k], ref[k]), k


# ------------------------------------------------------------------------------------------ bit for bit, origin tables
@pytest.mark.parametrize("densify", [None, "w"])
def test_origin_tables_flush_grid_and_uniform_tables(env, binding, densify):
    from be_hip import tiling
    n = env["native"]
    H, W = 200, 262
    img = _img(H, W, nshape=8)
    ys, xs = tiling.patch_grid(H, 2), tiling.patch_grid(W, 2)
    HP, WP = len(ys), len(xs)
    assert (HP, WP) == (91, 122) and ys[-2:] == [178, 179] and xs[-2:] == [240, 241]              # a flush row and a flush column
    est = T(synth.plausible_params12(HP * WP, name="any_200x262")).to(DEV)
    opts, w = env["helper"].render_opts(wrap_angles=False), densify == "w"
    rec = n.render_full_grid(opts, env["dcal"].consts, 10.39, w, est, img, ys, xs)
    ref = [n.fold_records_grid(opts, n.render_full_grid(opts, env["dcal"].consts, rho, w, est, img, ys, xs), H, W, ys, xs, w,
                               want=("refoc",))["refoc"] for rho in RHO]
    kc, slices = _slices()
    for rhos in slices:
        stack = n.fold_refocus_stack(opts, env["dcal"].consts, rec, rhos, H, W, ys=ys, xs=xs)
        assert stack.shape == (len(rhos), 3, H, W)
        for k, rho in enumerate(rhos):
            assert torch.isfinite(stack[k]).all()
            assert torch.equal(stack[k], ref[RHO.index(rho)]), (len(rhos), k, rho)
    dys, dxs = n.origin_table(ys, H, DEV), n.origin_table(xs, W, DEV)                            # device tables are taken as they are
    assert torch.equal(n.fold_refocus_stack(opts, env["dcal"].consts, rec, RHO[:3], H, W, ys=dys, xs=dxs, hp=HP, wp=WP), torch.stack(ref[:3]))
    # uniform tables 0, 2, 4, .. on 147 x 147 == the table-free call
    img, p12, opts, w = _g6(env, densify)
    rec, _ = n.render_full(opts, env["dcal"].consts, 10.39, w, p12, n.view_image_pair(img, 2), pixels=img)
    uni = list(range(0, 147 - R + 1, 2))
    a = n.fold_refocus_stack(opts, env["dcal"].consts, rec, RHO, 147, 147, ys=uni, xs=uni)
    b = n.fold_refocus_stack(opts, env["dcal"].consts, rec, RHO, 147, 147, hp=64, wp=64, stride=2)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("densify", [None, "w"])
def test_planes_against_the_float64_oracle_and_the_reference_run(env, densify):
    from oracle import render as orr, depth as od, tiling as ot
    n = env["native"]
    img, p12, opts, w = _g6(env, densify)
    rec, _ = n.render_full(opts, env["dcal"].consts, 10.39, w, p12, n.view_image_pair(img, 2), pixels=img)
    stack = n.fold_refocus_stack(opts, env["dcal"].consts, rec, RHO, 147, 147, hp=64, wp=64).cpu()
    assert torch.isfinite(stack).all()
    pat = ot.unfold_patches(img.cpu()).double()
    errs = []
    for k, rho in enumerate(RHO):
        r64 = orr.render_pass_b(od.depth_consts(), p12.cpu().double(), pat[0], pat[1], rho_prime=rho, densify=densify)
        errs.append(relmax(stack[k], ot.fold_mean(r64["refoc"][None], 147, 147)[0]))
    print(f"\nfocal stack vs float64 oracle, densify={densify}: relmax per power " + "  ".join(f"{r}: {e:.2e}" for r, e in zip(RHO, errs)))
    g = load_golden("g20_refocus_stack")
    gerr = []
    if densify is None:                                              # g20 is the reference's run with densify = None
        gerr = [relmax(stack[RHO.index(round(float(rho), 4))], g["fold_refoc"][j]) for j, rho in enumerate(g["rho_primes"])]
        assert len(gerr) == 3
        print("focal stack vs the reference's float64 run (g20): " + "  ".join(f"{e:.2e}" for e in gerr))
    for e in errs + gerr:
        assert e <= F64_REFOC, (errs, gerr)


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("entry,H,W", [("__call__", 147, 147), ("run_big", 235, 323), ("run_any", 200, 262)])
def test_pipeline_refocus_stack(pipe, entry, H, W):
    img = _img(H, W, nshape=8)
    run = pipe if entry == "__call__" else getattr(pipe, entry)
    maps = run(img)
    assert "records" in maps and set(maps["grid"]) == {"H", "W", "hp", "wp", "stride", "ys", "xs"}
    assert (maps["grid"]["ys"] is None) == (entry != "run_any")
    one = pipe.refocus_stack(maps, rho_primes=[pipe.rho_prime])
    assert one.shape == (1, 3, H, W) and torch.equal(one[0], maps["refoc"])                     # the default power IS maps["refoc"]
    a = pipe.refocus_stack(maps, focus_depths=[0.751])
    b = pipe.refocus_stack(maps, rho_primes=[pipe.dcal.focus2rho(0.751)])
    assert torch.equal(a, b)
    assert torch.equal(pipe.refocus_stack(maps, focus_depths=torch.tensor([0.751, 1.0])),
                       pipe.refocus_stack(maps, rho_primes=[pipe.dcal.focus2rho(0.751), pipe.dcal.focus2rho(1.0)]))
    stack = pipe.refocus_stack(maps, focus_depths=[2.3, 1.18, 0.95, 0.75, 0.65])
    assert stack.shape == (5, 3, H, W) and torch.isfinite(stack).all()
    assert not torch.equal(stack[0], stack[4])
    # the two new keys are additions: everything the entry point returned before is what a second call returns
    again = run(img)
    assert set(again) == set(maps)
    for k, v in maps.items():
        if k != "grid":
            assert _same_bits(v, again[k]), k
    # host checks with a live pipeline
    with pytest.raises(ValueError, match="exactly one"):
        pipe.refocus_stack(maps)
    with pytest.raises(ValueError, match="records"):
        pipe.refocus_stack({k: v for k, v in maps.items() if k != "records"}, rho_primes=[10.39])
    with pytest.raises(ValueError, match="GPU"):
        pipe.refocus_stack(dict(maps, records=maps["records"].cpu()), rho_primes=[10.39])
    with pytest.raises(ValueError, match="rho_primes"):
        pipe.refocus_stack(maps, rho_primes=[])


def test_native_errors(env):
    n = env["native"]
    img, p12, opts, w = _g6(env, None)
    rec, _ = n.render_full(opts, env["dcal"].consts, 10.39, w, p12, n.view_image_pair(img, 2), pixels=img)
    c = env["dcal"].consts
    with pytest.raises(ValueError, match="rho_primes"):
        n.fold_refocus_stack(opts, c, rec, [float("nan")], 147, 147, hp=64, wp=64)
    with pytest.raises(RuntimeError):
        n.fold_refocus_stack(opts, c, rec[:100], [10.39], 147, 147, hp=64, wp=64)             # records do not match the grid
    with pytest.raises(RuntimeError):
        n.fold_refocus_stack(opts, c, rec, [10.39], 147, 147)                                # uniform grid without hp / wp
    with pytest.raises(RuntimeError, match="exceeds the image"):
        n.fold_refocus_stack(opts, c, rec, [10.39], 145, 147, hp=64, wp=64)
    ys = list(range(0, 127, 2))
    with pytest.raises(ValueError, match="cover"):
        n.fold_refocus_stack(opts, c, rec[:63 * 64], [10.39], 147, 147, ys=ys[:-1], xs=ys)
    with pytest.raises(ValueError, match="both"):
        n.fold_refocus_stack(opts, c, rec, [10.39], 147, 147, ys=ys)


# ------------------------------------------------------------------------------------------ the workflow flag
def test_workflow_eval_refocus_stack_on_generated_pairs(tmp_path):
    """Two datagen_test pairs through `workflow eval --refocus_stack 4` with the shipped checkpoints: one [K,3,H,W] file per pair
    plus the powers; plane k is DepthPipeline.refocus_stack called directly.  Plain and --any modes (the same pairs)."""
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
    K = 4
    sweep = wf.focus_sweep(pipe.dcal, K, 0.75, 1.18)
    for mode in ((), ("--any",)):
        out = tmp_path / ("stack" + "".join(mode))
        res = wf.main(["eval", *mode, "--refocus_stack", str(K), "--out_path", str(out), "--model_path", ckpt, "--data_path", str(data_dir),
                       "--cuda", DEV])
        assert set(res) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
        rho = np.load(out / "rho_primes.npy")
        assert rho.shape == (K,) and rho.dtype == np.float32 and np.array_equal(rho, sweep.astype(np.float32))
        for j in range(2):
            got = np.load(out / f"refoc_stack_{j:04d}.npy")
            assert got.shape == (K, 3, 147, 147) and got.dtype == np.float32 and np.isfinite(got).all()
            img = ds[j][0].permute(0, 3, 1, 2).contiguous()
            maps = pipe.run_any(img) if mode else pipe(img)
            want = pipe.refocus_stack(maps, rho_primes=sweep.tolist())
            assert np.array_equal(got, want.cpu().numpy()), (mode, j)
            assert not np.array_equal(got[0], got[-1])
    # off by default: no file is written
    out = tmp_path / "none"
    wf.main(["eval", "--out_path", str(out), "--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV])
    assert not out.exists()
