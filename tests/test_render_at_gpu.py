"""GPU tests of the folds on a finer lattice (be_fold_records_at_f32, be_fold_refocus_stack_at_f32, native.fold_records_at,
native.fold_refocus_stack_at, DepthPipeline.render_at, DepthPipeline.refocus_stack(scale=..), `workflow eval --render_scale`).

Two bit contracts: at scale 1 over the whole image the new kernels equal fold_records / fold_records_grid / fold_refocus_stack, and
at every scale the samples [::k, ::k] equal the scale-1 maps - every k-th sample of the lattice IS an input pixel.  Windows are
slices of the full lattice.  The samples in between are held to the float64 restatement of tests/render_at_oracle.py (tied to the
pinned oracle by test_render_at_cpu.py), fed the GPU's own float32 records, at the bounds test_any_size_gpu.py holds the pixel maps
to.  Measured on the MI355X (relmax; densify None / 'w'): see profiles/HISTORY.md, round 12."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, relmax
from be_hip import synth, tiling
import render_at_oracle as rao

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R = 21
MAPS = ("image", "shpd", "refoc", "bndry", "depth", "conf")
RHO = [9.4928, 9.6830, 9.9054, 10.0, 10.0104, 10.1106, 10.2, 10.2344, 10.39, 10.5964, 11.0]     # as test_refocus_stack_gpu.py
SCALES = (2, 3, 4, 8)
# F64_BOUNDS of test_any_size_gpu.py; conf: a flip share of at most 2e-3, depth on the samples without a flip
F64_BOUNDS = dict(image=1e-4, shpd=1e-4, refoc=1e-4, bndry=1e-5, depth=1e-5, conf=1e-6)
F64_STACK = 1e-4


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
    """Both bindings of the new entries: torch.ops.be.* (the default) and the ctypes prototypes."""
    n = env["native"]
    assert n.ops() is not None
    if request.param == "ctypes":
        monkeypatch.setattr(n, "_ops", False)
        assert n.ops() is None
    return request.param


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_SCENES = {}


def _scene(env, kind, densify):
    """kind 'g6': the uniform 64 x 64 grid on the g6 inputs (147 x 147); 'flush': the 91 x 122 flush-edge grid of a 200 x 262 pair with
    the any_200x262 parameters.  -> dict(H, W, rec, grid keywords of the *_at wrappers, opts, w, ys, xs as lists)."""
    key = (kind, densify)
    if key not in _SCENES:
        n = env["native"]
        opts, w = env["helper"].render_opts(wrap_angles=False), densify == "w"
        if kind == "g6":
            H = W = 147
            img = T(synth.synthetic_image_pair(147, 147)[0]).to(DEV)
            p12 = T(synth.plausible_params12(4096, name="g6_est")).to(DEV)
            rec, _ = n.render_full(opts, env["dcal"].consts, 10.39, w, p12, n.view_image_pair(img, 2), pixels=img)
            ys = xs = list(range(0, 147 - R + 1, 2))
            grid = dict(hp=64, wp=64, stride=2)
        else:
            H, W = 200, 262
            img = T(synth.synthetic_image_pair(H, W, nshape=8)[0]).to(DEV)
            ys, xs = tiling.patch_grid(H, 2), tiling.patch_grid(W, 2)
            assert (len(ys), len(xs)) == (91, 122) and ys[-2:] == [178, 179] and xs[-2:] == [240, 241]
            est = T(synth.plausible_params12(len(ys) * len(xs), name="any_200x262")).to(DEV)
            rec = n.render_full_grid(opts, env["dcal"].consts, 10.39, w, est, img, ys, xs)
            grid = dict(ys=n.origin_table(ys, H, DEV, cover=True), xs=n.origin_table(xs, W, DEV, cover=True))
        _SCENES[key] = dict(H=H, W=W, rec=rec, grid=grid, opts=opts, w=w, ys=ys, xs=xs, kind=kind)
    return _SCENES[key]


def _pixel_fold(env, sc, want=MAPS):
    n = env["native"]
    if sc["kind"] == "g6":
        return n.fold_records(sc["opts"], sc["rec"], 64, 64, 147, 147, 2, sc["w"], want=want)
    return n.fold_records_grid(sc["opts"], sc["rec"], sc["H"], sc["W"], sc["ys"], sc["xs"], sc["w"], want=want)


def _pixel_stack(env, sc, rhos):
    return env["native"].fold_refocus_stack(sc["opts"], env["dcal"].consts, sc["rec"], rhos, sc["H"], sc["W"], **sc["grid"])


def _at(env, sc, scale=1, window=None, want=MAPS):
    return env["native"].fold_records_at(sc["opts"], sc["rec"], sc["H"], sc["W"], scale=scale, window=window, densify_w=sc["w"], want=want,
                                         **sc["grid"])


def _stack_at(env, sc, rhos, scale=1, window=None):
    return env["native"].fold_refocus_stack_at(sc["opts"], env["dcal"].consts, sc["rec"], rhos, sc["H"], sc["W"], scale=scale, window=window,
                                               **sc["grid"])


# ------------------------------------------------------------------------------------------ 1. scale 1 == the pixel kernels
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_scale_1_equals_the_pixel_folds_bit_for_bit(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    ref, got = _pixel_fold(env, sc), _at(env, sc)
    assert set(got) == set(MAPS)
    for k in MAPS:
        assert got[k].is_contiguous() and _same_bits(got[k], ref[k]), k
    one = _at(env, sc, want=("bndry", "conf"))                           # every map is optional
    assert set(one) == {"bndry", "conf"} and _same_bits(one["bndry"], ref["bndry"]) and _same_bits(one["conf"], ref["conf"])
    st = _stack_at(env, sc, RHO)
    assert st.shape == (len(RHO), 3, sc["H"], sc["W"]) and _same_bits(st, _pixel_stack(env, sc, RHO))
    if kind == "g6":                                                    # uniform tables == the table-free call
        uni = list(range(0, 147 - R + 1, 2))
        tab = env["native"].fold_records_at(sc["opts"], sc["rec"], 147, 147, scale=3, ys=uni, xs=uni, densify_w=sc["w"])
        fine = _at(env, sc, 3)
        for k in MAPS:
            assert _same_bits(tab[k], fine[k]), k


# ------------------------------------------------------------------------------------------ 2. every k-th sample is a pixel
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_every_kth_sample_is_the_pixel_map(env, binding, kind, densify):
    sc = _scene(env, kind, densify)
    ref, ref_stack = _pixel_fold(env, sc), _pixel_stack(env, sc, RHO)
    for k in SCALES:
        got = _at(env, sc, k)
        Ho, Wo = (sc["H"] - 1) * k + 1, (sc["W"] - 1) * k + 1
        for m in MAPS:
            assert got[m].shape[-2:] == (Ho, Wo), (k, m)
            assert torch.isfinite(got[m]).all(), (k, m)
            assert _same_bits(got[m][..., ::k, ::k], ref[m]), (k, m)
        assert not torch.equal(got["bndry"][1::k, 1::k][:sc["H"] - 1, :sc["W"] - 1], ref["bndry"][:-1, :-1])   # the rest is new
        rhos = RHO if k <= 3 else RHO[:9]                                # 9 = one full chunk and a short one
        st = _stack_at(env, sc, rhos, k)
        assert st.shape == (len(rhos), 3, Ho, Wo) and torch.isfinite(st).all()
        assert _same_bits(st[..., ::k, ::k], ref_stack[:len(rhos)]), k


# ------------------------------------------------------------------------------------------ 3. windows
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_windows_are_slices_of_the_full_lattice(env, binding, kind):
    sc = _scene(env, kind, None)
    H, W = sc["H"], sc["W"]
    wins = [(0, 0, H, W), (13, 29, 40, 57), (H - 23, W - 31, 23, 31), (H - 1, W - 1, 1, 1), (50, 0, 1, W), (0, W - 1, H, 1),
            (H - 17, 5, 17, 18), (31, 47, 2, 2)]
    for k in (1, 3, 4):
        full, full_stack = _at(env, sc, k), _stack_at(env, sc, RHO[:3], k)
        for t, l, h, w in wins:
            got = _at(env, sc, k, (t, l, h, w))
            sl = (Ellipsis, slice(t * k, (t + h - 1) * k + 1), slice(l * k, (l + w - 1) * k + 1))
            for m in MAPS:
                assert got[m].shape[-2:] == ((h - 1) * k + 1, (w - 1) * k + 1), (k, (t, l, h, w), m)
                assert _same_bits(got[m], full[m][sl]), (k, (t, l, h, w), m)
            assert _same_bits(_stack_at(env, sc, RHO[:3], k, (t, l, h, w)), full_stack[sl]), (k, (t, l, h, w))


def test_lattice_sample_under_no_patch_is_zero_over_zero(env, binding):
    """A uniform grid that stops short of the edge: 150 x 150 under the 64 x 64 stride-2 grid, which ends at pixel 146.  A lattice
    sample in (146, 149] is inside the window and under no patch - the pixel fold's 0/0 - and every k-th sample of a window that
    reaches the edge is still the pixel fold's, NaN bits included; the six maps and the stack (K = 9: a short last chunk)."""
    n = env["native"]
    sc = _scene(env, "g6", None)
    opts, consts, rec, uni = sc["opts"], env["dcal"].consts, sc["rec"], dict(hp=64, wp=64, stride=2)
    ref = n.fold_records(opts, rec, 64, 64, 150, 150, 2, False)
    ref_stack = n.fold_refocus_stack(opts, consts, rec, RHO[:9], 150, 150, **uni)
    assert torch.isnan(ref["bndry"][147:]).all() and torch.isnan(ref_stack[..., 147:, :]).all()
    assert torch.isfinite(ref["bndry"][:147, :147]).all() and torch.isfinite(ref_stack[..., :147, :147]).all()
    top, left, h, w = 131, 127, 19, 23
    sl = (Ellipsis, slice(top, top + h), slice(left, left + w))
    for k in (1, 3):
        got = n.fold_records_at(opts, rec, 150, 150, scale=k, window=(top, left, h, w), **uni)
        st = n.fold_refocus_stack_at(opts, consts, rec, RHO[:9], 150, 150, scale=k, window=(top, left, h, w), **uni)
        for m in MAPS:
            assert _same_bits(got[m][..., ::k, ::k], ref[m][sl]), (k, m)
        assert _same_bits(st[..., ::k, ::k], ref_stack[sl]), k
        ey, ex = (146 - top) * k, (146 - left) * k                      # the samples on pixel 146: the last ones under a patch
        for m in ("image", "shpd", "refoc", "bndry", "conf"):
            assert torch.isnan(got[m][..., ey + 1:, :]).all() and torch.isnan(got[m][..., :, ex + 1:]).all(), (k, m)
            assert torch.isfinite(got[m][..., :ey + 1, :ex + 1]).all(), (k, m)
        assert (got["depth"][ey + 1:] == 0).all() and (got["depth"][:, ex + 1:] == 0).all()     # depth divides by max(cntz, 1)
        assert torch.isnan(st[..., ey + 1:, :]).all() and torch.isnan(st[..., :, ex + 1:]).all(), k
        assert torch.isfinite(st[..., :ey + 1, :ex + 1]).all(), k


# ------------------------------------------------------------------------------------------ 4. against float64
@pytest.mark.parametrize("densify", [None, "w"])
@pytest.mark.parametrize("kind,k", [("g6", 3), ("flush", 2)])
def test_lattice_against_the_float64_restatement(env, kind, k, densify):
    """Measured on the MI355X, relmax against the helper in float64 (densify None / 'w'): profiles/HISTORY.md round 12."""
    from oracle import depth as od
    sc = _scene(env, kind, densify)
    got = {m: v.double().cpu().numpy() for m, v in _at(env, sc, k).items()}
    rhos = [RHO[0], RHO[8], RHO[10]]
    stack = _stack_at(env, sc, rhos, k).double().cpu().numpy()
    want = rao.fold_at(sc["rec"].cpu().numpy(), sc["ys"], sc["xs"], sc["H"], sc["W"], k, None, np.float64, densify_w=sc["w"],
                       rho_primes=rhos, consts=od.depth_consts())
    assert int(want["count"].min()) >= 1
    err = {m: relmax(got[m], want[m]) for m in MAPS}
    flips = np.abs(got["conf"] - want["conf"]) > 1e-6
    share = float(flips.mean())
    serr = [relmax(stack[p], want["stack"][p]) for p in range(len(rhos))]
    print(f"\nrender_at {kind} scale {k} densify={densify}: relmax vs float64 " + "  ".join(f"{m} {err[m]:.2e}" for m in MAPS)
          + f"  conf flip share {share:.2e} of {flips.size}  stack " + " ".join(f"{e:.2e}" for e in serr))
    for m in MAPS:
        assert np.isfinite(got[m]).all(), m
    for m in ("image", "shpd", "refoc", "bndry"):
        assert err[m] <= F64_BOUNDS[m], (m, err[m])
    if err["conf"] > F64_BOUNDS["conf"]:
        assert share <= 2e-3, share
        ok = ~flips
        assert relmax(got["depth"][ok], want["depth"][ok]) <= F64_BOUNDS["depth"]
    else:
        assert err["depth"] <= F64_BOUNDS["depth"], err["depth"]
    for e in serr:
        assert e <= F64_STACK, serr


# ------------------------------------------------------------------------------------------ 5. stack consistency
@pytest.mark.parametrize("kind", ["g6", "flush"])
def test_stack_plane_equals_the_fold_of_records_rendered_at_that_power(env, binding, kind):
    n = env["native"]
    sc = _scene(env, kind, None)
    st = _stack_at(env, sc, RHO, 4)
    for p, rho in enumerate(RHO):
        if kind == "g6":
            img = T(synth.synthetic_image_pair(147, 147)[0]).to(DEV)
            p12 = T(synth.plausible_params12(4096, name="g6_est")).to(DEV)
            rec, _ = n.render_full(sc["opts"], env["dcal"].consts, rho, False, p12, n.view_image_pair(img, 2), pixels=img)
        else:
            img = T(synth.synthetic_image_pair(200, 262, nshape=8)[0]).to(DEV)
            est = T(synth.plausible_params12(91 * 122, name="any_200x262")).to(DEV)
            rec = n.render_full_grid(sc["opts"], env["dcal"].consts, rho, False, est, img, sc["ys"], sc["xs"])
        ref = n.fold_records_at(sc["opts"], rec, sc["H"], sc["W"], scale=4, want=("refoc",), **sc["grid"])["refoc"]
        assert _same_bits(st[p], ref), (p, rho)
    assert not torch.equal(st[0], st[-1])


# ------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("entry,H,W", [("__call__", 147, 147), ("run_big", 235, 323), ("run_any", 200, 262)])
def test_pipeline_render_at(pipe, entry, H, W):
    img = T(synth.synthetic_image_pair(H, W, nshape=8)[0]).to(DEV)
    run = pipe if entry == "__call__" else getattr(pipe, entry)
    maps = run(img)
    keys = set(maps)
    for k in (1, 2, 3):
        fine = pipe.render_at(maps, scale=k)
        Ho, Wo = (H - 1) * k + 1, (W - 1) * k + 1
        assert set(fine) == set(MAPS) | {"depth_map", "lattice"}
        assert fine["lattice"] == dict(scale=k, window=(0, 0, H, W), Ho=Ho, Wo=Wo)
        for m in MAPS:
            assert fine[m].shape[-2:] == (Ho, Wo) and fine[m].dtype == torch.float32, (k, m)
            assert torch.isfinite(fine[m]).all(), (k, m)                # all three grids end on the last pixel: no 0/0
            assert _same_bits(fine[m][..., ::k, ::k], maps[m]), (k, m)
    # depth_map: self.depth_thres by default (__call__'s threshold); run_big / run_any use 0.05
    thres = pipe.depth_thres if entry == "__call__" else 0.05
    fine = pipe.render_at(maps, scale=2, depth_thres=thres)
    assert _same_bits(fine["depth_map"][::2, ::2], maps["depth_map"])
    assert _same_bits(fine["depth_map"], torch.where(fine["conf"] > thres, fine["depth"], torch.zeros_like(fine["depth"])))
    # a window, chosen maps
    win = (H - 30, W - 41, 30, 41)
    part = pipe.render_at(maps, scale=4, window=win, want=("bndry", "refoc"))
    assert set(part) == {"bndry", "refoc", "depth_map", "lattice"} and part["lattice"]["window"] == win
    assert part["bndry"].shape == (117, 161) and _same_bits(part["bndry"][::4, ::4], maps["bndry"][H - 30:, W - 41:])
    # the focal stack on the same lattice; the defaults are today's call
    rhos = [pipe.rho_prime, 9.9054, 10.5964]
    st1 = pipe.refocus_stack(maps, rho_primes=rhos)
    assert st1.shape == (3, 3, H, W) and torch.equal(st1[0], maps["refoc"])
    st = pipe.refocus_stack(maps, rho_primes=rhos, scale=3)
    assert st.shape == (3, 3, (H - 1) * 3 + 1, (W - 1) * 3 + 1) and torch.isfinite(st).all()
    assert _same_bits(st[..., ::3, ::3], st1)
    stw = pipe.refocus_stack(maps, focus_depths=[0.751, 1.0], scale=2, window=win)
    assert stw.shape == (2, 3, 59, 81)
    assert _same_bits(stw[..., ::2, ::2], pipe.refocus_stack(maps, focus_depths=[0.751, 1.0])[..., H - 30:, W - 41:])
    # nothing the entry point returns has changed: a second call gives the same keys and the same bits
    again = run(img)
    assert set(again) == keys == set(maps)
    for k, v in maps.items():
        if k != "grid":
            assert _same_bits(v, again[k]), k
    # the error cases, with a live pipeline
    with pytest.raises(ValueError, match="scale"):
        pipe.render_at(maps, scale=0)
    with pytest.raises(ValueError, match="scale"):
        pipe.render_at(maps, scale=17)
    with pytest.raises(ValueError, match="window"):
        pipe.render_at(maps, scale=2, window=(0, 0, H + 1, W))
    with pytest.raises(ValueError, match="records"):
        pipe.render_at({k: v for k, v in maps.items() if k != "records"}, scale=2)
    with pytest.raises(ValueError, match="GPU"):
        pipe.render_at(dict(maps, records=maps["records"].cpu()), scale=2)
    with pytest.raises(ValueError, match="unknown maps"):
        pipe.render_at(maps, want=("depth_map",))
    with pytest.raises(ValueError, match="scale"):
        pipe.refocus_stack(maps, rho_primes=rhos, scale=17)


def test_render_at_without_depth_map_under_densify_pp(pipe, env):
    """densify == 'pp': the U-Net is not defined off its native resolution, so there is no depth_map key."""
    import models
    from be_hip.pipeline import DepthPipeline
    unet = models.DepthCompletion()
    unet.load_state_dict({k: T(v) if v.dtype != np.int64 else torch.from_numpy(np.asarray(v)) for k, v in synth.unet_state_dict().items()})
    pp = DepthPipeline(pipe.local, pipe.globl, env["helper"], env["dcal"], densify="pp", densify_pp_module=unet.to(DEV).eval())
    img = T(synth.synthetic_image_pair(147, 147, nshape=8)[0]).to(DEV)
    maps = pp(img)
    fine = pp.render_at(maps, scale=2)
    assert set(fine) == set(MAPS) | {"lattice"}
    assert _same_bits(fine["depth"][::2, ::2], maps["depth"])


# ------------------------------------------------------------------------------------------ 7. the workflow flag
def test_workflow_eval_render_scale_on_generated_pairs(tmp_path):
    """Two datagen_test pairs through `workflow eval --render_scale 3` with the shipped checkpoints, plain and --any: one npz per pair
    whose arrays are DepthPipeline.render_at called directly; with --refocus_stack the stack is on the same lattice; a window; and no
    file when the flag is absent."""
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
    K = 3
    sweep = wf.focus_sweep(pipe.dcal, K, 0.75, 1.18)
    common = ["--model_path", ckpt, "--data_path", str(data_dir), "--cuda", DEV]
    for mode in ((), ("--any",)):
        out = tmp_path / ("fine" + "".join(mode))
        res = wf.main(["eval", *mode, "--render_scale", "3", "--refocus_stack", str(K), "--out_path", str(out), *common])
        assert set(res) == {"delta1", "delta2", "delta3", "RMSE", "AbsRel", "seconds_per_pair"}
        for j in range(2):
            got = dict(np.load(out / f"render_x3_{j:04d}.npz"))
            assert set(got) == set(names)
            img = ds[j][0].permute(0, 3, 1, 2).contiguous()
            maps = pipe.run_any(img) if mode else pipe(img)
            want = pipe.render_at(maps, scale=3, depth_thres=0.05 if mode else None)
            for k in names:
                assert got[k].dtype == np.float32 and got[k].shape[-2:] == (439, 439) and np.isfinite(got[k]).all(), (mode, j, k)
                assert np.array_equal(got[k], want[k].cpu().numpy()), (mode, j, k)
            assert np.array_equal(got["depth_map"][::3, ::3], maps["depth_map"].cpu().numpy())
            stack = np.load(out / f"refoc_stack_{j:04d}.npy")
            assert stack.shape == (K, 3, 439, 439)
            assert np.array_equal(stack, pipe.refocus_stack(maps, rho_primes=sweep.tolist(), scale=3).cpu().numpy())
    # a window at scale 1 is written too
    out = tmp_path / "win"
    wf.main(["eval", "--render_window", "100", "90", "47", "57", "--out_path", str(out), *common])
    got = dict(np.load(out / "render_x1_0000.npz"))
    maps = pipe(ds[0][0].permute(0, 3, 1, 2).contiguous())
    assert got["bndry"].shape == (47, 57) and np.array_equal(got["bndry"], maps["bndry"][100:, 90:].cpu().numpy())
    # off by default: no file is written
    out = tmp_path / "none"
    wf.main(["eval", "--out_path", str(out), *common])
    assert not out.exists()
    out = tmp_path / "one"
    wf.main(["eval", "--render_scale", "1", "--out_path", str(out), *common])
    assert not out.exists()
