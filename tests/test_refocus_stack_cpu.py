"""CPU-side tests of the focal stack: DepthEtas.focus2rho, the reference fixture g20 against the float64 oracle, and every check
DepthPipeline.refocus_stack / native.fold_refocus_stack / `workflow eval --refocus_stack` make on the host before native code runs."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, relmax
from be_hip import synth

RHO_G20 = (9.4928, 10.1106, 10.5964)          # focus at 2.30, 0.95, 0.65 m (tests/golden/make_golden_refocus.py)


def T(a, dt=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dt)


def _dcal():
    import utils
    return utils.DepthEtas(utils.get_args("eval", argv=[]), "cpu")


def test_focus2rho_is_the_zero_of_depth2sigma():
    from oracle import depth as od
    dcal, c = _dcal(), od.depth_consts()
    for z in (0.65, 0.75, 0.95, 1.18, 2.3):
        rho = dcal.focus2rho(z)
        assert isinstance(rho, float)
        assert float(od.depth2sigma(c, torch.tensor(z, dtype=torch.float64), rho)) <= 1e-6
        assert float(dcal.depth2sigma(torch.tensor(z, dtype=torch.float64), rho)) <= 1e-6
    assert round(dcal.focus2rho(0.751), 2) == 10.39                                 # the reference's default power
    for z, rho in zip((2.30, 0.95, 0.65), RHO_G20):
        assert abs(dcal.focus2rho(z) - rho) <= 5e-5                                 # the fixture's powers, four decimals
    zs = torch.tensor([0.65, 0.95, 2.3], dtype=torch.float64)
    r = dcal.focus2rho(zs)
    assert isinstance(r, torch.Tensor) and r.shape == zs.shape and r.dtype == zs.dtype
    assert torch.equal(r, torch.tensor([dcal.focus2rho(float(z)) for z in zs], dtype=torch.float64))
    assert float(od.depth2sigma(c, zs, r).max()) <= 1e-6
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError):
            dcal.focus2rho(bad)
    with pytest.raises(ValueError):
        dcal.focus2rho(torch.tensor([0.9, 0.0]))


def test_g20_fixture_is_what_the_float64_oracle_says():
    """The three reference planes against fold_mean(render_pass_b(float64, rho_prime)): ties the fixture to the restatement the GPU
    test holds every plane of the stack to.  float32 storage rounds at 6e-8."""
    from oracle import render as orr, depth as od, tiling as ot
    g = load_golden("g20_refocus_stack")
    assert g["fold_refoc"].shape == (3, 3, 147, 147) and g["sub_refoc"].shape == (3, 3, 21, 21, 4, 4)
    assert np.allclose(g["rho_primes"], RHO_G20, rtol=0, atol=1e-6)
    imgs, _ = synth.synthetic_image_pair(147, 147)
    pat = ot.unfold_patches(T(imgs)).double()
    p12 = T(synth.plausible_params12(4096, name="g6_est")).double()
    ii, jj = np.meshgrid(np.arange(20, 24), np.arange(30, 34), indexing="ij")
    sel = (ii * 64 + jj).ravel()
    for k, rho in enumerate(RHO_G20):
        r = orr.render_pass_b(od.depth_consts(), p12, pat[0], pat[1], rho_prime=rho)
        e = relmax(ot.fold_mean(r["refoc"][None], 147, 147)[0], g["fold_refoc"][k])
        a = g["sub_refoc"][k]
        es = relmax(r["refoc"][sel], np.moveaxis(a.reshape(a.shape[:-2] + (16,)), -1, 0))
        print(f"\ng20 plane {k} (rho' = {rho}): folded relmax {e:.2e}, 4x4 sub-grid relmax {es:.2e}")
        assert e <= 2e-7 and es <= 2e-7
    # the three planes are three different images
    assert relmax(g["fold_refoc"][0], g["fold_refoc"][2]) > 1e-2


def test_refocus_stack_host_checks():
    from be_hip.pipeline import DepthPipeline
    pipe = DepthPipeline(None, None, None, _dcal())
    rec = torch.zeros(4096, 32)
    grid = dict(H=147, W=147, hp=64, wp=64, stride=2, ys=None, xs=None)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.refocus_stack(dict(records=rec, grid=grid))
    with pytest.raises(ValueError, match="exactly one"):
        pipe.refocus_stack(dict(records=rec, grid=grid), rho_primes=[10.39], focus_depths=[0.751])
    with pytest.raises(ValueError, match="records"):
        pipe.refocus_stack(dict(grid=grid), rho_primes=[10.39])
    with pytest.raises(ValueError, match="grid"):
        pipe.refocus_stack(dict(records=rec), rho_primes=[10.39])
    with pytest.raises(ValueError, match="GPU"):
        pipe.refocus_stack(dict(records=rec, grid=grid), rho_primes=[10.39])        # CPU tensors: nothing computes on the CPU
    with pytest.raises(ValueError, match="GPU"):
        pipe.refocus_stack(dict(records=rec, grid=grid), focus_depths=[0.751])


def test_native_fold_refocus_stack_checks_the_powers_before_the_library(monkeypatch):
    from be_hip import native

    def no_lib():
        raise AssertionError("the library was touched before rho_primes was checked")
    monkeypatch.setattr(native, "lib", no_lib)
    monkeypatch.setattr(native, "ops", no_lib)
    opts, consts, rec = native.RenderOpts(), native.DepthConsts(), torch.zeros(4096, 32)
    for bad in ([], torch.zeros(0), [10.0, float("nan")], [float("inf")], torch.tensor([10.0, float("-inf")]), torch.zeros(2, 2)):
        with pytest.raises(ValueError, match="rho_primes"):
            native.fold_refocus_stack(opts, consts, rec, bad, 147, 147, hp=64, wp=64)
    with pytest.raises(ValueError, match="both"):
        native.fold_refocus_stack(opts, consts, rec, [10.39], 147, 147, ys=list(range(0, 127, 2)))
    with pytest.raises(RuntimeError, match=r"\[4096,32\]"):
        native.fold_refocus_stack(opts, consts, rec[:100], [10.39], 147, 147, hp=64, wp=64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        native.fold_refocus_stack(opts, consts, rec, [10.39], 147, 147, hp=64, wp=64)


def test_entry_point_is_declared_exported_and_registered():
    from be_hip import native
    from be_hip.pipeline import DepthPipeline
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_fold_refocus_stack_f32", "be_refocus_stack_chunk"):
        assert name in declared and name in native.EXPORTED and hasattr(lib, name), name
    assert lib.be_refocus_stack_chunk() == native.REFOCUS_STACK_KC >= 1
    assert int(re.search(r"#define BE_REFOCUS_STACK_KC (\d+)", hdr).group(1)) == native.REFOCUS_STACK_KC
    o = native.ops()
    assert o is not None and hasattr(o, "fold_refocus_stack")
    assert "Tensor rho_primes, Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride" in str(
        torch.ops.be.fold_refocus_stack.default._schema)
    assert callable(native.fold_refocus_stack) and hasattr(DepthPipeline, "refocus_stack")
    # host-side argument checks of the library fail before any launch (no GPU needed)
    ro, dc = native.RenderOpts(), native.DepthConsts()
    one = native.C.c_void_p(16)                                                     # a non-null, 16-byte aligned address; never read
    args = lambda **kw: [kw.get(k, d) for k, d in (("o", ro), ("dc", dc), ("rec", one), ("hp", 64), ("wp", 64), ("H", 147), ("W", 147),
                                                   ("stride", 2), ("ys", None), ("xs", None), ("rho", one), ("K", 1), ("out", one),
                                                   ("stream", None))]
    for kw, msg in ((dict(rec=None), b"null pointer"), (dict(rho=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(K=0), b"K must be"), (dict(rec=native.C.c_void_p(20)), b"16-byte aligned"),
                    (dict(ys=one), b"both"), (dict(xs=one), b"both"), (dict(hp=65), b"exceeds the image")):
        assert lib.be_fold_refocus_stack_f32(*args(**kw)) != 0, kw
        assert msg in lib.be_last_error(), (kw, lib.be_last_error())


def test_workflow_power_spacing_and_arguments():
    import utils
    from be_hip import workflow as wf
    a = utils.get_args("eval", argv=[])
    assert a.refocus_stack == 0 and a.focus_range == [0.75, 1.18] and isinstance(a.out_path, str)      # off by default
    a = utils.get_args("eval", big=True, argv=["--refocus_stack", "5", "--focus_range", "0.75", "1.18", "--out_path", "x"])
    assert (a.refocus_stack, a.focus_range, a.out_path) == (5, [0.75, 1.18], "x")
    dcal = _dcal()
    rho = wf.focus_sweep(dcal, a.refocus_stack, *a.focus_range)
    assert rho.shape == (5,) and rho.dtype == np.float64
    assert rho[0] == dcal.focus2rho(1.18) and rho[-1] == dcal.focus2rho(0.75)                          # far first: powers ascend
    steps = np.diff(rho)
    assert (steps > 0).all() and np.allclose(steps, steps[0], rtol=1e-12, atol=0)
    assert np.allclose(steps[0], (1 / 0.75 - 1 / 1.18) / 4, rtol=1e-12)
    assert wf.focus_sweep(dcal, 1, 0.75, 1.18).tolist() == [dcal.focus2rho(1.18)]
    for bad in ((0, 0.75, 1.18), (3, 1.18, 0.75), (3, 0.0, 1.0)):
        with pytest.raises(ValueError):
            wf.focus_sweep(dcal, *bad)
