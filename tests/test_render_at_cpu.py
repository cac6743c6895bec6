"""CPU-side tests of DepthPipeline.render_at: the sampling lattice (be_hip.tiling), the numpy restatement the GPU tests compare
against (tests/render_at_oracle.py) tied to the pinned oracle, and every check native.fold_records_at /
native.fold_refocus_stack_at / the two C entries / `workflow eval --render_scale` make on the host before a kernel is launched."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, relmax
from be_hip import synth, tiling
import render_at_oracle as rao

R = 21


def T(a, dt=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dt)


# ---------------------------------------------------------------------------------------------- lattice arithmetic
def test_lattice_sizes_and_checks():
    assert tiling.lattice(147, 147) == dict(scale=1, window=(0, 0, 147, 147), Ho=147, Wo=147)
    assert tiling.lattice(147, 200, 4) == dict(scale=4, window=(0, 0, 147, 200), Ho=585, Wo=797)
    assert tiling.lattice(147, 200, 3, (5, 7, 1, 10)) == dict(scale=3, window=(5, 7, 1, 10), Ho=1, Wo=28)
    assert tiling.lattice(147, 200, 16, (146, 199, 1, 1)) == dict(scale=16, window=(146, 199, 1, 1), Ho=1, Wo=1)
    for bad in (0, 17, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError, match="scale"):
            tiling.lattice(147, 147, bad)
    for bad in ((0, 0, 148, 147), (0, 0, 147, 148), (-1, 0, 10, 10), (0, -1, 10, 10), (140, 0, 8, 10), (0, 140, 10, 8), (0, 0, 0, 10),
                (0, 0, 10, 0), (0, 0, 10), (0.5, 0, 10, 10), "abcd"):
        with pytest.raises(ValueError, match="window"):
            tiling.lattice(147, 147, 2, bad)


def _pixel_run_uniform(y, s, n):
    """The pixel fold on a uniform grid (k_fold_pixels<.., false>): the run of grid lines covering integer pixel y."""
    lo = (y - (R - 1) + s - 1) // s if y - (R - 1) >= 0 else 0
    return lo, min(y // s, n - 1)


def _pixel_run_tables(y, lines):
    """The pixel fold with origin tables (k_fold_pixels<.., true>): the same from an origin table."""
    lo = 0
    while lo < len(lines) and lines[lo] < y - (R - 1):
        lo += 1
    hi = lo - 1
    while hi + 1 < len(lines) and lines[hi + 1] <= y:
        hi += 1
    return lo, hi


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_every_kth_sample_has_the_integer_pixel_run(k):
    for size, s in ((147, 1), (147, 2), (150, 2)):                      # 150: the uniform stride-2 grid stops one pixel short
        n = (size - R) // s + 1
        origins = [s * i for i in range(n)]
        Ho = (size - 1) * k + 1
        runs = tiling.lattice_runs(origins, Ho, k)
        for iy, (lo, hi, pos) in enumerate(runs):
            if hi >= lo:
                assert (lo, hi) == tiling.uniform_run(iy, k, s, n)
                assert all(0 <= q * k + r <= (R - 1) * k and (q < R - 1 or r == 0) for q, r in pos)
                assert len({r for _, r in pos}) == 1 and pos[0][1] == iy % k         # one remainder for all covering lines
            if iy % k == 0:
                plo, phi = _pixel_run_uniform(iy // k, s, n)
                assert (lo, hi) == (plo, phi) if hi >= lo else phi < plo, (size, s, iy)      # an empty run is empty in both
                assert [q for q, _ in pos] == [iy // k - origins[i] for i in range(lo, hi + 1)]
        uncovered = [iy for iy, (lo, hi, _) in enumerate(runs) if hi < lo]
        assert uncovered == ([] if size != 150 else list(range(148 * k + 1, Ho)))   # past the last patch's last pixel centre
    for size in (200, 262):                                             # flush-edge tables
        lines = tiling.patch_grid(size, 2)
        assert lines[-1] == size - R and lines[-1] - lines[-2] == 1
        runs = tiling.lattice_runs(lines, (size - 1) * k + 1, k)
        for iy, (lo, hi, pos) in enumerate(runs):
            assert hi >= lo, (size, iy)                                 # a covering grid leaves no sample uncovered
            assert all(lines[i] * k <= iy <= (lines[i] + R - 1) * k for i in range(lo, hi + 1))
            assert lo == 0 or lines[lo - 1] * k + (R - 1) * k < iy
            assert hi == len(lines) - 1 or lines[hi + 1] * k > iy
            assert hi - lo + 1 <= R
            if iy % k == 0:
                assert (lo, hi) == _pixel_run_tables(iy // k, lines), (size, iy)
        # the lines a 16-sample tile needs fit the 36 slots the kernel stages
        for Y0 in range(0, (size - 1) * k + 1, 16):
            need = {i for lo, hi, _ in runs[Y0:Y0 + 16] for i in range(lo, hi + 1)}
            first = Y0 // k + (1 if Y0 % k else 0) - (R - 1)
            i0 = next(i for i, o in enumerate(lines) if o >= first)
            assert min(need) >= i0 and max(need) - i0 < 16 + R - 1, (size, k, Y0)


def test_windows_are_slices_of_the_full_lattice():
    lines = tiling.patch_grid(200, 2)
    for k in (1, 3, 4):
        full = tiling.lattice_runs(lines, 199 * k + 1, k)
        for top, h in ((0, 200), (17, 30), (199, 1), (180, 20), (50, 1)):
            lat = tiling.lattice(200, 262, k, (top, 0, h, 262))
            assert lat["Ho"] == (h - 1) * k + 1
            assert tiling.lattice_runs(lines, lat["Ho"], k, first=top) == full[top * k: top * k + lat["Ho"]]


# ---------------------------------------------------------------------------------------------- the helper against the oracle
def g6_records64(densify=None, rho_prime=10.39):
    """A float64 [4096,32] record array on the g6 inputs from the pieces of oracle.render.render_pass_b, and that pass's output."""
    from oracle import render as orr, depth as od, tiling as ot
    imgs, _ = synth.synthetic_image_pair(147, 147)
    pat = ot.unfold_patches(T(imgs)).double()
    p12 = T(synth.plausible_params12(4096, name="g6_est")).double()
    r = orr.render_pass_b(od.depth_consts(), p12, pat[0], pat[1], rho_prime=rho_prime, densify=densify)
    t1, f1, t2, f2 = (p12[:, i] for i in range(4, 8))
    sg = lambda f: torch.where(torch.remainder(f, 2 * math.pi) < math.pi, torch.ones_like(f), -torch.ones_like(f))
    root2 = torch.sqrt(torch.tensor(2)).double()
    m = r["depth_mask"]
    flags = ((m == 1).sum(dim=(1, 2)) > 0).double() + 2 * ((m == 2).sum(dim=(1, 2)) > 0).double()
    rec = torch.cat([p12[:, :4], torch.stack([torch.sin(t1), torch.cos(t1), torch.sin(t1 + f1), torch.cos(t1 + f1), torch.sin(t2),
                                              torch.cos(t2), torch.sin(t2 + f2), torch.cos(t2 + f2), sg(f1), sg(f2)], dim=1),
                     root2 * r["etas"], root2 * r["sig_refoc"], r["colors"].reshape(-1, 9), r["depth1"][:, None], r["depth2"][:, None],
                     flags[:, None]], dim=1)
    assert rec.shape == (4096, 32)
    return rec.numpy(), r


@pytest.mark.parametrize("densify", [None, "w"])
def test_helper_at_scale_1_is_the_pinned_oracle_fold(densify):
    from oracle import tiling as ot
    rec, r = g6_records64(densify)
    uni = list(range(0, 147 - R + 1, 2))
    got = rao.fold_at(rec, uni, uni, 147, 147, 1, None, np.float64, densify_w=densify == "w")
    z, conf = ot.fold_depth(r["depth_map"][None], r["depth_mask"][None], 147, 147)
    want = dict(image=ot.fold_mean(torch.cat([r["patches1"], r["patches2"]], dim=1)[None], 147, 147)[0].view(2, 3, 147, 147),
                shpd=ot.fold_mean(r["shpd"][None], 147, 147)[0], refoc=ot.fold_mean(r["refoc"][None], 147, 147)[0],
                bndry=ot.fold_mean(r["boundary"][None, :, None], 147, 147)[0, 0], depth=z[0], conf=conf[0])
    assert int(got["count"].min()) >= 1 and int(got["count"].max()) == 121
    err = {k: relmax(got[k], want[k].numpy()) for k in rao.MAPS}
    print(f"\nhelper vs oracle fold, densify={densify}: " + "  ".join(f"{k} {e:.1e}" for k, e in err.items()))
    for k, e in err.items():
        assert got[k].shape == tuple(want[k].shape) and e <= 1e-12, (k, e)
    # the stack radii through oracle.depth.depth2sigma: the plane at the records' own power is their refoc map
    from oracle import depth as od
    st = rao.fold_at(rec, uni, uni, 147, 147, 1, (40, 50, 30, 30), np.float64, densify_w=densify == "w", rho_primes=[10.39, 9.4928],
                     consts=od.depth_consts(), want=("refoc",))
    assert relmax(st["stack"][0], st["refoc"]) <= 1e-12 and relmax(st["stack"][0], want["refoc"][:, 40:70, 50:80].numpy()) <= 1e-12
    assert relmax(st["stack"][1], st["refoc"]) > 1e-3


def test_conf_flip_share_between_float32_and_float64_helper_at_scale_3():
    """The cap the GPU test holds conf to (a depth-mask element on its threshold may flip between two evaluations; share <= 2e-3 of
    the samples, test_any_size_gpu.py) holds between the helper's own float32 and float64 runs, so the inputs sit inside it."""
    rec, _ = g6_records64(None)
    uni = list(range(0, 147 - R + 1, 2))
    a = rao.fold_at(rec, uni, uni, 147, 147, 3, None, np.float32, want=("bndry", "conf"))
    b = rao.fold_at(rec, uni, uni, 147, 147, 3, None, np.float64, want=("bndry", "conf"))
    assert a["conf"].dtype == np.float32 and a["conf"].shape == (439, 439) == b["conf"].shape
    share = float((np.abs(a["conf"].astype(np.float64) - b["conf"]) > 1e-6).mean())
    print(f"\nhelper float32 vs float64 at scale 3: conf flip share {share:.2e} of {a['conf'].size}, bndry relmax "
          f"{relmax(a['bndry'], b['bndry']):.2e}")
    assert share <= 2e-3
    assert np.array_equal(b["conf"][::3, ::3], rao.fold_at(rec, uni, uni, 147, 147, 1, None, np.float64, want=("conf",))["conf"])


# ---------------------------------------------------------------------------------------------- host checks
def test_native_wrappers_check_before_the_library(monkeypatch):
    from be_hip import native

    def no_lib():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(native, "lib", no_lib)
    monkeypatch.setattr(native, "ops", no_lib)
    opts, consts, rec = native.RenderOpts(), native.DepthConsts(), torch.zeros(4096, 32)
    uni = list(range(0, 127, 2))
    calls = (lambda **kw: native.fold_records_at(opts, kw.pop("rec", rec), 147, 147, **kw),
             lambda **kw: native.fold_refocus_stack_at(opts, consts, kw.pop("rec", rec), [10.39], 147, 147, **kw))
    for call in calls:
        for bad in (0, 17, 2.5):
            with pytest.raises(ValueError, match="scale"):
                call(scale=bad, hp=64, wp=64)
        for bad in ((0, 0, 148, 10), (140, 0, 10, 10), (0, 0, 0, 5), (-1, 0, 5, 5)):
            with pytest.raises(ValueError, match="window"):
                call(scale=2, window=bad, hp=64, wp=64)
        with pytest.raises(ValueError, match="both"):
            call(scale=2, ys=uni)
        with pytest.raises(ValueError, match="both"):
            call(scale=2, xs=uni)
        with pytest.raises(ValueError, match="cover"):
            call(scale=2, rec=rec[:63 * 64], ys=uni[:-1], xs=uni)
        with pytest.raises(RuntimeError, match=r"\[4096,32\]"):
            call(scale=2, rec=rec[:100], hp=64, wp=64)
        with pytest.raises(RuntimeError, match=r"\[P,32\]"):
            call(scale=2, rec=torch.zeros(64, 64, 32), hp=64, wp=64)
        with pytest.raises(RuntimeError, match="hp and wp"):
            call(scale=2)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(scale=2, hp=64, wp=64)                                 # CPU records
    with pytest.raises(ValueError, match="rho_primes"):
        native.fold_refocus_stack_at(opts, consts, rec, [], 147, 147, scale=2, hp=64, wp=64)


def test_pipeline_host_checks():
    import utils
    from be_hip.pipeline import DepthPipeline
    pipe = DepthPipeline(None, None, None, utils.DepthEtas(utils.get_args("eval", argv=[]), "cpu"))
    rec = torch.zeros(4096, 32)
    grid = dict(H=147, W=147, hp=64, wp=64, stride=2, ys=None, xs=None)
    maps = dict(records=rec, grid=grid)
    with pytest.raises(ValueError, match="records"):
        pipe.render_at(dict(grid=grid), scale=2)
    with pytest.raises(ValueError, match="grid"):
        pipe.render_at(dict(records=rec), scale=2)
    with pytest.raises(ValueError, match="scale"):
        pipe.render_at(maps, scale=17)
    with pytest.raises(ValueError, match="window"):
        pipe.render_at(maps, scale=2, window=(0, 0, 148, 147))
    with pytest.raises(ValueError, match="unknown maps"):
        pipe.render_at(maps, scale=2, want=("depth_map",))
    with pytest.raises(ValueError, match="GPU"):
        pipe.render_at(maps, scale=2)                                   # CPU records: nothing computes on the CPU
    with pytest.raises(ValueError, match="GPU"):
        pipe.refocus_stack(maps, rho_primes=[10.39], scale=2)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.refocus_stack(maps, scale=2)


def test_entries_are_declared_exported_bound_and_check_their_arguments():
    from be_hip import native
    from be_hip.pipeline import DepthPipeline
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_fold_records_at_f32", "be_fold_refocus_stack_at_f32"):
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    assert int(re.search(r"#define BE_RENDER_AT_MAX_SCALE (\d+)", hdr).group(1)) == tiling.MAX_SCALE == 16
    o = native.ops()
    assert o is not None and hasattr(o, "fold_records_at") and hasattr(o, "fold_refocus_stack_at")
    tail = "int hp, int wp, int H, int W, int stride, int scale, int top, int left, int h, int w"
    assert "Tensor? ys, Tensor? xs, " + tail + ", bool densify_w, int want" in str(torch.ops.be.fold_records_at.default._schema)
    assert "Tensor rho_primes, Tensor? ys, Tensor? xs, " + tail in str(torch.ops.be.fold_refocus_stack_at.default._schema)
    assert callable(native.fold_records_at) and callable(native.fold_refocus_stack_at) and hasattr(DepthPipeline, "render_at")
    # host-side argument checks of the library fail before any launch (no GPU needed)
    ro, dc = native.RenderOpts(), native.DepthConsts()
    one = native.C.c_void_p(16)                                         # a non-null, 16-byte aligned address; never read
    grid = (("hp", 64), ("wp", 64), ("H", 147), ("W", 147), ("stride", 2), ("ys", None), ("xs", None), ("scale", 2), ("top", 0),
            ("left", 0), ("h", 147), ("w", 147))
    fold = lambda **kw: [kw.get(k, d) for k, d in (("o", ro), ("rec", one)) + grid + (("densify_w", 0),) + tuple(
        (m, one) for m in native.FOLD_MAPS) + (("stream", None),)]
    stack = lambda **kw: [kw.get(k, d) for k, d in (("o", ro), ("dc", dc), ("rec", one)) + grid + (("rho", one), ("K", 1), ("out", one),
                                                                                                  ("stream", None))]
    shared = ((dict(rec=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(rec=native.C.c_void_p(20)), b"16-byte aligned"),
              (dict(scale=0), b"scale must be"), (dict(scale=17), b"scale must be"), (dict(ys=one), b"both"), (dict(xs=one), b"both"),
              (dict(hp=65), b"exceeds the image"), (dict(ys=one, xs=one, hp=128), b"HP / WP must be"),
              (dict(h=148), b"leaves the"), (dict(top=1), b"leaves the"), (dict(left=-1), b"leaves the"), (dict(w=0), b"leaves the"),
              (dict(H=2 ** 28, W=21, hp=1, wp=1, h=1, w=1, scale=16), b"too large"),
              (dict(H=70000, W=70000, hp=1, wp=1, h=70000, w=70000, scale=1), b"too large"))
    for fn, args, extra in ((lib.be_fold_records_at_f32, fold, ()),
                            (lib.be_fold_refocus_stack_at_f32, stack, ((dict(rho=None), b"null pointer"), (dict(out=None), b"null pointer"),
                                                                       (dict(dc=None), b"null pointer"), (dict(K=0), b"K must be")))):
        for kw, msg in shared + extra:
            assert fn(*args(**kw)) != 0, kw
            assert msg in lib.be_last_error(), (kw, lib.be_last_error())


def test_workflow_arguments():
    import utils
    a = utils.get_args("eval", argv=[])
    assert a.render_scale == 1 and a.render_window is None              # off by default
    a = utils.get_args("eval", big=True, argv=["--render_scale", "4", "--render_window", "10", "20", "30", "40", "--out_path", "x"])
    assert (a.render_scale, a.render_window, a.out_path) == (4, [10, 20, 30, 40], "x")
