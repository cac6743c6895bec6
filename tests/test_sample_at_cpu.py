"""CPU-side tests of DepthPipeline.sample_at: the host geometry (tiling.resize_points, tiling.point_run), the gather-form numpy
restatement the GPU tests compare against (tests/sample_at_oracle.py) tied to render_at_oracle.fold_at - and through it to the
pinned oracle - and every check native.fold_records_points / native.fold_refocus_stack_points / the two C entries /
DepthPipeline.sample_at / refocus_stack(points=) / the workflow flags make on the host before a kernel is launched."""
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, relmax
from be_hip import tiling
import render_at_oracle as rao
import sample_at_oracle as sao
from test_render_at_cpu import g6_records64

R = 21


# ---------------------------------------------------------------------------------------------- resize_points
def test_resize_points_values_and_checks():
    p = tiling.resize_points(147, 200, (220, 300))
    assert p.dtype == np.float32 and p.shape == (220, 300, 2)
    assert p[0, 0].tolist() == [0.0, 0.0] and p[-1, -1].tolist() == [146.0, 199.0]            # align corners
    for iy in (1, 7, 111, 218):
        assert p[iy, 5, 0] == np.float32((iy * 146) / 219) and p[iy, 5, 1] == np.float32((5 * 199) / 299)
    assert np.array_equal(p[:, 0, 0], p[:, 17, 0]) and np.array_equal(p[3, :, 1], p[100, :, 1])
    assert np.all(np.diff(p[:, 0, 0]) > 0) and np.all(np.diff(p[0, :, 1]) > 0)
    # down-sampling, a window, a single sample per axis
    q = tiling.resize_points(1080, 1920, (720, 1280))
    assert q.shape == (720, 1280, 2) and q[-1, -1].tolist() == [1079.0, 1919.0] and q[1, 1, 0] == np.float32(1079 / 719)
    wdw = tiling.resize_points(147, 200, (1, 5), (10, 20, 30, 41))
    assert wdw.shape == (1, 5, 2) and np.all(wdw[..., 0] == 10) and wdw[0, :, 1].tolist() == [20.0, 30.0, 40.0, 50.0, 60.0]
    one = tiling.resize_points(147, 200, (3, 1), (10, 20, 1, 1))
    assert np.all(one[..., 0] == 10) and np.all(one[..., 1] == 20)                           # h == 1: every sample on the one pixel
    assert sao.valid_points(p, 147, 200).all() and sao.valid_points(q, 1080, 1920).all()
    for bad in ((0, 5), (5, 0), (5,), (5, 5, 5), 7, None, (2.5, 4), "ab", (True, 4)):
        with pytest.raises(ValueError, match="size"):
            tiling.resize_points(147, 200, bad)
    with pytest.raises(ValueError, match="window"):
        tiling.resize_points(147, 200, (10, 10), (0, 0, 148, 200))


@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_resize_points_is_the_lattice_of_render_at_at_dyadic_ratios(k):
    for H, W, win in ((147, 147, None), (200, 262, None), (200, 262, (13, 29, 40, 57)), (1080, 1920, (1000, 1800, 80, 120))):
        lat = tiling.lattice(H, W, k, win)
        top, left, h, w = lat["window"]
        p = tiling.resize_points(H, W, (lat["Ho"], lat["Wo"]), win)
        assert p.shape == (lat["Ho"], lat["Wo"], 2)
        assert np.array_equal(p, sao.lattice_points(k, lat["window"]))
        # the kernel's split recovers the lattice's integers exactly: floor = Y // k, fraction = (Y % k) / k
        Y = top * k + np.arange(lat["Ho"])
        yq = np.floor(p[:, 0, 0]).astype(np.int64)
        assert np.array_equal(yq, Y // k) and np.array_equal(p[:, 0, 0] - yq.astype(np.float32), ((Y % k) / np.float32(k)).astype(np.float32))
        assert np.array_equal(p[::k, ::k, 0], np.broadcast_to(np.arange(top, top + h, dtype=np.float32)[:, None], (h, w)))


# ---------------------------------------------------------------------------------------------- point_run
def _grids():
    yield "147/1", list(range(0, 127, 1)), 147
    yield "147/2", list(range(0, 127, 2)), 147
    yield "150/2", list(range(0, 130, 2)), 150                          # the uniform stride-2 grid stops one pixel short
    yield "200", tiling.patch_grid(200, 2), 200
    yield "262", tiling.patch_grid(262, 2), 262


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16])
def test_point_run_on_lattice_points_is_lattice_runs(k):
    for name, origins, size in _grids():
        runs = tiling.lattice_runs(origins, (size - 1) * k + 1, k)
        for Y, (lo, hi, pos) in enumerate(runs):
            y = float(np.float32(Y / k)) if k != 3 else Y / 3                # dyadic: exact in float32 as well
            plo, phi, q, f = tiling.point_run(origins, y)
            if hi < lo:
                assert phi < plo, (name, Y)
                continue
            assert (plo, phi) == (lo, hi), (name, k, Y)
            assert q == [qq for qq, _ in pos], (name, k, Y)
            assert (f > 0) == (pos[0][1] > 0) and (k == 3 or f == pos[0][1] / k), (name, k, Y)


def test_point_run_against_brute_force_on_random_points():
    rng = np.random.default_rng(11)
    for name, origins, size in _grids():
        ys = np.concatenate([rng.random(3000) * (size - 1), np.arange(size, dtype=np.float64), [size - 1 - 1e-9, 1e-9, 20.0, 20.000001]])
        uncovered = 0
        for y in ys.astype(np.float32).astype(np.float64):
            lo, hi, q, f = tiling.point_run(origins, float(y))
            cover = [i for i, o in enumerate(origins) if o <= y <= o + R - 1]
            assert cover == list(range(lo, hi + 1)), (name, y)
            assert 0 <= f < 1 and math.floor(y) + f == y
            for i, qq in zip(cover, q):
                assert qq + f == y - origins[i] and 0 <= qq <= (R - 1 if f == 0 else R - 2), (name, y)   # lin[q+1] stays inside the table
            # the uniform closed form of the kernel
            if name != "200" and name != "262":
                s = origins[1] - origins[0]
                first = math.floor(y) + (1 if f > 0 else 0) - (R - 1)
                clo, chi = (first + s - 1) // s if first > 0 else 0, min(math.floor(y) // s, len(origins) - 1)
                assert (clo, chi) == (lo, hi) if cover else chi < clo, (name, y)
            uncovered += not cover
        assert (uncovered > 0) == (name == "150/2"), name               # only past the last patch of the short grid (y > 148)


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("densify", [None, "w"])
def test_gather_oracle_equals_the_lattice_oracle_exactly_on_a_k4_window(densify):
    """sample_at_oracle.fold_points (gather form) against render_at_oracle.fold_at (scatter form, tied to the pinned oracle by
    test_render_at_cpu.py) on the k = 4 lattice of a window, float64: the same arithmetic in the same order, difference 0."""
    from oracle import depth as od
    rec, _ = g6_records64(densify)
    uni = list(range(0, 147 - R + 1, 2))
    win = (100, 37, 12, 15)
    rhos = [10.39, 9.4928]
    want = rao.fold_at(rec, uni, uni, 147, 147, 4, win, np.float64, densify_w=densify == "w", rho_primes=rhos, consts=od.depth_consts())
    pts = tiling.resize_points(147, 147, (45, 57), win)
    got = sao.fold_points(rec, uni, uni, 147, 147, pts, np.float64, densify_w=densify == "w", rho_primes=rhos, consts=od.depth_consts())
    assert got["valid"].all() and np.array_equal(got["count"], want["count"])
    for k in rao.MAPS + ("stack",):
        assert got[k].shape == want[k].shape, k
        diff = float(np.abs(got[k] - want[k]).max())
        print(f"gather vs scatter oracle, densify={densify}: {k} {diff}")
        assert diff == 0.0, (k, diff)


def test_oracle_float32_against_float64_on_the_seeded_points():
    """The bounds and the flip cap the GPU test holds the kernel to are reachable by the reference arithmetic alone: the oracle's
    own float32 run against its float64 run on the g6 scene, seed 7, 20 000 points.  Measured: flip share 0, largest relmax 8.4e-7."""
    rec, _ = g6_records64(None)
    uni = list(range(0, 147 - R + 1, 2))
    pts = sao.random_points(147, 147, 20000, 7)
    frac = pts - np.floor(pts)
    assert sao.valid_points(pts, 147, 147).all() and ((frac > 0).mean() > 0.99)               # off the lattice
    a = sao.fold_points(rec, uni, uni, 147, 147, pts, np.float32)
    b = sao.fold_points(rec, uni, uni, 147, 147, pts, np.float64)
    assert a["bndry"].dtype == np.float32 and b["bndry"].dtype == np.float64 and int(b["count"].min()) >= 1
    flips = np.abs(a["conf"].astype(np.float64) - b["conf"]) > 1e-6
    share = float(flips.mean())
    err = {k: relmax(a[k][..., ~flips], b[k][..., ~flips]) if k in ("depth", "conf") else relmax(a[k], b[k]) for k in rao.MAPS}
    print(f"\noracle float32 vs float64, 20000 points: flip share {share:.2e}  " + "  ".join(f"{k} {e:.1e}" for k, e in err.items()))
    assert share <= 2e-3
    bounds = dict(image=1e-4, shpd=1e-4, refoc=1e-4, bndry=1e-5, depth=1e-5, conf=1e-6)
    for k, e in err.items():
        assert e <= bounds[k], (k, e)


def test_oracle_domain_and_integer_points():
    rec, _ = g6_records64(None)
    uni = list(range(0, 147 - R + 1, 2))
    pts = np.array([[146, 146], [-0.25, 3], [3, 146 + 1e-3], [np.nan, 3], [3, np.inf], [-np.inf, 3], [0, 0], [57, 90]], np.float32)
    got = sao.fold_points(rec, uni, uni, 147, 147, pts, np.float64)
    assert got["valid"].tolist() == [True, False, False, False, False, False, True, True]
    full = rao.fold_at(rec, uni, uni, 147, 147, 1, None, np.float64)
    for k in rao.MAPS:
        assert np.all(got[k][..., 1:6] == 0), k
        for n, (y, x) in ((0, (146, 146)), (6, (0, 0)), (7, (57, 90))):
            assert np.array_equal(got[k][..., n], full[k][..., y, x]), (k, n)


# ---------------------------------------------------------------------------------------------- host checks
def test_native_wrappers_check_before_the_library(monkeypatch):
    from be_hip import native

    def no_lib():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(native, "lib", no_lib)
    monkeypatch.setattr(native, "ops", no_lib)
    opts, consts, rec = native.RenderOpts(), native.DepthConsts(), torch.zeros(4096, 32)
    uni = list(range(0, 127, 2))
    pts = torch.zeros(5, 2)
    calls = (lambda **kw: native.fold_records_points(opts, kw.pop("rec", rec), 147, 147, kw.pop("pts", pts), **kw),
             lambda **kw: native.fold_refocus_stack_points(opts, consts, kw.pop("rec", rec), [10.39], 147, 147, kw.pop("pts", pts), **kw))
    for call in calls:
        for bad in (torch.zeros(5, 3), torch.zeros(5), torch.zeros(0, 2), torch.tensor(1.0)):
            with pytest.raises(ValueError, match=r"\[\.\.\.,2\]"):
                call(pts=bad, hp=64, wp=64)
        for bad in (torch.zeros(5, 2, dtype=torch.float64), torch.zeros(5, 2, dtype=torch.int32), [[1.0, 2.0]], np.zeros((5, 2), np.float32)):
            with pytest.raises(ValueError, match="float32"):
                call(pts=bad, hp=64, wp=64)
        with pytest.raises(ValueError, match="both"):
            call(ys=uni)
        with pytest.raises(ValueError, match="both"):
            call(xs=uni)
        with pytest.raises(ValueError, match="cover"):
            call(rec=rec[:63 * 64], ys=uni[:-1], xs=uni)
        with pytest.raises(RuntimeError, match=r"\[4096,32\]"):
            call(rec=rec[:100], hp=64, wp=64)
        with pytest.raises(RuntimeError, match=r"\[P,32\]"):
            call(rec=torch.zeros(64, 64, 32), hp=64, wp=64)
        with pytest.raises(RuntimeError, match="hp and wp"):
            call()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(hp=64, wp=64)                                          # CPU records
    with pytest.raises(ValueError, match="rho_primes"):
        native.fold_refocus_stack_points(opts, consts, rec, [], 147, 147, pts, hp=64, wp=64)


def test_pipeline_host_checks():
    import utils
    from be_hip.pipeline import DepthPipeline
    pipe = DepthPipeline(None, None, None, utils.DepthEtas(utils.get_args("eval", argv=[]), "cpu"))
    rec = torch.zeros(4096, 32)
    grid = dict(H=147, W=147, hp=64, wp=64, stride=2, ys=None, xs=None)
    maps = dict(records=rec, grid=grid)
    pts = [[1.5, 2.25], [3, 4]]
    with pytest.raises(ValueError, match="records"):
        pipe.sample_at(dict(grid=grid), pts)
    with pytest.raises(ValueError, match="grid"):
        pipe.sample_at(dict(records=rec), pts)
    for bad in (torch.zeros(5, 3), [1.0, 2.0, 3.0], 1.0, np.zeros((0, 2)), "ab", None, torch.zeros(2, 2, dtype=torch.complex64)):
        with pytest.raises(ValueError, match="points"):
            pipe.sample_at(maps, bad)
    with pytest.raises(ValueError, match="unknown maps"):
        pipe.sample_at(maps, pts, want=("depth_map",))
    for ok in (pts, np.asarray(pts), torch.tensor(pts, dtype=torch.float64), torch.tensor([[1, 2]])):
        with pytest.raises(ValueError, match="GPU"):                    # accepted, converted; CPU records: nothing computes on the CPU
            pipe.sample_at(maps, ok)
    with pytest.raises(ValueError, match="grid"):
        pipe.render_resized(dict(records=rec), (10, 10))
    with pytest.raises(ValueError, match="size"):
        pipe.render_resized(maps, (10, 0))
    with pytest.raises(ValueError, match="window"):
        pipe.render_resized(maps, (10, 10), window=(0, 0, 148, 147))
    with pytest.raises(ValueError, match="GPU"):
        pipe.render_resized(maps, (220, 220))
    for kw in (dict(scale=2), dict(window=(0, 0, 10, 10)), dict(scale=2, window=(0, 0, 10, 10))):
        with pytest.raises(ValueError, match="without scale / window"):
            pipe.refocus_stack(maps, rho_primes=[10.39], points=pts, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.refocus_stack(maps, points=pts)
    with pytest.raises(ValueError, match="GPU"):
        pipe.refocus_stack(maps, rho_primes=[10.39], points=pts)


def test_entries_are_declared_exported_bound_and_check_their_arguments():
    from be_hip import native
    from be_hip.pipeline import DepthPipeline
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_fold_records_points_f32", "be_fold_refocus_stack_points_f32"):
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    o = native.ops()
    assert o is not None and hasattr(o, "fold_records_points") and hasattr(o, "fold_refocus_stack_points")
    tail = "Tensor? ys, Tensor? xs, int hp, int wp, int H, int W, int stride, Tensor points"
    assert tail + ", bool densify_w, int want" in str(torch.ops.be.fold_records_points.default._schema)
    assert "Tensor rho_primes, " + tail in str(torch.ops.be.fold_refocus_stack_points.default._schema)
    assert callable(native.fold_records_points) and callable(native.fold_refocus_stack_points)
    assert hasattr(DepthPipeline, "sample_at") and hasattr(DepthPipeline, "render_resized")
    # host-side argument checks of the library fail before any launch (no GPU needed)
    ro, dc = native.RenderOpts(), native.DepthConsts()
    one = native.C.c_void_p(16)                                         # a non-null, 16-byte aligned address; never read
    grid = (("hp", 64), ("wp", 64), ("H", 147), ("W", 147), ("stride", 2), ("ys", None), ("xs", None), ("pts", one), ("N", 100))
    fold = lambda **kw: [kw.get(k, d) for k, d in (("o", ro), ("rec", one)) + grid + (("densify_w", 0),) + tuple(
        (m, one) for m in native.FOLD_MAPS) + (("stream", None),)]
    stack = lambda **kw: [kw.get(k, d) for k, d in (("o", ro), ("dc", dc), ("rec", one)) + grid + (("rho", one), ("K", 1), ("out", one),
                                                                                                  ("stream", None))]
    shared = ((dict(rec=None), b"null pointer"), (dict(o=None), b"null pointer"), (dict(pts=None), b"null pointer"),
              (dict(rec=native.C.c_void_p(20)), b"16-byte aligned"), (dict(ys=one), b"both"), (dict(xs=one), b"both"),
              (dict(hp=65), b"exceeds the image"), (dict(stride=0), b"bad sizes"), (dict(H=20), b"bad sizes"),
              (dict(ys=one, xs=one, hp=128), b"HP / WP must be"), (dict(N=0), b"N must be"), (dict(N=-5), b"N must be"),
              (dict(N=0xffffff * 256 + 1), b"N must be"), (dict(H=2 ** 24 + 1, hp=1, wp=1), b"too large"),
              (dict(H=70000, W=70000, hp=50000, wp=50000, stride=1), b"too large"))
    for fn, args, extra in ((lib.be_fold_records_points_f32, fold, ()),
                            (lib.be_fold_refocus_stack_points_f32, stack, ((dict(rho=None), b"null pointer"), (dict(out=None), b"null pointer"),
                                                                           (dict(dc=None), b"null pointer"), (dict(K=0), b"K must be"),
                                                                           (dict(K=65535 * lib.be_refocus_stack_chunk() + 1), b"K must be")))):
        for kw, msg in shared + extra:
            assert fn(*args(**kw)) != 0, kw
            assert msg in lib.be_last_error(), (kw, lib.be_last_error())


def test_workflow_arguments():
    import utils
    a = utils.get_args("eval", argv=[])
    assert a.render_size is None and a.sample_points is None            # off by default
    a = utils.get_args("eval", big=True, argv=["--render_size", "800", "600", "--sample_points", "p.npy", "--out_path", "x"])
    assert (a.render_size, a.sample_points, a.out_path) == ([800, 600], "p.npy", "x")
