"""CPU tests of the diffusion depth completion's host statement (be_hip/diffuse.py): the float64 direct solve against the equations
it states, what a harmonic fill buys over the nearest-sample fill (the ramp, the rooms), the float32 pyramid and sweeps - which
tests/test_diffuse_gpu.py holds the kernels of be_diffuse.hip to - against the direct solve, and the entry's declarations and
argument checks.  No GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from be_hip import diffuse, fill
import complete_scenes as cs
import diffuse_scenes as ds

ALL_SHAPES = ds.SHAPES + ((147, 147),)


def _equation_error(u, seeds, edge, leak=ds.LEAK):
    """max over the holes of |u_p sum_q c_pq - sum_q c_pq u_q|, written with explicit loops over the four neighbours."""
    H, W = u.shape
    e = np.zeros((H, W)) if edge is None else np.clip(np.nan_to_num(np.asarray(edge, np.float64), nan=0.0), 0, 1)
    worst = 0.0
    for y in range(H):
        for x in range(W):
            if seeds[y, x]:
                continue
            lhs = rhs = 0.0
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= yy < H and 0 <= xx < W:
                    c = max(float(np.float32(leak)), float(np.float32(1) - np.float32(max(e[y, x], e[yy, xx]))))
                    lhs += c * u[y, x]
                    rhs += c * u[yy, xx]
            worst = max(worst, abs(lhs - rhs))
    return worst


# ------------------------------------------------------------------------------------------ 1. the direct solve
@pytest.mark.parametrize("H,W", ds.SHAPES)
def test_solve_exact_satisfies_the_equations(H, W):
    for kind in ds.RANGE_KINDS:
        depth, weight, edge = ds.scene(kind, H, W)
        for r in ds.RADII:
            ex = ds.exact(kind, H, W, r)
            seeds = fill.seeds_of(depth, weight)
            assert np.array_equal(ex["seeds"], seeds) and ex["depth"].dtype == np.float64
            want_b = fill.local_mean(depth, weight, seeds, r, ds.SIGMA_Z) if r else depth
            assert np.array_equal(ex["u"][seeds], want_b[seeds].astype(np.float64))                 # the boundary values
            assert np.array_equal(ex["depth"][seeds], depth[seeds].astype(np.float64))              # the input at seeds
            assert np.array_equal(ex["depth"][~seeds], ex["u"][~seeds])
            err = _equation_error(ex["u"], seeds, edge)
            assert err <= 1e-10, (kind, H, W, r, err)


def test_conductances():
    edge = np.array([[0.0, 0.25, 1.0, 2.0], [np.nan, -1.0, 0.9995, 0.5]], np.float32)
    ce, cs_ = diffuse.conductances(edge, 2, 4, 1e-3)
    assert ce.dtype == np.float32 and cs_.dtype == np.float32 and ce.shape == (2, 4)
    leak = np.float32(1e-3)
    assert np.array_equal(ce[0], np.array([0.75, leak, leak, 0], np.float32))                       # 2.0 counts as 1: the leak is left
    assert np.array_equal(ce[1], np.array([1, leak, leak, 0], np.float32))                          # NaN and -1 count as 0; 1 - 0.9995 < leak
    assert np.array_equal(cs_[0], np.array([1, 0.75, leak, leak], np.float32)) and not cs_[1].any()
    one_e, one_s = diffuse.conductances(None, 3, 2, 0.5)
    assert np.array_equal(one_e, [[1, 0]] * 3) and np.array_equal(one_s, [[1, 1], [1, 1], [0, 0]])


# ------------------------------------------------------------------------------------------ 2. the ramp
@pytest.mark.parametrize("H,W", ds.PLANE_SHAPES)
def test_a_plane_between_two_bands_is_reproduced_where_nearest_fill_steps(H, W):
    depth, weight, edge, plane, between = ds.ramp(H, W)
    assert between.any()
    ex = diffuse.solve_exact(depth, weight, edge, smooth=0, leak=ds.LEAK)
    err = np.abs(ex["depth"] - plane)[between].max()
    near = np.abs(fill.fill_nearest_f32(depth, weight, 0, ds.SIGMA_Z)["depth"] - plane)[between].max()
    print(f"ramp {H} x {W}: harmonic {err:.2e} m, nearest {100 * near:.1f} cm off the plane")
    assert err <= 1e-6
    assert near > 0.05


# ------------------------------------------------------------------------------------------ 3. the rooms
@pytest.mark.parametrize("H,W", ds.PLANE_SHAPES)
def test_an_edge_keeps_two_rooms_apart(H, W):
    depth, weight, edge = ds.rooms(H, W)
    left, right = np.s_[:, :W // 2], np.s_[:, W // 2 + 1:]
    ex = diffuse.solve_exact(depth, weight, edge, smooth=0, leak=ds.LEAK)["depth"]
    print(f"rooms {H} x {W}: with the edge left max {ex[left].max():.4f}, right min {ex[right].min():.4f}")
    assert ex[left].max() < ds.NEAR + 0.03 and ex[right].min() > ds.FAR - 0.03
    open_ = diffuse.solve_exact(depth, weight, None, smooth=0, leak=ds.LEAK)["depth"]
    print(f"rooms {H} x {W}: without it left max {open_[left].max():.4f}")
    assert open_[left].max() > ds.NEAR + 0.12


# ------------------------------------------------------------------------------------------ 4. convergence of the statement
@pytest.mark.parametrize("H,W", ALL_SHAPES)
def test_the_float32_statement_converges_to_the_direct_solve(H, W):
    """Achieved (float32, default schedule): at most 1.6e-5 m over all contract scenes, shapes and radii (rooms, 147 x 147); the
    residual at most 6.4e-6."""
    for kind in ds.KINDS:
        depth, weight, _ = ds.scene(kind, H, W)
        seeds = fill.seeds_of(depth, weight)
        for r in ds.RADII:
            ex, ho = ds.exact(kind, H, W, r), ds.host(kind, H, W, r)
            err = np.abs(ho["depth"].astype(np.float64) - ex["depth"]).max()
            print(f"{kind} {H} x {W} r {r}: {err:.2e} m from the direct solve, residual {ho['residual']:.2e}")
            assert ho["depth"].dtype == np.float32 and ho["residual"].dtype == np.float32
            assert err <= ds.TOL, (kind, H, W, r, err)
            assert 0 <= ho["residual"] <= ds.RESIDUAL_CPU[kind], (kind, H, W, r, ho["residual"])
            near = fill.fill_nearest_f32(depth, weight, r, ds.SIGMA_Z)
            assert np.array_equal(ho["index"], near["index"]) and np.array_equal(ho["dist2"], near["dist2"])
            assert np.array_equal(ho["depth"].view(np.uint32)[seeds], depth.view(np.uint32)[seeds])     # seeds keep their bits


def test_the_schedule_is_a_function_of_the_shape_and_iters():
    assert diffuse.level_sizes(147, 147) == [(147, 147), (74, 74), (37, 37), (19, 19), (10, 10), (5, 5), (3, 3)]
    assert diffuse.level_sizes(1, 1) == [(1, 1)] and diffuse.level_sizes(1, 7) == [(1, 7), (1, 4)]
    assert diffuse.tiles_of(128, 128) == (1, 1) and diffuse.tiles_of(129, 20) == (2, 1) and diffuse.tiles_of(587, 587) == (7, 7)
    plan = diffuse.schedule(147, 147)
    assert [p[:2] for p in plan] == diffuse.level_sizes(147, 147)
    assert plan[0][2] == [16] * 37 and plan[1][2] == [304] and plan[-1][2] == [16]                 # 4 x 147 -> 592; one region: one launch
    assert diffuse.schedule(147, 147, 40)[0][2] == [16, 16, 8] and diffuse.schedule(147, 147, 40)[1][2] == [40]
    assert plan[0][3] == np.float32(2 / (1 + np.sin(np.pi / 147))) and plan[0][3].dtype == np.float32
    for bad in (0, -1, 4097, 1.5, True, "x"):
        with pytest.raises(ValueError, match="iters"):
            diffuse.schedule(37, 53, bad)
    with pytest.raises(ValueError, match="H and W"):
        diffuse.schedule(0, 5)
    # more sweeps move nothing by more than the bound
    depth, weight, edge = ds.scene("edge", 37, 53)
    twice = diffuse.fill_diffuse(depth, weight, edge, 2, ds.SIGMA_Z, ds.LEAK, iters=2 * diffuse.default_sweeps(37, 53))
    assert np.abs(twice["depth"] - ds.host("edge", 37, 53, 2)["depth"]).max() <= ds.TOL


# ------------------------------------------------------------------------------------------ 5. the range
@pytest.mark.parametrize("H,W", ALL_SHAPES)
def test_filled_values_stay_within_the_boundary_values(H, W):
    for kind in ds.RANGE_KINDS:
        for r in ds.RADII:
            ex, ho = ds.exact(kind, H, W, r), ds.host(kind, H, W, r)
            seeds = ex["seeds"]
            if seeds.all():
                continue
            lo, hi = ex["u"][seeds].min(), ex["u"][seeds].max()
            for what, u in (("exact", ex["depth"]), ("float32", ho["depth"])):
                assert lo - ds.TOL <= u[~seeds].min() and u[~seeds].max() <= hi + ds.TOL, (kind, H, W, r, what)


# ------------------------------------------------------------------------------------------ 6. arguments and special cases
def test_no_seed_all_seeds_and_odd_edge_values():
    nothing = ((np.zeros((4, 6), np.float32), None), (np.full((4, 6), np.nan, np.float32), np.ones((4, 6), np.float32)),
               (np.ones((4, 6), np.float32), np.zeros((4, 6), np.float32)), (np.full((1, 1), np.inf, np.float32), None))
    edge = np.full((4, 6), 0.5, np.float32)
    for d, w in nothing:
        for out in (diffuse.solve_exact(d, w, edge if d.shape == (4, 6) else None), diffuse.fill_diffuse(d, w)):
            assert not out["seeds"].any() and not out["depth"].any()
            assert (out["index"] == -1).all() and (out["dist2"] == -1).all()
        assert diffuse.fill_diffuse(d, w)["residual"] == 0
    rng = np.random.default_rng(3)
    full = rng.uniform(0.8, 1.1, (9, 12)).astype(np.float32)
    for r in ds.RADII:
        out = diffuse.fill_diffuse(full, None, None, r, ds.SIGMA_Z)
        assert np.array_equal(out["depth"].view(np.uint32), full.view(np.uint32)) and out["residual"] == 0        # a copy of the input
        assert np.array_equal(diffuse.solve_exact(full, None, None, r)["depth"], full.astype(np.float64))
    # NaN and negative edge values count as 0, values above 1 as 1
    depth, weight, edge = ds.rooms(24, 31)
    odd = edge.copy()
    odd[edge == 1] = 7.5
    odd[:, 5] = np.nan
    odd[:, 20] = -3.0
    for f in (diffuse.solve_exact, diffuse.fill_diffuse):
        assert np.array_equal(f(depth, weight, odd, 0)["depth"], f(depth, weight, edge, 0)["depth"])
    # the invalid depths of the nearest-fill tests are no seeds here either
    depth, weight, want = cs.invalid_depths()
    out = diffuse.fill_diffuse(depth, weight, None, 2, ds.SIGMA_Z)
    assert np.array_equal(out["seeds"], want) and np.isfinite(out["depth"]).all() and (out["depth"] > 0).all()
    assert np.abs(out["depth"] - diffuse.solve_exact(depth, weight, None, 2, ds.SIGMA_Z)["depth"]).max() <= ds.TOL
    for f, who in ((diffuse.solve_exact, "solve_exact"), (diffuse.fill_diffuse, "fill_diffuse")):
        for kw in (dict(smooth=9), dict(smooth=-1), dict(smooth=1.5), dict(sigma_z=0), dict(sigma_z=float("inf")), dict(leak=0),
                   dict(leak=-1), dict(leak=1.5), dict(leak=float("nan")), dict(leak="x")):
            with pytest.raises(ValueError, match=who):
                f(depth, weight, **kw)
        with pytest.raises(ValueError, match="edge"):
            f(depth, weight, np.zeros((9, 11), np.float32))
    with pytest.raises(ValueError, match="iters"):
        diffuse.fill_diffuse(depth, weight, iters=0)


def test_float64_statement_is_closer_to_the_direct_solve():
    """The same sweeps in float64 end within 1e-6 of the direct solve: what is left in float32 is rounding, not the schedule."""
    for kind, H, W in (("edge", 37, 53), ("rooms", 64, 64), ("dense", 65, 33)):
        out = diffuse.fill_diffuse(*ds.scene(kind, H, W), smooth=2, sigma_z=ds.SIGMA_Z, leak=ds.LEAK, dtype=np.float64)
        assert out["depth"].dtype == np.float64
        assert np.abs(out["depth"] - ds.exact(kind, H, W, 2)["depth"]).max() <= 1e-6


def test_entry_is_declared_exported_bound_and_checks_its_arguments():
    from be_hip import native
    from be_hip.pipeline import DepthPipeline
    import inspect
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_fill_diffuse_f32", "be_fill_diffuse_scratch_bytes"):
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name)
    o = native.ops()
    assert o is not None and hasattr(o, "fill_diffuse")
    assert ("Tensor depth, Tensor? weight, Tensor? edge, int smooth_r, float sigma_z, float leak, int iters, bool fuse"
            in str(torch.ops.be.fill_diffuse.default._schema))
    sig = inspect.signature(DepthPipeline.complete).parameters
    assert [k for k in sig][1:] == ["maps", "smooth", "sigma_z", "method", "edges", "leak", "iters"]
    assert sig["method"].default == "nearest" and sig["edges"].default is True and sig["leak"].default == 1e-3 and sig["iters"].default is None
    # the scratch size: be_fill_nearest_f32's three images, then u (twice), e and the fixed bytes of every level
    for H, W in ((1, 1), (37, 53), (147, 147), (587, 587)):
        words = 3 * H * W + sum(3 * h * w + (h * w + 3) // 4 for h, w in diffuse.level_sizes(H, W))
        assert lib.be_fill_diffuse_scratch_bytes(H, W) == 4 * words
    assert lib.be_fill_diffuse_scratch_bytes(0, 4) == -1 and lib.be_fill_diffuse_scratch_bytes(4, 16385) == -1
    # host-side argument checks of the library fail before any launch (no GPU needed)
    one = native.C.c_void_p(16)                                         # a non-null address; never read
    order = ("depth", "weight", "edge", "H", "W", "r", "sigma", "leak", "iters", "fuse", "scratch", "out", "index", "dist2", "residual",
             "stream")
    base = dict(depth=one, weight=None, edge=None, H=37, W=53, r=2, sigma=0.02, leak=1e-3, iters=0, fuse=1, scratch=one, out=one,
                index=one, dist2=one, residual=one, stream=None)
    for kw, msg in ((dict(depth=None), b"null pointer"), (dict(scratch=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(index=None), b"null pointer"), (dict(dist2=None), b"null pointer"), (dict(residual=None), b"null pointer"),
                    (dict(H=0), b"H and W"), (dict(W=16385), b"H and W"), (dict(r=-1), b"smooth_r"), (dict(r=9), b"smooth_r"),
                    (dict(sigma=0.0), b"sigma_z"), (dict(sigma=float("nan")), b"sigma_z"), (dict(leak=0.0), b"leak"),
                    (dict(leak=float("nan")), b"leak"), (dict(leak=1.5), b"leak"), (dict(iters=-1), b"iters"), (dict(iters=4097), b"iters"),
                    (dict(fuse=2), b"fuse")):
        args = dict(base, **kw)
        assert lib.be_fill_diffuse_f32(*[args[k] for k in order]) != 0, kw
        assert msg in lib.be_last_error(), (kw, lib.be_last_error())
    # native.fill_diffuse checks on the host, before the library is touched
    with pytest.raises(ValueError, match="GPU"):
        native.fill_diffuse(torch.zeros(4, 5))
    for bad in (torch.zeros(4, 5, dtype=torch.float64), torch.zeros(5), torch.zeros(0, 3), np.zeros((4, 5), np.float32)):
        with pytest.raises(ValueError, match="float32"):
            native.fill_diffuse(bad)


def test_complete_method_argument():
    import utils
    a = utils.get_args("eval", argv=[])
    assert a.complete is False and a.complete_method == "nearest"
    b = utils.get_args("eval", big=True, argv=["--complete", "--complete_method", "diffuse"])
    assert b.complete is True and b.complete_method == "diffuse"
    c = utils.get_args("eval", argv=["--complete_method", "diffuse"])
    rest = lambda ns: {k: v for k, v in vars(ns).items() if k != "complete_method"}
    assert rest(a) == rest(c)                                           # the option changes no other argument
    with pytest.raises(SystemExit):
        utils.get_args("eval", argv=["--complete_method", "linear"])
