"""Host side of DepthPipeline.run_any (no GPU): the flush-edge patch grid and the block schedule of be_hip/tiling.py, brute force
over sizes, and the plumbing of the two grid entry points (header, EXPORTED, torch.ops.be)."""
import math
import os
import re

import pytest
import torch

from be_hip import tiling
from be_hip.pipeline import DepthPipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 21
SIZES = list(range(147, 421)) + [480, 640, 1080, 1920]
PAIRS = [(147, 147), (200, 262), (480, 640), (640, 480), (1080, 1920), (235, 323), (587, 587), (148, 420)]


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_patch_grid_covers_every_pixel_and_is_todays_grid_where_that_is_defined(stride):
    for H in SIZES:
        g = tiling.patch_grid(H, stride)
        assert g[0] == 0 and g[-1] == H - R, (H, stride)
        gaps = [b - a for a, b in zip(g, g[1:])]
        assert all(0 < d <= stride for d in gaps), (H, stride)
        covered = [False] * H
        for o in g:
            for y in range(o, o + R):
                covered[y] = True
        assert all(covered), (H, stride)
        uniform = list(range(0, H - R + 1, stride))
        if (H - R) % stride == 0:
            assert g == uniform
        else:
            assert g == uniform + [H - R]                       # exactly one extra line, flush with the edge
        tiling.check_grid(g, H, stride)


def test_check_grid_refuses_tables_the_kernels_cannot_take():
    for bad in ([0, 2, 2, 4], [0, 4, 2, 6], [2, 4, 6], [0, 2, 4], [0, 3, 6], []):
        with pytest.raises(ValueError):
            tiling.check_grid(bad, 27, 2)
    tiling.check_grid([0, 2, 4, 6], 27, 2)
    tiling.check_grid([0, 2, 4, 5], 26, 2)
    with pytest.raises(ValueError):
        tiling.patch_grid(20)
    with pytest.raises(ValueError):
        tiling.patch_grid(147, 0)


@pytest.mark.parametrize("n_margin", [10, 0, 7])
def test_block_schedule_owns_every_line_once_and_keeps_the_margins(n_margin):
    hp = 64
    step = hp - 2 * n_margin
    for H in SIZES:
        n = len(tiling.patch_grid(H, 2))
        sched = tiling.block_schedule(n, hp, n_margin)
        assert len(sched) == max(1, math.ceil((n - 2 * n_margin) / step)), (H, n)
        owner = [0] * n
        for k, (st, ks, ke) in enumerate(sched):
            assert 0 <= st and st + hp <= n, (H, st)                                  # the window lies inside the grid
            assert 0 <= ks < ke <= hp, (H, k, ks, ke)
            for line in range(st + ks, st + ke):
                owner[line] += 1
            # a kept line is at least n_margin away from a block edge that is not a grid edge
            if st > 0:
                assert ks >= n_margin, (H, k, ks)
            if st + hp < n:
                assert ke <= hp - n_margin, (H, k, ke)
        assert owner == [1] * n, H
        starts = [st for st, _, _ in sched]
        assert starts == sorted(set(starts)) and starts[0] == 0 and starts[-1] == n - hp
        assert all(b - a <= step for a, b in zip(starts, starts[1:]))
    if n_margin == 10:
        for H in SIZES:                                                                # the reference's block count
            n = len(tiling.patch_grid(H, 2))
            assert len(tiling.block_schedule(n)) == math.ceil((n - 20) / 44)
    with pytest.raises(ValueError):
        tiling.block_schedule(63)
    with pytest.raises(ValueError):
        tiling.block_schedule(100, 64, 32)


def test_schedule_is_big_windows_for_the_sizes_the_reference_defines():
    for H in (147, 235, 323, 587):
        for W in (147, 235, 323, 587):
            ys, xs, blocks = tiling.any_windows(H, W)
            assert ys == list(range(0, H - R + 1, 2)) and xs == list(range(0, W - R + 1, 2))
            ref = DepthPipeline.big_windows(H, W)
            assert len(blocks) == len(ref)
            for ((sv, sh), kept, dest), (win, rkept, rdest) in zip(blocks, ref):
                assert (ys[sv], xs[sh], 147, 147) == tuple(win)
                assert tuple(kept) == tuple(rkept) and tuple(dest) == tuple(rdest)


def test_two_dimensional_schedule_on_awkward_sizes():
    for H, W in PAIRS:
        ys, xs, blocks = tiling.any_windows(H, W)
        HP, WP = len(ys), len(xs)
        assert len(blocks) == math.ceil((HP - 20) / 44) * math.ceil((WP - 20) / 44)
        owner = torch.zeros(HP, WP, dtype=torch.int32)
        for (sv, sh), (vs, ve, hs, he), (Vs, Hs) in blocks:
            assert sv + 64 <= HP and sh + 64 <= WP and (Vs, Hs) == (sv + vs, sh + hs)
            owner[Vs:Vs + ve - vs, Hs:Hs + he - hs] += 1
        assert bool((owner == 1).all()), (H, W)
    assert tuple(len(t) for t in tiling.any_windows(200, 262)[:2]) == (91, 122) and len(tiling.any_windows(200, 262)[2]) == 6
    assert len(tiling.any_windows(480, 640)[2]) == 5 * 7
    with pytest.raises(ValueError):
        tiling.any_windows(146, 200)


def test_grid_entry_points_are_declared_exported_and_registered():
    from be_hip import native
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_render_full_grid_f32", "be_fold_records_grid_f32"):
        assert name in declared and name in native.EXPORTED and hasattr(lib, name), name
    o = native.ops()
    assert o is not None and hasattr(o, "render_full_grid") and hasattr(o, "fold_records_grid")
    assert "Tensor ys, Tensor xs" in str(torch.ops.be.render_full_grid.default._schema)
    assert "Tensor ys, Tensor xs, int H, int W" in str(torch.ops.be.fold_records_grid.default._schema)
    assert callable(native.render_full_grid) and callable(native.fold_records_grid) and hasattr(DepthPipeline, "run_any")
    # the C boundary validates before it launches: null tables, empty grids, more lines than distinct origins
    assert lib.be_fold_records_grid_f32(None, None, 1, 1, 21, 21, None, None, 0, None, None, None, None, None, None, None) != 0
    assert b"null pointer" in lib.be_last_error()
    assert lib.be_render_full_grid_f32(None, None, 10.0, 0, None, None, 21, 21, None, None, 1, 1, None, None) != 0


def test_origin_tables_are_checked_on_the_host():
    """The kernels trust their tables; native.origin_table is where a bad one stops (before any device work)."""
    from be_hip import native
    for bad in ([0, 2, 2], [0, 4, 2], [-1, 1], [0, 2, 8], []):
        with pytest.raises(ValueError):
            native.origin_table(bad, 27, "cpu")
    with pytest.raises(ValueError):                        # in bounds and increasing, but pixel 26 is under no patch
        native.origin_table([0, 2, 4], 27, "cpu", cover=True)
    with pytest.raises(ValueError):                        # a gap wider than a patch
        native.origin_table([0, 22, 29], 50, "cpu", cover=True)
    t = native.origin_table([0, 2, 4, 6], 27, "cpu", cover=True)
    assert t.dtype == torch.int32 and t.tolist() == [0, 2, 4, 6]
