"""Patch grid and block schedule for image pairs of ANY size (host, pure Python).

The reference's tiler (blurry_edges_test_big.py:116-119, DepthPipeline.big_windows) is defined only for H = 59 + 88 k: its
uniform patch grid must end exactly on the last pixel and its block count must divide the grid.  The two functions here drop
both conditions and reduce to the reference's grid and schedule wherever those are defined:

  patch_grid      per axis, origins 0, s, 2s, .. plus - when that grid stops short of the edge - ONE more origin flush with the
                  edge at size - R, so every pixel is under a patch.  The 2-D grid stays separable: a row table and a column table.
  block_schedule  per axis, hp (64) consecutive grid lines per block, blocks `hp - 2 n_margin` (44) lines apart, the last one pulled
                  back to end on the grid's last line; every grid line is KEPT by exactly one block and no kept line sits closer
                  than n_margin to a block edge that is not a grid edge.

A block is always hp x hp consecutive grid lines, i.e. the 4096 tokens in the row-major layout GlobalStage was trained on.  The
one place its input geometry differs from training: in the last block of an axis with a flush line the final gap between two
lines is smaller than `s` pixels.
"""
from __future__ import annotations

R = 21          # patch side (BE_R)
MAX_SCALE = 16  # BE_RENDER_AT_MAX_SCALE: the finest sampling lattice of render_at


def patch_grid(size: int, stride: int = 2, r: int = R) -> list:
    """Origins of the patches along one axis of `size` pixels: range(0, size - r + 1, stride), and size - r appended if it is not
    already the last.  Strictly increasing, first 0, last size - r, every gap <= stride."""
    if stride < 1:
        raise ValueError(f"patch_grid: stride must be >= 1, got {stride}")
    if size < r:
        raise ValueError(f"patch_grid: {size} pixels do not hold one {r}-pixel patch")
    lines = list(range(0, size - r + 1, stride))
    if lines[-1] != size - r:
        lines.append(size - r)
    return lines


def check_grid(lines, size: int, stride: int, r: int = R) -> None:
    """The conditions render / fold over an origin table rest on (the kernels do not check them)."""
    lines = list(lines)
    if not lines or lines[0] != 0 or lines[-1] != size - r:
        raise ValueError(f"patch grid must start at 0 and end at {size - r}")
    for a, b in zip(lines, lines[1:]):
        if not 0 < b - a <= stride:
            raise ValueError(f"patch grid must be strictly increasing with gaps <= {stride}: {a} -> {b}")


def lattice(H: int, W: int, scale: int = 1, window=None) -> dict:
    """The sampling lattice of DepthPipeline.render_at, checked: `scale` = k, an integer in 1..16; window = (top, left, h, w) in
    input pixels, inside the H x W image with h, w >= 1 (None: the whole image).  -> dict(scale, window, Ho, Wo) with
    Ho = (h - 1) k + 1, Wo = (w - 1) k + 1: output sample (iy, ix) sits at Y = top k + iy, X = left k + ix in units of 1/k pixel,
    the samples with iy % k == 0 are input pixels and the lattice ends on the window's last pixel centre."""
    if isinstance(scale, bool) or not isinstance(scale, int) or not 1 <= scale <= MAX_SCALE:
        raise ValueError(f"lattice: scale must be an integer in [1, {MAX_SCALE}], got {scale!r}")
    if window is None:
        window = (0, 0, H, W)
    try:
        top, left, h, w = (int(v) for v in window)
        exact = all(int(v) == v for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"lattice: window must be (top, left, h, w), got {window!r}") from None
    if not exact or top < 0 or left < 0 or h < 1 or w < 1 or top + h > H or left + w > W:
        raise ValueError(f"lattice: window (top, left, h, w) = {tuple(window)} leaves the {H} x {W} image (or has h, w < 1)")
    return dict(scale=scale, window=(top, left, h, w), Ho=(h - 1) * scale + 1, Wo=(w - 1) * scale + 1)


def lattice_runs(origins, size_out: int, scale: int, first: int = 0, r: int = R) -> list:
    """Per output sample iy of one axis (Y = first * scale + iy), the grid lines that cover it: [(i_lo, i_hi, [(q, rem)])] with
    origins[i] * k <= Y <= (origins[i] + r - 1) * k for i_lo <= i <= i_hi (integer arithmetic, a contiguous run; i_hi < i_lo when
    no line covers the sample) and the patch-local position t = Y - origins[i] * k = q * k + rem of each.  The host statement of
    what k_fold_records_at computes; with scale 1 it is k_fold_records' run."""
    origins = list(origins)
    out = []
    for iy in range(size_out):
        Y = first * scale + iy
        cover = [i for i, o in enumerate(origins) if o * scale <= Y <= (o + r - 1) * scale]
        if cover and cover != list(range(cover[0], cover[-1] + 1)):
            raise ValueError("lattice_runs: the covering lines are not contiguous (origins must increase)")
        lo, hi = (cover[0], cover[-1]) if cover else (0, -1)
        out.append((lo, hi, [divmod(Y - origins[i] * scale, scale) for i in cover]))
    return out


def uniform_run(Y: int, scale: int, stride: int, n: int, r: int = R):
    """The closed form of lattice_runs on the uniform grid origins = stride * index, index < n:
    i_lo = max(0, ceil((Y - (r-1) k) / (s k))), i_hi = min(n - 1, floor(Y / (s k)))."""
    sk = stride * scale
    return max(0, -((-(Y - (r - 1) * scale)) // sk)), min(n - 1, Y // sk)


def resize_points(H: int, W: int, size, window=None):
    """The align-corners sampling grid of DepthPipeline.render_resized: size = (Ho, Wo) output samples over window = (top, left, h, w)
    of the H x W image (None: all of it) -> float32 numpy [Ho,Wo,2] of (y, x) positions.  Sample iy sits at
    top + (iy * (h-1)) / (Ho-1) - an integer product, one float64 division, then the cast to float32 - and at top when Ho == 1, so
    the first and last samples are the window's first and last pixel centres.  With Ho - 1 = k (h - 1), k in {2, 4, 8, 16}, the
    positions are exactly top + iy / k: the lattice of render_at."""
    import numpy as np
    top, left, h, w = lattice(H, W, 1, window)["window"]
    try:
        Ho, Wo = size
        ok = all(not isinstance(v, bool) and int(v) == v and v >= 1 for v in (Ho, Wo))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"resize_points: size must be (Ho, Wo), integers >= 1, got {size!r}")
    Ho, Wo = int(Ho), int(Wo)

    def axis(first, n, n_out):
        if n_out == 1:
            return np.full(1, first, np.float32)
        return (first + (np.arange(n_out, dtype=np.int64) * (n - 1)) / np.float64(n_out - 1)).astype(np.float32)
    pts = np.empty((Ho, Wo, 2), np.float32)
    pts[..., 0] = axis(top, h, Ho)[:, None]
    pts[..., 1] = axis(left, w, Wo)[None, :]
    return pts


def point_run(origins, y: float, r: int = R):
    """The grid lines that cover the real-valued position y on one axis: (i_lo, i_hi, q, f) with yq = floor(y), f = y - yq and
    yq + (f > 0) - (r-1) <= origins[i] <= yq for i_lo <= i <= i_hi (a contiguous run; i_hi < i_lo when no line covers y) and
    q = [yq - origins[i]], the index into the patch's coordinate table - at most r-1, and at most r-2 when f > 0.  The host
    statement of what k_fold_records_points computes; lattice_runs is this rule at y = Y / k."""
    import math
    origins = list(origins)
    yq = math.floor(y)
    f = y - yq
    first = yq + (1 if f > 0 else 0) - (r - 1)
    lo = 0
    while lo < len(origins) and origins[lo] < first:
        lo += 1
    hi = lo - 1
    while hi + 1 < len(origins) and origins[hi + 1] <= yq:
        hi += 1
    return lo, hi, [yq - origins[i] for i in range(lo, hi + 1)], f


def block_schedule(n: int, hp: int = 64, n_margin: int = 10) -> list:
    """Blocks along one axis of a grid of n lines -> [(start, ks, ke)]: the block holds grid lines start .. start + hp - 1 and
    KEEPS its local lines ks .. ke - 1 (global start + ks .. start + ke - 1).  Starts 0, step, 2 step, .. while start + hp < n,
    then a last block at n - hp; the first block keeps [0, hp - n_margin) (everything if it is alone), a middle block
    [n_margin, hp - n_margin), the last block everything from where its predecessor's kept range ended."""
    step = hp - 2 * n_margin
    if n_margin < 0 or step < 1:
        raise ValueError(f"block_schedule: n_margin {n_margin} leaves no kept lines in a block of {hp}")
    if n < hp:
        raise ValueError(f"block_schedule: {n} grid lines do not fill one block of {hp}")
    starts = []
    while len(starts) * step + hp < n:
        starts.append(len(starts) * step)
    starts.append(n - hp)
    out, kept_to = [], 0                                  # kept_to: first grid line no block has kept yet
    for k, st in enumerate(starts):
        ks = kept_to - st
        ke = hp if k == len(starts) - 1 else hp - n_margin
        out.append((st, ks, ke))
        kept_to = st + ke
    return out


def any_windows(H: int, W: int, block: int = 147, n_margin: int = 10, stride: int = 2, r: int = R):
    """-> (ys, xs, blocks): the two origin tables and the row-major block list
    [((sv, sh) first grid row / column of the block, (vs, ve, hs, he) kept local rows / columns, (Vs, Hs) where the kept window
    starts in the grid)] - big_windows with the pixel window replaced by the block's position in the grid (its pixel window is
    (ys[sv], xs[sh], block, block) whenever the block holds no flush line)."""
    if H < block or W < block:
        raise ValueError(f"an {H}x{W} image is smaller than one {block}x{block} block")
    hp = (block - r) // stride + 1
    ys, xs = patch_grid(H, stride, r), patch_grid(W, stride, r)
    blocks = [((sv, sh), (vs, ve, hs, he), (sv + vs, sh + hs))
              for sv, vs, ve in block_schedule(len(ys), hp, n_margin) for sh, hs, he in block_schedule(len(xs), hp, n_margin)]
    return ys, xs, blocks
