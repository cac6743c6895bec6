"""Host statement of the nearest-sample flood fill (native.fill_nearest, DepthPipeline.complete): the numpy restatement of what
k_fill_seeds, k_fill_pass and k_fill_tail of be_fill.hip compute, operation by operation - to those kernels what camera.splat_f32 is
to the z-buffer.  Pure numpy and python; nothing here needs a GPU.

The assignment is integer arithmetic (jump flooding over a seed map of linear indices y * W + x, every pass a minimum of the key
(squared distance, seed index) over nine candidates), the robust local mean float32 with one rounding per operation, summed in
row-major order.  Jump flooding is APPROXIMATE: a pixel can end with a seed that is not its nearest when the nearest never reaches
one of the nine positions it looks at.  With the leading step-1 pass ("1+JFA") that is rare and the seed found is barely farther
(tests/test_complete_cpu.py records the figures); nearest_seed_exact is the brute-force search the tests compare with.
"""
from __future__ import annotations

import numpy as np

_F = np.float32
MAX_SIDE = 16384            # d2 < 2^29 and a linear index < 2^28: the kernels work in int32
MAX_SMOOTH = 8
_NONE = np.int64(1) << np.int64(62)


def jfa_steps(H, W):
    """The schedule 1, 2^(L-1), .., 4, 2, 1 with L = ceil(log2(max(H, W))): [1] for a 1 x 1 image."""
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"jfa_steps: H and W must be in [1, {MAX_SIDE}], got {H} x {W}")
    L = (max(H, W) - 1).bit_length()
    return [1] + [1 << k for k in range(L - 1, -1, -1)]


def seeds_of(depth, weight=None):
    """Pixel p is a seed iff weight[p] > 0, depth[p] > 0 and depth[p] < inf (NaN fails all three); weight None: 1 everywhere."""
    z = np.asarray(depth, _F)
    if z.ndim != 2 or z.size == 0:
        raise ValueError(f"seeds_of: depth must be [H,W], got {z.shape}")
    with np.errstate(invalid="ignore"):
        ok = (z > 0) & (z < _F(np.inf))
        if weight is not None:
            w = np.asarray(weight, _F)
            if w.shape != z.shape:
                raise ValueError(f"seeds_of: weight must be {z.shape}, got {w.shape}")
            ok &= w > 0
    return ok


def jfa_pass(seed, s):
    """One pass with step s over the seed map [H,W] (linear indices, -1: none): per pixel, of the nine positions p + (dy, dx) s inside
    the image that hold a seed, the candidate with the smallest key d2 << 32 | c -> (the next seed map, that candidate's d2 or -1)."""
    H, W = seed.shape
    seed = seed.astype(np.int64)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    best = np.full((H, W), _NONE, np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y0, y1 = max(0, -dy * s), min(H, H - dy * s)
            x0, x1 = max(0, -dx * s), min(W, W - dx * s)
            if y0 >= y1 or x0 >= x1:
                continue
            cand = np.full((H, W), -1, np.int64)
            cand[y0:y1, x0:x1] = seed[y0 + dy * s:y1 + dy * s, x0 + dx * s:x1 + dx * s]
            cy, cx = cand // W, cand % W
            d2 = (y - cy) ** 2 + (x - cx) ** 2
            best = np.minimum(best, np.where(cand >= 0, (d2 << 32) | cand, _NONE))
    found = best != _NONE
    return np.where(found, best & 0xFFFFFFFF, -1).astype(np.int32), np.where(found, best >> 32, -1).astype(np.int32)


def nearest_seed(valid):
    """valid [H,W] bool -> (index [H,W] int32: the seed jump flooding assigns each pixel, as y * W + x; dist2 [H,W] int32: the
    squared distance to it); -1 in both everywhere when no pixel is valid.  A seed is assigned itself."""
    valid = np.asarray(valid, bool)
    if valid.ndim != 2 or valid.size == 0:
        raise ValueError(f"nearest_seed: valid must be [H,W], got {valid.shape}")
    H, W = valid.shape
    seed = np.where(valid, np.arange(H * W, dtype=np.int32).reshape(H, W), np.int32(-1))
    d2 = None
    for s in jfa_steps(H, W):
        seed, d2 = jfa_pass(seed, s)
    return seed, d2


def nearest_seed_exact(valid):
    """The brute-force nearest seed of every pixel (squared Euclidean distance, ties to the lower index) -> (index, dist2) as
    nearest_seed.  O(pixels x seeds): for the tests."""
    valid = np.asarray(valid, bool)
    H, W = valid.shape
    src = np.flatnonzero(valid.ravel())
    if src.size == 0:
        return np.full((H, W), -1, np.int32), np.full((H, W), -1, np.int32)
    y, x = np.mgrid[0:H, 0:W].astype(np.int32)
    sy, sx = (src // W).astype(np.int32), (src % W).astype(np.int32)
    d2 = (y.reshape(-1, 1) - sy[None]) ** 2 + (x.reshape(-1, 1) - sx[None]) ** 2
    k = d2.argmin(1)                                                # the first minimum: src is ascending
    return src[k].astype(np.int32).reshape(H, W), d2[np.arange(H * W), k].astype(np.int32).reshape(H, W)


def local_mean(depth, weight, valid, smooth, sigma_z, dtype=np.float32):
    """The robust local mean of every seed s, [H,W] (0 off the seeds): num / den over the seeds q of the window [sy-r, sy+r] x
    [sx-r, sx+r] clipped to the image, in row-major order, one rounding of `dtype` per operation: d = z_q - z_s;
    k = w_q / (1 + (d d) inv), inv = 1 / (sigma_z sigma_z); num += k z_q; den += k.  sigma_z is the float32 number the kernels take
    whatever dtype is."""
    T = np.dtype(dtype).type
    z = np.asarray(depth, _F).astype(T)
    w = np.ones_like(z) if weight is None else np.asarray(weight, _F).astype(T)
    H, W = z.shape
    r = int(smooth)
    sig = T(_F(sigma_z))
    inv = T(1) / (sig * sig)
    num, den = np.zeros((H, W), T), np.zeros((H, W), T)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                y0, y1 = max(0, -dy), min(H, H - dy)
                x0, x1 = max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                here = (slice(y0, y1), slice(x0, x1))
                there = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                d = z[there] - z[here]
                k = w[there] / (T(1) + (d * d) * inv)
                ok = valid[there] & valid[here]
                num[here] = np.where(ok, num[here] + k * z[there], num[here])
                den[here] = np.where(ok, den[here] + k, den[here])
        mean = np.where(valid, num / den, T(0))
    assert mean.dtype == T
    return mean


def fill_nearest(depth, weight=None, smooth=2, sigma_z=0.02, dtype=np.float32):
    """The statement of be_fill_nearest_f32 with the float arithmetic in `dtype` -> dict(depth [H,W] of `dtype`: the input at seeds,
    the seed's depth (smooth = 0) or robust local mean (smooth = r > 0) at holes; index, dist2 [H,W] int32 of nearest_seed; seeds
    [H,W] bool); 0 / -1 / -1 when there is no seed."""
    if isinstance(smooth, bool) or int(smooth) != smooth or not 0 <= smooth <= MAX_SMOOTH:
        raise ValueError(f"fill_nearest: smooth must be an integer in [0, {MAX_SMOOTH}], got {smooth!r}")
    if not 0 < float(sigma_z) < float("inf"):
        raise ValueError("fill_nearest: sigma_z must be a finite number > 0")
    T = np.dtype(dtype).type
    valid = seeds_of(depth, weight)
    index, dist2 = nearest_seed(valid)
    z = np.asarray(depth, _F).astype(T)
    src = local_mean(depth, weight, valid, smooth, sigma_z, dtype) if smooth > 0 else z
    found = index >= 0
    filled = src.ravel()[np.where(found, index, 0)]
    out = np.where(valid, z, np.where(found, filled, T(0)))
    assert out.dtype == T
    return dict(depth=out, index=index, dist2=dist2, seeds=valid)


def fill_nearest_f32(depth, weight=None, smooth=2, sigma_z=0.02):
    """fill_nearest in float32: the host statement of the kernels, bit for bit."""
    return fill_nearest(depth, weight, smooth, sigma_z, np.float32)
