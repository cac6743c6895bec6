"""Scenes shared by test_complete_cpu.py and test_complete_gpu.py: depth / weight pairs for the nearest-sample flood fill
(be_hip/fill.py, native.fill_nearest), each generated from a fixed seed, and the host statement of each, computed once."""
import numpy as np

from be_hip import fill

NEAR, FAR = np.float32(0.80), np.float32(1.10)                      # the two planes of the slanted-edge scene, metres
BAND, NOISE = 3.0, 0.01                                             # samples within 3 px of the edge, +-1 cm noise
SHAPES = ((1, 1), (1, 7), (5, 3), (37, 53), (64, 64), (65, 33), (147, 147))
KINDS = ("sparse", "dense", "edge", "corners", "one")
RADII = (0, 2, 8)
SIGMA_Z = 0.02


def slanted_edge(H, W, seed=0):
    """A slanted edge through the middle of the image between a plane at 0.80 m and one at 1.10 m; depth (with +-1 cm noise) and a
    weight in (0.1, 1] only within 3 px of the edge, on both sides, 0 elsewhere - the shape of the pipeline's depth_map and conf.
    -> (depth, weight, near_side [H,W] bool: the pixel lies on the 0.80 m plane)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dist = (x - (W - 1) / 2) * np.cos(0.35) + (y - (H - 1) / 2) * np.sin(0.35)
    near_side = dist < 0
    band = np.abs(dist) < BAND
    z = np.where(near_side, NEAR, FAR) + rng.uniform(-NOISE, NOISE, (H, W))
    depth = np.where(band, z, 0).astype(np.float32)
    weight = np.where(band, rng.uniform(0.1, 1.0, (H, W)), 0).astype(np.float32)
    return depth, weight, near_side


def scene(kind, H, W):
    """-> (depth, weight or None).  'sparse' / 'dense': random seeds at density 0.003 / 0.05 (at least one), depths in the working
    range, random weights; 'edge': the slanted-edge band, which reaches the image border at both ends; 'corners': a single seed in
    each of the four corners, no weight; 'one': one seed only, on the last row."""
    rng = np.random.default_rng(1000 * H + W)
    if kind == "edge":
        return slanted_edge(H, W)[:2]
    depth, weight = np.zeros((H, W), np.float32), None
    if kind in ("sparse", "dense"):
        on = rng.random((H, W)) < (0.003 if kind == "sparse" else 0.05)
        on[rng.integers(H), rng.integers(W)] = True
        on[H - 1, rng.integers(W)] = True                          # seeds on the border: windows clipped there
        on[rng.integers(H), 0] = True
        depth = np.where(on, rng.uniform(0.75, 1.18, (H, W)), 0).astype(np.float32)
        weight = np.where(rng.random((H, W)) < 0.9, rng.uniform(0.05, 1.0, (H, W)), 0).astype(np.float32)      # a tenth of them weight 0
        y, x = np.argwhere(on)[0]
        weight[y, x] = 0.5
    elif kind == "corners":
        for y, x, z in ((0, 0, 0.8), (0, W - 1, 0.9), (H - 1, 0, 1.0), (H - 1, W - 1, 1.1)):
            depth[y, x] = z
    elif kind == "one":
        depth[H - 1, W // 2] = 0.93
    else:
        raise ValueError(kind)
    return depth, weight


_HOST = {}


def host(kind, H, W, r):
    """fill.fill_nearest_f32 of scene(kind, H, W) at smooth radius r, computed once and shared: treat it as read-only."""
    key = (kind, H, W, r)
    if key not in _HOST:
        depth, weight = scene(kind, H, W)
        _HOST[key] = fill.fill_nearest_f32(depth, weight, r, SIGMA_Z)
    return _HOST[key]


def invalid_depths():
    """A 9 x 12 map whose first row holds depths that are never seeds (NaN, +-inf, 0, negative) under positive weights, and three
    good samples.  -> (depth, weight, the seeds expected)."""
    depth = np.zeros((9, 12), np.float32)
    weight = np.ones((9, 12), np.float32)
    depth[0, :6] = [np.nan, np.inf, -np.inf, 0.0, -1.0, -0.0]
    depth[4, 2], depth[8, 11], depth[2, 9] = 0.9, 1.0, 1.1
    depth[6, 6], weight[6, 6] = 0.95, 0.0                          # a good depth under weight 0
    depth[7, 1], weight[7, 1] = 0.95, np.nan                       # ... and under a NaN weight
    want = np.zeros((9, 12), bool)
    want[4, 2] = want[8, 11] = want[2, 9] = True
    return depth, weight, want
