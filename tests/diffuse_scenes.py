"""Scenes shared by test_diffuse_cpu.py and test_diffuse_gpu.py: depth / weight / edge triples for the diffusion depth completion
(be_hip/diffuse.py, native.fill_diffuse), and the float64 direct solve and the float32 statement of each, computed once."""
import numpy as np

from be_hip import diffuse
import complete_scenes as cs

SHAPES = ((1, 1), (1, 7), (5, 3), (24, 31), (37, 53), (64, 64), (65, 33))
PLANE_SHAPES = ((24, 31), (37, 53), (64, 64))                       # where the ramp and the rooms are judged
KINDS = ("ramp", "rooms", "sparse", "dense", "edge", "one")         # the contract scenes
RANGE_KINDS = KINDS + ("corners",)                                  # 'corners': near-singular, held to the range check only
RADII = (0, 2)
SIGMA_Z = cs.SIGMA_Z
LEAK = 1e-3
TOL = 1e-4                                                          # metres: the project's bound for maps against float64
NEAR, FAR = 0.80, 1.10

# max |avg - u| over the holes that diffuse.fill_diffuse (float32, default schedule) reached on each scene over SHAPES, 147 x 147
# and RADII, measured on the CPU and rounded up (2.4e-6, 6.4e-6, 2.3e-6, 2.0e-6, 2.3e-6, 0: one seed gives a constant, which the
# sweeps left unchanged); a GPU residual may be 4 x this
RESIDUAL_CPU = dict(ramp=2.5e-6, rooms=6.5e-6, sparse=2.5e-6, dense=2.0e-6, edge=2.5e-6, one=0.0)


def ramp(H, W):
    """A plane z = 0.80 + 0.30 x / (W - 1) measured on two full-height bands |x - W//5| < 2 and |x - 4W//5| < 2: the gradient runs
    along x only, so the harmonic fill between the bands is the plane itself.  -> (depth, weight None, edge None, plane [H,W]
    float64, between [H,W] bool: the holes between the two bands)."""
    x = np.broadcast_to(np.arange(W, dtype=np.float64), (H, W))
    plane = NEAR + 0.30 * x / max(W - 1, 1)
    a, b = W // 5, 4 * W // 5
    band = (np.abs(x - a) < 2) | (np.abs(x - b) < 2)
    depth = np.where(band, plane, 0).astype(np.float32)
    return depth, None, None, plane, ~band & (x > a) & (x < b)


def rooms(H, W, with_edge=True):
    """Two rooms: columns 1..2 measured at 0.80 m, columns W-3..W-2 at 1.10 m (column numbers clipped into the image, the far room
    written last), and a wall, edge = 1, on column W//2.  -> (depth, weight None, edge or None)."""
    depth = np.zeros((H, W), np.float32)
    depth[:, np.clip([1, 2], 0, W - 1)] = NEAR
    depth[:, np.clip([W - 3, W - 2], 0, W - 1)] = FAR
    edge = np.zeros((H, W), np.float32)
    edge[:, W // 2] = 1
    return depth, None, edge if with_edge else None


def scene(kind, H, W):
    """-> (depth, weight or None, edge or None)."""
    if kind == "ramp":
        return ramp(H, W)[:3]
    if kind == "rooms":
        return rooms(H, W)
    return cs.scene(kind, H, W) + (None,)


_EXACT, _HOST = {}, {}


def exact(kind, H, W, r):
    """diffuse.solve_exact of scene(kind, H, W) at smooth radius r, computed once and shared: treat it as read-only."""
    key = (kind, H, W, r)
    if key not in _EXACT:
        _EXACT[key] = diffuse.solve_exact(*scene(kind, H, W), smooth=r, sigma_z=SIGMA_Z, leak=LEAK)
    return _EXACT[key]


def host(kind, H, W, r):
    """diffuse.fill_diffuse (float32, default schedule) of scene(kind, H, W) at smooth radius r, computed once and shared."""
    key = (kind, H, W, r)
    if key not in _HOST:
        _HOST[key] = diffuse.fill_diffuse(*scene(kind, H, W), smooth=r, sigma_z=SIGMA_Z, leak=LEAK)
    return _HOST[key]
