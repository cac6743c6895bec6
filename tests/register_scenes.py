"""The inputs the registration tests share (test_register_cpu.py, test_register_gpu.py): one analytic surface seen by two views of
the fuse scenes' 37 x 53 camera.  View A's depth is the surface itself, given over A's normalised image coordinates; view B's is
obtained by ray casting in float64 - 80 steps of bisection on the depth along each of B's rays under the true pose B -> A - never
by splatting A, whose nearest-wins z-buffer would bias the depth towards the camera on slopes.  The plane scene is a true plane
in space, Z = 1.0 + 0.2 X - 0.1 Y in metres of A's frame."""
import numpy as np

from be_hip import camera, registration

CAM = camera.Pinhole(60, 58, 18.2, 25.7)
SIZE = (37, 53)
_F = np.float32

POSES = dict(small=((0.03, -0.04, 0.05), (0.03, -0.02, 0.015)),          # 4.05 degrees, 39 mm
             large=((0.08, -0.10, 0.12), (0.08, -0.05, 0.04)),
             identity=((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))


def curved(xn, yn):
    """The surface's depth over A's normalised image coordinates."""
    return 1.0 + 0.25 * xn - 0.18 * yn + 0.12 * np.sin(5 * xn) * np.cos(4 * yn) + 0.3 * xn * yn


def _gap_curved(P):
    return P[2] - curved(P[0] / P[2], P[1] / P[2])


def _gap_plane(P):
    return P[2] - (1.0 + 0.2 * P[0] - 0.1 * P[1])


def true_pose(name):
    """-> (R, t) float64 of the pose B -> A: R = exp([omega]x)."""
    om, t = POSES[name]
    R, _, _ = registration.compose(np.concatenate([om, np.zeros(3)]), np.eye(3), np.zeros(3))
    return R, np.asarray(t, np.float64)


def _rays(size=SIZE, cam=CAM, scale=1):
    H, W = size
    yn = ((np.arange(H) / scale - cam.cy) / cam.fy)[:, None] + np.zeros((1, W))
    xn = ((np.arange(W) / scale - cam.cx) / cam.fx)[None, :] + np.zeros((H, 1))
    return xn, yn


def cast(gap, R, t, size=SIZE, scale=1, cam=CAM):
    """The depth a camera sees whose frame maps to A's by X_A = R X + t: per ray, 80 steps of bisection on z in [0.3, 3] of
    gap(R (z d) + t), d = (xn, yn, 1) - negative in front of the surface, positive behind it."""
    xn, yn = _rays(size, cam, scale)
    d = np.stack([xn, yn, np.ones_like(xn)])
    lo, hi = np.full(xn.shape, 0.3), np.full(xn.shape, 3.0)
    at = lambda z: gap(np.einsum("ij,jhw->ihw", R, d * z) + t[:, None, None])
    assert (at(lo) < 0).all() and (at(hi) > 0).all()
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        behind = at(mid) > 0
        hi, lo = np.where(behind, mid, hi), np.where(behind, lo, mid)
    return 0.5 * (lo + hi)


_SCENES = {}


def scene(name="small", noisy=False, plane=False, scale=1):
    """-> dict(src = view B, dst = view A (the view dicts of registration.register), R, t = the true pose B -> A).  noisy: one
    default_rng(3) draws, for A and then for B, 5 mm of noise and then a 30 % dropout (depth 0).  scale: B on a lattice `scale`
    times finer than its pixels (109 x 157 at 3)."""
    key = (name, noisy, plane, scale)
    if key not in _SCENES:
        gap = _gap_plane if plane else _gap_curved
        R, t = true_pose(name)
        a = cast(gap, np.eye(3), np.zeros(3))
        size_b = tuple((n - 1) * scale + 1 for n in SIZE)
        b = cast(gap, R, t, size_b, scale)
        if not plane:
            assert np.abs(a - curved(*_rays())).max() < 1e-12
        if noisy:
            rng = np.random.default_rng(3)
            for d in (a, b):
                d += 0.005 * rng.standard_normal(d.shape)
                d[rng.random(d.shape) < 0.3] = 0
        view = lambda d, k: dict(depth=d.astype(_F), weight=None, cam=CAM, scale=k, window_origin=(0, 0))
        _SCENES[key] = dict(src=view(b, scale), dst=view(a, 1), R=R, t=t)
    return _SCENES[key]


def other_source(size):
    """View B of the "small" scene through a camera of another size over the same field of view: (1, N) is one row of N samples
    through the middle of the image, (147, 147) more samples than one pass of the kernels' grid.  -> the view dict."""
    key = ("other", size)
    if key not in _SCENES:
        H, W = size
        fy, cy = (CAM.fy, 0.0) if H == 1 else (CAM.fy * (H - 1) / (SIZE[0] - 1), CAM.cy * (H - 1) / (SIZE[0] - 1))
        fx, cx = (CAM.fx, 0.0) if W == 1 else (CAM.fx * (W - 1) / (SIZE[1] - 1), CAM.cx * (W - 1) / (SIZE[1] - 1))
        cam = camera.Pinhole(fy, fx, cy, cx)
        R, t = true_pose("small")
        _SCENES[key] = dict(depth=cast(_gap_curved, R, t, size, 1, cam).astype(_F), weight=None, cam=cam, scale=1, window_origin=(0, 0))
    return _SCENES[key]


def weights(shape, seed):
    """Random weights 0.25 + 0.75 u, float32."""
    return (0.25 + 0.75 * np.random.default_rng(seed).random(shape)).astype(_F)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a
