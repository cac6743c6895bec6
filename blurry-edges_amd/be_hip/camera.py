"""Host geometry of the forward reprojection (native.unproject, native.reproject, DepthPipeline.point_cloud / reproject): pinhole
intrinsics, rigid poses, and the numpy float32 statement of what k_unproject, k_splat_zbuf and k_resolve_zbuf compute, operation
by operation - to those kernels what tiling.point_run is to the covering rule.  Pure numpy and python; nothing here needs a GPU.

Conventions: pixel centres at the integers (sample_at's), (y, x) order for everything that indexes an image and (X, Y, Z) for
points in space, Z along the optical axis; a pose maps the source camera's frame to the target's, X' = R X + t.
"""
from __future__ import annotations

import numpy as np

_F = np.float32


class Pinhole:
    """fy, fx: focal lengths in pixels; cy, cx: the principal point.  Pinhole(K) takes a 3x3 matrix [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]."""
    __slots__ = ("fy", "fx", "cy", "cx")

    def __init__(self, fy, fx=None, cy=None, cx=None):
        if fx is None and cy is None and cx is None:
            K = np.asarray(fy, np.float64)
            if K.shape == (4,):
                fy, fx, cy, cx = K
            elif K.shape == (3, 3):
                if K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
                    raise ValueError(f"Pinhole: K must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew), got {K.tolist()}")
                fy, fx, cy, cx = K[1, 1], K[0, 0], K[1, 2], K[0, 2]
            else:
                raise ValueError(f"Pinhole: give (fy, fx, cy, cx) or a 3x3 K matrix, got an array of shape {K.shape}")
        elif fx is None or cy is None or cx is None:
            raise ValueError("Pinhole: give all of (fy, fx, cy, cx), or a 3x3 K matrix alone")
        self.fy, self.fx, self.cy, self.cx = float(fy), float(fx), float(cy), float(cx)
        if not all(np.isfinite(v) for v in self.tuple()) or self.fy <= 0 or self.fx <= 0:
            raise ValueError(f"Pinhole: focal lengths must be finite and > 0 and the principal point finite, got {self.tuple()}")

    @classmethod
    def of(cls, cam_params, mag, H, W):
        """The camera the pipeline's pixels belong to: the sensor sits s behind the lens and the pipeline sees pixels of pitch
        pixel_pitch * mag, so fy = fx = s / (pixel_pitch * mag) (python float64; 4709.9 px at the defaults), and the optical
        axis goes through the middle of the H x W image."""
        f = cam_params["s"] / (cam_params["pixel_pitch"] * mag)
        return cls(f, f, (H - 1) / 2, (W - 1) / 2)

    @property
    def focal_px(self):
        return self.fx

    def tuple(self):
        return (self.fy, self.fx, self.cy, self.cx)

    def f32(self):
        """The four float32 numbers the kernels take, (fy, fx, cy, cx)."""
        return np.array(self.tuple(), _F)

    def K(self):
        return np.array([[self.fx, 0, self.cx], [0, self.fy, self.cy], [0, 0, 1]], np.float64)

    def __eq__(self, other):
        return isinstance(other, Pinhole) and self.tuple() == other.tuple()

    def __repr__(self):
        return f"Pinhole(fy={self.fy!r}, fx={self.fx!r}, cy={self.cy!r}, cx={self.cx!r})"


def as_pinhole(cam, who="camera"):
    """A Pinhole, (fy, fx, cy, cx) or a 3x3 K -> Pinhole."""
    if isinstance(cam, Pinhole):
        return cam
    try:
        return Pinhole(cam)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{who}: {e}") from None


def pose(R=None, t=None):
    """R [3,3] and t [3] (either may be None: the identity, zero), or one 4x4 matrix [[R, t], [0, 1]] as R -> the 12 float32
    numbers the kernels take: R row-major, then t.  X' = R X + t maps the source camera's frame to the target's.  An R that is not
    a rotation (R R^T = I and det R = +1, to 1e-5) is rejected."""
    if R is not None and np.shape(R) == (4, 4):
        if t is not None:
            raise ValueError("pose: a 4x4 matrix holds the translation; pass it without t")
        M = np.asarray(R, np.float64)
        if not np.allclose(M[3], [0, 0, 0, 1], rtol=0, atol=1e-12):
            raise ValueError(f"pose: the last row of a 4x4 pose must be (0, 0, 0, 1), got {M[3].tolist()}")
        R, t = M[:3, :3], M[:3, 3]
    R = np.eye(3) if R is None else np.asarray(R, np.float64)
    t = np.zeros(3) if t is None else np.asarray(t, np.float64).reshape(-1)
    if R.shape != (3, 3) or t.shape != (3,):
        raise ValueError(f"pose: R must be [3,3] and t [3] (or R one 4x4 matrix), got {R.shape} and {t.shape}")
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        raise ValueError("pose: R and t must be finite")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-5 or abs(np.linalg.det(R) - 1) > 1e-5:
        raise ValueError("pose: R is not a rotation (R R^T = I and det R = +1 to 1e-5)")
    return np.concatenate([R.reshape(9), t]).astype(_F)


def as_pose(p, who="pose"):
    """None (identity), the 12 numbers of pose(), a 3x4 [R | t] or a 4x4 matrix -> the 12 float32 numbers, checked by pose()."""
    if p is None:
        return pose()
    a = np.asarray(p, np.float64)
    try:
        if a.shape == (12,):
            return pose(a[:9].reshape(3, 3), a[9:])
        if a.shape == (3, 4):
            return pose(a[:, :3], a[:, 3])
        if a.shape == (4, 4):
            return pose(a)
    except ValueError as e:
        raise ValueError(f"{who}: {e}") from None
    raise ValueError(f"{who}: expected 12 numbers (R row-major, then t), a 3x4 or a 4x4 matrix, got shape {a.shape}")


def check_size(who, size, max_side, wording, max_pixels=None):
    """size = (Ho, Wo) of a target image -> (Ho, Wo) as ints: whole numbers (no bools) in [1, max_side] whose product is at most
    max_pixels (None: no bound).  `wording` is the sentence of the refusal, "size must be (Ho, Wo), ..": the caller states its bound."""
    try:
        Ho, Wo = size
        ok = all(not isinstance(v, bool) and int(v) == v and 1 <= v <= max_side for v in (Ho, Wo))
        ok = ok and (max_pixels is None or Ho * Wo <= max_pixels)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{who}: {wording}, got {size!r}")
    return int(Ho), int(Wo)


def check_number(who, name, v, lo=0.0, hi=np.inf, lo_open=False, hi_closed=False):
    """v -> float(v), a finite number with lo <= v < hi (lo_open: lo < v; hi_closed: v <= hi); anything else - a string, None, NaN,
    an infinity - is refused as "{who}: {name} must be a finite number >= {lo}"."""
    try:
        v = float(v)
    except (TypeError, ValueError):
        v = np.nan
    if not (lo < v if lo_open else lo <= v) or not (v <= hi if hi_closed else v < hi) or v == np.inf:   # NaN fails
        raise ValueError(f"{who}: {name} must be a finite number {'>' if lo_open else '>='} {lo:g}"
                         + ("" if hi == np.inf else f" and {'<=' if hi_closed else '<'} {hi:g}"))
    return v


def _geometry(dtype, cam_src, cam_dst, pose12):
    s = np.asarray(as_pinhole(cam_src).f32(), dtype)
    d = np.asarray(as_pinhole(cam_dst).f32(), dtype)
    return s, d, np.asarray(as_pose(pose12), dtype)


def project(depth, cam_src, cam_dst, pose12=None, scale=1, window_origin=(0, 0), dtype=np.float32):
    """The arithmetic of be_reproject.hip on depth [Hs,Ws], one rounding of `dtype` per operation, in the kernels' order ->
    dict(xyz [3,Hs,Ws] = (Xd, Yd, Zd), u, v [Hs,Ws] = the target column / row, fu, fv = the same rounded, as floats, z_ok [Hs,Ws] = Z > 0 and
    finite).  Sample (iy, ix) sits at (top + iy / scale, left + ix / scale).  The cameras and the pose are the float32 numbers the
    kernels take whatever dtype is: with dtype=np.float64 this is the same function of the same inputs in double precision."""
    T = np.dtype(dtype).type
    (fy, fx, cy, cx), (fyd, fxd, cyd, cxd), p = _geometry(T, cam_src, cam_dst, pose12)
    Z = np.asarray(depth, _F).astype(T)
    if Z.ndim != 2:
        raise ValueError(f"project: depth must be [Hs,Ws], got {Z.shape}")
    top, left = window_origin
    k = T(scale)
    with np.errstate(all="ignore"):
        y = (T(top) + np.arange(Z.shape[0]).astype(T) / k)[:, None]
        x = (T(left) + np.arange(Z.shape[1]).astype(T) / k)[None, :]
        xn = (x - cx) / fx
        yn = (y - cy) / fy
        X = xn * Z
        Y = yn * Z
        Xd = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
        Yd = ((p[3] * X + p[4] * Y) + p[5] * Z) + p[10]
        Zd = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
        u = (fxd * Xd) / Zd + cxd
        v = (fyd * Yd) / Zd + cyd
        fu = np.floor(u + T(0.5))
        fv = np.floor(v + T(0.5))
        z_ok = (Z > 0) & np.isfinite(Z)
    assert Xd.dtype == T and fu.dtype == T
    return dict(xyz=np.stack([Xd, Yd, Zd]), u=u, v=v, fu=fu, fv=fv, z_ok=z_ok)


def project_f32(depth, cam_src, cam_dst, pose12=None, scale=1, window_origin=(0, 0)):
    """project in float32: the host statement of the kernels' arithmetic, bit for bit."""
    return project(depth, cam_src, cam_dst, pose12, scale, window_origin, np.float32)


def unproject_f32(depth, cam_src, pose12=None, scale=1, window_origin=(0, 0)):
    """The host statement of k_unproject: xyz [3,Hs,Ws] float32, 0 where Z is not a finite number > 0."""
    p = project_f32(depth, cam_src, cam_src, pose12, scale, window_origin)
    return np.where(p["z_ok"][None], p["xyz"], _F(0))


def taking_part(proj, size, near=1e-3):
    """Which samples of project()'s result splat: Z valid, near < Zd < inf (float32), and the rounded target inside size = (Ho, Wo)."""
    Ho, Wo = size
    T = proj["fu"].dtype.type
    with np.errstate(invalid="ignore"):
        return (proj["z_ok"] & (proj["xyz"][2] > T(_F(near))) & (proj["xyz"][2].astype(_F) < _F(np.inf)) & (proj["fu"] >= 0) & (proj["fu"] < T(Wo))
                & (proj["fv"] >= 0) & (proj["fv"] < T(Ho)))


def splat(proj, size, near=1e-3, feat=None):
    """The z-buffer over project()'s result: per target pixel the minimum of (bits of float32 Zd) << 32 | source linear index
    over the samples that take part (np.minimum.at on uint64 keys) -> dict(depth [Ho,Wo] float32, index [Ho,Wo] int32, valid,
    feat [C,Ho,Wo] or None, taking_part [Hs,Ws]); +0 / -1 / False / +0 where nothing landed."""
    Ho, Wo = size
    part = taking_part(proj, size, near)
    src = np.flatnonzero(part.ravel())
    zd = np.ascontiguousarray(proj["xyz"][2].astype(_F)).ravel()[src]
    keys = (zd.view(np.uint32).astype(np.uint64) << np.uint64(32)) | src.astype(np.uint64)
    dst = proj["fv"].ravel()[src].astype(np.int64) * Wo + proj["fu"].ravel()[src].astype(np.int64)
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    zbuf = np.full(Ho * Wo, empty, np.uint64)
    np.minimum.at(zbuf, dst, keys)
    hit = zbuf != empty
    index = np.where(hit, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
    depth = np.where(hit, (zbuf >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(_F)
    out = None
    if feat is not None:
        f = np.asarray(feat, _F).reshape(len(feat), -1)
        out = np.where(hit[None], f[:, np.where(hit, index, 0)], _F(0)).reshape(-1, Ho, Wo)
    return dict(depth=depth.reshape(Ho, Wo), index=index.reshape(Ho, Wo), valid=hit.reshape(Ho, Wo), feat=out, taking_part=part)


def splat_f32(depth, cam_src, cam_dst, pose12, size, feat=None, near=1e-3, scale=1, window_origin=(0, 0)):
    """The host statement of be_reproject_f32: splat over project_f32."""
    return splat(project_f32(depth, cam_src, cam_dst, pose12, scale, window_origin), size, near, feat)
