"""The contract of the truncated signed distance volume (native.tsdf_volume / tsdf_integrate / tsdf_raycast, DepthPipeline.integrate
/ raycast) as pure numpy: to k_tsdf_integrate, k_tsdf_mean and k_tsdf_raycast of csrc/be_tsdf.hip what fusion.fuse is to
be_fuse.hip.  Nothing here needs a GPU.

Conventions: points are (X, Y, Z), images (y, x).  A volume of dims = (Nz, Ny, Nx) voxels keeps its tensors as [Nz,Ny,Nx], x
fastest; origin = (X0, Y0, Z0) is the centre of voxel (0, 0, 0), voxel = (sX, sY, sZ) the spacing per axis, trunc the truncation
distance, all in metres in the volume's frame.  A view's pose maps the view's frame to the volume's (X' = R X + t, as in fuse).

State: sw int32 [Nz,Ny,Nx] (sum of quantised weights), swd int64 [Nz,Ny,Nx], swf int64 [C,Nz,Ny,Nx]; all zero at the start.

integrate, one view into the sums, per voxel (iz, iy, ix), in `dtype` arithmetic with one rounding per written operation:

  centre    x = X0 + (float) ix * sX, y and z likewise
  q         the inverse pose (R^T, -R^T t), formed in float64 and rounded to 12 float32 numbers (inverse_pose)
  point     X = ((q0 x + q1 y) + q2 z) + q9, Y and Z with rows 1 and 2: the centre in the view's frame
  pixel     u = (fx X) / Z + cx, v = (fy Y) / Z + cy
  sample    su = floorf((u - left) * k + 0.5), sv = floorf((v - top) * k + 0.5): the nearest sample of the view's lattice (sample
            (iy, ix) of scale k and window origin (top, left) sits at (top + iy / k, left + ix / k))
  takes part iff Z > near; 0 <= su < Ws and 0 <= sv < Hs (tested in float before any conversion: NaN fails); the sample's depth Zq
            is a finite number > 0; its weight w is > 0 (no weights: 1); sdf = Zq - Z >= -trunc; and
            wq = floorf(min(w, 16) * 256 + 0.5) != 0
  adds      dq = floorf(min(sdf, trunc) / trunc * 32768 + 0.5);  sw += wq;  swd += wq * dq;  swf[c] += wq * fq[c] with fusion's
            fq = floorf(clamp(f, -2048, 2048) * 65536 + 0.5) (NaN counts as 0)

Every sum is an integer owned by one voxel, so the result depends neither on the order of the views nor on how they are grouped
into calls.  The sums are exact below 2^19 views (wq <= 2^12 in an int32; |wq dq| <= 2^27 and |wq fq| <= 2^39 in an int64); that
limit is documented, not checked.

mean: D = (float)((double) swd / (double) sw * 2^-15) in [-1, 1] (units of trunc), W = (float)(sw * 2^-8),
Fm[c] = (float)((double) swf[c] / (double) sw * 2^-16); all +0 where sw == 0.

raycast, per pixel (v, u) of the target camera under `pose` (camera frame -> volume frame), in `dtype` arithmetic:

  ray       xn = (u - cx) / fx, yn = (v - cy) / fy
  samples   z_i = z_near + (float) i * step, i = 0 .. n - 1, n = ceil((z_far - z_near) / step) + 1 on the host, at most 4096
  point     (xn z, yn z, z) through the pose in the bracket form above -> P
  grid      g = (P - origin) / voxel per axis, i0 = floorf(g), f = g - i0
  valid     iff 0 <= i0 <= N - 2 on every axis (in float) and all 8 corners have W > 0
  F         the trilinear value of D, written a + t * (b - a), along x, then y, then z; Wt and the channels likewise
  hit       the first step whose previous and current samples are both valid with F_prev > 0 and F_cur <= 0:
            a = F_prev / (F_prev - F_cur), depth = z_prev + (z_cur - z_prev) * a, weight = Wt_prev + a * (Wt_cur - Wt_prev),
            channels likewise.  An invalid sample resets the bracket; a back-to-front crossing is walked through; no hit: +0 / False

Indices are clamped (where(ok, i, 0)) before every gather.  depth is Z in the target camera's frame (z_near > 0, so a hit's depth
is > 0), on the pixels of cam_dst: registration.normals_f32 / native.depth_normals take it as it is."""
from __future__ import annotations

import math

import numpy as np

from . import camera, fusion

_F = np.float32
MAX_DIM, MAX_TRUNC, MAX_STEPS = 1024, 4.0, 4096
MAX_CHANNELS = 64                                                       # BE_FUSE_MAX_CHANNELS
W_MAX = 16.0


def _triple(who, name, v, integer=False):
    try:
        a = [x for x in v]
        if len(a) != 3:
            raise TypeError
        if integer:
            if any(isinstance(x, bool) or int(x) != x for x in a):
                raise TypeError
            return tuple(int(x) for x in a)
        return tuple(float(_F(x)) for x in a)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{who}: {name} must hold three {'integers' if integer else 'numbers'}, got {v!r}") from None


def check_params(who, dims, origin, voxel, trunc, C=0):
    """The description of a volume, validated -> (dims = (Nz, Ny, Nx) ints, origin, voxel = python floats holding float32 values
    (X, Y, Z order), trunc likewise, C)."""
    dims = _triple(who, "dims = (Nz, Ny, Nx)", dims, integer=True)
    if not all(1 <= n <= MAX_DIM for n in dims) or dims[0] * dims[1] * dims[2] >= 1 << 31:
        raise ValueError(f"{who}: each of dims must be in [1, {MAX_DIM}] and their product < 2^31, got {dims}")
    origin = _triple(who, "origin = (X0, Y0, Z0)", origin)
    voxel = _triple(who, "voxel = (sX, sY, sZ)", voxel)
    if not all(math.isfinite(x) for x in origin):
        raise ValueError(f"{who}: origin must be finite, got {origin}")
    if not all(math.isfinite(x) and x > 0 for x in voxel):
        raise ValueError(f"{who}: voxel must be three finite numbers > 0 (metres per axis), got {voxel}")
    try:
        trunc = float(_F(trunc))
    except (TypeError, ValueError):
        trunc = -1.0
    if not 0 < trunc <= MAX_TRUNC:                                      # NaN fails
        raise ValueError(f"{who}: trunc must be a finite number of metres in (0, {MAX_TRUNC:g}]")
    if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or not 0 <= C <= MAX_CHANNELS:
        raise ValueError(f"{who}: C must be an integer in [0, {MAX_CHANNELS}], got {C!r}")
    return dims, origin, voxel, trunc, int(C)


def check_raycast(who, z_range, step, trunc):
    """-> (z_near, z_far, step as python floats holding float32 values, n): step None means trunc / 4."""
    try:
        z_near, z_far = (float(_F(z)) for z in z_range)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: z_range must be (z_near, z_far) in metres, got {z_range!r}") from None
    if not 0 < z_near < z_far < float("inf"):
        raise ValueError(f"{who}: z_range must satisfy 0 < z_near < z_far < inf, got {z_range!r}")
    try:
        step = float(_F(trunc) / _F(4)) if step is None else float(_F(step))
    except (TypeError, ValueError):
        step = -1.0
    if not 0 < step < float("inf"):
        raise ValueError(f"{who}: step must be a finite number of metres > 0")
    n = math.ceil((z_far - z_near) / step) + 1
    if n > MAX_STEPS:
        raise ValueError(f"{who}: {n} steps from {z_near:g} to {z_far:g} by {step:g}; at most {MAX_STEPS}")
    return z_near, z_far, step, n


class Volume:
    """The description (dims = (Nz, Ny, Nx), origin, voxel, trunc, C) and the three sums sw, swd, swf - numpy arrays here, tensors on
    the GPU when native.tsdf_volume made it.  Without arrays given, a numpy volume of zeros."""
    __slots__ = ("dims", "origin", "voxel", "trunc", "C", "sw", "swd", "swf", "meta")

    def __init__(self, dims, origin, voxel, trunc, C=0, sw=None, swd=None, swf=None):
        self.dims, self.origin, self.voxel, self.trunc, self.C = check_params("Volume", dims, origin, voxel, trunc, C)
        self.meta = {}                                                  # a caller's notes (DepthPipeline.integrate: the channel layout)
        self.sw = np.zeros(self.dims, np.int32) if sw is None else sw
        self.swd = np.zeros(self.dims, np.int64) if swd is None else swd
        self.swf = np.zeros((self.C,) + self.dims, np.int64) if swf is None else swf
        if tuple(self.sw.shape) != self.dims or tuple(self.swd.shape) != self.dims or tuple(self.swf.shape) != (self.C,) + self.dims:
            raise ValueError(f"Volume: sw, swd must be {self.dims} and swf {(self.C,) + self.dims}, got {tuple(self.sw.shape)}, "
                             f"{tuple(self.swd.shape)}, {tuple(self.swf.shape)}")

    def description(self):
        return dict(dims=self.dims, origin=self.origin, voxel=self.voxel, trunc=self.trunc, C=self.C)

    def numpy(self):
        """A copy on the host with numpy sums (the volume itself when it already is one)."""
        if isinstance(self.sw, np.ndarray):
            return self
        return Volume(self.dims, self.origin, self.voxel, self.trunc, self.C, self.sw.cpu().numpy(), self.swd.cpu().numpy(),
                      self.swf.cpu().numpy())

    def __repr__(self):
        return f"Volume(dims={self.dims}, origin={self.origin}, voxel={self.voxel}, trunc={self.trunc}, C={self.C})"


def inverse_pose(pose12):
    """The 12 float32 numbers of a pose (camera.as_pose) -> those of its inverse, X = R^T X' - R^T t: formed in float64 from the
    float32 numbers, each -(R^T t) component summed left to right, and rounded to float32 once."""
    p = [float(x) for x in camera.as_pose(pose12)]
    q = [p[3 * j + i] for i in range(3) for j in range(3)]
    q += [-((p[i] * p[9] + p[3 + i] * p[10]) + p[6 + i] * p[11]) for i in range(3)]
    return np.array(q, np.float64).astype(_F)


def quantise_weight(w, T=_F):
    """w -> int64 wq = floorf(min(w, 16) * 256 + 0.5) where w > 0, else 0 (NaN, 0, negatives)."""
    w = np.asarray(w, T)
    with np.errstate(invalid="ignore"):
        ok = w > 0
        q = np.floor(np.minimum(np.where(ok, w, T(0)), T(W_MAX)) * T(256) + T(0.5))
    return q.astype(np.int64)


def integrate_view(vol, view, near=1e-3, dtype=np.float32):
    """One view dict (fusion.VIEW_KEYS, numpy arrays) into the numpy volume `vol`, in place -> the number of voxels that took part."""
    T = np.dtype(dtype).type
    Nz, Ny, Nx = vol.dims
    depth = np.asarray(view["depth"], _F)
    if depth.ndim != 2:
        raise ValueError(f"integrate: depth must be [Hs,Ws], got {depth.shape}")
    Hs, Ws = depth.shape
    weight, feat = view.get("weight"), view.get("feat")
    if weight is not None and np.shape(weight) != depth.shape:
        raise ValueError(f"integrate: weight must be {depth.shape}, got {np.shape(weight)}")
    f = np.zeros((0, depth.size), _F) if feat is None else np.asarray(feat, _F).reshape(len(feat), -1)
    if f.shape != (vol.C, depth.size):
        raise ValueError(f"integrate: feat must be [{vol.C},{Hs},{Ws}] (the volume's C), got {np.shape(feat)}")
    fy, fx, cy, cx = np.asarray(camera.as_pinhole(view["cam_src"]).f32(), T)
    q = inverse_pose(view.get("pose")).astype(T)
    k = T(view.get("scale", 1))
    top, left = (T(v) for v in view.get("window_origin", (0, 0)))
    X0, Y0, Z0 = (T(v) for v in vol.origin)
    sX, sY, sZ = (T(v) for v in vol.voxel)
    trunc = T(vol.trunc)
    with np.errstate(all="ignore"):
        x = (X0 + np.arange(Nx).astype(T) * sX)[None, None, :]
        y = (Y0 + np.arange(Ny).astype(T) * sY)[None, :, None]
        z = (Z0 + np.arange(Nz).astype(T) * sZ)[:, None, None]
        X = ((q[0] * x + q[1] * y) + q[2] * z) + q[9]
        Y = ((q[3] * x + q[4] * y) + q[5] * z) + q[10]
        Z = ((q[6] * x + q[7] * y) + q[8] * z) + q[11]
        u = (fx * X) / Z + cx
        v = (fy * Y) / Z + cy
        su = np.floor((u - left) * k + T(0.5))
        sv = np.floor((v - top) * k + T(0.5))
        assert su.dtype == T and Z.dtype == T
        part = (Z > T(_F(near))) & (su >= 0) & (su < T(Ws)) & (sv >= 0) & (sv < T(Hs))
        j = np.where(part, sv, T(0)).astype(np.int64) * Ws + np.where(part, su, T(0)).astype(np.int64)
        Zq = depth.ravel()[j].astype(T)
        part &= (Zq > 0) & np.isfinite(Zq)
        w = np.ones(j.shape, T) if weight is None else np.asarray(weight, _F).ravel()[j].astype(T)
        part &= w > 0
        sdf = Zq - Z
        part &= sdf >= -trunc
        wq = quantise_weight(w, T)
        part &= wq != 0
        dq = np.floor(np.minimum(np.where(part, sdf, T(0)), trunc) / trunc * T(32768) + T(0.5))
    assert dq.dtype == T
    wq = np.where(part, wq, 0)
    vol.sw += wq.astype(np.int32)
    vol.swd += wq * dq.astype(np.int64)
    for c in range(vol.C):
        vol.swf[c] += wq * fusion.quantise_feat(f[c][j])
    return int(part.sum())


def integrate(vol, views, near=1e-3, dtype=np.float32):
    """Every view of `views` into the numpy volume `vol`, in place -> vol."""
    for view in views:
        integrate_view(vol, view, near, dtype)
    return vol


def mean(vol):
    """-> (D [Nz,Ny,Nx] float32 in units of trunc, W [Nz,Ny,Nx] float32, Fm [C,Nz,Ny,Nx] float32); +0 where sw == 0."""
    sw, swd, swf = (np.asarray(a) for a in (vol.sw, vol.swd, vol.swf))
    any_ = sw != 0
    with np.errstate(invalid="ignore", divide="ignore"):
        D = np.where(any_, (swd.astype(np.float64) / sw.astype(np.float64) * 2.0 ** -15).astype(_F), _F(0))
        W = (sw.astype(np.float64) * 2.0 ** -8).astype(_F)
        Fm = np.where(any_[None], (swf.astype(np.float64) / sw.astype(np.float64)[None] * 2.0 ** -16).astype(_F), _F(0))
    return D, W, Fm


def _locate(vol, T, p, xn, yn, z):
    """The grid position of the camera point (xn z, yn z, z) -> (ok, linear index of corner (0, 0, 0) clamped to 0, fx, fy, fz)."""
    Nz, Ny, Nx = vol.dims
    (X0, Y0, Z0), (sX, sY, sZ) = (tuple(T(v) for v in t) for t in (vol.origin, vol.voxel))
    X, Y = xn * z, yn * z
    Px = ((p[0] * X + p[1] * Y) + p[2] * z) + p[9]
    Py = ((p[3] * X + p[4] * Y) + p[5] * z) + p[10]
    Pz = ((p[6] * X + p[7] * Y) + p[8] * z) + p[11]
    gx, gy, gz = (Px - X0) / sX, (Py - Y0) / sY, (Pz - Z0) / sZ
    ix, iy, iz = np.floor(gx), np.floor(gy), np.floor(gz)
    ok = (ix >= 0) & (ix <= T(Nx - 2)) & (iy >= 0) & (iy <= T(Ny - 2)) & (iz >= 0) & (iz <= T(Nz - 2))
    i = lambda a: np.where(ok, a, T(0)).astype(np.int64)
    return ok, (i(iz) * Ny + i(iy)) * Nx + i(ix), gx - ix, gy - iy, gz - iz


def _corners(vol, ok, j):
    Nz, Ny, Nx = vol.dims
    return [np.where(ok, j + (dz * Ny + dy) * Nx + dx, 0) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]


def _trilinear(a, T, corners, fx, fy, fz):
    c = [a[k].astype(T) for k in corners]                               # order: (dz, dy, dx) = 000, 001, 010, 011, 100, ..
    c00, c01, c10, c11 = (c[2 * m] + fx * (c[2 * m + 1] - c[2 * m]) for m in range(4))
    c0, c1 = c00 + fy * (c01 - c00), c10 + fy * (c11 - c10)
    return c0 + fz * (c1 - c0)


def raycast(vol, cam_dst, pose, size, z_range, step=None, dtype=np.float32, field=None):
    """The ray cast of the head of this module out of the numpy volume `vol` -> dict(depth [Ho,Wo] float32, valid bool, weight
    float32, feat [C,Ho,Wo] float32 or None).  field: mean(vol) when the caller already holds it."""
    T = np.dtype(dtype).type
    z_near, z_far, step, n = check_raycast("raycast", z_range, step, vol.trunc)
    Ho, Wo = size
    D, W, Fm = mean(vol) if field is None else field
    D, W, Fm = D.reshape(-1), W.reshape(-1), Fm.reshape(vol.C, D.size)
    fy, fx, cy, cx = np.asarray(camera.as_pinhole(cam_dst).f32(), T)
    p = np.asarray(camera.as_pose(pose), T)
    z_near, step = T(z_near), T(step)
    No = Ho * Wo
    with np.errstate(all="ignore"):
        xn = np.tile((np.arange(Wo).astype(T) - cx) / fx, Ho)
        yn = np.repeat((np.arange(Ho).astype(T) - cy) / fy, Wo)
        hit = np.full(No, -1, np.int64)
        a_hit, depth = np.zeros(No, T), np.zeros(No, T)
        prev_ok, F_prev, z_prev = np.zeros(No, bool), np.zeros(No, T), z_near

        def sample(z, sel):
            ok, j, gx, gy, gz = _locate(vol, T, p, xn[sel], yn[sel], z)
            corners = _corners(vol, ok, j)
            for k in corners:
                ok = ok & (W[k] > 0)
            corners = [np.where(ok, k, 0) for k in corners]
            return ok, corners, gx, gy, gz

        everything = slice(None)
        for i in range(n):
            z = z_near + T(i) * step
            ok, corners, gx, gy, gz = sample(z, everything)
            F = _trilinear(D, T, corners, gx, gy, gz)
            new = (hit < 0) & prev_ok & ok & (F_prev > 0) & (F <= 0)
            a = F_prev / (F_prev - F)
            a_hit = np.where(new, a, a_hit)
            depth = np.where(new, z_prev + (z - z_prev) * a, depth)
            hit = np.where(new, i, hit)
            prev_ok, F_prev, z_prev = ok, F, z
        assert depth.dtype == T
        sel = np.flatnonzero(hit >= 0)
        weight, feat = np.zeros(No, T), np.zeros((vol.C, No), T)
        if sel.size:
            a = a_hit[sel]
            z_cur = z_near + hit[sel].astype(T) * step
            z_prv = z_near + (hit[sel] - 1).astype(T) * step
            _, c0, gx0, gy0, gz0 = sample(z_prv, sel)
            _, c1, gx1, gy1, gz1 = sample(z_cur, sel)
            for out, src in [(weight, W)] + [(feat[c], Fm[c]) for c in range(vol.C)]:
                v0, v1 = _trilinear(src, T, c0, gx0, gy0, gz0), _trilinear(src, T, c1, gx1, gy1, gz1)
                out[sel] = v0 + a * (v1 - v0)
    return dict(depth=depth.astype(_F).reshape(Ho, Wo), valid=(hit >= 0).reshape(Ho, Wo), weight=weight.astype(_F).reshape(Ho, Wo),
                feat=feat.astype(_F).reshape(vol.C, Ho, Wo) if vol.C else None)
