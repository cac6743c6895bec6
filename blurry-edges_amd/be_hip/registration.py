"""Depth registration (native.depth_normals, native.icp_linearize, native.register_depth, DepthPipeline.normals / register): the
pose between two views from their depth maps by point-to-plane ICP.  This module is the numpy statement of the two kernels of
csrc/be_register.hip, operation by operation - to them what camera.splat is to be_reproject.hip - and the host loop (solve,
compose, repeat) that the GPU path runs too.  Pure numpy; nothing here needs a GPU.

A view is a dict(depth [H,W] float32, weight [H,W] or None, cam, scale, window_origin), shaped like fusion's views; the target's
scale is 1 (its samples are the pixels of its camera).  A pose maps the source frame to the target's, X' = R X + t (camera.pose).

normals   P(y, x) is the unprojection of a good pixel (depth a finite number > 0; camera.project_f32 under the identity pose).  Along
          x the neighbour at x + r counts when it is inside, good and |Z(x + r) - Z(x)| <= max_jump * r; du = P(x + r) - P(x - r)
          when both neighbours count, the one-sided difference against P(x) when one does; dv likewise along y; n = du x dv,
          normalised, turned to face the camera (n . P <= 0).  Invalid pixels hold (+0, +0, +0).
rows      source sample i projects to P = (Xd, Yd, Zd) and the target pixel j = (fv, fu) (camera.project, camera.taking_part);
          Zq = depth_d[j] must be good and n = normal_d[:, j] non-zero; Q = (((fu - cxd) / fxd) Zq, ((fv - cyd) / fyd) Zq, Zq);
          D = P - Q must satisfy D . D <= max_dist^2; w = w_s[i] w_d[j] must satisfy 0 < w < inf; r = n . D; with huber > 0 and
          |r| > huber, w = w (huber / |r|); J = (P x n, n) is the derivative of r under the left-multiplied twist
          P' = P + omega x P + v.  All float32, one rounding per operation, in the order written here.
sums      the 8 floats J[0..5], r, w as doubles; 30 terms, each multiplied left to right in double: w J[a] J[b] for a <= b (21,
          row-major upper triangle), w J[a] r (6), w r r, w and 1.  ordered_sum adds them in the kernels' order, a function of the
          number of samples alone: nblocks = min(ceil(Ns / 256), 64); thread t of T = 256 nblocks adds samples t, t + T, .. in
          increasing order; a wave folds its 64 lanes by v[l] += v[l + off] for off = 32, 16, .., 1; a workgroup adds its four
          waves as (w0 + w1) + (w2 + w3); one wave folds the nblocks partials (zero beyond them) the same way.
step      A x = -b with A from the 21 sums and b from the 6, damped as A + damping diag(A), in float64; x = (omega, v);
          R <- exp([omega]x) R, t <- exp([omega]x) t + v by Rodrigues' formula in float64.  Each iteration linearises at the pose
          rounded to the 12 float32 numbers the kernel takes.

With the same sums the loop is the same code on both sides: a GPU run and this statement give the same iterates bit for bit."""
from __future__ import annotations

import numpy as np

from . import camera

_F = np.float32
MAX_STEP, MAX_BLOCKS, TERMS = 8, 64, 30
VIEW_KEYS = ("depth", "weight", "cam", "scale", "window_origin")


def _integer(who, name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{who}: {name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def check_normals_params(who, step, max_jump):
    """-> (step, max_jump as float): step an integer in 1..8, max_jump (metres per pixel of step) finite and >= 0."""
    return _integer(who, "step", step, 1, MAX_STEP), camera.check_number(who, "max_jump", max_jump)


def check_linearize_params(who, near, max_dist, huber):
    """-> (near, max_dist, huber) as floats: all finite and >= 0."""
    return camera.check_number(who, "near", near), camera.check_number(who, "max_dist", max_dist), camera.check_number(who, "huber", huber)


def check_params(who, iters, damping, max_dist, huber, step, max_jump, near, tol):
    """The parameter checks native.register_depth and this statement share -> the checked values in the same order."""
    iters = _integer(who, "iters", iters, 0, 1000)
    damping, tol = camera.check_number(who, "damping", damping), camera.check_number(who, "tol", tol)
    near, max_dist, huber = check_linearize_params(who, near, max_dist, huber)
    step, max_jump = check_normals_params(who, step, max_jump)
    return iters, damping, max_dist, huber, step, max_jump, near, tol


def _shift(a, r, axis, fill):
    """b[.., x, ..] = a[.., x + r, ..] along `axis` (r of either sign), `fill` where x + r leaves the image."""
    out = np.full_like(a, fill)
    n = a.shape[axis]
    if abs(r) >= n:
        return out
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    src[axis] = slice(r, n) if r > 0 else slice(0, n + r)
    dst[axis] = slice(0, n - r) if r > 0 else slice(-r, n)
    out[tuple(dst)] = a[tuple(src)]
    return out


def normals_f32(depth, cam, step=3, max_jump=0.05, scale=1, window_origin=(0, 0)):
    """The host statement of k_depth_normals: depth [H,W] on the lattice (scale, window_origin) of `cam` -> normal [3,H,W] float32,
    bit for bit; (+0, +0, +0) where the pixel is invalid."""
    step, max_jump = check_normals_params("normals_f32", step, max_jump)
    Z = np.asarray(depth, _F)
    if Z.ndim != 2:
        raise ValueError(f"normals_f32: depth must be [H,W], got {Z.shape}")
    P = camera.project_f32(Z, cam, cam, None, scale, window_origin)["xyz"]
    jump = _F(max_jump) * _F(step)
    with np.errstate(all="ignore"):
        good = (Z > 0) & np.isfinite(Z)

        def diff(axis):
            Zp, Zm = _shift(Z, step, axis, _F(0)), _shift(Z, -step, axis, _F(0))
            cp = (Zp > 0) & np.isfinite(Zp) & (np.abs(Zp - Z) <= jump)
            cm = (Zm > 0) & np.isfinite(Zm) & (np.abs(Zm - Z) <= jump)
            a = np.where(cp[None], _shift(P, step, axis + 1, _F(0)), P)
            b = np.where(cm[None], _shift(P, -step, axis + 1, _F(0)), P)
            return a - b, cp | cm

        du, has_u = diff(1)
        dv, has_v = diff(0)
        nx = du[1] * dv[2] - du[2] * dv[1]
        ny = du[2] * dv[0] - du[0] * dv[2]
        nz = du[0] * dv[1] - du[1] * dv[0]
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        valid = good & has_u & has_v & (l > 0) & np.isfinite(l)
        n = np.stack([nx / l, ny / l, nz / l])
        s = (n[0] * P[0] + n[1] * P[1]) + n[2] * P[2]
        n = np.where((s > 0)[None], -n, n)
    assert n.dtype == _F
    return np.where(valid[None], n, _F(0))


def _view(who, v, need_normal=False):
    if not isinstance(v, dict) or "depth" not in v or "cam" not in v:
        raise ValueError(f"{who}: a view is a dict with the keys {VIEW_KEYS} (depth and cam at least)")
    unknown = [k for k in v if k not in VIEW_KEYS + ("normal",)]
    if unknown:
        raise ValueError(f"{who}: unknown keys {unknown}; a view holds {VIEW_KEYS}")
    if need_normal and v.get("normal") is None:
        raise ValueError(f"{who}: the target lacks ['normal'] (normals_f32 of its depth)")


def rows(src, dst, pose12, near=1e-3, max_dist=0.1, huber=0.0, dtype=np.float32):
    """The per-sample rows of the linearised point-to-plane step at pose12, one rounding of `dtype` per operation -> dict(rows
    [8,Ns] = J[0..5], r, w in `dtype`, 0 where the sample takes no part; ok [Ns]; j [Ns] = the target pixel, 0 where none).  dst
    holds `normal` [3,Hd,Wd] beside its depth.  The inputs are the float32 numbers the kernel takes whatever dtype is."""
    _view("linearize(src)", src)
    _view("linearize(dst)", dst, need_normal=True)
    near, max_dist, huber = check_linearize_params("linearize", near, max_dist, huber)
    T = np.dtype(dtype).type
    Zs = np.asarray(src["depth"], _F)
    Zd = np.asarray(dst["depth"], _F)
    if Zs.ndim != 2 or Zd.ndim != 2:
        raise ValueError(f"linearize: depths must be [H,W], got {Zs.shape} and {Zd.shape}")
    if dst.get("scale", 1) != 1 or tuple(dst.get("window_origin", (0, 0))) != (0, 0):
        raise ValueError("linearize: the target's samples are the pixels of its camera: scale 1 and window_origin (0, 0)")
    Hd, Wd = Zd.shape
    nrm = np.asarray(dst["normal"], _F).reshape(3, -1)
    if nrm.shape[1] != Zd.size:
        raise ValueError(f"linearize: normal must be [3,{Hd},{Wd}], got {np.shape(dst['normal'])}")
    proj = camera.project(Zs, src["cam"], dst["cam"], pose12, src.get("scale", 1), src.get("window_origin", (0, 0)), dtype=T)
    part = camera.taking_part(proj, (Hd, Wd), near).ravel()
    fyd, fxd, cyd, cxd = np.asarray(camera.as_pinhole(dst["cam"]).f32(), T)
    fu, fv = proj["fu"].ravel(), proj["fv"].ravel()
    Px, Py, Pz = (c.ravel() for c in proj["xyz"])
    with np.errstate(all="ignore"):
        j = np.where(part, fv, 0).astype(np.int64) * Wd + np.where(part, fu, 0).astype(np.int64)
        zq = Zd.ravel()[j]
        ok = part & (zq > 0) & np.isfinite(zq)
        zq = zq.astype(T)
        nx, ny, nz = (c[j].astype(T) for c in nrm)
        ok &= (nx != 0) | (ny != 0) | (nz != 0)
        Qx = ((fu - cxd) / fxd) * zq
        Qy = ((fv - cyd) / fyd) * zq
        Dx, Dy, Dz = Px - Qx, Py - Qy, Pz - zq
        dd = (Dx * Dx + Dy * Dy) + Dz * Dz
        md = T(_F(max_dist))
        ok &= dd <= md * md
        ws = T(1) if src.get("weight") is None else np.asarray(src["weight"], _F).ravel().astype(T)
        wd = T(1) if dst.get("weight") is None else np.asarray(dst["weight"], _F).ravel()[j].astype(T)
        w = np.broadcast_to(ws * wd, Px.shape)
        ok &= (w > 0) & (w.astype(_F) < _F(np.inf))
        r = (nx * Dx + ny * Dy) + nz * Dz
        if huber > 0:
            hb, a = T(_F(huber)), np.abs(r)
            w = np.where(a > hb, w * (hb / a), w)
        out = np.stack([Py * nz - Pz * ny, Pz * nx - Px * nz, Px * ny - Py * nx, nx, ny, nz, r, w])
    assert out.dtype == T
    return dict(rows=np.where(ok[None], out, T(0)), ok=ok, j=np.where(ok, j, 0))


def terms(rows8, ok):
    """rows [8,Ns] and ok [Ns] -> the 30 double terms per sample [30,Ns], each multiplied left to right; 0 where ok is false."""
    J = np.asarray(rows8[:6], np.float64)
    r, w = np.asarray(rows8[6], np.float64), np.asarray(rows8[7], np.float64)
    wJ = [w * J[a] for a in range(6)]
    out = [wJ[a] * J[b] for a in range(6) for b in range(a, 6)] + [wJ[a] * r for a in range(6)] + [(w * r) * r, w, np.ones_like(w)]
    return np.where(np.asarray(ok, bool)[None], np.stack(out), 0.0)


def _wave_fold(v):
    """[.., 64] -> [..]: v[l] += v[l + off] for off = 32, 16, 8, 4, 2, 1; lane 0."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v[..., :off] + v[..., off:2 * off]
    return v[..., 0]


def ordered_sum(t):
    """t [K,Ns] float64 -> [K]: the sums in the order of k_icp_rows and k_icp_sum (the head of this module)."""
    t = np.asarray(t, np.float64)
    K, Ns = t.shape
    nb = min(-(-Ns // 256), MAX_BLOCKS)
    T = 256 * nb
    npass = -(-Ns // T)
    v = np.zeros((K, npass * T))
    v[:, :Ns] = t
    v = v.reshape(K, npass, T)
    acc = np.zeros((K, T))
    for p in range(npass):
        acc = acc + v[:, p]
    w = _wave_fold(acc.reshape(K, nb, 4, 64))
    part = np.zeros((K, MAX_BLOCKS))
    part[:, :nb] = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
    return _wave_fold(part)


def linearize(src, dst, pose12, near=1e-3, max_dist=0.1, huber=0.0, dtype=np.float32, want_rows=False):
    """The host statement of be_icp_linearize_f32 -> sums [32] float64 (layout: the head of this module; the last two 0), bit for
    bit with dtype=np.float32.  With dtype=np.float64 the rows are evaluated in double and added by np.sum: the same function of
    the same float32 inputs in double precision, the yardstick of the tests.  want_rows: -> dict(sums, rows, ok, j)."""
    R = rows(src, dst, pose12, near, max_dist, huber, dtype)
    t = terms(R["rows"], R["ok"])
    sums = np.zeros(32)
    sums[:TERMS] = ordered_sum(t) if np.dtype(dtype) == np.float32 else t.sum(1)
    return dict(R, sums=sums) if want_rows else sums


def unpack(sums):
    """sums [32] -> (A [6,6] symmetric, b [6], e = sum w r r, sw = sum w, count)."""
    s = np.asarray(sums, np.float64)
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, s[21:27].copy(), float(s[27]), float(s[28]), int(s[29])


def solve_step(sums, damping=1e-6):
    """(A + damping diag(A)) x = -b in float64 -> x = (omega, v), or None when fewer than 6 samples took part, a sum is not
    finite, or the damped system is not positive definite."""
    A, b, _, _, count = unpack(sums)
    if count < 6 or not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None
    M = A + damping * np.diag(np.diag(A))
    try:
        np.linalg.cholesky(M)
        x = np.linalg.solve(M, -b)
    except np.linalg.LinAlgError:
        return None
    return x if np.isfinite(x).all() else None


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def compose(x, R, t):
    """The twist x = (omega, v) applied on the left of (R, t), in float64: E = exp([omega]x) by Rodrigues' formula, R <- E R,
    t <- E t + v -> (R, t, pose12 = the 12 float32 numbers of camera.pose)."""
    x = np.asarray(x, np.float64)
    K = _hat(x[:3])
    th = float(np.sqrt(x[:3] @ x[:3]))
    if th < 1e-8:
        E = np.eye(3) + K + 0.5 * (K @ K)
    else:
        E = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K)
    R = E @ np.asarray(R, np.float64)
    t = E @ np.asarray(t, np.float64) + x[3:]
    return R, t, camera.pose(R, t)


def register(src, dst, pose0=None, iters=20, damping=1e-6, max_dist=0.1, huber=0.0, step=3, max_jump=0.05, near=1e-3, tol=1e-9,
             linearize=linearize, normals=normals_f32, who="register"):
    """Point-to-plane ICP of the source view onto the target view, from pose0 (None: the identity): the target's normals once
    (normals(depth, cam, step, max_jump)), then up to `iters` times: the sums at the current pose
    (linearize(src, dst with `normal`, pose12, near, max_dist, huber) -> 32 doubles), solve_step, compose; it stops early when
    |x|^2 < tol, and when solve_step has no step to give.  -> dict(pose = the 12 float32 numbers, source frame -> target frame;
    poses = every iterate, pose0 first; rms, count = sqrt(sum w r r / sum w) and the number of samples of every linearisation
    (rms[k], count[k] belong to poses[k]); A [6,6] float64, cond = its condition number and cov = inv(A) rms^2, all of the last
    linearisation (cond inf and cov None where A is singular); converged; iters = the steps taken).  A near-singular system - a
    plane, a narrow field of view - is reported through cond and cov, it is not an error.  `linearize` and `normals` are the
    numpy statements by default; native.register_depth passes the GPU entries, and the rest of this loop is shared."""
    iters, damping, max_dist, huber, step, max_jump, near, tol = check_params(who, iters, damping, max_dist, huber, step, max_jump, near, tol)
    _view(f"{who}(src)", src)
    _view(f"{who}(dst)", dst)
    pose12 = camera.as_pose(pose0, f"{who}(pose0)")
    R, t = pose12[:9].reshape(3, 3).astype(np.float64), pose12[9:].astype(np.float64)
    dstn = dict(dst, normal=normals(dst["depth"], dst["cam"], step, max_jump))
    poses, rms, count = [pose12], [], []
    A, converged = np.zeros((6, 6)), False
    for _ in range(iters):
        sums = np.asarray(linearize(src, dstn, pose12, near, max_dist, huber), np.float64)
        A, _, e, sw, cnt = unpack(sums)
        count.append(cnt)
        rms.append(float(np.sqrt(e / sw)) if sw > 0 else float("nan"))
        x = solve_step(sums, damping)
        if x is None:
            break
        R, t, pose12 = compose(x, R, t)
        poses.append(pose12)
        if float(x @ x) < tol:
            converged = True
            break
    cond, cov = float("inf"), None
    if rms and np.isfinite(A).all() and np.isfinite(rms[-1]):
        cond = float(np.linalg.cond(A))
        try:
            cov = np.linalg.inv(A) * rms[-1] ** 2
        except np.linalg.LinAlgError:
            cov = None
    return dict(pose=poses[-1], poses=np.stack(poses), rms=np.array(rms), count=np.array(count, np.int64), A=A, cond=cond, cov=cov,
                converged=converged, iters=len(poses) - 1)


def pose_gap(pose12, R_true, t_true):
    """-> (the rotation angle of R R_true^T in degrees, |t - t_true| in metres) between a pose and the truth."""
    p = np.asarray(pose12, np.float64)
    dR = p[:9].reshape(3, 3) @ np.asarray(R_true, np.float64).T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1)))
    return float(ang), float(np.linalg.norm(p[9:] - np.asarray(t_true, np.float64)))
