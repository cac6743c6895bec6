#!/usr/bin/env python3
"""Time the TSDF volume on the GPU (profiles/HISTORY.md): native.tsdf_integrate (k_tsdf_integrate, one launch per view over every
voxel) and native.tsdf_raycast (k_tsdf_mean, then k_tsdf_raycast, one thread per pixel that stops at its hit) against the same
arithmetic composed of stock torch operators on the same device - integration as the elementwise projection of every voxel centre
in float32, operation by operation, one gather per view and masked int64 adds; the ray cast as the means, then one pass of 16
gathers and the trilinear form per step over every pixel, with no early exit.  The torch composition is the yardstick; the kernels
are not measured against an earlier run of themselves, and no threshold is set: nothing measured exists to hold them to.

Scenes: V = 4 and 8 views of 147 x 147 and 587 x 587 samples (a far plane with a nearer block, 1 cm of noise, a fifth of the pixels
invalid, random weights in [0.25, 1], three channels) through the pipeline's own camera, each view a few millimetres from the
volume's frame, into volumes of 64 x 64 x 64 and 256 x 147 x 147 voxels that span the first view's frustum from 0.7 m to 1.25 m
with trunc = 0.05; the ray cast renders the 8-view volumes into targets of 147 x 147 and 587 x 587 pixels from view 0 with the
default step trunc / 4.  Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats with the sides
alternated in one process: torch, native, torch again - the distance between the two torch medians is the spread a difference has
to be read against.  Before timing the two results are compared: the sums and the depth must agree bit for bit on all but a few
elements (the two sides round the same float32 operations).  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_tsdf.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--sizes 147x147 587x587] [--views 4 8]
                                  [--json FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fuse import scene  # noqa: E402
from bench_render_at import alternate  # noqa: E402


def torch_integrate(sums, views, cs, desc, near):
    """native.tsdf_integrate in stock torch operators.  views: (depth, weight, feat [C,Ns], q = the inverse pose as 12 floats)."""
    sw, swd, swf = sums
    (nz, ny, nx), (X0, Y0, Z0), (sX, sY, sZ), trunc = desc["dims"], desc["origin"], desc["voxel"], desc["trunc"]
    dev = sw.device
    trunc_t = torch.tensor(trunc, dtype=torch.float32, device=dev)      # a tensor divisor: a python scalar would be multiplied by its reciprocal
    x = (X0 + torch.arange(nx, device=dev, dtype=torch.float32) * sX)[None, None, :]
    y = (Y0 + torch.arange(ny, device=dev, dtype=torch.float32) * sY)[None, :, None]
    z = (Z0 + torch.arange(nz, device=dev, dtype=torch.float32) * sZ)[:, None, None]
    for depth, weight, feat, q in views:
        Hs, Ws = depth.shape
        X = ((q[0] * x + q[1] * y) + q[2] * z) + q[9]
        Y = ((q[3] * x + q[4] * y) + q[5] * z) + q[10]
        Z = ((q[6] * x + q[7] * y) + q[8] * z) + q[11]
        su = torch.floor((cs[1] * X) / Z + cs[3] + 0.5)
        sv = torch.floor((cs[0] * Y) / Z + cs[2] + 0.5)
        part = (Z > near) & (su >= 0) & (su < Ws) & (sv >= 0) & (sv < Hs)
        j = torch.where(part, sv.to(torch.int64) * Ws + su.to(torch.int64), torch.zeros((), dtype=torch.int64, device=dev))
        Zq, w = depth.view(-1)[j], weight.view(-1)[j]
        sdf = Zq - Z
        wq = torch.floor(torch.clamp(w, max=16.0) * 256.0 + 0.5).to(torch.int64)
        part = part & (Zq > 0) & torch.isfinite(Zq) & (w > 0) & (sdf >= -trunc) & (wq != 0)
        wq = torch.where(part, wq, torch.zeros_like(wq))
        dq = torch.floor(torch.clamp(sdf, max=trunc) / trunc_t * 32768.0 + 0.5).to(torch.int64)
        sw += wq.to(torch.int32)
        swd += wq * torch.where(part, dq, torch.zeros_like(dq))
        fq = torch.floor(torch.clamp(torch.nan_to_num(feat[:, j.view(-1)], nan=0.0), -2048.0, 2048.0) * 65536.0 + 0.5).to(torch.int64)
        swf += (wq.view(1, -1) * fq).view(swf.shape)
    return sums


def _trilinear(a, idx, fx, fy, fz):
    c = [a[i] for i in idx]
    c00, c01, c10, c11 = (c[2 * m] + fx * (c[2 * m + 1] - c[2 * m]) for m in range(4))
    c0, c1 = c00 + fy * (c01 - c00), c10 + fy * (c11 - c10)
    return c0 + fz * (c1 - c0)


def torch_raycast(sums, cd, p, size, desc, z_near, step, n):
    """native.tsdf_raycast (mean, then the ray cast) in stock torch operators, every step over every pixel."""
    sw, swd, swf = sums
    (nz, ny, nx), (X0, Y0, Z0), (sX, sY, sZ) = desc["dims"], desc["origin"], desc["voxel"]
    dev = sw.device
    any_ = sw != 0
    zero = torch.zeros((), device=dev)
    D = torch.where(any_, (swd.double() / sw.double() * 2.0 ** -15).float(), zero).view(-1)
    W = (sw.double() * 2.0 ** -8).float().view(-1)
    Fm = torch.where(any_[None], (swf.double() / sw.double()[None] * 2.0 ** -16).float(), zero).view(swf.shape[0], -1)
    Ho, Wo = size
    # tensor divisors: torch multiplies by the reciprocal of a python scalar, the kernels divide
    sX, sY, sZ, fyd, fxd = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (sX, sY, sZ, cd[0], cd[1]))
    xn = ((torch.arange(Wo, device=dev, dtype=torch.float32) - cd[3]) / fxd)[None, :].expand(Ho, Wo).reshape(-1)
    yn = ((torch.arange(Ho, device=dev, dtype=torch.float32) - cd[2]) / fyd)[:, None].expand(Ho, Wo).reshape(-1)
    offs = [(dz * ny + dy) * nx + dx for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]

    def sample(z):
        X, Y = xn * z, yn * z
        gx = ((((p[0] * X + p[1] * Y) + p[2] * z) + p[9]) - X0) / sX
        gy = ((((p[3] * X + p[4] * Y) + p[5] * z) + p[10]) - Y0) / sY
        gz = ((((p[6] * X + p[7] * Y) + p[8] * z) + p[11]) - Z0) / sZ
        ix, iy, iz = torch.floor(gx), torch.floor(gy), torch.floor(gz)
        ok = (ix >= 0) & (ix <= nx - 2) & (iy >= 0) & (iy <= ny - 2) & (iz >= 0) & (iz <= nz - 2)
        j = torch.where(ok, (iz.to(torch.int64) * ny + iy.to(torch.int64)) * nx + ix.to(torch.int64), torch.zeros((), dtype=torch.int64, device=dev))
        idx = [torch.where(ok, j + o, j) for o in offs]
        for i in idx:
            ok = ok & (W[i] > 0)
        return ok, idx, gx - ix, gy - iy, gz - iz

    No = Ho * Wo
    done = torch.zeros(No, dtype=torch.bool, device=dev)
    depth, weight = torch.zeros(No, device=dev), torch.zeros(No, device=dev)
    feat = torch.zeros(Fm.shape[0], No, device=dev)
    prev = None
    for i in range(n):
        z = torch.tensor(z_near, dtype=torch.float32, device=dev) + torch.tensor(float(i), dtype=torch.float32, device=dev) * step
        ok, idx, fx, fy, fz = sample(z)
        F = _trilinear(D, idx, fx, fy, fz)
        Wt = _trilinear(W, idx, fx, fy, fz)
        Ft = torch.stack([_trilinear(Fm[c], idx, fx, fy, fz) for c in range(Fm.shape[0])]) if Fm.shape[0] else feat
        if prev is not None:
            ok_p, F_p, z_p, Wt_p, Ft_p = prev
            new = ~done & ok_p & ok & (F_p > 0) & (F <= 0)
            a = F_p / (F_p - F)
            depth = torch.where(new, z_p + (z - z_p) * a, depth)
            weight = torch.where(new, Wt_p + a * (Wt - Wt_p), weight)
            feat = torch.where(new[None], Ft_p + a[None] * (Ft - Ft_p), feat)
            done = done | new
        prev = (ok, F, z, Wt, Ft)
    return dict(depth=depth.view(Ho, Wo), valid=done.view(Ho, Wo), weight=weight.view(Ho, Wo), feat=feat.view(-1, Ho, Wo))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--volumes", nargs="+", default=["64x64x64", "256x147x147"])
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587"])
    ap.add_argument("--views", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native, volume
    dev = torch.device("cuda:0")
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    near, C, trunc = float(np.float32(1e-3)), 3, 0.05
    z_range = (0.7, 1.25)
    rows = []
    for vname in a.volumes:
        dims = tuple(int(v) for v in vname.split("x"))
        for size in a.sizes:
            H, W = (int(v) for v in size.split("x"))
            cam = dcal.intrinsics(H, W)
            cs = [float(v) for v in cam.f32()]
            half_x, half_y = 0.55 * W / cam.fx * z_range[1], 0.55 * H / cam.fy * z_range[1]
            desc = dict(dims=dims, origin=(-half_x, -half_y, z_range[0]), trunc=trunc,
                        voxel=(2 * half_x / (dims[2] - 1), 2 * half_y / (dims[1] - 1), (z_range[1] - z_range[0]) / (dims[0] - 1)))
            ref_vol = native.tsdf_volume(C=C, device=dev, **desc)
            desc = ref_vol.description()                                 # the float32 values both sides compute with
            desc.pop("C")
            zeros = lambda: (torch.zeros_like(ref_vol.sw), torch.zeros_like(ref_vol.swd), torch.zeros_like(ref_vol.swf))
            for V in a.views:
                sc = scene(H, W, V, dev, C)
                poses = [camera.pose(None, t) for _, _, _, t in sc]
                nat = [dict(depth=d, weight=w, feat=f, cam_src=cam, pose=p) for (d, w, f, _), p in zip(sc, poses)]
                tor = [(d, w, f.reshape(C, -1), [float(x) for x in volume.inverse_pose(p)]) for (d, w, f, _), p in zip(sc, poses)]
                vol = native.tsdf_volume(C=C, device=dev, **desc)
                tsums = zeros()

                def new():
                    native.tsdf_integrate(vol, nat, near=1e-3)

                def base():
                    torch_integrate(tsums, tor, cs, desc, near)

                new(), base()
                differ = int((vol.sw != tsums[0]).sum()) + int((vol.swd != tsums[1]).sum())
                n_vox = vol.sw.numel()
                if differ > 1e-3 * n_vox:
                    raise SystemExit(f"{vname}, {size}, {V} views: native.tsdf_integrate and the torch composition differ on {differ} of {n_vox} voxels")
                held = int((vol.sw != 0).sum())
                med = alternate(base, new, a.repeats, a.inner)           # the sums keep growing on both sides: the work does not change
                rows.append(dict(op="integrate", volume=vname, size=size, views=V, voxel_views=V * n_vox, voxels_held=held / n_vox,
                                 voxels_that_differ=differ, torch_ms=med["base_a"], torch_again_ms=med["base_b"], native_ms=med["new"],
                                 ratio=min(med["base_a"], med["base_b"]) / med["new"], launches=V,
                                 voxel_views_per_ns=V * n_vox / (med["new"] * 1e6)))
                print(json.dumps(rows[-1]), flush=True)
                del sc, nat, tor, tsums, vol
            # the ray cast: the largest view count's volume, built once, rendered from view 0
            V = max(a.views)
            sc = scene(H, W, V, dev, C)
            vol = native.tsdf_integrate(native.tsdf_volume(C=C, device=dev, **desc),
                                        [dict(depth=d, weight=w, feat=f, cam_src=cam, pose=camera.pose(None, t)) for d, w, f, t in sc], near=1e-3)
            sums = (vol.sw, vol.swd, vol.swf)
            z_near, _, step, n = volume.check_raycast("bench_tsdf", z_range, None, desc["trunc"])
            p = [float(x) for x in camera.pose()]
            new = lambda: native.tsdf_raycast(vol, cam, None, (H, W), z_range)
            base = lambda: torch_raycast(sums, cs, p, (H, W), desc, z_near, step, n)
            got, ref = new(), base()
            differ = int((got["depth"].view(torch.int32) != ref["depth"].view(torch.int32)).sum())
            if differ > 1e-3 * H * W:
                raise SystemExit(f"{vname}, {size}: native.tsdf_raycast and the torch composition differ on {differ} of {H * W} pixels")
            hit = int(got["valid"].sum())
            del got, ref
            med = alternate(base, new, a.repeats, a.inner)
            rows.append(dict(op="raycast", volume=vname, size=size, views=V, steps=n, pixels_hit=hit / (H * W), pixels_that_differ=differ,
                             torch_ms=med["base_a"], torch_again_ms=med["base_b"], native_ms=med["new"],
                             ratio=min(med["base_a"], med["base_b"]) / med["new"], launches=2))
            print(json.dumps(rows[-1]), flush=True)
            del sc, vol, sums, ref_vol
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
