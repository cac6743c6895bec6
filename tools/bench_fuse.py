#!/usr/bin/env python3
"""Time the multi-view depth fusion on the GPU (profiles/HISTORY.md, round 19): native.fuse_views (k_fuse_front, k_fuse_add and
k_fuse_step over V views: 4 V + 2 kernel launches and two memsets at recentre=True, peel=0) against the same merge composed of stock
torch operators on the same device - per view the elementwise projection in float32, operation by operation, one
scatter_reduce_(amin) of the depth bits into the front, and int64 index_add_ of the fixed-point terms into the sums, twice (the
recentred pass).  The torch composition is the yardstick; the kernels are not measured against an earlier run of themselves.

Scenes: V = 4 and 8 views of 147 x 147 and 587 x 587 samples (a far plane with a nearer block, 1 cm of noise, a fifth of the pixels
invalid, random weights in [0.25, 1], three channels) through the pipeline's own camera, each view a few millimetres from the
target, fused onto a target of the same size with tau = 0.05, min_views = 1, recentre on, peel 0.  Device events around --inner calls
per repeat, 5 warm-ups, --repeats timed repeats with the sides alternated in one process: torch, native, torch again - the distance
between the two torch medians is the spread a difference has to be read against.  Before timing the two results are compared: depth
must agree bit for bit on all but a few pixels (the two sides round the same float32 operations; a division that rounds differently
may move a sample across a pixel boundary).  Also printed: the integer atomics a call issues, counted from the result (one front
minimum per valid sample, four adds per agreeing sample in the first pass and 4 + C in the recentred one), and their payload bytes.
There is no CPU path: without a GPU the script fails.

usage: python tools/bench_fuse.py [--repeats 20] [--inner 10] [--sizes 147x147 587x587] [--views 4 8] [--json FILE]
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

from bench_render_at import alternate  # noqa: E402

EMPTY = 0x7FFFFFFF           # no front: as int32 above the bits of every finite positive float; as a float a NaN


def _project(depth, cs, cd, p, size, near, weight):
    """One view's samples in stock torch operators -> (Zd [Ns], dst int64 [Ns], part bool [Ns], wq int64 [Ns])."""
    Hs, Ws = depth.shape
    Ho, Wo = size
    dev = depth.device
    y = torch.arange(Hs, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(Ws, device=dev, dtype=torch.float32)[None, :]
    xn, yn = (x - cs[3]) / cs[1], (y - cs[2]) / cs[0]
    Z = depth
    X, Y = xn * Z, yn * Z
    Xd = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
    Yd = ((p[3] * X + p[4] * Y) + p[5] * Z) + p[10]
    Zd = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
    fu = torch.floor((cd[1] * Xd) / Zd + cd[3] + 0.5)
    fv = torch.floor((cd[0] * Yd) / Zd + cd[2] + 0.5)
    wq = torch.floor(torch.clamp(weight, max=16.0) * 65536.0 + 0.5).to(torch.int64).view(-1)
    part = ((Z > 0) & torch.isfinite(Z) & (Zd > near) & torch.isfinite(Zd) & (fu >= 0) & (fu < Wo) & (fv >= 0) & (fv < Ho) & (weight > 0)).view(-1)
    part = part & (wq != 0)
    dst = torch.where(part, fv.view(-1).to(torch.int64) * Wo + fu.view(-1).to(torch.int64), torch.zeros_like(wq))
    return Zd.reshape(-1), dst, part, wq


def torch_fuse(views, cs, cd, size, near, tau, min_views):
    """native.fuse_views(recentre=True, peel=0) in stock torch operators.  views: (depth, weight, feat [C,Ns], pose as 12 floats)."""
    Ho, Wo = size
    No = Ho * Wo
    dev = views[0][0].device
    S = [_project(d, cs, cd, p, size, near, w) for d, w, f, p in views]
    zmin = torch.full((No,), EMPTY, dtype=torch.int32, device=dev)
    for Zd, dst, part, wq in S:
        zmin.scatter_reduce_(0, dst, torch.where(part, Zd.view(torch.int32), torch.full_like(dst, EMPTY, dtype=torch.int32)), "amin")
    base = torch.where(zmin != EMPTY, zmin.view(torch.float32), torch.full((), float("nan"), device=dev))
    span = torch.tensor(tau, dtype=torch.float32, device=dev)
    C = views[0][2].shape[0]
    for last in (False, True):
        sw, swd = torch.zeros(No, dtype=torch.int64, device=dev), torch.zeros(No, dtype=torch.int64, device=dev)
        cnt, nviews = torch.zeros(No, dtype=torch.int32, device=dev), torch.zeros(No, dtype=torch.int32, device=dev)
        swf = torch.zeros(C, No, dtype=torch.int64, device=dev)
        for (Zd, dst, part, wq), (_, _, feat, _) in zip(S, views):
            d = Zd - base[dst]
            a = part & (d >= 0) & (d <= span)
            dq = torch.floor(torch.where(a, d, torch.zeros_like(d)) * 1048576.0 + 0.5).to(torch.int64)
            w = torch.where(a, wq, torch.zeros_like(wq))
            sw.index_add_(0, dst, w)
            swd.index_add_(0, dst, w * dq)
            seen = torch.zeros(No, dtype=torch.int32, device=dev).index_add_(0, dst, a.to(torch.int32))
            cnt += seen
            nviews += (seen > 0).to(torch.int32)
            if last:
                fq = torch.floor(torch.clamp(torch.nan_to_num(feat, nan=0.0), -2048.0, 2048.0) * 65536.0 + 0.5).to(torch.int64)
                swf.index_add_(1, dst, w[None] * fq)
        m = (base.double() + swd.double() / sw.double() * 2.0 ** -20).float()
        if not last:
            base, span = torch.where(cnt > 0, m - span, torch.full_like(m, float("nan"))), span + span
    fin = (cnt > 0) & (nviews >= min_views)
    zero = torch.zeros((), device=dev)
    return dict(depth=torch.where(fin, m, zero).view(Ho, Wo), valid=fin.view(Ho, Wo),
                weight=torch.where(fin, (sw.double() * 2.0 ** -16).float(), zero).view(Ho, Wo),
                views=torch.where(fin, nviews, torch.zeros_like(nviews)).view(Ho, Wo), count=torch.where(fin, cnt, torch.zeros_like(cnt)).view(Ho, Wo),
                feat=torch.where(fin[None], (swf.double() / sw.double() * 2.0 ** -16).float(), zero).view(C, Ho, Wo))


def scene(H, W, V, dev, C=3):
    """V views of a far plane with a nearer block: (depth, weight, feat, translation) per view, on the device."""
    rng = np.random.default_rng(1)
    views = []
    for v in range(V):
        t = (0.0, 0.0, 0.0) if v == 0 else (0.002 * np.cos(2.4 * v), 0.0015 * np.sin(2.4 * v), 0.001 * (v % 3 - 1))
        d = np.full((H, W), 1.10 - t[2])
        d[H // 4:3 * H // 4, W // 4:3 * W // 4] = 0.80 - t[2]
        d += 0.01 * rng.standard_normal((H, W))
        d[rng.random((H, W)) < 0.2] = 0
        w = 0.25 + 0.75 * rng.random((H, W))
        f = rng.random((C, H, W))
        views.append((torch.from_numpy(d.astype(np.float32)).to(dev), torch.from_numpy(w.astype(np.float32)).to(dev),
                      torch.from_numpy(f.astype(np.float32)).to(dev), t))
    return views


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587"])
    ap.add_argument("--views", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_fuse: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native
    dev = torch.device("cuda:0")
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    tau, near, C = 0.05, float(np.float32(1e-3)), 3
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        cam = dcal.intrinsics(H, W)
        cs = [float(v) for v in cam.f32()]
        for V in a.views:
            sc = scene(H, W, V, dev, C)
            poses = [camera.pose(None, t) for _, _, _, t in sc]
            nat = [dict(depth=d, weight=w, feat=f, cam_src=cam, pose=p) for (d, w, f, _), p in zip(sc, poses)]
            tor = [(d, w, f.reshape(C, -1), [float(x) for x in p]) for (d, w, f, _), p in zip(sc, poses)]
            new = lambda: native.fuse_views(nat, cam, (H, W), tau=tau, min_views=1, recentre=True, peel=0, near=1e-3)
            base = lambda: torch_fuse(tor, cs, cs, (H, W), near, float(np.float32(tau)), 1)
            got, ref = new(), base()
            differ = int((got["depth"].view(torch.int32) != ref["depth"].view(torch.int32)).sum())
            if differ > 1e-3 * H * W:
                raise SystemExit(f"{size}, {V} views: native.fuse_views and the torch composition differ on {differ} of {H * W} target pixels")
            filled, agree = int(got["valid"].sum()), int(got["count"].sum())
            valid = sum(int((d > 0).sum()) for d, _, _, _ in sc)
            atomics = valid + 4 * agree + (4 + C) * agree
            atomic_bytes = 4 * valid + 24 * agree + (24 + 8 * C) * agree
            del got, ref
            med = alternate(base, new, a.repeats, a.inner)
            rows.append(dict(size=size, views=V, samples=V * H * W, target_filled=filled / (H * W), pixels_that_differ=differ,
                             torch_ms=med["base_a"], torch_again_ms=med["base_b"], native_ms=med["new"],
                             ratio=min(med["base_a"], med["base_b"]) / med["new"], launches=4 * V + 2, atomics=atomics,
                             atomic_bytes=atomic_bytes, atomics_per_ns=atomics / (med["new"] * 1e6)))
            print(json.dumps(rows[-1]), flush=True)
            del sc, nat, tor
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
