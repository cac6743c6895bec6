#!/usr/bin/env python3
"""Time the depth registration on the GPU (profiles/HISTORY.md, round 22): native.depth_normals (k_depth_normals, one launch),
one native.icp_linearize (k_icp_rows + k_icp_sum, two launches) and a 20-iteration native.register_depth (one normals call, then
per iteration two launches, one 256-byte copy to the host - a synchronisation - and a 6 x 6 solve in numpy), against the same
linearisation composed of stock torch operators on the same device: the elementwise projection in float32, operation by
operation, a gather of the target's depth, normal and weight at the landing pixel, torch.cross for P x n, and one float64 einsum
of the [Ns,8] rows to the 27 sums.  The torch composition is the yardstick; the kernels are not measured against an earlier run of
themselves.

Scene: the analytic surface of tests/register_scenes.py (Z = 1 + 0.25 X - 0.18 Y + 0.12 sin 5X cos 4Y + 0.3 XY over normalised
image coordinates) at 147 x 147 and 587 x 587 through a camera of the same field of view, random weights in [0.25, 1] on both
sides, registered against itself from a pose 3 mm and 0.2 degrees off, tol = 0 so that all 20 iterations run.  Device events
around --inner calls per repeat, 5 warm-ups, --repeats timed repeats with the sides alternated in one process: torch, native,
torch again - the distance between the two torch medians is the spread a difference has to be read against.  register_depth
synchronises, so it is timed by the wall clock around one call, the median of --repeats calls.  Before timing the two
linearisations are compared: every sum must agree to 1e-3 of its sum of absolute terms (the two sides round the same float32
operations, but a sample that a rounding moves across a gate changes a sum by one part in the count).  There is no CPU path.

usage: python tools/bench_register.py [--repeats 20] [--inner 10] [--sizes 147x147 587x587] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render_at import alternate, timed  # noqa: E402


def torch_linearize(ds, ws, cs, dd, nd, wd, cd, p, near, max_dist):
    """native.icp_linearize(huber=0) in stock torch operators -> float64 [30] (the 21 + 6 sums, sum w r r, sum w, count)."""
    Hs, Ws = ds.shape
    Hd, Wd = dd.shape
    dev = ds.device
    y = torch.arange(Hs, device=dev, dtype=torch.float32)[:, None]
    x = torch.arange(Ws, device=dev, dtype=torch.float32)[None, :]
    xn, yn = (x - cs[3]) / cs[1], (y - cs[2]) / cs[0]
    Z = ds
    X, Y = xn * Z, yn * Z
    Xd = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
    Yd = ((p[3] * X + p[4] * Y) + p[5] * Z) + p[10]
    Zd = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
    fu = torch.floor((cd[1] * Xd) / Zd + cd[3] + 0.5)
    fv = torch.floor((cd[0] * Yd) / Zd + cd[2] + 0.5)
    part = ((Z > 0) & torch.isfinite(Z) & (Zd > near) & torch.isfinite(Zd) & (fu >= 0) & (fu < Wd) & (fv >= 0) & (fv < Hd)).view(-1)
    j = torch.where(part, fv.view(-1).to(torch.int64) * Wd + fu.view(-1).to(torch.int64), torch.zeros_like(part, dtype=torch.int64))
    zq = dd.view(-1)[j]
    n = nd.view(3, -1)[:, j]
    P = torch.stack([Xd.view(-1), Yd.view(-1), Zd.view(-1)])
    Q = torch.stack([((fu.view(-1) - cd[3]) / cd[1]) * zq, ((fv.view(-1) - cd[2]) / cd[0]) * zq, zq])
    D = P - Q
    w = ws.view(-1) * wd.view(-1)[j]
    ok = part & (zq > 0) & torch.isfinite(zq) & (n != 0).any(0) & ((D * D).sum(0) <= max_dist * max_dist) & (w > 0) & torch.isfinite(w)
    r = (n * D).sum(0)
    J = torch.cat([torch.cross(P, n, dim=0), n])
    rows = torch.where(ok[None], torch.cat([J, r[None]]), torch.zeros((), device=dev)).double()      # [7,Ns]
    w = torch.where(ok, w, torch.zeros((), device=dev)).double()
    M = torch.einsum("n,an,bn->ab", w, rows, rows)                                                     # [7,7]: A, b and sum w r r
    iu = torch.triu_indices(6, 6, device=dev)
    return torch.cat([M[iu[0], iu[1]], M[:6, 6], M[6, 6][None], w.sum()[None], ok.sum().double()[None]])


def surface(H, W, cam):
    yn = ((np.arange(H) - cam.cy) / cam.fy)[:, None]
    xn = ((np.arange(W) - cam.cx) / cam.fx)[None, :]
    return (1.0 + 0.25 * xn - 0.18 * yn + 0.12 * np.sin(5 * xn) * np.cos(4 * yn) + 0.3 * xn * yn).astype(np.float32)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_register: no GPU is visible; this measurement has no CPU form")
    from be_hip import camera, native, registration
    dev = torch.device("cuda:0")
    near, max_dist = float(np.float32(1e-3)), float(np.float32(0.1))
    R, t, pose = registration.compose([0.002, -0.002, 0.002, 0.002, -0.002, 0.001], np.eye(3), np.zeros(3))
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        cam = camera.Pinhole(60 * (H - 1) / 36, 58 * (W - 1) / 52, 18.2 * (H - 1) / 36, 25.7 * (W - 1) / 52)
        rng = np.random.default_rng(2)
        d = torch.from_numpy(surface(H, W, cam)).to(dev)
        ws, wd = (torch.from_numpy((0.25 + 0.75 * rng.random((H, W))).astype(np.float32)).to(dev) for _ in range(2))
        src, dst = dict(depth=d, weight=ws, cam=cam), dict(depth=d, weight=wd, cam=cam)
        nrm = native.depth_normals(d, cam)["normal"]
        cs, p = [float(v) for v in cam.f32()], [float(v) for v in pose]
        new = lambda: native.icp_linearize(src, dst, nrm, pose, near=1e-3, max_dist=0.1)["sums"]
        base = lambda: torch_linearize(d, ws, cs, d, nrm, wd, cs, p, near, max_dist)
        got, ref = new().cpu().numpy(), base().cpu().numpy()
        host = native.icp_linearize(src, dst, nrm, pose, rows=True)["rows"].cpu().numpy()
        scale = np.abs(registration.terms(host, host[7] != 0)).sum(1)
        worst = float((np.abs(got[:30] - ref) / np.maximum(scale, 1e-300)).max())
        if abs(got[29] - ref[29]) > 1e-4 * H * W or worst > 1e-3:
            raise SystemExit(f"{size}: native.icp_linearize and the torch composition differ: counts {got[29]} / {ref[29]}, worst sum {worst:.3g}")
        med = alternate(base, new, a.repeats, a.inner)
        normals_ms = statistics.median(timed(lambda: native.depth_normals(d, cam), a.inner) for _ in range(a.repeats))
        reg = lambda: native.register_depth(src, dst, pose0=pose, iters=20, tol=0.0)
        out = reg()
        walls = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reg()
            walls.append((time.perf_counter() - t0) * 1e3)
        gap = registration.pose_gap(out["pose"], np.eye(3), np.zeros(3))
        rows.append(dict(size=size, samples=H * W, taking_part=int(got[29]), normals_ms=normals_ms, torch_ms=med["base_a"],
                         torch_again_ms=med["base_b"], native_ms=med["new"], ratio=min(med["base_a"], med["base_b"]) / med["new"],
                         worst_relative_sum_difference=worst, register_20_iters_ms=statistics.median(walls),
                         register_ms_per_iteration=statistics.median(walls) / 20, iterations=int(out["iters"]),
                         end_gap_degrees=gap[0], end_gap_metres=gap[1], rms_first=float(out["rms"][0]), rms_last=float(out["rms"][-1])))
        print(json.dumps(rows[-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
