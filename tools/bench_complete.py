#!/usr/bin/env python3
"""Time the nearest-sample flood fill on the GPU (profiles/HISTORY.md, Round 15), milliseconds per call of native.fill_nearest
(k_fill_seeds, the leading pass, the passes above step 8 and the tail) with the fused tail - the steps 8, 4, 2, 1 as one launch over
LDS tiles - and without it, one launch per pass.  The unfused path is the yardstick of the fused one: `fuse=True` stays the default
of native.fill_nearest only while it is not slower at 587 x 587 in the same run.

Sources: a 147 x 147, a 587 x 587 and a 1080 x 1920 map shaped like the pipeline's depth_map - discs of a nearer surface on a far
plane, depth (with +-1 cm noise) and a confidence only within 3 px of a boundary, a tenth to a quarter of the pixels - filled with
smooth = 2.  Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats with the sides alternated in one
process: unfused, fused, unfused again - the distance between the two unfused medians is the spread a difference has to be read
against.  Before timing the two results are compared: they must be the same integers and the same depth bits.  There is no CPU
path: without a GPU the script fails.

usage: python tools/bench_complete.py [--repeats 20] [--inner 10] [--sizes 147x147 587x587 1080x1920] [--smooth 2] [--json FILE]
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


def source(H, W, dev, band=3.0):
    """-> (depth, conf) on dev: discs at 0.80 m on a plane at 1.10 m, samples within `band` px of a disc's rim only."""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    dist = np.full((H, W), 1e9, np.float32)                              # signed distance to the nearest rim, < 0 inside a disc
    for _ in range(max(3, H * W // 20000)):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(12, 48)
        dist = np.minimum(dist, np.hypot(y - cy, x - cx) - rad)
    on = np.abs(dist) < band
    z = np.where(dist < 0, 0.80, 1.10) + rng.uniform(-0.01, 0.01, (H, W))
    depth = np.where(on, z, 0).astype(np.float32)
    conf = np.where(on, rng.uniform(0.1, 1.0, (H, W)), 0).astype(np.float32)
    return torch.from_numpy(depth).to(dev), torch.from_numpy(conf).to(dev)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587", "1080x1920"])
    ap.add_argument("--smooth", type=int, default=2)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_complete: no GPU is visible; this measurement has no CPU form")
    from be_hip import fill, native
    dev = torch.device("cuda:0")
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        d, c = source(H, W, dev)
        fused = lambda: native.fill_nearest(d, c, smooth=a.smooth, fuse=True)
        plain = lambda: native.fill_nearest(d, c, smooth=a.smooth, fuse=False)
        got, ref = fused(), plain()
        for k in ("index", "dist2"):
            if not torch.equal(got[k], ref[k]):
                raise SystemExit(f"{size}: the fused and the unfused path differ in {k}")
        if not torch.equal(got["depth"].view(torch.int32), ref["depth"].view(torch.int32)):
            raise SystemExit(f"{size}: the fused and the unfused path differ in depth")
        seeds = int((got["dist2"] == 0).sum())
        far = float(got["dist2"].max()) ** 0.5
        del got, ref
        med = alternate(plain, fused, a.repeats, a.inner)
        rows.append(dict(size=size, pixels=H * W, seeds=seeds / (H * W), farthest_hole_px=far, passes=len(fill.jfa_steps(H, W)),
                         smooth=a.smooth, unfused_ms=med["base_a"], unfused_again_ms=med["base_b"], fused_ms=med["new"],
                         fused_ns_per_pixel=med["new"] * 1e6 / (H * W), ratio=min(med["base_a"], med["base_b"]) / med["new"]))
        print(json.dumps(rows[-1]), flush=True)
        del d, c
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
