#!/usr/bin/env python3
"""Time the diffusion depth completion on the GPU (profiles/HISTORY.md, Round 18), milliseconds per call:

* DepthPipeline.complete(maps, method="nearest") against method="diffuse" (the default schedule, the edge map on), and
* native.fill_diffuse with one sweep per launch (fuse=False) against the tiled launch (many sweeps per launch on LDS regions).

Sources: a 147 x 147 and a 587 x 587 map shaped like the pipeline's maps (tools/bench_complete.py: discs of a nearer surface on a far
plane, depth and a confidence only within 3 px of a rim) with a boundary map that is 1 within half a pixel of a rim.  Device events
around --inner calls per repeat, 5 warm-ups, --repeats timed repeats with the sides alternated in one process: base, new, base again
- the distance between the two base medians is the spread a difference has to be read against.  The residual of each result (the
largest |average of the neighbours - value| left at a hole) is printed with it.  There is no pass or fail on time, and no CPU path:
without a GPU the script fails.

usage: python tools/bench_diffuse.py [--repeats 20] [--inner 5] [--sizes 147x147 587x587] [--json FILE]
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
    """-> dict(depth_map, conf, bndry) on dev: bench_complete.source's discs, and bndry = 1 within half a pixel of a rim."""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    dist = np.full((H, W), 1e9, np.float32)
    for _ in range(max(3, H * W // 20000)):
        cy, cx, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(12, 48)
        dist = np.minimum(dist, np.hypot(y - cy, x - cx) - rad)
    on = np.abs(dist) < band
    z = np.where(dist < 0, 0.80, 1.10) + rng.uniform(-0.01, 0.01, (H, W))
    maps = dict(depth_map=np.where(on, z, 0), conf=np.where(on, rng.uniform(0.1, 1.0, (H, W)), 0), bndry=np.abs(dist) < 0.5)
    return {k: torch.from_numpy(v.astype(np.float32)).to(dev) for k, v in maps.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_diffuse: no GPU is visible; this measurement has no CPU form")
    import models
    import utils
    from be_hip import diffuse, native, synth
    from be_hip.pipeline import DepthPipeline
    dev = "cuda:0"
    args = utils.get_args("eval", argv=[])
    T = lambda v: torch.from_numpy(np.asarray(v)).float()
    lm, gm = models.LocalStage(), models.GlobalStage(device=dev)
    lm.load_state_dict({k: T(v) for k, v in synth.local_stage_state_dict().items()})
    gm.load_state_dict({k: T(v) for k, v in synth.global_stage_state_dict().items()})
    pipe = DepthPipeline(lm.to(dev).eval(), gm.to(dev).eval(), utils.PostProcessGlobalBase(args, dev), utils.DepthEtas(args, dev))
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        maps = source(H, W, dev)
        z, c, b = maps["depth_map"], maps["conf"], maps["bndry"]
        nearest = lambda: pipe.complete(maps)
        diffused = lambda: pipe.complete(maps, method="diffuse")
        tiled = lambda: native.fill_diffuse(z, c, b)
        single = lambda: native.fill_diffuse(z, c, b, fuse=False)
        got, ref, one = diffused(), tiled(), single()
        if not torch.equal(got["depth_dense"].view(torch.int32), ref["depth"].view(torch.int32)):
            raise SystemExit(f"{size}: complete(method='diffuse') and native.fill_diffuse differ")
        plan = diffuse.schedule(H, W)
        row = dict(size=size, pixels=H * W, seeds=int(got["measured"].sum()) / (H * W), levels=len(plan),
                   launches_tiled=sum(len(p[2]) for p in plan), launches_single=sum(sum(p[2]) for p in plan),
                   residual=float(ref["residual"]), residual_single=float(one["residual"]),
                   single_vs_tiled_max_m=float((one["depth"] - ref["depth"]).abs().max()),
                   diffuse_vs_nearest_max_m=float((got["depth_dense"] - nearest()["depth_dense"]).abs().max()))
        del got, ref, one
        med = alternate(nearest, diffused, a.repeats, a.inner)
        row.update(nearest_ms=med["base_a"], nearest_again_ms=med["base_b"], diffuse_ms=med["new"])
        med = alternate(single, tiled, a.repeats, a.inner)
        row.update(single_sweep_ms=med["base_a"], single_sweep_again_ms=med["base_b"], tiled_ms=med["new"],
                   ratio=min(med["base_a"], med["base_b"]) / med["new"])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del maps, z, c, b
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
