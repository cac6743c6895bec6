#!/usr/bin/env python3
"""Time the folds at arbitrary positions on the GPU (profiles/HISTORY.md, Round 13), nanoseconds per sample, on two record grids:
the uniform stride-2 grid of a 587 x 587 pair (284 x 284 patches) and the flush-edge grid of a 1080 x 1920 pair (origin tables).

  (a) pixels     the pixel lattice passed as points        against  fold_records / fold_records_grid (= render_at(1))
  (b) k = 4      the k = 4 lattice passed as points        against  fold_records_at(scale=4)
  (c) shuffled   a random permutation of (b): what losing the locality of the records costs
  (d) keypoints  10 000 random positions

All six maps each time.  The siblings the points kernels are measured against are the kernels of this same tree.  Parameters are
synth.plausible_params12 (the fold's time does not depend on trained weights).  Device events around --inner calls per repeat, 5
warm-ups, --repeats timed repeats with the sides alternated in one process: baseline, new, baseline again - the distance between
the two baseline medians is the spread a difference has to be read against.  Before timing, (a) and (b) are compared bit for bit
with their baselines.  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_sample_at.py [--repeats 20] [--inner 10] [--sizes 587x587 1080x1920] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_render_at import WARMUP, alternate, timed  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["587x587", "1080x1920"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample_at: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import native, synth, tiling
    dev = torch.device("cuda:0")
    args = utils.get_args("eval", argv=[])
    helper, dcal = utils.PostProcessGlobalBase(args, dev), utils.DepthEtas(args, dev)
    opts, consts = helper.render_opts(wrap_angles=False), dcal.consts
    same = lambda x, y: torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        img = torch.from_numpy(synth.synthetic_image_pair(H, W, nshape=14)[0]).to(dev)
        ys, xs = tiling.patch_grid(H, 2), tiling.patch_grid(W, 2)
        uniform = ys[-1] - ys[-2] == 2 and xs[-1] - xs[-2] == 2
        p12 = torch.from_numpy(synth.plausible_params12(len(ys) * len(xs), name=f"bench_sample_at_{size}")).to(dev)
        if uniform:
            rec, _ = native.render_full(opts, consts, 10.39, False, p12, native.view_image_pair(img, 2), pixels=img)
            grid = dict(hp=len(ys), wp=len(xs), stride=2)
            fold = lambda: native.fold_records(opts, rec, len(ys), len(xs), H, W, 2, False)
        else:
            rec = native.render_full_grid(opts, consts, 10.39, False, p12, img, ys, xs)
            grid = dict(ys=native.origin_table(ys, H, dev, cover=True), xs=native.origin_table(xs, W, dev, cover=True))
            fold = lambda: native.fold_records_grid(opts, rec, H, W, ys, xs, False)
        fold_at = lambda k: native.fold_records_at(opts, rec, H, W, scale=k, **grid)
        at_points = lambda p: native.fold_records_points(opts, rec, H, W, p, **grid)
        pix = torch.from_numpy(tiling.resize_points(H, W, (H, W))).to(dev)
        fine = torch.from_numpy(tiling.resize_points(H, W, ((H - 1) * 4 + 1, (W - 1) * 4 + 1))).to(dev)
        gen = torch.Generator().manual_seed(0)
        flat = fine.view(-1, 2)
        shuffled = flat[torch.randperm(flat.shape[0], generator=gen).to(dev)].contiguous()
        keys = (torch.rand(10000, 2, generator=gen) * torch.tensor([H - 1.0, W - 1.0])).to(dev)

        # results must not change: bit equality before any timing
        for name, got, ref in (("pixels", at_points(pix), fold()), ("k = 4", at_points(fine), fold_at(4))):
            for m, v in ref.items():
                if not same(got[m], v):
                    raise SystemExit(f"{size} {name}: map {m} of fold_records_points differs from its lattice sibling")
        del got, ref
        kind = "uniform" if uniform else "flush-edge tables"
        for what, pts, base, inner in (("(a) pixels as points vs the pixel fold", pix, fold, a.inner),
                                       ("(b) k=4 lattice as points vs fold_records_at(4)", fine, lambda: fold_at(4), max(1, a.inner // 4))):
            n = pts.shape[0] * pts.shape[1]
            med = alternate(base, lambda: at_points(pts), a.repeats, inner)
            rows.append(dict(what=what, size=size, grid=kind, samples=n, baseline_ns_per_sample=med["base_a"] * 1e6 / n,
                             baseline_again_ns_per_sample=med["base_b"] * 1e6 / n, points_ns_per_sample=med["new"] * 1e6 / n,
                             ratio=med["new"] / min(med["base_a"], med["base_b"])))
            print(json.dumps(rows[-1]), flush=True)
        for what, pts, inner in (("(c) k=4 lattice, shuffled", shuffled, max(1, a.inner // 4)), ("(d) 10000 random keypoints", keys, a.inner)):
            for _ in range(WARMUP):
                at_points(pts)
            torch.cuda.synchronize()
            ms = statistics.median(timed(lambda: at_points(pts), inner) for _ in range(a.repeats))
            rows.append(dict(what=what, size=size, grid=kind, samples=pts.shape[0], points_ms=ms, points_ns_per_sample=ms * 1e6 / pts.shape[0]))
            print(json.dumps(rows[-1]), flush=True)
        del rec, pix, fine, flat, shuffled, keys
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
