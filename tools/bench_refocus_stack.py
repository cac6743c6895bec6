#!/usr/bin/env python3
"""Time a K-plane focal stack two ways on the GPU (profiles/HISTORY.md, Round 11):

  baseline  K x ( render_full_grid(rho_prime = rho_k) + fold_records_grid(want=("refoc",)) )    what one had to do before
  new       1 x render_full_grid + 1 x fold_refocus_stack(K powers)

on the record grid of a 587 x 587 pair (284 x 284 patches) and of a 1080 x 1920 pair (flush-edge grid, 531 x 951 patches), for
K in {1, 8, 32}.  Parameters are synth.plausible_params12 (the fold's time does not depend on trained weights).  Device events
around each side, 5 warm-ups, --repeats timed repeats with the sides alternated in one process: baseline, new, baseline again -
the distance between the two baseline medians is the spread a K = 1 difference has to be read against.  Before timing, every
plane of the new side is compared bit for bit with the baseline's.  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_refocus_stack.py [--repeats 20] [--sizes 587x587 1080x1920] [--planes 1 8 32] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))

WARMUP = 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--sizes", nargs="+", default=["587x587", "1080x1920"])
    ap.add_argument("--planes", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_refocus_stack: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import native, synth, tiling, workflow
    dev = torch.device("cuda:0")
    args = utils.get_args("eval", argv=[])
    helper, dcal = utils.PostProcessGlobalBase(args, dev), utils.DepthEtas(args, dev)
    opts, consts = helper.render_opts(wrap_angles=False), dcal.consts
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        ys, xs = tiling.patch_grid(H, 2), tiling.patch_grid(W, 2)
        HP, WP = len(ys), len(xs)
        img = torch.from_numpy(synth.synthetic_image_pair(H, W, nshape=14)[0]).to(dev)
        p12 = torch.from_numpy(synth.plausible_params12(HP * WP, name=f"bench_refocus_{size}")).to(dev)
        dys, dxs = native.origin_table(ys, H, dev, cover=True), native.origin_table(xs, W, dev, cover=True)
        for K in a.planes:
            powers = workflow.focus_sweep(dcal, K, 0.75, 1.18).tolist()
            rho = torch.tensor(powers, dtype=torch.float32, device=dev)

            def baseline():
                return [native.fold_records_grid(opts, native.render_full_grid(opts, consts, r, False, p12, img, dys, dxs), H, W, dys, dxs,
                                                 False, want=("refoc",))["refoc"] for r in powers]

            def new():
                return native.fold_refocus_stack(opts, consts, native.render_full_grid(opts, consts, 10.39, False, p12, img, dys, dxs),
                                                 rho, H, W, ys=dys, xs=dxs)

            want, got = baseline(), new()
            for k in range(K):
                if not torch.equal(got[k], want[k]):
                    raise SystemExit(f"{size} K={K}: plane {k} differs from render_full_grid + fold_records_grid")
            del want, got
            for _ in range(WARMUP):
                baseline(), new()
            torch.cuda.synchronize()
            t = dict(base_a=[], new=[], base_b=[])
            for _ in range(a.repeats):
                t["base_a"].append(timed(baseline))
                t["new"].append(timed(new))
                t["base_b"].append(timed(baseline))
            med = {k: statistics.median(v) for k, v in t.items()}
            row = dict(size=size, grid=[HP, WP], K=K, repeats=a.repeats, baseline_ms=med["base_a"], baseline_again_ms=med["base_b"],
                       new_ms=med["new"], baseline_spread_ms=abs(med["base_a"] - med["base_b"]),
                       min_ms={k: min(v) for k, v in t.items()}, speedup=min(med["base_a"], med["base_b"]) / med["new"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    print(f"\n{'size':>10} {'K':>3} {'baseline ms':>12} {'again ms':>10} {'new ms':>9} {'baseline/new':>13}")
    for r in rows:
        print(f"{r['size']:>10} {r['K']:>3} {r['baseline_ms']:>12.3f} {r['baseline_again_ms']:>10.3f} {r['new_ms']:>9.3f} {r['speedup']:>13.2f}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
