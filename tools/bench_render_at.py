#!/usr/bin/env python3
"""Time the folds on a finer lattice on the GPU (profiles/HISTORY.md, Round 12), on the record grid of a 587 x 587 pair
(284 x 284 patches, uniform stride 2):

  scale 1   fold_records_at(scale=1)  against  fold_records            (all six maps; the baseline kernel is unchanged)
  scales    fold_records_at(scale=k), k in --scales: time per call and per output sample
  stack     fold_refocus_stack_at(scale=1, K = 8)  against  fold_refocus_stack(K = 8), and the lattice stack at --scales

Parameters are synth.plausible_params12 (the fold's time does not depend on trained weights).  Device events around --inner calls
per repeat (a single 587 x 587 fold is a fraction of a millisecond), 5 warm-ups, --repeats timed repeats with the sides alternated
in one process: baseline, new, baseline again - the distance between the two baseline medians is the spread a difference has to be
read against.  Before timing, the scale-1 outputs are compared bit for bit with the baseline's and every scale's [::k, ::k] samples
with the scale-1 map.  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_render_at.py [--repeats 20] [--inner 10] [--size 587x587] [--scales 2 4 8] [--json FILE]
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


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def alternate(base, new, repeats, inner):
    """-> medians (base, new, base again) in ms per call."""
    for _ in range(WARMUP):
        base(), new()
    torch.cuda.synchronize()
    t = dict(base_a=[], new=[], base_b=[])
    for _ in range(repeats):
        t["base_a"].append(timed(base, inner))
        t["new"].append(timed(new, inner))
        t["base_b"].append(timed(base, inner))
    return {k: statistics.median(v) for k, v in t.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--size", default="587x587")
    ap.add_argument("--scales", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_at: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import native, synth, workflow
    dev = torch.device("cuda:0")
    args = utils.get_args("eval", argv=[])
    helper, dcal = utils.PostProcessGlobalBase(args, dev), utils.DepthEtas(args, dev)
    opts, consts = helper.render_opts(wrap_angles=False), dcal.consts
    H, W = (int(v) for v in a.size.split("x"))
    hp, wp = (H - 21) // 2 + 1, (W - 21) // 2 + 1
    img = torch.from_numpy(synth.synthetic_image_pair(H, W, nshape=14)[0]).to(dev)
    p12 = torch.from_numpy(synth.plausible_params12(hp * wp, name=f"bench_render_at_{a.size}")).to(dev)
    rec, _ = native.render_full(opts, consts, 10.39, False, p12, native.view_image_pair(img, 2), pixels=img)
    rho = torch.tensor(workflow.focus_sweep(dcal, 8, 0.75, 1.18).tolist(), dtype=torch.float32, device=dev)
    grid = dict(hp=hp, wp=wp, stride=2)

    fold = lambda: native.fold_records(opts, rec, hp, wp, H, W, 2, False)
    fold_at = lambda k: native.fold_records_at(opts, rec, H, W, scale=k, **grid)
    stack = lambda: native.fold_refocus_stack(opts, consts, rec, rho, H, W, **grid)
    stack_at = lambda k: native.fold_refocus_stack_at(opts, consts, rec, rho, H, W, scale=k, **grid)

    # results must not change: bit equality before any timing
    ref, ref_stack = fold(), stack()
    one = fold_at(1)
    for m, v in ref.items():
        if not torch.equal(one[m].view(torch.int32), v.view(torch.int32)):
            raise SystemExit(f"scale 1: map {m} differs from fold_records")
    if not torch.equal(stack_at(1), ref_stack):
        raise SystemExit("scale 1: the stack differs from fold_refocus_stack")
    for k in a.scales:
        fine = fold_at(k)
        for m, v in ref.items():
            if not torch.equal(fine[m][..., ::k, ::k].contiguous().view(torch.int32), v.view(torch.int32)):
                raise SystemExit(f"scale {k}: the [::k, ::k] samples of {m} differ from fold_records")
        del fine
    del one

    rows = []
    med = alternate(fold, lambda: fold_at(1), a.repeats, a.inner)
    rows.append(dict(what="fold_records_at(scale=1) vs fold_records", size=a.size, samples=H * W, baseline_ms=med["base_a"],
                     baseline_again_ms=med["base_b"], new_ms=med["new"], ratio=med["new"] / min(med["base_a"], med["base_b"])))
    print(json.dumps(rows[-1]), flush=True)
    med = alternate(stack, lambda: stack_at(1), a.repeats, a.inner)
    rows.append(dict(what="fold_refocus_stack_at(scale=1, K=8) vs fold_refocus_stack(K=8)", size=a.size, samples=H * W,
                     baseline_ms=med["base_a"], baseline_again_ms=med["base_b"], new_ms=med["new"],
                     ratio=med["new"] / min(med["base_a"], med["base_b"])))
    print(json.dumps(rows[-1]), flush=True)
    base_ns = rows[0]["baseline_ms"] * 1e6 / (H * W)
    for k in a.scales:
        n = ((H - 1) * k + 1) * ((W - 1) * k + 1)
        inner = max(1, a.inner // k)
        for name, fn in (("fold_records_at", lambda: fold_at(k)), ("fold_refocus_stack_at(K=8)", lambda: stack_at(k))):
            for _ in range(WARMUP):
                fn()
            torch.cuda.synchronize()
            ms = statistics.median(timed(fn, inner) for _ in range(a.repeats))
            rows.append(dict(what=f"{name}(scale={k})", size=a.size, samples=n, new_ms=ms, ns_per_sample=ms * 1e6 / n,
                             fold_records_ns_per_pixel=base_ns))
            print(json.dumps(rows[-1]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
