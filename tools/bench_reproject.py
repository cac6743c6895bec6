#!/usr/bin/env python3
"""Time the forward reprojection on the GPU (profiles/HISTORY.md, Round 14), nanoseconds per source sample: native.reproject
(memset + k_splat_zbuf + k_resolve_zbuf) against the same warp composed of stock torch operators on the same device - the
elementwise projection in float32, operation by operation, int64 keys (depth bits << 32 | source index), one
scatter_reduce_(amin) into an int64 z-buffer, and the gathers.  The torch composition is the yardstick; the kernels are not
measured against an earlier run of themselves.

Sources: a 587 x 587 and a 1080 x 1920 depth map (a far plane with a nearer block, a fifth of the pixels invalid) at scale 1 and
scale 2 (the lattice of render_at: ((H-1) k + 1) x ((W-1) k + 1) samples), three feature channels, warped onto an equal-sized
target through the pipeline's own camera and a pose a few centimetres and a few milliradians away.  Device events around --inner
calls per repeat, 5 warm-ups, --repeats timed repeats with the sides alternated in one process: torch, native, torch again - the
distance between the two torch medians is the spread a difference has to be read against.  Before timing the two results are
compared: the index maps must agree on all but a few pixels (the two sides round the same float32 operations; a division that
rounds differently may move a sample across a pixel boundary).  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_reproject.py [--repeats 20] [--inner 10] [--sizes 587x587 1080x1920] [--scales 1 2] [--json FILE]
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

EMPTY = torch.iinfo(torch.int64).max


def torch_reproject(depth, cs, cd, p, size, feat, near, k, top, left):
    """The warp of native.reproject in stock torch operators.  cs / cd / p: python floats that hold the float32 numbers."""
    Hs, Ws = depth.shape
    Ho, Wo = size
    dev = depth.device
    y = (top + torch.arange(Hs, device=dev, dtype=torch.float32) / k)[:, None]
    x = (left + torch.arange(Ws, device=dev, dtype=torch.float32) / k)[None, :]
    xn, yn = (x - cs[3]) / cs[1], (y - cs[2]) / cs[0]
    Z = depth
    X, Y = xn * Z, yn * Z
    Xd = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[9]
    Yd = ((p[3] * X + p[4] * Y) + p[5] * Z) + p[10]
    Zd = ((p[6] * X + p[7] * Y) + p[8] * Z) + p[11]
    fu = torch.floor((cd[1] * Xd) / Zd + cd[3] + 0.5)
    fv = torch.floor((cd[0] * Yd) / Zd + cd[2] + 0.5)
    part = ((Z > 0) & torch.isfinite(Z) & (Zd > near) & (fu >= 0) & (fu < Wo) & (fv >= 0) & (fv < Ho)).view(-1)
    src = torch.arange(Hs * Ws, device=dev, dtype=torch.int64)
    keys = (Zd.contiguous().view(torch.int32).to(torch.int64).view(-1) << 32) | src
    keys = torch.where(part, keys, torch.full_like(keys, EMPTY))
    dst = torch.where(part, fv.view(-1).to(torch.int64) * Wo + fu.view(-1).to(torch.int64), torch.zeros_like(src))
    zbuf = torch.full((Ho * Wo,), EMPTY, dtype=torch.int64, device=dev)
    zbuf.scatter_reduce_(0, dst, keys, "amin")
    hit = zbuf != EMPTY
    index = torch.where(hit, zbuf & 0xFFFFFFFF, torch.full_like(zbuf, -1))
    out_depth = torch.where(hit, (zbuf >> 32).to(torch.int32).view(torch.float32), torch.zeros((), device=dev))
    out_feat = torch.where(hit[None], feat.view(feat.shape[0], -1)[:, index.clamp(min=0)], torch.zeros((), device=dev))
    return dict(depth=out_depth.view(Ho, Wo), index=index.to(torch.int32).view(Ho, Wo), valid=hit.view(Ho, Wo), feat=out_feat.view(-1, Ho, Wo))


def source(H, W, k, dev):
    rng = np.random.default_rng(1)
    d = 1.05 + 0.13 * rng.random((H, W))
    d[H // 4:3 * H // 4, W // 4:3 * W // 4] = 0.75 + 0.05 * rng.random((3 * H // 4 - H // 4, 3 * W // 4 - W // 4))
    d[rng.random((H, W)) < 0.2] = 0
    d = torch.from_numpy(d.astype(np.float32)).to(dev)
    Hs, Ws = (H - 1) * k + 1, (W - 1) * k + 1
    d = d.repeat_interleave(k, 0).repeat_interleave(k, 1)[:Hs, :Ws].contiguous()
    feat = torch.rand(3, Hs, Ws, generator=torch.Generator().manual_seed(0)).to(dev)
    return d, feat


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--sizes", nargs="+", default=["587x587", "1080x1920"])
    ap.add_argument("--scales", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_reproject: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native
    dev = torch.device("cuda:0")
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    c, s = np.cos(0.004), np.sin(0.004)
    pose = camera.pose(np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), (0.03, -0.01, 0.02))
    rows = []
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        cam = dcal.intrinsics(H, W)
        cs = [float(v) for v in cam.f32()]
        p = [float(v) for v in pose]
        near = float(np.float32(1e-3))
        for k in a.scales:
            d, feat = source(H, W, k, dev)
            ns = d.numel()
            new = lambda: native.reproject(d, cam, cam, pose, (H, W), feat=feat, near=1e-3, scale=k)
            base = lambda: torch_reproject(d, cs, cs, p, (H, W), feat, near, k, 0, 0)
            got, ref = new(), base()
            differ = int((got["index"] != ref["index"]).sum())
            if differ > 1e-3 * H * W:
                raise SystemExit(f"{size} scale {k}: native.reproject and the torch composition differ on {differ} of {H * W} target pixels")
            filled = int(got["valid"].sum())
            del got, ref
            med = alternate(base, new, a.repeats, a.inner)
            rows.append(dict(size=size, scale=k, samples=ns, target_filled=filled / (H * W), pixels_that_differ=differ,
                             torch_ns_per_sample=med["base_a"] * 1e6 / ns, torch_again_ns_per_sample=med["base_b"] * 1e6 / ns,
                             native_ns_per_sample=med["new"] * 1e6 / ns, native_ms=med["new"],
                             ratio=min(med["base_a"], med["base_b"]) / med["new"]))
            print(json.dumps(rows[-1]), flush=True)
            del d, feat
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
