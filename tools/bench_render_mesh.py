#!/usr/bin/env python3
"""Time mesh rasterisation on the GPU (profiles/HISTORY.md): native.raster_mesh - a memset, k_raster_vertices, k_raster_faces and
k_raster_resolve - of the meshes of the 8-view volumes of tools/bench_tsdf.py / bench_mesh.py into view 0's camera at 147 x 147
and at 587 x 587 (the same view, 4 samples per pixel pitch), beside native.tsdf_raycast of the same volume into the same camera.
Before anything is timed the GPU's result is compared with the host statement raster.render, bit for bit.  No threshold is set: it
is a record, with no earlier time to compare with.

Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats, medians.  There is no CPU path: without a GPU
the script fails.

The three kernels separately: device events cannot see inside one call, so they come from a kernel trace of this script,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_render_mesh.py --volumes 256x147x147 --sizes 587x587
    python tools/bench_render_mesh.py --kernel-stats DIR
which prints calls and the average time of every k_raster_* kernel in the trace (one volume and one size per trace, so that an
average belongs to one shape).

usage: python tools/bench_render_mesh.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--sizes 147x147 587x587] [--json FILE]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "blurry-edges_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fuse import scene  # noqa: E402
from bench_mesh import median_ms  # noqa: E402


def kernel_stats(root):
    """The k_raster_* rows of the kernel_stats.csv files under `root` -> [dict(kernel, calls, average_us)]."""
    rows = []
    for path in sorted(glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True)):
        for r in csv.DictReader(open(path)):
            name = r.get("Name", "")
            if "k_raster_" in name:
                short = name[name.index("k_raster_"):].split("(")[0]
                rows.append(dict(kernel=short, calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3))
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--volumes", nargs="+", default=["64x64x64", "256x147x147"])
    ap.add_argument("--sizes", nargs="+", default=["147x147", "587x587"])
    ap.add_argument("--json", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    a = ap.parse_args(argv)
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        if not rows:
            raise SystemExit(f"bench_render_mesh: no k_raster_* kernel in a kernel_stats.csv under {a.kernel_stats}")
        for r in rows:
            print(json.dumps(r))
        return
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_render_mesh: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native, raster
    dev = torch.device("cuda:0")
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    C, trunc, V, z_range = 3, 0.05, 8, (0.7, 1.25)
    H, W = 147, 147                                                      # the views' own size
    cam = dcal.intrinsics(H, W)
    rows = []
    for vname in a.volumes:
        dims = tuple(int(v) for v in vname.split("x"))
        half_x, half_y = 0.55 * W / cam.fx * z_range[1], 0.55 * H / cam.fy * z_range[1]
        desc = dict(dims=dims, origin=(-half_x, -half_y, z_range[0]), trunc=trunc,
                    voxel=(2 * half_x / (dims[2] - 1), 2 * half_y / (dims[1] - 1), (z_range[1] - z_range[0]) / (dims[0] - 1)))
        sc = scene(H, W, V, dev, C)
        vol = native.tsdf_integrate(native.tsdf_volume(C=C, device=dev, **desc),
                                    [dict(depth=d, weight=w, feat=f, cam_src=cam, pose=camera.pose(None, t)) for d, w, f, t in sc], near=1e-3)
        mesh = native.tsdf_mesh(vol)
        host = {k: None if t is None else t.cpu().numpy() for k, t in mesh.items()}
        for sname in a.sizes:
            Ho, Wo = (int(v) for v in sname.split("x"))
            k = (Wo - 1) / (W - 1)                                       # 587 = 4 * 146 + 1: view 0 sampled 4 times per pixel pitch
            target = camera.Pinhole(cam.fy * (Ho - 1) / (H - 1), cam.fx * k, (Ho - 1) / 2, (Wo - 1) / 2)
            got = native.raster_mesh(mesh, target, None, (Ho, Wo))
            ref = raster.render(host, target, None, (Ho, Wo))
            for key, r in ref.items():
                g = got[key].cpu().numpy()
                same = np.array_equal(g.view(np.uint32), r.view(np.uint32)) if r.dtype == np.float32 else np.array_equal(g, r)
                if not same:
                    raise SystemExit(f"{vname} at {sname}: native.raster_mesh and raster.render disagree in {key}")
            cast = native.tsdf_raycast(vol, target, None, (Ho, Wo), z_range)
            both = got["valid"] & cast["valid"]
            ms = dict(raster_mesh_ms=median_ms(lambda: native.raster_mesh(mesh, target, None, (Ho, Wo)), a.repeats, a.inner),
                      raster_depth_only_ms=median_ms(lambda: native.raster_mesh(mesh, target, None, (Ho, Wo), want=()), a.repeats, a.inner),
                      raycast_ms=median_ms(lambda: native.tsdf_raycast(vol, target, None, (Ho, Wo), z_range), a.repeats, a.inner))
            rows.append(dict(volume=vname, size=sname, views=V, vertices=int(mesh["vertices"].shape[0]), triangles=int(mesh["faces"].shape[0]),
                             pixels_seen=int(got["valid"].sum()), pixels_cast=int(cast["valid"].sum()),
                             median_abs_diff_to_raycast_m=float((got["depth"] - cast["depth"])[both].abs().median()) if bool(both.any()) else None,
                             bit_equal_to_statement=True, **ms))
            print(json.dumps(rows[-1]), flush=True)
        del sc, vol, mesh, host
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
