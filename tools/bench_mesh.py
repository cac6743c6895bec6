#!/usr/bin/env python3
"""Time mesh extraction on the GPU (profiles/HISTORY.md): the count phase (k_mesh_cells, k_mesh_edges and the two scans), the scan
alone, the emit phase (k_mesh_vertices, k_mesh_faces) and the whole of native.tsdf_mesh - tsdf_mean, count, the read-back of the
two totals, allocation, emit - on the 8-view volumes of tools/bench_tsdf.py, beside native.tsdf_raycast of the same volume into
view 0; and native.exclusive_scan beside torch.cumsum on the same counts (the per-voxel vertex counts, uint8 in, int32 out for
the scan, int32 in and out for cumsum, which has no uint8 -> int32 form).  No threshold is set: it is a measurement.

Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats, medians.  The phases are timed through the C
ABI on buffers allocated once; tsdf_mesh is timed whole, its synchronisation included.  There is no CPU path: without a GPU the
script fails.

usage: python tools/bench_mesh.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--size 147x147] [--json FILE]
"""
import argparse
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
from bench_render_at import WARMUP, timed  # noqa: E402


def median_ms(fn, repeats, inner):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    return statistics.median(timed(fn, inner) for _ in range(repeats))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--volumes", nargs="+", default=["64x64x64", "256x147x147"])
    ap.add_argument("--size", default="147x147")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native
    from be_hip.native import dptr, stream_ptr, check, _iptr, _fptr
    dev = torch.device("cuda:0")
    lib = native.lib()
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    C, trunc, V, z_range = 3, 0.05, 8, (0.7, 1.25)
    H, W = (int(v) for v in a.size.split("x"))
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
        D, Wt, Fm = native.tsdf_mean(vol)
        n = D.numel()
        idims, origin, voxel = np.array(dims, np.int32), np.array(vol.origin, np.float32), np.array(vol.voxel, np.float32)
        nt, mask = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
        voff, toff = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
        totals = torch.empty(2, dtype=torch.int64, device=dev)
        nbytes = lib.be_tsdf_mesh_workspace_bytes(n)
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        u8, i64 = (torch.uint8,), (torch.int64,)

        def count():
            check(lib.be_tsdf_mesh_count_f32(dptr(D), dptr(Wt), _iptr(idims), 0.0, dptr(nt, "nt", u8), dptr(mask, "mask", u8), dptr(voff), dptr(toff),
                                             dptr(totals, "totals", i64), dptr(ws, "ws", i64), nbytes, stream_ptr(dev)), "count")

        count()
        nV, nT = totals.tolist()
        vertices, normal = (torch.empty(nV, 3, dtype=torch.float32, device=dev) for _ in range(2))
        faces = torch.empty(nT, 3, dtype=torch.int32, device=dev)
        weight = torch.empty(nV, dtype=torch.float32, device=dev)
        feat = torch.empty(C, nV, dtype=torch.float32, device=dev)
        nvalid = torch.empty(nV, dtype=torch.bool, device=dev)
        edge = torch.empty(nV, dtype=torch.int64, device=dev)

        def emit():
            check(lib.be_tsdf_mesh_emit_f32(dptr(D), dptr(Wt), dptr(Fm), C, _iptr(idims), _fptr(origin), _fptr(voxel), 0.0, dptr(nt, "nt", u8),
                                            dptr(mask, "mask", u8), dptr(voff), dptr(toff), nV, nT, dptr(vertices), dptr(faces), dptr(weight),
                                            dptr(feat), dptr(normal), dptr(nvalid, "normal_valid", (torch.bool,)), dptr(edge, "edge", i64),
                                            stream_ptr(dev)), "emit")

        emit()
        whole = native.tsdf_mesh(vol)
        if not (torch.equal(whole["faces"], faces) and torch.equal(whole["vertices"].view(torch.int32), vertices.view(torch.int32))):
            raise SystemExit(f"{vname}: the phases timed alone and native.tsdf_mesh disagree")
        counts = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.uint8, device=dev)[mask.long()]
        counts32 = counts.to(torch.int32)
        off, tot = native.exclusive_scan(counts)
        cs = torch.cumsum(counts32, 0, dtype=torch.int32)
        if not (torch.equal(off[1:], cs[:-1]) and int(tot) == int(cs[-1]) == nV and torch.equal(off, voff)):
            raise SystemExit(f"{vname}: native.exclusive_scan, torch.cumsum and the count phase disagree")
        ms = dict(count_ms=median_ms(count, a.repeats, a.inner), scan_ms=median_ms(lambda: native.exclusive_scan(counts), a.repeats, a.inner),
                  cumsum_ms=median_ms(lambda: torch.cumsum(counts32, 0, dtype=torch.int32), a.repeats, a.inner),
                  emit_ms=median_ms(emit, a.repeats, a.inner), tsdf_mesh_ms=median_ms(lambda: native.tsdf_mesh(vol), a.repeats, a.inner),
                  mean_ms=median_ms(lambda: native.tsdf_mean(vol), a.repeats, a.inner),
                  raycast_ms=median_ms(lambda: native.tsdf_raycast(vol, cam, None, (H, W), z_range), a.repeats, a.inner))
        rows.append(dict(volume=vname, size=a.size, views=V, voxels=n, vertices=nV, triangles=nT, **ms,
                         count_bytes_per_voxel_min=8 + 2 + 8, count_gb_per_s=n * 18 / (ms["count_ms"] * 1e6)))
        print(json.dumps(rows[-1]), flush=True)
        del sc, vol, D, Wt, Fm, whole
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
