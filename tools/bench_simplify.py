#!/usr/bin/env python3
"""Time mesh simplification on the GPU (profiles/HISTORY.md): the labelling (be_mesh_cluster_f32: keys, the cluster table, the
scan, the ids), the count phase (be_mesh_simplify_count: the integer sums, the face table, the flags and their scan), the emit phase
(be_mesh_simplify_emit) and the whole of native.mesh_simplify - cluster, count, the one read-back, emit - on the meshes of the 8-view
volumes of tools/bench_tsdf.py, at cells of --cells voxels from the volume's origin.  Beside it the same clustering in stock torch
operators - torch.unique(dim=0) on the cell indices, index_add_ for the sums, unique on the face triples -, which must find the
same V' and T', and native.raster_mesh of the mesh before and after.  Before anything is timed the GPU results must equal the
statement be_hip/simplify.py bit for bit.  No threshold is set: it is a measurement.

Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats; the median, and the least and the largest
repeat beside it as the spread.  The phases are timed through the C ABI on buffers allocated once; mesh_simplify, the torch form
and raster_mesh are timed whole, their synchronisation included.  There is no CPU path: without a GPU the script fails.

usage: python tools/bench_simplify.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--cells 2 3] [--json FILE]
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


def spread_ms(fn, repeats, inner):
    """-> [median, least, largest] of `repeats` timings of `inner` calls each, in ms per call."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    t = [timed(fn, inner) for _ in range(repeats)]
    return [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]


def torch_simplify(m, cell, origin, flaps=False):
    """The same clustering in stock operators -> (V', T', vertices' [V',3] float64 means): unique rows for the cells and the face
    triples, index_add_ for the sums.  Its cluster ids follow the cells' order, not the least member's; only the counts are
    compared."""
    from be_hip import fusion
    dev = m["vertices"].device
    c, o = (torch.tensor(np.asarray(x, np.float32), device=dev) for x in (cell, origin))
    inv = (1.0 / c.double()).float()
    t = (m["vertices"] - o) * inv
    i = torch.floor(t)
    w = m["weight"]
    wq = torch.where(w > 0, torch.floor(torch.clamp(w, max=fusion.W_MAX) * 65536 + 0.5), torch.zeros_like(w)).double()
    usable = (i.abs() < 2 ** 20).all(1) & (wq != 0)
    uniq, inverse = torch.unique(i[usable].long(), dim=0, return_inverse=True)
    V2 = uniq.shape[0]
    cl = torch.full((t.shape[0],), -1, dtype=torch.int64, device=dev)
    cl[usable] = inverse
    sw = torch.zeros(V2, dtype=torch.float64, device=dev).index_add_(0, inverse, wq[usable])
    pos = torch.zeros(V2, 3, dtype=torch.float64, device=dev).index_add_(0, inverse, (wq[:, None] * m["vertices"].double())[usable]) / sw[:, None]
    k = cl[m["faces"].long()]
    ok = (k >= 0).all(1) & (k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])
    k = k[ok]
    s = k.argmin(1, keepdim=True)
    a, b, c3 = (k.gather(1, (s + d) % 3).squeeze(1) for d in range(3))
    wind = (b > c3).long()
    triples, group = torch.unique(torch.stack([a, torch.minimum(b, c3), torch.maximum(b, c3)], 1), dim=0, return_inverse=True)
    seen = torch.zeros(triples.shape[0], 2, dtype=torch.bool, device=dev)
    seen[group, wind] = True
    T2 = int(seen.sum()) if flaps else int((seen.sum(1) == 1).sum())    # the read-back
    return V2, T2, pos


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--volumes", nargs="+", default=["64x64x64", "256x147x147"])
    ap.add_argument("--cells", nargs="+", type=int, default=[2, 3])
    ap.add_argument("--size", default="147x147")
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_simplify: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native, simplify
    from be_hip.native import dptr, stream_ptr, check, _fptr
    dev = torch.device("cuda:0")
    lib = native.lib()
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    C, trunc, nviews, z_range = 3, 0.05, 8, (0.7, 1.25)
    H, W = (int(v) for v in a.size.split("x"))
    cam = dcal.intrinsics(H, W)
    i64, u8, bl = (torch.int64,), (torch.uint8,), (torch.bool,)
    rows = []
    for vname in a.volumes:
        dims = tuple(int(v) for v in vname.split("x"))
        half_x, half_y = 0.55 * W / cam.fx * z_range[1], 0.55 * H / cam.fy * z_range[1]
        desc = dict(dims=dims, origin=(-half_x, -half_y, z_range[0]), trunc=trunc,
                    voxel=(2 * half_x / (dims[2] - 1), 2 * half_y / (dims[1] - 1), (z_range[1] - z_range[0]) / (dims[0] - 1)))
        sc = scene(H, W, nviews, dev, C)
        vol = native.tsdf_integrate(native.tsdf_volume(C=C, device=dev, **desc),
                                    [dict(depth=d, weight=w, feat=f, cam_src=cam, pose=camera.pose(None, t)) for d, w, f, t in sc], near=1e-3)
        m = native.tsdf_mesh(vol)
        V, T = m["vertices"].shape[0], m["faces"].shape[0]
        host = {k: None if v is None else v.cpu().numpy() for k, v in m.items()}
        raster_before = spread_ms(lambda: native.raster_mesh(m, cam, None, (H, W)), a.repeats, a.inner)
        for k in a.cells:
            cell = tuple(k * v for v in desc["voxel"])
            # the statement first: nothing is timed that does not equal it
            ref, lab = simplify.simplify(host, cell, desc["origin"]), simplify.cluster(host, cell, desc["origin"])
            got, got_lab = native.mesh_simplify(m, cell, origin=desc["origin"]), native.mesh_cluster(m, cell, origin=desc["origin"])
            same = lambda t, r: (t is None and r is None) or (t.dtype == torch.from_numpy(r).dtype
                                                              and np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(r).view(np.uint8)))
            ok = all(same(got[n], ref[n]) for n in ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge", "cluster", "members",
                                                    "face_index"))
            ok = ok and all(same(got_lab[n], lab[n]) for n in ("label", "cluster", "members")) and got_lab["V"] == lab["V"]
            if not ok:
                raise SystemExit(f"{vname}, cells of {k} voxels: the GPU result and the statement be_hip/simplify.py disagree")
            V2, T2 = ref["vertices"].shape[0], ref["faces"].shape[0]
            tv, tt, tpos = torch_simplify(m, cell, desc["origin"])
            if (tv, tt) != (V2, T2):
                raise SystemExit(f"{vname}, cells of {k} voxels: the torch form finds {tv} vertices and {tt} triangles, native.mesh_simplify {V2} and {T2}")
            gc, go = simplify.grid(cell, desc["origin"])[::2]
            new = lambda *s, dtype=torch.int32: torch.empty(*s, dtype=dtype, device=dev)
            label, cluster, members, totals = new(V), new(V), new(V), new(2, dtype=torch.int64)
            nb = lib.be_mesh_cluster_workspace_bytes(V)
            ws = new((nb + 7) // 8, dtype=torch.int64)
            nrows = lib.be_mesh_simplify_sum_rows(C, 1)
            sums, fflag, foff, totals_f = new(nrows, V, dtype=torch.int64), new(T, dtype=torch.uint8), new(T), new(2, dtype=torch.int64)
            nbs = lib.be_mesh_simplify_workspace_bytes(T)
            wss = new((nbs + 7) // 8, dtype=torch.int64)
            o = dict(v=new(V2, 3, dtype=torch.float32), f=new(T2, 3), w=new(V2, dtype=torch.float32), ft=new(C, V2, dtype=torch.float32),
                     n=new(V2, 3, dtype=torch.float32), nv=new(V2, dtype=torch.bool), fi=new(T2))

            def f_cluster():
                check(lib.be_mesh_cluster_f32(dptr(m["vertices"]), dptr(m["weight"]), V, _fptr(gc), _fptr(go), dptr(label), dptr(cluster), dptr(members),
                                              dptr(totals, "totals", i64), dptr(ws, "ws", i64), nb, stream_ptr(dev)), "cluster")

            def f_count():
                check(lib.be_mesh_simplify_count(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(m["weight"]), dptr(m["feat"]), C, dptr(m["normal"]),
                                                 dptr(m["normal_valid"], "nv", bl), _fptr(gc), _fptr(go), dptr(cluster), 0, dptr(sums, "sums", i64),
                                                 dptr(fflag, "fflag", u8), dptr(foff), dptr(totals_f, "totals", i64), dptr(wss, "ws", i64), nbs,
                                                 stream_ptr(dev)), "count")

            def f_emit():
                check(lib.be_mesh_simplify_emit(dptr(m["vertices"]), dptr(m["faces"]), V, T, _fptr(gc), _fptr(go), dptr(label), dptr(cluster),
                                                dptr(members), dptr(sums, "sums", i64), C, 1, dptr(fflag, "fflag", u8), dptr(foff), V2, T2, dptr(o["v"]),
                                                dptr(o["f"]), dptr(o["w"]), dptr(o["ft"]), dptr(o["n"]), dptr(o["nv"], "nv", bl), dptr(o["fi"]),
                                                stream_ptr(dev)), "emit")

            f_cluster(), f_count(), f_emit()
            if not (torch.equal(label, got_lab["label"]) and torch.equal(o["v"], got["vertices"]) and torch.equal(o["f"], got["faces"])
                    and totals.tolist() == [V2, 0] and totals_f.tolist() == [T2, 0]):
                raise SystemExit(f"{vname}, cells of {k} voxels: the phases timed alone and native.mesh_simplify disagree")
            ms = dict(cluster_ms=spread_ms(f_cluster, a.repeats, a.inner), count_ms=spread_ms(f_count, a.repeats, a.inner),
                      emit_ms=spread_ms(f_emit, a.repeats, a.inner),
                      mesh_simplify_ms=spread_ms(lambda: native.mesh_simplify(m, cell, origin=desc["origin"]), a.repeats, a.inner),
                      torch_ms=spread_ms(lambda: torch_simplify(m, cell, desc["origin"]), a.repeats, max(1, a.inner // 5)),
                      raster_before_ms=raster_before, raster_after_ms=spread_ms(lambda: native.raster_mesh(got, cam, None, (H, W)), a.repeats, a.inner))
            rows.append(dict(volume=vname, views=nviews, cell_voxels=k, vertices=V, triangles=T, vertices_after=V2, triangles_after=T2,
                             table_probes="not measured", timing="[median, least, largest] ms over %d repeats of %d calls" % (a.repeats, a.inner), **ms))
            print(json.dumps(rows[-1]), flush=True)
            del got, got_lab, tpos
        del sc, vol, m
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
