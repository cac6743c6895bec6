#!/usr/bin/env python3
"""Time mesh cleaning on the GPU (profiles/HISTORY.md): the labelling (be_mesh_components_i32: init, link, flatten, the scan, the
ids), the per-component sums (be_mesh_components_stats), the selection (be_mesh_select_count and _emit) and the whole of
native.mesh_clean - label, stats, decide, count, the one read-back, emit - on the meshes of the 8-view volumes of
tools/bench_tsdf.py, beside native.tsdf_mesh of the same volume and beside the same labelling in stock torch operators: minimum
propagation with scatter_reduce_(amin) and pointer jumping to a fixed point, one read-back of a changed flag per round.  Before
anything is timed the GPU results must equal the statement be_hip/components.py bit for bit.  No threshold is set: it is a
measurement.

Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats, medians.  The phases are timed through the C
ABI on buffers allocated once; mesh_clean and tsdf_mesh are timed whole, their synchronisation included.  There is no CPU path:
without a GPU the script fails.

usage: python tools/bench_components.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--min_triangles 50] [--json FILE]
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

from bench_fuse import scene  # noqa: E402
from bench_mesh import median_ms  # noqa: E402


def torch_labels(faces, V):
    """The least index of every vertex's component in stock operators -> (label [V] int64, rounds)."""
    f = faces.long()
    flat = f.reshape(-1)
    lab = torch.arange(V, device=faces.device)
    rounds = 0
    while True:
        rounds += 1
        before = lab
        l = lab[f]
        m = l.amin(1, keepdim=True).expand(-1, 3).reshape(-1)
        lab = lab.clone()
        lab.scatter_reduce_(0, l.reshape(-1), m, "amin")
        lab.scatter_reduce_(0, flat, m, "amin")
        while True:
            nxt = lab[lab]
            if torch.equal(nxt, lab):
                break
            lab = nxt
        if torch.equal(lab, before):
            return lab, rounds


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--volumes", nargs="+", default=["64x64x64", "256x147x147"])
    ap.add_argument("--size", default="147x147")
    ap.add_argument("--min_triangles", type=int, default=50)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if a.repeats < 20:
        raise SystemExit("--repeats must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_components: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, components, native
    from be_hip.native import dptr, stream_ptr, check
    dev = torch.device("cuda:0")
    lib = native.lib()
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    C, trunc, nviews, z_range = 3, 0.05, 8, (0.7, 1.25)
    H, W = (int(v) for v in a.size.split("x"))
    cam = dcal.intrinsics(H, W)
    i64, u8 = (torch.int64,), (torch.bool,)
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
        # the statement first: nothing is timed that does not equal it
        host = {k: None if v is None else v.cpu().numpy() for k, v in m.items()}
        ref = components.clean(host, min_triangles=a.min_triangles)
        lab = components.label(V, host["faces"])
        got_lab, got = native.mesh_components(m), native.mesh_clean(m, min_triangles=a.min_triangles)
        same = lambda t, r: t.dtype == torch.from_numpy(r).dtype and np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(r).view(np.uint8))
        ok = all(same(got_lab[k], lab[k]) for k in ("label", "component", "face_component")) and got_lab["K"] == lab["K"]
        ok = ok and all(same(got["components"][k], ref["components"][k]) for k in ("triangles", "vertices", "area_q", "area", "keep"))
        ok = ok and all(same(got[k], ref[k]) for k in ("vertices", "faces", "weight", "feat", "normal", "normal_valid", "edge", "vertex_index",
                                                       "face_index", "component"))
        if not ok:
            raise SystemExit(f"{vname}: the GPU result and the statement be_hip/components.py disagree")
        tl, rounds = torch_labels(m["faces"], V)
        if not torch.equal(tl.int(), got_lab["label"]):
            raise SystemExit(f"{vname}: the torch labelling and native.mesh_components disagree")
        K, V2, T2 = lab["K"], ref["vertices"].shape[0], ref["faces"].shape[0]
        new = lambda *s, dtype=torch.int32: torch.empty(*s, dtype=dtype, device=dev)
        label, component, fc, total = new(V), new(V), new(T), new(1, dtype=torch.int64)
        nb = lib.be_mesh_components_workspace_bytes(V)
        ws = new((nb + 7) // 8, dtype=torch.int64)
        tri, nv, aq = new(K), new(K), new(K, dtype=torch.int64)
        vk = got_lab["component"].new_zeros(V, dtype=torch.bool)
        vk[got["vertex_index"].long()] = True
        voff, foff, totals = new(V), new(T), new(2, dtype=torch.int64)
        nbs = lib.be_mesh_select_workspace_bytes(V, T)
        wss = new((nbs + 7) // 8, dtype=torch.int64)
        o = dict(v=new(V2, 3, dtype=torch.float32), f=new(T2, 3), w=new(V2, dtype=torch.float32), ft=new(C, V2, dtype=torch.float32),
                 n=new(V2, 3, dtype=torch.float32), nv=new(V2, dtype=torch.bool), e=new(V2, dtype=torch.int64), vi=new(V2), fi=new(T2))

        def f_label():
            check(lib.be_mesh_components_i32(dptr(m["faces"]), V, T, dptr(label), dptr(component), dptr(fc), dptr(total, "total", i64),
                                             dptr(ws, "ws", i64), nb, stream_ptr(dev)), "label")

        def f_stats():
            check(lib.be_mesh_components_stats(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(component), K, dptr(tri), dptr(nv),
                                               dptr(aq, "area_q", i64), stream_ptr(dev)), "stats")

        def f_select():
            check(lib.be_mesh_select_count(dptr(m["faces"]), V, T, dptr(vk, "vk", u8), dptr(voff), dptr(foff), dptr(totals, "totals", i64),
                                           dptr(wss, "ws", i64), nbs, stream_ptr(dev)), "count")
            check(lib.be_mesh_select_emit(dptr(m["vertices"]), dptr(m["faces"]), V, T, dptr(m["weight"]), dptr(m["feat"]), C, dptr(m["normal"]),
                                          dptr(m["normal_valid"], "nv", u8), dptr(m["edge"], "edge", i64), None, dptr(vk, "vk", u8), dptr(voff),
                                          dptr(foff), V2, T2, dptr(o["v"]), dptr(o["f"]), dptr(o["w"]), dptr(o["ft"]), dptr(o["n"]),
                                          dptr(o["nv"], "nv", u8), dptr(o["e"], "edge", i64), None, dptr(o["vi"]), dptr(o["fi"]), stream_ptr(dev)),
                  "emit")

        f_label(), f_stats(), f_select()
        if not (torch.equal(label, got_lab["label"]) and torch.equal(aq, got_lab["area_q"]) and torch.equal(o["f"], got["faces"])
                and totals.tolist() == [V2, T2]):
            raise SystemExit(f"{vname}: the phases timed alone and native.mesh_clean disagree")
        ms = dict(label_ms=median_ms(f_label, a.repeats, a.inner), stats_ms=median_ms(f_stats, a.repeats, a.inner),
                  select_ms=median_ms(f_select, a.repeats, a.inner),
                  mesh_clean_ms=median_ms(lambda: native.mesh_clean(m, min_triangles=a.min_triangles), a.repeats, a.inner),
                  tsdf_mesh_ms=median_ms(lambda: native.tsdf_mesh(vol), a.repeats, a.inner),
                  torch_label_ms=median_ms(lambda: torch_labels(m["faces"], V), a.repeats, max(1, a.inner // 5)))
        sizes = np.sort(ref["components"]["triangles"])[::-1]
        rows.append(dict(volume=vname, views=nviews, vertices=V, triangles=T, components=K, largest=sizes[:4].tolist(), min_triangles=a.min_triangles,
                         vertices_kept=V2, triangles_kept=T2, torch_rounds=rounds, link_retries="not measured", **ms))
        print(json.dumps(rows[-1]), flush=True)
        del sc, vol, m, got, got_lab
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
