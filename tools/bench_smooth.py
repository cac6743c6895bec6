#!/usr/bin/env python3
"""Time mesh smoothing on the GPU (profiles/HISTORY.md): the setup (native.mesh_smooth at iters=0: flags, the edge table, the scan,
the rows, the quantisation and the finalisation - everything but the steps), one step as (the whole at 20 iterations - the whole at
10) / 20, the whole of native.mesh_smooth at iters=10 and native.mesh_normals, on the meshes of the 8-view volumes of
tools/bench_tsdf.py.  Beside it the same 10 iterations in stock torch operators - index_add_ on int64 over the slot lists, the
float64 operations of the statement -, whose slot lists, valences and boundary flags are the statement's, uploaded before the clock
starts: it has no setup of its own and compares with 20 steps, not with the whole.  Whether its positions equal the statement's is reported.
Before anything is timed the GPU results must equal the statement be_hip/smooth.py bit for bit.  No threshold is set: it is a
measurement.

Device events around --inner calls per repeat, 5 warm-ups, --repeats timed repeats; the median, and the least and the largest
repeat beside it as the spread.  Everything is timed whole, allocation included.  There is no CPU path: without a GPU the script
fails.

usage: python tools/bench_smooth.py [--repeats 20] [--inner 10] [--volumes 64x64x64 256x147x147] [--json FILE]
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
from bench_simplify import spread_ms  # noqa: E402


def torch_lists(host, dev):
    """The statement's rows, valences and movable flags (boundary held) of a host mesh, on the device."""
    from be_hip import smooth
    V = len(host["vertices"])
    vu, f, fu = smooth.usable(host)
    f = f[fu]
    valence, bnd = smooth._adjacency(V, f)
    nb, start = smooth.rows(V, f)
    owner = np.repeat(np.arange(V), 2 * valence)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(owner=up(owner), nb=up(nb), n=up((2 * valence).astype(np.float64)), movable=up((valence > 0) & ~bnd), usable=up(vu))


def torch_smooth(vertices, L, iters=10, lam=0.5, mu=-0.53):
    """The statement's iteration in stock operators -> vertices' [V,3] float32."""
    x = torch.where(L["usable"][:, None], vertices, torch.zeros_like(vertices)).double()
    Q0 = torch.round(x * 2.0 ** 30).long()
    Q = Q0
    for f in [lam, mu] * iters:
        S = torch.zeros_like(Q).index_add_(0, L["owner"], Q[L["nb"]])
        d = S.double() / L["n"][:, None] - Q.double()
        Q = Q + torch.where(L["movable"][:, None], torch.round(f * d), torch.zeros_like(d)).long()
    same = (Q == Q0).all(1, keepdim=True)
    return torch.where(same, vertices, (Q.double() * 2.0 ** -30).float())


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
        raise SystemExit("bench_smooth: no GPU is visible; this measurement has no CPU form")
    import utils
    from be_hip import camera, native, smooth
    dev = torch.device("cuda:0")
    dcal = utils.DepthEtas(utils.get_args("eval", argv=[]), dev)
    C, trunc, nviews, z_range = 3, 0.05, 8, (0.7, 1.25)
    H, W = (int(v) for v in a.size.split("x"))
    cam = dcal.intrinsics(H, W)
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
        # the statement first: nothing is timed that does not equal it
        same = lambda t, r: (t is None and r is None) or (t.dtype == torch.from_numpy(np.ascontiguousarray(r)).dtype
                                                          and np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(r).view(np.uint8)))
        for kw in (dict(iters=0), dict(iters=10), dict(iters=20), dict(iters=10, boundary="free", normals="recompute")):
            ref, got = smooth.smooth(host, **kw), native.mesh_smooth(m, **kw)
            if not all(same(got[k], ref[k]) for k in ("vertices", "normal", "normal_valid", "valence", "boundary", "displacement")):
                raise SystemExit(f"{vname}, {kw}: the GPU result and the statement be_hip/smooth.py disagree")
        ref_n, got_n, ref_a, got_a = smooth.vertex_normals(host), native.mesh_normals(m), smooth.adjacency(host), native.mesh_adjacency(m)
        if not (all(same(got_n[k], ref_n[k]) for k in ref_n) and all(same(got_a[k], ref_a[k]) for k in ref_a)):
            raise SystemExit(f"{vname}: mesh_normals or mesh_adjacency and the statement disagree")
        ref10 = smooth.smooth(host)
        L = torch_lists(host, dev)
        torch_equal = bool(same(torch_smooth(m["vertices"], L), ref10["vertices"]))   # reported, not demanded: it is the comparison, not the product
        whole = {i: spread_ms(lambda i=i: native.mesh_smooth(m, iters=i), a.repeats, a.inner) for i in (0, 10, 20)}
        ms = dict(setup_ms=whole[0], mesh_smooth_ms=whole[10], mesh_smooth_20_ms=whole[20], step_ms=round((whole[20][0] - whole[10][0]) / 20, 5),
                  adjacency_ms=spread_ms(lambda: native.mesh_adjacency(m), a.repeats, a.inner),
                  normals_ms=spread_ms(lambda: native.mesh_normals(m), a.repeats, a.inner),
                  torch_20_steps_ms=spread_ms(lambda: torch_smooth(m["vertices"], L), a.repeats, max(1, a.inner // 5)))
        rows.append(dict(volume=vname, views=nviews, vertices=V, triangles=T, slots=int(L["nb"].shape[0]), moved=int((ref10["displacement"] > 0).sum()),
                         boundary=int(ref10["boundary"].sum()), longest_row=int(2 * ref10["valence"].max()), torch_equals_statement=torch_equal, kernel_traces="not measured",
                         table_probes="not measured", lanes_per_row_variant="not measured",
                         timing="[median, least, largest] ms over %d repeats of %d calls" % (a.repeats, a.inner), **ms))
        print(json.dumps(rows[-1]), flush=True)
        del sc, vol, m, L
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
