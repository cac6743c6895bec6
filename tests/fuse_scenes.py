"""The inputs the multi-view fusion tests share (test_fuse_cpu.py, test_fuse_gpu.py): a square at 0.80 m in front of a wall at
1.10 m, seen by up to 8 translated views of one 37 x 53 camera with noise, dropout and random weights; an outlier variant; the
quality counts; and the statement of the merge without the peel machinery."""
import numpy as np

from be_hip import camera, fusion

CAM = camera.Pinhole(60, 58, 18.2, 25.7)
SIZE = (37, 53)
NEAR = 1e-3
_F = np.float32


def view_translation(v):
    return (0.0, 0.0, 0.0) if v == 0 else (0.04 * np.cos(2.4 * v), 0.03 * np.sin(2.4 * v), 0.01 * (v % 3 - 1))


def truth(v):
    """The depth view v sees, by ray casting in float64 (R = I: the view's frame is the target's moved by -t)."""
    tx, ty, tz = view_translation(v)
    H, W = SIZE
    yn = ((np.arange(H) - CAM.cy) / CAM.fy)[:, None]
    xn = ((np.arange(W) - CAM.cx) / CAM.fx)[None, :]
    zs = 0.80 - tz
    X, Y = xn * zs + tx, yn * zs + ty
    return np.where((-0.12 < X) & (X < 0.10) & (-0.08 < Y) & (Y < 0.09), zs, 1.10 - tz)


_SCENES = {}


def scene(V=8, sigma=0.01, outliers=False, C=0):
    """-> a list of V view dicts (fusion.VIEW_KEYS).  One default_rng(5) runs through the views; per view it draws the noise, the
    dropout mask (30 %, depth 0) and the weights 0.25 + 0.75 u, in that order.  outliers: one default_rng(9) pulls 2 % of each
    view's samples 0.3 m forward.  C > 0: C channels from their own generator ride along (they do not disturb the other draws)."""
    key = (V, sigma, outliers, C)
    if key not in _SCENES:
        rng, out_rng, f_rng = np.random.default_rng(5), np.random.default_rng(9), np.random.default_rng(11)
        views = []
        for v in range(V):
            d = truth(v) + sigma * rng.standard_normal(SIZE)
            d[rng.random(SIZE) < 0.3] = 0
            w = 0.25 + 0.75 * rng.random(SIZE)
            if outliers:
                d = np.where((out_rng.random(SIZE) < 0.02) & (d > 0), d - 0.3, d)
            feat = f_rng.standard_normal((C,) + SIZE).astype(_F) if C else None
            views.append(dict(depth=d.astype(_F), weight=w.astype(_F), feat=feat, cam_src=CAM, pose=camera.pose(None, view_translation(v)),
                              scale=1, window_origin=(0, 0)))
        _SCENES[key] = views
    return _SCENES[key]


def quality(out):
    """-> dict(coverage = the share of all pixels that hold a depth; rmse (metres) and wrong = the number of pixels with
    |error| > 0.15 m, both over the pixels further than 1 from the truth's depth step) of a fusion result in the frame of view 0."""
    t = truth(0)
    H, W = SIZE
    p = np.pad(t, 1, mode="edge")
    step = np.zeros(SIZE, bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            step |= p[dy:dy + H, dx:dx + W] != t
    keep = ~step
    ok = out["valid"] & keep
    err = out["depth"][ok].astype(np.float64) - t[ok]
    return dict(coverage=float(out["valid"].mean()), rmse=float(np.sqrt(np.mean(err ** 2))), wrong=int((np.abs(err) > 0.15).sum()),
                pixels=int(keep.sum()))


def fuse_one_layer(views, cam_dst, size, tau, min_views, recentre, near=1e-3):
    """The merge at peel = 0 written without rounds, floors or a done state: one front over every sample that takes part, add, mean,
    the optional recentred pass, and the view-count test."""
    Ho, Wo = size
    No = Ho * Wo
    S = [fusion.view_samples(v, cam_dst, size, near) for v in views]
    C = S[0]["fq"].shape[0]
    tau = _F(tau)
    zmin = np.full(No, fusion.EMPTY, np.uint32)
    for s in S:
        np.minimum.at(zmin, s["dst"], s["zd"].view(np.uint32))
    base, span = zmin.view(_F), tau
    sw, swd, cnt, mask, swf = fusion._add(S, base, span, C, No)
    m = fusion._mean(base, sw, swd, cnt)
    if recentre:
        base, span = (m - tau).astype(_F), tau + tau
        sw, swd, cnt, mask, swf = fusion._add(S, base, span, C, No)
        m = fusion._mean(base, sw, swd, cnt)
    pop = fusion._popcount(mask)
    fin = (cnt > 0) & (pop >= min_views)
    with np.errstate(invalid="ignore", divide="ignore"):
        weight = (sw.astype(np.float64) * 2.0 ** -16).astype(_F)
        feat = (swf.astype(np.float64) / sw.astype(np.float64) * 2.0 ** -16).astype(_F)
    z = np.zeros(No, _F)
    r = lambda a: a.reshape(Ho, Wo)
    return dict(depth=r(np.where(fin, m, z)), valid=r(fin), weight=r(np.where(fin, weight, z)), views=r(np.where(fin, pop, 0).astype(np.int32)),
                count=r(np.where(fin, cnt, 0).astype(np.int32)), layer=r(np.where(fin, 0, -1).astype(np.int32)),
                feat=np.where(fin[None], feat, z).reshape(C, Ho, Wo) if C else None)


def same(a, b, keys=("depth", "valid", "weight", "views", "count", "layer", "feat")):
    """Two results (numpy) are equal bit for bit in every output."""
    for k in keys:
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (k, int((x != y).sum()))
    return True
