"""The contract of the multi-view depth merge (native.fuse_views, DepthPipeline.fuse) as pure numpy: to k_fuse_front, k_fuse_add
and k_fuse_step of csrc/be_fuse.hip what camera.splat is to be_reproject.hip.  Nothing here needs a GPU.

V views (1 <= V <= 32), each a depth map with weights and channels riding on it, its own camera and its pose into the target
frame, are merged in one target camera.  A sample takes part iff it passes camera.taking_part (reproject's test) under
camera.project_f32, its weight w is > 0 (NaN fails) and its quantised weight wq = floorf(min(w, 16) * 65536 + 0.5) is non-zero (a
None weight: wq = 65536).  Per target pixel, in rounds r = 0..peel:

  front   zmin = the minimum, over the samples on the pixel that take part and lie behind the pixel's floor (Zd > floor, floor 0 at
          the start), of the bits of Zd as uint32; all-ones = none
  add     base = zmin as a float, span = tau: a sample agrees iff d = Zd - base satisfies 0 <= d <= span; with
          dq = floorf(d * 2^20 + 0.5): sw += wq, swd += wq * dq, cnt += 1, mask |= 1 << v, swf_c += wq * fq_c with
          fq_c = floorf(clamp(f, -2048, 2048) * 65536 + 0.5) (NaN counts as 0)
  mean    m = (float)((double) base + (double) swd / (double) sw * 2^-20) where cnt > 0
  recentre (optional) base = m - tau (NaN where cnt == 0), span = tau + tau, the sums cleared, add and mean again: measuring
          from the noisy front biases the mean forward, measuring symmetrically about the first mean removes most of that
  decide  a pixel not yet done with cnt > 0 and popcount(mask) >= min_views is finalised in layer r: depth = m,
          weight = sw * 2^-16, views = popcount(mask), count = cnt, feat_c = swf_c / sw * 2^-16; with cnt > 0 and too few views
          its front cluster is peeled off (floor = base + span) and the next round looks behind it; with cnt == 0 nothing is left

Every sum is an integer under an associative, commutative operation (min, add, or), so the result depends neither on the order of
execution nor on the order of the views.  The sums are exact in 64 bits while fewer than 2^16 samples agree on one pixel
(wq <= 2^20, dq <= 2^23, |fq| <= 2^27); that limit is documented, not checked.  The unit of a depth offset is 2^-20 m; against the
unquantised float64 mean over the same members the result is within 1e-5 m for weights >= 0.25 and tau <= 0.05 (each offset is
off by at most 2^-21 m = 4.8e-7, each weight by at most 2^-17, which is 2^-15 of a weight >= 0.25 and moves a mean of offsets
<= 0.1 m by at most 3.1e-6 m, and the final rounding to float32 is 6e-8 m at 1 m; measured 5.8e-7 m).

With tau = 0, recentre off, peel = 0, min_views = 1 and one view, depth and valid are camera.splat_f32's, bit for bit."""
from __future__ import annotations

import numpy as np

from . import camera

_F = np.float32
MAX_VIEWS, MAX_TAU, MAX_PEEL = 32, 4.0, 8
W_MAX, F_MAX = 16.0, 2048.0
EMPTY = np.uint32(0xFFFFFFFF)
VIEW_KEYS = ("depth", "weight", "feat", "cam_src", "pose", "scale", "window_origin")


def quantise_weight(w):
    """w float32 -> uint64 wq = floorf(min(w, 16) * 65536 + 0.5) in float32 arithmetic where w > 0, else 0 (NaN, 0, negatives)."""
    w = np.asarray(w, _F)
    with np.errstate(invalid="ignore"):
        ok = w > 0
        q = np.floor(np.minimum(np.where(ok, w, _F(0)), _F(W_MAX)) * _F(65536) + _F(0.5))
    assert q.dtype == _F
    return q.astype(np.uint64)


def quantise_feat(f):
    """f float32 -> int64 fq = floorf(min(max(f, -2048), 2048) * 65536 + 0.5) in float32 arithmetic; NaN counts as 0."""
    f = np.asarray(f, _F)
    f = np.where(np.isnan(f), _F(0), f)
    q = np.floor(np.minimum(np.maximum(f, _F(-F_MAX)), _F(F_MAX)) * _F(65536) + _F(0.5))
    assert q.dtype == _F
    return q.astype(np.int64)


def check_params(who, V, tau, min_views, recentre, peel):
    """The parameter checks native.fuse_views and this statement share -> (tau as float, min_views, recentre, peel)."""
    if not 1 <= V <= MAX_VIEWS:
        raise ValueError(f"{who}: views must hold 1 to {MAX_VIEWS} views, got {V}")
    try:
        tau = float(tau)
    except (TypeError, ValueError):
        tau = -1.0
    if not 0 <= tau <= MAX_TAU:                                         # NaN fails
        raise ValueError(f"{who}: tau must be a finite number of metres in [0, {MAX_TAU:g}]")
    if isinstance(min_views, bool) or not isinstance(min_views, (int, np.integer)) or not 1 <= min_views <= V:
        raise ValueError(f"{who}: min_views must be an integer in [1, {V}] (the number of views), got {min_views!r}")
    if isinstance(peel, bool) or not isinstance(peel, (int, np.integer)) or not 0 <= peel <= MAX_PEEL:
        raise ValueError(f"{who}: peel must be an integer in [0, {MAX_PEEL}], got {peel!r}")
    return tau, int(min_views), bool(recentre), int(peel)


def view_samples(view, cam_dst, size, near=1e-3):
    """One view's samples that take part -> dict(zd float32 [n], dst int64 [n] = the target pixel's linear index, wq uint64 [n],
    fq int64 [C,n], w, f = the unquantised weights and channels (float32), src int64 [n] = the sample's linear index)."""
    Ho, Wo = size
    depth = np.asarray(view["depth"], _F)
    proj = camera.project_f32(depth, view["cam_src"], cam_dst, view.get("pose"), view.get("scale", 1), view.get("window_origin", (0, 0)))
    part = camera.taking_part(proj, size, near)
    weight = view.get("weight")
    w = np.ones(depth.shape, _F) if weight is None else np.asarray(weight, _F)
    if w.shape != depth.shape:
        raise ValueError(f"fuse: weight must be {depth.shape}, got {w.shape}")
    wq = quantise_weight(w)
    part = part & (wq != 0)
    src = np.flatnonzero(part.ravel())
    feat = view.get("feat")
    f = np.zeros((0, depth.size), _F) if feat is None else np.asarray(feat, _F).reshape(len(feat), -1)
    if f.shape[1] != depth.size:
        raise ValueError(f"fuse: feat must be [C,{depth.shape[0]},{depth.shape[1]}], got {np.shape(feat)}")
    zd = np.ascontiguousarray(proj["xyz"][2].astype(_F)).ravel()[src]
    dst = proj["fv"].ravel()[src].astype(np.int64) * Wo + proj["fu"].ravel()[src].astype(np.int64)
    return dict(zd=zd, dst=dst, wq=wq.ravel()[src], fq=quantise_feat(f[:, src]), w=w.ravel()[src], f=f[:, src], src=src)


def _front(samples, floor, No):
    zmin = np.full(No, EMPTY, np.uint32)
    for s in samples:
        sel = s["zd"] > floor[s["dst"]]
        np.minimum.at(zmin, s["dst"][sel], s["zd"][sel].view(np.uint32))
    return zmin


def _add(samples, base, span, C, No, members=None):
    """The sums of one add pass over every view.  members: a list that receives, per view, the agreeing samples' positions."""
    sw, swd = np.zeros(No, np.uint64), np.zeros(No, np.uint64)
    cnt, mask = np.zeros(No, np.uint32), np.zeros(No, np.uint32)
    swf = np.zeros((C, No), np.int64)
    for v, s in enumerate(samples):
        with np.errstate(invalid="ignore"):
            d = s["zd"] - base[s["dst"]]
            assert d.dtype == _F
            a = (d >= 0) & (d <= span)
            dq = np.floor(np.where(a, d, _F(0)) * _F(1 << 20) + _F(0.5))
        assert dq.dtype == _F
        dst, wq, dq = s["dst"][a], s["wq"][a], dq[a].astype(np.uint64)
        np.add.at(sw, dst, wq)
        np.add.at(swd, dst, wq * dq)
        np.add.at(cnt, dst, np.uint32(1))
        np.bitwise_or.at(mask, dst, np.uint32(1 << v))
        for c in range(C):
            np.add.at(swf[c], dst, wq.astype(np.int64) * s["fq"][c][a])
        if members is not None:
            members.append(np.flatnonzero(a))
    return sw, swd, cnt, mask, swf


def _mean(base, sw, swd, cnt):
    with np.errstate(invalid="ignore", divide="ignore"):
        m = (base.astype(np.float64) + swd.astype(np.float64) / sw.astype(np.float64) * 2.0 ** -20).astype(_F)
    return np.where(cnt > 0, m, _F(np.nan))


def _popcount(mask):
    return np.unpackbits(np.ascontiguousarray(mask, np.uint32).view(np.uint8)).reshape(-1, 32).sum(1).astype(np.int32).reshape(mask.shape)


def fuse(views, cam_dst, size, tau=0.05, min_views=1, recentre=True, peel=0, near=1e-3, want_members=False):
    """views: a list of dicts with the keys VIEW_KEYS (numpy arrays; weight, feat, pose may be None, scale 1 and window_origin (0, 0)
    by default) -> dict(depth [Ho,Wo] float32, valid bool, weight float32, views, count, layer int32, feat [C,Ho,Wo] float32 or
    None), the statement at the head of this module; depth +0, weight 0, views 0, count 0, layer -1, feat +0 where no pixel was
    finalised.  want_members: also `members`, per view the positions (into view_samples' arrays) of the samples that made each
    finalised mean, with `samples` - what the float64 comparison of the tests reads."""
    tau, min_views, recentre, peel = check_params("fuse", len(views), tau, min_views, recentre, peel)
    Ho, Wo = size
    No = Ho * Wo
    samples = [view_samples(v, cam_dst, size, near) for v in views]
    Cs = {s["fq"].shape[0] for s in samples}
    if len(Cs) != 1:
        raise ValueError(f"fuse: every view must carry the same number of feat channels, got {sorted(Cs)}")
    C = Cs.pop()
    tau32 = _F(tau)
    floor, done = np.zeros(No, _F), np.zeros(No, bool)
    depth, weight = np.zeros(No, _F), np.zeros(No, _F)
    nviews, count, layer = np.zeros(No, np.int32), np.zeros(No, np.int32), np.full(No, -1, np.int32)
    feat = np.zeros((C, No), _F)
    final_members = [np.zeros(0, np.int64) for _ in views]
    for r in range(peel + 1):
        zmin = _front(samples, floor, No)
        base, span = zmin.view(_F), tau32                               # all-ones is a NaN: it fails every test of add
        members = [] if want_members else None
        sw, swd, cnt, mask, swf = _add(samples, base, span, C, No, members)
        m = _mean(base, sw, swd, cnt)
        if recentre:
            with np.errstate(invalid="ignore"):
                base = np.where(cnt > 0, m - tau32, _F(np.nan)).astype(_F)
            span = tau32 + tau32
            members = [] if want_members else None
            sw, swd, cnt, mask, swf = _add(samples, base, span, C, No, members)
            m = _mean(base, sw, swd, cnt)
        pop = _popcount(mask)
        fin = ~done & (cnt > 0) & (pop >= min_views)
        with np.errstate(invalid="ignore", divide="ignore"):
            depth[fin] = m[fin]
            weight[fin] = (sw.astype(np.float64) * 2.0 ** -16).astype(_F)[fin]
            feat[:, fin] = (swf.astype(np.float64) / sw.astype(np.float64) * 2.0 ** -16).astype(_F)[:, fin]
            behind = (base + span).astype(_F)
        nviews[fin], count[fin], layer[fin] = pop[fin], cnt[fin].astype(np.int32), r
        if want_members:
            for v, (s, a) in enumerate(zip(samples, members)):
                final_members[v] = np.concatenate([final_members[v], a[fin[s["dst"][a]]]])
        peeled = ~done & ~fin & (cnt > 0)
        floor = np.where(peeled, behind, _F(np.inf)).astype(_F)         # finalised, exhausted (cnt == 0) and done pixels: +inf
        done |= fin
    out = dict(depth=depth.reshape(Ho, Wo), valid=(layer >= 0).reshape(Ho, Wo), weight=weight.reshape(Ho, Wo),
               views=nviews.reshape(Ho, Wo), count=count.reshape(Ho, Wo), layer=layer.reshape(Ho, Wo),
               feat=feat.reshape(C, Ho, Wo) if C else None)
    if want_members:
        out.update(members=final_members, samples=samples)
    return out


def mean_f64(out):
    """The unquantised float64 weighted mean of Zd over the members of fuse(.., want_members=True) -> float64 [Ho,Wo], NaN where
    no pixel was finalised: what the fixed-point result is measured against."""
    No = out["depth"].size
    num, den = np.zeros(No), np.zeros(No)
    for s, a in zip(out["samples"], out["members"]):
        w = np.minimum(s["w"][a].astype(np.float64), W_MAX)
        np.add.at(num, s["dst"][a], w * s["zd"][a].astype(np.float64))
        np.add.at(den, s["dst"][a], w)
    with np.errstate(invalid="ignore"):
        return (num / den).reshape(out["depth"].shape)
