"""The numpy statement of the multi-view depth merge (be_hip/fusion.py) tied to other statements of the same thing: the z-buffer
of camera.splat_f32 at tau = 0 with one view, a hand-worked scene whose every term is exact in binary, the merge written without
the peel machinery, the unquantised float64 mean, and the quality figures of the prototype (profiles/HISTORY.md).  No GPU: the
kernels are held to fusion.fuse bit for bit by test_fuse_gpu.py."""
import numpy as np
import pytest

from be_hip import camera, fusion
import fuse_scenes as fs
import reproject_scenes as rs

_F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _one(depth, cam_src, pose=None, scale=1, origin=(0, 0), weight=None, feat=None):
    return dict(depth=depth, weight=weight, feat=feat, cam_src=cam_src, pose=pose, scale=scale, window_origin=origin)


# ------------------------------------------------------------------------------------------ 1. tau = 0, one view: the z-buffer
@pytest.mark.parametrize("case", ["scene", 1, 3, 2])
def test_tau_0_with_one_view_is_the_z_buffer_bit_for_bit(case):
    if case == "scene":
        v = fs.scene(1)[0]
        view, dst, size, near = dict(v, weight=None), fs.CAM, fs.SIZE, fs.NEAR
    else:
        c = rs.lattice_case(case)
        view, dst, size, near = _one(c["depth"], rs.SRC, c["pose"], c["scale"], c["origin"]), rs.DST, rs.SIZE, rs.NEAR
    ref = camera.splat_f32(view["depth"], view["cam_src"], dst, view["pose"], size, None, near, view["scale"], view["window_origin"])
    out = fusion.fuse([view], dst, size, tau=0, min_views=1, recentre=False, peel=0, near=near)
    assert ref["valid"].sum() > 100
    assert np.array_equal(_bits(out["depth"]), _bits(ref["depth"])) and np.array_equal(out["valid"], ref["valid"])
    assert np.array_equal(out["views"], ref["valid"].astype(np.int32)) and np.array_equal(out["layer"], np.where(ref["valid"], 0, -1))
    if case != "scene":
        # collisions included: count holds the samples that tie with the winner, at least one wherever something landed
        n_in, filled, _ = rs.COUNTS[case]
        assert int(ref["taking_part"].sum()) == n_in and int(out["valid"].sum()) == filled and (out["count"][ref["valid"]] >= 1).all()
        assert out["count"].sum() <= n_in
    # recentring at tau = 0 measures from the mean itself: the same depth
    again = fusion.fuse([view], dst, size, tau=0, min_views=1, recentre=True, peel=0, near=near)
    assert np.array_equal(_bits(again["depth"]), _bits(ref["depth"]))


# ------------------------------------------------------------------------------------------ 2. the hand-worked scene
def test_hand_worked_two_views_every_term_exact():
    """Two views of the plane Z = 1 through HAND_CAM (9 x 12), the second moved so that its samples land 3 columns to the right
    (rs.HAND_POSE), every weight 1.  The second view's sample (4, 5) is at Z = 1.03125 with weight 0.5: it lands on column
    64 (x_n 1.03125 + 3/64) / 1.03125 + 6 = 5 + 2.909 -> 8 of row 4, where view 0 has Z = 1, weight 1.
    tau = 0.0625, no recentring.  On that pixel base = 1, d = (0, 0.03125), dq = (0, 32768), wq = (65536, 32768):
    sw = 98304, swd = 2^30, depth = 1 + (2^30 / 98304) 2^-20 = 1 + 0.03125 / 3 rounded to float32 once, weight 1.5, views 2, count 2.
    Columns 3..11 elsewhere: both views at Z = 1, depth 1, weight 2, views 2.  Columns 0..2: view 0 alone, weight 1, views 1."""
    d1 = rs.shift_scene().copy()
    d1[4, 5] = 1.03125
    w1 = np.ones((9, 12), _F)
    w1[4, 5] = 0.5
    views = [_one(rs.shift_scene(), rs.HAND_CAM, weight=np.ones((9, 12), _F)), _one(d1, rs.HAND_CAM, rs.HAND_POSE, weight=w1)]
    out = fusion.fuse(views, rs.HAND_CAM, (9, 12), tau=0.0625, min_views=1, recentre=False)
    depth = np.ones((9, 12), _F)
    depth[4, 8] = _F(1 + 0.03125 / 3)
    weight = np.full((9, 12), 2, _F)
    weight[:, :3] = 1
    weight[4, 8] = 1.5
    nviews = np.full((9, 12), 2, np.int32)
    nviews[:, :3] = 1
    assert np.array_equal(_bits(out["depth"]), _bits(depth)) and out["valid"].all()
    assert np.array_equal(out["weight"], weight) and np.array_equal(out["views"], nviews) and np.array_equal(out["count"], nviews)
    assert (out["layer"] == 0).all() and out["feat"] is None
    # min_views = 2 drops the three columns only view 0 sees
    two = fusion.fuse(views, rs.HAND_CAM, (9, 12), tau=0.0625, min_views=2, recentre=False)
    assert not two["valid"][:, :3].any() and two["valid"][:, 3:].all() and np.array_equal(_bits(two["depth"][:, 3:]), _bits(depth[:, 3:]))
    assert (two["layer"][:, :3] == -1).all() and not two["weight"][:, :3].any() and not two["depth"][:, :3].any()
    # tau below the offset: the far sample does not agree; the pixel is view 0's alone
    near = fusion.fuse(views, rs.HAND_CAM, (9, 12), tau=0.03, min_views=1, recentre=False)
    assert near["depth"][4, 8] == 1 and near["weight"][4, 8] == 1 and near["views"][4, 8] == 1
    # ... and with min_views = 2 and one round of peeling the pixel stays empty: behind the peeled front is one view again
    peeled = fusion.fuse(views, rs.HAND_CAM, (9, 12), tau=0.03, min_views=2, recentre=False, peel=1)
    assert peeled["layer"][4, 8] == -1 and (peeled["layer"][:, 3:].ravel() == 0).sum() == 9 * 9 - 1
    # the channels are the weighted means: a constant 3 and the view number
    for v, view in enumerate(views):
        view["feat"] = np.stack([np.full((9, 12), 3, _F), np.full((9, 12), v, _F)])
    f = fusion.fuse(views, rs.HAND_CAM, (9, 12), tau=0.0625, recentre=False)["feat"]
    assert (f[0] == 3).all() and (f[1, :, :3] == 0).all() and f[1, 4, 8] == _F(0.5 / 1.5) and f[1, 0, 5] == 0.5


# ------------------------------------------------------------------------------------------ 3. order, and the peel machinery
@pytest.mark.parametrize("outliers", [False, True])
def test_view_permutation_leaves_every_output_bit_equal(outliers):
    views = fs.scene(5, outliers=outliers, C=2)
    kw = dict(tau=0.05, min_views=2, recentre=True, peel=2)
    first = fusion.fuse(views, fs.CAM, fs.SIZE, **kw)
    assert 0 < (first["layer"] == 1).sum() or not outliers
    for perm in ([4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
        assert fs.same(first, fusion.fuse([views[i] for i in perm], fs.CAM, fs.SIZE, **kw))


@pytest.mark.parametrize("recentre", [False, True])
@pytest.mark.parametrize("min_views", [1, 2])
@pytest.mark.parametrize("outliers", [False, True])
def test_peel_0_equals_the_merge_without_the_peel_machinery(outliers, min_views, recentre):
    views = fs.scene(5, outliers=outliers, C=1)
    for tau in (0.0, 0.05):
        out = fusion.fuse(views, fs.CAM, fs.SIZE, tau=tau, min_views=min_views, recentre=recentre, peel=0)
        assert fs.same(out, fs.fuse_one_layer(views, fs.CAM, fs.SIZE, tau, min_views, recentre))
        # further rounds never touch a pixel that round 0 kept
        more = fusion.fuse(views, fs.CAM, fs.SIZE, tau=tau, min_views=min_views, recentre=recentre, peel=2)
        keep = out["valid"]
        assert (more["layer"][keep] == 0).all() and np.array_equal(_bits(more["depth"][keep]), _bits(out["depth"][keep]))
        assert (more["layer"][~keep] != 0).all()


# ------------------------------------------------------------------------------------------ 4. the fixed-point error
def test_fixed_point_error_against_the_float64_mean():
    """Weights in [0.25, 1], tau = 0.05: each offset is quantised to 2^-20 m (off by <= 2^-21 = 4.8e-7), each weight to 2^-16 (2^-15
    relative to 0.25, which moves a mean of offsets <= 0.1 by <= 3.1e-6), the result is rounded to float32 (<= 6e-8 at 1.1 m): the
    bound of 1e-5 m is the sum with room; measured 6e-7 in the prototype."""
    worst = 0.0
    for V, recentre, outliers in ((8, True, False), (8, False, False), (5, True, True)):
        out = fusion.fuse(fs.scene(V, outliers=outliers), fs.CAM, fs.SIZE, tau=0.05, recentre=recentre, peel=2, min_views=2 if outliers else 1,
                          want_members=True)
        ref = fusion.mean_f64(out)
        ok = out["valid"]
        assert ok.sum() > 1500 and np.isfinite(ref[ok]).all() and np.isnan(ref[~ok]).all()
        err = np.abs(out["depth"][ok].astype(np.float64) - ref[ok]).max()
        print(f"V = {V}, recentre {recentre}, outliers {outliers}: fixed point against the float64 mean, max |error| {err:.3e} m")
        worst = max(worst, err)
    assert worst <= 1e-5


# ------------------------------------------------------------------------------------------ 5. the quality figures
def test_quality_more_views_more_coverage_less_noise():
    single = fs.quality(fusion.fuse(fs.scene(1), fs.CAM, fs.SIZE, tau=0.05, recentre=True))
    print(f"1 view: coverage {single['coverage']:.3f}, RMSE {100 * single['rmse']:.2f} cm, wrong-surface {single['wrong']}")
    # 30 % dropout over 1961 pixels: 0.70 with a standard deviation of 0.01
    assert 0.66 <= single["coverage"] <= 0.74 and single["wrong"] == 0
    for V, cov, ratio in ((5, 0.98, 0.70), (8, 0.99, 0.55)):
        q = fs.quality(fusion.fuse(fs.scene(V), fs.CAM, fs.SIZE, tau=0.05, recentre=True))
        print(f"{V} views: coverage {q['coverage']:.3f}, RMSE {100 * q['rmse']:.2f} cm = {q['rmse'] / single['rmse']:.2f} of the single view's, "
              f"wrong-surface {q['wrong']}")
        assert q["coverage"] >= cov and q["rmse"] / single["rmse"] <= ratio and q["wrong"] == 0


def test_quality_min_views_and_peeling_reject_outliers():
    views = fs.scene(5, outliers=True)
    run = lambda **kw: fusion.fuse(views, fs.CAM, fs.SIZE, tau=0.05, recentre=True, **kw)
    one, two, peeled = run(min_views=1), run(min_views=2, peel=0), run(min_views=2, peel=2)
    q1, q2, q3 = fs.quality(one), fs.quality(two), fs.quality(peeled)
    layers = [int((peeled["layer"] == r).sum()) for r in range(3)]
    print(f"outliers, 5 views: min_views 1: wrong-surface {q1['wrong']}; min_views 2: {q2['wrong']}, coverage {q2['coverage']:.3f}; "
          f"min_views 2, peel 2: {q3['wrong']}, coverage {q3['coverage']:.3f}, layers {layers}")
    assert q1["wrong"] >= 50
    assert q2["wrong"] <= 3 and q2["coverage"] < 0.90
    assert q3["wrong"] <= 3 and q3["coverage"] >= 0.92
    assert layers == [1729, 102, 1]


# ------------------------------------------------------------------------------------------ 6. samples and parameters
def test_weights_and_channels_are_quantised_as_stated():
    w = np.array([0, -1, np.nan, np.inf, 16, 17, 1, 0.25, 2.0 ** -17, 2.0 ** -18, 1e-30], _F)
    assert fusion.quantise_weight(w).tolist() == [0, 0, 0, 1 << 20, 1 << 20, 1 << 20, 65536, 16384, 1, 0, 0]
    f = np.array([np.nan, np.inf, -np.inf, 3000, -3000, 1, -1, 2.0 ** -17, -(2.0 ** -17), 0.3], _F)
    assert fusion.quantise_feat(f).tolist() == [0, 1 << 27, -(1 << 27), 1 << 27, -(1 << 27), 65536, -65536, 1, 0, 19661]
    v = fs.scene(1)[0]
    planted = v["weight"].copy()
    planted[0, :4] = [0, -1, np.nan, 2.0 ** -18]
    base = fusion.view_samples(v, fs.CAM, fs.SIZE)
    s = fusion.view_samples(dict(v, weight=planted), fs.CAM, fs.SIZE)
    lost = np.setdiff1d(base["src"], s["src"])
    assert set(lost) <= {0, 1, 2, 3} and len(lost) == int((v["depth"][0, :4] > 0).sum())


def test_parameters_are_checked():
    views = fs.scene(3)
    for kw, match in ((dict(tau=-0.01), "tau"), (dict(tau=float("nan")), "tau"), (dict(tau=4.5), "tau"), (dict(min_views=0), "min_views"),
                      (dict(min_views=4), "min_views"), (dict(peel=-1), "peel"), (dict(peel=9), "peel"), (dict(min_views=1.5), "min_views")):
        with pytest.raises(ValueError, match=match):
            fusion.fuse(views, fs.CAM, fs.SIZE, **kw)
    with pytest.raises(ValueError, match="views"):
        fusion.fuse([], fs.CAM, fs.SIZE)
    with pytest.raises(ValueError, match="views"):
        fusion.fuse(views * 11, fs.CAM, fs.SIZE)
    with pytest.raises(ValueError, match="feat"):
        fusion.fuse([views[0], dict(views[1], feat=np.zeros((1,) + fs.SIZE, _F))], fs.CAM, fs.SIZE)
