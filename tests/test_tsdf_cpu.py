"""The numpy statement of the truncated signed distance volume (be_hip/volume.py) tied to other statements of the same thing: a
2 x 2 x 2 volume worked by hand, a fronto-parallel plane on which trilinear interpolation is exact, the same function in float64,
the freedom from the order and the grouping of the views, and the quality figures of the prototype (profiles/HISTORY.md).  No GPU:
the kernels are held to volume.integrate / mean / raycast bit for bit by test_tsdf_gpu.py."""
import numpy as np
import pytest

from be_hip import camera, volume
import fuse_scenes as fs

_F = np.float32
# the volume of the prototype: 96 x 40 x 56 voxels (Nz, Ny, Nx) of (18, 17.5, 6) mm in (X, Y, Z) from (-0.5, -0.35, 0.62)
DIMS, ORIGIN, VOXEL, TRUNC = (96, 40, 56), (-0.5, -0.35, 0.62), (0.018, 0.0175, 0.006), 0.04
Z_RANGE = (0.65, 1.25)


def _same_sums(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in ((a.sw, b.sw), (a.swd, b.swd), (a.swf, b.swf)))


_VOLUMES = {}


def _scene_volume(V, dtype=np.float32):
    """The prototype's volume with views 0 .. V-1 of fuse_scenes.scene(V) integrated, once per (V, dtype)."""
    if (V, dtype) not in _VOLUMES:
        _VOLUMES[V, dtype] = volume.integrate(volume.Volume(DIMS, ORIGIN, VOXEL, TRUNC), fs.scene(V), fs.NEAR, dtype)
    return _VOLUMES[V, dtype]


_CASTS = {}


def _scene_cast(V, dtype=np.float32):
    if (V, dtype) not in _CASTS:
        _CASTS[V, dtype] = volume.raycast(_scene_volume(V, dtype), fs.CAM, None, fs.SIZE, Z_RANGE, dtype=dtype)
    return _CASTS[V, dtype]


# ------------------------------------------------------------------------------------------ 1. a volume worked by hand
def test_hand_worked_volume():
    """Camera (fy, fx, cy, cx) = (1, 1, 0, 0), one pixel: depth 13/16 = 0.8125, weight 0.5, one channel 0.25; identity pose.
    Volume 2 x 2 x 2: x, y in {0, 1/8}, z in {1/2, 1}, trunc 1/2.  Every centre projects to u = x / z in {0, 1/8, 1/4}, so
    su = floorf(u + 0.5) = 0 (and sv likewise): all 8 voxels read the one sample.  wq = floorf(0.5 * 256 + 0.5) = 128.
      z = 1/2: sdf = 13/16 - 1/2 = 5/16, / trunc = 5/8, dq = floorf(5/8 * 32768 + 0.5) = 20480, swd = 128 * 20480 = 2621440
      z = 1:   sdf = 13/16 - 1 = -3/16 >= -1/2, / trunc = -3/8, dq = floorf(-12288 + 0.5) = -12288, swd = -1572864
      fq = 0.25 * 65536 = 16384, swf = 128 * 16384 = 2097152
    Means: D = 5/8 on the near plane, -3/8 on the far one, W = 128 / 256 = 0.5, Fm = 0.25.
    The ray of pixel (0, 0) of the same camera is the axis x = y = 0: gx = gy = 0, gz = (z - 1/2) / (1/2), valid while
    floorf(gz) = 0, and F = 5/8 + gz * (-3/8 - 5/8) = 5/8 - gz.  With z_near = 1/2 and step = trunc / 4 = 1/8:
      z = 1/2: F = 5/8;  5/8: 3/8;  3/4: 1/8;  7/8: gz = 3/4, F = -1/8 <= 0 -> the hit, between 3/4 and 7/8:
      a = (1/8) / (1/8 + 1/8) = 1/2, depth = 3/4 + (1/8) * (1/2) = 13/16 - the sample's depth; weight 0.5, channel 0.25."""
    cam = camera.Pinhole(1, 1, 0, 0)
    vol = volume.Volume((2, 2, 2), (0, 0, 0.5), (0.125, 0.125, 0.5), 0.5, C=1)
    view = dict(depth=np.full((1, 1), 0.8125, _F), weight=np.full((1, 1), 0.5, _F), feat=np.full((1, 1, 1), 0.25, _F), cam_src=cam, pose=None)
    assert volume.integrate_view(vol, view) == 8
    assert vol.sw.dtype == np.int32 and vol.swd.dtype == np.int64 and vol.swf.dtype == np.int64
    assert (vol.sw == 128).all()
    assert (vol.swd[0] == 2621440).all() and (vol.swd[1] == -1572864).all()
    assert (vol.swf == 2097152).all()
    D, W, Fm = volume.mean(vol)
    assert D.dtype == _F and (D[0] == 0.625).all() and (D[1] == -0.375).all() and (W == 0.5).all() and (Fm == 0.25).all()
    out = volume.raycast(vol, cam, None, (1, 1), (0.5, 1.0))
    assert out["valid"].all() and out["depth"][0, 0] == _F(0.8125) and out["weight"][0, 0] == _F(0.5) and out["feat"][0, 0, 0] == _F(0.25)
    # a second view of the same sample doubles every sum and moves no mean
    volume.integrate_view(vol, view)
    assert (vol.sw == 256).all() and (vol.swd[0] == 2 * 2621440).all()
    assert np.array_equal(volume.mean(vol)[0], D)
    # a range that starts behind the crossing, and one that ends before it: no hit
    for zr in ((0.875, 1.0), (0.5, 0.75)):
        miss = volume.raycast(vol, cam, None, (1, 1), zr)
        assert not miss["valid"].any() and miss["depth"][0, 0] == 0 and miss["weight"][0, 0] == 0 and miss["feat"][0, 0, 0] == 0


# ------------------------------------------------------------------------------------------ 2. a plane: interpolation is exact
def test_fronto_parallel_plane_is_recovered():
    """One identity view of the plane Z = 0.9137 (off every sample position 0.65 + 0.0125 i and every voxel plane 0.62 + 0.006 i): the
    projective signed distance Zq - Z is linear in z and constant across x and y, so trilinear interpolation is exact.  What is left
    is two dq values each off by at most half of trunc / 32768 = 0.76e-6 m, and a few float32 ulps at 1 m: 1e-5 m bounds it."""
    trunc = 0.05
    vol = volume.Volume(DIMS, ORIGIN, VOXEL, trunc)
    volume.integrate(vol, [dict(depth=np.full(fs.SIZE, 0.9137, _F), weight=None, feat=None, cam_src=fs.CAM, pose=None)])
    out = volume.raycast(vol, fs.CAM, None, fs.SIZE, Z_RANGE)
    err = np.abs(out["depth"][out["valid"]].astype(np.float64) - float(_F(0.9137)))
    print(f"plane: {int(out['valid'].sum())} of {out['valid'].size} pixels hit, worst error {err.max():.3e} m")
    assert out["valid"].mean() > 0.8                                     # the frame's rim lacks observed corners, nothing else does
    assert err.max() <= 1e-5
    assert (out["depth"][~out["valid"]] == 0).all() and out["feat"] is None
    assert np.allclose(out["weight"][out["valid"]], 1.0, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------ 3. float32 against float64
@pytest.mark.parametrize("V", [1, 5, 8])
def test_float32_against_float64(V):
    """The float64 evaluation is the same function at dtype=np.float64.  valid may differ on at most 1 % of the pixels (a sample
    on the edge of a cell, or F_cur <= 0 on the decision boundary); where both hit, depth agrees to 2e-6 m = 16 ulps at 1 m (the
    hit formula divides two interpolated values).  Measured: profiles/HISTORY.md."""
    a, b = _scene_cast(V), _scene_cast(V, np.float64)
    differ = int((a["valid"] != b["valid"]).sum())
    both = a["valid"] & b["valid"]
    worst = float(np.abs(a["depth"][both].astype(np.float64) - b["depth"][both]).max())
    print(f"V = {V}: valid differs on {differ} of {both.size} pixels, depth differs by at most {worst:.3e} m on {int(both.sum())}")
    assert differ <= 0.01 * both.size
    assert both.sum() > 100 and worst <= 2e-6


# ------------------------------------------------------------------------------------------ 4. order and grouping
def test_neither_the_order_nor_the_grouping_of_the_views_changes_a_bit():
    views = fs.scene(5, C=2)
    new = lambda: volume.Volume(DIMS, ORIGIN, VOXEL, TRUNC, C=2)
    ref = volume.integrate(new(), views)
    assert int((ref.sw != 0).sum()) > 10000 and (ref.swf != 0).any()
    for perm in ((4, 3, 2, 1, 0), (2, 0, 4, 1, 3)):
        assert _same_sums(ref, volume.integrate(new(), [views[i] for i in perm]))
    one_by_one = new()
    for v in views:
        volume.integrate(one_by_one, [v])
    assert _same_sums(ref, one_by_one)
    two_calls = volume.integrate(volume.integrate(new(), views[:2]), views[2:])
    assert _same_sums(ref, two_calls)


# ------------------------------------------------------------------------------------------ 5. quality
def test_quality_on_the_fusion_scene():
    """fuse_scenes.quality on the ray cast from view 0.  No pixel lands on the wrong surface, the RMSE falls with the views and
    stays under the scene's own noise of 1 cm, and 8 views cover at least 0.9 of the frame (the prototype: coverage 0.14 / 0.92 /
    0.97 and RMSE 0.62 / 0.38 / 0.31 cm at 1 / 5 / 8 views; fuse at 8 views: 0.47 cm at 0.999)."""
    q = {V: fs.quality(_scene_cast(V)) for V in (1, 5, 8)}
    for V in (1, 5, 8):
        print(f"V = {V}: coverage {q[V]['coverage']:.3f}, rmse {100 * q[V]['rmse']:.3f} cm, wrong {q[V]['wrong']}")
        assert q[V]["wrong"] == 0
        assert q[V]["rmse"] < 0.01
    assert q[1]["rmse"] > q[5]["rmse"] > q[8]["rmse"]
    assert q[8]["coverage"] >= 0.9


# ------------------------------------------------------------------------------------------ 6. rejected inputs
def test_rejected_inputs():
    ok = dict(dims=(4, 4, 4), origin=(0, 0, 0), voxel=(0.01, 0.01, 0.01), trunc=0.05)
    volume.Volume(**ok)
    bad = [dict(dims=(0, 4, 4)), dict(dims=(4, 4, 1025)), dict(dims=(4, 4)), dict(dims=(4, 4, 2.5)), dict(dims=(True, 4, 4)), dict(dims=None),
           dict(voxel=(0.01, 0, 0.01)), dict(voxel=(0.01, -1, 0.01)), dict(voxel=(0.01, float("nan"), 0.01)), dict(voxel=(0.01, float("inf"), 0.01)),
           dict(voxel=0.01), dict(origin=(0, float("nan"), 0)), dict(origin=(0, 0)),
           dict(trunc=0), dict(trunc=-0.05), dict(trunc=4.5), dict(trunc=float("nan")), dict(trunc="x"),
           dict(C=-1), dict(C=65), dict(C=1.5), dict(C=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            volume.Volume(**dict(ok, **kw))
    # the largest volume the bounds allow, 2^30 voxels, passes the checks (no tensor is made)
    assert volume.check_params("t", (1024, 1024, 1024), ok["origin"], ok["voxel"], 0.05, 64)[0] == (1024, 1024, 1024)
    vol = volume.Volume(**ok)
    for kw in (dict(step=0), dict(step=-0.01), dict(step=float("nan")), dict(step=float("inf")), dict(step=1e-6),
               dict(z_range=(0, 1)), dict(z_range=(1.0, 0.5)), dict(z_range=(0.5, float("inf"))), dict(z_range=0.5)):
        with pytest.raises(ValueError):
            volume.raycast(vol, fs.CAM, None, (2, 2), **dict(dict(z_range=(0.5, 1.0)), **kw))
    assert volume.check_raycast("t", (0.5, 1.0), None, 0.05)[2:] == (float(_F(0.05) / _F(4)), 41)
    # a view must carry the volume's channels
    view = dict(depth=np.ones((3, 3), _F), weight=None, feat=np.ones((2, 3, 3), _F), cam_src=fs.CAM, pose=None)
    with pytest.raises(ValueError):
        volume.integrate(vol, [view])
    with pytest.raises(ValueError):
        volume.integrate(volume.Volume(**ok, C=2), [dict(view, feat=None)])
    with pytest.raises(ValueError):
        volume.integrate(vol, [dict(view, feat=None, weight=np.ones((2, 3), _F))])


def test_the_inverse_pose_undoes_the_pose():
    import reproject_scenes as rs
    p = rs.reference_pose()
    q = volume.inverse_pose(p)
    assert q.dtype == _F and q.shape == (12,)
    R, t, Rq, tq = (a.astype(np.float64) for a in (p[:9].reshape(3, 3), p[9:], q[:9].reshape(3, 3), q[9:]))
    assert np.array_equal(Rq, R.T) and np.abs(Rq @ t + tq).max() < 1e-7
    assert np.array_equal(volume.inverse_pose(None), camera.pose())


def test_the_fusion_settings_file_takes_a_volume(tmp_path):
    from be_hip import workflow as wf
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    np.savez(tmp_path / "plain.npz", poses=poses)
    assert "tsdf" not in wf.load_fusion(str(tmp_path / "plain.npz"))
    np.savez(tmp_path / "vol.npz", poses=poses, tsdf_dims=(8, 4, 6), tsdf_origin=(-0.5, 0, 0.25), tsdf_voxel=(0.5, 0.25, 0.125))
    assert wf.load_fusion(str(tmp_path / "vol.npz"))["tsdf"] == dict(dims=(8, 4, 6), origin=(-0.5, 0.0, 0.25), voxel=(0.5, 0.25, 0.125),
                                                                    trunc=float(_F(0.05)))
    for name, kw in (("a", dict(tsdf_dims=(8, 4, 6))), ("b", dict(tsdf_trunc=0.05)),
                     ("c", dict(tsdf_dims=(8, 4, 0), tsdf_origin=(0, 0, 0), tsdf_voxel=(1, 1, 1))),
                     ("d", dict(tsdf_dims=(8, 4, 6), tsdf_origin=(0, 0, 0), tsdf_voxel=(1, 1, 1), tsdf_trunc=5.0))):
        np.savez(tmp_path / f"{name}.npz", poses=poses, **kw)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / f"{name}.npz"))
