"""Host geometry of the forward reprojection (be_hip/camera.py): the intrinsics the pipeline's own constants imply, poses, and the
numpy float32 statement of the kernels (project_f32, splat_f32) on scenes worked by hand - every term exact in binary - and on the
reference scene against the same function in float64.  No GPU."""
import numpy as np
import pytest

from be_hip import camera
import reproject_scenes as rs


def test_pinhole_of_the_default_camera_and_poses():
    import utils
    a = utils.get_args("eval", argv=[])
    cam = camera.Pinhole.of(a.cam_params, a.mag, 147, 147)
    assert cam.focal_px == 0.1104 / (5.86e-6 * 4) and cam.fy == cam.fx == cam.focal_px
    assert abs(cam.focal_px - 4709.9) < 0.05
    assert (cam.cy, cam.cx) == (73.0, 73.0)
    assert camera.Pinhole.of(a.cam_params, a.mag, 200, 262).tuple()[2:] == (99.5, 130.5)
    # a K matrix, the 4 numbers and the keyword form are one camera
    K = np.array([[58, 0, 25.7], [0, 60, 18.2], [0, 0, 1]])
    assert camera.Pinhole(K) == camera.Pinhole(60, 58, 18.2, 25.7) == camera.Pinhole((60, 58, 18.2, 25.7)) == rs.SRC
    assert np.array_equal(camera.Pinhole(K).K(), K)
    for bad in ((60, 58, 18.2), np.eye(4), np.array([[58, 1, 25.7], [0, 60, 18.2], [0, 0, 1]])):
        with pytest.raises(ValueError, match="Pinhole"):
            camera.Pinhole(bad)
    with pytest.raises(ValueError, match="focal"):
        camera.Pinhole(0, 58, 1, 1)
    # poses
    eye = camera.pose()
    assert eye.dtype == np.float32 and eye.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
    p = rs.reference_pose()
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = p[:9].astype(np.float64).reshape(3, 3), p[9:]
    assert np.array_equal(camera.pose(M), p) and np.array_equal(camera.as_pose(M[:3]), p) and np.array_equal(camera.as_pose(p), p)
    with pytest.raises(ValueError, match="rotation"):
        camera.pose(np.diag([1, 1, 1.001]))
    with pytest.raises(ValueError, match="rotation"):
        camera.pose(np.diag([1, 1, -1]))                                # a reflection
    bad = M.copy()
    bad[:3, :3] *= 2
    with pytest.raises(ValueError, match="rotation"):
        camera.pose(bad)
    with pytest.raises(ValueError, match="last row"):
        camera.pose(2 * M)
    with pytest.raises(ValueError, match="4x4"):
        camera.pose(M, (0, 0, 0))
    with pytest.raises(ValueError, match="pose"):
        camera.as_pose(np.zeros(7))


def test_depth_etas_intrinsics():
    import utils
    a = utils.get_args("eval", argv=[])
    d = utils.DepthEtas(a, "cpu")
    assert d.focal_px == 0.1104 / (5.86e-6 * 4)
    assert d.intrinsics(147, 147) == camera.Pinhole.of(a.cam_params, a.mag, 147, 147)
    assert d.intrinsics(200, 262).tuple() == (d.focal_px, d.focal_px, 99.5, 130.5)


def test_hand_worked_shift():
    r = camera.splat_f32(rs.shift_scene(), rs.HAND_CAM, rs.HAND_CAM, rs.HAND_POSE, (9, 12))
    depth, index = rs.expected_shift()
    assert r["depth"].dtype == np.float32 and r["index"].dtype == np.int32
    assert np.array_equal(r["depth"], depth) and np.array_equal(r["index"], index)
    assert np.array_equal(r["valid"], index >= 0) and not r["valid"][:, :3].any() and r["valid"][:, 3:].all()
    assert int(r["taking_part"].sum()) == 9 * 9                         # source columns 9..11 leave the frame


def test_occlusion_the_nearer_surface_wins():
    d = rs.occlusion_scene()
    feat = rs.feat_for(9, 12, 2)
    r = camera.splat_f32(d, rs.HAND_CAM, rs.HAND_CAM, rs.HAND_POSE, (9, 12), feat=feat)
    depth, index = rs.expected_occlusion()
    assert np.array_equal(r["depth"], depth) and np.array_equal(r["index"], index)
    sq = r["depth"][3:6, 8:11]
    assert (sq == 0.5).all() and np.array_equal(r["index"][3:6, 8:11], np.arange(3, 6)[:, None] * 12 + np.arange(2, 5)[None, :])
    assert (d[3:6, 5:8] == 1.0).all()                                   # background samples do land under the square
    assert np.array_equal(r["feat"][:, r["valid"]], feat.reshape(2, -1)[:, r["index"][r["valid"]]])
    assert (r["feat"][:, ~r["valid"]] == 0).all()


def test_tie_the_lowest_source_index_wins():
    r = camera.splat_f32(rs.shift_scene(), rs.TIE_SRC, rs.TIE_DST, None, rs.TIE_SIZE)
    assert r["valid"].all() and (r["depth"] == 1.0).all()
    assert np.array_equal(r["index"], rs.expected_tie())
    assert r["index"][1, 1] == 1 * 12 + 1 and r["index"][4, 6] == 7 * 12 + 11     # of (1|2, 1|2) and (7|8, 11)


@pytest.mark.parametrize("k", [1, 3, 2])
def test_project_f32_against_float64_on_the_reference_scene(k):
    scale, win, (Hs, Ws) = rs.LATTICES[k]
    d = rs.lattice_depth(k)
    assert d.shape == (Hs, Ws) and d.dtype == np.float32
    pose = rs.reference_pose()
    p32 = camera.project_f32(d, rs.SRC, rs.DST, pose, scale, win[:2])
    p64 = camera.project(d, rs.SRC, rs.DST, pose, scale, win[:2], np.float64)
    assert p32["xyz"].dtype == np.float32 and p64["xyz"].dtype == np.float64
    ok = p32["z_ok"]
    assert np.array_equal(ok, d > 0) and np.array_equal(ok, p64["z_ok"])
    # the float32 and float64 target pixels agree for every sample, Zd to 2e-7 relative
    assert np.array_equal(p32["fu"][ok].astype(np.float64), p64["fu"][ok]) and np.array_equal(p32["fv"][ok].astype(np.float64), p64["fv"][ok])
    rel = np.abs(p32["xyz"][2][ok].astype(np.float64) - p64["xyz"][2][ok]) / p64["xyz"][2][ok]
    print(f"k = {k}: Zd float32 against float64, relmax {rel.max():.3e}")
    assert rel.max() <= 2e-7
    # the table of the scene: samples in frame, target pixels filled, collisions
    r = camera.splat(p32, rs.SIZE, rs.NEAR)
    n, filled = int(r["taking_part"].sum()), int(r["valid"].sum())
    assert (n, filled, n - filled) == rs.COUNTS[k]
    assert np.array_equal(r["taking_part"], camera.taking_part(p64, rs.SIZE, rs.NEAR))
    r64 = camera.splat(p64, rs.SIZE, rs.NEAR)
    assert np.array_equal(r64["valid"], r["valid"])
    # unproject: the points, 0 where the depth is invalid
    xyz = camera.unproject_f32(d, rs.SRC, pose, scale, win[:2])
    assert np.array_equal(xyz[:, ok], p32["xyz"][:, ok]) and (xyz[:, ~ok] == 0).all()
    hit = r["valid"]
    assert np.array_equal(r["depth"][hit], xyz[2].ravel()[r["index"][hit]])


def test_rejected_samples_on_the_host():
    d = rs.shift_scene().copy()
    d[0, :4] = [0, -1, np.nan, np.inf]
    r = camera.splat_f32(d, rs.HAND_CAM, rs.HAND_CAM, None, (9, 12))
    assert not r["valid"][0, :4].any() and r["valid"].sum() == 9 * 12 - 4 and np.isfinite(r["depth"]).all()
    assert (r["depth"][0, :4].view(np.uint32) == 0).all() and (r["index"][0, :4] == -1).all()
    # behind near: the plane at Z = 1 pulled back by 1 - 1e-3 / 2
    r = camera.splat_f32(rs.shift_scene(), rs.HAND_CAM, rs.HAND_CAM, camera.pose(None, (0, 0, -0.9995)), (9, 12), near=1e-3)
    assert not r["valid"].any()
    # a finite depth on the optical axis whose Zd overflows: 3e38 under a pose that adds 3e38 more; u = finite / inf + cx would be the principal point
    d = rs.shift_scene().copy()
    d[4, 6] = 3e38
    p = camera.project_f32(d, rs.HAND_CAM, rs.HAND_CAM, camera.pose(None, (0, 0, 3e38)))
    assert np.isinf(p["xyz"][2][4, 6]) and p["z_ok"][4, 6] and (p["fv"][4, 6], p["fu"][4, 6]) == (4, 6)
    r = camera.splat(p, (9, 12))
    assert not r["taking_part"][4, 6] and r["taking_part"].sum() == 9 * 12 - 1      # the others, Zd = 3e38, all land on (4, 6)
    assert r["valid"].sum() == 1 and r["index"][4, 6] == 0 and np.isfinite(r["depth"]).all()


def test_eval_arguments():
    import utils
    a = utils.get_args("eval", argv=[])
    assert a.point_cloud is False and a.reproject is None               # off by default
    a = utils.get_args("eval", big=True, argv=["--point_cloud", "--reproject", "cam.npz", "--out_path", "x"])
    assert (a.point_cloud, a.reproject, a.out_path) == (True, "cam.npz", "x")


@pytest.mark.parametrize("k", [1, 3, 2])
def test_float32_statement_against_float64_splat(k):
    """The second guard of the GPU tests, applied to the host statement itself."""
    r = rs.lattice_case(k)["r32"]
    rs.check_against_f64(k, r["depth"], r["index"], r["valid"], r["feat"])
