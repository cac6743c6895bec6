"""The inputs the reprojection tests share (test_reproject_cpu.py, test_reproject_gpu.py): the reference scene with its three source
lattices, and the hand-worked shift, occlusion and tie scenes whose every term is exact in binary."""
import numpy as np

from be_hip import camera

SRC = camera.Pinhole(60, 58, 18.2, 25.7)
DST = camera.Pinhole(75, 77, 20.3, 33.1)
SIZE = (41, 67)
NEAR = 1e-3
# lattice k -> (scale, window (top, left, h, w), samples (Hs, Ws)); in frame / target pixels filled / collisions in float32
LATTICES = {1: (1, (0, 0, 37, 53), (37, 53)), 3: (3, (5, 7, 12, 17), (34, 49)), 2: (2, (0, 0, 37, 53), (73, 105))}
COUNTS = {1: (1372, 1368, 4), 3: (1282, 287, 995), 2: (5419, 2312, 3107)}


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[axis]


def reference_pose():
    return camera.pose(rot("z", 0.05) @ rot("y", -0.03) @ rot("x", 0.02), (0.03, -0.02, 0.05))


def reference_depth():
    rng = np.random.default_rng(1)
    d = 1.05 + 0.13 * rng.random((37, 53))
    d[9:27, 14:36] = 0.75 + 0.05 * rng.random((18, 22))
    d[rng.random((37, 53)) < 0.2] = 0
    return d.astype(np.float32)


def lattice_depth(k):
    """The reference depth on lattice k: expanded by np.repeat along both axes, cropped to the window and the lattice size."""
    scale, (top, left, h, w), (Hs, Ws) = LATTICES[k]
    d = reference_depth()[top:top + h, left:left + w]
    return np.ascontiguousarray(np.repeat(np.repeat(d, scale, 0), scale, 1)[:Hs, :Ws])


def feat_for(Hs, Ws, C=5, seed=7):
    return np.random.default_rng(seed).standard_normal((C, Hs, Ws)).astype(np.float32)


# ---- hand-worked scenes: both cameras (64, 64, 4, 6), a 9 x 12 source, Z = 1 (and a 3 x 3 square at Z = 0.5) -----------------
HAND_CAM = camera.Pinhole(64, 64, 4, 6)
HAND_POSE = camera.pose(None, (3 / 64, 0, 0))


def shift_scene():
    return np.ones((9, 12), np.float32)


def occlusion_scene():
    d = np.ones((9, 12), np.float32)
    d[3:6, 2:5] = 0.5                       # shifted by 64 * (3/64) / 0.5 = 6 columns: lands on columns 8..10
    return d


def expected_shift():
    """Target column c holds source column c - 3; columns 0..2 are empty."""
    depth = np.zeros((9, 12), np.float32)
    index = np.full((9, 12), -1, np.int32)
    depth[:, 3:] = 1.0
    index[:, 3:] = np.arange(9)[:, None] * 12 + np.arange(0, 9)[None, :]
    return depth, index


def expected_occlusion():
    """The background shifts 3 columns, the square 6: it covers target rows 3..5, columns 8..10, where background samples land too."""
    d = occlusion_scene()
    depth = np.zeros((9, 12), np.float32)
    index = np.full((9, 12), -1, np.int32)
    for r in range(9):
        for c in range(12):                                             # background first, then the nearer square on top
            if d[r, c] == 1.0 and c + 3 < 12:
                depth[r, c + 3], index[r, c + 3] = 1.0, r * 12 + c
    for r in range(3, 6):
        for c in range(2, 5):
            depth[r, c + 6], index[r, c + 6] = 0.5, r * 12 + c
    return depth, index


TIE_SRC = camera.Pinhole(64, 64, 4, 6)
TIE_DST = camera.Pinhole(32, 32, 2, 3)
TIE_SIZE = (5, 7)


def expected_tie():
    """A constant plane (9 x 12, Z = 1) onto a half-size target with halved focal lengths: u = x / 2, fu = floor(x / 2 + 0.5).
    Each target pixel keeps the lowest source index of those that land on it."""
    index = np.full(TIE_SIZE, -1, np.int64)
    for r in range(9):
        for c in range(12):
            tr, tc = int(np.floor(r / 2 + 0.5)), int(np.floor(c / 2 + 0.5))
            if tr < TIE_SIZE[0] and tc < TIE_SIZE[1] and index[tr, tc] < 0:
                index[tr, tc] = r * 12 + c
    return index.astype(np.int32)


def lattice_case(k, C=5):
    """Everything the tests of lattice k share, computed once: the depth, a C-channel feat, the float32 statement, the float64
    evaluation, and the target pixels the float64 comparison leaves out.  A sample is ambiguous when its float64 u + 0.5 or
    v + 0.5 lies within 1e-3 of an integer - float32 may round it to the neighbouring pixel; every pixel such a sample could reach
    (both roundings, per axis) is left out.  left_out: the ambiguous samples among those in frame."""
    if k not in _CASES:
        scale, win, (Hs, Ws) = LATTICES[k]
        d, pose = lattice_depth(k), reference_pose()
        feat = feat_for(Hs, Ws, C)
        p32 = camera.project_f32(d, SRC, DST, pose, scale, win[:2])
        p64 = camera.project(d, SRC, DST, pose, scale, win[:2], np.float64)
        r32, r64 = camera.splat(p32, SIZE, NEAR, feat), camera.splat(p64, SIZE, NEAR, feat)
        with np.errstate(invalid="ignore"):
            amb = ((np.abs(p64["u"] + 0.5 - np.round(p64["u"] + 0.5)) < 1e-3) | (np.abs(p64["v"] + 0.5 - np.round(p64["v"] + 0.5)) < 1e-3))
            amb &= p64["z_ok"] & (p64["xyz"][2] > np.float64(np.float32(NEAR)))
        skip = np.zeros(SIZE, bool)
        for du in (-1e-3, 1e-3):
            for dv in (-1e-3, 1e-3):
                tu, tv = np.floor(p64["u"][amb] + 0.5 + du).astype(np.int64), np.floor(p64["v"][amb] + 0.5 + dv).astype(np.int64)
                ok = (tu >= 0) & (tu < SIZE[1]) & (tv >= 0) & (tv < SIZE[0])
                skip[tv[ok], tu[ok]] = True
        _CASES[k] = dict(scale=scale, origin=win[:2], depth=d, pose=pose, feat=feat, p32=p32, p64=p64, r32=r32, r64=r64, skip=skip,
                         left_out=int((amb & r64["taking_part"]).sum()), in_frame=int(r64["taking_part"].sum()))
    return _CASES[k]


_CASES = {}
F64_LEFT_OUT = {1: 8, 3: 5, 2: 25}          # what the float64 statement alone leaves out: 0.6 %, 0.4 %, 0.5 % of the samples in frame


def check_against_f64(k, depth, index, valid, feat):
    """depth / index / valid [Ho,Wo], feat [C,Ho,Wo] (numpy) against the float64 evaluation of lattice k on the target pixels that
    are not left out: the same pixels filled by the same samples, their depth the float64 Zd to 2e-7 relative (the float32
    statement's own distance from float64, test_reproject_cpu.py), feat gathered from that sample."""
    c = lattice_case(k)
    assert c["left_out"] == F64_LEFT_OUT[k] and c["left_out"] <= 0.02 * c["in_frame"]
    keep, r64 = ~c["skip"], c["r64"]
    assert keep.sum() >= 0.9 * keep.size
    assert np.array_equal(valid[keep], r64["valid"][keep])
    assert np.array_equal(index[keep], r64["index"][keep])
    hit = keep & r64["valid"]
    z64 = c["p64"]["xyz"][2].ravel()[r64["index"][hit]]
    rel = np.abs(depth[hit].astype(np.float64) - z64) / z64
    print(f"k = {k}: depth against float64 on {int(hit.sum())} pixels ({int(c['skip'].sum())} left out), relmax {rel.max():.3e}")
    assert rel.max() <= 2e-7
    assert (depth[keep & ~r64["valid"]] == 0).all()
    assert np.array_equal(feat[:, keep], r64["feat"][:, keep])
