"""CPU tests of the rasteriser's statement, be_hip/raster.py (no GPU): triangles placed by hand on the pixel lattice at the smallest
shapes, ties and facing, the closed ellipsoid of mesh_scenes.py seen from outside, the plane, float32 against float64 and against
volume.raycast on the fusion scene, the interpolation, empty meshes, every refused input, the settings file and the plumbing of the
new entry.  test_raster_gpu.py holds the kernels to this statement bit for bit.  The scenes are those of tests/raster_scenes.py."""
import os
import re

import numpy as np
import pytest
import torch

from be_hip import camera, raster, volume
import fuse_scenes as fs
import mesh_scenes as ms
import raster_scenes as rc
from conftest import ROOT

_F = np.float32
ULP = float(np.spacing(_F(1)))                                           # 2^-23


def _pixels(valid):
    return {(int(y), int(x)) for y, x in zip(*np.nonzero(valid))}


# ------------------------------------------------------------------------------------------ 1. hand-worked cases
def test_one_pixel_under_one_triangle():
    out = rc.reference("one pixel")
    assert out["depth"].shape == (1, 1) and out["valid"][0, 0] and out["face"][0, 0] == 0 and out["depth"][0, 0] == _F(1)
    # the centre (0, 0) of the triangle (-1, -1), (2, -1), (-1, 2) is its centroid: E_i = A / 3 exactly
    third = _F(1) / _F(3)
    assert (out["bary"][:, 0, 0] == third * _F(1) * _F(1)).all()
    m = rc.get("one pixel")["mesh"]
    want = (third * m["weight"][0] + third * m["weight"][1]) + third * m["weight"][2]
    assert out["weight"][0, 0] == want and out["feat"].shape == (2, 1, 1) and out["normal"].shape == (3, 1, 1) and out["normal_valid"][0, 0]
    assert abs(float(np.sqrt((out["normal"].astype(np.float64) ** 2).sum())) - 1) < 4 * ULP


def test_a_vertex_on_a_pixel_centre_and_the_top_left_rule():
    # (2, 2), (5, 2), (2, 5): the top edge y = 2 and the left edge x = 2 belong to it, the hypotenuse x + y = 7 does not
    out = rc.reference("vertex on a centre")
    assert _pixels(out["valid"]) == {(2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (4, 2)}
    assert (out["bary"][:, 2, 2] == (1, 0, 0)).all()                     # at vertex 0
    assert (out["depth"][out["valid"]] == _F(1)).all() and (out["face"][~out["valid"]] == -1).all()
    assert (out["depth"][~out["valid"]].view(np.uint32) == 0).all()


@pytest.mark.parametrize("kind", ["horizontal", "vertical", "diagonal"])
def test_a_shared_edge_covers_each_centre_once(kind):
    want = rc.SQUARE_PIXELS if kind == "diagonal" else rc.DIAMOND_PIXELS
    for name in (f"pair {kind}", f"pair {kind} reversed"):
        counts = rc.fragment_counts(name)
        assert _pixels(counts == 1) == want and int(counts.sum()) == len(want), name
        assert _pixels(rc.reference(name)["valid"]) == want
    # the reversed pair is the same picture seen from the other side: the same pixels, faces and depths
    a, b = rc.reference(f"pair {kind}"), rc.reference(f"pair {kind} reversed")
    assert np.array_equal(a["face"], b["face"]) and np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["bary"][0], b["bary"][0])
    assert np.array_equal(a["bary"][1], b["bary"][2]) and np.array_equal(a["feat"].view(np.uint32), b["feat"].view(np.uint32))


def test_triangles_that_give_no_fragment():
    for name in ("no centre", "zero area", "no faces", "empty"):
        out = rc.reference(name)
        assert not out["valid"].any() and (out["face"] == -1).all() and (out["depth"].view(np.uint32) == 0).all(), name
        assert int(rc.fragment_counts(name).sum()) == 0
        assert (out["bary"].view(np.uint32) == 0).all() and out["feat"].shape == (2, 9, 9) and not out["normal_valid"].any()
    bare = rc.reference("bare")
    assert bare["valid"].all() and all(bare[k] is None for k in ("weight", "feat", "normal", "normal_valid")) and bare["bary"] is not None


def test_a_triangle_with_an_unusable_vertex_is_dropped_whole():
    c = rc.get("dropped")
    vs = raster.vertex_stage(c["mesh"]["vertices"], c["cam"], c["pose"])
    assert vs["usable"].tolist() == [True, True, True, False, False, False, False, False, True]
    out = rc.reference("dropped")
    assert set(np.unique(out["face"])) == {-1, 4}
    alone = raster.render(dict(c["mesh"], faces=c["mesh"]["faces"][4:5]), c["cam"], c["pose"], c["size"])
    assert np.array_equal(alone["valid"], out["valid"]) and np.array_equal(alone["feat"].view(np.uint32), out["feat"].view(np.uint32))
    assert _pixels(out["valid"]) == {(y, x) for y in range(1, 7) for x in range(1, 7) if x + y < 8}
    # near is a parameter: behind near = 2 nothing is left
    assert not raster.render(c["mesh"], c["cam"], c["pose"], c["size"], near=2.0)["valid"].any()


def test_a_triangle_far_larger_than_the_frame_and_large_edge_functions():
    out = rc.reference("larger than the frame")
    assert out["valid"].all() and (out["face"] == 0).all()
    assert np.abs(out["depth"].astype(np.float64) - 1).max() <= 4 * ULP  # the three rounded w_i need not sum to 1 exactly
    c = rc.get("large edge functions")
    vs = raster.vertex_stage(c["mesh"]["vertices"], c["cam"], c["pose"])
    x, y = vs["xs"], vs["ys"]
    A = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    assert abs(int(A)) > 1 << 36                                         # int64 -> float32 rounds: 2^24 is far below
    a, b = rc.reference("large edge functions"), rc.reference("large edge functions", np.float64)
    assert a["valid"].all() and np.array_equal(a["valid"], b["valid"])
    err = np.abs(a["depth"].astype(np.float64) - b["depth"]) / b["depth"]
    print(f"large edge functions: depth float32 against float64, relative {err.max():.2e}")
    assert err.max() < 16 * ULP                                          # a dozen roundings of 2^-24 each, relative


# ------------------------------------------------------------------------------------------ 2. ties and facing
def test_coincident_faces_the_lower_index_wins():
    out = rc.reference("coincident")
    assert _pixels(out["valid"]) == rc.SQUARE_PIXELS and set(np.unique(out["face"][out["valid"]])) == {0, 2}
    assert int(rc.fragment_counts("coincident").max()) == 2


def test_interpenetrating_triangles_per_pixel_nearest():
    c = rc.get("interpenetrating")
    out = rc.reference("interpenetrating")
    halves = [raster.render(dict(c["mesh"], faces=c["mesh"]["faces"][s]), c["cam"], c["pose"], c["size"]) for s in (slice(0, 2), slice(2, 4))]
    assert out["valid"].all() and all(h["valid"].all() for h in halves)
    assert np.array_equal(out["depth"], np.minimum(halves[0]["depth"], halves[1]["depth"]))
    rising = halves[0]["depth"] < halves[1]["depth"]
    assert rising.any() and (~rising).any() and np.array_equal(out["face"] < 2, rising | (halves[0]["depth"] == halves[1]["depth"]))


def test_cull_modes():
    none, back, front = (rc.reference(f"cull {k}") for k in raster.CULL)
    assert _pixels(none["valid"]) == rc.SQUARE_PIXELS
    assert set(np.unique(back["face"])) == {-1, 1} and set(np.unique(front["face"])) == {-1, 0}
    assert not (back["valid"] & front["valid"]).any() and np.array_equal(back["valid"] | front["valid"], none["valid"])


# ------------------------------------------------------------------------------------------ 3. a closed surface, a plane
def test_the_ellipsoid_seen_from_outside():
    counts, culled = rc.fragment_counts("ellipsoid none"), rc.fragment_counts("ellipsoid back")
    covered = counts > 0
    print(f"ellipsoid: {int(covered.sum())} covered pixels, fragments {np.unique(counts[covered]).tolist()}, culled {np.unique(culled[covered]).tolist()}")
    assert covered.sum() > 40 and (counts[covered] == 2).all() and (culled[covered] == 1).all() and not culled[~covered].any()
    a, b = rc.reference("ellipsoid none"), rc.reference("ellipsoid back")
    assert rc.same(a, b)                                                 # the front layer is the nearer one: culling changes nothing
    assert np.array_equal(a["valid"], covered) and a["normal_valid"][covered].all()
    # the gradient normals point out of the ellipsoid: towards the camera
    assert (a["normal"][2][covered] < 0).all()


def test_the_plane_through_the_fusion_camera():
    out = rc.reference("plane")
    err = np.abs(out["depth"][out["valid"]].astype(np.float64) - ms.PLANE_Z)
    print(f"plane: {int(out['valid'].sum())} pixels, depth error {err.max():.2e} m")
    assert out["valid"].sum() > 1500 and err.max() < 1e-5                # the bound test_mesh_cpu.py holds the plane to


# ------------------------------------------------------------------------------------------ 4. float64 and the ray cast
# the median of |mesh - ray cast| this file measured on the CPU (V: metres); the test holds twice that
RAYCAST_MEDIAN = {1: 7.1e-4, 8: 5.1e-4}


@pytest.mark.parametrize("V", [1, 8])
def test_float32_against_float64_and_against_the_ray_cast(V):
    """float32 statement on the float32 mesh against the float64 evaluation on the float64 mesh.  Measured here: 0 of 1961 pixels
    differ in face or valid on both scenes; depth on agreeing pixels differs by 3.0e-5 m (1 view) and 1.7e-5 m (8 views).  That
    gap is not float32 noise: a vertex's snapped coordinate differs by one unit of 1/256 pixel between the two evaluations, which
    on the faces that span the 0.3 m depth step moves depth by 0.3 m / (pixels across the face) / 256.
    Against volume.raycast of the same volume, where both are valid: median 0.71 mm and maximum 9.2 mm (1 view), 0.50 mm and 8.2 mm
    (8 views); the maximum is at the step.  The two methods interpolate differently - linearly on a triangle, trilinearly along a
    ray - so this belongs to neither; only the median is held, to twice the value measured."""
    fld = ms.scene_field(ms.BIG, V)
    m64 = ms.reference(("scene", ms.BIG, V, 2), fld, dtype=np.float64)
    a = rc.reference(f"scene {ms.BIG} {V}")
    b = raster.render(m64, fs.CAM, None, fs.SIZE, dtype=np.float64)
    differ = (a["face"] != b["face"]) | (a["valid"] != b["valid"])
    agree = ~differ & a["valid"]
    gap = np.abs(a["depth"].astype(np.float64) - b["depth"])[agree].max()
    print(f"{V} views: {int(differ.sum())} of {differ.size} pixels differ, depth gap {gap:.2e} m on {int(agree.sum())}")
    assert differ.mean() <= 0.01 and agree.sum() > 250
    assert gap < 1e-4                                                    # the project's float64 bound for maps
    cast = volume.raycast(ms.scene_volume(ms.BIG, V), fs.CAM, None, fs.SIZE, (0.62, 1.2))
    both = cast["valid"] & a["valid"]
    d = np.abs(cast["depth"].astype(np.float64) - a["depth"])[both]
    print(f"{V} views: against the ray cast on {int(both.sum())} pixels, median {np.median(d):.2e} m, maximum {d.max():.2e} m")
    assert both.sum() > 250 and np.median(d) <= 2 * RAYCAST_MEDIAN[V]


# ------------------------------------------------------------------------------------------ 5. the interpolation
@pytest.mark.parametrize("name", ["ellipsoid none", f"scene {ms.BIG} 8", "large edge functions", "interpenetrating"])
def test_bary_sums_to_one_and_camera_z_interpolates_back_to_depth(name):
    c = rc.get(name)
    out = rc.reference(name)
    v = out["valid"]
    bary = out["bary"][:, v]
    assert (bary >= 0).all() and (out["bary"][:, ~v].view(np.uint32) == 0).all()
    total = (bary[0] + bary[1]) + bary[2]
    print(f"{name}: |sum of bary - 1| <= {np.abs(total - 1).max():.2e}")
    assert np.abs(total - 1).max() <= 4 * ULP
    Zc = raster.vertex_stage(c["mesh"]["vertices"], c["cam"], c["pose"])["Zc"]
    kw = {k: x for k, x in c["kw"].items() if k != "want"}
    back = raster.render(dict(vertices=c["mesh"]["vertices"], faces=c["mesh"]["faces"], weight=np.where(np.isfinite(Zc), Zc, 0).astype(_F)),
                         c["cam"], c["pose"], c["size"], want=("weight",), **kw)
    rel = np.abs(back["weight"][v].astype(np.float64) / out["depth"][v] - 1)
    print(f"{name}: camera Z interpolated against depth, relative {rel.max():.2e}")
    assert rel.max() <= 4 * ULP


def test_want_subsets_and_planted_nan():
    full = rc.reference("ellipsoid none")
    part = rc.reference("ellipsoid want")
    assert part["weight"] is None and part["feat"] is None and np.array_equal(part["bary"], full["bary"]) and np.array_equal(part["normal"], full["normal"])
    only = rc.reference("ellipsoid depth only")
    assert all(only[k] is None for k in ("weight", "feat", "normal", "normal_valid", "bary")) and np.array_equal(only["depth"], full["depth"])
    bad = rc.reference("ellipsoid nan")
    assert bad["valid"].sum() > 40 and np.isfinite(bad["depth"]).all()   # the planted vertices only drop their triangles
    assert not np.isfinite(bad["normal"]).all() or not bad["normal_valid"][bad["valid"]].all()
    assert (~bad["normal_valid"] | np.isfinite(bad["normal"]).all(0)).all()      # a normal that is valid is finite


# ------------------------------------------------------------------------------------------ 6. refused inputs, settings, plumbing
def test_every_refused_input():
    c = rc.get("one pixel")
    m = c["mesh"]
    ok = dict(mesh=m, cam_dst=c["cam"], pose=None, size=(3, 3))
    raster.render(**ok)
    bad_faces = [np.array([[0, 1, 3]], np.int32), np.array([[0, -1, 2]], np.int32)]
    for kw in ([dict(mesh=dict(m, faces=f)) for f in bad_faces]
               + [dict(cam_dst=(np.nan, 1, 0, 0)), dict(cam_dst=(1, np.inf, 0, 0)), dict(cam_dst=(1, 1, 0)), dict(pose=np.full(12, np.nan))]
               + [dict(size=s) for s in ((0, 3), (3, 16385), (3,), (2.5, 3), (True, 3), None)]
               + [dict(near=n) for n in (-1.0, float("nan"), float("inf"), "x")]
               + [dict(cull=k) for k in ("both", None, 1)] + [dict(want=("depth",)), dict(want=("feat", "colour"))]
               + [dict(mesh=dict(m, feat=m["feat"][:, :2])), dict(mesh=dict(m, weight=m["weight"][:2])), dict(mesh=dict(m, normal=m["normal"][:2])),
                  dict(mesh=dict(m, vertices=m["vertices"][:, :2])), dict(mesh=dict(m, faces=m["faces"][:, :2])), dict(mesh=[1, 2]),
                  dict(mesh=dict(faces=m["faces"]))]):
        with pytest.raises(ValueError):
            raster.render(**dict(ok, **kw))
    raster.render(m, c["cam"], None, (16384, 1), want=())               # the largest size


def test_the_fusion_settings_file_takes_mesh_render(tmp_path):
    from be_hip import workflow as wf
    poses = np.stack([camera.pose(), camera.pose(None, (0.0005, 0, 0))])
    vol = dict(tsdf_dims=(8, 4, 6), tsdf_origin=(-0.5, 0, 0.25), tsdf_voxel=(0.5, 0.25, 0.125))
    np.savez(tmp_path / "vol.npz", poses=poses, **vol)
    assert "mesh_render" not in wf.load_fusion(str(tmp_path / "vol.npz"))
    np.savez(tmp_path / "render.npz", poses=poses, mesh_render=1, **vol)
    cfg = wf.load_fusion(str(tmp_path / "render.npz"))
    assert cfg["mesh_render"] == 1 and "tsdf_mesh" not in cfg and set(cfg["tsdf"]) == {"dims", "origin", "voxel", "trunc"}
    np.savez(tmp_path / "off.npz", poses=poses, mesh_render=0)
    assert wf.load_fusion(str(tmp_path / "off.npz"))["mesh_render"] == 0
    np.savez(tmp_path / "lone.npz", poses=poses, mesh_render=1)
    with pytest.raises(ValueError, match="tsdf_dims.*tsdf_origin.*tsdf_voxel"):
        wf.load_fusion(str(tmp_path / "lone.npz"))
    for bad in (-1, 1.5):
        np.savez(tmp_path / "bad.npz", poses=poses, mesh_render=bad, **vol)
        with pytest.raises(ValueError):
            wf.load_fusion(str(tmp_path / "bad.npz"))


def test_entry_is_declared_exported_bound_and_checks_its_arguments():
    from be_hip import native
    from be_hip.pipeline import DepthPipeline
    hdr = open(os.path.join(ROOT, "include", "blurry_edges_hip.h")).read()
    declared = set(re.findall(r"\b(be_[a-z0-9_]+)\s*\(", hdr))
    lib = native.lib()
    for name in ("be_mesh_raster_f32", "be_mesh_raster_workspace_bytes"):
        assert name in declared and name in native.EXPORTED and name in native._SIGNATURES and hasattr(lib, name), name
    for name, value in (("BE_RASTER_SUB", raster.SUB), ("BE_RASTER_GUARD", raster.GUARD), ("BE_RASTER_MAX_SIZE", raster.MAX_SIZE)):
        assert re.search(rf"#define {name} {value}\b", hdr), name
    o = native.ops()
    assert o is not None and hasattr(o, "mesh_raster")
    assert "Tensor vertices, Tensor faces, Tensor? weight, Tensor? feat, Tensor? normal, Tensor? normal_valid, Tensor cam_dst" in str(
        torch.ops.be.mesh_raster.default._schema)
    assert callable(native.raster_mesh) and hasattr(DepthPipeline, "render_mesh")
    assert lib.be_mesh_raster_workspace_bytes(10, 3, 5) == 10 * 16 + 3 * 5 * 8 and lib.be_mesh_raster_workspace_bytes(0, 1, 1) == 8
    assert lib.be_mesh_raster_workspace_bytes(-1, 3, 5) == 0 and lib.be_mesh_raster_workspace_bytes(10, 0, 5) == 0
    assert lib.be_mesh_raster_workspace_bytes(10, 3, 16385) == 0
    # host-side argument checks of the library fail before any launch (no GPU needed)
    one = native.C.c_void_p(32)                                          # a non-null, 16-byte aligned address; never read
    cam = (native.C.c_float * 4)(60, 58, 18.2, 25.7)
    pose = (native.C.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)
    order = ("vertices", "V", "faces", "T", "weight", "feat", "C", "normal", "normal_valid", "cam", "pose", "near", "cull", "Ho", "Wo", "depth", "face",
             "weight_out", "feat_out", "normal_out", "normal_valid_out", "bary", "ws", "ws_bytes", "stream")
    base = dict(vertices=one, V=10, faces=one, T=4, weight=one, feat=one, C=2, normal=one, normal_valid=one, cam=cam, pose=pose, near=1e-3, cull=0,
                Ho=3, Wo=5, depth=one, face=one, weight_out=one, feat_out=one, normal_out=one, normal_valid_out=one, bary=one, ws=one,
                ws_bytes=10 * 16 + 3 * 5 * 8, stream=None)
    nan_cam = (native.C.c_float * 4)(60, float("nan"), 18.2, 25.7)
    flat_cam = (native.C.c_float * 4)(0, 58, 18.2, 25.7)
    inf_pose = (native.C.c_float * 12)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, float("inf"))
    for kw, msg in ((dict(V=-1), b"2^31"), (dict(T=1 << 31), b"2^31"), (dict(Ho=0), b"size"), (dict(Wo=16385), b"size"), (dict(cam=None), b"null pointer"),
                    (dict(pose=None), b"null pointer"), (dict(depth=None), b"null pointer"), (dict(face=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                    (dict(vertices=None), b"null vertices"), (dict(faces=None), b"null faces"), (dict(cam=nan_cam), b"cam_dst"), (dict(cam=flat_cam), b"cam_dst"),
                    (dict(pose=inf_pose), b"pose"), (dict(near=-1.0), b"near"), (dict(near=float("nan")), b"near"), (dict(near=float("inf")), b"near"),
                    (dict(cull=3), b"cull"), (dict(cull=-1), b"cull"), (dict(C=-1), b"C must"), (dict(C=65), b"C must"), (dict(feat=None), b"C must"),
                    (dict(weight=None), b"weight_out needs"), (dict(normal=None), b"normal_out"), (dict(normal_valid_out=None), b"normal_out"),
                    (dict(ws=native.C.c_void_p(40)), b"workspace"), (dict(ws_bytes=10 * 16 + 3 * 5 * 8 - 1), b"workspace")):
        args = dict(base, **kw)
        assert lib.be_mesh_raster_f32(*[args[k] for k in order]) != 0, kw
        assert msg in lib.be_last_error(), (kw, lib.be_last_error())
    # native.raster_mesh checks on the host, before the library is touched
    m = {k: torch.from_numpy(v) for k, v in rc.get("one pixel")["mesh"].items()}
    with pytest.raises(ValueError, match="GPU"):
        native.raster_mesh(m, rc.UNIT, None, (3, 3))
    for bad in (dict(m, faces=m["faces"].long()), dict(m, vertices=m["vertices"].double()), dict(m, feat=m["feat"][:, :2]),
                dict(m, normal_valid=m["normal_valid"].to(torch.uint8)), rc.get("one pixel")["mesh"], [1]):
        with pytest.raises(ValueError):
            native.raster_mesh(bad, rc.UNIT, None, (3, 3))
    for kw in (dict(size=(0, 3)), dict(cull="both"), dict(near=-1), dict(want=("depth",))):
        with pytest.raises(ValueError):
            native.raster_mesh(**dict(dict(mesh=m, cam_dst=rc.UNIT, pose=None, size=(3, 3)), **kw))
