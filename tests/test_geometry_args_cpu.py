"""CPU tests of the argument statements the geometry entries share (be_hip/native.py: _target_size, _near, _depth_map, _map_like,
_channels, _view, view_list, _fill_args; be_hip/camera.py: check_size, check_number; be_hip/pipeline.py: pack_channels,
unpack_channels, _view_pairs, DepthPipeline._views).  Each helper against a table of good and bad values: every refusal is a
ValueError that names the caller and the argument.  No GPU needed: the tensor checks take CPU tensors, only _depth_map asks where
they live."""
import numpy as np
import pytest
import torch

from be_hip import camera, native, pipeline, raster

WHO = "some_entry"


def refused(name, fn, *args, **kw):
    with pytest.raises(ValueError) as e:
        fn(*args, **kw)
    assert str(e.value).startswith(f"{WHO}: ") and name in str(e.value), str(e.value)
    return str(e.value)


# ---- target size ------------------------------------------------------------------------------------------------------------------
BAD_SIZES = ((0, 5), (3,), (True, 4), (2.5, 4), "ab", None, 7, (1, 2, 3), (4, -1), ("3", "x"))


def test_target_size():
    for bad in BAD_SIZES:
        assert "(Ho, Wo)" in refused("size", native._target_size, WHO, bad)
    for good, want in (((3, 4), (3, 4)), ([1, 1], (1, 1)), ((np.int64(5), 6.0), (5, 6)), ((1 << 24, 127), (1 << 24, 127))):
        got = native._target_size(WHO, good)
        assert got == want and all(type(v) is int for v in got)
    # the two bounds, each at and just over: a side of 2^24, a product of 2^31 - 1
    assert native.TARGET_MAX_SIDE == 1 << 24 and native.TARGET_MAX_PIXELS == 2 ** 31 - 1
    assert native._target_size(WHO, (1, 1 << 24)) == (1, 1 << 24)
    refused("size", native._target_size, WHO, (1, (1 << 24) + 1))
    # 2^31 - 1 is prime, so no two sides multiply to the bound itself: test_check_size_.. meets a product bound exactly
    assert native._target_size(WHO, (65536, 32767)) == (65536, 32767)                             # 2^31 - 65536: the last row that fits
    refused("size", native._target_size, WHO, (65536, 32768))                                     # 2^31: just over
    assert native._target_size(WHO, (46340, 46341)) == (46340, 46341)                             # 2147441940
    refused("size", native._target_size, WHO, (46341, 46342))                                     # 2147534622


def test_check_size_takes_the_bound_and_the_wording():
    assert camera.check_size(WHO, (7, 1), 7, "size must be small") == (7, 1)
    assert "size must be small, got (8, 1)" in refused("size", camera.check_size, WHO, (8, 1), 7, "size must be small")
    assert camera.check_size(WHO, (3, 4), 7, "size ..", max_pixels=12) == (3, 4)                   # a product at the bound
    refused("size", camera.check_size, WHO, (3, 5), 7, "size ..", max_pixels=14)                   # and just over it


def test_the_rasteriser_states_its_own_size_bound():
    ok = lambda size: raster.check_params(WHO, size, 1e-3, "none", ())[:2]
    assert ok((raster.MAX_SIZE, 1)) == (raster.MAX_SIZE, 1) and raster.MAX_SIZE == 16384 < native.TARGET_MAX_SIDE
    assert str(raster.MAX_SIZE) in refused("size", ok, (raster.MAX_SIZE + 1, 1))
    for bad in BAD_SIZES:
        refused("size", ok, bad)


# ---- a finite number in a range -----------------------------------------------------------------------------------------------------
def test_finite_number():
    for bad in (float("nan"), float("inf"), -float("inf"), -1, "x", None, [1, 2], -1e-30):
        assert "near must be a finite number >= 0" in refused("near", native._near, WHO, bad)
        refused("sigma_z", camera.check_number, WHO, "sigma_z", bad, lo_open=True)
        refused("leak", camera.check_number, WHO, "leak", bad, lo_open=True, hi=1, hi_closed=True)
    for good in (0, 0.0, 1e-3, 5, np.float32(0.25), "2.5", True):
        got = native._near(WHO, good)
        assert type(got) is float and got == float(good)
    # open and closed ends
    assert "> 0" in refused("sigma_z", camera.check_number, WHO, "sigma_z", 0, lo_open=True)
    assert camera.check_number(WHO, "sigma_z", 1e-30, lo_open=True) == 1e-30
    assert camera.check_number(WHO, "leak", 1, lo_open=True, hi=1, hi_closed=True) == 1.0
    assert "<= 1" in refused("leak", camera.check_number, WHO, "leak", 1.0000001, lo_open=True, hi=1, hi_closed=True)
    assert "< 1" in refused("x", camera.check_number, WHO, "x", 1, hi=1)
    assert camera.check_number(WHO, "x", 0.5, hi=1) == 0.5


# ---- the tensors ------------------------------------------------------------------------------------------------------------------
DEPTH = torch.arange(20, dtype=torch.float32).reshape(4, 5)


def test_depth_map():
    for bad in (DEPTH.double(), DEPTH[0], torch.zeros(0, 3), torch.zeros(1, 4, 5), DEPTH.numpy(), None, 3.0):
        assert "float32" in refused("depth", native._depth_map, WHO, bad, "fill.fill_nearest_f32", on_gpu=False)
    assert native._depth_map(WHO, DEPTH, "camera.splat_f32", on_gpu=False) is DEPTH
    msg = refused("depth", native._depth_map, WHO, DEPTH, "camera.splat_f32")
    assert "not on the GPU" in msg and "camera.splat_f32 is the host statement" in msg
    assert "[H,W]" in refused("depth", native._depth_map, WHO, None, "x", "[H,W]")


def test_map_like():
    for bad in (DEPTH.double(), DEPTH > 3, DEPTH.to(torch.int32), DEPTH[:3], DEPTH.reshape(5, 4), DEPTH.reshape(1, 4, 5), DEPTH.numpy(),
                3.0, "w"):
        assert "[4,5]" in refused("weight", native._map_like, WHO, "weight", bad, DEPTH)
    for bad in (DEPTH.double(), DEPTH.to(torch.uint8), DEPTH[:, :4], DEPTH.numpy()):
        assert "mask" in refused("weight", native._map_like, WHO, "weight", bad, DEPTH, (torch.float32, torch.bool), "a float32 (or bool: a mask)")
    assert native._map_like(WHO, "edge", None, DEPTH) is None
    got = native._map_like(WHO, "edge", DEPTH, DEPTH)
    assert got.dtype == torch.float32 and got.is_contiguous() and got.data_ptr() == DEPTH.data_ptr()
    strided = torch.arange(40, dtype=torch.float32).reshape(4, 10)[:, ::2]
    got = native._map_like(WHO, "weight", strided, DEPTH)
    assert got.is_contiguous() and torch.equal(got, strided)
    got = native._map_like(WHO, "weight", DEPTH > 3, DEPTH, (torch.float32, torch.bool), "a float32 (or bool: a mask)")
    assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, (DEPTH > 3).float())
    assert "is on meta" in refused("weight", native._map_like, WHO, "weight", DEPTH.to("meta"), DEPTH)


def test_channels():
    f3 = torch.arange(60, dtype=torch.float32).reshape(3, 4, 5)
    for bad in (f3.double(), f3[:, :3], f3.reshape(3, 5, 4), f3.reshape(60), f3.reshape(1, 3, 4, 5), f3.reshape(3, 2, 10), DEPTH.reshape(20),
                f3.numpy(), "f"):
        assert "[C,4,5] or [C,20]" in refused("feat", native._channels, WHO, "feat", bad, DEPTH)
    assert native._channels(WHO, "feat", None, DEPTH) is None
    for good in (f3, f3.reshape(3, 20), f3.permute(0, 2, 1).contiguous().permute(0, 2, 1), torch.zeros(0, 4, 5), f3[:1]):
        got = native._channels(WHO, "feat", good, DEPTH)
        assert got.shape == (good.shape[0], 20) and got.is_contiguous() and got.dtype == torch.float32
        assert torch.equal(got, good.reshape(good.shape[0], 20))
    # a fixed channel count, and a map that may not be absent (icp_linearize's normal_d)
    assert native._channels(WHO, "normal_d", f3, DEPTH, C=3, required=True).shape == (3, 20)
    for bad in (None, f3[:2], torch.zeros(4, 20)):
        assert "[3,4,5] or [3,20]" in refused("normal_d", native._channels, WHO, "normal_d", bad, DEPTH, C=3, required=True)
    assert "is on meta" in refused("feat", native._channels, WHO, "feat", f3.to("meta"), DEPTH)


def test_fill_args_before_the_gpu_is_asked_for():
    for who, fn, statement in (("fill_nearest", native.fill_nearest, "fill.fill_nearest_f32"), ("fill_diffuse", native.fill_diffuse, "diffuse.fill_diffuse")):
        with pytest.raises(ValueError, match=f"{who}: depth is not on the GPU.*{statement}"):
            fn(DEPTH)
        with pytest.raises(ValueError, match=f"{who}: depth must be a float32 tensor .H,W."):
            fn(DEPTH.double())


# ---- view dicts and views lists -----------------------------------------------------------------------------------------------------
CAM = (100.0, 100.0, 1.5, 2.0)


@pytest.mark.parametrize("keys, cam_key", [(native.FUSE_VIEW_KEYS, "cam_src"), (native.ICP_VIEW_KEYS, "cam")])
def test_view_dict(keys, cam_key):
    view = lambda v: native._view(WHO, v, keys, cam_key)
    for bad in (None, 5, [DEPTH, CAM], (("depth", DEPTH),), {"depth": DEPTH}, {cam_key: CAM}, {}):
        msg = refused("depth", view, bad)                                # a non-dict, and a dict without depth or the camera
        assert cam_key in msg and str(keys) in msg
    assert "unknown keys ['colour']" in refused("colour", view, {"depth": DEPTH, cam_key: CAM, "colour": 1})
    other = "cam" if cam_key == "cam_src" else "cam_src"                 # the other family's camera key is unknown here
    assert "unknown keys" in refused(other, view, {"depth": DEPTH, cam_key: CAM, other: CAM})
    msg = refused("depth", view, {"depth": DEPTH, cam_key: CAM})         # a CPU depth: refused before anything is computed
    assert "not on the GPU; nothing here computes on the CPU" in msg
    assert "float32" in refused("depth", view, {"depth": DEPTH.double(), cam_key: CAM})


def test_entries_name_themselves_in_a_view_refusal():
    with pytest.raises(ValueError, match=r"fuse_views\(views\[0\]\): depth is not on the GPU"):
        native.fuse_views([dict(depth=DEPTH, cam_src=CAM)], CAM, (4, 5))
    with pytest.raises(ValueError, match=r"icp_linearize\(src\): depth is not on the GPU"):
        native.icp_linearize(dict(depth=DEPTH, cam=CAM), dict(depth=DEPTH, cam=CAM), torch.zeros(3, 4, 5), None)
    with pytest.raises(ValueError, match=r"register_depth\(src\): unknown keys \['pose'\]"):
        native.register_depth(dict(depth=DEPTH, cam=CAM, pose=None), dict(depth=DEPTH, cam=CAM))


def test_views_list():
    assert native.view_list(WHO, (v for v in (1, 2)), "things") == [1, 2]
    for bad in (5, None, 2.5):
        assert "a list of (maps, pose)" in refused("views", native.view_list, WHO, bad, "(maps, pose)")
        refused("views", pipeline._view_pairs, WHO, bad)
    assert "at least one" in refused("views", pipeline._view_pairs, WHO, [])
    assert pipeline._view_pairs(WHO, ((1, 2),)) == [(1, 2)]
    with pytest.raises(ValueError, match="fuse_views: views must be a list of dicts"):
        native.fuse_views(5, CAM, (4, 5))


def test_view_builder():
    pipe = pipeline.DepthPipeline.__new__(pipeline.DepthPipeline)       # the refusals below come before any member is read
    pipe.densify = None
    for entry, kw in ((pipe.fuse, {}), (pipe.integrate, dict(dims=(4, 4, 4), origin=(0, 0, 1), voxel=(1, 1, 1)))):
        who = entry.__name__
        with pytest.raises(ValueError, match=f"{who}: views must be a list of .maps, pose."):
            entry(5, **kw)
        with pytest.raises(ValueError, match=f"{who}: views must hold at least one"):
            entry([], **kw)
        for bad in (5, (1, 2, 3), "abc", None):
            with pytest.raises(ValueError, match=rf"{who}: views\[0\] must be .maps, pose."):
                entry([bad], **kw)
            with pytest.raises(ValueError, match=rf"{who}: views\[1\] must be .maps, pose."):
                _second_is_bad(pipe, who, bad)
        with pytest.raises(ValueError, match=rf"{who}\(views\[0\]\): maps lacks \['records', 'grid'\]"):
            entry([({}, None)], **kw)
        cpu = dict(records=torch.zeros(4, 32), grid=dict(H=21, W=21), depth_map=torch.zeros(21, 21))
        with pytest.raises(ValueError, match=rf"{who}\(views\[0\]\): maps\['records'\] is not on the GPU"):
            entry([(cpu, None)], **kw)


def _second_is_bad(pipe, who, bad):
    """_views over [a good pair whose samples a stub supplies, bad]: the refusal names index 1."""
    z = torch.ones(4, 5)
    src = dict(depth_map=z, conf=torch.ones(4, 5), shpd=torch.zeros(3, 4, 5))
    pipe._depth_samples = lambda who_, maps, scale, window, want, thres: (src, dict(scale=1, window=(0, 0, 4, 5)))
    pipe.dcal = type("Cal", (), dict(intrinsics=staticmethod(lambda H, W: CAM)))()
    try:
        pipe._views(who, [(dict(grid=dict(H=4, W=5)), None), bad], ("shpd",))
    finally:
        del pipe._depth_samples


def test_view_builder_builds_the_native_views():
    pipe = pipeline.DepthPipeline.__new__(pipeline.DepthPipeline)
    z = torch.arange(20, dtype=torch.float32).reshape(4, 5)
    src = dict(depth_map=z, conf=torch.full((1, 4, 5), 0.5, dtype=torch.float64), shpd=torch.arange(60, dtype=torch.float32).reshape(3, 4, 5))
    pipe._depth_samples = lambda who, maps, scale, window, want, thres: (src, dict(scale=scale, window=(0, 0, 4, 5)))
    pipe.dcal = type("Cal", (), dict(intrinsics=staticmethod(lambda H, W: (H, W))))()
    pose = np.arange(12.0)
    vs, layout = pipe._views("fuse", [(dict(grid=dict(H=4, W=5)), None), (dict(grid=dict(H=8, W=9)), pose)], ("shpd",), scale=2)
    assert layout == dict(want=("shpd",), channels=[("shpd", (3,), 3)], camera=(4, 5), size=(4, 5))       # the first view's
    assert [set(v) for v in vs] == [set(native.FUSE_VIEW_KEYS)] * 2
    assert vs[0]["pose"] is None and vs[1]["pose"] is pose and vs[1]["cam_src"] == (8, 9)
    for v in vs:
        assert v["depth"] is z and v["scale"] == 2 and v["window_origin"] == (0, 0)
        assert v["weight"].dtype == torch.float32 and v["weight"].shape == (4, 5) and bool((v["weight"] == 0.5).all())
        assert torch.equal(v["feat"], src["shpd"].reshape(3, 20))


# ---- the channel layout -------------------------------------------------------------------------------------------------------------
def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(7)
    src = dict(a=torch.randn(4, 5, generator=g), b=torch.randn(3, 4, 5, generator=g), c=torch.randn(2, 3, 4, 5, generator=g),
               unused=torch.randn(4, 5, generator=g))
    want = ("a", "b", "c")
    feat, channels = pipeline.pack_channels(src, want, 20)
    literal = torch.cat([src["a"].reshape(1, 20), src["b"].reshape(3, 20), src["c"].reshape(6, 20)])
    assert feat.shape == (10, 20) and torch.equal(feat, literal)
    assert channels == [("a", (), 1), ("b", (3,), 3), ("c", (2, 3), 6)]
    # what an entry returns for those channels over a 3 x 7 target, split by hand
    out = torch.randn(10, 21, generator=g)
    got = pipeline.unpack_channels(out.reshape(10, 3, 7), channels, (3, 7))
    assert list(got) == list(want)
    assert got["a"].shape == (3, 7) and torch.equal(got["a"], out[0].reshape(3, 7))
    assert got["b"].shape == (3, 3, 7) and torch.equal(got["b"], out[1:4].reshape(3, 3, 7))
    assert got["c"].shape == (2, 3, 3, 7) and torch.equal(got["c"], out[4:10].reshape(2, 3, 3, 7))
    # the inputs themselves come back when the tail is the lattice they were packed from
    back = pipeline.unpack_channels(feat, channels, (4, 5))
    assert all(torch.equal(back[k], src[k]) for k in want)
    # another order of want is another order of channels
    feat2, channels2 = pipeline.pack_channels(src, ("c", "a"), 20)
    assert torch.equal(feat2, torch.cat([src["c"].reshape(6, 20), src["a"].reshape(1, 20)])) and [c[0] for c in channels2] == ["c", "a"]
    # nothing wanted
    assert pipeline.pack_channels(src, (), 20) == (None, [])
    assert pipeline.unpack_channels(None, [], (3, 7)) == {} and pipeline.unpack_channels(None, (), (3, 7)) == {}
    # per-vertex maps (a mesh): one tail axis; and the layout a volume keeps in meta["channels"] (lists after a round trip through json)
    mesh = dict(shpd=torch.randn(3, 11, generator=g), conf=torch.randn(11, generator=g))
    featv, chv = pipeline.pack_channels(mesh, ("shpd", "conf"), 11, tail=1)
    assert torch.equal(featv, torch.cat([mesh["shpd"], mesh["conf"].reshape(1, 11)])) and chv == [("shpd", (3,), 3), ("conf", (), 1)]
    old_meta = [["shpd", [3], 3], ["conf", [], 1]]
    got = pipeline.unpack_channels(featv, old_meta, (11,))
    assert torch.equal(got["shpd"], mesh["shpd"]) and torch.equal(got["conf"], mesh["conf"])
