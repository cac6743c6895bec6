"""The textured test-set generator's host side (be_hip.datagen_test, no GPU): the render entry's argument checks, the restated
cv2 resize and crop arithmetic, the sources, the depth planes / key points / PSF tables against the reference (golden g19), and
the driver's flags."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from conftest import load_golden

EPS = np.finfo(np.float64).eps


def digest(a):
    """SHA-256 of a float64 array's bytes, as tests/golden/make_golden_textured.py stores full outputs."""
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def _dt():
    from be_hip import datagen_test
    return datagen_test


# ------------------------------------------------------------------------------------------------------ C ABI argument checks
def _render_call(**over):
    from be_hip import native
    p = C.c_void_p(4096)                                 # never dereferenced: every call below must fail before a launch
    a = dict(bkgd=p, frgd=p, mask=p, depth_bg=p, depth_fg=p, keys=p, psf=p, psf_k=p, psf_len=10 ** 9, kmax=17, n=2, H=8, W=8,
             n_interval=4, all_layers=0, img_clean=p, mask_blur=p, stream=None)
    a.update(over)
    rc = native.lib().be_datagen_test_render_f64(*a.values())
    return rc, native.lib().be_last_error().decode()


@pytest.mark.parametrize("over, msg", [
    (dict(n=-1), "n = -1"),
    (dict(n_interval=0), "n_interval = 0"),
    (dict(H=0), "bad image size"),
    (dict(W=0), "bad image size"),
    (dict(kmax=-1), "kmax"),
    (dict(kmax=65), "kmax"),
    (dict(all_layers=2), "all_layers"),
    (dict(psf=None), "null pointer"),
    (dict(mask_blur=None), "null pointer"),
    (dict(psf_len=2 * 4 * 5 * 35 * 35 - 1), "overruns"),
])
def test_render_entry_rejects_bad_arguments_before_any_launch(over, msg):
    rc, err = _render_call(**over)
    assert rc == -1 and msg in err, (rc, err)


def test_render_entry_sizes_its_psf_table_and_accepts_an_empty_batch():
    from be_hip import native
    lib = native.lib()
    assert lib.be_datagen_test_psf_doubles(2, 4, 17) == 2 * 4 * 5 * 35 * 35
    assert lib.be_datagen_test_psf_doubles(-1, 4, 17) == 0 and lib.be_datagen_test_psf_doubles(1, 0, 17) == 0
    rc, _ = _render_call(n=0, psf_len=0)
    assert rc == 0                                       # N = 0 launches nothing (and so succeeds without a GPU)


# ---------------------------------------------------------------------------------------------------- resize + crop arithmetic
def test_resize_upscale_2x2_to_4x4_known_answer():
    # x_src = (x + .5) / 2 - .5 = -.25 (clamped: 0), .25, .75, 1.25 (clamped: 1); weights (2048, 0), (1536, 512), (512, 1536), (2048, 0)
    # row 1, column 1: 1536 * (512 * 255) + 512 * (1536 * 255) = 401080320; + 2^21 >> 22 = 96
    src = np.array([[0, 255], [255, 0]], np.uint8)
    want = np.array([[0, 64, 191, 255], [64, 96, 159, 191], [191, 159, 96, 64], [255, 191, 64, 0]], np.uint8)
    assert np.array_equal(_dt().resize_linear_u8(src, (4, 4)), want)
    rgb = np.stack([src, 255 - src, src // 5], axis=-1)                  # channels are resized independently
    out = _dt().resize_linear_u8(rgb, (4, 4))
    assert out.shape == (4, 4, 3) and np.array_equal(out[..., 0], want) and np.array_equal(out[..., 1], 255 - want)


def test_resize_downscale_known_answers():
    d = _dt()
    # exact 2x: x_src = 2x + .5, weights (1024, 1024) both ways -> (a + b + c + d + 2) >> 2
    assert np.array_equal(d.resize_linear_u8((np.arange(16).reshape(4, 4) * 10).astype(np.uint8), (2, 2)), [[25, 45], [105, 125]])
    # 3 -> 2: x_src = .25, 1.75; weights (1536, 512), (512, 1536); [0 20 40] -> (0*1536 + 20*512)/2048 = 5, (20*512 + 40*1536)/2048 = 35
    src = (np.arange(9).reshape(3, 3) * 20).astype(np.uint8)
    assert np.array_equal(d.resize_linear_u8(src, (2, 2)), [[20, 50], [110, 140]])
    # 5 -> 3: x_src = (x + .5) * 5/3 - .5 = 1/3, 2, 11/3; weights (round(2048 * 2/3), round(2048/3)) = (1365, 683), (2048, 0),
    # (683, 1365): 60 * 683 / 2048 = 20.01 -> 20, 120, (180 * 683 + 240 * 1365) / 2048 = 219.99 -> 220 (one row: weight 2048 on it)
    row = np.array([[0, 60, 120, 180, 240]], np.uint8)
    assert np.array_equal(d.resize_linear_u8(row, (3, 1)), [[20, 120, 220]])
    # a tie: 2 -> 3 gives x_src = -1/6 (clamped), 1/2, 7/6 (clamped); 1/2 weighs (1024, 1024): (10 + 13) * 1024 * 2048 + 2^21 >> 22 = 12
    assert np.array_equal(d.resize_linear_u8(np.array([[10, 13]], np.uint8), (3, 1)), [[10, 12, 13]])
    with pytest.raises(TypeError):
        d.resize_linear_u8(src.astype(np.float64), (2, 2))


@pytest.mark.parametrize("shape, size", [((13, 7), (5, 9)), ((9, 15), (7, 7)), ((31, 17), (11, 6)), ((6, 5), (5, 7))])
def test_scale_crop_follows_the_reference_formulas_on_odd_sizes(shape, size):
    d = _dt()
    h, w = shape
    H, W = size
    img = (np.arange(h * w * 3).reshape(h, w, 3) % 251).astype(np.uint8)
    scale = max(H, W) / min(h, w)
    big = d.resize_linear_u8(img, (int(round(w * scale)), int(round(h * scale))))
    r0, c0 = big.shape[0] // 2 - H // 2, big.shape[1] // 2 - W // 2
    out = d.scale_crop(img, size)
    assert out.shape == (H, W, 3) and np.array_equal(out, big[r0:r0 + H, c0:c0 + W])
    assert min(big.shape[:2]) == max(H, W)


def test_count_components_uses_4_connectivity():
    d = _dt()
    m = np.zeros((6, 6), bool)
    assert d.count_components(m) == 0
    m[1, 1] = m[2, 2] = True                             # diagonal neighbours: two components (scipy.ndimage.label's default)
    assert d.count_components(m) == 2
    m[1, 2] = True
    assert d.count_components(m) == 1
    m[4:, 4:] = True
    assert d.count_components(m) == 2


# ------------------------------------------------------------------------------------------------------------------- sources
def test_procedural_source_is_deterministic_one_component_and_above_the_area_bound():
    d = _dt()
    a = d.ProceduralSource(11).draw(5, (147, 147))
    b = d.ProceduralSource(11).draw(5, (147, 147))
    c = d.ProceduralSource(12).draw(5, (147, 147))
    tail = d.ProceduralSource(11).draw(2, (147, 147), first=3)
    for k in ("bkgd", "frgd", "mask"):
        assert np.array_equal(a[k], b[k]) and not np.array_equal(a[k], c[k])
        assert np.array_equal(a[k][3:], tail[k])         # image i depends on (seed, i) only: chunking does not change it
    assert a["bkgd"].dtype == np.uint8 and a["frgd"].dtype == np.uint8 and a["mask"].dtype == bool
    for i in range(5):
        m = a["mask"][i]
        assert d.count_components(m) == 1 and m.mean() >= d.PROCEDURAL_MIN_FRACTION
        assert not a["frgd"][i][~m].any() and a["frgd"][i][m].any()
        assert a["bkgd"][i].std() > 10                   # textured, not flat
    small = d.ProceduralSource(3).draw(3, (64, 96))
    assert all(d.count_components(m) == 1 and m.mean() >= d.PROCEDURAL_MIN_FRACTION for m in small["mask"])


def test_folder_source_reads_bgr_and_applies_the_selection_rules(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    d = _dt()
    fg, bg = tmp_path / "fg", tmp_path / "bg"
    fg.mkdir(), bg.mkdir()
    rgb = np.zeros((240, 320, 3), np.uint8)
    rgb[..., 0] = 200                                    # red in RGB: channel 2 in BGR
    rgb[..., 1] = 30
    Image.fromarray(rgb).save(fg / "good.png")
    mask = np.zeros((240, 320), np.uint8)
    mask[10:230, 20:250] = 255                           # 220 * 230 = 50600 >= 40000, one component
    Image.fromarray(mask).save(fg / "good_mask.png")
    Image.fromarray(rgb).save(fg / "two.png")
    two = np.zeros_like(mask)
    two[:, :150] = 255
    two[:, 160:] = 255                                   # two components
    Image.fromarray(two).save(fg / "two_mask.png")
    Image.fromarray(rgb).save(fg / "small.png")
    small = np.zeros_like(mask)
    small[:150, :200] = 255                              # 30000 < 40000
    Image.fromarray(small).save(fg / "small_mask.png")
    Image.fromarray(rgb).save(fg / "nomask.jpg")
    blue = np.zeros((100, 130, 3), np.uint8)
    blue[..., 2] = 180
    Image.fromarray(blue).save(bg / "blue.png")
    src = d.FolderSource(str(fg), str(bg), seed=5)
    assert [os.path.basename(p) for p, _ in src.frgd] == ["good.png"]
    out = src.draw(2, (60, 50))
    assert out["bkgd"].shape == (2, 60, 50, 3) and out["mask"].dtype == bool
    assert (out["bkgd"][..., 0] == 180).all() and (out["bkgd"][..., 2] == 0).all()
    m = out["mask"][0]
    want = d.scale_crop(mask // 255, (60, 50)) > 0
    assert np.array_equal(m, want) and m.any() and not m.all()
    # object = image * mask, resized on its own (the reference's order): BGR inside, blended with zeros along the mask's edge
    assert (out["frgd"][0][..., 0] == 0).all() and np.array_equal(out["frgd"][0][30, 25], [0, 30, 200])
    assert out["frgd"][0][..., 2].max() == 200 and not out["frgd"][0][0, :, 2].any()
    with pytest.raises(ValueError, match="no usable foreground"):
        d.FolderSource(str(fg), str(bg), min_area=10 ** 6)


# ------------------------------------------------------------------------------------------ host arithmetic vs the reference
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_depth_planes_and_key_points_match_the_reference_bit_for_bit(case):
    d = _dt()
    g = load_golden("g19_textured_render")
    mask = g[f"{case}_mask"]
    dbg, dfg, dep = d.depth_planes(g[f"{case}_rel"], g[f"{case}_angle_u"] * 2 * np.pi, mask)
    assert digest(dbg) == str(g[f"{case}_sha_depth_bg"]) and digest(dfg) == str(g[f"{case}_sha_depth_fg"])
    assert digest(dep) == str(g[f"{case}_sha_depth"])
    assert np.array_equal(d.key_points(dbg, dfg, mask, int(g[f"{case}_n_interval"])), g[f"{case}_keys"])


def test_host_psf_tables_equal_the_references_to_one_ulp():
    d = _dt()
    g = load_golden("g19_textured_render")
    psfs = d.psf_list(g["b_keys"][None])[0]
    L = g["b_keys"].shape[1]
    ks = np.array([[[(psfs[s][a][j].shape[0] - 1) // 2 for j in range(L)] for a in range(2)] for s in range(2)])
    assert np.array_equal(ks, g["b_psf_k"])
    flat = np.concatenate([psfs[s][a][j].reshape(-1) for s in range(2) for a in range(2) for j in range(L)])
    ulp = np.spacing(np.abs(g["b_psf_flat"]))
    assert (np.abs(flat - g["b_psf_flat"]) <= ulp).all()
    assert (np.abs(flat) <= EPS).any() and (flat == 0).any()           # the near-focus layers with skipped taps are present
    tab, k, kmax = d.pack_psf([psfs])
    assert tab.shape == (1, 2, 2, L, 2 * kmax + 1, 2 * kmax + 1) and kmax == int(g["b_psf_k"].max())
    j = int(np.argmin(k[0, 0, 0]))
    c = int(k[0, 0, 0, j])
    assert np.array_equal(tab[0, 0, 0, j, kmax - c:kmax + c + 1, kmax - c:kmax + c + 1], psfs[0][0][j])
    assert tab[0, 0, 0, j].sum() == psfs[0][0][j].sum()                 # zero outside the kernel's own (2k+1)^2 window


def test_scene_parameters_are_sorted_seeded_and_in_range():
    d = _dt()
    a, b = d.draw_test_scenes(50, seed=4), d.draw_test_scenes(50, seed=4)
    c = d.draw_test_scenes(50, seed=5)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["rel"], c["rel"])
    assert (np.diff(a["rel"], axis=1) <= 0).all() and ((a["rel"] >= 0) & (a["rel"] < 1)).all()
    assert ((a["angles"] >= 0) & (a["angles"] < 2 * np.pi)).all()
    assert ((a["alphas"] >= 180) & (a["alphas"] < 200)).all()


# -------------------------------------------------------------------------------------------------------------------- driver
def test_driver_flags():
    d = _dt()
    a = d.parse_args(["--data_path", "out/T", "--num_sample_test", "5"])
    assert (a.big, a.source, a.seed, a.n_interval) == (False, "procedural", 1869, 150)
    assert a.size == (147, 147) and a.data_path == "out/T" and a.num_sample_test == 5
    assert a.Z_range == [0.75, 1.18] and a.alpha == [180, 200] and a.sigma == 2
    b = d.parse_args(["--big", "--source", "folder", "--frgd_path", "F/", "--bkgd_path", "B/", "--seed", "3", "--n_interval", "20"])
    assert (b.big, b.source, b.seed, b.n_interval, b.size) == (True, "folder", 3, 20, (587, 587))
    assert (b.frgd_path, b.bkgd_path) == ("F/", "B/")
    with pytest.raises(SystemExit):
        d.parse_args(["--n_interval", "0"])
    with pytest.raises(SystemExit):
        d.parse_args(["--source", "coco"])
    with pytest.raises(SystemExit):
        d.parse_args(["--no_such_flag", "1"])                # utils.get_args still rejects what neither parser knows
    import utils
    assert not hasattr(utils.get_args("data_gen_test", argv=[]), "n_interval")   # utils/args.py is the reference's


def test_driver_refuses_to_run_without_a_gpu(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(SystemExit, match="no GPU"):
        _dt().main(["--num_sample_test", "1", "--data_path", "/nonexistent"])
