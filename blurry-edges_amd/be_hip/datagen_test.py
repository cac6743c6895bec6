"""Textured test set on the GPU: the counterpart of test_data_generator.py (utils/args.py mode 'data_gen_test').

Per image: a masked foreground object over a background texture, each on its own tilted depth plane, defocused per
aperture through n_interval+1 depth layers (the reference's render_layer / render_image, :87-121), then photon + read
noise (:147-151).  Arrays keep the reference's layouts, dtypes (float64), BGR channel order and file names, so
data.TestDataset (and `python -m be_hip.workflow eval`) reads what `save` writes.

Split of the work:
  sources : foreground object + mask and background, uint8 BGR [n,H,W,3] - `ProceduralSource` (no data, deterministic) or
            `FolderSource` (user images, the reference's selection rules and scale-and-centre-crop).  Inputs, like decoding a JPEG.
  host    : scene parameters from be_hip.synth's counter-based streams (`draw_test_scenes`), the depth planes (:81-85,
            :123-133), the layer key points (:116-117) and the PSF tables (utils/data_generator.py:16-23; np.exp stays here).
  GPU     : the layered render (be_datagen_test_render_f64, csrc/be_datagen_test.hip) and the noise (be_datagen_noise_f64,
            the same arithmetic as :149-151 on the un-rounded clean image).

The reference draws its foregrounds from MS-COCO val2017 annotations and its backgrounds from a folder of paintings; turning
COCO annotations into FolderSource's layout (NAME.jpg + NAME_mask.png) is the user's step.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import native, synth
from .native import check, lib, stream_ptr

MIN_MASK_AREA = 40000              # the reference's COCO annotation area bound (:46), applied to the original mask
PROCEDURAL_MIN_FRACTION = 0.08     # ProceduralSource's foreground covers at least this fraction of the image
CHUNK = 8                          # images per render launch (bounded device footprint: PSF tables ~6 MB per image)


def dptr(t, name="tensor"):
    return native.dptr(t, name, dtypes=(torch.float64, torch.int32))


# ------------------------------------------------------------------------------------------------------------ image helpers
def count_components(mask: np.ndarray) -> int:
    """Number of 4-connected components of a 2-D boolean mask (scipy.ndimage.label's default structure, :22-24), by repeated
    masked dilation from one seed per component (numpy only: scipy need not be installed)."""
    left = np.asarray(mask, dtype=bool).copy()
    n = 0
    while left.any():
        n += 1
        grown = np.zeros_like(left)
        grown.flat[int(np.flatnonzero(left)[0])] = True
        while True:
            g = grown.copy()
            g[1:] |= grown[:-1]
            g[:-1] |= grown[1:]
            g[:, 1:] |= grown[:, :-1]
            g[:, :-1] |= grown[:, 1:]
            g &= left
            if np.array_equal(g, grown):
                break
            grown = g
        left &= ~grown
    return n


def _linear_coeffs(ssize: int, dsize: int):
    """Source index pairs and 11-bit weights of one axis of cv2.resize(INTER_LINEAR) on 8-bit data."""
    scale = 1.0 / (dsize / ssize)
    f = ((np.arange(dsize, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= ssize - 1
    f[low | high] = 0
    s[low] = 0
    s[high] = ssize - 1
    w0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)      # saturate_cast<short>: round half to even
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, np.minimum(s + 1, ssize - 1), w0, w1


def resize_linear_u8(src: np.ndarray, dsize) -> np.ndarray:
    """cv2.resize(src, dsize=(width, height), interpolation=INTER_LINEAR) for uint8 [h,w] or [h,w,c], restated: half-pixel
    centres (x_src = (x + 0.5) * w_src / w_dst - 0.5, computed in double, rounded to float), clamped to the edge, weights rounded
    to 11-bit fixed point (round((1 - f) * 2048), round(f * 2048)), a horizontal pass into int sums, a vertical pass and
    (sum + (1 << 21)) >> 22.  This follows OpenCV's scalar resize code (HResizeLinear / VResizeLinear with FixedPtCast); cv2 is
    not available offline, so it could not be checked against cv2 itself - OpenCV's SIMD vertical pass (shifting the
    intermediate sums before the multiply) may round differently by one in rare cases.  Known answers worked by hand pin it
    (tests/test_datagen_test_cpu.py)."""
    src = np.asarray(src)
    if src.dtype != np.uint8:
        raise TypeError("resize_linear_u8: uint8 input expected")
    dw, dh = int(dsize[0]), int(dsize[1])
    h, w = src.shape[:2]
    x0, x1, a0, a1 = _linear_coeffs(w, dw)
    y0, y1, b0, b1 = _linear_coeffs(h, dh)
    s = src.astype(np.int64)
    cw, ch = (1, dw) + (1,) * (src.ndim - 2), (dh, 1) + (1,) * (src.ndim - 2)
    rows = s[:, x0] * a0.reshape(cw) + s[:, x1] * a1.reshape(cw)         # [h, dw, ...] horizontal pass, scale 2^11
    out = rows[y0] * b0.reshape(ch) + rows[y1] * b1.reshape(ch)          # vertical pass, scale 2^22
    return np.clip((out + (1 << 21)) >> 22, 0, 255).astype(np.uint8)


def scale_crop(img: np.ndarray, size) -> np.ndarray:
    """The reference's scale-and-centre-crop (:59-65, :74-78): scale = max(size) / min(h, w), resize to
    (int(round(w * scale)), int(round(h * scale))), then rows from h'//2 - H//2 (H of them), columns likewise."""
    H, W = int(size[0]), int(size[1])
    scale = max(H, W) / min(img.shape[:2])
    r = resize_linear_u8(img, (int(round(img.shape[1] * scale)), int(round(img.shape[0] * scale))))
    top, left = r.shape[0] // 2 - H // 2, r.shape[1] // 2 - W // 2
    return r[top:top + H, left:left + W]


# ------------------------------------------------------------------------------------------------------------------ sources
class ProceduralSource:
    """Deterministic textures, no data.  Image i of seed s is a function of (s, i) only.
    background: three colour gratings of random orientation, frequency and phase plus smooth value noise (bilinear
    interpolation of a hashed 9x9 lattice); foreground mask: a star-shaped blob r(theta) = r0 (1 + sum_k a_k cos(k theta + p_k))
    around a point near the centre - star-shaped about an inside point, so one component - covering at least
    PROCEDURAL_MIN_FRACTION of the image; foreground object: its own texture times the mask.  uint8, BGR."""

    def __init__(self, seed: int = synth.SEED_DEFAULT):
        self.seed = int(seed)

    def _u(self, i, tag, shape):
        return synth.hash_uniform(self.seed, f"procedural.{i}.{tag}", shape)

    def _texture(self, i, tag, H, W):
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        g = self._u(i, tag + ".grating", (3, 5))
        img = np.zeros((H, W, 3))
        for k in range(3):
            th, per, ph = g[k, 0] * np.pi, 6.0 + g[k, 1] * 30.0, g[k, 2] * 2 * np.pi
            wave = 0.5 + 0.5 * np.sin(2 * np.pi * (x * np.cos(th) + y * np.sin(th)) / per + ph)
            col = self._u(i, f"{tag}.colour{k}", (3,))
            img += wave[..., None] * col * (0.25 + 0.25 * g[k, 3])
        lat = self._u(i, tag + ".noise", (9, 9, 3))
        gy, gx = y / max(H - 1, 1) * 8, x / max(W - 1, 1) * 8
        iy, ix = np.minimum(gy.astype(int), 7), np.minimum(gx.astype(int), 7)
        fy, fx = (gy - iy)[..., None], (gx - ix)[..., None]
        noise = (lat[iy, ix] * (1 - fy) * (1 - fx) + lat[iy + 1, ix] * fy * (1 - fx) + lat[iy, ix + 1] * (1 - fy) * fx
                 + lat[iy + 1, ix + 1] * fy * fx)
        img = img + 0.4 * noise
        img = img / img.max() * 255.0
        return np.clip(np.floor(img), 0, 255).astype(np.uint8)

    def _mask(self, i, H, W):
        p = self._u(i, "mask", (12,))
        m = min(H, W)
        cy, cx = (H - 1) / 2 + (p[0] - 0.5) * 0.1 * m, (W - 1) / 2 + (p[1] - 0.5) * 0.1 * m
        y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        th, r = np.arctan2(y - cy, x - cx), np.hypot(y - cy, x - cx)
        r0 = (0.25 + 0.1 * p[2]) * m
        shape = 1.0
        for k, (a, ph) in enumerate(zip(p[3:7], p[7:11]), start=2):
            shape = shape + 0.1 * a * np.cos(k * th + 2 * np.pi * ph)     # sum of amplitudes <= 0.4: r >= 0.6 r0 > 0
        return r <= r0 * shape

    def draw(self, n: int, size, first: int = 0) -> dict:
        H, W = int(size[0]), int(size[1])
        out = dict(bkgd=np.zeros((n, H, W, 3), np.uint8), frgd=np.zeros((n, H, W, 3), np.uint8), mask=np.zeros((n, H, W), bool))
        for j in range(n):
            i = first + j
            mask = self._mask(i, H, W)
            out["mask"][j] = mask
            out["frgd"][j] = self._texture(i, "fg", H, W) * mask[..., None]
            out["bkgd"][j] = self._texture(i, "bg", H, W)
        return out


def _read_bgr(path):
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("1", "L", "LA", "I", "I;16", "F"):
            return None                                                   # grey images are skipped (:55-56)
        a = np.asarray(im.convert("RGB"), dtype=np.uint8)
    return np.ascontiguousarray(a[..., ::-1])


class FolderSource:
    """User images read through PIL.  frgd_path: NAME.png / NAME.jpg with NAME_mask.png (nonzero = object); bkgd_path: any
    .png / .jpg / .jpeg.  Foregrounds obey the reference's rules: one connected component, mask area >= MIN_MASK_AREA
    pixels on the original mask, colour image; object = image * mask; both scale-and-centre-cropped to the image size
    (`scale_crop`).  Image i's choice of foreground and background comes from the counter-based streams of (seed, i);
    files are taken in sorted order.  uint8, BGR as cv2.imread gives."""

    _EXT = (".png", ".jpg", ".jpeg")

    def __init__(self, frgd_path: str, bkgd_path: str, seed: int = synth.SEED_DEFAULT, min_area: int = MIN_MASK_AREA):
        self.seed = int(seed)
        self.bkgd = sorted(os.path.join(bkgd_path, f) for f in os.listdir(bkgd_path) if f.lower().endswith(self._EXT))
        self.frgd = []
        for f in sorted(os.listdir(frgd_path)):
            stem, ext = os.path.splitext(f)
            if ext.lower() not in self._EXT or stem.endswith("_mask"):
                continue
            mpath = os.path.join(frgd_path, stem + "_mask.png")
            if not os.path.exists(mpath):
                continue
            from PIL import Image
            with Image.open(mpath) as im:
                mask = np.asarray(im.convert("L")) > 0
            if int(mask.sum()) < min_area or count_components(mask) != 1:
                continue
            self.frgd.append((os.path.join(frgd_path, f), mpath))
        if not self.frgd:
            raise ValueError(f"FolderSource: no usable foreground (NAME.png|jpg + NAME_mask.png, one component, area >= {min_area}) in {frgd_path}")
        if not self.bkgd:
            raise ValueError(f"FolderSource: no background image in {bkgd_path}")

    def draw(self, n: int, size, first: int = 0) -> dict:
        from PIL import Image
        H, W = int(size[0]), int(size[1])
        out = dict(bkgd=np.zeros((n, H, W, 3), np.uint8), frgd=np.zeros((n, H, W, 3), np.uint8), mask=np.zeros((n, H, W), bool))
        uf = synth.hash_uniform(self.seed, "folder.frgd", (first + n,))[first:]
        ub = synth.hash_uniform(self.seed, "folder.bkgd", (first + n,))[first:]
        for j in range(n):
            ipath, mpath = self.frgd[int(uf[j] * len(self.frgd))]
            img = _read_bgr(ipath)
            if img is None:
                raise ValueError(f"FolderSource: {ipath} is not a colour image")
            with Image.open(mpath) as im:
                mask = (np.asarray(im.convert("L")) > 0).astype(np.uint8)
            if mask.shape != img.shape[:2]:
                raise ValueError(f"FolderSource: {mpath} is {mask.shape}, its image {img.shape[:2]}")
            out["mask"][j] = scale_crop(mask, (H, W)) > 0
            out["frgd"][j] = scale_crop(img * mask[..., None], (H, W))
            bimg = _read_bgr(self.bkgd[int(ub[j] * len(self.bkgd))])
            if bimg is None:
                raise ValueError(f"FolderSource: background {self.bkgd[int(ub[j] * len(self.bkgd))]} is not a colour image")
            out["bkgd"][j] = scale_crop(bimg, (H, W))
        return out


# ------------------------------------------------------------------------------------------------------------ scene + depth
def draw_test_scenes(n, seed=synth.SEED_DEFAULT, alpha_range=(180, 200), name="test_scenes"):
    """Scene parameters of n images: the values the reference draws from np.random, kept raw so a test can replay it.
    rel [n,4] = four relative depths sorted descending (bg1, bg2, fg1, fg2; :123), angles [n,2] in [0, 2 pi) (:124),
    alphas [n] (:144)."""
    u = lambda tag, shape: synth.hash_uniform(seed, f"{name}.{tag}", shape)
    rel = np.flip(np.sort(u("depth", (n, 4)), axis=1), axis=1).copy()
    angles = u("angle", (n, 2)) * 2 * np.pi
    alphas = u("alpha", (n,)) * (alpha_range[1] - alpha_range[0]) + alpha_range[0]
    return dict(rel=rel, angles=angles, alphas=alphas)


def depth_planes(rel, angles, mask, z_range=(0.75, 1.18)):
    """One image's depth_bkgd, depth_frgd and the combined depth map [H,W] (:81-85, :125-133), the reference's operations."""
    H, W = mask.shape
    y, x = np.meshgrid(np.linspace(0, H - 1, H), np.linspace(0, W - 1, W), indexing="ij")
    org = np.array([W // 2, H // 2])
    modi = -np.sin(angles[:, None, None]) * (x[None, :, :] - org[0]) + np.cos(angles[:, None, None]) * (y[None, :, :] - org[1])

    def norm(m, kp):
        return (m - m.min()) / (m.max() - m.min()) * (kp[0] - kp[1]) + kp[1]

    def real(d):
        return (z_range[1] - z_range[0]) * d + z_range[0]

    bg, fg = norm(modi[0], rel[:2]), norm(modi[1], rel[2:])
    combined = bg * (1 - mask) + fg * mask
    return real(bg), real(fg), real(combined)


def key_points(depth_bg, depth_fg, mask, n_interval):
    """[2, n_interval+1]: np.linspace(max, min, n_interval+1) of the background plane and of the foreground plane over its mask."""
    return np.stack([np.linspace(depth_bg.max(), depth_bg.min(), n_interval + 1),
                     np.linspace(depth_fg[mask].max(), depth_fg[mask].min(), n_interval + 1)])


DEFAULT_CAM = dict(s=0.1104, rho=(10.0, 10.2), sigma_cam=0.003, pixel_pitch=5.86e-6, mag=4.0)


def cam_from_args(a):
    c = a.cam_params
    return dict(s=c["s"], rho=(c["rho_1"], c["rho_2"]), sigma_cam=c["sigma_cam"], pixel_pitch=c["pixel_pitch"], mag=a.mag)


def blur_kernel(sigma):
    """One PSF (utils/data_generator.py:19-23): (2k+1)^2, k = ceil(3 sigma), normalised, the reference's numpy operations."""
    sigma = max(sigma, 1e-6)
    k = np.ceil(np.abs(sigma) * 3).astype(np.int64)
    x, y = np.meshgrid(np.linspace(-k, k, k * 2 + 1), np.linspace(-k, k, k * 2 + 1))
    psf = np.exp(-np.power((x ** 2 + y ** 2) / (2 * sigma ** 2), 2 / 2))
    return psf / np.sum(psf)


def kernel_sigmas(z, cam=DEFAULT_CAM):
    """[2] PSF radius in pixels at depth z per aperture (utils/data_generator.py:16-17)."""
    rhos = np.array(cam["rho"], dtype=np.float64)
    return np.abs((1 / z - rhos) * cam["s"] + 1) * cam["sigma_cam"] / cam["pixel_pitch"] / cam["mag"]


def psf_list(keys, cam=DEFAULT_CAM):
    """keys [n,2,L] -> nested list [n][set][aperture][layer] of PSF arrays."""
    n, _, L = keys.shape
    out = [[[[None] * L for _ in range(2)] for _ in range(2)] for _ in range(n)]
    for i in range(n):
        for s in range(2):
            for j in range(L):
                for a, sig in enumerate(kernel_sigmas(keys[i, s, j], cam)):
                    out[i][s][a][j] = blur_kernel(sig)
    return out


def pack_psf(psfs, kmax=None):
    """Nested [n][2][2][L] PSFs -> (table [n,2,2,L,S,S] float64 with each kernel centred in its S = 2 kmax + 1 slot, k [n,2,2,L]
    int32, kmax): the layout be_datagen_test_render_f64 reads."""
    n, L = len(psfs), len(psfs[0][0][0])
    ks = np.array([[[[(p.shape[0] - 1) // 2 for p in layer] for layer in ap] for ap in img] for img in psfs], dtype=np.int32)
    kmax = int(ks.max()) if kmax is None else int(kmax)
    S = 2 * kmax + 1
    tab = np.zeros((n, 2, 2, L, S, S), dtype=np.float64)
    for i in range(n):
        for s in range(2):
            for a in range(2):
                for j in range(L):
                    k = int(ks[i, s, a, j])
                    tab[i, s, a, j, kmax - k:kmax + k + 1, kmax - k:kmax + k + 1] = psfs[i][s][a][j]
    return tab, ks, kmax


# ------------------------------------------------------------------------------------------------------------------- render
def render(bkgd, frgd, mask, depth_bg, depth_fg, keys, psf_table, psf_k, kmax, dev, all_layers=False):
    """The layered render on the GPU.  numpy inputs: bkgd, frgd [n,H,W,3], mask [n,H,W], depth_bg, depth_fg [n,H,W], keys
    [n,2,L], psf_table / psf_k / kmax from `pack_psf`.  Returns float64 GPU tensors img_clean [n,2,H,W,3], mask_blur [n,2,H,W]."""
    n, H, W = np.asarray(mask).shape
    t = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev)
    ins = [t(bkgd), t(frgd), t(mask), t(depth_bg), t(depth_fg), t(keys), t(psf_table), t(psf_k, torch.int32)]
    img = torch.empty(n, 2, H, W, 3, dtype=torch.float64, device=dev)
    mb = torch.empty(n, 2, H, W, dtype=torch.float64, device=dev)
    L = int(np.asarray(keys).shape[-1])
    check(lib().be_datagen_test_render_f64(*[dptr(x) for x in ins], ins[6].numel(), int(kmax), n, H, W, L - 1, int(bool(all_layers)),
                                           dptr(img), dptr(mb), stream_ptr(dev)), "be_datagen_test_render_f64")
    return img, mb


def generate(source, n, size, dev, seed=synth.SEED_DEFAULT, n_interval=150, z_range=(0.75, 1.18), alpha_range=(180, 200),
             sigma_read=2.0, cam=DEFAULT_CAM, chunk=CHUNK):
    """n textured image pairs.  Returns numpy float64 arrays with the reference's shapes (:138-158): images_gt, images_ny
    [n,2,H,W,3], depth_maps [n,H,W], alphas [n]; plus the clean render img_clean [n,2,H,W,3] and the masks [n,H,W]."""
    H, W = int(size[0]), int(size[1])
    sc = draw_test_scenes(n, seed=seed, alpha_range=alpha_range)
    alphas_t = torch.from_numpy(sc["alphas"]).to(dev)
    out = dict(images_gt=np.zeros((n, 2, H, W, 3)), images_ny=np.zeros((n, 2, H, W, 3)), depth_maps=np.zeros((n, H, W)),
               alphas=sc["alphas"].copy(), img_clean=np.zeros((n, 2, H, W, 3)), masks=np.zeros((n, H, W), bool))
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        src = source.draw(m, (H, W), first=first)
        dbg, dfg, keys = np.zeros((m, H, W)), np.zeros((m, H, W)), np.zeros((m, 2, n_interval + 1))
        for j in range(m):
            i = first + j
            dbg[j], dfg[j], out["depth_maps"][i] = depth_planes(sc["rel"][i], sc["angles"][i], src["mask"][j], z_range)
            keys[j] = key_points(dbg[j], dfg[j], src["mask"][j], n_interval)
        tab, ks, kmax = pack_psf(psf_list(keys, cam))
        img, _ = render(src["bkgd"], src["frgd"], src["mask"], dbg, dfg, keys, tab, ks, kmax, dev)
        gt = torch.empty_like(img)
        ny = torch.empty_like(img)
        check(lib().be_datagen_noise_f64(dptr(img), dptr(alphas_t[first:first + m]), float(sigma_read),
                                         (int(seed) + first) & 0xffffffff, m, 2 * H * W * 3, dptr(gt), dptr(ny), stream_ptr(dev)),
              "be_datagen_noise_f64")
        out["img_clean"][first:first + m] = img.cpu().numpy()
        out["images_gt"][first:first + m] = gt.cpu().numpy()
        out["images_ny"][first:first + m] = ny.cpu().numpy()
        out["masks"][first:first + m] = src["mask"]
    return out


def save(out, data_path, z_range=(0.75, 1.18)):
    """The files of :138-158: clean/{i}_{a}.png, noisy/{i}_{a}.png, depth_maps/{i}.png (as cv2.imwrite writes them: the BGR
    arrays flipped to RGB for PIL) and images_gt / images_ny / depth_maps / alphas .npy."""
    from PIL import Image
    for d in ("clean", "noisy", "depth_maps"):
        os.makedirs(os.path.join(data_path, d), exist_ok=True)
    n = out["alphas"].shape[0]
    for i in range(n):
        a = out["alphas"][i]
        for ap in range(2):
            for d, k in (("clean", "images_gt"), ("noisy", "images_ny")):
                px = (out[k][i, ap] / a * 255).astype(np.uint8)
                Image.fromarray(np.ascontiguousarray(px[..., ::-1])).save(os.path.join(data_path, d, f"{i}_{ap}.png"))
        dm = ((out["depth_maps"][i] - z_range[0]) / (z_range[1] - z_range[0]) * 255).astype(np.uint8)
        Image.fromarray(dm).save(os.path.join(data_path, "depth_maps", f"{i}.png"))
    for k in ("images_gt", "images_ny", "depth_maps", "alphas"):
        np.save(os.path.join(data_path, f"{k}.npy"), out[k])


def parse_args(argv=None):
    """utils.get_args('data_gen_test') plus the build's own flags (parsed here, so utils/args.py stays the reference's):
    --big, --source {procedural, folder}, --seed, --n_interval."""
    import argparse
    import utils
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--big", action="store_true")
    p.add_argument("--source", choices=("procedural", "folder"), default="procedural")
    p.add_argument("--seed", type=int, default=synth.SEED_DEFAULT)
    p.add_argument("--n_interval", type=int, default=150)
    own, rest = p.parse_known_args(argv)
    if own.n_interval < 1:
        raise SystemExit("--n_interval must be >= 1")
    a = utils.get_args("data_gen_test", argv=rest)
    for k, v in vars(own).items():
        setattr(a, k, v)
    a.size = tuple(a.big_img_size if own.big else a.img_size)
    return a


def main(argv=None):
    """`python -m be_hip.datagen_test [--big] --data_path T [--source procedural|folder] [--frgd_path F --bkgd_path B]
    [--num_sample_test N] [--seed S] [--n_interval 150]`: the build's test_data_generator.py."""
    import time
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("be_hip.datagen_test renders on the GPU; no GPU is visible")
    dev = torch.device(a.cuda)
    source = ProceduralSource(a.seed) if a.source == "procedural" else FolderSource(a.frgd_path, a.bkgd_path, seed=a.seed)
    t0 = time.perf_counter()
    out = generate(source, a.num_sample_test, a.size, dev, seed=a.seed, n_interval=a.n_interval, z_range=tuple(a.Z_range),
                   alpha_range=tuple(a.alpha), sigma_read=a.sigma, cam=cam_from_args(a))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    save(out, a.data_path, z_range=tuple(a.Z_range))
    n = a.num_sample_test
    print(f"test set: {n} image pairs {a.size[0]}x{a.size[1]} ({a.source}) in {dt:.2f} s ({n / dt:.2f} images/s) -> {a.data_path}")


if __name__ == "__main__":
    main()
