"""End-to-end depth estimation for one image pair: the build's counterpart of the reference's evaluation
harness (depth_estimator in blurry_edges_test.py:102-145 and blurry_edges_test_big.py:113-192).

image pair [2,3,H,W]  ->  unfold  ->  LocalStage (HIP)  ->  pass-A colours (HIP)  ->  feature normalisation (HIP)
  ->  GlobalStage (HIP)  ->  de-normalisation (HIP)  ->  pass-B records (HIP)
  ->  owner-computes fold (HIP)  ->  six maps + thresholded depth (or, with densify='pp', the DepthCompletion U-Net
  on the folded depth map, blurry_edges_test.py:141-142).
DepthPipeline.__call__ is the reference's one 147x147 pair, run_big its big-image tiler (sizes 59 + 88 k), run_any the same
pipeline for a pair of any size >= one block (flush-edge patch grid, be_hip/tiling.py).
All three return `records` (the [HP*WP,32] grid they fold) and `grid` (its geometry); DepthPipeline.refocus_stack turns those into a
focal stack - the pair refocused at K optical powers - with one more launch and no second pass B.
Nothing here computes on the CPU; tensors stay on the GPU until the caller asks for them.
"""
from __future__ import annotations

import math

import torch

from . import native, tiling


def params_src_layout(pm):
    """pm [P,38] = [P, (aperture, 19)] -> [2,P,19], the per-image layout global_data_pre_cal.py:27-32 saves in
    params_src_*.npy (and global_training.py reads back)."""
    return pm.view(-1, 2, 19).permute(1, 0, 2)


class DepthPipeline:
    def __init__(self, local_module, global_module, helper, depth_cal, rho_prime=10.39, densify=None, stride=2,
                 densify_pp_module=None):
        """helper: a utils.PostProcessGlobalBase (render options); depth_cal: utils.DepthEtas;
        densify_pp_module: a models.DepthCompletion in eval mode, required for densify='pp'."""
        if densify not in (None, "w", "pp"):
            raise ValueError(f"densify must be None, 'w' or 'pp' (utils/args.py:40), got {densify!r}")
        if densify == "pp" and densify_pp_module is None:
            raise ValueError("densify='pp' needs densify_pp_module (models.DepthCompletion, blurry_edges_test.py:193-196)")
        self.local, self.globl, self.pp = local_module, global_module, densify_pp_module
        self.helper, self.dcal = helper, depth_cal
        self.rho_prime, self.densify, self.stride = rho_prime, densify, stride
        self.depth_thres = 0.0 if densify == "w" else 0.05          # blurry_edges_test.py:109-112
        # global_module / depth_cal may be None when only local_pass is used (global_data_pre_cal.py counterpart)

    # ---- stages --------------------------------------------------------------------------------------
    def local_pass(self, img, window=None):
        """img [2,3,H,W] -> (view of the patch grid, est10 [2P,10], colors [2P,3,3], pm [P,38]).  Both kernels gather
        their 21x21 windows from the image; the unfolded [2,P,3,21,21] tensor of blurry_edges_test.py:120-121 is
        never written."""
        view = native.view_image_pair(img, self.stride, window)
        est10 = self.local.forward_image_pair(img, self.stride, window)
        colors, _ = native.render_colors_view(self.helper.render_opts(wrap_angles=True), est10, view, est10.shape[0] // 2)
        pm = native.local_features(est10, colors)
        return view, est10, colors, pm

    def global_pass(self, pm):
        """pm [P,38] -> est12 [P,12] (de-normalised wedge parameters)."""
        y = self.globl(pm.unsqueeze(0))
        return native.global_denorm(y[0])

    def records(self, est12, img, want=(), window=None):
        opts = self.helper.render_opts(wrap_angles=False)
        return native.render_full(opts, self.dcal.consts, self.rho_prime, self.densify == "w", est12,
                                  native.view_image_pair(img, self.stride, window), want=want, pixels=img)

    # ---- one 147x147 pair (blurry_edges_test.py:117-145) ---------------------------------------------
    @torch.no_grad()
    def __call__(self, img):
        img = img.contiguous()
        _, _, H, W = img.shape
        hp, wp = (H - native.BE_R) // self.stride + 1, (W - native.BE_R) // self.stride + 1
        _, est10, colors, pm = self.local_pass(img)
        est12 = self.global_pass(pm)
        rec, _ = self.records(est12, img)
        maps = native.fold_records(self.helper.render_opts(False), rec, hp, wp, H, W, self.stride, self.densify == "w")
        if self.densify == "pp":
            maps["depth_map"] = self.pp(maps["depth"][None, None])[0, 0]
        else:
            maps["depth_map"] = torch.where(maps["conf"] > self.depth_thres, maps["depth"], torch.zeros_like(maps["depth"]))
        maps.update(est10=est10, colors_a=colors, est12=est12, records=rec,
                    grid=dict(H=H, W=W, hp=hp, wp=wp, stride=self.stride, ys=None, xs=None))
        return maps

    # ---- big image: 147x147 blocks with margin patches dropped (blurry_edges_test_big.py:116-189) -----
    @staticmethod
    def big_windows(H, W, block=147, n_margin=10, stride=2, R=21):
        """Block schedule of the big-image tiler (blurry_edges_test_big.py:118-119,166-177): a list of
        ((top, left, block, block) pixel window, (vs, ve, hs, he) kept rows/cols of the block's patch grid,
        (Vs, Hs) where that kept window starts in the big patch grid)."""
        bstride = block - R + stride - 2 * stride * n_margin                        # 88
        nb_v = math.ceil((H - R - 2 * stride * n_margin + stride) / bstride)
        nb_h = math.ceil((W - R - 2 * stride * n_margin + stride) / bstride)
        hp = (block - R) // stride + 1                                              # 64
        step = hp - 2 * n_margin                                                    # 44 patches = bstride / stride
        out = []
        for bi in range(nb_v):
            for bj in range(nb_h):
                vs = 0 if bi == 0 else n_margin
                ve = hp if bi == nb_v - 1 else hp - n_margin
                hs = 0 if bj == 0 else n_margin
                he = hp if bj == nb_h - 1 else hp - n_margin
                out.append(((bi * bstride, bj * bstride, block, block), (vs, ve, hs, he), (bi * step + vs, bj * step + hs)))
        return out

    @torch.no_grad()
    def run_big(self, img, block=147, n_margin=10, rank=0, world=1, group=None, dedup=True):
        """rank / world: this process handles the blocks shard.my_blocks gives it; the record grid is completed with one
        all-reduce (shard.assemble_records) and every rank folds the full image.  world = 1: no communication.

        dedup=True (default): the reference calls the CNN once per 147x147 block (blurry_edges_test_big.py:142-165): 36 x 8192 =
        294 912 patches for the 2 x 284 x 284 = 161 312 DISTINCT windows of a 587x587 pair (neighbouring blocks share their 20
        margin rows / columns of patches).  LocalStage, pass A and the feature glue are per-patch and position-independent bit for
        bit, so here they run ONCE over the whole patch grid and every block gathers its 64x64 rows of `pm` from it: same
        numbers, 45 % fewer patches.  With world > 1 the local pass is sharded by rows of the patch grid (shard.row_range) and the
        feature grid is completed by one all-reduce before the blocks - which GlobalStage's attention keeps whole - are dealt out.
        dedup=False: the reference's schedule, one local pass per block."""
        from . import shard
        img = img.contiguous()
        _, _, H, W = img.shape
        s, R = self.stride, native.BE_R
        hp = (block - R) // s + 1
        HP, WP = (H - R) // s + 1, (W - R) // s + 1                                 # 284
        # blocks are windows of the big image: no cropped copies, no unfolded copies
        big = torch.zeros(HP * WP, native.RECORD_FLOATS, dtype=torch.float32, device=img.device).view(HP, WP, -1)
        wins = self.big_windows(H, W, block, n_margin, s, R)
        mine = shard.my_blocks(len(wins), rank, world)
        if dedup:
            r0, r1 = shard.row_range(HP, rank, world)
            if world > 1:
                grid = torch.zeros(HP, WP, 38, dtype=torch.float32, device=img.device)
                if r1 > r0:
                    grid[r0:r1] = self.local_pass(img, (r0 * s, 0, (r1 - r0 - 1) * s + R, W))[3].view(r1 - r0, WP, 38)
                grid = shard.assemble_records(grid, group)                          # x + 0 is exact: rows are owned once
            else:
                grid = self.local_pass(img)[3].view(HP, WP, 38)
            # a block whose pixel window starts at (top, left) owns the patch rows top/s .. top/s + hp - 1 of the big grid
            feats = [grid[wins[k][0][0] // s:wins[k][0][0] // s + hp, wins[k][0][1] // s:wins[k][0][1] // s + hp].reshape(hp * hp, 38)
                     for k in mine]
        else:
            # local stage block by block (8192 patches each = one CNN sub-batch)
            feats = [self.local_pass(img, wins[k][0])[3] for k in mine]
        # GlobalStage on groups of blocks in one batch (attention at batch 1 leaves three quarters of the SIMD slots empty),
        # then pass B per block
        est = []
        for g0 in range(0, len(mine), 12):
            y = self.globl(torch.stack(feats[g0:g0 + 12]))                          # [g,4096,12]
            est.extend(native.global_denorm(y[i]) for i in range(y.shape[0]))
        for k, est12 in zip(mine, est):
            win, (vs, ve, hs, he), (Vs, Hs) = wins[k]
            rec, _ = self.records(est12, img, window=win)
            big[Vs:Vs + ve - vs, Hs:Hs + he - hs] = rec.view(hp, hp, -1)[vs:ve, hs:he]
        if world > 1:
            big = shard.assemble_records(big, group)
        maps = native.fold_records(self.helper.render_opts(False), big.view(HP * WP, -1), HP, WP, H, W, s, self.densify == "w")
        if self.densify == "pp":
            maps["depth_map"] = self.pp(maps["depth"][None, None])[0, 0]
        else:                                                                       # blurry_edges_test_big.py:189
            maps["depth_map"] = torch.where(maps["conf"] > 0.05, maps["depth"], torch.zeros_like(maps["depth"]))
        maps.update(records=big.view(HP * WP, -1), grid=dict(H=H, W=W, hp=HP, wp=WP, stride=s, ys=None, xs=None))
        return maps

    # ---- any size >= one block: flush-edge patch grid + pulled-back last block (be_hip/tiling.py) -----------------------
    def local_grid(self, img):
        """pm of every patch of the flush-edge grid, [HP, WP, 38], each distinct window through LocalStage once: the uniform part
        of the grid in one local pass over the image, the flush row / column / corner (where the size asks for them) in one
        local pass each over the 21-pixel strip that holds them."""
        _, _, H, W = img.shape
        s, R = self.stride, native.BE_R
        hu, wu = (H - R) // s + 1, (W - R) // s + 1
        fv, fh = (H - R) % s != 0, (W - R) % s != 0
        core = self.local_pass(img)[3].view(hu, wu, 38)
        if not (fv or fh):
            return core
        grid = torch.empty(hu + fv, wu + fh, 38, dtype=torch.float32, device=img.device)
        grid[:hu, :wu] = core
        if fv:
            grid[hu, :wu] = self.local_pass(img, (H - R, 0, R, W))[3]
        if fh:
            grid[:hu, wu] = self.local_pass(img, (0, W - R, H, R))[3]
        if fv and fh:
            grid[hu, wu] = self.local_pass(img, (H - R, W - R, R, R))[3][0]
        return grid

    @torch.no_grad()
    def run_any(self, img, block=147, n_margin=10):
        """img [2,3,H,W] with H, W >= block, ANY such size -> the dict of run_big (image, shpd, refoc, bndry, depth, conf,
        depth_map, records [HP*WP,32], grid; plus est12 [HP*WP,12] of the whole grid; grid holds the device origin tables).

        Patch grid: tiling.patch_grid per axis - origins 0, s, 2s, .. and one more flush with the edge at H - 21 when the
        uniform grid stops short of it, so every pixel is covered (the uniform fold leaves 0/0 in the last row / column
        otherwise).  Blocks: tiling.block_schedule - 64 consecutive grid lines each, 44 apart, the last pulled back to end on
        the grid's last line; a grid line is kept by one block and never closer than n_margin to an inner block edge.  For the
        sizes the reference defines (59 + 88 k) grid and schedule ARE run_big's and the maps are equal bit for bit (147x147:
        equal to __call__).  GlobalStage always sees 64 x 64 tokens in the layout it was trained on; in the last block of an
        axis with a flush line the final gap between two lines is smaller than the stride - the one place the input geometry
        differs from training.

        LocalStage runs once per distinct window (as run_big(dedup=True)); the blocks go through GlobalStage in groups of 12 in
        row-major order (run_big's grouping); the kept est12 rows are gathered into ONE [HP,WP,12] grid, rendered by one
        render_full_grid launch and folded by one fold_records_grid launch.  Single process only: sharding over ranks
        (run_big's rank / world) is not offered here."""
        img = img.contiguous()
        if img.dim() != 4 or img.shape[0] != 2 or img.shape[1] != 3:
            raise ValueError(f"run_any: expected img [2,3,H,W], got {tuple(img.shape)}")
        _, _, H, W = img.shape
        if H < block or W < block:
            raise ValueError(f"run_any: a {H}x{W} pair is smaller than one {block}x{block} block; DepthPipeline.__call__ takes "
                             f"a pair whose whole patch grid fits one GlobalStage input")
        s, R = self.stride, native.BE_R
        hp = (block - R) // s + 1
        ys, xs, blocks = tiling.any_windows(H, W, block, n_margin, s, R)
        tiling.check_grid(ys, H, s, R)
        tiling.check_grid(xs, W, s, R)
        HP, WP = len(ys), len(xs)
        grid = self.local_grid(img)
        assert tuple(grid.shape) == (HP, WP, 38)
        feats = [grid[sv:sv + hp, sh:sh + hp].reshape(hp * hp, 38) for (sv, sh), _, _ in blocks]
        est = torch.empty(HP, WP, 12, dtype=torch.float32, device=img.device)
        for g0 in range(0, len(blocks), 12):
            y = self.globl(torch.stack(feats[g0:g0 + 12]))                          # [g,4096,12]
            for i in range(y.shape[0]):
                _, (vs, ve, hs, he), (Vs, Hs) = blocks[g0 + i]
                est[Vs:Vs + ve - vs, Hs:Hs + he - hs] = native.global_denorm(y[i]).view(hp, hp, 12)[vs:ve, hs:he]
        est = est.view(HP * WP, 12)
        dev_ys = native.origin_table(ys, H, img.device, "run_any(ys)", cover=True)
        dev_xs = native.origin_table(xs, W, img.device, "run_any(xs)", cover=True)
        rec = native.render_full_grid(self.helper.render_opts(False), self.dcal.consts, self.rho_prime, self.densify == "w", est, img,
                                      dev_ys, dev_xs)
        maps = native.fold_records_grid(self.helper.render_opts(False), rec, H, W, dev_ys, dev_xs, self.densify == "w")
        if self.densify == "pp":
            maps["depth_map"] = self.pp(maps["depth"][None, None])[0, 0]
        else:                                                                       # as run_big (blurry_edges_test_big.py:189)
            maps["depth_map"] = torch.where(maps["conf"] > 0.05, maps["depth"], torch.zeros_like(maps["depth"]))
        maps.update(est12=est, records=rec, grid=dict(H=H, W=W, hp=HP, wp=WP, stride=s, ys=dev_ys, xs=dev_xs))
        return maps

    # ---- focal stack from one depth estimate ----------------------------------------------------------------------------
    @torch.no_grad()
    def refocus_stack(self, maps, rho_primes=None, focus_depths=None, scale=1, window=None, points=None):
        """maps: what __call__, run_big or run_any returned.  Exactly one of rho_primes (optical powers, dioptres) and
        focus_depths (metres, through DepthEtas.focus2rho) -> [K,3,H,W]: the pair refocused at each of them.  Plane k is what
        maps["refoc"] would be had the pipeline been built with rho_prime = rho_primes[k] - the colours and wedge depths in
        maps["records"] do not depend on rho_prime, so pass B is not run again and one launch folds all K planes
        (native.fold_refocus_stack).  scale / window other than (1, None): the planes on the lattice of render_at,
        [K,3,Ho,Wo] (native.fold_refocus_stack_at); their [::scale, ::scale] samples are the pixels of the default call.
        points [...,2] (instead of scale / window): the planes at those (y, x) positions, the positions of sample_at (float32),
        [K,3,*lead] (native.fold_refocus_stack_points); a point outside the image gives 0 in every plane."""
        if (rho_primes is None) == (focus_depths is None):
            raise ValueError("refocus_stack: give exactly one of rho_primes (optical powers) and focus_depths (metres)")
        if points is not None and (scale != 1 or window is not None):
            raise ValueError("refocus_stack: points replaces the lattice; pass it without scale / window")
        if not isinstance(maps, dict) or "records" not in maps or "grid" not in maps:
            missing = [k for k in ("records", "grid") if not isinstance(maps, dict) or k not in maps]
            raise ValueError(f"refocus_stack: maps lacks {missing}; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        rec, g = maps["records"], maps["grid"]
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise ValueError("refocus_stack: maps['records'] is not on the GPU; nothing here computes on the CPU "
                             "(keep the dict the pipeline returned, or move records - and the ys / xs of grid - back to the device)")
        if focus_depths is not None:
            if isinstance(focus_depths, torch.Tensor):
                rho_primes = self.dcal.focus2rho(focus_depths.detach().double().cpu()).tolist()
            else:
                rho_primes = [self.dcal.focus2rho(z) for z in focus_depths]
        if points is not None:
            return native.fold_refocus_stack_points(self.helper.render_opts(False), self.dcal.consts, rec, rho_primes, g["H"], g["W"],
                                                    _points_on(points, rec.device, "refocus_stack"), hp=g["hp"], wp=g["wp"],
                                                    stride=g["stride"], ys=g["ys"], xs=g["xs"])
        if scale == 1 and window is None:
            return native.fold_refocus_stack(self.helper.render_opts(False), self.dcal.consts, rec, rho_primes, g["H"], g["W"],
                                             hp=g["hp"], wp=g["wp"], stride=g["stride"], ys=g["ys"], xs=g["xs"])
        return native.fold_refocus_stack_at(self.helper.render_opts(False), self.dcal.consts, rec, rho_primes, g["H"], g["W"], scale=scale,
                                            window=window, hp=g["hp"], wp=g["wp"], stride=g["stride"], ys=g["ys"], xs=g["xs"])

    # ---- the folded maps on a finer lattice -----------------------------------------------------------------------------
    @torch.no_grad()
    def render_at(self, maps, scale=1, window=None, want=None, depth_thres=None):
        """maps: what __call__, run_big or run_any returned (maps["records"], maps["grid"] are read) -> the folded maps sampled on a
        lattice `scale` (an integer k in 1..16) times finer than the pixels, over window = (top, left, h, w) in input pixels (None:
        the whole image): each map [..,Ho,Wo] with Ho = (h-1) k + 1, Wo = (w-1) k + 1.  The record grid is a continuous description
        of the scene, so the finer samples are evaluated from the wedges, not interpolated from the pixel maps; out[..., ::k, ::k]
        equals the pixel map over the window bit for bit.  want: names out of native.FOLD_MAPS (None: all six).  Also returned:
        lattice = dict(scale, window, Ho, Wo) and - unless densify == 'pp', whose U-Net is not defined off its native resolution -
        depth_map = where(conf > depth_thres, depth, 0).  depth_thres defaults to self.depth_thres, the threshold of __call__;
        run_big and run_any use 0.05 whatever densify is, so pass depth_thres=0.05 to continue their depth_map."""
        if not isinstance(maps, dict) or "records" not in maps or "grid" not in maps:
            missing = [k for k in ("records", "grid") if not isinstance(maps, dict) or k not in maps]
            raise ValueError(f"render_at: maps lacks {missing}; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        rec, g = maps["records"], maps["grid"]
        lat = tiling.lattice(g["H"], g["W"], scale, window)
        want = native.FOLD_MAPS if want is None else tuple(want)
        unknown = [k for k in want if k not in native.FOLD_MAPS]
        if unknown:
            raise ValueError(f"render_at: unknown maps {unknown}; choose from {native.FOLD_MAPS}")
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise ValueError("render_at: maps['records'] is not on the GPU; nothing here computes on the CPU "
                             "(keep the dict the pipeline returned, or move records - and the ys / xs of grid - back to the device)")
        need = want if self.densify == "pp" else tuple(k for k in native.FOLD_MAPS if k in want or k in ("depth", "conf"))
        out = native.fold_records_at(self.helper.render_opts(False), rec, g["H"], g["W"], scale=scale, window=window, hp=g["hp"], wp=g["wp"],
                                     stride=g["stride"], ys=g["ys"], xs=g["xs"], densify_w=self.densify == "w", want=need)
        res = {k: out[k] for k in want}
        if self.densify != "pp":
            thres = self.depth_thres if depth_thres is None else depth_thres
            res["depth_map"] = torch.where(out["conf"] > thres, out["depth"], torch.zeros_like(out["depth"]))
        res["lattice"] = lat
        return res

    # ---- the folded maps at arbitrary positions -------------------------------------------------------------------------
    @torch.no_grad()
    def sample_at(self, maps, points, want=None, depth_thres=None):
        """maps: what __call__, run_big or run_any returned (maps["records"], maps["grid"] are read); points [...,2]: (y, x)
        positions in input-pixel coordinates, pixel centres at the integers, the coordinate top + iy / k of render_at -> the
        folded maps at those positions, evaluated from the wedges, not interpolated: image [2,3,*lead], shpd / refoc [3,*lead],
        bndry / depth / conf [*lead].  Positions are float32: a tensor, or anything torch.as_tensor takes, of another dtype or on
        another device is converted.  The domain is closed, 0 <= y <= H-1 and 0 <= x <= W-1; valid [*lead] (bool, computed on the
        device, no sync) says which points lie in it, the others (NaN included) have 0 in every map.  A point on a pixel centre
        equals the pixel map bit for bit, a point of render_at's lattice at scale 2, 4, 8 or 16 equals that sample, and every
        point is evaluated on its own.  want, depth_thres and depth_map (absent under densify == 'pp'): as render_at."""
        if not isinstance(maps, dict) or "records" not in maps or "grid" not in maps:
            missing = [k for k in ("records", "grid") if not isinstance(maps, dict) or k not in maps]
            raise ValueError(f"sample_at: maps lacks {missing}; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        rec, g = maps["records"], maps["grid"]
        points = _points_on(points, None, "sample_at")
        want = native.FOLD_MAPS if want is None else tuple(want)
        unknown = [k for k in want if k not in native.FOLD_MAPS]
        if unknown:
            raise ValueError(f"sample_at: unknown maps {unknown}; choose from {native.FOLD_MAPS}")
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise ValueError("sample_at: maps['records'] is not on the GPU; nothing here computes on the CPU "
                             "(keep the dict the pipeline returned, or move records - and the ys / xs of grid - back to the device)")
        points = points.to(rec.device)
        need = want if self.densify == "pp" else tuple(k for k in native.FOLD_MAPS if k in want or k in ("depth", "conf"))
        out = native.fold_records_points(self.helper.render_opts(False), rec, g["H"], g["W"], points, hp=g["hp"], wp=g["wp"],
                                         stride=g["stride"], ys=g["ys"], xs=g["xs"], densify_w=self.densify == "w", want=need)
        res = {k: out[k] for k in want}
        y, x = points[..., 0], points[..., 1]
        res["valid"] = (y >= 0) & (y <= g["H"] - 1) & (x >= 0) & (x <= g["W"] - 1)      # the kernel's predicate, in float32
        if self.densify != "pp":
            thres = self.depth_thres if depth_thres is None else depth_thres
            res["depth_map"] = torch.where(out["conf"] > thres, out["depth"], torch.zeros_like(out["depth"]))
        return res

    @torch.no_grad()
    def render_resized(self, maps, size, window=None, want=None, depth_thres=None):
        """The maps of sample_at on the align-corners grid of size = (Ho, Wo) samples over window = (top, left, h, w) in input
        pixels (None: the whole image), tiling.resize_points: each map [..,Ho,Wo], the first and last samples on the window's
        first and last pixel centres.  Any ratio, up or down; (k (h-1) + 1, k (w-1) + 1) with k = 2, 4, 8, 16 is
        render_at(scale=k) bit for bit.  Also returned: lattice = dict(size, window); valid is all True."""
        if not isinstance(maps, dict) or "grid" not in maps:
            raise ValueError("render_resized: maps lacks ['grid']; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        g = maps["grid"]
        pts = tiling.resize_points(g["H"], g["W"], size, window)
        res = self.sample_at(maps, torch.from_numpy(pts), want=want, depth_thres=depth_thres)
        res["lattice"] = dict(size=(pts.shape[0], pts.shape[1]), window=tiling.lattice(g["H"], g["W"], 1, window)["window"])
        return res


    # ---- forward reprojection: the depth map and the maps that ride on it, seen from another camera ----------------------
    def _depth_samples(self, who, maps, scale, window, want, depth_thres):
        """The source of point_cloud and reproject: the samples of render_at(scale, window) with their depth_map.  At the defaults
        the maps already in `maps` are used and nothing is launched.  -> (dict of the wanted maps and depth_map, lattice)."""
        if not isinstance(maps, dict) or "records" not in maps or "grid" not in maps:
            missing = [k for k in ("records", "grid") if not isinstance(maps, dict) or k not in maps]
            raise ValueError(f"{who}: maps lacks {missing}; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        rec, g = maps["records"], maps["grid"]
        lat = tiling.lattice(g["H"], g["W"], scale, window)
        unknown = [k for k in want if k not in native.FOLD_MAPS]
        if unknown:
            raise ValueError(f"{who}: unknown maps {unknown}; choose from {native.FOLD_MAPS}")
        if not isinstance(rec, torch.Tensor) or not rec.is_cuda:
            raise ValueError(f"{who}: maps['records'] is not on the GPU; nothing here computes on the CPU "
                             "(keep the dict the pipeline returned, or move records - and the ys / xs of grid - back to the device)")
        if self.densify == "pp" and scale != 1:
            raise ValueError(f"{who}: densify='pp' has no depth_map off the pixels (the U-Net is not defined off its native "
                             f"resolution): scale must be 1, got {scale}")
        if "depth_map" not in maps and (self.densify == "pp" or (scale == 1 and window is None and depth_thres is None)):
            raise ValueError(f"{who}: maps lacks ['depth_map']; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        if scale == 1 and window is None and depth_thres is None:
            # the pixels themselves: maps["depth_map"] is the depth source whatever threshold its entry point used (run_big and
            # run_any: 0.05), and only a wanted map that `maps` does not hold is rendered again
            missing = tuple(k for k in want if k not in maps)
            src = {k: maps[k] for k in want if k in maps}
            if missing:
                src.update({k: v for k, v in self.render_at(maps, want=missing).items() if k in missing})
            src["depth_map"] = maps["depth_map"]
            return src, lat
        src = self.render_at(maps, scale=scale, window=window, want=want, depth_thres=depth_thres)
        if self.densify == "pp":
            top, left, h, w = lat["window"]
            src["depth_map"] = maps["depth_map"][top:top + h, left:left + w].contiguous()
        return src, lat

    @torch.no_grad()
    def point_cloud(self, maps, pose=None, scale=1, window=None, depth_thres=None):
        """maps: what __call__, run_big or run_any returned -> the samples of render_at(scale, window) (the pixels by default) as
        points in space: xyz [3,Ho,Wo] = (X, Y, Z) in metres, Z = depth_map along the optical axis, through the pinhole camera
        dcal.intrinsics(H, W), in the frame `pose` maps the camera's to (camera.pose; None: the camera's own).  valid [Ho,Wo]:
        depth_map is a finite number > 0 (on the device, no sync); xyz is 0 elsewhere.  Also returned: shpd [3,Ho,Wo] and conf of
        the same samples, and lattice.  depth_thres: as render_at."""
        src, lat = self._depth_samples("point_cloud", maps, scale, window, ("shpd", "conf"), depth_thres)
        g = maps["grid"]
        z = src["depth_map"]
        xyz = native.unproject(z, self.dcal.intrinsics(g["H"], g["W"]), pose, scale=lat["scale"], window_origin=lat["window"][:2])
        return dict(xyz=xyz, valid=(z > 0) & torch.isfinite(z), shpd=src["shpd"], conf=src["conf"], lattice=lat)

    @torch.no_grad()
    def reproject(self, maps, cam_dst=None, pose=None, size=None, want=("shpd",), scale=1, window=None, near=1e-3, depth_thres=None,
                  cam_src=None):
        """"Align depth to colour": maps (what __call__, run_big or run_any returned) forward-warped to the camera cam_dst
        (camera.Pinhole, (fy, fx, cy, cx) or a 3x3 K) that sits at `pose` (camera.pose: X' = R X + t from this camera's frame to
        that one's), size = (Ho, Wo) pixels -> depth [Ho,Wo] along cam_dst's axis, valid, index (the winner's linear index in the
        source lattice, -1 where nothing landed) and the `want`ed maps out of native.FOLD_MAPS gathered from the winning sample,
        with the channel counts render_at gives them.  Where two samples land on one pixel the nearer wins; where none lands
        every map is 0 - holes are left open.  The source samples and their depth_map are those of render_at(scale, window,
        depth_thres=..) - at scale 1 without a window and a depth_thres, maps["depth_map"] itself, with the threshold of the entry
        that made it; off those defaults pass depth_thres=0.05 to continue run_big's / run_any's: scale = k splats k^2 samples per pixel, each evaluated from the wedges, which closes the cracks of a
        magnifying view.  Defaults: cam_src = dcal.intrinsics(H, W), cam_dst = cam_src, size = (H, W), the identity pose - which
        returns the maps themselves wherever depth_map > 0.  Under densify == 'pp' the depth source is maps["depth_map"] and scale
        must be 1.  lattice: the source lattice."""
        want = tuple(want)
        src, lat = self._depth_samples("reproject", maps, scale, window, want, depth_thres)
        g = maps["grid"]
        cam_src = self.dcal.intrinsics(g["H"], g["W"]) if cam_src is None else cam_src
        cam_dst = cam_src if cam_dst is None else cam_dst
        size = (g["H"], g["W"]) if size is None else size
        z = src["depth_map"]
        feat, channels = pack_channels(src, want, z.numel())
        out = native.reproject(z, cam_src, cam_dst, pose, size, feat=feat, near=near, scale=lat["scale"],
                               window_origin=lat["window"][:2])
        res = dict(depth=out["depth"], valid=out["valid"], index=out["index"], lattice=lat)
        res.update(unpack_channels(out["feat"], channels, out["depth"].shape))
        return res


    # ---- multi-view fusion: the depth of several pairs, each with its pose, merged in one camera -----------------------------
    def _views(self, who, views, want, scale=1, depth_thres=None, source="depth_map", complete_kw=None):
        """[(maps, pose), ..] of fuse / integrate (a list: _view_pairs) -> (the view dicts native.fuse_views and native.tsdf_integrate
        take - the samples of _depth_samples, conf as weight, the `want`ed maps packed as feat, each view in the camera
        dcal.intrinsics(H, W) of its own size; source="complete": complete(maps, **complete_kw)'s dense depth in place of depth_map -,
        the first view's layout = dict(want, channels (pack_channels), camera, size))."""
        vs, layout = [], None
        for i, item in enumerate(views):
            try:
                maps, pose = item
            except (TypeError, ValueError):
                raise ValueError(f"{who}: views[{i}] must be (maps, pose)") from None
            src, lat = self._depth_samples(f"{who}(views[{i}])", maps, scale, None, want + ("conf",), depth_thres)
            g = maps["grid"]
            cam = self.dcal.intrinsics(g["H"], g["W"])
            z = src["depth_map"] if source == "depth_map" else self.complete(maps, **dict(complete_kw or {}))["depth_dense"]
            feat, channels = pack_channels(src, want, z.numel())
            if layout is None:
                layout = dict(want=want, channels=channels, camera=cam, size=(g["H"], g["W"]))
            vs.append(dict(depth=z, weight=src["conf"].reshape(z.shape).to(torch.float32), feat=feat, cam_src=cam, pose=pose,
                           scale=lat["scale"], window_origin=lat["window"][:2]))
        return vs, layout

    @torch.no_grad()
    def fuse(self, views, cam_dst=None, size=None, want=("shpd",), tau=0.05, min_views=1, recentre=True, peel=0, scale=1, near=1e-3,
             depth_thres=None):
        """views: a list of 1..32 (maps, pose) - what __call__, run_big or run_any returned for one pair, and the pose of that
        pair's camera into the target frame (camera.pose: X' = R X + t; None: the identity) -> the depth of all of them merged in
        the camera cam_dst, size = (Ho, Wo): depth [Ho,Wo] along cam_dst's axis, valid, weight (the sum of the conf of the samples
        that agreed), views and count (how many distinct views and how many samples agreed), layer (the round that kept the pixel,
        -1 where none did) and the `want`ed maps out of native.FOLD_MAPS as the conf-weighted mean over those samples, with the
        channel counts reproject gives them.  Each view's samples are those reproject would splat (render_at(scale, depth_thres)
        with their depth_map; the maps themselves at the defaults), each in the camera dcal.intrinsics(H, W) of its own size;
        their weights are conf.  tau (metres), min_views, recentre, peel: native.fuse_views - samples within tau behind the
        nearest are averaged, a pixel needs min_views distinct views, and a front that too few views confirm is peeled off in up to
        `peel` further rounds.  More views give more coverage and less noise, and min_views >= 2 rejects what no second view
        confirms.  Defaults: the first view's camera and size.  The result does not depend on the order of the views.  Holes are
        left open: native.fill_nearest and native.fill_diffuse, called as (out["depth"], out["weight"]), close what is left."""
        want = tuple(want)
        vs, layout = self._views("fuse", _view_pairs("fuse", views), want, scale, depth_thres)
        cam_dst = layout["camera"] if cam_dst is None else cam_dst
        size = layout["size"] if size is None else size
        out = native.fuse_views(vs, cam_dst, size, tau=tau, min_views=min_views, recentre=recentre, peel=peel, near=near)
        res = {k: out[k] for k in ("depth", "valid", "weight", "views", "count", "layer")}
        res.update(unpack_channels(out["feat"], layout["channels"], out["depth"].shape))
        return res


    # ---- TSDF volumes: views integrated one at a time into a voxel grid, any camera ray-cast and a mesh extracted out of it ---
    @torch.no_grad()
    def integrate(self, views, volume=None, dims=None, origin=None, voxel=None, trunc=0.05, want=("shpd",), source="depth_map",
                  near=1e-3, complete_kw=None):
        """views: a list of (maps, pose) as fuse takes them - what __call__, run_big or run_any returned for one pair, and the pose
        of that pair's camera into the volume's frame (camera.pose; None: the identity) - integrated into a truncated signed
        distance volume -> the volume (volume.Volume, its sums on the GPU).  volume=None makes a new one from dims = (Nz, Ny, Nx),
        origin = (X0, Y0, Z0), voxel = (sX, sY, sZ) and trunc (native.tsdf_volume; metres; the camera sees 3 cm across at 1 m with
        centimetres of depth noise, so the voxels want to be much longer along Z than across); passing a volume adds to it, and
        its own `want` holds.  Samples, weights (conf) and the `want`ed maps out of native.FOLD_MAPS are taken exactly as fuse
        takes them, each view in the camera dcal.intrinsics(H, W) of its own size; source="complete" integrates
        complete(maps, **complete_kw)["depth_dense"] instead of depth_map.  Views may come one at a time, in any order and any
        grouping: the sums are the same bits.  raycast renders the result."""
        want = tuple(want)
        if source not in ("depth_map", "complete"):
            raise ValueError(f"integrate: source must be 'depth_map' or 'complete', got {source!r}")
        if complete_kw and source != "complete":
            raise ValueError(f"integrate: {sorted(complete_kw)} are keywords of complete; they need source='complete'")
        views = _view_pairs("integrate", views)
        if volume is not None:
            if dims is not None or origin is not None or voxel is not None:
                raise ValueError("integrate: pass either a volume or dims, origin and voxel, not both")
            want = tuple(volume.meta.get("want", want))
        elif dims is None or origin is None or voxel is None:
            raise ValueError("integrate: without a volume, dims = (Nz, Ny, Nx), origin = (X0, Y0, Z0) and voxel = (sX, sY, sZ) are needed")
        vs, layout = self._views("integrate", views, want, source=source, complete_kw=complete_kw)
        if volume is None:
            volume = native.tsdf_volume(dims, origin, voxel, trunc, C=sum(n for _, _, n in layout["channels"]), device=vs[0]["depth"].device)
            volume.meta.update(layout)
        elif "want" not in volume.meta:
            volume.meta.update(layout)
        return native.tsdf_integrate(volume, vs, near=near)

    @torch.no_grad()
    def raycast(self, volume, cam_dst=None, pose=None, size=None, z_range=None, step=None, normals=False, normals_kw=None):
        """volume: what integrate returned -> the camera cam_dst at `pose` (camera.pose: the camera's frame -> the volume's; None:
        the identity), size = (Ho, Wo), rendered out of it (native.tsdf_raycast): depth [Ho,Wo] along cam_dst's axis, valid,
        weight (the interpolated sum of conf) and the maps the volume was integrated with, with the channel counts fuse gives
        them; with normals=True also normal [3,Ho,Wo] and normal_valid (native.depth_normals on depth, **normals_kw).  +0 / False
        where no ray met a surface.  Defaults: the camera and size of the first view integrated, the identity pose, z_range = the
        extent of the volume's corners along the camera's axis under `pose`, step = trunc / 4 (at most 4096 samples: pass a
        narrower z_range or a longer step otherwise).  The rendered view is what register takes as a frame-to-model target."""
        meta = getattr(volume, "meta", None) or {}
        cam_dst = meta.get("camera") if cam_dst is None else cam_dst
        size = meta.get("size") if size is None else size
        if cam_dst is None or size is None:
            raise ValueError("raycast: this volume was not made by integrate: pass cam_dst and size")
        if z_range is None:
            import numpy as np
            from . import volume as volume_
            q = volume_.inverse_pose(pose).astype(np.float64)
            ends = [(o, o + (n - 1) * s) for o, s, n in zip(volume.origin, volume.voxel, volume.dims[::-1])]
            zs = [q[6] * x + q[7] * y + q[8] * z + q[11] for x in ends[0] for y in ends[1] for z in ends[2]]
            z_range = (max(min(zs), min(volume.voxel)), max(zs))
        out = native.tsdf_raycast(volume, cam_dst, pose, size, z_range, step=step, normals=normals, normals_kw=normals_kw)
        res = {k: out[k] for k in ("depth", "valid", "weight")}
        res.update(unpack_channels(out["feat"], meta.get("channels", ()), out["depth"].shape))
        if normals:
            res.update(normal=out["normal"], normal_valid=out["normal_valid"])
        return res

    @torch.no_grad()
    def extract_mesh(self, volume, min_weight=0.0, normals=True):
        """volume: what integrate returned -> the surface it holds as one triangle mesh in the volume's frame (native.tsdf_mesh:
        marching tetrahedra over the cells whose 8 voxels hold a sum of conf > min_weight): dict(vertices [V,3] = (X, Y, Z) in
        metres, faces [T,3] int32 into the vertices, wound so that their normals face free space (the cameras' side), weight [V]
        = the interpolated sum of conf, the maps the volume was integrated with as [channels,V] (shpd [3,V]), split as raycast
        splits them, and normal [V,3] / normal_valid [V] = the normalised gradient of the signed distance (None with
        normals=False)).  Vertices are shared between triangles; V == 0 is a legal result.  camera.pose moves the mesh into another
        frame; save_mesh writes it."""
        meta = getattr(volume, "meta", None) or {}
        out = native.tsdf_mesh(volume, min_weight=min_weight, normals=normals)
        res = {k: out[k] for k in ("vertices", "faces", "weight")}
        res.update(unpack_channels(out["feat"], meta.get("channels", ()), out["vertices"].shape[:1]))
        res.update(normal=out["normal"], normal_valid=out["normal_valid"])
        return res

    @torch.no_grad()
    def render_mesh(self, mesh, cam_dst=None, pose=None, size=None, want=("shpd",), cull="none", normals=True):
        """mesh: what extract_mesh returned (or any dict of vertices [V,3], faces [T,3] int32 and per-vertex maps on the GPU) -> the
        camera cam_dst at `pose` (camera.pose: the camera's frame -> the mesh's; None: the identity), size = (Ho, Wo), looking at
        it (native.raster_mesh: a z-buffered rasteriser, exact coverage on a 1/256 pixel lattice, perspective-correct
        interpolation, the nearest surface per pixel): depth [Ho,Wo] along cam_dst's axis, valid, face [Ho,Wo] int32 = the
        triangle each pixel sees (-1: none), weight (the interpolated sum of conf, None when the mesh has none), the `want`ed
        maps of the mesh named as extract_mesh names them (shpd [3,Ho,Wo]; any [.., V] map of the mesh may be asked for), and,
        with normals=True and a mesh that holds them, normal [3,Ho,Wo] in the camera's frame and normal_valid (None otherwise).
        +0 / -1 / False where nothing landed.  Defaults: the pipeline's own camera dcal.intrinsics(Ho, Wo) of the size asked
        for and the identity pose; size is needed.  Triangles that reach behind the camera are dropped whole, not clipped; cull =
        "back" keeps only the triangles that face the camera.  The result holds the keys register's destination view takes
        (depth, weight, normal): like raycast's, it is a frame-to-model target, from the mesh instead of the volume."""
        if size is None:
            raise ValueError("render_mesh: size = (Ho, Wo) is needed (a mesh does not remember a camera)")
        if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
            raise ValueError("render_mesh: mesh must be the dict extract_mesh returned (vertices, faces, ...)")
        want = (want,) if isinstance(want, str) else tuple(want)
        V = mesh["vertices"].shape[0]
        for k in want:
            t = mesh.get(k)
            if k in ("vertices", "faces", "weight", "normal", "normal_valid", "feat") or not isinstance(t, torch.Tensor) or t.shape[-1] != V:
                raise ValueError(f"render_mesh: want names the maps of the mesh with a last axis of {V} vertices; {k!r} is not one")
        feat, channels = pack_channels({k: mesh[k].to(torch.float32) for k in want}, want, V, tail=1)
        if cam_dst is None:
            try:
                cam_dst = self.dcal.intrinsics(*size)
            except TypeError:
                raise ValueError(f"render_mesh: size must be (Ho, Wo), got {size!r}") from None
        m = dict(vertices=mesh["vertices"], faces=mesh["faces"], weight=mesh.get("weight"), feat=feat,
                 normal=mesh.get("normal") if normals else None, normal_valid=mesh.get("normal_valid") if normals else None)
        out = native.raster_mesh(m, cam_dst, pose, size, cull=cull, want=("feat", "weight") + (("normal",) if normals else ()))
        res = {k: out[k] for k in ("depth", "valid", "face", "weight")}
        res.update(unpack_channels(out["feat"], channels, out["depth"].shape))
        res.update(normal=out["normal"], normal_valid=out["normal_valid"])
        return res

    @torch.no_grad()
    def clean_mesh(self, mesh, min_triangles=None, min_area=None, largest=False):
        """mesh: what extract_mesh returned (or any dict of vertices [V,3], faces [T,3] int32 and per-vertex maps on the GPU) -> the
        mesh without its small connected components (native.mesh_clean): a component - the vertices a chain of faces joins -
        stays when it holds at least min_triangles triangles and min_area square metres (None: not asked), and with largest=True
        only the one with the most triangles does.  The islands of triangles that depth outliers leave in front of a surface are
        such components; the surfaces themselves are the large ones.  The result holds the keys of `mesh` - vertices, faces
        (re-indexed), weight, normal, normal_valid and every [.., V] map such as shpd [3,V'] - and adds component [V'] int32 = the
        id each vertex's component had and components = dict(triangles, vertices, area_q, area, keep), one entry per component of
        the mesh that came in.  It goes straight into render_mesh, save_mesh and clean_mesh again.  One read-back."""
        if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
            raise ValueError("clean_mesh: mesh must be the dict extract_mesh returned (vertices, faces, ...)")
        V = mesh["vertices"].shape[0]
        fixed = ("vertices", "faces", "weight", "normal", "normal_valid", "edge", "component", "components", "vertex_index", "face_index", "cluster",
                 "members", "valence", "boundary", "displacement")           # what simplify_mesh and smooth_mesh add: they describe another mesh
        maps = [k for k, t in mesh.items() if k not in fixed and isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[-1] == V]
        for k in maps:
            if mesh[k].dtype != torch.float32:
                raise ValueError(f"clean_mesh: the map {k!r} must be float32, got {mesh[k].dtype}")
        feat, channels = pack_channels(mesh, maps, V, tail=1)
        m = dict(vertices=mesh["vertices"], faces=mesh["faces"], feat=feat, **{k: mesh.get(k) for k in ("weight", "normal", "normal_valid", "edge")})
        out = native.mesh_clean(m, min_triangles=min_triangles, min_area=min_area, largest=largest)
        res = {k: v for k, v in mesh.items() if k not in fixed and k not in maps}
        res.update({k: out[k] for k in ("vertices", "faces", "weight", "normal", "normal_valid", "edge") if k in mesh})
        res.update(unpack_channels(out["feat"], channels, out["vertices"].shape[:1]))
        res.update(component=out["component"], components=out["components"])
        return res

    @torch.no_grad()
    def simplify_mesh(self, mesh, cell, origin=(0, 0, 0), flaps=False):
        """mesh: what extract_mesh or clean_mesh returned (or any dict of vertices [V,3], faces [T,3] int32 and per-vertex maps on
        the GPU) -> the mesh made coarser by vertex clustering (native.mesh_simplify): every vertex falls into a cell of a regular
        grid - `cell` metres, one number or three (cX, cY, cZ), because the voxels are per axis too; `origin` a corner of cell
        (0, 0, 0) - and every occupied cell becomes one vertex at the weighted mean of its members, which also averages depth
        noise.  Faces are re-indexed; those that collapse or repeat are dropped, and with flaps=False so are the back-to-back
        pairs that name the same three cells in both windings.  The result holds the keys of `mesh` - vertices, faces, weight
        (the mean), normal (the normalised mean), normal_valid and every [.., V] map such as shpd [3,V'] (the weighted mean) - but
        edge, component, components, vertex_index, which do not survive, and adds cluster [V] int32 = the new id of every old
        vertex (-1: it took no part), members [V'] int32 and face_index [T'] int32 = the old position of every face that stayed.
        It goes straight into render_mesh, save_mesh, clean_mesh and simplify_mesh again.  Clean first: simplification keeps
        a floater's vertex while it thins the surface around it.  One read-back."""
        if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
            raise ValueError("simplify_mesh: mesh must be the dict extract_mesh returned (vertices, faces, ...)")
        V = mesh["vertices"].shape[0]
        fixed = ("vertices", "faces", "weight", "normal", "normal_valid", "edge", "component", "components", "vertex_index", "face_index", "cluster",
                 "members", "valence", "boundary", "displacement")
        maps = [k for k, t in mesh.items() if k not in fixed and isinstance(t, torch.Tensor) and t.dim() >= 1 and t.shape[-1] == V]
        for k in maps:
            if mesh[k].dtype != torch.float32:
                raise ValueError(f"simplify_mesh: the map {k!r} must be float32, got {mesh[k].dtype}")
        feat, channels = pack_channels(mesh, maps, V, tail=1)
        m = dict(vertices=mesh["vertices"], faces=mesh["faces"], feat=feat, **{k: mesh.get(k) for k in ("weight", "normal", "normal_valid")})
        out = native.mesh_simplify(m, cell, origin=origin, flaps=flaps)
        res = {k: v for k, v in mesh.items() if k not in fixed and k not in maps}
        res.update({k: out[k] for k in ("vertices", "faces", "weight", "normal", "normal_valid") if k in mesh})
        res.update(unpack_channels(out["feat"], channels, out["vertices"].shape[:1]))
        res.update(cluster=out["cluster"], members=out["members"], face_index=out["face_index"])
        return res

    @torch.no_grad()
    def smooth_mesh(self, mesh, iters=10, lam=0.5, mu=-0.53, boundary="fixed", normals="keep"):
        """mesh: what extract_mesh, clean_mesh or simplify_mesh returned (or any dict of vertices [V,3], faces [T,3] int32 and
        per-vertex maps on the GPU) -> the mesh denoised at its own resolution by Taubin smoothing (native.mesh_smooth): `iters`
        times every vertex steps towards the mean of its neighbours by `lam` and away from the new mean by `mu` (mu = 0: a plain
        Laplacian, which shrinks what it smooths).  No vertex or face is lost.  boundary="fixed" holds the vertices on the rim of
        the mesh - those that touch an edge only one face holds -, "free" moves them too.  normals="keep" leaves normal /
        normal_valid as they are - the volume's gradient is the better normal of a depth-noise mesh -, "recompute" replaces them
        by the area-weighted normals of the new faces (native.mesh_normals), "drop" sets both to None.  The result holds the keys
        of `mesh` with new vertices, but edge (a moved vertex has left its lattice edge), and adds valence [V] int32, boundary [V]
        bool and displacement [V] = how far each vertex moved, in metres.  It goes straight into render_mesh, save_mesh,
        clean_mesh, simplify_mesh and smooth_mesh again.  Clean first: smoothing drags a surface toward a floater that touches
        it.  The same bits on every run; no read-back."""
        if not isinstance(mesh, dict) or "vertices" not in mesh or "faces" not in mesh:
            raise ValueError("smooth_mesh: mesh must be the dict extract_mesh returned (vertices, faces, ...)")
        m = dict(vertices=mesh["vertices"], faces=mesh["faces"], normal=mesh.get("normal"), normal_valid=mesh.get("normal_valid"))
        out = native.mesh_smooth(m, iters=iters, lam=lam, mu=mu, boundary=boundary, normals=normals)
        res = {k: v for k, v in mesh.items() if k != "edge"}
        res["vertices"] = out["vertices"]
        if normals != "keep":
            res.update(normal=out["normal"], normal_valid=out["normal_valid"])
        res.update(valence=out["valence"], boundary=out["boundary"], displacement=out["displacement"])
        return res

    @staticmethod
    def save_mesh(path, mesh):
        """mesh: what extract_mesh returned -> a binary PLY file at `path` (mesh.write_ply): positions, normals when the mesh holds
        them, faces, and shpd as 8-bit vertex colours when the mesh holds it."""
        from . import mesh as mesh_
        host = lambda t: None if t is None else t.detach().cpu().numpy()
        shpd = mesh.get("shpd")
        mesh_.write_ply(path, dict(vertices=host(mesh["vertices"]), faces=host(mesh["faces"]), normal=host(mesh.get("normal"))),
                        colour=None if shpd is None else host(shpd).reshape(3, -1))


    # ---- registration: surface normals of a depth map, and the pose between two pairs from their depth ---------------------
    def _depth_view(self, who, maps, source, weights, complete_kw):
        """One pair as a view of native.register_depth: its depth (depth_map, or complete()'s dense depth), its weights and its
        camera dcal.intrinsics(H, W)."""
        if source not in ("depth_map", "complete"):
            raise ValueError(f"{who}: source must be 'depth_map' or 'complete', got {source!r}")
        if weights not in ("conf", None):
            raise ValueError(f"{who}: weights must be 'conf' or None, got {weights!r}")
        if not isinstance(maps, dict) or "grid" not in maps:
            raise ValueError(f"{who}: maps lacks ['grid']; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        if source == "complete":
            done = self.complete(maps, **complete_kw)
            z, measured, conf = done["depth_dense"], done["measured"], maps["conf"]
        else:
            if complete_kw:
                raise ValueError(f"{who}: {sorted(complete_kw)} are keywords of complete; they need source='complete'")
            src, _ = self._depth_samples(who, maps, 1, None, ("conf",) if weights else (), None)
            z, measured, conf = src["depth_map"], None, src.get("conf")
        w = None
        if weights == "conf":
            conf = conf.reshape(z.shape).to(torch.float32)
            w = conf if measured is None else torch.where(measured, conf, torch.ones_like(conf))
        g = maps["grid"]
        return dict(depth=z, weight=w, cam=self.dcal.intrinsics(g["H"], g["W"]), scale=1, window_origin=(0, 0))

    @torch.no_grad()
    def normals(self, maps, step=3, max_jump=0.05, source="depth_map", scale=1, window=None, depth_thres=None, **complete_kw):
        """maps: what __call__, run_big or run_any returned -> the surface normals of its depth: normal [3,Ho,Wo] = the unit normal
        (X, Y, Z) in the camera's frame, facing the camera, valid [Ho,Wo] (normal non-zero; on the device, no sync) and lattice.
        source="depth_map": the samples are those of point_cloud (render_at(scale, window, depth_thres) with their depth_map) -
        depth_map holds depth in a band along the boundaries only, and a normal needs a neighbour `step` samples away along x and
        along y, so most of the image stays invalid; source="complete": the depth is complete(maps, **complete_kw)["depth_dense"],
        normals everywhere, and scale must be 1 without a window.  step, max_jump: native.depth_normals - differences over `step`
        samples, and no difference across a depth step larger than max_jump * step metres."""
        if source == "complete":
            if scale != 1 or window is not None or depth_thres is not None:
                raise ValueError("normals: source='complete' works on the pixels: scale must be 1, window and depth_thres None")
            view = self._depth_view("normals", maps, source, None, complete_kw)
            g = maps["grid"]
            z, lat = view["depth"], tiling.lattice(g["H"], g["W"], 1, None)
        elif source == "depth_map":
            if complete_kw:
                raise ValueError(f"normals: {sorted(complete_kw)} are keywords of complete; they need source='complete'")
            src, lat = self._depth_samples("normals", maps, scale, window, (), depth_thres)
            z = src["depth_map"]
        else:
            raise ValueError(f"normals: source must be 'depth_map' or 'complete', got {source!r}")
        g = maps["grid"]
        out = native.depth_normals(z, self.dcal.intrinsics(g["H"], g["W"]), step=step, max_jump=max_jump, scale=lat["scale"],
                                   window_origin=lat["window"][:2])
        return dict(normal=out["normal"], valid=out["valid"], lattice=lat)

    @torch.no_grad()
    def register(self, maps_src, maps_dst, pose0=None, source="complete", weights="conf", complete_kw=None, **kw):
        """The pose of one pair's camera in another's frame, from their depth: point-to-plane ICP (native.register_depth) of
        maps_src's depth onto maps_dst's, each in the camera dcal.intrinsics(H, W) of its own size, from pose0 (None: the
        identity).  -> the dict of native.register_depth; its `pose` (X' = R X + t, source frame -> target frame) goes straight
        into fuse([(maps_dst, None), (maps_src, pose)]).  source="complete": both depths are complete(maps, **complete_kw) - dense,
        so that normals exist and samples meet; "depth_map": the thresholded depth as it is.  weights="conf": a sample weighs conf
        where it was measured and 1 where completion filled it; None: no weights.  kw: iters, damping, max_dist, huber, step,
        max_jump, near, tol of registration.register.  Each iteration synchronises with the host once (32 doubles).
        Conditioning: the pipeline's own camera is narrow (4709.9 px of focal length on 147 px: under 2 degrees of view), so
        rotations and in-plane translations are nearly interchangeable.  On a well-curved synthetic surface through such a camera
        the 6 x 6 system's condition number was 1.9e4; on a single plane, where translation in the plane and rotation about its
        normal are not observable at all, 2.6e8.  `cond` and `cov` are returned so that a caller can tell such cases apart: a
        near-singular system is reported, it is not an error."""
        complete_kw = dict(complete_kw or {})
        src = self._depth_view("register(maps_src)", maps_src, source, weights, complete_kw)
        dst = self._depth_view("register(maps_dst)", maps_dst, source, weights, complete_kw)
        return native.register_depth(src, dst, pose0, **kw)


    # ---- dense depth: the holes of depth_map closed by nearest-sample flood fill or by edge-aware diffusion -----------------
    @torch.no_grad()
    def complete(self, maps, smooth=2, sigma_z=0.02, method="nearest", edges=True, leak=1e-3, iters=None):
        """maps: what __call__, run_big or run_any returned (maps["depth_map"], maps["conf"] are read) -> a dense depth map.
        depth_map holds depth only where conf passes the threshold, a band on both sides of every boundary; the nearest sample of a
        hole therefore lies on the hole's own side of the nearest boundary, and every hole takes the depth of its nearest sample
        (native.fill_nearest: jump flooding, weights conf; smooth = r > 0 replaces a sample's depth by the conf-weighted robust mean
        of the samples within r of it, which averages their noise down; sigma_z in metres).  -> depth_dense [H,W] (depth_map itself
        wherever it is a finite number > 0 under conf > 0), measured [H,W] bool (those pixels), index [H,W] int32 (the sample's linear
        index y * W + x, the pixel's own where measured) and dist [H,W] float32 (pixels to that sample; -1, with index -1 and depth 0,
        when the pair has no sample at all).  Nothing synchronises with the host.  Under densify == 'pp' or 'w' depth_map is already
        dense: it is returned unchanged, every pixel measured.
        native.fill_nearest is general: with depth=out["depth"], weight=out["valid"] it also closes the holes of a reproject
        result - a separate call, because a disocclusion wants a rule that prefers the background, which this one is not.
        method="diffuse": the holes take the edge-aware harmonic interpolant of the same samples instead (native.fill_diffuse): a
        surface whose depth changes between two boundaries comes out as the smooth surface through both bands, where the nearest
        sample puts a step halfway.  edges=True passes maps["bndry"] as the edge map, which keeps two regions from mixing where the
        samples along a boundary are missing (leak: the conductance left across a full edge); iters: the sweeps per pyramid level,
        None for the default schedule.  The same keys (measured, index and dist are those of "nearest") plus residual [1]: the
        largest |average of the neighbours - value| left at a hole, 0 under densify 'pp' / 'w'."""
        if method not in ("nearest", "diffuse"):
            raise ValueError(f"complete: method must be 'nearest' or 'diffuse', got {method!r}")
        if not isinstance(maps, dict) or "depth_map" not in maps or "conf" not in maps:
            missing = [k for k in ("depth_map", "conf") if not isinstance(maps, dict) or k not in maps]
            raise ValueError(f"complete: maps lacks {missing}; pass the dict DepthPipeline.__call__, run_big or run_any returned")
        z, conf = maps["depth_map"], maps["conf"]
        for k, t in (("depth_map", z), ("conf", conf)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"complete: maps['{k}'] is not on the GPU; nothing here computes on the CPU "
                                 "(keep the dict the pipeline returned, or move it back to the device)")
        if z.dim() != 2 or conf.shape != z.shape:
            raise ValueError(f"complete: depth_map and conf must be [H,W], got {tuple(z.shape)} and {tuple(conf.shape)}")
        H, W = z.shape
        edge = None
        if method == "diffuse" and edges:
            edge = maps.get("bndry")
            if edge is None:
                raise ValueError("complete: maps lacks ['bndry'], the edge map of method='diffuse'; pass the dict DepthPipeline.__call__, "
                                 "run_big or run_any returned, or edges=False")
            if not isinstance(edge, torch.Tensor) or not edge.is_cuda:
                raise ValueError("complete: maps['bndry'] is not on the GPU; nothing here computes on the CPU "
                                 "(keep the dict the pipeline returned, or move it back to the device)")
            if edge.numel() != H * W or tuple(edge.shape[-2:]) != (H, W):
                raise ValueError(f"complete: bndry must be [..,{H},{W}] with leading dimensions of 1, got {tuple(edge.shape)}")
            edge = edge.reshape(H, W).to(torch.float32)
        if self.densify in ("pp", "w"):
            res = dict(depth_dense=z, measured=torch.ones_like(z, dtype=torch.bool),
                       index=torch.arange(H * W, dtype=torch.int32, device=z.device).view(H, W), dist=torch.zeros_like(z))
            if method == "diffuse":
                res["residual"] = torch.zeros(1, dtype=torch.float32, device=z.device)
            return res
        if method == "diffuse":
            out = native.fill_diffuse(z, conf, edge, smooth=smooth, sigma_z=sigma_z, leak=leak, iters=iters)
        else:
            out = native.fill_nearest(z, conf, smooth=smooth, sigma_z=sigma_z)
        d2 = out["dist2"]
        res = dict(depth_dense=out["depth"], measured=d2 == 0, index=out["index"],
                   dist=torch.where(d2 >= 0, d2.to(torch.float32).sqrt(), torch.full_like(z, -1.0)))
        if method == "diffuse":
            res["residual"] = out["residual"]
        return res


def pack_channels(src, want, N, tail=2):
    """The maps src[k] [*lead, *tail] for k in `want`, N samples in the `tail` last axes (2: a lattice [Hs,Ws]; 1: vertices [V]) ->
    (feat [C,N] - the maps flattened to channels and stacked in the order of want, None when want is empty -, channels =
    [(k, lead, n), ..]: what unpack_channels needs to split a result again, and what volume.meta["channels"] keeps)."""
    parts = [src[k].reshape(-1, N) for k in want]
    channels = [(k, tuple(src[k].shape[:-tail]), p.shape[0]) for k, p in zip(want, parts)]
    return (torch.cat(parts) if parts else None), channels


def unpack_channels(feat, channels, tail_shape):
    """feat [C, ..] as an entry returned it for pack_channels' feat, over samples of shape tail_shape -> {k: [*lead, *tail_shape]};
    {} when feat is None."""
    res, c = {}, 0
    for k, lead, n in channels if feat is not None else ():
        res[k] = feat[c:c + n].reshape(tuple(lead) + tuple(tail_shape))
        c += n
    return res


def _view_pairs(who, views):
    """views of fuse / integrate -> a list of at least one (maps, pose); the pairs themselves are unpacked by DepthPipeline._views."""
    views = native.view_list(who, views, "(maps, pose)")
    if not views:
        raise ValueError(f"{who}: views must hold at least one (maps, pose)")
    return views


def _points_on(points, device, who):
    """points: a tensor or array-like [...,2] of (y, x) -> float32, on `device` when one is given."""
    try:
        points = torch.as_tensor(points)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{who}: points must be a tensor or array-like [...,2] of (y, x) positions") from None
    if points.dim() < 1 or points.shape[-1] != 2 or points.numel() == 0 or points.is_complex():
        raise ValueError(f"{who}: points must be [...,2] (y, x) with at least one point, got shape {tuple(points.shape)}")
    return points.detach().to(device=device, dtype=torch.float32)
