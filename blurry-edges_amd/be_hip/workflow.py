"""The reference's driver scripts as functions + a small CLI, running on this package's HIP path and the reference's file
formats (argument names and defaults = utils/args.py of the reference):

    python -m be_hip.datagen      [...]        train_val_data_generator.py  (data set -> .npy files)
    python -m be_hip.workflow local_train      local_training.py:68-121     (ShapeDataset 'local' -> best_run_exp_local_stage.pth)
    python -m be_hip.workflow global_pre       global_data_pre_cal.py:52-69 (local stage over images -> params_src_*.npy)
    python -m be_hip.workflow global_train     global_training.py:168-224   (ShapeDataset 'global' -> best_run_exp_global_stage.pth)
    python -m be_hip.workflow eval [--big]     blurry_edges_test.py:102-176 / blurry_edges_test_big.py (TestDataset -> metrics)
    python -m be_hip.workflow eval --any       the same for image pairs of any size >= 147 x 147 (DepthPipeline.run_any)
    ... eval --refocus_stack K [--focus_range NEAR FAR] [--out_path DIR]   also write every pair's K-plane focal stack
    ... eval --render_scale K [--render_window T L H W] [--out_path DIR]   also write every pair's maps on a K times finer lattice
    ... eval --render_size HO WO [--out_path DIR]          also write every pair's maps resampled to HO x WO samples
    ... eval --sample_points FILE.npy [--out_path DIR]     also write every pair's maps at the [N,2] (y, x) positions of FILE
    ... eval --point_cloud [--out_path DIR]                also write every pair's depth map as points in space
    ... eval --reproject CAM.npz [--out_path DIR]          also write every pair's depth and colours as the camera of CAM sees them
    ... eval --fuse FILE.npz [--out_path DIR]              also merge every V consecutive pairs, with the poses of FILE, in one camera
                                                           (with tsdf_dims / tsdf_origin / tsdf_voxel in FILE: also in a TSDF volume)
                                                           (with tsdf_mesh > 0 beside them: also that volume's triangle mesh)
                                                           (with mesh_render > 0 beside them: also that mesh seen by view 0's camera)
                                                           (with mesh_min_triangles > 0 beside them: the mesh without its small components)
                                                           (with mesh_smooth > 0 beside them: the mesh smoothed by that many Taubin iterations)
                                                           (with mesh_cell beside them: the mesh simplified on cells of that size)
    ... eval --normals [--out_path DIR]                    also write every pair's surface normals (of its completed depth)
    ... eval --complete [--out_path DIR]                   also write and score every pair's depth map completed to a dense one
    ... eval --complete --complete_method diffuse          ... by edge-aware diffusion instead of the nearest sample's depth

Data parallel (BASELINE configs[4]): the two training commands run under torchrun, one process per GPU -
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m be_hip.workflow local_train ...
every rank keeps a replica, takes every world-th batch of the epoch, gradients are averaged over RCCL (be_hip.dp), rank 0 logs and
writes the checkpoints (the reference has no distributed code at all: this part is the build's own).

Checkpoints are `torch.save(model.state_dict())` files in the reference's key layout, so they are interchangeable with
the reference's.  Epoch loops, schedules (beta / gamma ramps, ReduceLROnPlateau with the growing patience), xavier
initialisation, clipping and AdamW settings follow the scripts cited above; the compute inside a step is the HIP path.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch


def _device(args):
    return torch.device(args.cuda if torch.cuda.is_available() else "cpu")


def _dist():
    """(rank, world, dist module or None) for a run started by torchrun (one process per GPU, configs[4]); a plain `python -m
    be_hip.workflow ...` is (0, 1, None).  Backend nccl (= RCCL); BE_DIST_BACKEND=gloo + BE_LOCAL_DEVICE=0 rehearse it on one GPU."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1, None
    import torch.distributed as dist
    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("BE_DIST_BACKEND", "nccl")
        lr = int(os.environ.get("BE_LOCAL_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        if torch.cuda.is_available():
            torch.cuda.set_device(lr)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", lr))
        else:
            dist.init_process_group(backend)
    return dist.get_rank(), dist.get_world_size(), dist


def _xavier_(model):
    for p in model.parameters():
        if p.dim() > 1:
            torch.nn.init.xavier_normal_(p)


def _log_header(f, args):
    print('Arguments:', file=f, flush=True)
    for k in vars(args):
        print(f'{k:<20}: {getattr(args, k)}', file=f, flush=True)
    print('\nTraining:', file=f, flush=True)
    print(f'{"Epoch":<10} {"Loss":<20} {"Scheduler patience":<20} {"Learning rate"}', file=f, flush=True)


# ---------------------------------------------------------------------------------------------- local_training.py
def local_train(args, quiet=False, graph=True):
    """graph: replay the training step as a hipGraph (train_local.GraphedStep); batches are gathered on the device
    (data.ShapeDataset.batches) instead of sample by sample."""
    import data, models, utils
    from . import dp
    from .train_local import BetaSchedule, GraphedStep, train_step
    rank, world, dist = _dist()
    utils.set_seed(1869)
    if rank == 0:
        utils.create_directory(args.log_path, overwrite=False)
        os.makedirs(args.model_path, exist_ok=True)
    if dist is not None:
        dist.barrier()
    dev = _device(args) if world == 1 else torch.device("cuda", torch.cuda.current_device())
    tr = data.ShapeDataset(dev, data_path=args.data_path, train=True)
    va = data.ShapeDataset(dev, data_path=args.data_path, train=False)
    model = models.LocalStage().to(dev)
    _xavier_(model)
    # data parallel (configs[4]): every rank keeps a replica, takes every world-th batch of the epoch's (identically shuffled)
    # batch sequence - a global batch of batch_size x world - and the gradients are averaged by the bucketed all-reduce (four buckets) that
    # overlaps the backward (be_hip.dp.GradSync).  graph=True: the step is six hipGraph segments with the RCCL calls between
    # them (train_local.SegmentedGraphStep); one GPU: one hipGraph (GraphedStep)
    sync = dp.GradSync(world) if world > 1 else None
    if world > 1:
        dp.broadcast_parameters(model, src=0)
    from .optim import ClipAdamW
    opt = ClipAdamW(model.parameters(), lr=args.learning_rate)   # AdamW defaults of local_training.py:86, fused with the clipping
    helper = utils.PostProcessLocalBase(args, dev)
    if not graph:
        gstep = None
    elif world > 1:
        from .train_local import SegmentedGraphStep
        gstep = SegmentedGraphStep(model, helper, opt, sync, world=world)
    else:
        gstep = GraphedStep(model, helper, opt)
    sampler = torch.Generator().manual_seed(1869)
    beta = BetaSchedule(args.beta_bndry_loc, args.beta_smthns, args.dynamic_epoch)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', factor=0.9, patience=2, min_lr=args.learning_rate * 0.1)
    curve = np.zeros((args.epoch_num,), dtype=float)
    best, best_epoch = np.inf, 0
    with open(f'{args.log_path}/exp_local_stage_training.txt' if rank == 0 else os.devnull, 'wt') as f:
        _log_header(f, args)
        for epoch in range(args.epoch_num):
            beta.step()
            model.train()
            # every rank takes the same number of steps (collectives pair up) and gathers only its own batches
            for img_ny, img_gt, bndry_dist, deri in tr.batches(args.batch_size, shuffle=True, drop_last=True, generator=sampler,
                                                               rank=rank, world=world):
                b = dict(img_ny=img_ny, img_gt=img_gt, bndry_dist=bndry_dist, deri=deri)
                if gstep is not None:
                    gstep(b, beta.beta_b, beta.beta_s)
                else:
                    train_step(model, helper, opt, b, beta.beta_b, beta.beta_s, world=world, sync=sync)
            if world > 1:
                # BatchNorm statistics are per replica during the epoch; rank 0's go to everyone before validation, so that every
                # rank sees the same validation loss (same lr schedule everywhere) and the checkpoint is what was validated
                dp.broadcast_bn_stats(model, src=0)
            # validation with the final betas (local_training.py:54-66)
            model.eval()
            total = 0.0
            with torch.no_grad():
                for img_ny, img_gt, bndry_dist, deri in va.batches(args.batch_size, shuffle=False, drop_last=True):
                    est = model(img_ny.permute(0, 3, 1, 2).contiguous())
                    total += float(utils.local_loss(helper, est, img_ny, img_gt, bndry_dist, deri, args.beta_bndry_loc,
                                                    args.beta_smthns))
            curve[epoch] = total / max(len(va) // args.batch_size, 1)
            sched.step(curve[epoch])
            sched.patience = 2 + int(np.log2(epoch + 1)) * 3
            print(f'{epoch + 1:<10} {curve[epoch]:<20.10f} {sched.patience:<20} {opt.param_groups[0]["lr"]:.4e}', file=f, flush=True)
            if curve[epoch] < best:
                best, best_epoch = curve[epoch], epoch
                if rank == 0:
                    torch.save(model.state_dict(), f'{args.model_path}/best_run_exp_local_stage.pth')
            if not quiet and rank == 0:
                print(f'epoch {epoch + 1}: validation loss {curve[epoch]:.6f}')
        print(f'\n-- Best epoch is the {best_epoch + 1:d}th, with average loss of {best:.10f}', file=f, flush=True)
    if rank == 0:
        np.save(f'{args.log_path}/loss_curve_exp_local_stage.npy', curve)
        utils.showCurve(args, curve, 'loss_curve_exp_local_stage')
    if dist is not None:
        dist.barrier()
    return curve


# ------------------------------------------------------------------------------------------- global_data_pre_cal.py
@torch.no_grad()
def global_pre(args, local_weights=None, quiet=False):
    """params_src_{train,val}.npy [n, 2, P, 19] float64: the normalised local-stage output + colours of every image."""
    import data, models, utils
    from . import native
    from .pipeline import DepthPipeline, params_src_layout
    dev = _device(args)
    model = models.LocalStage().to(dev)
    model.load_state_dict(torch.load(local_weights or f'{args.model_path}/pretrained_local_stage.pth', map_location=dev))
    model.eval()
    pipe = DepthPipeline(model, None, utils.PostProcessGlobalBase(args, dev), None, stride=args.stride)
    for part, train in (("train", True), ("val", False)):
        ds = data.ShapeDataset(dev, data_path=args.data_path, train=train, mode='global_pre')
        out = None
        for j in range(len(ds)):
            img = ds[j].permute(0, 3, 1, 2).contiguous()                     # [2,3,H,W]
            pm = pipe.local_pass(img)[3]                                      # [P,38] = [P, (aperture, 19)]
            if out is None:
                out = np.zeros((len(ds), 2, pm.shape[0], 19), dtype=np.float64)
            out[j] = params_src_layout(pm).cpu().numpy()
        np.save(f'{args.data_path}/params_src_{part}.npy', out)
        if not quiet:
            print(f'{part}: {len(ds)} images -> params_src_{part}.npy')


# ------------------------------------------------------------------------------------------------ global_training.py
def global_train(args, quiet=False):
    import data, models, utils
    from . import dp
    from .train_global import GammaSchedule, train_step
    rank, world, dist = _dist()
    utils.set_seed(1898)
    if rank == 0:
        utils.create_directory(args.log_path, overwrite=False)
        os.makedirs(args.model_path, exist_ok=True)
    if dist is not None:
        dist.barrier()
    dev = _device(args) if world == 1 else torch.device("cuda", torch.cuda.current_device())
    tr = data.ShapeDataset(dev, data_path=args.data_path, train=True, mode='global')
    va = data.ShapeDataset(dev, data_path=args.data_path, train=False, mode='global')
    sampler = torch.Generator().manual_seed(1898)
    model = models.GlobalStage(in_parameter_size=args.input_size, out_parameter_size=args.output_size, device=dev).to(dev)
    _xavier_(model)
    # data parallel: replicas aligned with rank 0, every world-th batch per rank, ONE all-reduce of the 4.27 MB gradient per step
    flat = dp.flat_grad_buffer(model.parameters()) if world > 1 else None
    if world > 1:
        dp.broadcast_parameters(model, src=0)
        for p_ in model.parameters():
            p_.grad = None
        # every rank seeds torch identically (same shuffle, same initial weights); the dropout masks must NOT be identical across
        # the replicas of one global batch, so each rank salts the seed GlobalStage draws per step
        model.dropout_seed_salt = (rank * 0x9E3779B1) & 0x7FFFFFFF
    from .optim import ClipAdamW
    opt = ClipAdamW(model.parameters(), lr=args.learning_rate, gather=True)      # AdamW defaults of global_training.py:196, fused with the clipping
    helper = utils.PostProcessGlobalBase(args, dev)
    dcal = utils.DepthEtas(args, dev)
    gamma = GammaSchedule(args)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, 'min', factor=0.975, patience=5, min_lr=args.learning_rate * 0.5)
    curve = np.zeros((args.epoch_num,), dtype=float)
    best, best_epoch = np.inf, 0
    feats = lambda p: p.permute(0, 2, 1, 3).flatten(2, 3).contiguous()          # [B,2,P,19] -> [B,P,38]
    # --resume (not in the reference): everything the loop carries from one epoch to the next is in {model_path}/global_resume.ckpt -
    # weights, AdamW moments, both schedules, the shuffling generator and torch's RNG (the dropout seeds come from it), the curve and
    # the best checkpoint - so a resumed run takes exactly the steps the uninterrupted one would have taken
    resume_path = f'{args.model_path}/global_resume.ckpt'
    first_epoch = 0
    resumed = bool(getattr(args, "resume", False)) and os.path.exists(resume_path)
    if resumed:
        ck = torch.load(resume_path, map_location=dev, weights_only=False)
        model.load_state_dict(ck["model"])
        opt.load_state_dict(ck["opt"])
        sched.load_state_dict(ck["sched"])
        gamma.idx = ck["gamma_idx"]
        sampler.set_state(ck["sampler"].cpu())                       # generator states are CPU byte tensors (map_location moved them)
        torch.set_rng_state(ck["torch_rng"].cpu())
        first_epoch, best, best_epoch = ck["epoch"], ck["best"], ck["best_epoch"]
        curve[:first_epoch] = ck["curve"][:first_epoch]
        if rank == 0 and ck.get("best_model") is not None:
            torch.save(ck["best_model"], f'{args.model_path}/best_run_exp_global_stage.pth')
    t_start = time.perf_counter()
    budget = float(getattr(args, "time_budget", 0.0) or 0.0)
    stopped_early = False
    with open(f'{args.log_path}/exp_global_stage_training.txt' if rank == 0 else os.devnull, 'at' if resumed else 'wt') as f:
        if not resumed:
            _log_header(f, args)
        for epoch in range(first_epoch, args.epoch_num):
            g = gamma.step()
            model.train()
            for param, _, img_gt, bndry_dist, deri, bndry_depth in tr.batches(args.batch_size, shuffle=True, drop_last=True,
                                                                             generator=sampler, rank=rank, world=world):
                train_step(model, helper, dcal, opt, dict(pm=feats(param), img_gt=img_gt, bndry_dist=bndry_dist, deri=deri,
                                                          bndry_depth=bndry_depth), g, flat=flat, world=world)
            model.eval()
            total, gf = 0.0, gamma.final()
            with torch.no_grad():
                for param, img_ny, img_gt, bndry_dist, deri, bndry_depth in va.batches(args.batch_size, shuffle=False, drop_last=True):
                    est = model(feats(param))
                    total += float(utils.global_loss(helper, dcal, est, img_ny, img_gt, bndry_dist, deri, bndry_depth, gf, empty_mask="zero"))
            gamma.step(idx_update=False)
            curve[epoch] = total / max(len(va) // args.batch_size, 1)
            print(f'{epoch + 1:<10} {curve[epoch]:<20.10f} {sched.patience:<20} {opt.param_groups[0]["lr"]:.4e}', file=f, flush=True)
            if curve[epoch] < best:
                best, best_epoch = curve[epoch], epoch
                if rank == 0:
                    torch.save(model.state_dict(), f'{args.model_path}/best_run_exp_global_stage.pth')
            if epoch >= args.dynamic_epoch[1]:
                sched.step(curve[epoch])
            if not quiet and rank == 0:
                print(f'epoch {epoch + 1}: validation loss {curve[epoch]:.6f}', flush=True)
            if rank == 0 and (getattr(args, "resume", False) or budget > 0):
                bm = f'{args.model_path}/best_run_exp_global_stage.pth'
                torch.save(dict(model=model.state_dict(), opt=opt.state_dict(), sched=sched.state_dict(), gamma_idx=gamma.idx,
                                sampler=sampler.get_state(), torch_rng=torch.get_rng_state(), epoch=epoch + 1, best=best,
                                best_epoch=best_epoch, curve=curve.copy(),
                                best_model=torch.load(bm, map_location="cpu") if os.path.exists(bm) else None), resume_path + ".tmp")
                os.replace(resume_path + ".tmp", resume_path)
            if budget > 0 and epoch + 1 < args.epoch_num:
                stopped_early = time.perf_counter() - t_start > budget
                if dist is not None:                                   # rank 0's clock decides for everyone (collectives pair up)
                    flag = torch.tensor([int(stopped_early)], device=dev if dist.get_backend() == "nccl" else "cpu")
                    dist.broadcast(flag, 0)
                    stopped_early = bool(flag.item())
                if stopped_early:
                    if rank == 0:
                        print(f'-- time budget reached after epoch {epoch + 1} of {args.epoch_num}: continue with --resume', flush=True)
                    break
        if not stopped_early:
            print(f'\n-- Best epoch is the {best_epoch + 1:d}th, with average loss of {best:.10f}.', file=f, flush=True)
    if rank == 0:
        np.save(f'{args.log_path}/loss_curve_exp_global_stage.npy', curve)
        utils.showCurve(args, curve, 'loss_curve_exp_global_stage')
    if dist is not None:
        dist.barrier()
    return curve


# ------------------------------------------------------------------------- blurry_edges_test.py / blurry_edges_test_big.py
def focus_sweep(dcal, k, near, far):
    """The optical powers of `eval --refocus_stack k --focus_range near far`: k values evenly spaced in dioptres (= evenly spaced in
    blur radius) from focus2rho(far) up to focus2rho(near), float64 [k]; k = 1 focuses at `far`."""
    if k < 1:
        raise ValueError(f"--refocus_stack: the number of planes must be >= 1, got {k}")
    if not 0 < near < far:
        raise ValueError(f"--focus_range: expected 0 < NEAR < FAR (metres), got {near} {far}")
    return np.linspace(dcal.focus2rho(far), dcal.focus2rho(near), k)


def _npz_size(who, f):
    """size = (Ho, Wo) out of a settings .npz -> two ints >= 1 (the entry that takes them states its own upper bound)."""
    size = np.asarray(f["size"]).reshape(-1)
    if size.shape != (2,) or not all(int(v) == v and v >= 1 for v in size):
        raise ValueError(f"{who}: size must be (Ho, Wo), integers >= 1, got {f['size']!r}")
    return int(size[0]), int(size[1])


def load_camera(path):
    """The settings file of `eval --reproject`: an .npz holding K ([4] = fy, fx, cy, cx, or [3,3]), R [3,3] and t [3] (the pose from
    the depth camera's frame to this camera's; absent: the identity, zero), size = (Ho, Wo) and optionally scale (the source
    lattice, default 1) -> dict(cam, pose, size, scale), checked by be_hip.camera."""
    from . import camera
    with np.load(path) as f:
        missing = [k for k in ("K", "size") if k not in f]
        if missing:
            raise ValueError(f"--reproject: {path} lacks {missing}; it must hold K, size and optionally R, t, scale")
        size = _npz_size("--reproject", f)
        scale = int(np.asarray(f["scale"]).reshape(-1)[0]) if "scale" in f else 1
        return dict(cam=camera.as_pinhole(f["K"], "--reproject(K)"),
                    pose=camera.pose(f["R"] if "R" in f else None, f["t"] if "t" in f else None),
                    size=size, scale=scale)


def load_fusion(path):
    """The settings file of `eval --fuse`: an .npz holding poses [V,12], [V,3,4] or [V,4,4] (pair i of a group -> the target frame,
    1 <= V <= 32) and optionally K ([4] = fy, fx, cy, cx, or [3,3]) and size = (Ho, Wo) of the target camera (absent: the first
    pair's), tau, min_views, peel, recentre and scale (the source lattice) -> dict(poses, cam, size, scale, kw = the keywords of
    DepthPipeline.fuse that the file sets), checked by be_hip.camera; tau, min_views and peel by native.fuse_views.  An optional
    integer `register` > 0 (-> cfg["register"]) asks for every view's pose to be refined against view 0 by that many iterations of
    DepthPipeline.register, starting from the pose given, before the group is merged.  tsdf_dims, tsdf_origin, tsdf_voxel (and
    optionally tsdf_trunc) describe a TSDF volume (-> cfg["tsdf"]); an integer tsdf_mesh > 0 beside them (-> cfg["tsdf_mesh"]) asks
    for that volume's mesh as well, and an integer mesh_render > 0 (-> cfg["mesh_render"]) for that mesh rendered into view 0's
    camera.  mesh_cell = one number or three (cX, cY, cZ) > 0, in metres (-> cfg["mesh_cell"], three numbers), asks for that mesh
    simplified on cells of that size.  An integer mesh_smooth > 0 (-> cfg["mesh_smooth"]) asks for that mesh smoothed by that many
    iterations of DepthPipeline.smooth_mesh at its defaults, after the cleaning and before the simplification."""
    from . import camera
    with np.load(path) as f:
        if "poses" not in f:
            raise ValueError(f"--fuse: {path} lacks ['poses']; it must hold poses [V,..] and optionally K, size, tau, min_views, peel, "
                             "recentre, scale")
        P = np.asarray(f["poses"], np.float64)
        if P.ndim < 2 or not 1 <= P.shape[0] <= 32 or tuple(P.shape[1:]) not in ((12,), (3, 4), (4, 4)):
            raise ValueError(f"--fuse: poses must be [V,12], [V,3,4] or [V,4,4] with 1 <= V <= 32, got {P.shape}")
        poses = [camera.as_pose(p, f"--fuse(poses[{i}])") for i, p in enumerate(P)]
        size = _npz_size("--fuse", f) if "size" in f else None
        one = lambda k, t: t(np.asarray(f[k]).reshape(-1)[0])
        kw = {k: one(k, t) for k, t in (("tau", float), ("min_views", int), ("peel", int), ("recentre", bool)) if k in f}
        cfg = dict(poses=poses, cam=camera.as_pinhole(f["K"], "--fuse(K)") if "K" in f else None, size=size,
                   scale=one("scale", int) if "scale" in f else 1, kw=kw)
        if "register" in f:                                                 # absent: the dict holds what it held before
            n = np.asarray(f["register"]).reshape(-1)[0]
            if int(n) != n or not 0 <= n <= 1000:
                raise ValueError(f"--fuse: register must be an integer number of iterations in [0, 1000], got {f['register']!r}")
            cfg["register"] = int(n)
        if any(k in f for k in ("tsdf_dims", "tsdf_origin", "tsdf_voxel", "tsdf_trunc")):   # absent: the dict holds what it held before
            from . import volume
            missing = [k for k in ("tsdf_dims", "tsdf_origin", "tsdf_voxel") if k not in f]
            if missing:
                raise ValueError(f"--fuse: a TSDF volume needs tsdf_dims = (Nz, Ny, Nx), tsdf_origin = (X0, Y0, Z0) and tsdf_voxel = "
                                 f"(sX, sY, sZ) (tsdf_trunc is optional: 0.05); {path} lacks {missing}")
            dims, origin, voxel, trunc, _ = volume.check_params("--fuse(tsdf)", np.asarray(f["tsdf_dims"]).reshape(-1).tolist(),
                                                                np.asarray(f["tsdf_origin"]).reshape(-1).tolist(),
                                                                np.asarray(f["tsdf_voxel"]).reshape(-1).tolist(),
                                                                one("tsdf_trunc", float) if "tsdf_trunc" in f else 0.05)
            cfg["tsdf"] = dict(dims=dims, origin=origin, voxel=voxel, trunc=trunc)
        if "tsdf_mesh" in f:                                                # absent: the dict holds what it held before
            n = np.asarray(f["tsdf_mesh"]).reshape(-1)[0]
            if int(n) != n or n < 0:
                raise ValueError(f"--fuse: tsdf_mesh must be an integer >= 0 (> 0: also write the volume's mesh), got {f['tsdf_mesh']!r}")
            if n > 0 and "tsdf" not in cfg:
                raise ValueError(f"--fuse: tsdf_mesh extracts the mesh of the TSDF volume; {path} lacks the keys that describe one: "
                                 "tsdf_dims, tsdf_origin, tsdf_voxel (tsdf_trunc is optional)")
            cfg["tsdf_mesh"] = int(n)
        if "mesh_render" in f:                                              # absent: the dict holds what it held before
            n = np.asarray(f["mesh_render"]).reshape(-1)[0]
            if int(n) != n or n < 0:
                raise ValueError(f"--fuse: mesh_render must be an integer >= 0 (> 0: also render the volume's mesh), got {f['mesh_render']!r}")
            if n > 0 and "tsdf" not in cfg:
                raise ValueError(f"--fuse: mesh_render renders the mesh of the TSDF volume; {path} lacks the keys that describe one: "
                                 "tsdf_dims, tsdf_origin, tsdf_voxel (tsdf_trunc is optional)")
            cfg["mesh_render"] = int(n)
        if "mesh_min_triangles" in f:                                       # absent: the dict holds what it held before
            n = np.asarray(f["mesh_min_triangles"]).reshape(-1)[0]
            if int(n) != n or not 0 <= n < 1 << 31:
                raise ValueError("--fuse: mesh_min_triangles must be an integer >= 0 (> 0: drop the mesh's components of fewer triangles), "
                                 f"got {f['mesh_min_triangles']!r}")
            if n > 0 and not (cfg.get("tsdf_mesh", 0) > 0 or cfg.get("mesh_render", 0) > 0):
                raise ValueError(f"--fuse: mesh_min_triangles cleans the mesh of the TSDF volume; {path} asks for no mesh: "
                                 "tsdf_mesh > 0 or mesh_render > 0 (beside tsdf_dims, tsdf_origin, tsdf_voxel)")
            cfg["mesh_min_triangles"] = int(n)
        if "mesh_cell" in f:                                                # absent: the dict holds what it held before
            from . import simplify
            try:
                cell = simplify.grid(np.asarray(f["mesh_cell"]).reshape(-1).tolist(), who="--fuse(mesh_cell)")[0]
            except ValueError:
                raise ValueError("--fuse: mesh_cell must be one number or three (cX, cY, cZ) > 0, in metres (the cells the mesh's vertices are "
                                 f"clustered in), got {f['mesh_cell']!r}") from None
            if not (cfg.get("tsdf_mesh", 0) > 0 or cfg.get("mesh_render", 0) > 0):
                raise ValueError(f"--fuse: mesh_cell simplifies the mesh of the TSDF volume; {path} asks for no mesh: "
                                 "tsdf_mesh > 0 or mesh_render > 0 (beside tsdf_dims, tsdf_origin, tsdf_voxel)")
            cfg["mesh_cell"] = tuple(float(c) for c in cell)
        if "mesh_smooth" in f:                                              # absent: the dict holds what it held before
            n = np.asarray(f["mesh_smooth"]).reshape(-1)[0]
            if int(n) != n or not 0 <= n <= 10000:
                raise ValueError("--fuse: mesh_smooth must be an integer in [0, 10000] (> 0: that many iterations of Taubin smoothing on the "
                                 f"mesh's vertices), got {f['mesh_smooth']!r}")
            if n > 0 and not (cfg.get("tsdf_mesh", 0) > 0 or cfg.get("mesh_render", 0) > 0):
                raise ValueError(f"--fuse: mesh_smooth smooths the mesh of the TSDF volume; {path} asks for no mesh: "
                                 "tsdf_mesh > 0 or mesh_render > 0 (beside tsdf_dims, tsdf_origin, tsdf_voxel)")
            cfg["mesh_smooth"] = int(n)
        return cfg


def refine_poses(pipe, group, poses, iters):
    """The poses of `eval --fuse` with `register` > 0: view 0 keeps its pose T0; view v's pose Tv (its frame -> the target frame)
    gives the start inv(T0) Tv of DepthPipeline.register(view v, view 0), and the refined relative pose P comes back as T0 P.
    -> (poses [V] as 12 float32 numbers, rms [V] = the last rms of each registration, 0 for view 0)."""
    from . import camera
    mat = lambda p: np.vstack([np.concatenate([np.asarray(p, np.float64)[:9].reshape(3, 3), np.asarray(p, np.float64)[9:, None]], 1), [0, 0, 0, 1]])
    T0 = mat(poses[0])
    out, rms = [np.asarray(poses[0], np.float32)], [0.0]
    for maps, p in zip(group[1:], poses[1:]):
        res = pipe.register(maps, group[0], pose0=np.linalg.inv(T0) @ mat(p), iters=iters)
        out.append(camera.pose(T0 @ mat(res["pose"])))
        rms.append(float(res["rms"][-1]) if len(res["rms"]) else float("nan"))
    return out, rms


@torch.no_grad()
def evaluate(args, big=False, local_weights=None, global_weights=None, pp_weights=None, quiet=False, any_size=False):
    """-> dict(delta1, delta2, delta3, RMSE, AbsRel, seconds_per_pair), averaged over the test set as the scripts do.
    any_size: pairs of any size >= 147 x 147 through DepthPipeline.run_any (checkpoint names and arguments as big).
    args.refocus_stack = K > 0 (not in the reference): every pair's focal stack over args.focus_range goes to
    {args.out_path}/refoc_stack_{j:04d}.npy ([K,3,H,W] float32) and the powers to rho_primes.npy, outside the timed region.
    args.render_scale = k > 1 (not in the reference; 1 = off): every pair's maps on the k times finer lattice of
    DepthPipeline.render_at, over args.render_window (top left h w; default the whole image), go to
    {args.out_path}/render_x{k}_{j:04d}.npz (shpd, refoc, bndry, depth, conf and - unless --densify pp - depth_map, float32; depth_map
    with the threshold of the mode: 0.05 under --big / --any), outside the timed region; a focal stack asked for in the same run
    is written on the same lattice.
    args.render_size = (HO, WO) (not in the reference): every pair's maps resampled to HO x WO samples, DepthPipeline.render_resized,
    go to {args.out_path}/render_{HO}x{WO}_{j:04d}.npz (the arrays of --render_scale); args.sample_points = an .npy file holding an
    [N,2] array of (y, x) positions: the same maps at those positions, DepthPipeline.sample_at, and `valid` go to
    {args.out_path}/samples_{j:04d}.npz.  Both outside the timed region.
    args.point_cloud (not in the reference): every pair's depth_map as points in the camera's frame, DepthPipeline.point_cloud, goes
    to {args.out_path}/cloud_{j:04d}.npz (xyz [3,H,W], valid, shpd, conf); args.reproject = an .npz file of settings (load_camera: K,
    R, t, size, optional scale): the pair forward-warped to that camera, DepthPipeline.reproject, goes to
    {args.out_path}/reproj_{j:04d}.npz (depth, valid, index, shpd, refoc at `size`).  Both outside the timed region, with the
    depth threshold of the mode.
    args.complete (not in the reference): every pair's depth_map completed to a dense one, DepthPipeline.complete, goes to
    {args.out_path}/complete_{j:04d}.npz (depth_dense, measured, index, dist), outside the timed region; one more metrics line per
    pair and in the average scores depth_dense with the same utils.eval_depth call, and the averages are returned under the key
    `dense`.  Without the flag, output and return value are what they were.  args.complete_method 'diffuse' completes by edge-aware
    diffusion (DepthPipeline.complete(method="diffuse")): the npz also holds `residual`, and the lines read "(completed, diffuse)".
    args.fuse = an .npz file of settings (load_fusion: poses [V,..], optional K, size, tau, min_views, peel, recentre, scale; not in
    the reference): every V consecutive pairs of the test set are one group whose pair i has pose i; the group merged in one camera,
    DepthPipeline.fuse, goes to {args.out_path}/fused_{g:04d}.npz (depth, valid, weight, views, count, layer, shpd), outside the
    timed region; a remainder of fewer than V pairs is skipped, with a printed note.  With an integer `register` > 0 in the settings
    file every view's pose is first refined against view 0 (refine_poses, that many iterations of DepthPipeline.register), and the
    npz also holds poses_refined [V,12] and register_rms [V]; without the key the file holds what it held before.  With tsdf_dims
    = (Nz, Ny, Nx), tsdf_origin = (X0, Y0, Z0) and tsdf_voxel = (sX, sY, sZ) (and optionally tsdf_trunc, 0.05) in the settings file
    each group is also integrated into a TSDF volume of that description, DepthPipeline.integrate, and ray-cast into view 0's
    camera, DepthPipeline.raycast: {args.out_path}/tsdf_{g:04d}.npz (depth, valid, weight, normal, shpd), outside the timed region.
    With an integer tsdf_mesh > 0 beside them the volume's surface is also extracted, DepthPipeline.extract_mesh, in the frame of the
    poses: {args.out_path}/mesh_{g:04d}.ply (positions, normals, shpd as colours) and mesh_{g:04d}.npz (vertices, faces, weight, shpd,
    normal, normal_valid), outside the timed region.  With an integer mesh_render > 0 beside them that mesh is also rasterised into
    view 0's camera, DepthPipeline.render_mesh: {args.out_path}/mesh_render_{g:04d}.npz (depth, valid, face, normal, shpd), outside
    the timed region; without the key nothing changes.  With an integer mesh_min_triangles > 0 beside them the mesh is first cleaned,
    DepthPipeline.clean_mesh: its connected components of fewer triangles - the islands depth outliers leave - are dropped before
    either file is written, and mesh_{g:04d}.npz also holds component [V'] and components_triangles (every component's size).
    With an integer mesh_smooth > 0 beside them the mesh is then smoothed, DepthPipeline.smooth_mesh with that many iterations at its
    defaults - after the cleaning, because smoothing drags a surface toward a floater that touches it, and before the
    simplification -, and mesh_{g:04d}.npz also holds valence, boundary and displacement (unless mesh_cell follows).
    With mesh_cell = one number or three (cX, cY, cZ) > 0, in metres, beside them the mesh is then simplified,
    DepthPipeline.simplify_mesh on the grid of such cells from the volume's origin - after the cleaning, because clustering keeps a
    floater's vertex while it thins the surface around it - before either file is written, and mesh_{g:04d}.npz holds the coarser
    mesh with cluster, members and face_index (and no component: its ids name the mesh before).
    args.normals (not in the reference): every pair's surface normals, DepthPipeline.normals(source="complete"), go to
    {args.out_path}/normals_{j:04d}.npz (normal [3,H,W], valid), outside the timed region."""
    import data, models, utils
    from .pipeline import DepthPipeline
    dev = _device(args)
    load = lambda m, path: (m.load_state_dict(torch.load(path, map_location=dev)), m.eval())[1]
    local = load(models.LocalStage().to(dev), local_weights or f'{args.model_path}/pretrained_local_stage.pth')
    # blurry_edges_test.py:187-190 loads pretrained_global_stage_w.pth for `--densify w`; the big-image script
    # (blurry_edges_test_big.py) always loads the plain name
    gname = 'pretrained_global_stage_w.pth' if (args.densify == 'w' and not (big or any_size)) else 'pretrained_global_stage.pth'
    globl = load(models.GlobalStage(in_parameter_size=38, out_parameter_size=12, device=dev).to(dev),
                 global_weights or f'{args.model_path}/{gname}')
    pp = None
    if args.densify == 'pp':
        pp = load(models.DepthCompletion().to(dev), pp_weights or f'{args.model_path}/pretrained_depth_completion_pp.pth')
    pipe = DepthPipeline(local, globl, utils.PostProcessGlobalBase(args, dev), utils.DepthEtas(args, dev),
                         rho_prime=args.rho_prime, densify=args.densify, stride=args.stride, densify_pp_module=pp)
    ds = data.TestDataset(dev, data_path=args.data_path)
    rscale, rwin = getattr(args, "render_scale", 1), getattr(args, "render_window", None)
    rwin = None if rwin is None else tuple(rwin)
    render = rscale != 1 or rwin is not None
    if render:
        from . import tiling
        tiling.lattice(1, 1, rscale, (0, 0, 1, 1))                                  # the scale now; the window against each pair's size
        os.makedirs(args.out_path, exist_ok=True)
    rsize, spoints = getattr(args, "render_size", None), getattr(args, "sample_points", None)
    if spoints is not None:
        spoints = np.load(spoints)
        if spoints.ndim != 2 or spoints.shape[1] != 2 or spoints.shape[0] == 0:
            raise ValueError(f"--sample_points: the file must hold an [N,2] array of (y, x) positions, got {spoints.shape}")
    cloud, rcam = getattr(args, "point_cloud", False), getattr(args, "reproject", None)
    if rcam is not None:
        rcam = load_camera(rcam)
    fcfg = getattr(args, "fuse", None)
    if fcfg is not None:
        fcfg = load_fusion(fcfg)
    group = []
    complete = getattr(args, "complete", False)
    cmethod = getattr(args, "complete_method", "nearest")
    clabel = "completed" if cmethod == "nearest" else f"completed, {cmethod}"
    want_normals = getattr(args, "normals", False)
    if rsize is not None or spoints is not None or cloud or rcam is not None or complete or fcfg is not None or want_normals:
        os.makedirs(args.out_path, exist_ok=True)
    fine_maps, fine_thres = ("shpd", "refoc", "bndry", "depth", "conf"), 0.05 if (big or any_size) else None
    sweep = None
    if getattr(args, "refocus_stack", 0):
        sweep = focus_sweep(pipe.dcal, args.refocus_stack, *args.focus_range)
        os.makedirs(args.out_path, exist_ok=True)
        np.save(os.path.join(args.out_path, "rho_primes.npy"), sweep.astype(np.float32))
    tot, tot_dense = np.zeros(5), np.zeros(5)
    secs = 0.0
    for j in range(len(ds)):
        img_ny, gt = ds[j]
        img = img_ny.permute(0, 3, 1, 2).contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if any_size:
            maps = pipe.run_any(img, n_margin=args.n_margin_patch)
        else:
            maps = pipe.run_big(img, n_margin=args.n_margin_patch) if big else pipe(img)
        torch.cuda.synchronize()
        secs += time.perf_counter() - t0
        if sweep is not None:
            stack = pipe.refocus_stack(maps, rho_primes=sweep.tolist(), scale=rscale, window=rwin)
            np.save(os.path.join(args.out_path, f"refoc_stack_{j:04d}.npy"), stack.cpu().numpy())
        if render:
            fine = pipe.render_at(maps, scale=rscale, window=rwin, want=("shpd", "refoc", "bndry", "depth", "conf"),
                                  depth_thres=0.05 if (big or any_size) else None)
            np.savez(os.path.join(args.out_path, f"render_x{rscale}_{j:04d}.npz"),
                     **{k: v.cpu().numpy() for k, v in fine.items() if k != "lattice"})
        if rsize is not None:
            fine = pipe.render_resized(maps, tuple(rsize), want=fine_maps, depth_thres=fine_thres)
            np.savez(os.path.join(args.out_path, f"render_{rsize[0]}x{rsize[1]}_{j:04d}.npz"),
                     **{k: v.cpu().numpy() for k, v in fine.items() if k not in ("lattice", "valid")})
        if spoints is not None:
            fine = pipe.sample_at(maps, spoints, want=fine_maps, depth_thres=fine_thres)
            np.savez(os.path.join(args.out_path, f"samples_{j:04d}.npz"), **{k: v.cpu().numpy() for k, v in fine.items()})
        if cloud:
            pc = pipe.point_cloud(maps)
            np.savez(os.path.join(args.out_path, f"cloud_{j:04d}.npz"), **{k: v.cpu().numpy() for k, v in pc.items() if k != "lattice"})
        if want_normals:
            nrm = pipe.normals(maps, source="complete")
            np.savez(os.path.join(args.out_path, f"normals_{j:04d}.npz"), normal=nrm["normal"].cpu().numpy(), valid=nrm["valid"].cpu().numpy())
        if rcam is not None:
            # at scale 1 the maps the mode produced are the source (its own threshold); finer samples continue that threshold
            warped = pipe.reproject(maps, cam_dst=rcam["cam"], pose=rcam["pose"], size=rcam["size"], want=("shpd", "refoc"),
                                    scale=rcam["scale"], depth_thres=fine_thres if rcam["scale"] > 1 else None)
            np.savez(os.path.join(args.out_path, f"reproj_{j:04d}.npz"),
                     **{k: v.cpu().numpy() for k, v in warped.items() if k != "lattice"})
        if fcfg is not None:
            group.append(maps)
            if len(group) == len(fcfg["poses"]):
                gposes, extra = fcfg["poses"], {}
                if fcfg.get("register", 0) > 0:
                    gposes, grms = refine_poses(pipe, group, fcfg["poses"], fcfg["register"])
                    extra = dict(poses_refined=np.stack(gposes), register_rms=np.asarray(grms, np.float64))
                fused = pipe.fuse(list(zip(group, gposes)), cam_dst=fcfg["cam"], size=fcfg["size"], scale=fcfg["scale"],
                                  depth_thres=fine_thres if fcfg["scale"] > 1 else None, **fcfg["kw"])
                np.savez(os.path.join(args.out_path, f"fused_{j // len(group):04d}.npz"), **{k: v.cpu().numpy() for k, v in fused.items()},
                         **extra)
                if "tsdf" in fcfg:
                    vol = pipe.integrate(list(zip(group, gposes)), want=("shpd",), **fcfg["tsdf"])
                    cast = pipe.raycast(vol, pose=gposes[0], normals=True)           # view 0's camera, where view 0 stands
                    np.savez(os.path.join(args.out_path, f"tsdf_{j // len(group):04d}.npz"),
                             **{k: cast[k].cpu().numpy() for k in ("depth", "valid", "weight", "normal", "shpd")})
                    tri = pipe.extract_mesh(vol) if fcfg.get("tsdf_mesh", 0) > 0 or fcfg.get("mesh_render", 0) > 0 else None
                    cleaned = {}
                    if tri is not None and fcfg.get("mesh_min_triangles", 0) > 0:
                        tri = pipe.clean_mesh(tri, min_triangles=fcfg["mesh_min_triangles"])
                        cleaned = dict(components_triangles=tri.pop("components")["triangles"].cpu().numpy())
                    if tri is not None and fcfg.get("mesh_smooth", 0) > 0:           # after the cleaning: a floater that touches a surface drags it
                        tri = pipe.smooth_mesh(tri, iters=fcfg["mesh_smooth"])
                    if tri is not None and "mesh_cell" in fcfg:                      # after the cleaning: a floater's vertex would stay
                        tri = pipe.simplify_mesh(tri, fcfg["mesh_cell"], origin=fcfg["tsdf"]["origin"])
                    if fcfg.get("tsdf_mesh", 0) > 0:
                        pipe.save_mesh(os.path.join(args.out_path, f"mesh_{j // len(group):04d}.ply"), tri)
                        np.savez(os.path.join(args.out_path, f"mesh_{j // len(group):04d}.npz"), **{k: v.cpu().numpy() for k, v in tri.items()},
                                 **cleaned)
                    if fcfg.get("mesh_render", 0) > 0:                               # view 0's camera, where view 0 stands
                        seen = pipe.render_mesh(tri, cam_dst=vol.meta["camera"], pose=gposes[0], size=vol.meta["size"])
                        np.savez(os.path.join(args.out_path, f"mesh_render_{j // len(group):04d}.npz"),
                                 **{k: seen[k].cpu().numpy() for k in ("depth", "valid", "face", "normal", "shpd")})
                group = []
        depth = maps["depth_map"][None]
        m = np.array(utils.eval_depth(depth, gt[None].to(depth.dtype), depth, crop=args.crop))
        tot += m
        if not quiet:
            print(f'Image pair #{j}: delta1 ={m[0]: .3f}, delta2 ={m[1]: .3f}, delta3 ={m[2]: .3f}, RMSE ={m[3]: .3f} cm, '
                  f'AbsRel ={m[4]: .3f} cm')
        if complete:
            done = pipe.complete(maps) if cmethod == "nearest" else pipe.complete(maps, method=cmethod)
            np.savez(os.path.join(args.out_path, f"complete_{j:04d}.npz"), **{k: v.cpu().numpy() for k, v in done.items()})
            dense = done["depth_dense"][None]
            m = np.array(utils.eval_depth(dense, gt[None].to(dense.dtype), dense, crop=args.crop))
            tot_dense += m
            if not quiet:
                print(f'Image pair #{j} ({clabel}): delta1 ={m[0]: .3f}, delta2 ={m[1]: .3f}, delta3 ={m[2]: .3f}, RMSE ={m[3]: .3f} cm, '
                      f'AbsRel ={m[4]: .3f} cm')
    if group and not quiet:
        print(f'--fuse: the last {len(group)} pair(s) do not fill a group of {len(fcfg["poses"])} and were not fused')
    n = max(len(ds), 1)
    res = dict(zip(("delta1", "delta2", "delta3", "RMSE", "AbsRel"), (tot / n).tolist()), seconds_per_pair=secs / n)
    if not quiet:
        print(f'\nAverage running time:{secs / n: .3f} s')
        print('Average metrics for whole dataset: ' + ', '.join(f'{k} ={v: .3f}' for k, v in res.items() if k != "seconds_per_pair"))
    if complete:
        res["dense"] = dict(zip(("delta1", "delta2", "delta3", "RMSE", "AbsRel"), (tot_dense / n).tolist()))
        if not quiet:
            print(f'Average metrics for whole dataset ({clabel}): ' + ', '.join(f'{k} ={v: .3f}' for k, v in res["dense"].items()))
    return res


def main(argv=None):
    import utils
    argv = list(sys.argv[1:] if argv is None else argv)
    if not argv or argv[0] not in ("local_train", "global_pre", "global_train", "eval"):
        raise SystemExit("usage: python -m be_hip.workflow {local_train|global_pre|global_train|eval} [--big | --any] [reference arguments]")
    cmd, rest = argv[0], argv[1:]
    big, any_size = "--big" in rest, "--any" in rest
    rest = [a for a in rest if a not in ("--big", "--any")]
    if cmd == "eval":
        if big and any_size:
            raise SystemExit("eval: --big (the reference's tiler, sizes 59 + 88 k) and --any (any size >= 147 x 147) exclude each other")
        # --any takes the big-image arguments (--n_margin_patch, default --data_path ./data/data_test_big)
        return evaluate(utils.get_args('eval', big=big or any_size, argv=rest), big=big, any_size=any_size)
    elif cmd == "local_train":
        local_train(utils.get_args('local_train', argv=rest))
    elif cmd == "global_pre":
        global_pre(utils.get_args('global_pre', argv=rest))
    else:
        global_train(utils.get_args('global_train', argv=rest))


if __name__ == "__main__":
    main()
