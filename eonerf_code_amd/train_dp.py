#!/usr/bin/env python3
"""Data-parallel EO-NeRF training launcher -- the loop of train_eonerf.py:96-161,304 on the HIP hot path.

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \\
        -m eonerf_code_amd.train_dp --rays table.pt --n_images 19 --batch_size 4096 --max_train_steps 300000

`--rays` is a torch file {"rays": [N,11] fp32 normalised rays, "ts": [N] int64 image index, "rgbs": [N,3]} as
datasets/satellite.py:406-481 builds it (eonerf_code_amd.datasets.satellite.generate_rays produces the rays on the
GPU); without it a synthetic JAX_068-like table is used.  Same schedule as the reference: seed 42, Adam lr 5e-4,
StepLR gamma 0.9 per epoch, MSE for epoch < 2 then the uncertainty loss with the shadow pass on.

`--gt_dsm` is a torch file {"dsm": [H,W] fp32 lidar DSM, "roi": [xoff, yoff, size, res], "scene_offset": [3], "scene_scale": [3],
optional "water": [H,W] uint8, optional "sun": [elevation_deg, azimuth_deg] of the nadir camera's sun direction}.  With it, after
every epoch (val_freq, train_eonerf.py:194) every rank checks its device status and rank 0 renders the nadir DSM, registers it on
the ground truth and prints val/mae -- all on the GPU (eonerf_code_amd.dsm.evaluate_dsm).  Without it nothing changes.

`--init_dsm` is a torch file {"dsm": [H,W] fp32 initial DSM, "bounds": [left, bottom, right, top] (UTM metres), "zone", "south",
"scene_offset": [3], "scene_scale": [3], "rpcs": one rpcm dict per image at the table's downscale, "shapes": [n_img, 2], optional
"conf": [H,W]} -- the reference's --init_dsm_path / --init_conf_path (opt.py:88-91) as tensors.  With it every rank builds the depth
priors of the whole table on its own device at start-up (eonerf_code_amd.priors.depth_priors_from_dsm; deterministic, hence the same
on every rank), carries them as a RayTable extra and adds metrics.depth_loss_L2 with weight --w_depth, multiplied by 0.8 after every
epoch (train_eonerf.py:94,145-149,305-306); the status line gains train/depth_l2 and depth_weight.  Each rank takes the masked mean
over its own rays.  Without it nothing changes.

`--occ_grid` mirrors the reference's occupancy grid (train_eonerf.py:74,112-119): rank 0 updates a 128^3 grid from the field's density
every `--occ_every` steps on the training context (eonerf_code_amd.occupancy.OccupancyGrid), the per-epoch validation renders
(`--gt_dsm`, `--val_images`) skip the samples of its empty cells (the grid dilated by one cell), and checkpoints carry it.  The training
step itself never reads the grid.  Without the flag nothing changes.

`--ortho` is a torch file {"images": K tensors [h_k, w_k, C], "rpcs": one rpcm dict per image, "size": [h, w] of the mosaic, "min_alt",
"max_alt", "scene_offset": [3], "scene_scale": [3], "zone", "south"}.  With it, after the last step, rank 0 makes the true orthophoto
of the images on the nadir grid (eonerf_code_amd.ortho.orthorectify: the images gathered through their RPCs on the rendered surface,
occluded cells left out, median-fused) and torch.saves the result dict plus "geotransform" to `--ortho_out`.  `--occ_grid` and the step
size reach that render as they reach the validation renders.  Without the flag nothing changes.

`--mesh_out PATH` writes, after the last step and on rank 0 only, a triangle mesh of the field's density level set as a binary PLY
(eonerf_code_amd.mesh.extract_mesh / save_ply: marching tetrahedra on a `--mesh_res`^3 lattice over the normalised cube, per-vertex
normals and albedo).  `--mesh_level` is the density of the level set; its default (half opacity over one render step of 128 samples) is
a guess that has not been measured on a converged scene.  `--mesh_min_component N` drops every solid of fewer than N lattice points,
`--mesh_keep_largest K` all but the K largest, `--mesh_fill_cavities` the closed inner surfaces no view can see
(mesh.filter_components); all three are off by default -- a good N has not been measured -- and act only together with `--mesh_out`;
with any of them the PLY also carries each vertex' component id.  `--mesh_simplify K` (with `--mesh_representative mean|nearest`,
default mean) clusters the mesh's vertices on cells of K lattice spacings before normals and albedo are taken (mesh.simplify_mesh); the
status line then also shows the counts before, `vertices_in=` and `faces_in=`.  It is off by default -- what it costs in DSM MAE on a
converged scene has not been measured -- and acts only together with `--mesh_out`.  `--mesh_smooth K` (with `--mesh_smooth_lambda L`
and `--mesh_smooth_mu M`, defaults 0.5 and -0.53) runs K lambda|mu iterations of Taubin smoothing in units of one lattice spacing on
the extracted mesh, before the simplification, the normals and the albedo (mesh.smooth_mesh); it moves vertices and keeps every vertex
and face, vertices on an open boundary stay put, and the status line then ends in `smooth=K | open=N`, N the open vertices.  It is off
by default -- what it does to the DSM MAE is a measurement in profiles/smooth_ab.txt, not a default -- and acts only together with
`--mesh_out`.  `--mesh_method tetra|dual` (default tetra) chooses the mesher: marching tetrahedra, or dual contouring
(mesh.dual_contour: one vertex per surface cell from the density gradient at the crossing points of its edges, which keeps ridges and
corners, at about a third of the triangles) with `--mesh_dual_reg L` as its regularisation (default 0.1, a guess that has not been
measured); the three component flags still filter the volume in front of it, but a dual mesh carries no per-vertex component id,
and the status line then ends in `method=dual | clamped=N`.  It acts only together with `--mesh_out`.  Together with `--gt_dsm` rank 0 then rasterises
the mesh it saved (filtered, smoothed, simplified) straight from above on the lidar DSM's grid, registers it and prints `mesh/mae=` once
(eonerf_code_amd.mesh.evaluate_mesh_dsm): the mesh on the scale of val/mae.  Without the flag nothing changes.
`--mesh_views` (with `--mesh_out` and `--val_images`; refused without them) casts the rays of every held-out image against the saved
mesh on rank 0 (eonerf_code_amd.mesh.mesh_view_metrics) and prints `mesh/view_depth=`, the mean |mesh depth - field depth| over the rays
that hit, the field depth from a depth-only export render of the same rays; `mesh/view_hits=`; and `mesh/shadow_agree=`, the share of
hit rays where the mesh's hard shadow for the image's sun equals geo_shadows >= 0.5.  Without the flag nothing changes.
`--mesh_texture FILE` (with `--mesh_out`; refused without it) is a torch file in the format of `--ortho` ("size" is not read).  After the
mesh is saved, rank 0 bakes the images onto it (eonerf_code_amd.texture.bake_texture: a per-face atlas of `--mesh_texels` texels a leg,
every texel projected through each image's RPC, occlusion against the mesh itself, median-fused) and writes <PATH stem>.obj, .mtl and
.png beside the PLY (texture.save_obj); it prints `mesh/texels=`, the texels a face owns, and `mesh/textured=`, the share of them at
least one image sees.  Without the flag nothing changes.
"""
import argparse
import os
import time

import torch


def depth_prior_term(extras, w_depth, record=None):
    """The aux_loss of one batch (train_eonerf.py:145-149): metrics.depth_loss_L2 of the batch's priors (RayTable extras "prior_depth",
    optional "prior_conf") on the rendered depth, column 3 of the packed outputs.  record: a one-element list that receives the term."""
    from .priors import depth_loss_L2

    def aux(out):
        term = depth_loss_L2(extras["prior_depth"], out[:, 3], extras.get("prior_conf"), w_depth)
        if record is not None:
            record[0] = term.detach()
        return term
    return aux


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", default=None)
    ap.add_argument("--n_images", type=int, default=19)
    ap.add_argument("--batch_size", type=int, default=4096, help="rays per GPU per step")
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--max_train_steps", type=int, default=1000)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--n_samples", type=int, default=128, help="samples per ray = int(2 / render_step_size) (opt.py:54): 2 .. 256")
    ap.add_argument("--logs_dir", default="logs")
    ap.add_argument("--exp_name", default="eonerf_hip")
    ap.add_argument("--synthetic_rays", type=int, default=1 << 20)
    ap.add_argument("--check_every", type=int, default=1000, help="steps between host syncs (loss print + device status on every rank)")
    ap.add_argument("--dump_params", default=None, help="write the final flat parameters of every rank to <path>.rank<r>")
    ap.add_argument("--gt_dsm", default=None, help="torch file with the lidar DSM, its ROI and the scene normalisation: DSM MAE after every epoch")
    ap.add_argument("--val_chunk", type=int, default=5120, help="rays per chunk of the validation render")
    ap.add_argument("--val_images", default=None, help="torch file with held-out images (rays, rgbs, h, w): image loss and PSNR after every epoch")
    ap.add_argument("--val_max", type=int, default=5, help="validation images rendered per epoch (train_eonerf.py:200)")
    ap.add_argument("--init_dsm", default=None, help="torch file with an initial DSM, its bounds / UTM zone, the scene normalisation and the images' RPCs: depth supervision")
    ap.add_argument("--w_depth", type=float, default=100.0, help="weight of the depth term (x 0.8 after every epoch)")
    ap.add_argument("--occ_grid", action="store_true", help="keep an occupancy grid (rank 0): validation renders cull by it, checkpoints carry it")
    ap.add_argument("--occ_every", type=int, default=50, help="steps between occupancy grid updates (train_eonerf.py:112-119)")
    ap.add_argument("--early_stop_eps", type=float, default=0.0, help="validation renders stop a ray below this transmittance (0: off)")
    ap.add_argument("--march_block", type=int, default=32, help="sampler slots per round of a render with --early_stop_eps: 16, 32 or 64")
    ap.add_argument("--dsm_quantile", type=float, default=None, help="val/mae and val/img_mae read the depth at this opacity quantile (0.5: the median surface) instead of the expected depth")
    ap.add_argument("--ortho", default=None, help="torch file with the input images, their RPCs, the mosaic size and the scene normalisation: true orthophoto after the last step")
    ap.add_argument("--ortho_out", default=None, help="where rank 0 saves the orthophoto (default: <logs_dir>/<exp_name>/ortho.pt)")
    ap.add_argument("--mesh_out", default=None, help="where rank 0 saves a PLY mesh of the density level set after the last step")
    ap.add_argument("--mesh_res", type=int, default=256, help="lattice points per axis of the mesh extraction")
    ap.add_argument("--mesh_level", type=float, default=None, help="density of the extracted level set (default: mesh.level_from_opacity(0.5, 2 / 128))")
    ap.add_argument("--mesh_min_component", type=int, default=0, help="drop solids of fewer lattice points from the mesh (0: keep all; only with --mesh_out)")
    ap.add_argument("--mesh_keep_largest", type=int, default=0, help="keep the K largest solids of the mesh, ties included (0: keep all; only with --mesh_out)")
    ap.add_argument("--mesh_fill_cavities", action="store_true", help="drop closed inner surfaces from the mesh (only with --mesh_out)")
    ap.add_argument("--mesh_simplify", type=int, default=0, help="cluster the mesh's vertices on cells of K lattice spacings (0: off; only with --mesh_out)")
    ap.add_argument("--mesh_smooth", type=int, default=0, help="lambda|mu iterations of Taubin smoothing on the extracted mesh (0: off; only with --mesh_out)")
    ap.add_argument("--mesh_smooth_lambda", type=float, default=0.5, help="the positive factor of a smoothing iteration")
    ap.add_argument("--mesh_smooth_mu", type=float, default=-0.53, help="the negative factor of a smoothing iteration (0: plain Laplacian)")
    ap.add_argument("--mesh_method", choices=["tetra", "dual"], default="tetra", help="the mesher: marching tetrahedra or dual contouring (only with --mesh_out)")
    ap.add_argument("--mesh_dual_reg", type=float, default=0.1, help="regularisation of --mesh_method dual, in lattice spacings (2^-10 .. 16)")
    ap.add_argument("--mesh_views", action="store_true",
                    help="cast every --val_images view's rays against the saved mesh: depth against the field's, hits, shadow agreement (only with --mesh_out and --val_images)")
    ap.add_argument("--mesh_texture", default=None, help="torch file in the format of --ortho: bake the images onto the saved mesh, write <stem>.obj/.mtl/.png (only with --mesh_out)")
    ap.add_argument("--mesh_texels", type=int, default=4, help="texels per triangle leg of the texture atlas (1 .. 64)")
    ap.add_argument("--mesh_representative", choices=["mean", "nearest"], default="mean", help="a cell's vertex: the mean of its vertices, or the one nearest to it")
    ap.add_argument("--rpc_correction", action="store_true", help="learn a 3-D offset per image, added to that image's ray origins (opt.py:80); single process only")
    ap.add_argument("--rpc_lr", type=float, default=None, help="learning rate of the offsets (default: --lr)")
    ap.add_argument("--resume", default=None, help="checkpoint to continue from (weights, optimizer state and, with --rpc_correction, the offsets)")
    args = ap.parse_args()
    if args.mesh_views and not (args.mesh_out and args.val_images):
        raise SystemExit("--mesh_views: the views of --val_images are cast against the mesh of --mesh_out; give both")
    if args.mesh_texture and not args.mesh_out:
        raise SystemExit("--mesh_texture: the images are baked onto the mesh of --mesh_out; give both")

    world, rank, local = int(os.environ.get("WORLD_SIZE", 1)), int(os.environ.get("RANK", 0)), int(os.environ.get("LOCAL_RANK", 0))
    # EONERF_DP_REHEARSAL=1 (tests on a one-GPU box, not a deployment mode): every rank on cuda:0, gloo instead of RCCL; run it with
    # EONERF_PIPE=0 -- the pipelined backward assumes the card to itself
    rehearsal = os.environ.get("EONERF_DP_REHEARSAL") == "1"
    if args.rpc_correction and world > 1:
        raise SystemExit("--rpc_correction: the offsets are not exchanged between ranks yet; run it on one GPU (WORLD_SIZE=1)")
    if rehearsal:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # (EONERF_FORCE_ALLREDUCE=1: the process group and the gradient exchange also at world size 1 -- the N > 1 code path on a one-GPU box)
    if world > 1 or os.environ.get("EONERF_FORCE_ALLREDUCE") == "1":
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        if rehearsal:
            torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
        else:
            torch.distributed.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from .checkpoint import load_checkpoint, save_checkpoint
    from .radiance_fields.eonerf import EONerfMLP
    from .synthetic import synthetic_batch
    from .trainer import FusedTrainer, RayTable

    torch.manual_seed(42)                                                   # train_eonerf.py:37
    if args.rays:
        d = torch.load(args.rays, map_location="cpu")
        rays, ts, rgbs = d["rays"], d["ts"], d["rgbs"]
    else:
        rays, ts, rgbs = synthetic_batch(args.synthetic_rays, args.n_images)
    extras = None
    if args.init_dsm:
        from .priors import depth_priors_from_dsm
        p = torch.load(args.init_dsm, map_location="cpu")
        for key in ("dsm", "bounds", "zone", "south", "scene_offset", "scene_scale", "rpcs", "shapes"):
            if key not in p:
                raise SystemExit(f"--init_dsm {args.init_dsm}: missing entry '{key}'")
        conf = p["conf"].to(dev) if p.get("conf") is not None else None
        prior, prior_conf = depth_priors_from_dsm(p["dsm"].to(dev), [float(x) for x in p["bounds"]], p["rpcs"], p["shapes"],
                                                  rays.to(dev, torch.float32).contiguous(), p["scene_offset"], p["scene_scale"],
                                                  int(p["zone"]), bool(p["south"]), conf=conf)
        extras = {"prior_depth": prior} if prior_conf is None else {"prior_depth": prior, "prior_conf": prior_conf}
    w_depth, depth_term = args.w_depth, [None]
    table = RayTable(rays, ts, rgbs, dev, seed=42, rank=rank, world=world, extras=extras)
    field = EONerfMLP(args.n_images, radiometric_normalization=True, precision=args.precision).to(dev)
    trainer = FusedTrainer(field, lr=args.lr, max_rays=args.batch_size, keep_message=False, n_samples=args.n_samples,
                           origin_offsets=args.rpc_correction, offsets_lr=args.rpc_lr)
    trainer.set_noise_seed(42 + 1000003 * rank)                              # per-rank jitter stream
    steps_per_epoch = max(1, table.steps_per_epoch(args.batch_size))
    occ = None
    if args.occ_grid and rank == 0:
        from .occupancy import OccupancyGrid
        occ = OccupancyGrid(128, device=dev)                                   # opt.py:86
    gt = None
    if args.gt_dsm:
        gt = torch.load(args.gt_dsm, map_location="cpu")
        for key in ("dsm", "roi", "scene_offset", "scene_scale"):
            if key not in gt:
                raise SystemExit(f"--gt_dsm {args.gt_dsm}: missing entry '{key}'")
        if rank == 0:
            gt["dsm"] = gt["dsm"].to(dev, torch.float32)
            gt["water"] = gt["water"].to(dev, torch.uint8) if gt.get("water") is not None else None
    val_images = None
    if args.val_images:
        v = torch.load(args.val_images, map_location="cpu")
        if "images" not in v:
            raise SystemExit(f"--val_images {args.val_images}: missing entry 'images'")
        for k, im in enumerate(v["images"]):
            for key in ("rays", "rgbs", "h", "w"):
                if key not in im:
                    raise SystemExit(f"--val_images {args.val_images}: image {k}: missing entry '{key}'")
        if rank == 0:
            # "img_idx" (optional): the image's row of the offset table -- with --rpc_correction its rays are corrected before validation
            val_images = [{"rays": im["rays"].to(dev, torch.float32), "rgbs": im["rgbs"].to(dev, torch.float32), "h": int(im["h"]),
                           "w": int(im["w"]), "img_idx": (int(im["img_idx"]) if im.get("img_idx") is not None else None)}
                          for im in v["images"][:max(0, args.val_max)]]
    ortho = None
    if args.ortho:
        ortho = torch.load(args.ortho, map_location="cpu")
        for key in ("images", "rpcs", "size", "min_alt", "max_alt", "scene_offset", "scene_scale", "zone", "south"):
            if key not in ortho:
                raise SystemExit(f"--ortho {args.ortho}: missing entry '{key}'")
    mesh_texture = None
    if args.mesh_texture:
        mesh_texture = torch.load(args.mesh_texture, map_location="cpu")
        for key in ("images", "rpcs", "min_alt", "max_alt", "scene_offset", "scene_scale", "zone", "south"):
            if key not in mesh_texture:
                raise SystemExit(f"--mesh_texture {args.mesh_texture}: missing entry '{key}'")
    pose_field = ""
    if args.resume:
        load_checkpoint(args.resume, field, trainer, occ_grid=occ)
        if args.rpc_correction and rank == 0:
            from .pose import max_offset
            print(f"resumed={args.resume} | pose/max_offset={float(max_offset(trainer.origin_offsets)):.6g}", flush=True)
    step, tic = 0, time.time()
    for epoch in range(10 ** 7):
        for i in range(steps_per_epoch):
            aux = None
            if extras is None:
                r, im, px = table.batch(epoch, i, args.batch_size)
            else:
                r, im, px, ex = table.batch(epoch, i, args.batch_size, with_extras=True)
                aux = depth_prior_term(ex, w_depth, depth_term)
            nxt = None
            if trainer._exchanges() and i + 1 < steps_per_epoch:                     # the next batch's sampler runs under this step's gradient exchange
                r2, im2, _ = table.batch(epoch, i + 1, args.batch_size)
                nxt = (r2, im2, epoch) if extras is None else (r2, im2, epoch, True)
            loss = trainer.step(r, im, px, epoch, next_batch=nxt, aux_loss=aux)
            if occ is not None:                                             # train_eonerf.py:112-119 (no host sync)
                occ.update_every_n_steps(step, field, 2.0 / args.n_samples, n=args.occ_every)
            if step % args.check_every == 0:                                # the only host sync, every 1000 steps (:173-178)
                # on EVERY rank: raises (-> non-zero exit of the job) if a device-side hand-off timed out on ANY rank since the last
                # check; the fault flag of the gradient message has kept all replicas from applying an update since
                trainer.check_device_status()
            if step % args.check_every == 0 and rank == 0:
                el = time.time() - tic
                prior_fields = "" if extras is None else f" | train/depth_l2={float(depth_term[0]):.5f} | depth_weight={w_depth:.6g}"
                if args.rpc_correction:                                     # largest row norm in scene units: a drifting gauge shows here
                    from .pose import max_offset
                    pose_field = f" | pose/max_offset={float(max_offset(trainer.origin_offsets)):.6g}"
                print(f"epoch={epoch} | elapsed_time={el:.2f}s | step={step} | loss={float(loss):.5f} | "
                      f"rays/s={(step + 1) * args.batch_size * world / max(el, 1e-9):.0f}{prior_fields}{pose_field}", flush=True)
            save_now = step > 0 and step % (4 * steps_per_epoch) == 0         # save_freq, :180-191 (the same decision on every rank)
            if save_now and step % args.check_every != 0:
                # a checkpoint must not hold updates that were skipped: after a device-side fault the Adam kernel leaves the weights alone
                # while the host's step count keeps running -- every rank checks (and raises together) BEFORE rank 0 writes
                trainer.check_device_status()
            if save_now and rank == 0:
                save_checkpoint(os.path.join(args.logs_dir, args.exp_name, f"ckpts/epoch={epoch}.ckpt"), epoch, field, trainer, loss, occ_grid=occ,
                                origin_offsets=trainer if args.rpc_correction else None)
            if step == args.max_train_steps:
                trainer.check_device_status()
                if ortho is not None and rank == 0:
                    from .ortho import nadir_geotransform, orthorectify
                    oh, ow = (int(x) for x in ortho["size"])
                    k_img = len(ortho["images"])
                    res = orthorectify(field, ortho["images"], ortho["rpcs"], ortho["scene_offset"], ortho["scene_scale"], int(ortho["zone"]),
                                       bool(ortho["south"]), oh, ow, float(ortho["min_alt"]), float(ortho["max_alt"]), chunk=args.val_chunk,
                                       occupancy_grid=occ, radiometric=(k_img == args.n_images and ortho["images"][0].shape[-1] == 3))
                    res = {k: v.cpu() for k, v in res.items()}
                    res["geotransform"] = nadir_geotransform(oh, ow, ortho["scene_offset"], ortho["scene_scale"])
                    path = args.ortho_out or os.path.join(args.logs_dir, args.exp_name, "ortho.pt")
                    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                    torch.save(res, path)
                    print(f"step={step} | ortho={path} | cells={int((res['count'] > 0).sum())}/{oh * ow}", flush=True)
                if args.mesh_out and rank == 0:
                    from .mesh import extract_mesh, save_ply
                    cleaned = bool(args.mesh_min_component or args.mesh_keep_largest or args.mesh_fill_cavities)
                    mesh = extract_mesh(field, resolution=args.mesh_res, level=args.mesh_level, min_component_points=args.mesh_min_component,
                                        keep_largest=args.mesh_keep_largest, fill_cavities=args.mesh_fill_cavities,
                                        components=cleaned and args.mesh_method == "tetra",
                                        simplify=args.mesh_simplify, representative=args.mesh_representative, smooth=args.mesh_smooth,
                                        smooth_lambda=args.mesh_smooth_lambda, smooth_mu=args.mesh_smooth_mu, method=args.mesh_method,
                                        dual_regularisation=args.mesh_dual_reg)
                    os.makedirs(os.path.dirname(os.path.abspath(args.mesh_out)), exist_ok=True)
                    save_ply(args.mesh_out, mesh)
                    print(f"step={step} | mesh={args.mesh_out} | vertices={mesh['vertices'].shape[0]} | faces={mesh['faces'].shape[0]} | "
                          f"level={mesh['level']:.6g}" +
                          (f" | vertices_in={mesh['simplify']['vertices_in']} | faces_in={mesh['simplify']['faces_in']}" if args.mesh_simplify else "") +
                          (f" | smooth={args.mesh_smooth} | open={mesh['smooth']['open']}" if args.mesh_smooth else "") +
                          (f" | method=dual | clamped={mesh['dual']['clamped']}" if args.mesh_method == "dual" else ""), flush=True)
                    if cleaned and "component" in mesh:
                        sizes = mesh["component_points"]
                        print(f"step={step} | mesh_components={int(torch.unique(mesh['component']).numel())} | "
                              f"smallest_component={int(sizes.min()) if sizes.numel() else 0} | " +
                              " | ".join(f"{k}={v}" for k, v in mesh["report"].items()), flush=True)
                    if gt is not None:                                      # the saved (filtered) mesh on the scale of val/mae
                        from .mesh import evaluate_mesh_dsm
                        mesh_mae, mesh_cells = evaluate_mesh_dsm(mesh, gt["dsm"], [float(x) for x in gt["roi"]], gt["scene_offset"],
                                                                 gt["scene_scale"], water=gt["water"]).tolist()
                        print(f"step={step} | mesh/mae={mesh_mae:.4f} | mesh/cells={int(mesh_cells)}", flush=True)
                    if args.mesh_views and val_images:                      # the saved mesh through the cameras of the held-out images
                        from .mesh import mesh_view_metrics
                        view_depth, view_hits, shadow_agree, view_rays = mesh_view_metrics(field, mesh, val_images, chunk=args.val_chunk, occupancy_grid=occ).tolist()
                        print(f"step={step} | mesh/view_depth={view_depth:.5f} | mesh/view_hits={int(view_hits)} | mesh/view_rays={int(view_rays)} | "
                              f"mesh/shadow_agree={shadow_agree:.4f}", flush=True)
                    if mesh_texture is not None:                            # the images on the saved mesh: <stem>.obj / .mtl / .png
                        from .texture import bake_texture, save_obj
                        mt = mesh_texture
                        radiometric = len(mt["images"]) == args.n_images and mt["images"][0].shape[-1] == 3
                        tex = bake_texture(mesh, mt["images"], mt["rpcs"], mt["scene_offset"], mt["scene_scale"], int(mt["zone"]), bool(mt["south"]),
                                           float(mt["min_alt"]), float(mt["max_alt"]), texels=args.mesh_texels, field=field if radiometric else None)
                        dev_v = mesh["vertices"].device
                        mesh["vertices_utm"] = (mesh["vertices"].double() * torch.as_tensor(mt["scene_scale"], dtype=torch.float32).reshape(3).double().to(dev_v)
                                                + torch.as_tensor(mt["scene_offset"], dtype=torch.float32).reshape(3).double().to(dev_v))
                        obj = save_obj(os.path.splitext(args.mesh_out)[0] + ".obj", mesh, tex)[0]
                        owned = tex["face"] >= 0
                        n_owned = int(owned.sum())
                        textured = int(((tex["count"] > 0) & owned).sum()) / max(n_owned, 1)
                        print(f"step={step} | mesh_obj={obj} | mesh/texels={n_owned} | mesh/textured={textured:.4f}", flush=True)
                if args.dump_params:                                        # replica-equality checks of the tests
                    torch.save(field.flat_params().detach().cpu(), f"{args.dump_params}.rank{rank}")
                if torch.distributed.is_initialized():
                    torch.distributed.destroy_process_group()
                return
            step += 1
        if gt is not None:                                                  # val_freq = one epoch (:194)
            trainer.check_device_status()                                   # on every rank: no validation of weights a fault has frozen
            if rank == 0:
                from .dsm import evaluate_dsm
                sun = [float(x) for x in gt.get("sun", (0.0, 0.0))]
                mae = evaluate_dsm(field, gt["dsm"], [float(x) for x in gt["roi"]], gt["scene_offset"], gt["scene_scale"], sun,
                                   chunk=args.val_chunk, water=gt["water"], occupancy_grid=occ,
                                   early_stop_eps=args.early_stop_eps, march_block=args.march_block, depth_quantile=args.dsm_quantile)
                mae, n_valid = mae.tolist()                                 # the validation's one read-back
                print(f"epoch={epoch} | elapsed_time={time.time() - tic:.2f}s | step={step} | val/mae={mae:.4f} | val/cells={int(n_valid)}", flush=True)
        if args.val_images:                                                 # the held-out images of the same block (:199-294)
            if gt is None:
                trainer.check_device_status()                               # on every rank (with --gt_dsm the check above has just run)
            if rank == 0 and val_images:
                from .validation import validate_images
                images = val_images
                if args.rpc_correction:                                     # the tables whose image index is known render on corrected rays
                    from .pose import apply_origin_offsets
                    images = [im if im["img_idx"] is None else
                              dict(im, rays=apply_origin_offsets(im["rays"], torch.full((im["rays"].shape[0],), im["img_idx"], dtype=torch.int64, device=dev),
                                                                 trainer.origin_offsets)) for im in val_images]
                _, means = validate_images(field, images, epoch, chunk=args.val_chunk, gt=gt, max_images=args.val_max, occupancy_grid=occ,
                                           early_stop_eps=args.early_stop_eps, march_block=args.march_block, depth_quantile=args.dsm_quantile)
                names = ("loss", "coarse_color", "coarse_logbeta", "psnr") + (("mae",) if gt is not None else ())
                vals = torch.stack([means[k] for k in names]).tolist()      # the validation's one read-back
                line = (f"epoch={epoch} | elapsed_time={time.time() - tic:.2f}s | step={step} | val/loss={vals[0]:.5f} | "
                        f"val/coarse_color={vals[1]:.5f} | val/coarse_logbeta={vals[2]:.5f} | val/psnr={vals[3]:.4f}")
                print(line + (f" | val/img_mae={vals[4]:.4f}" if gt is not None else ""), flush=True)
        trainer.set_lr(trainer.lr * 0.9)                                    # StepLR(step_size=1, gamma=0.9), :64,304
        w_depth *= 0.8                                                      # :305-306


if __name__ == "__main__":
    main()
