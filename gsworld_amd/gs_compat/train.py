#!/usr/bin/env python
"""``train.py`` of the 3DGS python layer on the MI355X: a COLMAP capture on disk -> a trained ``point_cloud.ply``
(step 1 of GSWorld's real2sim recipe: ``python train.py -s DATA -m MODEL --disable_viewer --iterations N``).

Upstream's command line and loop.  Every kernel of an iteration is this package's: the rasterizer forward / backward, the
loss (``gsworld_amd.ssim.training_loss``: exposure, clamp, alpha mask, L1 + ssim and the inverse-depth term as one node;
``--composed_loss`` builds it from torch operations and ``fused_ssim`` as upstream does), ``SparseGaussianAdam``, the
densification statistics and densify-and-prune.  An iteration reads nothing from the device; the progress line does every
tenth iteration.  Not provided: the network viewer (``--ip --port --disable_viewer`` are accepted and ignored, no socket is
opened), the Blender reader, ``render.py`` / ``metrics.py`` and LPIPS."""
import os
import sys
import uuid
from argparse import ArgumentParser, Namespace
from random import randint

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "dropin"), os.path.dirname(os.path.dirname(_HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from arguments import ModelParams, OptimizationParams, PipelineParams  # noqa: E402
from utils.general_utils import get_expon_lr_func, safe_state  # noqa: E402

try:
    from torch.utils.tensorboard import SummaryWriter
    TENSORBOARD_FOUND = True
except ImportError:
    TENSORBOARD_FOUND = False


def composed_training_loss(render_pkg, viewpoint_cam, lambda_dssim, depth_weight):
    """Upstream's composition on ``render()``'s clamped (and exposed) image: the reference for ``training_loss``."""
    from fused_ssim import fused_ssim
    from utils.loss_utils import l1_loss

    image = render_pkg["render"]
    if viewpoint_cam.alpha_mask is not None:
        image = image * viewpoint_cam.alpha_mask.cuda()
    gt_image = viewpoint_cam.original_image.cuda()
    loss = (1.0 - lambda_dssim) * l1_loss(image, gt_image) + \
        lambda_dssim * (1.0 - fused_ssim(image.unsqueeze(0), gt_image.unsqueeze(0)))
    if depth_weight > 0 and viewpoint_cam.depth_reliable:
        mono_invdepth = viewpoint_cam.invdepthmap.cuda()
        depth_mask = viewpoint_cam.depth_mask.cuda()
        loss = loss + depth_weight * torch.abs((render_pkg["depth"] - mono_invdepth) * depth_mask).mean()
    return loss


def training_step(gaussians, viewpoint_cam, iteration, opt, pipe, background, train_test_exp=False, depth_weight=0.0,
                  composed_loss=False, between=None):
    """One iteration: learning rates, SH degree, render, loss, backward, densification statistics, ``between(render_pkg)``
    (the loop's densify / report / save, or None), the optimizer steps.  Nothing is read from the device.  -> the loss."""
    from gaussian_renderer import render

    gaussians.update_learning_rate(iteration)
    if iteration % 1000 == 0:
        gaussians.oneupSHdegree()
    if composed_loss:
        render_pkg = render(viewpoint_cam, gaussians, pipe, background, use_trained_exp=train_test_exp)
        loss = composed_training_loss(render_pkg, viewpoint_cam, opt.lambda_dssim, depth_weight)
    else:
        from gsworld_amd.ssim import training_loss

        render_pkg = render(viewpoint_cam, gaussians, pipe, background, use_trained_exp=train_test_exp, raw_color=True)
        depth = depth_weight > 0 and viewpoint_cam.depth_reliable
        loss = training_loss(
            render_pkg["render"], viewpoint_cam.original_image.cuda(), opt.lambda_dssim,
            exposure=gaussians.get_exposure_from_name(viewpoint_cam.image_name) if train_test_exp else None,
            alpha_mask=viewpoint_cam.alpha_mask.cuda() if viewpoint_cam.alpha_mask is not None else None,
            invdepth=render_pkg["depth"] if depth else None,
            mono_invdepth=viewpoint_cam.invdepthmap.cuda() if depth else None,
            depth_mask=viewpoint_cam.depth_mask.cuda() if depth else None, depth_weight=depth_weight if depth else 0.0)
    loss.backward()
    with torch.no_grad():
        radii = render_pkg["radii"]
        if iteration < opt.densify_until_iter:
            gaussians.add_densification_stats(render_pkg["viewspace_points"], radii)
        if between is not None:
            between(render_pkg)
        if iteration < opt.iterations:
            if gaussians.exposure_optimizer is not None:
                gaussians.exposure_optimizer.step()
                gaussians.exposure_optimizer.zero_grad(set_to_none=True)
            if gaussians.optimizer_type == "sparse_adam":
                gaussians.optimizer.step(radii, radii.shape[0])
            else:
                gaussians.optimizer.step()
            gaussians.optimizer.zero_grad(set_to_none=True)
    return loss.detach()


def training(dataset, opt, pipe, testing_iterations, saving_iterations, checkpoint_iterations, checkpoint, debug_from,
             composed_loss=False):
    from scene import GaussianModel, Scene

    first_iter = 0
    tb_writer = prepare_output_and_logger(dataset)
    gaussians = GaussianModel(dataset.sh_degree, opt.optimizer_type)
    scene = Scene(dataset, gaussians)
    gaussians.training_setup(opt)
    if checkpoint:
        model_params, first_iter = torch.load(checkpoint, weights_only=False)
        gaussians.restore(model_params, opt)

    bg_color = [1, 1, 1] if dataset.white_background else [0, 0, 0]
    background = torch.tensor(bg_color, dtype=torch.float32, device="cuda")
    depth_l1_weight = get_expon_lr_func(opt.depth_l1_weight_init, opt.depth_l1_weight_final, max_steps=opt.iterations)

    viewpoint_stack = scene.getTrainCameras().copy()
    ema_loss_for_log = 0.0
    try:
        from tqdm import tqdm
        progress_bar = tqdm(range(first_iter, opt.iterations), desc="Training progress")
    except ImportError:
        progress_bar = None
    first_iter += 1
    for iteration in range(first_iter, opt.iterations + 1):
        if not viewpoint_stack:
            viewpoint_stack = scene.getTrainCameras().copy()
        viewpoint_cam = viewpoint_stack.pop(randint(0, len(viewpoint_stack) - 1))
        if (iteration - 1) == debug_from:
            pipe.debug = True
        bg = torch.rand((3), device="cuda") if opt.random_background else background

        def between(render_pkg, iteration=iteration):
            training_report(tb_writer, iteration, testing_iterations, scene, pipe, background, dataset.train_test_exp)
            if iteration in saving_iterations:
                print(f"\n[ITER {iteration}] Saving Gaussians")
                scene.save(iteration)
            if iteration < opt.densify_until_iter:
                if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                    size_threshold = 20 if iteration > opt.opacity_reset_interval else None
                    gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, scene.cameras_extent, size_threshold,
                                                render_pkg["radii"])
                if iteration % opt.opacity_reset_interval == 0 or \
                        (dataset.white_background and iteration == opt.densify_from_iter):
                    gaussians.reset_opacity()

        loss = training_step(gaussians, viewpoint_cam, iteration, opt, pipe, bg, dataset.train_test_exp,
                             float(depth_l1_weight(iteration)), composed_loss, between)

        if iteration % 10 == 0:  # (the only read of the device in the loop)
            ema_loss_for_log = 0.4 * loss.item() + 0.6 * ema_loss_for_log
            if tb_writer:
                tb_writer.add_scalar("train_loss_patches/total_loss", loss.item(), iteration)
            if progress_bar is not None:
                progress_bar.set_postfix({"Loss": f"{ema_loss_for_log:.7f}"})
                progress_bar.update(10)
        if iteration == opt.iterations and progress_bar is not None:
            progress_bar.close()
        if iteration in checkpoint_iterations:
            print(f"\n[ITER {iteration}] Saving Checkpoint")
            torch.save((gaussians.capture(), iteration), os.path.join(scene.model_path, f"chkpnt{iteration}.pth"))
    return scene


def prepare_output_and_logger(args):
    if not args.model_path:
        unique_str = os.getenv("OAR_JOB_ID") or str(uuid.uuid4())
        args.model_path = os.path.join("./output/", unique_str[0:10])
    print(f"Output folder: {args.model_path}")
    os.makedirs(args.model_path, exist_ok=True)
    with open(os.path.join(args.model_path, "cfg_args"), "w") as f:
        f.write(str(Namespace(**vars(args))))
    if TENSORBOARD_FOUND:
        return SummaryWriter(args.model_path)
    print("Tensorboard not available: not logging progress")
    return None


@torch.no_grad()
def training_report(tb_writer, iteration, testing_iterations, scene, pipe, background, train_test_exp):
    """L1 and PSNR over the test cameras and five training cameras at the ``--test_iterations``."""
    if iteration not in testing_iterations:
        return
    from gaussian_renderer import render
    from utils.image_utils import psnr
    from utils.loss_utils import l1_loss

    train = scene.getTrainCameras()
    configs = ({"name": "test", "cameras": scene.getTestCameras()},
               {"name": "train", "cameras": [train[idx % len(train)] for idx in range(5, 30, 5)] if train else []})
    for config in configs:
        if not config["cameras"]:
            continue
        l1_test = psnr_test = 0.0
        for viewpoint in config["cameras"]:
            image = render(viewpoint, scene.gaussians, pipe, background, use_trained_exp=train_test_exp)["render"]
            image = torch.clamp(image, 0.0, 1.0)
            gt_image = torch.clamp(viewpoint.original_image.to("cuda"), 0.0, 1.0)
            if train_test_exp:  # (the exposure of a view was fitted on its left half: the right half is scored)
                image = image[..., image.shape[-1] // 2:]
                gt_image = gt_image[..., gt_image.shape[-1] // 2:]
            l1_test += l1_loss(image, gt_image).mean().double().item()
            psnr_test += psnr(image, gt_image).mean().double().item()
        l1_test /= len(config["cameras"])
        psnr_test /= len(config["cameras"])
        print(f"\n[ITER {iteration}] Evaluating {config['name']}: L1 {l1_test} PSNR {psnr_test}")
        if tb_writer:
            tb_writer.add_scalar(config["name"] + "/loss_viewpoint - l1_loss", l1_test, iteration)
            tb_writer.add_scalar(config["name"] + "/loss_viewpoint - psnr", psnr_test, iteration)
    if tb_writer:
        tb_writer.add_scalar("total_points", scene.gaussians.get_xyz.shape[0], iteration)


def build_parser():
    parser = ArgumentParser(description="Training script parameters")
    lp = ModelParams(parser)
    op = OptimizationParams(parser)
    pp = PipelineParams(parser)
    parser.add_argument("--ip", type=str, default="127.0.0.1", help="accepted and ignored: there is no network viewer")
    parser.add_argument("--port", type=int, default=6009, help="accepted and ignored")
    parser.add_argument("--debug_from", type=int, default=-1)
    parser.add_argument("--detect_anomaly", action="store_true", default=False)
    parser.add_argument("--test_iterations", nargs="+", type=int, default=[7_000, 30_000])
    parser.add_argument("--save_iterations", nargs="+", type=int, default=[7_000, 30_000])
    parser.add_argument("--quiet", action="store_true")
    parser.add_argument("--disable_viewer", action="store_true", default=False, help="accepted and ignored")
    parser.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[])
    parser.add_argument("--start_checkpoint", type=str, default=None)
    parser.add_argument("--fused_activations", action="store_true", default=False,
                        help="sigmoid / exp / normalize and their chain rule inside the rasterizer's kernels")
    parser.add_argument("--composed_loss", action="store_true", default=False,
                        help="build the loss from torch operations and fused_ssim as upstream does, instead of the fused "
                             "gsworld_amd.ssim.training_loss")
    return parser, lp, op, pp


def main(argv=None):
    parser, lp, op, pp = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    args.save_iterations.append(args.iterations)
    print("Optimizing " + args.model_path)
    safe_state(args.quiet)
    torch.autograd.set_detect_anomaly(args.detect_anomaly)
    pipe = pp.extract(args)
    pipe.fused_activations = bool(args.fused_activations)
    training(lp.extract(args), op.extract(args), pipe, args.test_iterations, args.save_iterations,
             args.checkpoint_iterations, args.start_checkpoint, args.debug_from, composed_loss=args.composed_loss)
    print("\nTraining complete.")


if __name__ == "__main__":
    main()
