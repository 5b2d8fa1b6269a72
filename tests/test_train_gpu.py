"""``gs_compat/train.py`` end to end on a synthetic capture (tests/colmap_fixture.py): the capture loads, an iteration reads
nothing from the device, 300 iterations train -- with the fused loss at least half as many dB as with upstream's composition
(``--composed_loss``, the reference) --, the output folder is what the merger and a resumed run read, and the exposure and
depth terms act."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from tests import colmap_fixture as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gs_paths():
    added = [os.path.join(ROOT, "gsworld_amd", "dropin"), os.path.join(ROOT, "gsworld_amd", "gs_compat")]
    for p in added:
        sys.path.insert(0, p)
    yield
    for p in added:
        sys.path.remove(p)


@pytest.fixture(scope="module")
def capture(cuda_device, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("capture"))
    return root, cf.build_capture(root, cuda_device)


@pytest.fixture(scope="module")
def capture_exp_depth(cuda_device, tmp_path_factory):
    """The same capture with view 2 darkened by a gain of 0.5, and monocular inverse depths (the ground truth's own)."""
    root = str(tmp_path_factory.mktemp("capture_exp_depth"))
    return root, cf.build_capture(root, cuda_device, gains={2: 0.5}, depths=True)


def parse(argv):
    import train

    parser, lp, op, pp = train.build_parser()
    args = parser.parse_args(argv)
    pipe = pp.extract(args)
    pipe.fused_activations = bool(args.fused_activations)
    return args, lp.extract(args), op.extract(args), pipe


def run_training(argv, save=(), checkpoints=(), test=(), composed=False):
    import train
    from utils.general_utils import safe_state

    args, dataset, opt, pipe = parse(argv)
    safe_state(False)
    scene = train.training(dataset, opt, pipe, list(test), list(save), list(checkpoints), args.start_checkpoint, -1,
                           composed_loss=composed)
    return scene, pipe


@torch.no_grad()
def mean_psnr(scene, pipe, train_test_exp=False):
    from gaussian_renderer import render
    from utils.image_utils import psnr

    bg = torch.zeros(3, device="cuda")
    vals = [psnr(render(cam, scene.gaussians, pipe, bg, use_trained_exp=train_test_exp)["render"],
                 cam.original_image.cuda()).mean() for cam in scene.getTrainCameras()]
    return float(torch.stack(vals).mean())


def test_scene_loads_the_capture(gs_paths, capture, tmp_path):
    from scene import GaussianModel, Scene
    from scene.dataset_readers import readColmapSceneInfo

    root, truth = capture
    info = readColmapSceneInfo(root, "images", "", False, False)
    assert len(info.train_cameras) == 8 and len(info.test_cameras) == 0 and len(info.point_cloud.points) == 500
    centre = truth["centres"].mean(0)
    extent = 1.1 * np.linalg.norm(truth["centres"] - centre, axis=1).max()
    assert abs(info.nerf_normalization["radius"] - extent) < 1e-6
    args, dataset, opt, pipe = parse(["-s", root, "-m", str(tmp_path)])
    scene = Scene(dataset, GaussianModel(3), shuffle=True)
    cams = scene.getTrainCameras()
    assert len(cams) == 8 and scene.getTestCameras() == [] and abs(scene.cameras_extent - extent) < 1e-6
    assert scene.gaussians.get_xyz.shape == (500, 3) and scene.gaussians._exposure.shape == (8, 3, 4)
    for cam in cams:
        k = truth["names"].index(cam.image_name)
        want = truth["views"][k]
        assert (cam.image_width, cam.image_height) == (64, 64) and abs(cam.FoVx - want.FoVx) < 1e-12
        assert float((cam.world_view_transform.cpu() - want.world_view_transform).abs().max()) <= 1e-6
        assert float((cam.original_image.cpu() - truth["images"][k]).abs().max()) < 1e-6
    assert len(json.load(open(tmp_path / "cameras.json"))) == 8 and (tmp_path / "input.ply").exists()


@pytest.mark.parametrize("with_exposure_and_depth", [False, True])
def test_training_step_reads_nothing_from_the_device(gs_paths, capture, capture_exp_depth, tmp_path, with_exposure_and_depth):
    import train
    from scene import GaussianModel, Scene

    root = (capture_exp_depth if with_exposure_and_depth else capture)[0]
    argv = ["-s", root, "-m", str(tmp_path), "--optimizer_type", "sparse_adam", "--fused_activations"]
    if with_exposure_and_depth:
        argv += ["--train_test_exp", "-d", "depths"]
    args, dataset, opt, pipe = parse(argv)
    gaussians = GaussianModel(3, opt.optimizer_type)
    scene = Scene(dataset, gaussians, shuffle=False)
    gaussians.training_setup(opt)
    cams = scene.getTrainCameras()
    bg = torch.zeros(3, device="cuda")
    if with_exposure_and_depth:
        assert all(c.depth_reliable and c.invdepthmap is not None and c.depth_mask is not None for c in cams)
    for cam in cams:
        cam.original_image  # (the lazy conversion of the PNG: once per camera, outside the loop)
    kw = dict(train_test_exp=with_exposure_and_depth, depth_weight=1.0 if with_exposure_and_depth else 0.0)
    xyz0 = gaussians.get_xyz.detach().clone()
    train.training_step(gaussians, cams[0], 1, opt, pipe, bg, **kw)  # (warm-up: code objects, allocator)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for it in range(2, 32):
            loss = train.training_step(gaussians, cams[it % 8], it, opt, pipe, bg, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert loss.shape == () and math.isfinite(float(loss)) and not torch.equal(gaussians.get_xyz.detach(), xyz0)
    assert float(gaussians.denom.sum()) > 0  # (the densification statistics were kept on the way)
    if with_exposure_and_depth:
        assert not torch.equal(gaussians._exposure.detach()[0].cpu(), torch.eye(3, 4))


E2E = ["--iterations", "300", "--densify_from_iter", "100", "--densification_interval", "100", "--opacity_reset_interval",
       "3000", "--optimizer_type", "sparse_adam"]


@pytest.fixture(scope="module")
def trained(gs_paths, capture, tmp_path_factory):
    """Both 300-iteration runs from the same seed, and the model before iteration 1."""
    import scene as scene_mod

    root = capture[0]
    out = {k: str(tmp_path_factory.mktemp(k)) for k in ("init", "fused", "composed")}
    init, pipe = run_training(["-s", root, "-m", out["init"], "--optimizer_type", "sparse_adam", "--iterations", "0"])
    res = {"out": out, "psnr_before": mean_psnr(init, pipe), "saved_n": {}}
    orig_save = scene_mod.Scene.save

    def save(self, iteration):
        res["saved_n"][self.model_path] = int(self.gaussians.get_xyz.shape[0])
        return orig_save(self, iteration)

    scene_mod.Scene.save = save
    try:
        for name in ("fused", "composed"):
            scene, pipe = run_training(["-s", root, "-m", out[name]] + E2E, save=[300], checkpoints=[200], test=[300],
                                       composed=name == "composed")
            res["psnr_" + name] = mean_psnr(scene, pipe)
            res["n_" + name] = int(scene.gaussians.get_xyz.shape[0])
    finally:
        scene_mod.Scene.save = orig_save
    print("TRAIN_SYNTHETIC " + json.dumps({k: v for k, v in res.items() if k.startswith(("psnr", "n_"))}))
    return res


def test_fused_loss_trains_as_the_composed_loss_does(trained):
    """Mean PSNR over the 8 training views before iteration 1 and after iteration 300, sparse_adam, densification at 200 and
    300 (the model as the loop leaves it, the last densification included).  Measured on the MI355X: before 15.62 dB;
    composed 18.76 dB; fused 18.76 dB (gains 3.14 and 3.14 dB; profiles/train/train_synthetic.json)."""
    before, fused, composed = trained["psnr_before"], trained["psnr_fused"], trained["psnr_composed"]
    print(f"PSNR before {before:.3f} dB; after 300 iterations: composed {composed:.3f} dB, fused {fused:.3f} dB")
    assert composed > before  # (a condition on the fixture)
    assert fused - before >= 0.5 * (composed - before)


def test_output_folder(gs_paths, capture, trained, cuda_device):
    from argparse import ArgumentParser

    from arguments import ModelParams, get_combined_args
    from scene import GaussianModel, Scene

    from gsworld_amd.ply import read_gaussian_ply

    out = trained["out"]["fused"]
    for name in ("cfg_args", "cameras.json", "input.ply", "point_cloud/iteration_300/point_cloud.ply",
                 "exposure.json", "chkpnt200.pth"):
        assert os.path.exists(os.path.join(out, name)), name
    assert len(json.load(open(os.path.join(out, "cameras.json")))) == 8
    assert len(json.load(open(os.path.join(out, "exposure.json")))) == 8
    n = trained["saved_n"][out]
    assert n > 0
    ply = os.path.join(out, "point_cloud/iteration_300/point_cloud.ply")
    a = GaussianModel(3)
    a.load_ply(ply)

    class Bare:
        max_sh_degree = 3

    b = Bare()
    read_gaussian_ply(ply, b, device=cuda_device)
    for m in (a, b):
        assert m._xyz.shape == (n, 3) and m._features_rest.shape == (n, 15, 3)
        for t in (m._xyz, m._features_dc, m._features_rest, m._opacity, m._scaling, m._rotation):
            assert bool(torch.isfinite(t).all())
    parser = ArgumentParser()
    ModelParams(parser, sentinel=True)
    merged = get_combined_args(parser, ["-m", out])
    assert merged.source_path == os.path.abspath(capture[0]) and merged.sh_degree == 3 and merged.model_path == out
    again = Scene(merged, GaussianModel(3), load_iteration=-1, shuffle=False)
    assert again.loaded_iter == 300 and again.gaussians.get_xyz.shape == (n, 3) and len(again.getTrainCameras()) == 8


def test_resume_from_a_checkpoint(gs_paths, capture, trained, tmp_path, monkeypatch):
    import train

    seen = []
    step = train.training_step

    def recording(gaussians, cam, iteration, *a, **kw):
        seen.append((iteration, int(gaussians.get_xyz.shape[0])))
        return step(gaussians, cam, iteration, *a, **kw)

    monkeypatch.setattr(train, "training_step", recording)
    ckpt = os.path.join(trained["out"]["fused"], "chkpnt200.pth")
    scene, _ = run_training(["-s", capture[0], "-m", str(tmp_path), "--start_checkpoint", ckpt] + E2E)
    assert [s[0] for s in seen] == list(range(201, 301))
    assert seen[0][1] != 500  # (the checkpoint's model -- densified at 200 --, not the sparse points)
    assert bool(torch.isfinite(scene.gaussians.get_xyz).all())


def test_exposure_and_depth_terms_act(gs_paths, capture_exp_depth, tmp_path_factory):
    """300 iterations with ``--train_test_exp`` on the capture whose view 2 is darkened by 0.5: every visit of a view moves
    its exposure by about the exposure learning rate (Adam, 0.01 -> 0.001) while the gradient keeps its sign, and a view is
    visited about 37 times, so the darkened view's gain (mean diagonal of its 3 x 3) must end at least 0.05 below every
    other view's.

    The depth term: two runs from the same seed that differ in nothing but the term (the ground truth's own inverse depths
    as the monocular ones, every pixel in the mask, the weight held at 10 where upstream decays 1 -> 0.01: no densification
    before iteration 500, so both keep the 500 initial Gaussians).  The mean |rendered - monocular| inverse depth over all
    pixels of the 8 views must end at least 1 % lower with the term.  The margin is set against what else separates two such
    runs -- float32 rounding and the order of atomic sums, which moved the final PSNR of two identical runs by 0.001 dB in
    18.76 dB, i.e. below 0.01 % -- and not against the size of the effect.

    Measured on the MI355X: gain of the darkened view 0.839, the others 1.005 .. 1.032; depth error 0.06872 with the term,
    0.07275 without (5.5 % lower)."""
    from gaussian_renderer import render

    root, truth = capture_exp_depth
    common = ["-s", root, "--iterations", "300", "--optimizer_type", "sparse_adam", "--train_test_exp"]
    common += ["--depth_l1_weight_init", "10", "--depth_l1_weight_final", "10"]
    with_d, pipe = run_training(common + ["-m", str(tmp_path_factory.mktemp("with_depth")), "-d", "depths"])
    without, _ = run_training(common + ["-m", str(tmp_path_factory.mktemp("without_depth"))])
    g = with_d.gaussians
    gain = {name: float(g.get_exposure_from_name(name).detach()[:3, :3].diagonal().mean()) for name in truth["names"]}
    dark = gain.pop(truth["names"][2])
    print(f"gain of the darkened view {dark:.3f}; the others {sorted(gain.values())}")
    assert dark < min(gain.values()) - 0.05

    @torch.no_grad()
    def depth_error(scene):
        bg = torch.zeros(3, device="cuda")
        cams = {c.image_name: c for c in with_d.getTrainCameras()}  # (the cameras that carry the depth maps)
        return float(torch.stack([(render(c, scene.gaussians, pipe, bg)["depth"] - c.invdepthmap.cuda()).abs().mean()
                                  for c in cams.values()]).mean())

    e_with, e_without = depth_error(with_d), depth_error(without)
    print(f"mean |invdepth - mono|: with the depth term {e_with:.5f}, without {e_without:.5f}")
    assert e_with <= 0.99 * e_without
