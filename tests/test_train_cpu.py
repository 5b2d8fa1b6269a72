"""The python layer ``train.py`` stands on, as far as it runs without a device: COLMAP readers against bytes packed here,
the learning-rate schedule, the scene normalisation, ``cameras.json`` entries, the argument groups and the C ABI's refusals."""
import ctypes as C
import math
import os
import subprocess
import sys
from argparse import ArgumentParser, Namespace

import numpy as np
import pytest

from tests import colmap_fixture as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def gs_paths():
    added = [os.path.join(ROOT, "gsworld_amd", "dropin"), os.path.join(ROOT, "gsworld_amd", "gs_compat")]
    for p in added:
        sys.path.insert(0, p)
    yield
    for p in added:
        sys.path.remove(p)


Q90Z = (math.sqrt(0.5), 0.0, 0.0, math.sqrt(0.5))
CAMERAS = [(1, 1, 640, 480, (500.5, 501.25, 320.0, 240.5)), (7, 0, 1920, 1080, (1400.125, 960.0, 540.0))]
IMAGES = [
    (1, (1.0, 0.0, 0.0, 0.0), (0.1, -0.2, 0.3), 1, "a.png", [(10.5, 20.25, 3), (1.0, 2.0, -1)]),
    (2, Q90Z, (1.5, 2.5, -3.5), 7, "sub/frame.0002.jpg", [(0.125, 7.0, 11)]),
    (5, (0.5, 0.5, 0.5, 0.5), (0.0, 0.0, 1.0), 1, "c.JPG", [(3.0, 4.0, 3), (5.0, 6.0, 4), (7.5, 8.5, -1)]),
]
POINTS = [
    (3, (0.5, -1.5, 2.25), (255, 0, 17), 0.75, [(1, 0), (5, 0)]),
    (4, (1.0, 2.0, 3.0), (1, 2, 3), 1.5, [(5, 1)]),
    (11, (-4.0, 0.0, 0.125), (128, 64, 32), 0.0, [(2, 0), (1, 1), (5, 2)]),
    (12, (9.0, 8.0, 7.0), (0, 0, 0), 2.0, []),
]


def _check_records(cams, imgs, pts, arrays):
    assert sorted(cams) == [1, 7]
    for cid, model, w, h, params in CAMERAS:
        c = cams[cid]
        assert (c.id, c.model, c.width, c.height) == (cid, cf.MODEL_PARAMS[model][0], w, h)
        assert c.params.tolist() == list(params)
    assert sorted(imgs) == [1, 2, 5]
    for iid, q, t, cid, name, p2d in IMAGES:
        im = imgs[iid]
        assert (im.id, im.camera_id, im.name) == (iid, cid, name)
        assert im.qvec.tolist() == list(q) and im.tvec.tolist() == list(t)
        assert im.xys.shape == (len(p2d), 2) and im.xys.tolist() == [[x, y] for x, y, _ in p2d]
        assert im.point3D_ids.tolist() == [pid for _, _, pid in p2d]
    assert sorted(pts) == [3, 4, 11, 12]
    for pid, xyz, rgb, err, track in POINTS:
        p = pts[pid]
        assert p.xyz.tolist() == list(xyz) and p.rgb.tolist() == list(rgb) and p.error == err
        assert p.image_ids.tolist() == [a for a, _ in track] and p.point2D_idxs.tolist() == [b for _, b in track]
    xyz, rgb, err = arrays
    assert xyz.tolist() == [list(p[1]) for p in POINTS] and rgb.tolist() == [list(p[2]) for p in POINTS]
    assert err.tolist() == [[p[3]] for p in POINTS]


def test_colmap_readers_binary_and_text(gs_paths, tmp_path):
    from scene import colmap_loader as cl

    b = {n: str(tmp_path / f"{n}.bin") for n in ("cameras", "images", "points3D")}
    t = {n: str(tmp_path / f"{n}.txt") for n in ("cameras", "images", "points3D")}
    cf.write_cameras_bin(b["cameras"], CAMERAS)
    cf.write_images_bin(b["images"], IMAGES)
    cf.write_points3D_bin(b["points3D"], POINTS)
    cf.write_cameras_txt(t["cameras"], CAMERAS)
    cf.write_images_txt(t["images"], IMAGES)
    cf.write_points3D_txt(t["points3D"], POINTS)
    _check_records(cl.read_intrinsics_binary(b["cameras"]), cl.read_extrinsics_binary(b["images"]),
                   cl.read_points3D_records_binary(b["points3D"]), cl.read_points3D_binary(b["points3D"]))
    _check_records(cl.read_intrinsics_text(t["cameras"]), cl.read_extrinsics_text(t["images"]),
                   cl.read_points3D_records_text(t["points3D"]), cl.read_points3D_text(t["points3D"]))
    # the file's size is what the layout says: nothing read past it, nothing left
    assert os.path.getsize(b["images"]) == 8 + sum(4 + 56 + 4 + len(i[4]) + 1 + 8 + 24 * len(i[5]) for i in IMAGES)
    assert os.path.getsize(b["points3D"]) == 8 + sum(8 + 24 + 3 + 8 + 8 + 8 * len(p[4]) for p in POINTS)
    opencv = [(1, 4, 640, 480, (500.0, 500.0, 320.0, 240.0, 0.1, 0.01, 0.0, 0.0))]
    cf.write_cameras_bin(b["cameras"], opencv)
    cf.write_cameras_txt(t["cameras"], opencv)
    for read, path in ((cl.read_intrinsics_binary, b["cameras"]), (cl.read_intrinsics_text, t["cameras"])):
        with pytest.raises(AssertionError, match="undistorted"):
            read(path)


def test_qvec2rotmat(gs_paths):
    from scene.colmap_loader import qvec2rotmat

    assert np.array_equal(qvec2rotmat((1, 0, 0, 0)), np.eye(3))
    np.testing.assert_allclose(qvec2rotmat(Q90Z), [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    R = qvec2rotmat(cf.rotmat_to_qvec(qvec2rotmat((0.5, -0.5, 0.5, 0.5))))
    np.testing.assert_allclose(R, qvec2rotmat((0.5, -0.5, 0.5, 0.5)), atol=1e-15)


def test_expon_lr_func(gs_paths):
    from arguments import OptimizationParams
    from utils.general_utils import get_expon_lr_func

    init, final, mx = 3e-3, 7e-6, 4000
    f = get_expon_lr_func(init, final, max_steps=mx)
    rel = lambda a, b: abs(a - b) / abs(b)  # noqa: E731
    assert rel(f(0), init) < 1e-12 and rel(f(mx), final) < 1e-12 and rel(f(mx / 2), math.sqrt(init * final)) < 1e-12
    assert rel(f(10 * mx), final) < 1e-12 and f(-1) == 0.0
    d = get_expon_lr_func(init, final, lr_delay_steps=100, lr_delay_mult=0.01, max_steps=mx)
    assert rel(d(0), 0.01 * init) < 1e-12 and rel(d(100), f(100)) < 1e-12 and d(50) < f(50)
    assert get_expon_lr_func(0.0, 0.0)(5) == 0.0
    op = OptimizationParams(ArgumentParser())
    g = get_expon_lr_func(op.position_lr_init, op.position_lr_final, lr_delay_mult=op.position_lr_delay_mult,
                          max_steps=op.position_lr_max_steps)
    assert rel(g(0), 1.6e-4) < 1e-12 and rel(g(30_000), 1.6e-6) < 1e-12 and op.position_lr_max_steps == 30_000


def _info(R, T, name="x.png"):
    from scene.dataset_readers import CameraInfo

    return CameraInfo(uid=1, R=R, T=T, FovY=0.9, FovX=1.1, depth_params=None, image_path="", image_name=name, depth_path="",
                      width=640, height=480, is_test=False)


def test_nerfpp_norm_and_camera_json(gs_paths):
    from scene.colmap_loader import qvec2rotmat
    from scene.dataset_readers import getNerfppNorm
    from utils.camera_utils import camera_to_JSON
    from utils.graphics_utils import fov2focal

    # four centres at the corners of a square of side 2 about (1, 2, 3), every camera turned by 90 degrees about z
    Rw2c = qvec2rotmat(Q90Z)
    corners = [np.array([1.0 + sx, 2.0 + sy, 3.0]) for sx in (-1, 1) for sy in (-1, 1)]
    infos = [_info(Rw2c.T, -Rw2c @ c) for c in corners]  # (R is stored transposed; T = -R_w2c C)
    norm = getNerfppNorm(infos)
    np.testing.assert_allclose(norm["translate"], [-1.0, -2.0, -3.0], atol=1e-6)
    assert abs(norm["radius"] - 1.1 * math.sqrt(2.0)) < 1e-6
    j = camera_to_JSON(4, infos[0])
    assert list(j) == ["id", "img_name", "width", "height", "position", "rotation", "fy", "fx"]
    assert (j["id"], j["img_name"], j["width"], j["height"]) == (4, "x.png", 640, 480)
    np.testing.assert_allclose(j["position"], corners[0], atol=1e-12)
    np.testing.assert_allclose(j["rotation"], Rw2c.T, atol=1e-12)  # camera-to-world
    assert j["fy"] == fov2focal(0.9, 480) and j["fx"] == fov2focal(1.1, 640)


def test_store_ply_writes_uchar_colours(gs_paths, tmp_path):
    from scene.dataset_readers import fetchPly, storePly

    xyz = np.array([[0.5, -1.5, 2.25], [1.0, 2.0, 3.0]])
    rgb = np.array([[255, 0, 17], [1, 2, 3]])
    path = str(tmp_path / "points3D.ply")
    storePly(path, xyz, rgb)
    raw = open(path, "rb").read()
    header, body = raw.split(b"end_header\n")
    assert b"property uchar red" in header and b"property float x" in header and b"property float nz" in header
    assert len(body) == 2 * (6 * 4 + 3) and body[24:27] == bytes([255, 0, 17])
    pcd = fetchPly(path)
    assert np.array_equal(pcd.points, xyz.astype(np.float32)) and np.array_equal(pcd.colors, rgb.astype(np.float32) / 255.0)
    assert pcd.normals.shape == (2, 3) and not pcd.normals.any()


def test_held_out_views_are_split_in_halves_under_train_test_exp(gs_paths, tmp_path):
    """``--eval --train_test_exp``: a held-out view sits in BOTH camera lists; the training copy keeps its left half (the
    exposure is fitted there), the test copy its right half (scored there); other views and other settings get no mask."""
    from PIL import Image

    from utils.camera_utils import cameraList_from_camInfos

    W, H = 10, 6
    Image.fromarray(np.full((H, W, 3), 200, np.uint8)).save(tmp_path / "rgb.png")
    rgba = np.full((H, W, 4), 200, np.uint8)
    rgba[:, 2:, 3] = 255
    rgba[:, :2, 3] = 0
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    la = np.full((H, W, 2), 200, np.uint8)
    Image.fromarray(la, mode="LA").save(tmp_path / "la.png")

    def info(name, is_test):
        return _info(np.eye(3), np.zeros(3), name)._replace(image_path=str(tmp_path / name), width=W, height=H,
                                                            is_test=is_test)

    args = Namespace(resolution=1, data_device="cpu", train_test_exp=True)
    infos = [info("rgb.png", True), info("rgba.png", True), info("rgb.png", False)]
    train = cameraList_from_camInfos(infos, 1.0, args, False, False)
    test = cameraList_from_camInfos(infos[:2], 1.0, args, False, True)
    ones = np.ones((1, H, W), np.float32)
    left, right = ones.copy(), ones.copy()
    left[..., W // 2:] = 0
    right[..., :W // 2] = 0
    assert np.array_equal(train[0].alpha_mask.numpy(), left) and np.array_equal(test[0].alpha_mask.numpy(), right)
    own = ones.copy()
    own[..., :2] = 0  # (the PNG's own alpha stays under the half mask)
    assert np.array_equal(train[1].alpha_mask.numpy(), left * own) and np.array_equal(test[1].alpha_mask.numpy(), right * own)
    assert train[2].alpha_mask is None
    assert tuple(train[1].original_image.shape) == (3, H, W)
    off = cameraList_from_camInfos(infos, 1.0, Namespace(resolution=1, data_device="cpu", train_test_exp=False), False, False)
    assert off[0].alpha_mask is None and np.array_equal(off[1].alpha_mask.numpy(), own)
    # a two-band image (grey + alpha) has no fourth channel to take a mask from
    two = cameraList_from_camInfos([info("la.png", False)], 1.0, args, False, False)
    assert two[0].alpha_mask is None


def test_argument_groups(gs_paths, tmp_path):
    from arguments import ModelParams, OptimizationParams, PipelineParams, get_combined_args

    parser = ArgumentParser()
    lp, op, pp = ModelParams(parser), OptimizationParams(parser), PipelineParams(parser)
    args = parser.parse_args(["-s", "X", "-m", "Y", "--iterations", "5", "-r", "2"])
    m, o = lp.extract(args), op.extract(args)
    assert m.source_path == os.path.abspath("X") and m.model_path == "Y" and m.resolution == 2 and o.iterations == 5
    assert (m.sh_degree, m.images, m.depths, m.white_background, m.train_test_exp, m.data_device, m.eval) == \
        (3, "images", "", False, False, "cuda", False)
    want = dict(position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
                position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.025, scaling_lr=0.005, rotation_lr=0.001,
                exposure_lr_init=0.01, exposure_lr_final=0.001, exposure_lr_delay_steps=0, exposure_lr_delay_mult=0.0,
                percent_dense=0.01, lambda_dssim=0.2, densification_interval=100, opacity_reset_interval=3000,
                densify_from_iter=500, densify_until_iter=15_000, densify_grad_threshold=0.0002, depth_l1_weight_init=1.0,
                depth_l1_weight_final=0.01, random_background=False, optimizer_type="default")
    assert {k: getattr(o, k) for k in want} == want and OptimizationParams(ArgumentParser()).iterations == 30_000
    assert vars(pp.extract(args)) == dict(convert_SHs_python=False, compute_cov3D_python=False, debug=False,
                                          antialiasing=False)
    for flag in ("-i", "-d", "-w"):
        assert flag in parser.format_help()
    # PipelineParams() without a parser: as ever
    p0 = PipelineParams()
    assert (p0.convert_SHs_python, p0.compute_cov3D_python, p0.debug, p0.antialiasing) == (False, False, False, False)
    # cfg_args written by the trainer merges under the command line
    (tmp_path / "cfg_args").write_text(str(Namespace(sh_degree=2, source_path="/data/scene", model_path="old", eval=True)))
    p2 = ArgumentParser()
    ModelParams(p2, sentinel=True)
    merged = get_combined_args(p2, ["-m", str(tmp_path)])
    assert merged.sh_degree == 2 and merged.source_path == "/data/scene" and merged.eval is True
    assert merged.model_path == str(tmp_path)


def test_train_help_runs_without_a_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gsworld_amd", "gs_compat", "train.py"), "--help"],
                       capture_output=True, text=True, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr
    for flag in ("--source_path", "--iterations", "--test_iterations", "--save_iterations", "--checkpoint_iterations",
                 "--start_checkpoint", "--disable_viewer", "--ip", "--port", "--quiet", "--detect_anomaly", "--debug_from",
                 "--fused_activations", "--composed_loss", "--optimizer_type", "--train_test_exp", "--eval"):
        assert flag in r.stdout, flag


def test_train_loss_symbols_and_refusals():
    from gsworld_amd import _lib

    from gsworld_amd import _C

    names = {"gsr_train_loss", "gsr_train_loss_backward", "gsr_train_loss_scratch_floats", "gsr_train_loss_scratch_needed"}
    assert names <= set(_lib.exported_symbols())
    L = _lib.lib()
    assert all(hasattr(L, n) for n in names)
    E = _lib.GSR_E_INVALID
    assert L.gsr_train_loss(None, None) == E and L.gsr_train_loss_backward(None, None) == E
    assert L.gsr_train_loss_scratch_floats(0, 16) == 0 and L.gsr_train_loss_scratch_floats(16, 16) > 4 * 3 * 256
    P = 256  # (never dereferenced: every call below is refused first)

    def args(**kw):
        a = _lib.GsrTrainLoss(struct_size=C.sizeof(_lib.GsrTrainLoss), H=16, W=16, lambda_dssim=0.2, color=P, target=P,
                              scratch=P, loss=P)
        for k, v in kw.items():
            setattr(a, k, v)
        if "scratch_floats" not in kw:
            a.scratch_floats = L.gsr_train_loss_scratch_needed(C.byref(a)) 
        return a

    # what a call needs: less without exposure and alpha mask, never more than the bound for the size
    plain, masked, full = (L.gsr_train_loss_scratch_needed(C.byref(args(**kw)))
                           for kw in (dict(), dict(alpha_mask=P), dict(alpha_mask=P, exposure=P)))
    assert 0 < plain < masked < full == L.gsr_train_loss_scratch_floats(16, 16)
    assert masked - plain == 3 * 256 and L.gsr_train_loss_scratch_needed(None) == 0
    assert _C.train_loss_scratch_needed(16, 16, False, False) == plain
    assert _C.train_loss_scratch_needed(16, 16, True, True) == full
    for size in (4, C.sizeof(_lib.GsrTrainLoss) + 8):
        assert L.gsr_train_loss(C.byref(args(struct_size=size)), None) == E and b"struct_size" in L.gsr_last_error()
    for kw in (dict(H=0), dict(W=-1), dict(color=None), dict(target=None), dict(scratch=None), dict(loss=None),
               dict(invdepth=P), dict(invdepth=P, mono_invdepth=P), dict(lambda_dssim=float("nan")),
               dict(depth_weight=float("inf")), dict(scratch_floats=plain - 1), dict(exposure=P, scratch_floats=full - 1),
               dict(alpha_mask=P, scratch_floats=plain), dict(scratch=P + 4)):
        assert L.gsr_train_loss(C.byref(args(**kw)), None) == E, kw
    assert b"8-byte" in L.gsr_last_error()
    for kw in (dict(), dict(dL_dcolor=P, exposure=P), dict(dL_dcolor=P, invdepth=P, mono_invdepth=P, depth_mask=P)):
        assert L.gsr_train_loss_backward(C.byref(args(**kw)), None) == E, kw
