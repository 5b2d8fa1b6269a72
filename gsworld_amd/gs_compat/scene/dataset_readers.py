"""``scene.dataset_readers``: a COLMAP capture on disk -> ``SceneInfo`` (camera records, the initial point cloud, the
normalisation the learning rates and densification limits are scaled by).  The Blender reader is not provided."""
import json
import os
import sys
from typing import NamedTuple

import numpy as np

from scene.colmap_loader import (qvec2rotmat, read_extrinsics_binary, read_extrinsics_text, read_intrinsics_binary,
                                 read_intrinsics_text, read_points3D_binary, read_points3D_text)
from utils.graphics_utils import BasicPointCloud, focal2fov, getWorld2View2


class CameraInfo(NamedTuple):
    uid: int
    R: np.array
    T: np.array
    FovY: np.array
    FovX: np.array
    depth_params: dict
    image_path: str
    image_name: str
    depth_path: str
    width: int
    height: int
    is_test: bool


class SceneInfo(NamedTuple):
    point_cloud: BasicPointCloud
    train_cameras: list
    test_cameras: list
    nerf_normalization: dict
    ply_path: str
    is_nerf_synthetic: bool


def getNerfppNorm(cam_info):
    """translate = -(mean camera centre); radius = 1.1 x the largest distance of a centre from that mean."""
    centres = []
    for cam in cam_info:
        C2W = np.linalg.inv(getWorld2View2(cam.R, cam.T))
        centres.append(C2W[:3, 3:4])
    centres = np.hstack(centres)
    centre = centres.mean(axis=1, keepdims=True)
    diagonal = np.linalg.norm(centres - centre, axis=0).max()
    return {"translate": -centre.flatten(), "radius": diagonal * 1.1}


def readColmapCameras(cam_extrinsics, cam_intrinsics, depths_params, images_folder, depths_folder, test_cam_names_list):
    cam_infos = []
    for idx, key in enumerate(cam_extrinsics):
        extr = cam_extrinsics[key]
        intr = cam_intrinsics[extr.camera_id]
        height, width = intr.height, intr.width
        R = np.transpose(qvec2rotmat(extr.qvec))
        T = np.array(extr.tvec)
        if intr.model == "SIMPLE_PINHOLE":
            FovY, FovX = focal2fov(intr.params[0], height), focal2fov(intr.params[0], width)
        elif intr.model == "PINHOLE":
            FovY, FovX = focal2fov(intr.params[1], height), focal2fov(intr.params[0], width)
        else:
            raise AssertionError("Colmap camera model not handled: only undistorted datasets (PINHOLE or SIMPLE_PINHOLE "
                                 "cameras) supported!")
        n_remove = len(extr.name.split(".")[-1]) + 1
        depth_params = None
        if depths_params is not None:
            try:
                depth_params = depths_params[extr.name[:-n_remove]]
            except KeyError:
                print("\n", key, "not found in depths_params")
        image_path = os.path.join(images_folder, extr.name)
        depth_path = os.path.join(depths_folder, f"{extr.name[:-n_remove]}.png") if depths_folder != "" else ""
        cam_infos.append(CameraInfo(uid=intr.id, R=R, T=T, FovY=FovY, FovX=FovX, depth_params=depth_params,
                                    image_path=image_path, image_name=extr.name, depth_path=depth_path, width=width,
                                    height=height, is_test=extr.name in test_cam_names_list))
    return cam_infos


def fetchPly(path):
    """x y z [nx ny nz] red green blue of a binary little-endian PLY -> BasicPointCloud (colours in [0, 1])."""
    from gsworld_amd.ply import read_ply

    c = read_ply(path)
    xyz = np.stack((c["x"], c["y"], c["z"]), axis=1)
    rgb = np.stack((c["red"], c["green"], c["blue"]), axis=1) / 255.0
    if "nx" in c:
        normals = np.stack((c["nx"], c["ny"], c["nz"]), axis=1)
    else:
        normals = np.zeros_like(xyz)
    return BasicPointCloud(points=xyz, colors=rgb, normals=normals)


def storePly(path, xyz, rgb):
    """float x y z nx ny nz, uchar red green blue (0 .. 255), binary little-endian: the file COLMAP and upstream write."""
    xyz = np.asarray(xyz, dtype=np.float32)
    names = ("x", "y", "z", "nx", "ny", "nz")
    rec = np.zeros(len(xyz), dtype=[(k, "<f4") for k in names] + [(k, "u1") for k in ("red", "green", "blue")])
    rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    rgb = np.clip(np.rint(np.asarray(rgb, dtype=np.float64)), 0, 255).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    with open(path, "wb") as f:
        f.write(f"ply\nformat binary_little_endian 1.0\nelement vertex {len(xyz)}\n".encode())
        f.write("".join(f"property float {k}\n" for k in names).encode())
        f.write(b"property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
        rec.tofile(f)


def readColmapSceneInfo(path, images, depths, eval, train_test_exp, llffhold=8):
    try:
        cam_extrinsics = read_extrinsics_binary(os.path.join(path, "sparse/0", "images.bin"))
        cam_intrinsics = read_intrinsics_binary(os.path.join(path, "sparse/0", "cameras.bin"))
    except FileNotFoundError:
        cam_extrinsics = read_extrinsics_text(os.path.join(path, "sparse/0", "images.txt"))
        cam_intrinsics = read_intrinsics_text(os.path.join(path, "sparse/0", "cameras.txt"))

    depths_params = None
    if depths != "":
        depth_params_file = os.path.join(path, "sparse/0", "depth_params.json")
        try:
            with open(depth_params_file) as f:
                depths_params = json.load(f)
            scales = np.array([depths_params[k]["scale"] for k in depths_params])
            med_scale = float(np.median(scales[scales > 0])) if (scales > 0).sum() else 0
            for k in depths_params:
                depths_params[k]["med_scale"] = med_scale
        except FileNotFoundError:
            print(f"Error: depth_params.json file not found at path '{depth_params_file}'.")
            sys.exit(1)

    if eval:
        if "360" in path:
            llffhold = 8
        if llffhold:
            print("------------LLFF HOLD-------------")
            names = sorted(cam_extrinsics[i].name for i in cam_extrinsics)
            test_cam_names_list = [name for idx, name in enumerate(names) if idx % llffhold == 0]
        else:
            with open(os.path.join(path, "sparse/0", "test.txt")) as f:
                test_cam_names_list = [line.strip() for line in f]
    else:
        test_cam_names_list = []

    reading_dir = "images" if images is None else images
    cam_infos = readColmapCameras(cam_extrinsics, cam_intrinsics, depths_params, os.path.join(path, reading_dir),
                                  os.path.join(path, depths) if depths != "" else "", test_cam_names_list)
    cam_infos = sorted(cam_infos, key=lambda c: c.image_name)
    train_cam_infos = [c for c in cam_infos if train_test_exp or not c.is_test]
    test_cam_infos = [c for c in cam_infos if c.is_test]
    nerf_normalization = getNerfppNorm(train_cam_infos)

    ply_path = os.path.join(path, "sparse/0/points3D.ply")
    if not os.path.exists(ply_path):
        print("Converting point3d.bin to .ply, will happen only the first time you open the scene.")
        try:
            xyz, rgb, _ = read_points3D_binary(os.path.join(path, "sparse/0/points3D.bin"))
        except FileNotFoundError:
            xyz, rgb, _ = read_points3D_text(os.path.join(path, "sparse/0/points3D.txt"))
        storePly(ply_path, xyz, rgb)
    try:
        pcd = fetchPly(ply_path)
    except Exception:  # noqa: BLE001
        pcd = None
    return SceneInfo(point_cloud=pcd, train_cameras=train_cam_infos, test_cameras=test_cam_infos,
                     nerf_normalization=nerf_normalization, ply_path=ply_path, is_nerf_synthetic=False)


sceneLoadTypeCallbacks = {"Colmap": readColmapSceneInfo}
