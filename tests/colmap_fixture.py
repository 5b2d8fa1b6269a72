"""Writers of a COLMAP sparse model -- ``cameras`` / ``images`` / ``points3D`` as ``.bin`` (little-endian, packed with
``struct`` from the layouts COLMAP documents) and ``.txt`` -- and a synthetic capture built from them: a ground-truth model
rendered by this package from cameras on an arc, saved as PNG next to the sparse model a trainer starts from."""
import math
import os
import struct

import numpy as np

MODEL_PARAMS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 4: ("OPENCV", 8)}


def write_cameras_bin(path, cameras):
    """cameras: [(id, model_id, width, height, params)]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for cid, model, w, h, params in cameras:
            f.write(struct.pack("<iiQQ", cid, model, w, h))
            f.write(struct.pack("<" + "d" * len(params), *params))


def write_images_bin(path, images):
    """images: [(id, qvec (w,x,y,z), tvec, camera_id, name, [(x, y, point3D_id)])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for iid, q, t, cid, name, pts in images:
            f.write(struct.pack("<i4d3di", iid, *q, *t, cid))
            f.write(name.encode("utf-8") + b"\x00")
            f.write(struct.pack("<Q", len(pts)))
            for x, y, pid in pts:
                f.write(struct.pack("<ddq", x, y, pid))


def write_points3D_bin(path, points):
    """points: [(id, xyz, rgb, error, [(image_id, point2D_idx)])]"""
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(points)))
        for pid, xyz, rgb, err, track in points:
            f.write(struct.pack("<Q3d3BdQ", pid, *xyz, *rgb, err, len(track)))
            for a, b in track:
                f.write(struct.pack("<ii", a, b))


def write_cameras_txt(path, cameras):
    with open(path, "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for cid, model, w, h, params in cameras:
            f.write(f"{cid} {MODEL_PARAMS[model][0]} {w} {h} " + " ".join(repr(float(p)) for p in params) + "\n")


def write_images_txt(path, images):
    with open(path, "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for iid, q, t, cid, name, pts in images:
            f.write(f"{iid} " + " ".join(repr(float(v)) for v in (*q, *t)) + f" {cid} {name}\n")
            f.write(" ".join(f"{float(x)!r} {float(y)!r} {pid}" for x, y, pid in pts) + "\n")


def write_points3D_txt(path, points):
    with open(path, "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for pid, xyz, rgb, err, track in points:
            f.write(f"{pid} " + " ".join(repr(float(v)) for v in xyz) + " " + " ".join(str(int(v)) for v in rgb) +
                    f" {float(err)!r} " + " ".join(f"{a} {b}" for a, b in track) + "\n")


def rotmat_to_qvec(R):
    """(w, x, y, z) of a rotation matrix, w >= 0 (Shepperd's method, binary64)."""
    R = np.asarray(R, dtype=np.float64)
    tr = np.trace(R)
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
        q = np.zeros(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def arc_views(n=8, size=64, fov_deg=60.0, radius=3.0, span_deg=80.0):
    """``n`` look-at cameras on an arc of ``radius`` about (0, 0, 3) in the x-z plane (the middle of the span is the
    identity view at the origin)."""
    from gsworld_amd.camera import look_at_view

    fov = math.radians(fov_deg)
    views = []
    for k in range(n):
        a = math.radians(-span_deg / 2 + span_deg * k / (n - 1))
        eye = [radius * math.sin(a), 0.0, 3.0 - radius * math.cos(a)]
        views.append(look_at_view(eye, [0.0, 0.0, 3.0], [0.0, -1.0, 0.0], fov, fov, size, size))
    return views


def build_capture(root, device, seed=3, n_gaussians=2000, n_points=500, n_views=8, size=64, fov_deg=60.0, gains=None,
                  depths=False):
    """A capture under ``root``: ``images/view_XX.png`` rendered from ``scenes.random_scene_camera_frame(n_gaussians, seed)``,
    ``sparse/0/{cameras,images,points3D}.bin``; points3D = ``n_points`` ground-truth centres + 1 cm noise with their DC
    colours.  ``gains``: {view index: factor} darkens that view's image.  ``depths``: also ``depths/view_XX.png`` (16-bit
    inverse depths of the ground truth x 2^16) and ``sparse/0/depth_params.json`` (scale 1, offset 0).
    -> dict(views=[ViewParams], images=[(3,H,W) float tensors on the CPU], centres=(n_views,3), names=[...])"""
    import json

    import torch
    from PIL import Image

    from gsworld_amd import scenes
    from gsworld_amd.renderer import FrameRenderer

    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "sparse", "0"), exist_ok=True)
    raw = scenes.random_scene_camera_frame(n_gaussians, seed).to(device)
    views = arc_views(n_views, size, fov_deg)
    renderer = FrameRenderer(device)
    bg = torch.zeros(3, device=device)
    focal = size / (2 * math.tan(math.radians(fov_deg) / 2))
    cameras = [(1, 1, size, size, (focal, focal, size / 2, size / 2))]
    images, gts, names, centres, depth_params = [], [], [], [], {}
    if depths:
        os.makedirs(os.path.join(root, "depths"), exist_ok=True)
    for k, v in enumerate(views):
        color, _, invd = renderer.render(v.to(device), raw.xyz, raw.opacity, shs=raw.features_dc, shs_rest=raw.features_rest,
                                         scales=raw.scaling, rotations=raw.rotation, param_space=7, bg=bg)
        img = color.clamp(0, 1).cpu() * float((gains or {}).get(k, 1.0))
        u8 = (img.permute(1, 2, 0).numpy() * 255.0 + 0.5).astype(np.uint8)
        name = f"view_{k:02d}.png"
        Image.fromarray(u8).save(os.path.join(root, "images", name))
        gts.append(torch.from_numpy(u8).permute(2, 0, 1).float() / 255.0)
        if depths:
            d16 = (invd[0].clamp(0, 0.9999).cpu().numpy() * 65536.0).astype(np.uint16)
            Image.fromarray(d16).save(os.path.join(root, "depths", name))
            depth_params[name[:-4]] = {"scale": 1.0, "offset": 0.0}
        w2c = v.world_view_transform.double().numpy().T
        images.append((k + 1, rotmat_to_qvec(w2c[:3, :3]), w2c[:3, 3], 1, name, [(1.0 + k, 2.0, k)]))
        names.append(name)
        centres.append(v.camera_center.double().numpy())
    if depths:
        with open(os.path.join(root, "sparse", "0", "depth_params.json"), "w") as f:
            json.dump(depth_params, f)
    rng = np.random.default_rng(seed)
    pick = rng.choice(n_gaussians, n_points, replace=False)
    xyz = raw.xyz.cpu().numpy()[pick].astype(np.float64) + rng.normal(0, 0.01, (n_points, 3))
    rgb = np.clip(raw.features_dc.cpu().numpy()[pick, 0, :] * 0.28209479177387814 + 0.5, 0, 1)
    points = [(i + 1, xyz[i], (rgb[i] * 255).astype(np.uint8), 0.5, [(1, i % 3)]) for i in range(n_points)]
    write_cameras_bin(os.path.join(root, "sparse", "0", "cameras.bin"), cameras)
    write_images_bin(os.path.join(root, "sparse", "0", "images.bin"), images)
    write_points3D_bin(os.path.join(root, "sparse", "0", "points3D.bin"), points)
    return {"views": views, "images": gts, "centres": np.array(centres), "names": names}
