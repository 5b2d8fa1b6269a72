"""``utils.camera_utils`` of the 3DGS python layer: ``CameraInfo`` records -> ``scene.cameras.Camera`` objects, and the
``cameras.json`` entries written next to a trained model."""
import numpy as np
from PIL import Image

from scene.cameras import Camera
from utils.graphics_utils import fov2focal

WARNED = False


def loadCam(args, id, cam_info, resolution_scale, is_nerf_synthetic=False, is_test_dataset=False):
    global WARNED
    image = Image.open(cam_info.image_path)
    invdepthmap = None
    if getattr(cam_info, "depth_path", ""):
        # 16-bit PNG of inverse depths, scaled by 2^16 (a nerf-synthetic depth is used as it is)
        raw = np.asarray(Image.open(cam_info.depth_path)).astype(np.float32)
        invdepthmap = raw if is_nerf_synthetic else raw / float(2 ** 16)
    orig_w, orig_h = image.size
    if args.resolution in (1, 2, 4, 8):
        resolution = round(orig_w / (resolution_scale * args.resolution)), round(orig_h / (resolution_scale * args.resolution))
    else:
        if args.resolution == -1:
            if orig_w > 1600:
                if not WARNED:
                    print("[ INFO ] Encountered quite large input images (>1.6K pixels width), rescaling to 1.6K.\n "
                          "If this is not desired, please explicitly specify '--resolution/-r' as 1")
                    WARNED = True
                global_down = orig_w / 1600
            else:
                global_down = 1
        else:
            global_down = orig_w / args.resolution
        scale = float(global_down) * float(resolution_scale)
        resolution = (int(orig_w / scale), int(orig_h / scale))
    return Camera(resolution, colmap_id=cam_info.uid, R=cam_info.R, T=cam_info.T, FoVx=cam_info.FovX, FoVy=cam_info.FovY,
                  depth_params=cam_info.depth_params, image=image, invdepthmap=invdepthmap, image_name=cam_info.image_name,
                  uid=id, data_device=args.data_device, train_test_exp=args.train_test_exp, is_test_dataset=is_test_dataset,
                  is_test_view=cam_info.is_test)


def cameraList_from_camInfos(cam_infos, resolution_scale, args, is_nerf_synthetic=False, is_test_dataset=False):
    return [loadCam(args, id, c, resolution_scale, is_nerf_synthetic, is_test_dataset) for id, c in enumerate(cam_infos)]


def camera_to_JSON(id, camera):
    """One entry of ``cameras.json``: position and rotation are the camera-to-world of the record's ``R`` (stored
    transposed, i.e. already camera-to-world) and ``T`` (world-to-camera translation)."""
    W2C = np.zeros((4, 4))
    W2C[:3, :3] = np.asarray(camera.R).transpose()
    W2C[:3, 3] = np.asarray(camera.T)
    W2C[3, 3] = 1.0
    C2W = np.linalg.inv(W2C)
    return {"id": id, "img_name": camera.image_name, "width": camera.width, "height": camera.height,
            "position": C2W[:3, 3].tolist(), "rotation": [row.tolist() for row in C2W[:3, :3]],
            "fy": fov2focal(camera.FovY, camera.height), "fx": fov2focal(camera.FovX, camera.width)}
