"""``scene`` package of the 3DGS python layer, as far as GSWorld touches it: ``scene.cameras.Camera`` and
``scene.gaussian_model.GaussianModel``."""
import json
import os
import random


def searchForMaxIteration(folder):
    return max(int(name.split("_")[-1]) for name in os.listdir(folder))


class Scene:
    """A capture on disk and the model trained on it: reads ``args.source_path`` (a COLMAP capture), builds the train /
    test cameras, and either initialises ``gaussians`` from the sparse points or loads ``point_cloud/iteration_N``."""

    def __init__(self, args, gaussians, load_iteration=None, shuffle=True, resolution_scales=[1.0]):  # noqa: B006
        from scene.dataset_readers import sceneLoadTypeCallbacks
        from utils.camera_utils import cameraList_from_camInfos, camera_to_JSON

        self.model_path = args.model_path
        self.loaded_iter = None
        self.gaussians = gaussians
        if load_iteration:
            if load_iteration == -1:
                self.loaded_iter = searchForMaxIteration(os.path.join(self.model_path, "point_cloud"))
            else:
                self.loaded_iter = load_iteration
            print(f"Loading trained model at iteration {self.loaded_iter}")
        self.train_cameras = {}
        self.test_cameras = {}

        if os.path.exists(os.path.join(args.source_path, "sparse")):
            scene_info = sceneLoadTypeCallbacks["Colmap"](args.source_path, args.images, args.depths, args.eval,
                                                          args.train_test_exp)
        elif os.path.exists(os.path.join(args.source_path, "transforms_train.json")):
            raise NotImplementedError("the Blender (transforms_train.json) reader is not provided: COLMAP captures only")
        else:
            raise AssertionError("Could not recognize scene type!")

        if not self.loaded_iter:
            with open(scene_info.ply_path, "rb") as src, open(os.path.join(self.model_path, "input.ply"), "wb") as dst:
                dst.write(src.read())
            camlist = list(scene_info.test_cameras or []) + list(scene_info.train_cameras or [])
            with open(os.path.join(self.model_path, "cameras.json"), "w") as f:
                json.dump([camera_to_JSON(id, cam) for id, cam in enumerate(camlist)], f)

        if shuffle:
            random.shuffle(scene_info.train_cameras)
            random.shuffle(scene_info.test_cameras)
        self.cameras_extent = scene_info.nerf_normalization["radius"]

        for scale in resolution_scales:
            print("Loading Training Cameras")
            self.train_cameras[scale] = cameraList_from_camInfos(scene_info.train_cameras, scale, args,
                                                                 scene_info.is_nerf_synthetic, False)
            print("Loading Test Cameras")
            self.test_cameras[scale] = cameraList_from_camInfos(scene_info.test_cameras, scale, args,
                                                                scene_info.is_nerf_synthetic, True)

        if self.loaded_iter:
            self.gaussians.load_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{self.loaded_iter}",
                                                 "point_cloud.ply"), args.train_test_exp)
        else:
            self.gaussians.create_from_pcd(scene_info.point_cloud, scene_info.train_cameras, self.cameras_extent)

    def save(self, iteration):
        folder = os.path.join(self.model_path, f"point_cloud/iteration_{iteration}")
        self.gaussians.save_ply(os.path.join(folder, "point_cloud.ply"))
        exposure = self.gaussians.get_exposure
        mapping = getattr(self.gaussians, "exposure_mapping", None) or {}
        with open(os.path.join(self.model_path, "exposure.json"), "w") as f:
            json.dump({name: exposure[idx].detach().cpu().numpy().tolist() for name, idx in mapping.items()}
                      if exposure is not None else {}, f, indent=2)

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]


def __getattr__(name):  # (`from scene import Scene, GaussianModel` as upstream's train.py writes it; imported on first use)
    if name == "GaussianModel":
        from .gaussian_model import GaussianModel

        return GaussianModel
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
