"""``scene.gaussian_model.GaussianModel`` -- the parameter container GSWorld subclasses
(``Semantic3DGSWrapper(GaussianModel)``, /root/reference/gsworld/mani_skill/utils/wrappers/semantic_3dgs_wrapper.py:34-184)
and merges (/root/reference/gsworld/utils/gaussian_merger.py:213-274).

Restates the layout and activations of the 3DGS python layer: raw parameters
``_xyz (N,3)``, ``_features_dc (N,1,3)``, ``_features_rest (N,15,3)``, ``_scaling (N,3)`` (log), ``_rotation (N,4)``
(r,x,y,z), ``_opacity (N,1)`` (logit); getters apply exp / normalize / sigmoid / cat.  The optimiser side:
training_setup, the two hooks subclasses override (prune_points, densification_postfix), and upstream's densify_and_prune /
densify_and_clone / densify_and_split / reset_opacity -- fused on the device for a stock model (gsworld_amd.optim), the
literal torch sequence through the hooks for a subclass that overrides them.
"""
import os

import numpy as np
import torch
from torch import nn

from utils.general_utils import build_scaling_rotation, inverse_sigmoid, strip_symmetric
from utils.system_utils import mkdir_p
from gsworld_amd.sh import RGB2SH


class GaussianModel:
    def setup_functions(self):
        def build_covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
            L = build_scaling_rotation(scaling_modifier * scaling, rotation)
            return strip_symmetric(L @ L.transpose(1, 2))

        self.scaling_activation = torch.exp
        self.scaling_inverse_activation = torch.log
        self.covariance_activation = build_covariance_from_scaling_rotation
        self.opacity_activation = torch.sigmoid
        self.inverse_opacity_activation = inverse_sigmoid
        self.rotation_activation = torch.nn.functional.normalize

    def __init__(self, sh_degree, optimizer_type="default"):
        self.active_sh_degree = 0
        self.optimizer_type = optimizer_type
        self.max_sh_degree = sh_degree
        self._xyz = torch.empty(0)
        self._features_dc = torch.empty(0)
        self._features_rest = torch.empty(0)
        self._scaling = torch.empty(0)
        self._rotation = torch.empty(0)
        self._opacity = torch.empty(0)
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0
        self.spatial_lr_scale = 0
        self.pretrained_exposures = None
        self.setup_functions()

    # ---- state ---------------------------------------------------------------------------------------------
    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling,
                self._rotation, self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom,
                self.optimizer.state_dict() if self.optimizer is not None else None, self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
         self._opacity, self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        if training_args is not None:
            self.training_setup(training_args)
            if opt_dict is not None:
                self.optimizer.load_state_dict(opt_dict)
        self.xyz_gradient_accum = xyz_gradient_accum
        self.denom = denom

    # ---- activated views (what render() passes to the rasterizer) ----------------------------------------
    @property
    def get_scaling(self):
        return self.scaling_activation(self._scaling)

    @property
    def get_rotation(self):
        return self.rotation_activation(self._rotation)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    @property
    def get_features_dc(self):
        return self._features_dc

    @property
    def get_features_rest(self):
        return self._features_rest

    @property
    def get_opacity(self):
        return self.opacity_activation(self._opacity)

    @property
    def get_exposure(self):
        return getattr(self, "_exposure", None)

    def get_exposure_from_name(self, image_name):
        if self.pretrained_exposures is None:
            return self._exposure[self.exposure_mapping[image_name]]
        return self.pretrained_exposures[image_name]

    def get_covariance(self, scaling_modifier=1):
        return self.covariance_activation(self.get_scaling, scaling_modifier, self._rotation)

    def oneupSHdegree(self):
        if self.active_sh_degree < self.max_sh_degree:
            self.active_sh_degree += 1

    # ---- initialisation from a point cloud: the one caller of simple_knn.distCUDA2 ------------------------
    def create_from_pcd(self, pcd, cam_infos, spatial_lr_scale):
        from simple_knn._C import distCUDA2

        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.tensor(np.asarray(pcd.points)).float().cuda()
        color = RGB2SH(torch.tensor(np.asarray(pcd.colors)).float().cuda())
        features = torch.zeros((color.shape[0], 3, (self.max_sh_degree + 1) ** 2)).float().cuda()
        features[:, :3, 0] = color
        print("Number of points at initialisation : ", pts.shape[0])
        dist2 = torch.clamp_min(distCUDA2(pts), 0.0000001)
        scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((pts.shape[0], 4), device="cuda")
        rots[:, 0] = 1
        opacities = self.inverse_opacity_activation(0.1 * torch.ones((pts.shape[0], 1), dtype=torch.float,
                                                                     device="cuda"))
        self._xyz = nn.Parameter(pts.requires_grad_(True))
        self._features_dc = nn.Parameter(features[:, :, 0:1].transpose(1, 2).contiguous().requires_grad_(True))
        self._features_rest = nn.Parameter(features[:, :, 1:].transpose(1, 2).contiguous().requires_grad_(True))
        self._scaling = nn.Parameter(scales.requires_grad_(True))
        self._rotation = nn.Parameter(rots.requires_grad_(True))
        self._opacity = nn.Parameter(opacities.requires_grad_(True))
        self.max_radii2D = torch.zeros((self.get_xyz.shape[0]), device="cuda")
        if cam_infos:
            self.exposure_mapping = {cam_info.image_name: idx for idx, cam_info in enumerate(cam_infos)}
            exposure = torch.eye(3, 4, device="cuda")[None].repeat(len(cam_infos), 1, 1)
            self._exposure = nn.Parameter(exposure.requires_grad_(True))

    # ---- optimiser plumbing (what prune / densify hooks of the subclass rely on) -------------------------
    def training_setup(self, training_args):
        self.percent_dense = training_args.percent_dense
        n = self.get_xyz.shape[0]
        dev = self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        groups = [
            {"params": [self._xyz], "lr": training_args.position_lr_init * self.spatial_lr_scale, "name": "xyz"},
            {"params": [self._features_dc], "lr": training_args.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": training_args.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": training_args.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": training_args.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": training_args.rotation_lr, "name": "rotation"},
        ]
        if self.optimizer_type == "sparse_adam":
            # upstream: `from diff_gaussian_rasterization import SparseGaussianAdam`; here it lives in gsworld_amd.optim
            from gsworld_amd.optim import SparseGaussianAdam

            self.optimizer = SparseGaussianAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        # the schedules and the exposure optimizer of upstream's training_setup: built for an args object that carries the
        # exposure_lr_* fields (OptimizationParams); one set up the old way keeps the constant rates above and has neither
        self.exposure_optimizer = None
        self.xyz_scheduler_args = self.exposure_scheduler_args = None
        if hasattr(training_args, "exposure_lr_init"):
            from utils.general_utils import get_expon_lr_func

            if getattr(self, "_exposure", None) is not None:
                self.exposure_optimizer = torch.optim.Adam([self._exposure])
            self.xyz_scheduler_args = get_expon_lr_func(
                lr_init=training_args.position_lr_init * self.spatial_lr_scale,
                lr_final=training_args.position_lr_final * self.spatial_lr_scale,
                lr_delay_mult=training_args.position_lr_delay_mult, max_steps=training_args.position_lr_max_steps)
            self.exposure_scheduler_args = get_expon_lr_func(
                training_args.exposure_lr_init, training_args.exposure_lr_final,
                lr_delay_steps=training_args.exposure_lr_delay_steps, lr_delay_mult=training_args.exposure_lr_delay_mult,
                max_steps=training_args.iterations)

    def update_learning_rate(self, iteration):
        """Learning rates of this iteration: the exposure optimizer's and the xyz group's; -> the xyz rate."""
        if self.xyz_scheduler_args is None:
            raise RuntimeError("update_learning_rate: training_setup was given no schedule (args without exposure_lr_*)")
        if self.exposure_optimizer is not None and self.pretrained_exposures is None:
            for group in self.exposure_optimizer.param_groups:
                group["lr"] = self.exposure_scheduler_args(iteration)
        for group in self.optimizer.param_groups:
            if group["name"] == "xyz":
                group["lr"] = lr = self.xyz_scheduler_args(iteration)
                return lr

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        """upstream's bookkeeping of an iteration.  ``update_filter`` = the int32 ``radii`` of the frame: one fused launch
        that reads them on the device (no ``nonzero``, no host read; ``max_radii2D`` is updated in the same pass); a mask
        or index tensor: upstream's two lines."""
        if update_filter.dtype == torch.int32:
            from gsworld_amd.optim import densification_stats

            if self.max_radii2D.numel() != update_filter.numel():
                self.max_radii2D = torch.zeros((update_filter.numel(),), device=update_filter.device)
            densification_stats(update_filter, viewspace_point_tensor.grad, self.xyz_gradient_accum, self.denom,
                                self.max_radii2D)
            return
        self.xyz_gradient_accum[update_filter] += torch.norm(viewspace_point_tensor.grad[update_filter, :2], dim=-1,
                                                             keepdim=True)
        self.denom[update_filter] += 1

    def _swap_group_tensor(self, group, new_tensor, state_map):
        old = group["params"][0]
        state = self.optimizer.state.pop(old, None)
        group["params"][0] = nn.Parameter(new_tensor.requires_grad_(True))
        if state is not None:
            state["exp_avg"] = state_map(state["exp_avg"])
            state["exp_avg_sq"] = state_map(state["exp_avg_sq"])
            self.optimizer.state[group["params"][0]] = state
        return group["params"][0]

    def _rebind(self, tensors):
        self._xyz, self._features_dc, self._features_rest = tensors["xyz"], tensors["f_dc"], tensors["f_rest"]
        self._opacity, self._scaling, self._rotation = tensors["opacity"], tensors["scaling"], tensors["rotation"]

    def _current(self):
        return {"xyz": self._xyz, "f_dc": self._features_dc, "f_rest": self._features_rest,
                "opacity": self._opacity, "scaling": self._scaling, "rotation": self._rotation}

    def prune_points(self, mask):
        keep = ~mask
        if self.optimizer is not None:
            out = {}
            for group in self.optimizer.param_groups:
                out[group["name"]] = self._swap_group_tensor(group, group["params"][0][keep],
                                                             lambda s: s[keep])
            self._rebind(out)
        else:
            self._rebind({k: (nn.Parameter(v[keep]) if isinstance(v, nn.Parameter) else v[keep])
                          for k, v in self._current().items()})
        if self.xyz_gradient_accum.numel():
            self.xyz_gradient_accum = self.xyz_gradient_accum[keep]
            self.denom = self.denom[keep]
        if self.max_radii2D.numel():
            self.max_radii2D = self.max_radii2D[keep]
        if getattr(self, "tmp_radii", None) is not None:
            self.tmp_radii = self.tmp_radii[keep]

    def densification_postfix(self, new_xyz, new_features_dc, new_features_rest, new_opacities, new_scaling,
                              new_rotation, new_tmp_radii):
        extra = {"xyz": new_xyz, "f_dc": new_features_dc, "f_rest": new_features_rest, "opacity": new_opacities,
                 "scaling": new_scaling, "rotation": new_rotation}
        if self.optimizer is not None:
            out = {}
            for group in self.optimizer.param_groups:
                add = extra[group["name"]]
                out[group["name"]] = self._swap_group_tensor(
                    group, torch.cat((group["params"][0], add), dim=0),
                    lambda s, add=add: torch.cat((s, torch.zeros_like(add)), dim=0))
            self._rebind(out)
        else:
            self._rebind({k: torch.cat((v, extra[k]), dim=0) for k, v in self._current().items()})
        if getattr(self, "tmp_radii", None) is not None and new_tmp_radii is not None:
            self.tmp_radii = torch.cat((self.tmp_radii, new_tmp_radii))
        n = self.get_xyz.shape[0]
        dev = self._xyz.device
        self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
        self.denom = torch.zeros((n, 1), device=dev)
        self.max_radii2D = torch.zeros((n,), device=dev)

    # ---- densification (every densification_interval iterations) and opacity reset ------------------------------
    def replace_tensor_to_optimizer(self, tensor, name):
        """-> {name: the new parameter}; both moments of the group become zeros (``step`` stays)."""
        out = {}
        for group in self.optimizer.param_groups:
            if group["name"] == name:
                out[name] = self._swap_group_tensor(group, tensor, torch.zeros_like)
        return out

    @torch.no_grad()
    def reset_opacity(self):
        """opacity = inverse_sigmoid(min(get_opacity, 0.01)), its moments zeroed (every opacity_reset_interval iterations)."""
        opacities_new = self.inverse_opacity_activation(torch.min(self.get_opacity,
                                                                  torch.ones_like(self.get_opacity) * 0.01))
        if self.optimizer is None:
            self._opacity = nn.Parameter(opacities_new) if isinstance(self._opacity, nn.Parameter) else opacities_new
            return
        self._opacity = self.replace_tensor_to_optimizer(opacities_new, "opacity")["opacity"]

    def densify_and_clone(self, grads, grad_threshold, scene_extent):
        selected = torch.norm(grads, dim=-1) >= grad_threshold
        selected = torch.logical_and(selected,
                                     torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent)
        tmp_radii = getattr(self, "tmp_radii", None)
        self.densification_postfix(self._xyz[selected], self._features_dc[selected], self._features_rest[selected],
                                   self._opacity[selected], self._scaling[selected], self._rotation[selected],
                                   tmp_radii[selected] if tmp_radii is not None else None)

    def densify_and_split(self, grads, grad_threshold, scene_extent, N=2, noise=None):
        """``noise``: ``(n, N, 3)`` standard normals indexed by parent row (n = the rows ``grads`` covers); a child's offset
        is ``exp(scaling) * noise`` where upstream draws ``torch.normal(0, exp(scaling))`` -- the same distribution.  A row is
        split when it is hot and NOT small (``~(max <= limit)``, the complement of densify_and_clone's test; upstream
        writes ``max > limit``, which differs only for a NaN scale)."""
        from utils.general_utils import build_rotation

        n_init = self.get_xyz.shape[0]
        dev = self._xyz.device
        padded_grad = torch.zeros((n_init,), device=dev)
        padded_grad[:grads.shape[0]] = grads.squeeze(-1) if grads.dim() > 1 else grads
        selected = padded_grad >= grad_threshold
        selected = torch.logical_and(selected, torch.logical_not(
            torch.max(self.get_scaling, dim=1).values <= self.percent_dense * scene_extent))
        stds = self.get_scaling[selected].repeat(N, 1)
        if noise is None:
            samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
        else:
            padded = torch.zeros((n_init, N, 3), device=dev)
            padded[:noise.shape[0]] = noise
            samples = stds * padded[selected].transpose(0, 1).reshape(-1, 3)
        rots = build_rotation(self._rotation[selected]).repeat(N, 1, 1)
        new_xyz = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + self.get_xyz[selected].repeat(N, 1)
        new_scaling = self.scaling_inverse_activation(self.get_scaling[selected].repeat(N, 1) / (0.8 * N))
        tmp_radii = getattr(self, "tmp_radii", None)
        self.densification_postfix(new_xyz, self._features_dc[selected].repeat(N, 1, 1),
                                   self._features_rest[selected].repeat(N, 1, 1), self._opacity[selected].repeat(N, 1),
                                   new_scaling, self._rotation[selected].repeat(N, 1),
                                   tmp_radii[selected].repeat(N) if tmp_radii is not None else None)
        prune_filter = torch.cat((selected, torch.zeros(N * int(selected.sum()), device=dev, dtype=torch.bool)))
        self.prune_points(prune_filter)

    def _fused_densify(self):
        """The fused route is taken when the tensors are on a HIP device and the class overrides neither hook (a subclass
        that does -- GSWorld's Semantic3DGSWrapper gives new rows zero semantics there -- goes through its hooks)."""
        cls = type(self)
        return (self._xyz.is_cuda and cls.prune_points is GaussianModel.prune_points
                and cls.densification_postfix is GaussianModel.densification_postfix)

    @torch.no_grad()
    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size, radii, noise=None):
        """Upstream's sequence: clone the small hot Gaussians, split the large hot ones in two, prune the transparent and
        (``if max_screen_size:``) the oversized ones; rows come out as kept | clones | first children | second children.

        ``densification_postfix`` zeroes ``max_radii2D`` before the final prune reads it, so inside this sequence upstream's
        screen-size test (``max_radii2D > max_screen_size``) selects nothing and only its world-size companion acts.  Both
        routes reproduce that and do not repair it: the fused one (``gsworld_amd.optim.densify_and_prune``: one host read
        instead of some forty compactions) reads neither ``max_radii2D`` nor ``radii``.  ``noise``: ``(N, 2, 3)`` standard
        normals indexed by parent, drawn when not given.  Afterwards ``xyz_gradient_accum``, ``denom`` and ``max_radii2D``
        are zeros of the new size and ``tmp_radii`` is None."""
        self.last_densify_route = "fused" if self._fused_densify() else "literal"
        if self.last_densify_route == "fused":
            from gsworld_amd.optim import densify_and_prune

            out, _, _ = densify_and_prune(self._current(), self.optimizer, self.xyz_gradient_accum, self.denom,
                                          grad_threshold=max_grad, min_opacity=min_opacity, extent=extent,
                                          percent_dense=self.percent_dense, prune_world_size=bool(max_screen_size),
                                          noise=noise)
            self._rebind(out)
            n, dev = self._xyz.shape[0], self._xyz.device
            self.xyz_gradient_accum = torch.zeros((n, 1), device=dev)
            self.denom = torch.zeros((n, 1), device=dev)
            self.max_radii2D = torch.zeros((n,), device=dev)
            self.tmp_radii = None
            return
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        self.tmp_radii = radii
        self.densify_and_clone(grads, max_grad, extent)
        self.densify_and_split(grads, max_grad, extent, noise=noise)
        prune_mask = (self.get_opacity < min_opacity).squeeze(-1)
        if max_screen_size:
            big_points_vs = self.max_radii2D > max_screen_size
            big_points_ws = self.get_scaling.max(dim=1).values > 0.1 * extent
            prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
        self.prune_points(prune_mask)
        self.tmp_radii = None

    # ---- PLY interchange (property order of SURVEY.md 8f-3) -------------------------------------------------
    def construct_list_of_attributes(self):
        names = ["x", "y", "z", "nx", "ny", "nz"]
        names += [f"f_dc_{i}" for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        names += [f"f_rest_{i}" for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        names.append("opacity")
        names += [f"scale_{i}" for i in range(self._scaling.shape[1])]
        names += [f"rot_{i}" for i in range(self._rotation.shape[1])]
        return names

    def save_ply(self, path):
        from gsworld_amd.ply import write_gaussian_ply

        mkdir_p(os.path.dirname(path))
        write_gaussian_ply(path, self)

    def load_ply(self, path, use_train_test_exp=False):
        from gsworld_amd.ply import read_gaussian_ply

        # the stock loader: trainable nn.Parameters, _opacity (N,1).  GSWorld's Semantic3DGSWrapper overrides load_ply
        # (frozen tensors, (N,1,1) opacity, semantics) -- that flavour is read_gaussian_ply's default.
        read_gaussian_ply(path, self, upstream=True)
        self.active_sh_degree = self.max_sh_degree
        if use_train_test_exp:  # the exposures `Scene.save` left in the model path, two folders above the PLY
            import json

            exposure_file = os.path.join(os.path.dirname(path), os.pardir, os.pardir, "exposure.json")
            if os.path.exists(exposure_file):
                with open(exposure_file) as f:
                    exposures = json.load(f)
                self.pretrained_exposures = {name: torch.tensor(e, dtype=torch.float32, device=self._xyz.device)
                                             for name, e in exposures.items()}
                print("Pretrained exposures loaded.")
            else:
                print(f"No exposure to be loaded at {exposure_file}")
                self.pretrained_exposures = None
