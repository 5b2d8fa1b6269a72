"""Render side of GSWorld's closed loop (BASELINE.json configs[2]) without the wrapper's per-step torch glue.

``GSWorldWrapper.step`` / ``reset`` (/root/reference/gsworld/mani_skill/utils/wrappers/gs_world_wrapper.py:176-198)
do two things after the physics step: ``transform_gs_perlink`` (``:110-162``: one ``transform_gaussians`` per robot link
and tracked actor) and ``_render_gsworld`` (``:232-275``: per camera and per environment a deep copy of the model, the
masked write-back of every moved part, ``render()``, uint8 conversion).  :class:`ClosedLoopRenderer` is that pair for a
scene held on one MI355X:

* the pose table of the step is packed on the device (``gsr_pack_part_transforms``), one fused pass moves every labelled
  Gaussian (``gsr_transform_gaussians_batch``; ``E`` environments at once),
* all ``E x C`` frames of the step are enqueued on their own HIP streams with their own renderer state
  (:class:`gsworld_amd.renderer.MultiCameraRenderer`), the compositor writes GSWorld's uint8 frames itself,
* the whole GPU side of a step can be captured once and replayed as one hipGraph.

Returns what ``_render_gsworld`` returns: ``{camera name: uint8 (num_envs, H, W, 3)}``.

SAPIEN / PhysX do not run on a headless GPU box, so when the loop is measured (``bench.py``,
``tools/closed_loop_surrogate.py``) :mod:`gsworld_amd.rollouts` stands in for the simulator (link poses of a seeded
random-action rollout from forward kinematics of the reference's xarm6 URDF, pushed through :func:`part_poses_from_sim`).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _C, _lib
from . import transform as tf
from ._lib import FRAME_KEPT, RAW_ROTATIONS, RAW_SCALES, model_version
from .renderer import MultiCameraRenderer


def _to_mirror(dst: torch.Tensor, dst_np, src: torch.Tensor) -> None:
    """``dst.copy_(src.to(float32).reshape(dst.shape))`` for the host mirror; a float32 host tensor that needs no
    conversion goes through numpy (same memory, a fraction of a torch op's dispatch)."""
    if src.dtype == torch.float32 and src.device.type == "cpu" and not src.requires_grad and src.is_contiguous() and \
            src.numel() == dst_np.size:
        np.copyto(dst_np, src.numpy().reshape(dst_np.shape))
    else:
        dst.copy_(src.detach().to("cpu", torch.float32).reshape(dst.shape))


MAP_KINDS = ("segmentation", "depth")


def _camera_list(name, value, num_envs: int, per_env: bool) -> list:
    """A camera argument as the list of ViewParams its environments see: one for all (``per_env`` False, or a single
    ViewParams), or E of one image size (``ValueError`` otherwise)."""
    from .camera import ViewParams

    if isinstance(value, ViewParams) or not isinstance(value, (list, tuple)):
        return [value] * (num_envs if per_env else 1)
    if not per_env:
        raise ValueError(f"camera {name!r}: one ViewParams per camera (a list per environment needs per_env_cameras=True)")
    if len(value) != num_envs:
        raise ValueError(f"camera {name!r}: {len(value)} ViewParams for {num_envs} environments")
    if len({(int(c.image_width), int(c.image_height)) for c in value}) != 1:
        raise ValueError(f"camera {name!r}: every environment's camera must have the same image size")
    return list(value)


def check_sim2real(sim2real):
    """``(rigid_sim2real (4,4), scale_sim2real)`` -> (16 row-major floats, scale) as ``gsr_cameras_from_extrinsics`` takes
    them; ``ValueError`` for anything else."""
    if not isinstance(sim2real, (list, tuple)) or len(sim2real) != 2:
        raise ValueError("sim2real must be (rigid_sim2real (4,4), scale_sim2real)")
    R = sim2real[0].detach().cpu().numpy() if isinstance(sim2real[0], torch.Tensor) else np.asarray(sim2real[0])
    s = sim2real[1].detach().cpu().numpy() if isinstance(sim2real[1], torch.Tensor) else np.asarray(sim2real[1])
    R, s = R.astype(np.float64), s.astype(np.float64)
    if R.shape != (4, 4) or not np.all(np.isfinite(R)) or s.size != 1 or not np.isfinite(s.reshape(-1)[0]) or \
            float(s.reshape(-1)[0]) == 0.0:
        raise ValueError("sim2real must be (rigid_sim2real (4,4) finite, scale_sim2real finite and non-zero)")
    return [float(x) for x in R.reshape(-1)], float(s.reshape(-1)[0])


def check_extrinsics(name, value, num_envs: int, per_env: bool, has_sim2real: bool) -> torch.Tensor:
    """An ``extrinsic_cv`` argument of :meth:`ClosedLoopRenderer.set_extrinsics` as a float32 tensor of the shape the loop
    stages, ``(E,3,4)`` (per-environment cameras) or ``(1,3,4)``; ``ValueError`` for a wrong shape or a loop built without
    ``sim2real``."""
    if not has_sim2real:
        raise ValueError("extrinsics need sim2real=(rigid_sim2real, scale_sim2real) at construction")
    t = value if isinstance(value, torch.Tensor) else torch.as_tensor(np.asarray(value))
    want = (num_envs, 3, 4) if per_env else (1, 3, 4)
    if not (tuple(t.shape) == want or (not per_env and tuple(t.shape) == (3, 4))):
        raise ValueError(f"extrinsics of camera {name!r}: expected shape {want}" + ("" if per_env else " or (3, 4)") +
                         f", got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    return t.reshape(want)


def check_map_labels(labels: torch.Tensor) -> torch.Tensor:
    """The per-Gaussian semantic labels of a segmentation map as ``gsr_render_maps`` reads them: (P,) float32, dense, on the
    labels' device.  Every label must be an integral value inside int16 (the map stores ``(int16)(int)label``); anything else
    raises ``ValueError`` -- once, when a loop is built, not per frame."""
    lab = labels.detach().reshape(-1).to(torch.float32).contiguous()
    if lab.numel() and not bool(torch.all(torch.isfinite(lab) & (lab == torch.round(lab)) & (lab >= -32768) & (lab <= 32767))):
        raise ValueError("segmentation maps need integral semantic labels in the int16 range [-32768, 32767]")
    return lab


class ClosedLoopRenderer:
    def __init__(self, raw, part_labels: dict, cameras: dict, scaled_parts=(), num_envs: int = 1, device="cuda",
                 background=None, fuse_transform: bool = True, growth: float = 2.0, bound_capacity="auto",
                 layout: bool = True, min_capacity: int | None = None, share_model_of=None, batched: bool = True,
                 keep_float: bool = False, block_cache: bool = True, tile_reuse: bool = True, maps=(),
                 depth_scale: float = 1.0, pointcloud=None, per_env_cameras: bool = False, sim2real=None, appearance=None):
        """``raw``: :class:`gsworld_amd.scenes.RawGaussians` (or any object with the same raw parameter tensors, e.g. a
        merged semantic model's ``_xyz`` ... under those names); ``part_labels``: part name -> semantic label(s), in
        the order the pose matrices will arrive; ``cameras``: name -> :class:`gsworld_amd.camera.ViewParams`;
        ``scaled_parts``: the tracked actors (their log-scales are rewritten per step as the reference does).
        ``fuse_transform`` (default): the step's rigid transforms are applied INSIDE each frame's preprocess
        (``GsrInputs.part_*``): every (environment, camera) frame reads the one base model plus that environment's pose
        table, and no transformed copy of the model is written -- per step that saves a 60 B/Gaussian pass per
        environment (88 MB at 1.47 M) and, for ``num_envs`` > 1, the (E,P,.) buffers themselves.  ``False``: one
        ``gsr_transform_gaussians_batch`` pass per step, frames read its outputs (same bytes out: tests).
        ``growth``: every lane's binning capacity is ``max(growth x R, 2 N)`` instances, ``R`` the instance count of
        the frame that sized it (:meth:`reset`, or the re-render after an overflow).  An arm sweeping past a wrist
        camera changes that count far more than a fixed camera ever sees (0.39 M .. 1.46 M over the xarm6 random-action
        rollout, against 0.71 M at reset): the margin costs a few tens of MB per lane and keeps that rollout clear of
        the limit; :meth:`overflow_frames` says, without a per-step sync, whether a rollout stayed clear.
        ``bound_capacity`` (``"auto"`` / True / False): size every lane's list by the bound no frame can exceed, N x
        tiles (7 GB per lane at 1.47 M Gaussians, 640 x 480), so that a frame CANNOT overflow whatever the arm does.
        ``"auto"``: when all lanes together stay below a quarter of the device's free memory and 64 GiB -- one
        environment with two or three cameras on a 288 GB MI355X; larger batches keep the ``growth`` rule.
        ``layout`` (with ``fuse_transform``): the loop keeps its OWN copy of the model in Morton order per part and size
        class, with block bounds (:mod:`gsworld_amd.layout`): every frame's per-Gaussian pass skips the blocks of the
        model that the step's poses put outside the camera's frustum (two thirds of them from a sensor camera).  Same
        frames, bit for bit (tests/test_layout_gpu.py, tests/test_closed_loop_gpu.py).
        ``share_model_of``: another loop over the SAME model on the same device whose (laid-out) model tensors this one
        reads instead of making its own copy (:class:`PipelinedClosedLoop`); everything per step -- poses, cameras,
        renderer states, frames, graph -- stays its own.
        ``keep_float``: the loop returns GSWorld's uint8 frames and, by default, writes nothing else -- the float colour /
        inverse-depth images of its lanes (16 bytes per pixel nobody reads) are left out (``GsrOutputs``: NULL images for an
        inference frame with ``out_rgb8``).  True keeps them in ``multi.lanes[k]._out`` (tests that compare float colour).
        ``tile_reuse`` (with ``block_cache``; default): ``self.frames`` are the loop's own buffers and nobody else writes
        them (READ the returned frames, copy them if you want to draw into them): a 16 x 16 tile that no recomputed Gaussian
        touches under an unchanged camera and background is left as the previous step composited it (include/gsr.h
        GSR_FRAME_KEPT; csrc/render.hip "tile reuse") -- from a fixed sensor camera everything but the tiles the robot and the
        tracked objects cover, now or a step ago.  Same frames, bit for bit.  ``False`` for a caller that writes into them.
        ``batched`` (default): the E x C frames of a step go through ``gsr_forward_batch`` -- one set of launches on the
        step's stream whose grids span the frames -- instead of one pipeline per frame on its own stream
        (:class:`gsworld_amd.renderer.MultiCameraRenderer`); same frames bit for bit (tests/test_batch_gpu.py).
        ``maps``: any subset of ``("segmentation", "depth")`` -- every step then also writes per-pixel maps of the splatted
        scene into :attr:`maps`, ``{camera: {"segmentation": (E,H,W,1) int16, "depth": (E,H,W,1) float32}}`` (the kinds
        asked for), loop-owned buffers overwritten by the next step like :attr:`frames`; :meth:`step` still returns the
        frames.  A pixel's label and depth are those of its median contributor, the first Gaussian after which the
        transmittance drops below 0.5 (include/gsr.h ``gsr_render_maps``); background: label -1, depth 0.0.  Labels are the
        model's semantics (integral, inside int16: ``ValueError`` otherwise).  Depth is ``depth_scale`` x the view depth in
        the scene's units; for GSWorld pass ``depth_scale = 1 / scale_sim2real`` to get the simulator's metres, since
        ``cam_maniskill2gs`` scales camera translations by ``scale_sim2real`` (gs_world_wrapper.py:298).  With the default
        ``()`` nothing changes: no buffer, no launch, :attr:`maps` is None.
        ``pointcloud``: a :class:`gsworld_amd.pointcloud.PointCloudSpec` -- every step then also writes the point cloud of
        each environment's cameras into :attr:`pointcloud`, ``{"xyzw": (E,N,4) float32, "rgb": (E,N,3) uint8,
        "segmentation": (E,N,1) int16, "count": (E,) int32}`` (N: every pixel of every camera, or the spec's
        ``num_points``), loop-owned buffers overwritten by the next step like :attr:`frames`.  It is made from this step's
        depth / label maps (rendered into private buffers where ``maps`` does not ask for them: :attr:`maps` keeps what
        ``maps`` asked for), frames and device-resident camera matrices, behind the maps on the same stream (include/gsr.h
        ``gsr_render_pointcloud``).  Labels are the model's semantics (as for segmentation maps).  With the default None
        nothing changes: no buffer, no launch, :attr:`pointcloud` is None.
        ``per_env_cameras``: every camera has one record per environment -- ``cameras[name]`` is a ViewParams (every
        environment starts there) or a sequence of ``num_envs`` of one image size (field of view may differ per
        environment; it is fixed at construction).  :meth:`set_cameras` / :meth:`step` take the same two forms, and
        :attr:`env_cameras` ``[name][e]`` are the device-resident cameras environment e's frames read.  False (default):
        one camera per name for every environment, as the reference's wrapper does (environment 0's sensor pose).
        ``sim2real``: ``(rigid_sim2real (4,4), scale_sim2real)`` of the wrapper -- needed to hand over the simulator's
        ``extrinsic_cv`` directly (:meth:`set_extrinsics`): the camera records are then computed on the device in the
        step itself (include/gsr.h ``gsr_cameras_from_extrinsics``).
        ``appearance``: ``{group name: label or labels}`` -- per-environment appearance randomization (include/gsr.h
        ``GsrInputs.appearance``; :mod:`gsworld_amd.appearance`): the Gaussians of each named group (and group 0, everything
        else) take their environment's colour affine, and every environment has its own background colour.  Tables and
        backgrounds start at the identity and ``background``, and are set with :meth:`set_appearance` or ``step(appearance=)``
        -- they travel in the step's staging vector, so every step mode reads them.  ``background`` may then also be
        ``(E, 3)``.  With the default None nothing changes."""
        maps = tuple(maps or ())
        if appearance is not None:
            from .appearance import check_groups

            sem = getattr(raw, "semantics", None)
            sem = getattr(raw, "_semantics", None) if sem is None else sem
            self._app_names, app_lut, self._app_G = check_groups(
                appearance, sem.detach().cpu().numpy() if isinstance(sem, torch.Tensor) else sem)
            if background is not None and tuple(torch.as_tensor(background).shape) not in ((3,), (int(num_envs), 3)):
                raise ValueError(f"background must be (3,) or ({int(num_envs)}, 3) with appearance")
        else:
            self._app_names, app_lut, self._app_G = None, None, 0
        self.per_env_cameras = bool(per_env_cameras)
        E0 = int(num_envs)
        cam_lists = {n: _camera_list(n, v, E0, self.per_env_cameras) for n, v in cameras.items()}
        self._sim2real = check_sim2real(sim2real) if sim2real is not None else None
        if any(m not in MAP_KINDS for m in maps) or len(set(maps)) != len(maps):
            raise ValueError(f"maps must be a subset of {MAP_KINDS}, got {maps!r}")
        if pointcloud is not None:
            from .pointcloud import PointCloudSpec

            if not isinstance(pointcloud, PointCloudSpec):
                raise ValueError("pointcloud must be None or a gsworld_amd.pointcloud.PointCloudSpec")
            pointcloud.validated()
            if int(num_envs) * len(cameras) > _lib.PC_MAX_VIEWS:
                raise ValueError(f"pointcloud: at most {_lib.PC_MAX_VIEWS} (environment, camera) views per loop")
        self.device = torch.device(device)
        dev = self.device
        self.num_envs = int(num_envs)
        self.names = list(cameras.keys())
        self._given_cameras = [cam_lists[n][0] for n in self.names]
        self.cameras = self._given_cameras  # (image sizes; replaced by device-resident copies once the staging vector exists)
        g = lambda a, b: getattr(raw, a) if hasattr(raw, a) else getattr(raw, b)  # noqa: E731
        other = share_model_of
        if other is not None:
            if other.device != dev or bool(other.layout is not None) != bool(layout and fuse_transform):
                raise ValueError("share_model_of: the other loop must live on the same device and use the same layout option")
            self.xyz, self.rotation, self.scaling = other.xyz, other.rotation, other.scaling
            self.features_dc, self.features_rest, self.opacity = other.features_dc, other.features_rest, other.opacity
            self.layout, semantics = other.layout, other._semantics
            if other.layout is not None:
                self.perm = other.perm
        else:
            self.xyz = g("xyz", "_xyz").detach().to(dev, torch.float32).contiguous()
            self.rotation = g("rotation", "_rotation").detach().to(dev, torch.float32).contiguous()
            self.scaling = g("scaling", "_scaling").detach().to(dev, torch.float32).contiguous()
            self.features_dc = g("features_dc", "_features_dc").detach().to(dev, torch.float32).contiguous()
            self.features_rest = g("features_rest", "_features_rest").detach().to(dev, torch.float32).contiguous()
            # opacity is never moved (new_opacity=None at both call sites of the wrapper): activate it once
            self.opacity = torch.sigmoid(g("opacity", "_opacity").detach().to(dev, torch.float32).reshape(-1, 1)).contiguous()
            semantics = g("semantics", "_semantics")
            self.layout = None
        if other is None and layout and fuse_transform:
            from .layout import SceneLayout

            # A permuted copy of the model (orig_index) is only taken by inference frames on the default sort / placement
            # path (gsr_forward rejects it elsewhere: api.hip make_plan): tile grids up to 16384 tiles and 256 tiles
            # wide, no A/B selector that leaves that path.  Where a camera cannot have that, the loop keeps the model in
            # the caller's order and hands over the block bounds alone (valid for any order, any path; rarely tight).
            reorder = all(self._takes_permuted_model(c, int(self.xyz.shape[0])) for c in self.cameras)
            L = SceneLayout.build(self.xyz, self.scaling, self.rotation,
                                  labels=semantics.detach().to(dev, torch.float32).reshape(-1),
                                  param_space=RAW_SCALES | RAW_ROTATIONS, reorder=reorder, features_dc=self.features_dc,
                                  features_rest=self.features_rest, opacity=self.opacity)
            a = L.arrays
            self.xyz, self.scaling, self.rotation = a["means3D"], a["scales"], a["rotations"]
            self.features_dc, self.features_rest, self.opacity = a["features_dc"], a["features_rest"], a["opacity"]
            semantics = a["labels"]
            self.layout = L.layout
            self.perm = L.perm  # (position in the loop's arrays -> number in the caller's model)
        self._semantics = semantics
        self.map_kinds = tuple(m for m in MAP_KINDS if m in maps)
        # (what the maps pass writes: the kinds asked for, and both when a point cloud is made from them)
        self._map_kinds_run = MAP_KINDS if pointcloud is not None else self.map_kinds
        self.depth_scale = float(depth_scale)
        # (the labels of the loop's own arrays -- the permuted copy when laid out -- checked once)
        self._map_labels = check_map_labels(semantics.to(dev)) if "segmentation" in self._map_kinds_run else None
        self.op = tf.FusedPartTransform(part_labels, semantics.to(dev), scaled_parts=scaled_parts)
        self.rescaled = len(tuple(scaled_parts)) > 0
        if self.num_envs > 1:
            # A part with EXACTLY num_envs Gaussians takes a degenerate branch in the reference (gs_utils.py:331
            # `rot_mat.size(0) == xyz.size(0)`: Gaussian g is rotated by environment g's matrix; the wrapper's
            # `shape[0] == num_envs` write-back then broadcasts row i over the part -- recorded from the reference
            # itself in tests/golden/wrapper_glue.npz).  That is an accident of shapes, not a behaviour anyone relies
            # on; it is not mirrored here: every part moves rigidly under its environment's pose.  Say so, loudly.
            lab = semantics.reshape(-1).long()
            for name, labels in part_labels.items():
                ids = torch.as_tensor(labels if isinstance(labels, (list, tuple)) else [labels], device=lab.device)
                if int(torch.isin(lab, ids.long()).sum()) == self.num_envs:
                    import warnings

                    warnings.warn(f"part {name!r} has exactly num_envs = {self.num_envs} Gaussians: the reference's "
                                  "shape tests mis-broadcast such a part; it is moved rigidly here", stacklevel=2)
        self.fuse_transform = bool(fuse_transform)
        self.K = len(self.op.names)
        H, W = self.cameras[0].image_height, self.cameras[0].image_width
        self.frames = {n: torch.zeros((self.num_envs, c.image_height, c.image_width, 3), dtype=torch.uint8, device=dev)
                       for n, c in zip(self.names, self.cameras)}
        dts = {"segmentation": torch.int16, "depth": torch.float32}
        self._map_bufs = {n: {m: torch.zeros((self.num_envs, c.image_height, c.image_width, 1), dtype=dts[m], device=dev)
                              for m in self._map_kinds_run} for n, c in zip(self.names, self.cameras)} \
            if self._map_kinds_run else None
        self.maps = {n: {m: b[m] for m in self.map_kinds} for n, b in self._map_bufs.items()} if self.map_kinds else None
        self._maps_pack = None  # (the gsr_render_maps arguments of the lanes, and the state addresses they were built for)
        if appearance is None:
            self.bg = torch.zeros(3, device=dev) if background is None else background.to(dev, torch.float32)
        # the loop never differentiates a frame: inference frames (GsrSettings.forward_only), no radii array
        lanes = self.num_envs * len(self.cameras)
        if bound_capacity == "auto":
            per_lane = max(4 * int(self.xyz.shape[0]) * ((c.image_width + 15) // 16) * ((c.image_height + 15) // 16)
                           for c in self.cameras)
            free = torch.cuda.mem_get_info(dev)[0] if dev.type == "cuda" and torch.cuda.is_available() else 0
            bound_capacity = lanes * per_lane <= min(free // 4, 64 << 30)
        # (... and keeps the uint8 frames only: where the frames take the compositor that can leave the float images out --
        #  inference frames on the default path, the library's own answer -- they are not written either)
        from ._lib import plan_query

        plans = [plan_query(c.image_width, c.image_height, int(self.xyz.shape[0]), forward_only=True) for c in self.cameras]
        no_float = not keep_float and all(p is not None and p["super"] for p in plans)
        self.multi = MultiCameraRenderer(lanes, dev, forward_only=True, want_radii=False, want_float=not no_float, growth=growth,
                                         min_capacity=(2 * int(self.xyz.shape[0]) if min_capacity is None else int(min_capacity)),
                                         bound_capacity=bool(bound_capacity), overflow_mirror=True, batched=batched)
        # Six frames and more per step (three environments with two cameras) go as at least TWO sets of launches on streams of
        # their own (MultiCameraRenderer: up to three in flight), at most eight frames each: the latency-bound stages of one
        # set are filled by the other's.  Same box, configs[2]'s surrogate / the arm-shaped one, frames/s enqueued ahead:
        # 4 environments 14.0 -> 14.6 k / 17.8 -> 18.0 k (policy in the loop 13.5 -> 14.1 / 16.8 -> 17.5), 8 environments
        # 14.2 -> 16.5 k / 17.9 -> 21.4 k, 16 environments 14.1 -> 16.9 k / 17.3 -> 22.0 k.  Fewer frames stay one set (two
        # environments as 2 + 2: 11.6 -> 11.4 k).
        if lanes >= 6:  # (three environments as 3 + 3 frames: 12.95 -> 13.2 k, policy in the loop 12.4 -> 12.8 k)
            self.multi.set_frames = min(8, (lanes + 1) // 2)
        self.recovered_steps = 0      # steps re-rendered because a lane had overflowed (see step())
        self.late_overflow_frames = 0  # overflowed frames that were only noticed after their step had been returned
        lead = (self.num_envs, self.K) if self.num_envs > 1 else (self.K,)
        # Everything a step reads that changes from step to step -- part matrices, uniform scales, camera matrices --
        # lives in ONE device vector: `matrices`, `scales` and the cameras' tensors are views into it.  Values handed over
        # as HOST tensors (the usual case: a CPU simulator, a test) are collected in a host mirror and go up in one copy
        # per step (round 4: five small copies, 5 us each on the step's stream, 8 % of a step); device tensors (ManiSkill
        # link poses on the GPU) are copied view by view, device to device.
        nm, ns = self.num_envs * self.K * 16, self.num_envs * self.K
        self._seg = {"poses": (0, nm + (ns + 3) // 4 * 4)}
        off = self._seg["poses"][1]
        # (per_env_cameras: E records per camera, environment e's at +36 e)
        self._ecam = self.num_envs if self.per_env_cameras else 1
        for n in self.names:
            self._seg[n] = (off, off + 36 * self._ecam)  # world_view (16) | full_proj (16) | centre (3) + pad
            off += 36 * self._ecam
        # with sim2real: the simulator's extrinsics (12 floats per record) travel in the staging vector too, and
        # gsr_cameras_from_extrinsics turns them into the records above on the device, inside the step
        self._ext_segs = ["ext:" + n for n in self.names] if self._sim2real is not None else []
        for n in self._ext_segs:
            self._seg[n] = (off, off + 12 * self._ecam)
            off += 12 * self._ecam
        # with appearance: per environment its G x 12 table and background (may come from device tensors) and, apart, the
        # G + 1 version words of the block cache (always from the host: the loop draws them)
        G = self._app_G
        app_segs = []
        if G:
            self._app_stride, self._ver_stride = G * 12 + 4, (G + 1 + 3) // 4 * 4
            self._seg["app"] = (off, off + self.num_envs * self._app_stride)
            off = self._seg["app"][1]
            self._seg["appver"] = (off, off + self.num_envs * self._ver_stride)
            off = self._seg["appver"][1]
            app_segs = ["app", "appver"]
        self._seg_order = ["poses"] + self.names + self._ext_segs + app_segs
        self._stage = torch.zeros(off, device=dev)
        self._host = torch.zeros(off)
        pin = dev.type == "cuda" and torch.cuda.is_available()
        self._ring = [torch.zeros(off).pin_memory() if pin else torch.zeros(off) for _ in range(8)]
        self._ring_ev, self._ring_k, self._ring_waited = [None] * len(self._ring), 0, -1
        self._on_gpu = pin
        self._dirty, self._stale = set(), set()  # segments changed on the host / last written from a device tensor

        def views(buf):
            v = {"matrices": buf[:nm].view(*lead, 4, 4), "scales": buf[nm:nm + ns].view(lead)}
            for n in self.names:
                o = self._seg[n][0]
                v[n] = [(buf[r:r + 16].view(4, 4), buf[r + 16:r + 32].view(4, 4), buf[r + 32:r + 35])
                        for r in range(o, o + 36 * self._ecam, 36)]
            for n in self._ext_segs:
                o = self._seg[n][0]
                v[n] = buf[o:o + 12 * self._ecam].view(self._ecam, 3, 4)
            if G:
                lo, hi = self._seg["app"]
                rows = buf[lo:hi].view(self.num_envs, self._app_stride)
                v["app_tables"], v["app_bg"] = rows[:, :G * 12].view(self.num_envs, G, 3, 4), rows[:, G * 12:G * 12 + 3]
                lo, hi = self._seg["appver"]
                v["appver"] = buf[lo:hi].view(self.num_envs, self._ver_stride)
            return v

        self._hv, dv = views(self._host), views(self._stage)
        # (the same host memory as numpy arrays: what a step writes into the mirror and the ring are a dozen copies of a
        #  few hundred bytes, ~0.4 us each through numpy against 1.5-2 us through a torch op -- with the policy in the loop
        #  the host's share of a step is on the critical path: round 6, tools/host_step_profile.py)
        self._hv_np = {k: ([tuple(x.numpy() for x in r) for r in v] if isinstance(v, list) else v.numpy())
                       for k, v in self._hv.items()}
        self._host_np = self._host.numpy()
        self._ring_np = [r.numpy() for r in self._ring]
        self._hv["matrices"].copy_(torch.eye(4).expand(*lead, 4, 4))
        self._hv["scales"].fill_(1.0)
        if G:
            import random

            self._ver_next = random.getrandbits(23)
            self._hv["app_tables"].copy_(torch.eye(3, 4).expand(self.num_envs, G, 3, 4))
            if background is not None:
                self._hv["app_bg"].copy_(torch.as_tensor(background).detach().to("cpu", torch.float32).expand(self.num_envs, 3))
            self._new_versions(range(self.num_envs))
        from .camera import ViewParams

        self.env_cameras = {}
        for n in self.names:
            recs = []
            for j, cam in enumerate(cam_lists[n]):
                for dst, src in zip(self._hv[n][j], (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)):
                    dst.copy_(src.detach().to("cpu", torch.float32))
                recs.append(ViewParams(cam.image_width, cam.image_height, cam.FoVx, cam.FoVy, *dv[n][j]))
            self.env_cameras[n] = recs if self.per_env_cameras else recs * self.num_envs
        self.cameras = [self.env_cameras[n][0] for n in self.names]
        self._stage.copy_(self._host)
        # extrinsic-fed cameras (set_extrinsics): their records are written by gsr_cameras_from_extrinsics from the staged
        # extrinsics at the start of every step; the call's pack is rebuilt when the set of such cameras changes
        self._dv = dv
        self._ext_names, self._cams_pack, self._ext_changed = [], None, False
        if self._sim2real is not None:
            from .camera import sensor_projection

            # (one float32 projection per record, fixed for the loop's lifetime: camera by camera, environment e at +16 e)
            self._proj = torch.stack([sensor_projection(c.FoVx, c.FoVy) for n in self.names
                                      for c in self.env_cameras[n][:self._ecam]]).to(dev).contiguous()
        # the point cloud's call, packed once: every buffer it reads or writes is the loop's own and never moves (the camera
        # matrices are the device views of the staging vector, rewritten every step before the frames read them)
        self.pointcloud, self._cloud_pack = None, None
        if pointcloud is not None:
            from .pointcloud import prepare

            cams = dict(self.env_cameras) if self.per_env_cameras else dict(zip(self.names, self.cameras))
            self._cloud_pack = prepare({n: b["depth"] for n, b in self._map_bufs.items()},
                                       {n: b["segmentation"] for n, b in self._map_bufs.items()}, self.frames, cams,
                                       pointcloud, self.depth_scale, device=dev)
            self.pointcloud = self._cloud_pack[1]
        # device-resident pose buffers: what a GPU simulator hands over (ManiSkill link poses are device tensors)
        self.matrices, self.scales = dv["matrices"], dv["scales"]
        if G:
            # (environment e's frames read row block e, background e and version words e of the staging vector)
            self._app_lut = torch.as_tensor(app_lut).to(dev)
            self._app_labels = None if self.fuse_transform else \
                semantics.detach().reshape(-1).to(dev, torch.float32).contiguous()  # (fused: the part labels)
            self.bg = dv["app_bg"]
            self.appearance_tables, self.appearance_backgrounds = dv["app_tables"], dv["app_bg"]
        # The 17-float pose table(s) the frames read (fuse_transform) live in one persistent buffer and are packed WHERE THE
        # POSES ARRIVE, not inside the step: host poses by the kernel that brings the step's host values to the device
        # (gsr_stage_step reads the pinned slot directly: one launch instead of an H2D copy + the pack kernel), device
        # poses by gsr_pack_part_transforms right behind their device-to-device copy (set_poses).
        self._table = None
        self._ring_dev = None  # device-visible addresses of the pinned slots (gsr_pinned_device_address), resolved once
        if self.fuse_transform and pin:
            import ctypes as C

            from ._lib import lib

            self._table = self.op.pack_on_device(self.matrices, self.scales)
            addr = []
            for slot in self._ring:
                d = C.c_void_p()
                if lib().gsr_pinned_device_address(C.c_void_p(slot.data_ptr()), C.byref(d)) != 0:
                    addr = None  # (not device-visible: the steps' host values go up by copies, the table by its own kernel)
                    break
                addr.append(d.value)
            self._ring_dev = addr
        # The model is this object's own copy (laid out at construction, never written afterwards): the frames may keep the
        # blocks of 256 Gaussians whose camera and part pose are the previous frame's bit for bit (include/gsr.h
        # GSR_MODEL_VERSION; csrc/preprocess.hip prep_block_cached) -- under a fixed sensor camera everything that is not a
        # robot link or a tracked object.  A random version per object: a state buffer the allocator hands from one loop to
        # another never vouches for the other's model.  ``block_cache=False``: every block recomputed every frame.
        import random

        self._model_version = model_version(random.getrandbits(24) | 1) if (block_cache and self.fuse_transform and
                                                                            self.layout is not None) else 0
        if self._model_version != 0 and tile_reuse and not keep_float:
            self._model_version |= FRAME_KEPT
        self._graph = None    # the captured step (host values staged OUTSIDE it: a copy / a launch between two replays) ...
        self._graphs = None   # ... or one captured step per ring slot, each staging its slot itself (see capture())
        self._pack = None     # the step's argument pack (MultiCameraRenderer.last_pack): eager steps without the Python
        self.eager_when_ahead = True  # step(ensure=False) issues the launches one by one instead of replaying the graph
        self._stage_fn = getattr(_C._ext, "stage_host_values", None) if _C._ext is not None else None
        self._sync_fn = getattr(_C._ext, "sync_current_stream", None) if (_C._ext is not None and dev.type == "cuda") else None
        self._dev_index = dev.index if dev.index is not None else (torch.cuda.current_device() if dev.type == "cuda" else 0)
        self._mat_shape = tuple(self.matrices.shape)
        self._cam_meta = {n: (self._seg[n][0], c.image_width, c.image_height,
                              [(v.FoVx, v.FoVy) for v in self.env_cameras[n][:self._ecam]])
                          for n, c in zip(self.names, self.cameras)}
        self.eager_when_waited = False  # ... step(ensure=True) too (A/B: the graph's one submission against eleven launches)
        self.image_size = (H, W)

    @staticmethod
    def _takes_permuted_model(cam, P: int) -> bool:
        """Will a frame of this camera over a model of ``P`` Gaussians be an inference frame on the default sort /
        placement path (the only frames that take ``GsrInputs.orig_index``)?  The library's own decision
        (``gsr_plan_query`` = csrc/api.hip make_plan, asked on the host): tile grids up to 16384 tiles and 256 tiles wide,
        no A/B selector that leaves the path, and a model the sample sort takes (up to 8 388 608 Gaussians -- beyond that
        the frames fall back to the LSD radix depth sort, which knows nothing of a permutation)."""
        from ._lib import plan_query

        plan = plan_query(cam.image_width, cam.image_height, P, permuted=True, forward_only=True)
        return plan is not None and bool(plan["infer"])

    # ---- one step ------------------------------------------------------------------------------------------------
    def _gpu_step(self):
        """Everything the GPU does per step: pose table, fused transform, E x C frames (reads self.matrices / scales)."""
        E, C = self.num_envs, len(self.cameras)
        if not (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self._flush()
        self._run_cameras()
        if self.fuse_transform:
            # (the pose table was packed when the poses arrived: _flush / set_poses)
            parts = self.op.parts_of_table(self._table) if self._table is not None else \
                self.op.parts(self.matrices, self.scales)
            views, outs, per_lane = [], [], []
            for e in range(E):
                for c in range(C):
                    views.append(self.env_cameras[self.names[c]][e])
                    outs.append(self.frames[self.names[c]][e])
                    per_lane.append(dict(parts=parts if E == 1 else parts[e], **self._app_lane(e)))
            self.multi.render(views, self.xyz, self.opacity, rgb8_out=outs, shs=self.features_dc,
                              shs_rest=self.features_rest, scales=self.scaling, rotations=self.rotation,
                              param_space=RAW_SCALES | RAW_ROTATIONS | self._model_version, bg=self.bg, per_lane=per_lane,
                              layout=self.layout)
            self._run_maps()
            return
        if self.rescaled:
            xyz, rot, scaling = self.op.apply(self.xyz, self.rotation, self.matrices, self.scales, scaling=self.scaling)
        else:
            xyz, rot = self.op.apply(self.xyz, self.rotation, self.matrices, self.scales)
            scaling = self.scaling
        # lane e * C + c renders environment e from camera c; the transformed quaternions keep their norm (reference
        # semantics) and the scales stay logs: preprocess activates both on load
        views, outs = [], []
        for e in range(E):
            for c in range(C):
                views.append(self.env_cameras[self.names[c]][e])
                outs.append(self.frames[self.names[c]][e])
        if E == 1:
            self.multi.render(views, xyz, self.opacity, rgb8_out=outs, shs=self.features_dc,
                              shs_rest=self.features_rest, scales=scaling, rotations=rot,
                              param_space=RAW_SCALES | RAW_ROTATIONS, bg=self.bg,
                              per_lane=[self._app_lane(0) for _ in range(C)] if self._app_G else None)
        else:
            per_lane = [dict(means3D=xyz[e], scales=(scaling[e] if scaling.dim() == 3 else scaling), rotations=rot[e],
                             **self._app_lane(e)) for e in range(E) for _ in range(C)]
            self.multi.render(views, None, self.opacity, rgb8_out=outs, shs=self.features_dc,
                              shs_rest=self.features_rest, param_space=RAW_SCALES | RAW_ROTATIONS, bg=self.bg,
                              per_lane=per_lane)
        self._run_maps()

    def _app_lane(self, e: int) -> dict:
        """The per-lane render arguments of environment e's appearance (device views of the staging vector), or {}."""
        if not self._app_G:
            return {}
        return dict(appearance=(self._dv["app_tables"][e], self._app_lut, self._app_labels,
                                self._dv["appver"][e, :self._app_G + 1].view(torch.int32)),
                    bg=self._dv["app_bg"][e])

    def _new_versions(self, env_ids):
        """Fresh block-cache version words for these environments (every group and the whole table): what a table handed
        over promises to the frames (include/gsr.h GsrInputs.appearance_versions) -- bit patterns of floats in [1, 2), so that
        the staging copy moves them as they are."""
        words = self._hv_np["appver"].view(np.uint32)
        G = self._app_G
        for e in env_ids:
            for k in range(G + 1):
                self._ver_next = (self._ver_next + 1) & 0x7FFFFF
                words[e, k] = 0x3F800000 | self._ver_next
        self._dirty.add("appver")

    def set_appearance(self, tables, backgrounds=None, env_ids=None):
        """Appearance of the next steps: ``tables`` ``(n, G, 3, 4)`` float32 colour affines (group 0 first, then the named
        groups in the order given at construction; :class:`gsworld_amd.appearance.AppearanceRandomizer` draws them) and
        optional ``backgrounds`` ``(n, 3)``, for all environments (n = E) or the ``env_ids`` given (a partial reset), on the
        host or the device.  Host values travel with the step's other host values (no synchronisation, no re-capture);
        device values are copied device to device -- the first of them on a loop with staged graphs makes the next step
        capture once more, as device poses do, and host values after device ones read the segment back once (a blocking
        copy).  Every table handed over counts as changed: the frames of those environments recompute their blocks once
        (block cache, tile reuse), then keep them while the table rests."""
        if not self._app_G:
            raise ValueError("set_appearance needs a loop built with appearance={group name: labels}")
        from .appearance import check_tables

        t, b, ids = check_tables(tables, backgrounds, env_ids, self.num_envs, self._app_G)
        for name, val, seg in (("app_tables", t, "app"), ("app_bg", b, "app")):
            if val is None:
                continue
            if val.is_cuda:
                self._flush()
                for j, e in enumerate(ids):
                    self._dv[name][e].copy_(val[j], non_blocking=True)
                self._stale.add(seg)
            else:
                if seg in self._stale and seg not in self._dirty:
                    # (the segment was last written from device tensors: its other rows are read back once -- a host
                    #  synchronisation on the change from device to host tables only)
                    lo, hi = self._seg[seg]
                    self._host[lo:hi].copy_(self._stage[lo:hi].to("cpu"))
                hv = self._hv_np[name]
                src = val.detach().cpu().numpy()
                for j, e in enumerate(ids):
                    hv[e] = src[j]
                self._dirty.add(seg)
        self._new_versions(ids)

    def _run_cameras(self):
        """The records of the extrinsic-fed cameras from their staged extrinsics (``gsr_cameras_from_extrinsics``, one
        launch on the current stream, capturable) -- behind the step's staging, ahead of its frames."""
        if self._ext_names:
            _C.run_cameras(self._cameras_pack(), self.device)

    def _cameras_pack(self):
        """The ``gsr_cameras_from_extrinsics`` arguments of the current set of extrinsic-fed cameras (built when the set
        changes, outside any capture: set_extrinsics / set_cameras): views environment-major, every record read and
        written in place in the staging vector."""
        if self._cams_pack is None:
            offs = []
            for e in range(self._ecam):
                for n in self._ext_names:
                    c = self.names.index(n)
                    offs += [self._seg["ext:" + n][0] + 12 * e, 16 * (c * self._ecam + e), self._seg[n][0] + 36 * e]
            t = torch.tensor(offs, dtype=torch.int32, device=self.device)
            rigid, scale = self._sim2real
            self._cams_pack = (_C.pack_cameras(len(offs) // 3, self._stage, self._proj, self._stage, t, rigid, scale), t)
        return self._cams_pack[0]

    def _ext_set(self, names):
        """The extrinsic-fed cameras are now ``names``: a new call pack, and a captured step is captured again."""
        names = [n for n in self.names if n in names]
        if names != self._ext_names:
            self._ext_names, self._cams_pack, self._ext_changed = names, None, True
            if names:
                self._cameras_pack()

    def _run_maps(self):
        """The step's segmentation / depth maps (``maps``), behind its frames on the current stream: one ``gsr_render_maps``
        call over every lane (capturable), then the point cloud from them (``pointcloud``).  The argument pack is kept while
        no lane's state buffer moves."""
        if self._map_bufs is None:
            return
        lanes = self.multi.lanes
        key = tuple(l._map_key() for l in lanes)
        if self._maps_pack is None or self._maps_pack[0] != key:
            C = len(self.cameras)
            frames = []
            for k, lane in enumerate(lanes):
                e, name = k // C, self.names[k % C]
                m = self._map_bufs[name]
                seg, dep = m.get("segmentation"), m.get("depth")
                f, _, _ = lane._map_frame(self._map_labels if seg is not None else None, self.depth_scale,
                                          seg[e].view(seg.shape[1], seg.shape[2]) if seg is not None else None,
                                          dep[e].view(dep.shape[1], dep.shape[2]) if dep is not None else None)
                if dep is None:
                    f["out_depth"] = None  # (_map_frame allocated one: the loop was not asked for depth)
                frames.append(f)
            self._maps_pack = (key, _C.pack_maps(frames))
        _C.run_maps(self._maps_pack[1], self.device)
        if self._cloud_pack is not None:
            _C.run_pointcloud(self._cloud_pack[0], self.device)

    def _flush(self):
        """Host-side changes since the last flush go up in as few copies as possible: one contiguous run of the staging
        vector from the first to the last changed segment, unless a segment in between was last written from a DEVICE
        tensor (its host mirror is stale: the run is cut around it).  Every copy reads from its own pinned slot of a
        ring, so the caller may overwrite its tensors -- and this object its mirror -- right away."""
        if not self._dirty:
            return
        order = self._seg_order
        runs, cur = [], None
        first = min(order.index(n) for n in self._dirty)
        last = max(order.index(n) for n in self._dirty)
        for n in order[first:last + 1]:
            if n in self._stale and n not in self._dirty:
                cur = None
                continue
            lo, hi = self._seg[n]
            if cur is None:
                cur = [lo, hi]
                runs.append(cur)
            else:
                cur[1] = hi
        for lo, hi in runs:
            k = self._slot_acquire()
            slot = self._ring[k]
            slot[lo:hi].copy_(self._host[lo:hi])
            if not self._stage_poses(k, lo, hi):
                self._stage[lo:hi].copy_(slot[lo:hi], non_blocking=True)
            self._slot_release(k, False)
        self._stale -= self._dirty
        self._dirty.clear()

    def _stage_poses(self, k: int, lo: int, hi: int) -> bool:
        """A run of the staging vector that holds this step's poses goes up through ``gsr_stage_step``: the kernel reads
        pinned slot ``k`` itself, writes the device twin and packs the pose table(s) in the same launch.  -> False: not
        such a run (cameras only), or no pose table to pack -- the caller copies."""
        if self._table is None or self._ring_dev is None or lo != 0 or "poses" not in self._dirty:
            return False
        self._launch_stage(k, hi)
        return True

    def _launch_stage(self, k: int, n: int):
        """``gsr_stage_step`` of the first ``n`` floats of ring slot ``k`` on the current stream (capturable)."""
        import ctypes as C

        from ._lib import check, lib

        nm, ns = self.num_envs * self.K * 16, self.num_envs * self.K
        with torch.cuda.device(self.device):
            check(lib().gsr_stage_step(n, C.c_void_p(self._ring_dev[k]), C.c_void_p(self._stage.data_ptr()), ns, 0, nm,
                                       C.c_void_p(self._table.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    def _slot_stage(self) -> int:
        """The host mirror into the next pinned ring slot (what the step's staging kernel reads)."""
        k = self._slot_acquire()
        np.copyto(self._ring_np[k], self._host_np)
        self._dirty.clear()
        return k

    def _stage_host_values_fast(self, matrices, scales, cameras, extrinsics=None):
        """This step's poses and cameras -- plain host float32 tensors, the usual case -- into the host mirror and the next
        ring slot in ONE call into the compiled binding (csrc_torch/ext.cpp stage_host_values) instead of set_poses +
        set_cameras + the ring copy: 13 -> ~4 us of host work that sits on the critical path of a waited-for step.
        Returns the slot, or None when anything is not of that kind (nothing written: the general path takes over)."""
        segs = []
        if matrices is not None:
            # (device tensors, other dtypes, strided views: the compiled side says no and nothing is written)
            if tuple(matrices.shape) != self._mat_shape or (scales is not None and scales.numel() != self.num_envs * self.K):
                return None
            segs.append((0, matrices))
            if scales is not None:
                segs.append((self.num_envs * self.K * 16, scales))
        if cameras:
            for name, cams in cameras.items():
                meta = self._cam_meta.get(name)
                if meta is None or name in self._ext_names:
                    return None  # (set_cameras raises the KeyError / takes the camera off the extrinsic-fed set)
                o, w, h, fovs = meta
                if isinstance(cams, (list, tuple)):
                    if len(cams) != len(fovs):
                        return None
                else:
                    cams = [cams] * len(fovs)
                for j, (cam, (fx, fy)) in enumerate(zip(cams, fovs)):
                    if cam.image_width != w or cam.image_height != h or abs(cam.FoVx - fx) > 1e-9 or \
                            abs(cam.FoVy - fy) > 1e-9:
                        return None  # (set_cameras raises the ValueError)
                    wv, fp, cc = cam.world_view_transform, cam.full_proj_transform, cam.camera_center
                    if wv.numel() != 16 or fp.numel() != 16 or cc.numel() != 3:
                        return None
                    r = o + 36 * j
                    segs += [(r, wv), (r + 16, fp), (r + 32, cc)]
        if extrinsics:
            for name, ext in extrinsics.items():
                if name not in self._ext_names or not isinstance(ext, torch.Tensor) or ext.numel() != 12 * self._ecam:
                    return None  # (set_extrinsics adds the camera or raises)
                segs.append((self._seg["ext:" + name][0], ext))
        # (the slot is taken before the write: its last reader has finished by then)
        ring_k, ring_ev, waited = self._ring_k, list(self._ring_ev), self._ring_waited
        k = self._slot_acquire()
        if not self._stage_fn(self._host, self._ring[k], segs):
            self._ring_k, self._ring_ev, self._ring_waited = ring_k, ring_ev, waited  # (slot handed back)
            return None
        self._dirty.clear()
        return k

    def set_poses(self, matrices: torch.Tensor, scales: torch.Tensor | None = None):
        """This step's part poses ((K,4,4) or (E,K,4,4), host or device; + uniform scales) for the persistent device
        buffers the (possibly captured) step reads.  Host tensors are taken over at once (the caller may reuse them) and
        uploaded with the step's other host values in one copy; device tensors are copied device to device."""
        if tuple(matrices.shape) != tuple(self.matrices.shape):
            raise ValueError(f"expected poses of shape {tuple(self.matrices.shape)}, got {tuple(matrices.shape)}")
        if matrices.is_cuda or (scales is not None and scales.is_cuda):
            self._flush()  # (host values set earlier keep their order with respect to this write)
            self.matrices.copy_(matrices.to(torch.float32), non_blocking=True)
            if scales is not None:
                self.scales.copy_(scales.to(torch.float32).reshape(self.scales.shape), non_blocking=True)
            if self._table is not None:
                self.op.pack_on_device(self.matrices, self.scales)  # (into self._table: the buffer is persistent)
            self._stale.add("poses")
            return
        if "poses" in self._stale and scales is None:
            # the poses were last written from device tensors: the mirror's scales are read back once (a host
            # synchronisation on the change from device to host poses only -- a GPU simulator that falls back to host
            # poses in mid-rollout keeps going)
            self._hv["scales"].copy_(self.scales.detach().to("cpu"))
        _to_mirror(self._hv["matrices"], self._hv_np["matrices"], matrices)
        if scales is not None:
            _to_mirror(self._hv["scales"], self._hv_np["scales"], scales)
        self._dirty.add("poses")

    def set_cameras(self, cameras: dict):
        """This step's camera poses: ``{name: ViewParams}`` for any subset of the cameras given at construction -- the
        wrapper recomputes them from the simulator's sensor parameters on every render
        (gs_world_wrapper.py:238 ``self.gs_cam = self.cam_maniskill2gs(self.base_env.get_sensor_params(), ...)``), which
        is how a wrist-mounted camera follows the arm.  The matrices are copied INTO the device tensors the (possibly
        captured) step reads; image size and field of view are part of the launch and must not change."""
        lists = {}
        for name, cam in cameras.items():
            if name not in self.names:
                raise KeyError(f"unknown camera {name!r} (known: {self.names})")
            lists[name] = _camera_list(name, cam, self.num_envs, self.per_env_cameras)
            for cam, mine in zip(lists[name], self.env_cameras[name]):
                if (cam.image_width, cam.image_height) != (mine.image_width, mine.image_height) or \
                        abs(cam.FoVx - mine.FoVx) > 1e-9 or abs(cam.FoVy - mine.FoVy) > 1e-9:
                    raise ValueError(f"camera {name!r}: image size / field of view are fixed at construction")
        for name, cams in lists.items():
            srcs = [(c.world_view_transform, c.full_proj_transform, c.camera_center) for c in cams]
            if any(t.is_cuda for src in srcs for t in src):
                self._flush()
                for mine, src in zip(self.env_cameras[name], srcs):
                    for dst, t in zip((mine.world_view_transform, mine.full_proj_transform, mine.camera_center), src):
                        dst.copy_(t.to(torch.float32), non_blocking=True)
                self._stale.add(name)
            else:
                for j, src in enumerate(srcs):
                    for dst, dst_np, t in zip(self._hv[name][j], self._hv_np[name][j], src):
                        _to_mirror(dst, dst_np, t)
                self._dirty.add(name)
        if any(n in self._ext_names for n in lists):
            self._ext_set([n for n in self._ext_names if n not in lists])

    def set_extrinsics(self, extrinsics: dict):
        """This step's camera poses as the simulator holds them: ``{name: extrinsic_cv}`` (OpenCV world -> camera, float32;
        ManiSkill ``base_env.get_sensor_params()[name]["extrinsic_cv"]``), ``(E,3,4)`` with ``per_env_cameras`` or
        ``(3,4)`` / ``(1,3,4)`` without, on the host or the device.  Needs ``sim2real`` at construction.  Host values travel
        with the step's other host values; device values are copied device to device into the loop's buffer.  The step then
        computes the cameras' records on the GPU (include/gsr.h ``gsr_cameras_from_extrinsics``: what ``cam_maniskill2gs``
        computes on the host, with each camera's field of view as given at construction) before its frames read them.  A
        camera stays extrinsic-fed until :meth:`set_cameras` hands it a ViewParams again."""
        checked = {}
        for name, ext in extrinsics.items():
            if name not in self.names:
                raise KeyError(f"unknown camera {name!r} (known: {self.names})")
            checked[name] = check_extrinsics(name, ext, self.num_envs, self.per_env_cameras, self._sim2real is not None)
        for name, t in checked.items():
            seg = "ext:" + name
            if t.is_cuda:
                self._flush()
                self._dv[seg].copy_(t, non_blocking=True)
                self._stale.add(seg)
            else:
                _to_mirror(self._hv[seg], self._hv_np[seg], t)
                self._dirty.add(seg)
        self._ext_set(self._ext_names + list(checked))

    def step(self, matrices: torch.Tensor | None = None, scales: torch.Tensor | None = None,
             cameras: dict | None = None, ensure: bool = False, extrinsics: dict | None = None, appearance=None) -> dict:
        """-> {camera name: uint8 (num_envs, H, W, 3)} -- renderer-owned tensors, overwritten by the next step.

        ``cameras``: as :meth:`set_cameras`; ``extrinsics``: as :meth:`set_extrinsics` (this step's simulator sensor poses);
        ``appearance``: as :meth:`set_appearance` -- the ``(E, G, 3, 4)`` tables, or a dict of its keyword arguments.

        A lane whose instance list is sized from earlier frames (no ``bound_capacity``) can be outgrown by a later frame
        -- an arm swinging past a wrist camera triples the count -- and such a frame shows the background only.  That is
        never silent here: every frame copies its state's overflow count to pinned host memory
        (``FrameRenderer(overflow_mirror=True)``, 8 bytes, also under graph replay), and this method compares the counts
        it can see with the ones it has handled, WITHOUT synchronising:

        * ``ensure=True`` -- what a closed loop does anyway, since the policy reads the frames before it acts: wait for
          this step's frames, and if a lane overflowed, grow it, re-render the step and re-capture the graph.  The
          frames returned are always valid.
        * ``ensure=False`` (throughput mode): no wait.  An overflow of an EARLIER step shows up here as soon as its
          mirror copy has landed (normally within a step or two); the loop then recovers as above -- the current step
          is rendered correctly -- and :attr:`late_overflow_frames` counts the frames that had already been handed out
          invalid."""
        if appearance is not None:
            if isinstance(appearance, dict):
                self.set_appearance(**appearance)
            else:
                self.set_appearance(appearance)
        pre_k = None
        if self._graphs is not None and not self._stale and self._stage_fn is not None:
            # (None: not plain host tensors -- the general path)
            pre_k = self._stage_host_values_fast(matrices, scales, cameras, extrinsics)
        if pre_k is None:
            if matrices is not None:
                self.set_poses(matrices, scales)
            if cameras:
                self.set_cameras(cameras)
            if extrinsics:
                self.set_extrinsics(extrinsics)
        if (self._graphs is not None and self._stale) or (self._ext_changed and self.captured):
            # (device tensors arrived since the capture: their values must not be staged over; or the set of extrinsic-fed
            #  cameras changed: the captured conversion launch converts the old set)
            self.capture()
        if (not ensure or self.eager_when_waited) and self.eager_when_ahead and self._pack is not None and \
                self._table is not None and self._ring_dev is not None and not self._stale and \
                (self._graphs is not None or self._graph is None):
            # Steps enqueued AHEAD of the device (nobody waits for this step's frames before the next is issued): the step's
            # eleven launches one by one, from the argument pack of the last eager step.  Two graph replays in a row leave the
            # device idle for ~14 us between them (kernel trace: the last kernel of one to the first of the next, however far
            # ahead the host is); launches queue back to back.  8.58 k against 8.36 k frames/s on the configs[2] surrogate.
            # With the policy in the loop the graph wins -- one submission instead of eleven in front of every wait: 7.67 k
            # against 7.25 k -- and `ensure=True` takes it.
            k = pre_k if pre_k is not None else self._slot_stage()
            pack, caps = self._pack
            if pack[0] == "pack" and (not self._ext_names or self._cameras_pack()[0] == "ext"):
                # (the staging kernel and the frames' launches in ONE call into the compiled binding: csrc_torch/ext.cpp StepPack)
                nm, ns = self.num_envs * self.K * 16, self.num_envs * self.K
                with torch.cuda.device(self.device):
                    if self._ext_names:  # (the camera records of the staged extrinsics between staging and frames)
                        pack[1].run_staged_cams(int(self._stage.numel()), self._ring_dev[k], self._stage.data_ptr(), ns, 0,
                                                nm, self._table.data_ptr(), self._cameras_pack()[1])
                    else:
                        pack[1].run_staged(int(self._stage.numel()), self._ring_dev[k], self._stage.data_ptr(), ns, 0, nm,
                                           self._table.data_ptr())
                for lane, cap in caps:
                    lane._finish(cap)
            else:
                self._launch_stage(k, int(self._stage.numel()))
                self._run_cameras()
                self.multi.rerun(self._pack)
            self._run_maps()
            self._slot_release(k, ensure)
        elif self._graphs is not None:
            # this step's host values travel INSIDE its graph: the whole mirror into the next pinned slot (a host copy of a
            # kilobyte), then the replay of the graph that was captured reading that slot
            k = pre_k if pre_k is not None else self._slot_stage()
            self._graphs[k].replay()
            self._slot_release(k, ensure)
        elif self._graph is not None:
            self._flush()  # this step's host values: one copy / launch on the step's stream, ahead of the replay
            self._graph.replay()
        elif self._pack is not None and self.fuse_transform and self._table is not None:
            self._flush()
            self._run_cameras()
            self.multi.rerun(self._pack)  # (the frames' arguments have not changed: device buffers, written by the flush)
            self._run_maps()
        else:
            self._gpu_step()
            self._pack = self.multi.last_pack if self.fuse_transform and self._table is not None else None
        if ensure:
            if self._sync_fn is not None:
                self._sync_fn(self._dev_index)
            else:
                torch.cuda.current_stream(self.device).synchronize()
        self._check_overflow(late=not ensure)
        return self.frames

    # The pinned ring: slot k is read by the device during the step that staged it, and written again eight steps later.
    # An event behind EVERY step is a marker the queue stops at: ~6 us between a step's last kernel and the next step's
    # first by the kernel trace (round 6).  So only every fourth step records one, and a slot's writer waits for the first
    # event at or after the step that last read the slot -- at most three steps later, still five steps back.
    _EV_EVERY = 4

    def _slot_acquire(self) -> int:
        n = len(self._ring)
        s = self._ring_k
        self._ring_k += 1
        last_reader = s - n
        if last_reader >= 0 and self._on_gpu:
            e = last_reader + ((self._EV_EVERY - 1 - last_reader) % self._EV_EVERY)  # first recording step >= last_reader
            ev = self._ring_ev[e % n]
            if ev is not None and ev[0] == e:
                ev[1].synchronize()
            elif ev is None or ev[0] < last_reader:
                # (no marker covers the slot's last reader -- e.g. that step ended in a wait of its own: ensure=True)
                if self._ring_waited < last_reader:
                    torch.cuda.current_stream(self.device).synchronize()
                    self._ring_waited = s - 1
        return s % n

    def _slot_release(self, k: int, waited: bool):
        s = self._ring_k - 1
        if waited:
            self._ring_waited = s  # (the caller waits for this step's frames: every slot up to here is free after that)
        elif s % self._EV_EVERY == self._EV_EVERY - 1 and self._on_gpu:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
            self._ring_ev[s % len(self._ring)] = (s, ev)

    def _check_overflow(self, late: bool):
        pending = 0
        for lane in self.multi.lanes:
            if lane._mirror is not None and not lane.bounded:
                seen = lane.overflows_seen()
                if seen < lane.overflows_handled:
                    # the lane's state was reallocated (its count restarts at 0) or its mirror has not landed yet: the
                    # tally restarts with it -- a stale, larger "handled" would hide this lane's next overflows, and
                    # summed over the lanes would cancel another lane's
                    lane.overflows_handled = seen
                pending += seen - lane.overflows_handled
        if pending <= 0:
            return
        recapture = self._graph is not None or self._graphs is not None
        torch.cuda.synchronize(self.device)
        for lane in self.multi.lanes:
            if lane._mirror is not None and not lane.bounded:
                lane.overflows_handled = lane.overflows_seen()
        # frames of the CURRENT step are re-rendered below; with late=True the earlier ones had been returned already
        seen_now = sum(1 for lane in self.multi.lanes if lane.stats().overflow)
        if late:
            self.late_overflow_frames += max(pending - seen_now, 0)
        self._graph = self._graphs = None
        self._pack = None  # (capacities change below: the pack holds the old ones)
        self._flush_all()
        for lane in self.multi.lanes:
            st = lane.stats()
            if st.overflow:
                lane.r_capacity = lane._capacity_for(st.num_rendered)
        # exact-mode safety net for whatever the grown capacities still do not hold
        self._gpu_step()
        self.multi.ensure_valid(self._gpu_step)
        torch.cuda.synchronize(self.device)
        for lane in self.multi.lanes:
            if lane._mirror is not None and not lane.bounded:
                lane.overflows_handled = lane.overflows_seen()
        self.recovered_steps += 1
        if recapture:
            self.capture()

    def reset(self, matrices: torch.Tensor | None = None, scales: torch.Tensor | None = None) -> dict:
        """First frame(s): exact-mode render that sizes every lane's binning capacity, then the validity check."""
        if matrices is not None:
            self.set_poses(matrices, scales)
        self._pack = None
        self._gpu_step()
        self.multi.ensure_valid(self._gpu_step)
        self._overflows_acknowledged()
        return self.frames

    def _overflows_acknowledged(self):
        """(after a synchronising validity check: what the mirrors show from now on is news)"""
        torch.cuda.synchronize(self.device)
        for lane in self.multi.lanes:
            if lane._mirror is not None and not lane.bounded:
                lane.overflows_handled = lane.overflows_seen()

    def ensure_valid(self):
        """Overflow check of the last step (synchronises); re-renders exactly if a lane's capacity was exceeded.  A
        captured graph is dropped in that case (its capacities are baked in): call :meth:`capture` again."""
        def again():
            self._graph = self._graphs = None
            self._pack = None
            self._flush_all()
            self._gpu_step()
        return self.multi.ensure_valid(again)

    def overflow_frames(self) -> int:
        """How many frames of this loop exceeded their lane's binning capacity since the lane's state was allocated
        (such a frame shows the background only).  Counted on the device by the frames themselves, so a rollout that
        never calls :meth:`ensure_valid` between steps can still tell at its end whether every frame was valid
        (synchronises)."""
        return sum(lane.stats().overflow_frames for lane in self.multi.lanes)

    @property
    def captured(self) -> bool:
        """A step is replayed from a hipGraph (one graph, or one per ring slot with the host values staged inside)."""
        return self._graph is not None or self._graphs is not None

    def _flush_all(self):
        """(after staged graphs: the eager path stages what is dirty only -- everything the host holds is, once)"""
        self._dirty.update(n for n in self._seg_order if n not in self._stale)

    def capture(self):
        """Captures the GPU side of a step into a hipGraph (call after :meth:`reset`).

        When every per-step value comes from the host (poses and cameras handed over as host tensors: a CPU simulator, the
        rollouts of the tests and of ``bench.py``), the step's host values are staged INSIDE the graph: one graph per pinned
        ring slot, each starting with the ``gsr_stage_step`` launch that reads its slot -- :meth:`step` then writes the
        host mirror into the next slot and replays that slot's graph: nothing is enqueued between two replays (round 5: an
        H2D copy and the pack kernel; an eager launch between two graph replays costs ~14 us of idle device per step by the
        kernel trace).  Values handed over as device tensors are never staged over: such a loop captures ONE graph of the
        frames, and whatever the host still provides goes up in front of each replay."""
        dev = self.device
        self._graph = self._graphs = None
        self._ext_changed = False
        self._gpu_step()
        self.multi.ensure_valid(self._gpu_step)
        self._pack = self.multi.last_pack if self.fuse_transform and self._table is not None else None
        staged = self._table is not None and self._ring_dev is not None and not self._stale and self.fuse_transform
        n_all = int(self._stage.numel())

        def one(k):
            if k is not None:
                self._launch_stage(k, n_all)
            self._gpu_step()

        graphs = []
        for k in (range(len(self._ring)) if staged else [None]):
            if k is not None:
                self._ring[k].copy_(self._host)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                one(k)
            torch.cuda.current_stream(dev).wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                one(k)
            graphs.append(g)
        if staged:
            self._graphs = graphs
            self._dirty.clear()
        else:
            self._graph = graphs[0]
        self._overflows_acknowledged()
        return graphs[0]


class PipelinedClosedLoop:
    """``depth`` closed loops over ONE copy of the model that take the steps of a rollout in turn, each on its own HIP
    stream with its own poses, cameras, renderer states, frames and graph: step k + 1 is enqueued while step k still
    renders, so ``depth x cameras`` frames are in flight instead of ``cameras``.

    A single :class:`ClosedLoopRenderer` replays one graph per step on one stream: the two frames of a step overlap,
    consecutive steps do not, and at 640 x 480 two frames leave the chip half idle (section 4 of DESIGN.md: 9.7 k frames/s
    with two identical frames in flight against 11.9 k with four).  Whether consecutive steps MAY overlap is the caller's
    matter: a random-action or scripted rollout (BASELINE.json configs[2]: ``gsworld_rand_action_tabletop.py:107-133``
    never looks at its observations), an open-loop replay, a data-collection run with a planner, or several environments
    stepping independently can; a policy that needs frame k before it chooses action k + 1 cannot, and gains nothing
    here.

    :meth:`step` returns the frames of the step it enqueued -- tensors owned by that step's loop, overwritten ``depth``
    steps later.  With ``wait=True`` (default) the CURRENT stream is made to wait for them, so whatever the caller
    enqueues next may read them; poses handed over as DEVICE tensors are read after what the current stream has already
    enqueued (a GPU simulator).  Both are stream dependencies, never host synchronisations; but a current stream that
    waits for step k and then produces the poses of step k + 1 chains the steps together again -- hand host (pinned)
    poses over, or ``wait=False`` and :meth:`wait_for` before reading, to keep them apart.

    Reading a step's frames: enqueue the reads (or a clone) on the stream that waited for them BEFORE the next call of
    :meth:`step`.  That call marks the consumer stream, and the step that reuses the loop -- ``depth`` calls later, on
    another stream -- waits for the mark before it overwrites the frames (write-after-read across streams: the step's
    own stream knows nothing of the caller's reads).  The mark is taken before the consumer stream is made to wait for
    the NEW step, so it orders against the reads only and consecutive steps still overlap."""

    def __init__(self, raw, part_labels: dict, cameras: dict, depth: int = 2, **kw):
        if depth < 1:
            raise ValueError("depth must be >= 1")
        if kw.get("maps"):
            raise ValueError("PipelinedClosedLoop does not render segmentation / depth maps: use ClosedLoopRenderer(maps=...)")
        if kw.get("pointcloud") is not None:
            raise ValueError("PipelinedClosedLoop does not make point clouds: use ClosedLoopRenderer(pointcloud=...)")
        if kw.get("appearance") is not None:
            raise ValueError("PipelinedClosedLoop does not randomize appearance: use ClosedLoopRenderer(appearance=...)")
        first = ClosedLoopRenderer(raw, part_labels, cameras, **kw)
        self.loops = [first] + [ClosedLoopRenderer(raw, part_labels, cameras, share_model_of=first, **kw)
                                for _ in range(depth - 1)]
        self.device = first.device
        self.streams = [torch.cuda.Stream(self.device) for _ in self.loops]
        self._events = [None] * depth
        self._released = [None] * depth   # per loop: event on its consumer stream, recorded behind the reads of its frames
        self._consumer = [None] * depth   # per loop: the stream that was made to wait for its last step (None: nobody yet)
        self._k = 0

    @property
    def depth(self) -> int:
        return len(self.loops)

    def reset(self, matrices=None, scales=None) -> dict:
        """Sizes every loop's lanes on the reset poses; returns the first loop's frames."""
        cur = torch.cuda.current_stream(self.device)
        out = None
        for loop, st in zip(self.loops, self.streams):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                f = loop.reset(matrices, scales)
            out = out if out is not None else f
        torch.cuda.synchronize(self.device)
        self._k = 0
        self._released = [None] * len(self.loops)
        self._consumer = [None] * len(self.loops)
        return out

    def capture(self):
        for loop, st in zip(self.loops, self.streams):
            with torch.cuda.stream(st):
                loop.capture()
        torch.cuda.synchronize(self.device)

    def step(self, matrices=None, scales=None, cameras: dict | None = None, wait: bool = True, ensure: bool = False,
             extrinsics: dict | None = None) -> dict:
        """(``per_env_cameras`` / ``sim2real`` go to every loop; ``cameras`` / ``extrinsics`` as
        :meth:`ClosedLoopRenderer.step`)"""
        i = self._k % len(self.loops)
        self._k += 1
        loop, st = self.loops[i], self.streams[i]
        cur = torch.cuda.current_stream(self.device)
        for j, consumer in enumerate(self._consumer):
            if consumer is not None:
                # whatever the caller has enqueued behind those frames on the stream that was made to wait for them
                rel = torch.cuda.Event()
                rel.record(consumer)
                self._released[j] = rel
                self._consumer[j] = None
        if self._released[i] is not None:  # this loop's frames were handed out `depth` steps ago: their readers first
            st.wait_event(self._released[i])
            self._released[i] = None
        on_device = any(isinstance(t, torch.Tensor) and t.is_cuda for t in (matrices, scales)) or \
            any(c.world_view_transform.is_cuda for v in (cameras or {}).values()
                for c in (v if isinstance(v, (list, tuple)) else [v])) or \
            any(isinstance(t, torch.Tensor) and t.is_cuda for t in (extrinsics or {}).values())
        if on_device:
            st.wait_stream(cur)  # the poses were produced by what the current stream holds
        with torch.cuda.stream(st):
            frames = loop.step(matrices, scales, cameras, ensure=ensure, extrinsics=extrinsics)
            ev = torch.cuda.Event()
            ev.record(st)
        self._events[i] = ev
        if wait:
            cur.wait_event(ev)
            self._consumer[i] = cur
        return frames

    def wait_for(self, frames: dict | None = None, stream=None):
        """Makes ``stream`` (default: current) wait for the step that produced ``frames`` (default: every step enqueued so
        far)."""
        stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        for i, (loop, ev) in enumerate(zip(self.loops, self._events)):
            if ev is not None and (frames is None or frames is loop.frames):
                stream.wait_event(ev)
                self._consumer[i] = stream

    def overflow_frames(self) -> int:
        return sum(loop.overflow_frames() for loop in self.loops)

    def ensure_valid(self):
        return [s for loop in self.loops for s in loop.ensure_valid()]


def part_poses_from_sim(sim2gs_arm: torch.Tensor, link_now: torch.Tensor, link_scan: torch.Tensor, link_offset=None,
                         actor_now: torch.Tensor | None = None, sim2gs_obj: torch.Tensor | None = None,
                         actor_offset: torch.Tensor | None = None, actor_scale: torch.Tensor | None = None):
    """The per-part matrices of one simulation step, from what a ManiSkill env exposes -- the host-side arithmetic of
    ``GSWorldWrapper.transform_gs_perlink`` (gs_world_wrapper.py:114-120, 139-156) in its float32 operation order, so a
    caller holding the simulator state gets exactly the ``rot_mat`` / ``translation`` / ``scale`` the reference hands
    to ``transform_gaussians`` (pinned by tests/golden/wrapper_glue.npz, which records those arguments from the
    reference's own run).

    ``link_now`` (E,L,4,4): ``link.pose.to_transformation_matrix()`` of every robot link; ``link_scan`` (L,4,4): the same
    at the qpos the robot was scanned in (``gs_link_pose_mats``, ``__init__`` :94-103); ``link_offset`` (3,): the
    ``object_offset["xarm_arm"]`` shift added to every link position for xarm robots (:117-119) or None;
    ``actor_now`` (E,A,4,4): tracked actor poses; ``sim2gs_obj`` (A,4,4): their ``sim2gs_object_transforms``;
    ``actor_offset`` (A,3) and ``actor_scale`` (A,): ``object_offset`` / ``object_scale`` of each (zeros / ones when an
    actor has no entry).  -> ``(matrices (E,L+A,4,4), scales (E,L+A))`` in link-then-actor order, the layout
    :class:`ClosedLoopRenderer` takes (links carry scale 1 and are not rescaled)."""
    from .camera import extract_rigid_transform

    f32 = torch.float32
    dev = link_now.device  # (a GPU simulator hands over device tensors: everything is computed where the poses live)
    on = lambda t: torch.as_tensor(t, dtype=f32, device=dev)  # noqa: E731
    sim2gs_arm = on(sim2gs_arm)
    inv_arm = torch.linalg.inv(sim2gs_arm)
    link_mat = link_now.to(f32).clone()
    link_scan = on(link_scan)
    E, L = link_mat.shape[:2]
    if link_offset is not None:
        link_mat[:, :, :3, 3] += on(link_offset)
    mats, scales = [], []
    for k in range(L):  # (:120) sim2gs @ link_now @ inv(link_scan) @ inv(sim2gs), left to right
        mats.append(sim2gs_arm @ link_mat[:, k] @ torch.linalg.inv(link_scan[k]) @ inv_arm)
        scales.append(torch.ones(E, dtype=f32, device=dev))
    if actor_now is not None:
        A = actor_now.shape[1]
        sim2gs_obj = on(sim2gs_obj)
        for a in range(A):
            mat = on(actor_now[:, a]).clone()
            if actor_offset is not None:
                mat[:, :3, 3] += on(actor_offset[a])
            full = sim2gs_arm @ mat @ torch.linalg.inv(sim2gs_obj[a])  # (:147)
            rigid, scale, _, _ = extract_rigid_transform(full)          # (:150)
            mats.append(rigid)
            scales.append(on(scale) * (1.0 if actor_scale is None else on(actor_scale[a])))
    return torch.stack(mats, 1).contiguous(), torch.stack(scales, 1).to(f32).contiguous()


_ROLLOUT_NAMES = ("small_rigid", "random_walk_poses", "xarm6_rollout", "rollout_poses", "xarm6_rollout_parts", "xarm6_parts")


def __getattr__(name):
    """The synthetic rollouts (stand-ins for the simulator) live in :mod:`gsworld_amd.rollouts`; their old names here
    keep resolving."""
    if name in _ROLLOUT_NAMES:
        from . import rollouts

        return getattr(rollouts, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
