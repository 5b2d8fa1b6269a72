"""Point-cloud observations of the splatted scene (include/gsr.h ``gsr_render_pointcloud``, csrc/pointcloud.hip).

ManiSkill's ``obs_mode="pointcloud"`` concatenates, per environment, the points of every camera's pixels (camera by
camera, row-major by pixel) in the world frame, with their colour and segmentation.  Point-cloud policies (PointNet,
DP3-style diffusion policies) then take a fixed-size cloud: cropped to the workspace, with the table / background labels
removed, usually farthest-point sampled.  Here all of that is one capturable sequence of at most four launches per step
over every environment, from the depth / label maps of ``gsr_render_maps``, the uint8 frames and the cameras' device-
resident view matrices -- no host round trip, no variable-size tensor.

* :class:`PointCloudSpec` -- what cloud to make (dense, stride- or FPS-sampled, crop, excluded labels, output frame).
* :func:`sim_from_scene` -- the affine that takes the splatted scene's frame to GSWorld's simulator frame in metres.
* :func:`render_pointcloud` -- the functional form over plain tensors; :class:`gsworld_amd.closed_loop.ClosedLoopRenderer`
  (``pointcloud=PointCloudSpec(...)``) runs it behind every step into ``loop.pointcloud``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _C, _lib

SAMPLES = ("fps", "stride")


@dataclass
class PointCloudSpec:
    """``num_points``: None -- the dense cloud, one slot per pixel of every camera (ManiSkill's own shape, w = 0 where a
    pixel holds no valid point); else K slots (1 .. 8192) chosen by ``sample``: ``"fps"`` (farthest-point sampling from the
    first of ``fps_candidates`` evenly strided valid points, up to 16384) or ``"stride"`` (evenly strided valid points).
    ``crop``: None or ``(lo, hi)``, each three floats, an inclusive box in the OUTPUT frame.  ``exclude_labels``: semantic
    labels (int16) whose points are dropped (table, background).  ``out_from_scene``: None (identity) or a 3 x 4 / 4 x 4
    affine applied to every scene point (:func:`sim_from_scene` for GSWorld's simulator frame)."""
    num_points: int | None = None
    sample: str = "fps"
    crop: tuple | None = None
    exclude_labels: tuple = ()
    out_from_scene: object = None
    fps_candidates: int = 8192

    @property
    def mode(self) -> int:
        if self.num_points is None:
            return _lib.PC_DENSE
        return _lib.PC_FPS if self.sample == "fps" else _lib.PC_STRIDE

    def validated(self) -> "PointCloudSpec":
        """Checks every field (``ValueError``) -> self."""
        if self.num_points is not None:
            if isinstance(self.num_points, bool) or int(self.num_points) != self.num_points or \
                    not 1 <= int(self.num_points) <= _lib.PC_MAX_K:
                raise ValueError(f"num_points must be None (dense) or an integer in [1, {_lib.PC_MAX_K}]")
            if self.sample not in SAMPLES:
                raise ValueError(f"sample must be one of {SAMPLES}, got {self.sample!r}")
            if self.sample == "fps" and (isinstance(self.fps_candidates, bool) or
                                         int(self.fps_candidates) != self.fps_candidates or
                                         not 1 <= int(self.fps_candidates) <= _lib.PC_MAX_FPS_CANDIDATES):
                raise ValueError(f"fps_candidates must be an integer in [1, {_lib.PC_MAX_FPS_CANDIDATES}]")
        if self.crop is not None:
            lo, hi = (np.asarray(x, dtype=np.float64) for x in self.crop) if len(self.crop) == 2 else (None, None)
            if lo is None or lo.shape != (3,) or hi.shape != (3,) or not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
                raise ValueError("crop must be None or (lo, hi) with three finite floats each")
        for lab in self.exclude_labels:
            if isinstance(lab, bool) or int(lab) != lab or not -32768 <= int(lab) <= 32767:
                raise ValueError(f"exclude_labels must be integers in the int16 range, got {lab!r}")
        self.affine()
        return self

    def affine(self) -> list:
        """``out_from_scene`` as the 12 floats (row-major 3 x 4) the library takes."""
        if self.out_from_scene is None:
            return [1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0]
        A = self.out_from_scene
        A = A.detach().cpu().numpy() if isinstance(A, torch.Tensor) else np.asarray(A)
        A = A.astype(np.float64)
        if A.shape not in ((3, 4), (4, 4)) or not np.all(np.isfinite(A[:3])):
            raise ValueError("out_from_scene must be a finite 3 x 4 or 4 x 4 affine")
        return [float(x) for x in A[:3].reshape(-1)]

    def exclusion_bitmap(self) -> np.ndarray | None:
        """The 65536-bit exclusion set over (uint16)label as 2048 little-endian 32-bit words (None: no set)."""
        if not len(self.exclude_labels):
            return None
        bits = np.zeros(2048, np.uint32)
        for lab in self.exclude_labels:
            u = int(lab) & 0xFFFF
            bits[u >> 5] |= np.uint32(1 << (u & 31))
        return bits


def sim_from_scene(rigid_sim2real, scale_sim2real) -> np.ndarray:
    """The 3 x 4 affine (float64) from the splatted scene's frame to GSWorld's simulator frame, in metres:
    ``diag(1/s) . rigid_sim2real^-1``.  ``cam_maniskill2gs`` (gs_world_wrapper.py:297-301; :func:`gsworld_amd.camera.
    cam_maniskill2gs`) places a simulator camera in the scene by scaling its translation by ``s = scale_sim2real`` and
    left-multiplying by ``rigid_sim2real``, so a simulator point x appears at ``rigid_sim2real (s x)``; this undoes that."""
    R = rigid_sim2real.detach().cpu().numpy() if isinstance(rigid_sim2real, torch.Tensor) else np.asarray(rigid_sim2real)
    R = R.astype(np.float64)
    if R.shape == (3, 4):
        R = np.vstack([R, [0.0, 0.0, 0.0, 1.0]])
    if R.shape != (4, 4):
        raise ValueError("rigid_sim2real must be 4 x 4 (or 3 x 4)")
    s = float(scale_sim2real)
    if not np.isfinite(s) or s == 0.0:
        raise ValueError("scale_sim2real must be finite and non-zero")
    return np.linalg.inv(R)[:3] / s


def _per_camera(x, names, what):
    if x is None:
        return [None] * len(names)
    if isinstance(x, dict):
        missing = [n for n in names if n not in x]
        if missing:
            raise ValueError(f"{what}: no entry for camera(s) {missing}")
        return [x[n] for n in names]
    x = list(x)
    if len(x) != len(names):
        raise ValueError(f"{what}: one entry per camera ({len(names)}) expected")
    return x


def _check(t, dtype, shape, dev, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.device != dev or not t.is_contiguous() or \
            t.numel() != int(np.prod(shape)) or t.shape[0] != shape[0]:
        raise ValueError(f"{what} must be a dense {dtype} tensor of shape {shape} on {dev}")


def prepare(depth, labels, frames, cameras, spec: PointCloudSpec, depth_scale: float = 1.0, out=None, device=None,
            binding: str = "auto"):
    """Everything one ``gsr_render_pointcloud`` call needs, checked and packed once: -> (pack, out, keep) with ``out`` the
    output dict (see :func:`render_pointcloud`) and ``keep`` the tensors the pack points to besides the caller's.  A caller
    that runs the same call step after step (the closed loop) keeps the triple and calls
    ``_C.run_pointcloud(pack, device)``; the view matrices are read at run time, so a camera that moves between runs is
    seen where its matrix now says it is."""
    spec = spec.validated()
    if isinstance(cameras, dict):
        names, cams = list(cameras), list(cameras.values())
    else:
        cams = list(cameras)
        names = list(range(len(cams)))
    if not cams:
        raise ValueError("at least one camera")
    # (a camera may be a list: environment e's own camera at [e], one image size -- ClosedLoopRenderer(per_env_cameras=True))
    env_cams = [list(c) if isinstance(c, (list, tuple)) else None for c in cams]
    cams = [ec[0] if ec else c for c, ec in zip(cams, env_cams)]
    deps = _per_camera(depth, names, "depth")
    labs = _per_camera(labels, names, "labels")
    rgbs = _per_camera(frames, names, "frames")
    dev = torch.device(device) if device is not None else deps[0].device
    if dev.type != "cuda":
        raise ValueError("render_pointcloud runs on the GPU: depth maps must be device tensors")
    E = int(deps[0].shape[0])
    Cn = len(cams)
    if E * Cn > _lib.PC_MAX_VIEWS:
        raise ValueError(f"at most {_lib.PC_MAX_VIEWS} (environment, camera) views per call, got {E} x {Cn}")
    if spec.exclude_labels and any(l is None for l in labs):
        raise ValueError("exclude_labels needs every camera's label map")
    keep, vms = [], []
    for cam, ec, d, l, r in zip(cams, env_cams, deps, labs, rgbs):
        H, W = int(cam.image_height), int(cam.image_width)
        _check(d, torch.float32, (E, H, W), dev, "depth")
        if l is not None:
            _check(l, torch.int16, (E, H, W), dev, "labels")
        if r is not None:
            _check(r, torch.uint8, (E, H, W, 3), dev, "frames")
        if ec is not None and (len(ec) != E or any((int(c.image_width), int(c.image_height)) != (W, H) for c in ec)):
            raise ValueError(f"a per-environment camera list needs {E} cameras of one image size")
        per = []
        for c in (ec if ec is not None else [cam] * E):
            vm = c.world_view_transform
            if vm.device != dev or vm.dtype != torch.float32 or not vm.is_contiguous():
                vm = vm.detach().to(dev, torch.float32).contiguous()
                keep.append(vm)
            per.append((vm, c.tanfovx, c.tanfovy))
        vms.append(per)
    N = sum(int(c.image_width) * int(c.image_height) for c in cams)
    S = N if spec.mode == _lib.PC_DENSE else int(spec.num_points)
    if out is None:
        out = {"xyzw": torch.empty((E, S, 4), dtype=torch.float32, device=dev),
               "rgb": torch.empty((E, S, 3), dtype=torch.uint8, device=dev),
               "segmentation": torch.empty((E, S, 1), dtype=torch.int16, device=dev),
               "count": torch.empty((E,), dtype=torch.int32, device=dev)}
    for k, dt, shp in (("xyzw", torch.float32, (E, S, 4)), ("rgb", torch.uint8, (E, S, 3)),
                       ("segmentation", torch.int16, (E, S, 1)), ("count", torch.int32, (E,))):
        _check(out.get(k), dt, shp, dev, f"out[{k!r}]")
    views = []
    for e in range(E):
        for c, cam in enumerate(cams):
            vm, tx, ty = vms[c][e]
            views.append(dict(width=cam.image_width, height=cam.image_height, tanfovx=tx, tanfovy=ty,
                              viewmatrix=vm, depth=deps[c][e], depth_scale=float(depth_scale),
                              label=labs[c][e] if labs[c] is not None else None,
                              rgb8=rgbs[c][e] if rgbs[c] is not None else None))
    bits = spec.exclusion_bitmap()
    exclude = torch.from_numpy(bits.view(np.int32)).to(dev) if bits is not None else None
    crop = spec.crop
    d = dict(E=E, C=Cn, views=views, out_from_scene=spec.affine(), crop=crop, exclude=exclude, mode=spec.mode,
             K=0 if spec.num_points is None else int(spec.num_points),
             fps_candidates=int(spec.fps_candidates) if spec.mode == _lib.PC_FPS else 0,
             xyzw=out["xyzw"], rgb=out["rgb"], segmentation=out["segmentation"], count=out["count"])
    ws_bytes = workspace_bytes(d)
    ws = torch.empty((max(ws_bytes, 256),), dtype=torch.uint8, device=dev)
    d["workspace"] = ws
    keep += [ws] + ([exclude] if exclude is not None else [])
    return _C.pack_pointcloud(d, binding), out, keep


def workspace_bytes(d: dict) -> int:
    """``gsr_pointcloud_workspace`` of a :func:`gsworld_amd._C.pack_pointcloud` spec dict (host only)."""
    views = (_lib.GsrCloudView * len(d["views"]))(*[_lib.GsrCloudView(int(v["width"]), int(v["height"])) for v in d["views"]])
    cs = _lib.GsrCloudSpec()
    cs.struct_size = C.sizeof(_lib.GsrCloudSpec)
    cs.E, cs.C, cs.views = int(d["E"]), int(d["C"]), views
    cs.mode, cs.K, cs.fps_candidates = int(d["mode"]), int(d["K"]), int(d["fps_candidates"])
    n = C.c_int64(0)
    _lib.check(_lib.lib().gsr_pointcloud_workspace(C.byref(cs), C.byref(n)))
    return int(n.value)


def render_pointcloud(depth, labels, frames, cameras, spec: PointCloudSpec, depth_scale: float = 1.0, out=None,
                      binding: str = "auto") -> dict:
    """The point cloud of E environments seen by C cameras, on the current stream (no synchronisation).

    ``cameras``: ``{name: ViewParams}`` (or a list) -- size, field of view and ``world_view_transform`` (read on the
    device when it lives there; copied up otherwise); a camera may also be a list of E ViewParams of one image size,
    environment e's own camera at [e].  ``depth``: per camera (E, H, W[, 1]) float32 depth maps as
    ``gsr_render_maps`` writes them (0.0 = no point), written with ``depth_scale``; ``labels``: per camera (E, H, W[, 1])
    int16 label maps, or None (segmentation -1); ``frames``: per camera (E, H, W, 3) uint8 frames, or None (rgb 0).  Per-
    camera arguments are dicts keyed like ``cameras`` or lists in its order.

    -> ``{"xyzw": (E, S, 4) float32, "rgb": (E, S, 3) uint8, "segmentation": (E, S, 1) int16, "count": (E,) int32}`` with
    S = the pixels of all cameras (dense) or ``spec.num_points``; a slot without a point holds xyzw = 0, rgb = 0,
    segmentation = -1.  ``out``: such a dict to write into.  The definition, arithmetic order included, is
    csrc/pointcloud.hip's header comment."""
    # (the temporaries in `keep` go back to the caching allocator on this stream: stream-ordered, nothing waits)
    pack, out, keep = prepare(depth, labels, frames, cameras, spec, depth_scale, out, binding=binding)
    _C.run_pointcloud(pack, out["xyzw"].device)
    return out
