"""``_C`` of the drop-in ``diff_gaussian_rasterization`` package: the three functions the upstream pybind
module exports (rasterize_points.h / ext.cpp), same positional signatures, same return
tuples, same error strings -- implemented over the C ABI of libgsr_hip.so (include/gsr.h).

Caller: ``_RasterizeGaussians`` in :mod:`gsworld_amd.rasterizer`, which GSWorld reaches through
``gaussian_renderer.render`` (/root/reference/gsworld/mani_skill/utils/wrappers/gs_world_wrapper.py:266-267).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import (GsrBuffers, GsrFrameStats, GsrInputs, GsrOutputs, GsrSettings, RESIZE_FN, check, lib)

# The compiled binding (csrc_torch/ext.cpp, built by gsworld_amd/build_ext.py): the `_C` pybind module upstream's
# python package imports.  Used whenever it has been built; the ctypes path below drives the SAME shared library and
# remains for environments without the torch headers (GSWORLD_AMD_CTYPES=1 forces it, e.g. to A/B the host overhead).
import os as _os

_ext = None
if _os.environ.get("GSWORLD_AMD_CTYPES", "") != "1":
    try:
        from . import _C_ext as _ext  # noqa: F401
    except ImportError:
        _ext = None


def _tuning_list(forward_only=None):
    """The A/B selectors of this call.  ``forward_only`` None: a frame whose state a backward will read (the
    ``rasterize_gaussians*`` paths) -- a forced ``TUNING["forward_only"]`` (GSWORLD_AMD_TUNING, an A/B aid for the frame
    renderers) must never turn such a frame into an inference frame: gsr_backward would carve the full state layout
    over a lean buffer."""
    t = _lib.TUNING
    if forward_only is None:
        fo = 0
    else:
        fo = int(t["forward_only"]) if int(t["forward_only"]) >= 0 else int(forward_only)
    return [int(t["binning_path"]), int(t["render_variant"]), int(t["render_blocks_per_cu"]), int(t["depth_sort"]),
            int(t["render_split"]), fo]


# GSWorld's edit of cuda_rasterizer/auxiliary.h (/root/reference/README.md:33).  Module-level so that a stock
# 3DGS caller can restore 0.2 without touching the ABI.
NEAR_PLANE = _lib.GSR_NEAR_PLANE


def _ptr(t: torch.Tensor | None):
    if t is None or t.numel() == 0:
        return None
    return C.c_void_p(t.data_ptr())


def _f32(t: torch.Tensor, device, what: str) -> torch.Tensor:
    if t.numel() == 0:
        return t
    if t.dtype != torch.float32:
        raise RuntimeError(f"{what} must be float32")
    if t.device != device:
        t = t.to(device)
    return t.contiguous()


def _resizer(t: torch.Tensor, header: bool = False):
    """``header``: the geometry state -- storage the allocator hands out may be a freed state of another renderer, whose
    frame header still says how many of ITS frames overflowed: on new storage the count (the header's last two words)
    is zeroed, enqueued on the frame's stream ahead of the frame's first kernel.  The rest of a recycled header is left
    alone on purpose: kept splitters / cuts are tied to model size and layout and checked before use (depthsort.hip),
    and a training loop, which gets the block it freed a step ago back every step, keeps its splitters that way."""
    def fn(_user, nbytes):
        before = t.data_ptr() if t.numel() else 0
        t.resize_(int(nbytes))
        if header and t.data_ptr() != before and nbytes >= 256:
            t[248:256].zero_()
        return t.data_ptr()

    return RESIZE_FN(fn)


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on {t.device}: the MI355X rasterizer has no CPU path (tensors must live on a HIP device)")


def appearance_args(appearance, P: int, device):
    """An ``appearance`` argument -- ``(table (G,3,4) | (G,12), lut (L,) int, labels (P,) | None[, versions (G+1,) | None])`` --
    as the tensors the library reads (GsrInputs.appearance*): float32 / int32, dense, on ``device``; labels None = the part
    labels.  ``ValueError`` for anything else (checked before any device work)."""
    if not isinstance(appearance, (tuple, list)) or len(appearance) not in (3, 4):
        raise ValueError("appearance must be (table (G,3,4), lut (L,) int32, labels (P,) | None[, versions (G+1,) | None])")
    table, lut, labels = appearance[:3]
    versions = appearance[3] if len(appearance) == 4 else None
    as_t = lambda x, dt: (x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))).to(device, dt)  # noqa: E731
    table = as_t(table, torch.float32)
    if table.dim() not in (2, 3) or table.shape[-1] != (4 if table.dim() == 3 else 12) or \
            (table.dim() == 3 and table.shape[1] != 3):
        raise ValueError(f"appearance table must be (G,3,4) or (G,12), got {tuple(table.shape)}")
    G = int(table.shape[0])
    if not 1 <= G <= _lib.APPEARANCE_MAX_GROUPS:
        raise ValueError(f"appearance: 1 <= G <= {_lib.APPEARANCE_MAX_GROUPS} groups, got {G}")
    lut = as_t(lut, torch.int32).reshape(-1).contiguous()
    if lut.numel() < 1:
        raise ValueError("appearance LUT must have at least one entry")
    if labels is not None:
        labels = as_t(labels, torch.float32).reshape(-1).contiguous()
        if labels.numel() != P:
            raise ValueError(f"appearance labels must be ({P},), got {labels.numel()} values")
    if versions is not None:
        versions = as_t(versions, torch.int32).reshape(-1).contiguous()
        if versions.numel() != G + 1:
            raise ValueError(f"appearance versions must be (G + 1,) = ({G + 1},), got {versions.numel()} values")
    return table.reshape(G, 12).contiguous(), lut, labels, versions


def _app_tensors(appearance, e, ei):
    """(table, lut, labels, versions) for the compiled binding: the empty tensors e (float32) / ei (int32) stand for NULL."""
    if appearance is None:
        return e, ei, e, ei
    t, lut, lab, ver = appearance
    return t, lut, lab if lab is not None else e, ver if ver is not None else ei


def forward_raw(settings: GsrSettings, background, means3D, colors, opacity, scales, rotations, cov3D_precomp,
                viewmatrix, projmatrix, sh, campos, out_color, out_invdepth, radii, geomBuffer, binningBuffer,
                imgBuffer, r_capacity: int = 0, want_stats: bool = True, sh_rest=None, param_space: int = 0,
                rgb8_out=None, parts=None, forward_only: bool | None = False, layout=None, overflow_mirror: int = 0,
                appearance=None):
    """Thin call into gsr_forward with caller-owned output and state tensors (no allocation here).
    ``overflow_mirror``: GsrOutputs.overflow_mirror as an address (0 = not wanted).
    ``sh_rest``: optional features_rest (P,M-1,3); ``sh`` is then features_dc (P,1,3) -- no per-frame concatenation.
    ``param_space``: OR of ``_lib.RAW_*`` -- opacity logits / log scales / un-normalised rotations are activated
    inside preprocess instead of by three torch passes.
    ``parts``: optional ``(labels (P,) float32, lut (L,) int32, table (K,17) float32, rescale (K,) uint8 | None)`` -- the
    per-frame rigid transform of labelled Gaussians applied inside preprocess (GsrInputs.part_*).
    ``forward_only``: GsrSettings.forward_only (inference frame; ``radii`` may then be None); None = a training frame
    (never an inference frame, whatever ``TUNING["forward_only"]`` forces for A/B runs).
    ``layout``: optional ``(cull_blocks (ceil(P/256),8) float32, orig_index (P,) int32 | None)`` -- block bounds for
    view-frustum culling and the original numbering of a permuted model (GsrInputs.cull_blocks / orig_index;
    :mod:`gsworld_amd.layout` builds them).
    ``appearance``: optional ``(table (G,12) float32, lut (L,) int32, labels (P,) float32 | None, versions (G+1,) int32 |
    None)`` as :func:`appearance_args` returns it -- per-group colour affines inside preprocess (GsrInputs.appearance*)."""
    dev = means3D.device
    if _ext is not None:
        st = settings
        e = torch.empty(0, device=dev)
        ei = torch.empty(0, dtype=torch.int32, device=dev)
        nv, nr, ov = _ext.forward_frame(
            st.image_height, st.image_width, st.tanfovx, st.tanfovy, st.scale_modifier, st.sh_degree, st.sh_coeffs,
            bool(st.antialiasing), bool(st.debug), st.near_plane, background, means3D,
            colors if colors is not None else e, opacity, scales if scales is not None else e,
            rotations if rotations is not None else e, cov3D_precomp if cov3D_precomp is not None else e, viewmatrix,
            projmatrix, sh if sh is not None else e, sh_rest if sh_rest is not None else e, campos, out_color,
            out_invdepth, radii if radii is not None else torch.empty(0, dtype=torch.int32, device=dev), geomBuffer,
            binningBuffer, imgBuffer,
            rgb8_out if rgb8_out is not None else torch.empty(0, dtype=torch.uint8, device=dev), int(r_capacity),
            bool(want_stats), int(param_space), _tuning_list(forward_only),
            parts[0] if parts is not None else e, parts[1] if parts is not None else ei,
            parts[2] if parts is not None else e,
            parts[3] if (parts is not None and parts[3] is not None) else torch.empty(0, dtype=torch.uint8, device=dev),
            layout[0] if layout is not None else e,
            layout[1] if (layout is not None and layout[1] is not None) else ei,
            int(overflow_mirror or 0), *_app_tensors(appearance, e, ei))
        stats = GsrFrameStats()
        stats.num_visible, stats.num_rendered, stats.overflow = nv, nr, ov
        return stats
    settings, inp, out, buf, _keep = _frame_structs(
        settings, background, means3D, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix, sh,
        campos, out_color, out_invdepth, radii, geomBuffer, binningBuffer, imgBuffer, sh_rest=sh_rest,
        param_space=param_space, rgb8_out=rgb8_out, parts=parts, forward_only=forward_only, layout=layout,
        overflow_mirror=overflow_mirror, appearance=appearance)
    stats = GsrFrameStats()
    with torch.cuda.device(dev):
        check(lib().gsr_forward(C.byref(settings), C.byref(inp), C.byref(out), C.byref(buf), C.c_int64(r_capacity),
                                C.byref(stats) if want_stats else None, _stream(dev)))
    return stats


def _frame_structs(settings: GsrSettings, background, means3D, colors, opacity, scales, rotations, cov3D_precomp,
                   viewmatrix, projmatrix, sh, campos, out_color, out_invdepth, radii, geomBuffer, binningBuffer,
                   imgBuffer, sh_rest=None, param_space: int = 0, rgb8_out=None, parts=None,
                   forward_only: bool | None = False, layout=None, overflow_mirror: int = 0, appearance=None):
    """The four argument structs of one frame (include/gsr.h) from tensors; the fifth value keeps the resize callbacks
    alive while the structs are in use."""
    settings.forward_only = int(bool(forward_only))
    _lib.apply_tuning(settings, allow_forward_only=forward_only is not None)
    inp = GsrInputs(
        P=means3D.size(0), background=_ptr(background), means3D=_ptr(means3D), shs=_ptr(sh),
        colors_precomp=_ptr(colors), opacities=_ptr(opacity), scales=_ptr(scales), rotations=_ptr(rotations),
        cov3D_precomp=_ptr(cov3D_precomp), viewmatrix=_ptr(viewmatrix), projmatrix=_ptr(projmatrix),
        campos=_ptr(campos), shs_rest=_ptr(sh_rest) if sh_rest is not None else None, param_space=int(param_space))
    if parts is not None:
        labels, lut, table, rescale = parts
        inp.part_labels, inp.part_lut, inp.part_lut_size = _ptr(labels), _ptr(lut), int(lut.numel())
        inp.part_transforms, inp.part_count = _ptr(table), int(table.shape[0])
        inp.part_rescale = _ptr(rescale) if rescale is not None else None
    if layout is not None:
        blocks, orig = layout
        if blocks.numel() != 8 * ((means3D.size(0) + 255) // 256) or blocks.dtype != torch.float32:
            raise ValueError("layout: cull_blocks must be a float32 tensor of shape (ceil(P / 256), 8)")
        if orig is not None and (orig.numel() != means3D.size(0) or orig.dtype != torch.int32):
            raise ValueError("layout: orig_index must be an int32 tensor of shape (P,)")
        inp.cull_blocks = _ptr(blocks)
        inp.orig_index = _ptr(orig) if orig is not None else None
    if appearance is not None:
        table, lut, labels, versions = appearance
        inp.appearance, inp.appearance_lut, inp.appearance_lut_size = _ptr(table), _ptr(lut), int(lut.numel())
        inp.appearance_groups = int(table.shape[0])
        inp.appearance_versions = _ptr(versions) if versions is not None else None
        inp.appearance_labels = _ptr(labels) if labels is not None else None
    out = GsrOutputs(_ptr(out_color), _ptr(out_invdepth), _ptr(radii),
                     _ptr(rgb8_out) if rgb8_out is not None else None, int(overflow_mirror) if overflow_mirror else None)
    cbs = (_resizer(geomBuffer, header=True), _resizer(binningBuffer), _resizer(imgBuffer))
    buf = GsrBuffers(cbs[0], None, cbs[1], None, cbs[2], None)
    return settings, inp, out, buf, cbs


MAX_FRAMES_PER_LAUNCH = 8  # include/gsr.h GSR_MAX_FRAMES_PER_LAUNCH


def forward_batch_raw(frames, device=None):
    """B frames of one step through gsr_forward_batch: one set of launches whose grids span the frames (include/gsr.h;
    GSWorld's per-step double loop over cameras and environments, gs_world_wrapper.py:238-267).  ``frames``: a list of
    dicts with the keyword arguments of :func:`forward_raw` (``settings`` ... ``imgBuffer``, ``r_capacity`` > 0 for the
    frames that are to share launches, no ``want_stats``: nothing is read back).  Enqueued on the current stream of the
    frames' device; returns nothing -- ``gsr_frame_stats`` on a frame's geometry state tells V / R / overflow."""
    if not frames:
        return
    dev = frames[0]["means3D"].device if device is None else device
    run_packed_batch(pack_batch(frames), dev)


def pack_batch(frames):
    """The argument pack of :func:`forward_batch_raw` for these frames, built once: a caller that renders the SAME frames
    again and again -- same tensors, same settings, same state buffers: a closed loop whose per-step values live in device
    buffers the kernels read -- keeps it and calls :func:`run_packed_batch` per step (the per-frame Python that builds it
    costs more host time than the step's eleven launches).  With the compiled binding the pack is a ``StepPack``: the argument
    structs are filled ONCE, so every tensor but the three state buffers (which the resize callbacks follow) must keep its
    storage for as long as the pack is used -- build a new pack after replacing or resizing any of them."""
    B = len(frames)
    dev = frames[0]["means3D"].device
    if _ext is not None and hasattr(_ext, "forward_batch"):
        e = torch.empty(0, device=dev)
        ei = torch.empty(0, dtype=torch.int32, device=dev)
        eb = torch.empty(0, dtype=torch.uint8, device=dev)
        packed = []
        for f in frames:
            st, parts, layout = f["settings"], f.get("parts"), f.get("layout")
            o = lambda k, d=e: f.get(k) if f.get(k) is not None else d  # noqa: E731
            packed.append((
                st.image_height, st.image_width, st.tanfovx, st.tanfovy, st.scale_modifier, st.sh_degree, st.sh_coeffs,
                bool(st.antialiasing), bool(st.debug), st.near_plane, f["background"], f["means3D"], o("colors"),
                f["opacity"], o("scales"), o("rotations"), o("cov3D_precomp"), f["viewmatrix"], f["projmatrix"],
                o("sh"), o("sh_rest"), f["campos"], f["out_color"], f["out_invdepth"], o("radii", ei), f["geomBuffer"],
                f["binningBuffer"], f["imgBuffer"], o("rgb8_out", eb), int(f.get("r_capacity", 0)),
                int(f.get("param_space", 0)), _tuning_list(f.get("forward_only", False)),
                parts[0] if parts is not None else e, parts[1] if parts is not None else ei,
                parts[2] if parts is not None else e,
                parts[3] if (parts is not None and parts[3] is not None) else eb,
                layout[0] if layout is not None else e,
                layout[1] if (layout is not None and layout[1] is not None) else ei,
                int(f.get("overflow_mirror") or 0), *_app_tensors(f.get("appearance"), e, ei)))
        if hasattr(_ext, "StepPack"):
            return ("pack", _ext.StepPack(packed))  # (the argument structs filled once, kept on the C++ side)
        return ("ext", packed)
    built, caps = [], (C.c_int64 * B)()
    for k, f in enumerate(frames):
        f = dict(f)
        caps[k] = int(f.pop("r_capacity", 0))
        f.pop("want_stats", None)
        built.append(_frame_structs(**f))
    St = (GsrSettings * B)(*[b[0] for b in built])
    In = (GsrInputs * B)(*[b[1] for b in built])
    Out = (GsrOutputs * B)(*[b[2] for b in built])
    Buf = (GsrBuffers * B)(*[b[3] for b in built])
    return ("ctypes", (B, St, In, Out, Buf, caps, built, frames))  # (built / frames: keep callbacks and tensors alive)


def run_packed_batch(pack, device):
    """Enqueues the frames of :func:`pack_batch` on the current stream of ``device``."""
    kind, p = pack
    if kind == "pack":
        p.run()
        return
    if kind == "ext":
        _ext.forward_batch(p)
        return
    B, St, In, Out, Buf, caps = p[:6]
    with torch.cuda.device(device):
        check(lib().gsr_forward_batch(B, St, In, Out, Buf, caps, _stream(device)))


def pack_maps(frames, binding: str = "auto"):
    """The arguments of one ``gsr_render_maps`` call (include/gsr.h) for these frames, built once: a loop that asks for the
    maps of the same lanes step after step keeps the pack while no state buffer moves.  ``frames``: dicts with ``settings``
    (the frame's GsrSettings), ``P``, ``permuted``, ``r_capacity``, ``geom`` / ``binning`` / ``image`` (state tensors),
    ``labels`` ((P,) float32 or None), ``depth_scale``, ``out_label`` ((H,W) int16 or None), ``out_depth`` ((H,W) float32 or
    None).  ``binding``: "auto" (the compiled one when built), "ext" or "ctypes" -- the same library call either way."""
    def ptr(t):
        return int(t.data_ptr()) if t is not None and t.numel() else 0

    vals = []
    for f in frames:
        st = f["settings"]
        vals.append((tuple(getattr(st, n) for n, _ in GsrSettings._fields_), int(f["P"]), int(bool(f["permuted"])),
                     int(f["r_capacity"]), ptr(f["geom"]), ptr(f["binning"]), ptr(f["image"]), ptr(f.get("labels")),
                     float(f.get("depth_scale", 1.0)), ptr(f.get("out_label")), ptr(f.get("out_depth"))))
    use_ext = _ext is not None and hasattr(_ext, "render_maps") if binding == "auto" else binding == "ext"
    if use_ext:
        if _ext is None or not hasattr(_ext, "render_maps"):
            raise RuntimeError("the compiled binding (gsworld_amd._C_ext) with render_maps is not built")
        return ("ext", vals)
    B = len(vals)
    sts = (GsrSettings * max(B, 1))()
    arr = (_lib.GsrMapFrame * max(B, 1))()
    for k, v in enumerate(vals):
        sts[k] = GsrSettings(*v[0])
        arr[k] = _lib.GsrMapFrame(C.sizeof(_lib.GsrMapFrame), C.pointer(sts[k]), v[1], v[2], v[3], v[4] or None, v[5] or None,
                                  v[6] or None, v[7] or None, v[8], v[9] or None, v[10] or None)
    return ("ctypes", (B, arr, sts))


def run_maps(pack, device) -> None:
    """Enqueues the ``gsr_render_maps`` call of :func:`pack_maps` on the current stream of ``device`` (capturable)."""
    kind, p = pack
    dev = torch.device(device)
    if kind == "ext":
        _ext.render_maps(dev.index if dev.index is not None else torch.cuda.current_device(), p)
        return
    B, arr, _ = p
    with torch.cuda.device(dev):
        check(lib().gsr_render_maps(B, arr, _stream(dev)))


def render_maps(frames, device, binding: str = "auto") -> None:
    """Segmentation / depth maps of rendered frames from their state (``gsr_render_maps``): :func:`pack_maps` +
    :func:`run_maps`."""
    run_maps(pack_maps(frames, binding), device)


def pack_pointcloud(spec: dict, binding: str = "auto"):
    """The arguments of one ``gsr_render_pointcloud`` call (include/gsr.h), built once: a loop that asks for the clouds of
    the same buffers step after step keeps the pack while no buffer moves.  ``spec``: ``E``, ``C``, ``views`` (E*C dicts:
    ``width``, ``height``, ``tanfovx``, ``tanfovy``, ``viewmatrix``, ``depth``, ``depth_scale``, ``label``, ``rgb8`` --
    tensors or None), ``out_from_scene`` (12 floats, row-major 3 x 4), ``crop`` (None or (lo, hi)), ``exclude`` ((2048,)
    int32 bitmap or None), ``mode``, ``K``, ``fps_candidates``, ``xyzw`` / ``rgb`` / ``segmentation`` / ``count`` (outputs),
    ``workspace`` (uint8 tensor).  ``binding``: "auto" (the compiled one when built), "ext" or "ctypes"."""
    def ptr(t):
        return int(t.data_ptr()) if t is not None and t.numel() else 0

    views = [(int(v["width"]), int(v["height"]), float(v["tanfovx"]), float(v["tanfovy"]), ptr(v["viewmatrix"]),
              ptr(v["depth"]), float(v["depth_scale"]), ptr(v.get("label")), ptr(v.get("rgb8"))) for v in spec["views"]]
    crop = spec.get("crop")
    lo, hi = ([float(x) for x in crop[0]], [float(x) for x in crop[1]]) if crop is not None else ([0.0] * 3, [0.0] * 3)
    ws = spec["workspace"]
    vals = (int(spec["E"]), int(spec["C"]), views, [float(x) for x in spec["out_from_scene"]], int(crop is not None), lo, hi,
            ptr(spec.get("exclude")), int(spec["mode"]), int(spec.get("K", 0)), int(spec.get("fps_candidates", 0)),
            ptr(spec["xyzw"]), ptr(spec["rgb"]), ptr(spec["segmentation"]), ptr(spec["count"]), ptr(ws), int(ws.numel()))
    use_ext = _ext is not None and hasattr(_ext, "CloudPack") if binding == "auto" else binding == "ext"
    if use_ext:
        if _ext is None or not hasattr(_ext, "CloudPack"):
            raise RuntimeError("the compiled binding (gsworld_amd._C_ext) with CloudPack is not built")
        return ("ext", _ext.CloudPack(vals))
    arr = (_lib.GsrCloudView * len(views))(*[_lib.GsrCloudView(*v) for v in views])
    cs = _lib.GsrCloudSpec()
    cs.struct_size = C.sizeof(_lib.GsrCloudSpec)
    cs.E, cs.C, cs.views = vals[0], vals[1], arr
    cs.out_from_scene[:] = vals[3]
    cs.crop = vals[4]
    cs.crop_lo[:], cs.crop_hi[:] = lo, hi
    (cs.exclude, cs.mode, cs.K, cs.fps_candidates, cs.out_xyzw, cs.out_rgb, cs.out_segmentation, cs.out_count,
     cs.workspace, cs.workspace_bytes) = (vals[7] or None, *vals[8:11], *(v or None for v in vals[11:16]), vals[16])
    return ("ctypes", (cs, arr))


def run_pointcloud(pack, device) -> None:
    """Enqueues the ``gsr_render_pointcloud`` call of :func:`pack_pointcloud` on the current stream of ``device``
    (capturable)."""
    kind, p = pack
    dev = torch.device(device)
    if kind == "ext":
        p.run(dev.index if dev.index is not None else torch.cuda.current_device())
        return
    with torch.cuda.device(dev):
        check(lib().gsr_render_pointcloud(C.byref(p[0]), _stream(dev)))


def pack_cameras(n: int, extrinsic, projection, out, offsets, rigid_sim2real, scale_sim2real, binding: str = "auto"):
    """The arguments of one ``gsr_cameras_from_extrinsics`` call (include/gsr.h), built once: ``n`` views, device tensors
    ``extrinsic`` / ``projection`` / ``out`` (float32) and ``offsets`` (int32, 3 per view, or None: packed views), the
    16 floats of ``rigid_sim2real`` (row-major) and ``scale_sim2real``.  The tensors must outlive the pack.  ``binding``:
    "auto" (the compiled one when built), "ext" or "ctypes"."""
    def ptr(t):
        return int(t.data_ptr()) if t is not None and t.numel() else 0

    vals = (int(n), ptr(extrinsic), ptr(projection), ptr(out), ptr(offsets), [float(x) for x in rigid_sim2real],
            float(scale_sim2real))
    use_ext = _ext is not None and hasattr(_ext, "CamPack") if binding == "auto" else binding == "ext"
    if use_ext:
        if _ext is None or not hasattr(_ext, "CamPack"):
            raise RuntimeError("the compiled binding (gsworld_amd._C_ext) with CamPack is not built")
        return ("ext", _ext.CamPack(vals))
    cs = _lib.GsrSensorCameras()
    cs.struct_size = C.sizeof(_lib.GsrSensorCameras)
    cs.n = vals[0]
    cs.extrinsic, cs.projection, cs.out, cs.offsets = (v or None for v in vals[1:5])
    cs.rigid_sim2real[:] = vals[5]
    cs.scale_sim2real = vals[6]
    return ("ctypes", cs)


def run_cameras(pack, device) -> None:
    """Enqueues the ``gsr_cameras_from_extrinsics`` call of :func:`pack_cameras` on the current stream of ``device``
    (capturable)."""
    kind, p = pack
    dev = torch.device(device)
    if kind == "ext":
        p.run(dev.index if dev.index is not None else torch.cuda.current_device())
        return
    with torch.cuda.device(dev):
        check(lib().gsr_cameras_from_extrinsics(C.byref(p), _stream(dev)))


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, antialiasing, debug, sh_rest=None, param_space: int = 0):
    """-> (num_rendered, out_color (3,H,W), radii (P,), geomBuffer, binningBuffer, imgBuffer, out_invdepth (1,H,W)).

    Upstream's positional signature; the extensions are keywords (forward only): ``sh_rest`` -- ``sh`` = features_dc
    (P,1,3), ``sh_rest`` = features_rest (P,M-1,3), read in place instead of a per-frame ``cat``; ``param_space`` --
    OR of ``_lib.RAW_*``: ``opacity`` / ``scales`` / ``rotations`` are the raw parameters and are activated inside
    preprocess."""
    if _ext is not None:
        return _ext.rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, float(scale_modifier),
                                        cov3D_precomp, viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy),
                                        int(image_height), int(image_width), sh, int(degree), campos,
                                        bool(prefiltered), bool(antialiasing), bool(debug), sh_rest, int(param_space),
                                        float(NEAR_PLANE), _tuning_list(None))
    if means3D.ndim != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if sh_rest is not None and (sh.ndim != 3 or sh.size(1) != 1 or sh_rest.ndim != 3 or sh_rest.size(0) != sh.size(0)):
        raise RuntimeError("sh_rest needs sh = features_dc of shape (num_points, 1, 3)")
    _require_gpu(means3D, "means3D")
    dev = means3D.device
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=dev)
    # (a frame writes every pixel and every radius itself; upstream's zero fill is what P == 0 returns)
    alloc = torch.empty if P != 0 else torch.zeros
    out_color = alloc((3, H, W), **f32)
    out_invdepth = alloc((1, H, W), **f32)
    radii = alloc((P,), dtype=torch.int32, device=dev)
    geomBuffer = torch.empty(0, dtype=torch.uint8, device=dev)
    binningBuffer = torch.empty(0, dtype=torch.uint8, device=dev)
    imgBuffer = torch.empty(0, dtype=torch.uint8, device=dev)
    rendered = 0
    if P != 0:
        M = sh.size(1) if sh.numel() != 0 else 0
        if sh_rest is not None:
            M = 1 + sh_rest.size(1)
        st = GsrSettings(H, W, float(tan_fovx), float(tan_fovy), float(scale_modifier), int(degree), int(M),
                         int(bool(prefiltered)), int(bool(antialiasing)), int(bool(debug)), float(NEAR_PLANE))
        stats = forward_raw(
            st, _f32(background, dev, "background"), _f32(means3D, dev, "means3D"), _f32(colors, dev, "colors"),
            _f32(opacity, dev, "opacity"), _f32(scales, dev, "scales"), _f32(rotations, dev, "rotations"),
            _f32(cov3D_precomp, dev, "cov3D_precomp"), _f32(viewmatrix, dev, "viewmatrix"),
            _f32(projmatrix, dev, "projmatrix"), _f32(sh, dev, "sh"), _f32(campos, dev, "campos"),
            out_color, out_invdepth, radii, geomBuffer, binningBuffer, imgBuffer, r_capacity=0,
            sh_rest=_f32(sh_rest, dev, "sh_rest") if sh_rest is not None else None, param_space=param_space,
            forward_only=None)
        rendered = int(stats.num_rendered)
    return rendered, out_color, radii, geomBuffer, binningBuffer, imgBuffer, out_invdepth


# Largest instance list the no-sync training forward may allocate (bytes; 4 per instance).  288 GB of HBM make the TRUE
# bound affordable for training-sized problems: a Gaussian touches at most every tile, so num_rendered <= P x tiles.
NOSYNC_LIST_BYTES = 8 << 30
_FREE_CACHE = {}


def nosync_capacity(P: int, image_height: int, image_width: int, device=None):
    """Instance capacity with which a frame can never overflow (P x tiles), or None when that list would not fit
    ``NOSYNC_LIST_BYTES`` -- or, with ``device``, a quarter of what is free there -- or the grid is wider than the
    counting placement takes: the caller keeps sizing the list from a read-back."""
    gx, gy = (int(image_width) + 15) // 16, (int(image_height) + 15) // 16
    cap = int(P) * gx * gy
    # (gx * gy > 16384 = GSR_MAX_COUNT_TILES: such grids take the radix placement, whose binning state is 24 B per
    # instance plus sort tables, not 4 -- the byte budget below would be off by 6x)
    if P <= 0 or gx > 256 or gx * gy > 16384 or cap >= (1 << 31) or 4 * cap > NOSYNC_LIST_BYTES:
        return None
    if device is not None:
        # a quarter of what is free, looked up at most every 32nd call per (size, device): hipMemGetInfo is a driver call
        key = (int(P), gx, gy, str(device))
        n, free = _FREE_CACHE.get(key, (0, None))
        if free is None or n % 32 == 0:
            free = torch.cuda.mem_get_info(device)[0]
        _FREE_CACHE[key] = (n + 1, free)
        if 4 * cap > free // 4:
            return None
    if _lib.TUNING["binning_path"] != 0 or _lib.TUNING["depth_sort"] != 0:
        return None  # (A/B paths keep keys / ping-pong sides per instance: their lists are sized exactly)
    return cap


def rasterize_gaussians_nosync(capacity, background, means3D, opacity, scales, rotations, scale_modifier, viewmatrix,
                               projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                               antialiasing, debug, sh_rest=None, param_space: int = 0, colors=None, cov3D_precomp=None):
    """The training forward WITHOUT upstream's host read of num_rendered in the middle of the frame (a ~40 us hole in
    the GPU's timeline per step: D2H copy, host wake-up, allocation, launch): the instance list is sized by ``capacity``
    = :func:`nosync_capacity`, a bound no frame can exceed, so nothing has to be read back.  Same kernels, same image
    and state as :func:`rasterize_gaussians`; returns ``capacity`` where that returns num_rendered (it is what the
    backward carves the binning buffer with)."""
    _require_gpu(means3D, "means3D")
    dev = means3D.device
    P = means3D.size(0)
    H, W = int(image_height), int(image_width)
    f32 = dict(dtype=torch.float32, device=dev)
    out_color, out_invdepth = torch.empty((3, H, W), **f32), torch.empty((1, H, W), **f32)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    geomBuffer, imgBuffer = (torch.empty(0, dtype=torch.uint8, device=dev) for _ in range(2))
    # the instance list is allocated HERE (4 B per instance on the counting placement + one alignment unit; nosync_capacity
    # only hands out capacities for that path): a list that does not fit raises torch.cuda.OutOfMemoryError in Python,
    # where the caller's fallback to exact sizing catches it -- inside the library's resize callback the exception would be
    # swallowed by ctypes and come back as a generic allocation error.  The callback's resize_ to a smaller size keeps
    # this storage.
    binningBuffer = torch.empty(4 * int(capacity) + 512, dtype=torch.uint8, device=dev)
    M = (1 + sh_rest.size(1)) if sh_rest is not None else (sh.size(1) if sh.numel() != 0 else 0)
    st = GsrSettings(H, W, float(tan_fovx), float(tan_fovy), float(scale_modifier), int(degree), int(M), 0,
                     int(bool(antialiasing)), int(bool(debug)), float(NEAR_PLANE))
    e = torch.empty(0, device=dev)
    forward_raw(st, _f32(background, dev, "background"), _f32(means3D, dev, "means3D"),
                _f32(colors, dev, "colors") if colors is not None else e,
                _f32(opacity, dev, "opacity"), _f32(scales, dev, "scales"), _f32(rotations, dev, "rotations"),
                _f32(cov3D_precomp, dev, "cov3D_precomp") if cov3D_precomp is not None else e,
                _f32(viewmatrix, dev, "viewmatrix"), _f32(projmatrix, dev, "projmatrix"), _f32(sh, dev, "sh"),
                _f32(campos, dev, "campos"), out_color, out_invdepth, radii, geomBuffer, binningBuffer, imgBuffer,
                r_capacity=int(capacity), want_stats=False,
                sh_rest=_f32(sh_rest, dev, "sh_rest") if sh_rest is not None else None, param_space=param_space,
                forward_only=None)
    return int(capacity), out_color, radii, geomBuffer, binningBuffer, imgBuffer, out_invdepth


def rasterize_gaussians_backward(background, means3D, radii, colors, opacities, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_invdepth, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                 antialiasing, debug, sh_rest=None, param_space=0):
    """-> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)
    [+ dL_dsh_rest with ``sh_rest``; opacity / scale / rotation gradients w.r.t. the raw parameters with ``param_space``]."""
    if _ext is not None:
        return tuple(_ext.rasterize_gaussians_backward(
            background, means3D, radii, colors, opacities, scales, rotations, float(scale_modifier), cov3D_precomp,
            viewmatrix, projmatrix, float(tan_fovx), float(tan_fovy), dL_dout_color,
            dL_dout_invdepth if dL_dout_invdepth is not None else None, sh, int(degree), campos, geomBuffer, int(R),
            binningBuffer, imageBuffer, bool(antialiasing), bool(debug), sh_rest, int(param_space), float(NEAR_PLANE)))
    from . import _backward

    return _backward.rasterize_gaussians_backward(
        background, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
        projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_invdepth, sh, degree, campos, geomBuffer, R,
        binningBuffer, imageBuffer, antialiasing, debug, NEAR_PLANE, sh_rest=sh_rest, param_space=param_space)


def mark_visible(means3D, viewmatrix, projmatrix):
    """-> bool (P,): Gaussians in front of the near plane (upstream markVisible; projmatrix is unused there too)."""
    if _ext is not None:
        return _ext.mark_visible(means3D, viewmatrix, projmatrix, float(NEAR_PLANE))
    _require_gpu(means3D, "means3D")
    dev = means3D.device
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P != 0:
        m3 = _f32(means3D, dev, "means3D")
        vm = _f32(viewmatrix, dev, "viewmatrix")
        with torch.cuda.device(dev):
            check(lib().gsr_mark_visible(P, _ptr(m3), _ptr(vm), C.c_float(NEAR_PLANE), C.c_void_p(present.data_ptr()),
                                         _stream(dev)))
    return present


# ---- the optimizer step and the densification statistics (include/gsr.h gsr_adam_update / gsr_densification_stats) ----
def _dense_f32(t, what: str, numel: int, dev=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{what} must be a tensor")
    _require_gpu(t, what)
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{what} is on {t.device}, the other tensors of the call on {dev}")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous float32 tensor")
    if t.numel() != numel:
        raise RuntimeError(f"{what} has {t.numel()} elements, {numel} expected")
    return t


def _visible_arg(visible, N: int, dev):
    """-> (tensor kept alive | None, GSR_VISIBLE_* kind) of a ``visible`` argument: None, a bool / uint8 mask or int32 radii."""
    if visible is None:
        return None, _lib.VISIBLE_ALL
    if not isinstance(visible, torch.Tensor) or visible.dtype not in (torch.bool, torch.uint8, torch.int32):
        raise RuntimeError("visible must be None, a bool / uint8 mask or the int32 radii tensor")
    _require_gpu(visible, "visible")
    if visible.device != dev or visible.numel() != N:
        raise RuntimeError(f"visible must hold {N} values on {dev}")
    return visible.contiguous(), (_lib.VISIBLE_RADII if visible.dtype == torch.int32 else _lib.VISIBLE_MASK8)


def _use_ext(binding: str, name: str) -> bool:
    if binding == "auto":
        return _ext is not None and hasattr(_ext, name)
    if binding == "ext":
        if _ext is None or not hasattr(_ext, name):
            raise RuntimeError(f"the compiled binding (gsworld_amd._C_ext) with {name} is not built")
        return True
    if binding != "ctypes":
        raise ValueError(f"binding must be 'auto', 'ext' or 'ctypes', got {binding!r}")
    return False


def adam_update_groups(groups, visible, N: int, binding: str = "auto") -> None:
    """One ``gsr_adam_update`` launch for every group of an optimizer step (include/gsr.h holds the definition): Adam without
    bias correction on the Gaussians ``visible`` marks -- None (all), a bool / uint8 ``(N,)`` mask or the int32 ``radii`` of the
    forward (> 0) --; the others keep parameter and moments bit for bit.  ``groups``: 1 .. 8 dicts with ``param``, ``grad``,
    ``exp_avg``, ``exp_avg_sq`` (``N * M`` float32 each; a non-contiguous grad is made contiguous, the others must be),
    ``lr``, ``eps`` and optionally ``beta1`` / ``beta2`` (0.9 / 0.999) and ``M`` (else ``param.numel() // N``).  Enqueued on
    the current stream, no synchronisation.  ``binding``: "auto" (the compiled one when built), "ext" or "ctypes"."""
    N = int(N)
    if not 1 <= len(groups) <= _lib.ADAM_MAX_GROUPS:
        raise RuntimeError(f"adam_update_groups: 1 .. {_lib.ADAM_MAX_GROUPS} groups per call, got {len(groups)}")
    if N < 0:
        raise RuntimeError(f"adam_update_groups: N = {N}")
    dev = None
    vals, keep = [], []
    for k, g in enumerate(groups):
        p = g["param"]
        if isinstance(p, torch.Tensor):
            _require_gpu(p, f"group {k}: param")
            dev = p.device if dev is None else dev
        M = int(g["M"]) if g.get("M") is not None else (p.numel() // N if N else 1)
        if not 1 <= M <= _lib.ADAM_MAX_M:
            raise RuntimeError(f"group {k}: M = {M} floats per Gaussian (1 .. {_lib.ADAM_MAX_M})")
        p = _dense_f32(p, f"group {k}: param", N * M, dev)
        m = _dense_f32(g["exp_avg"], f"group {k}: exp_avg", N * M, dev)
        v = _dense_f32(g["exp_avg_sq"], f"group {k}: exp_avg_sq", N * M, dev)
        grad = g["grad"]
        if isinstance(grad, torch.Tensor) and grad.is_cuda and not grad.is_contiguous():
            grad = grad.contiguous()
        grad = _dense_f32(grad, f"group {k}: grad", N * M, dev)
        keep.append(grad)
        vals.append((p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), M, float(g["lr"]),
                     float(g.get("beta1", 0.9)), float(g.get("beta2", 0.999)), float(g["eps"])))
    vis, kind = _visible_arg(visible, N, dev)
    if N == 0:
        return
    vptr = vis.data_ptr() if vis is not None else 0
    if _use_ext(binding, "adam_update"):
        _ext.adam_update(dev.index if dev.index is not None else torch.cuda.current_device(), N, vptr, kind, vals)
        return
    s = _lib.GsrAdamStep()
    s.struct_size, s.N, s.num_groups, s.visible_kind, s.visible = C.sizeof(_lib.GsrAdamStep), N, len(vals), kind, vptr or None
    for k, t in enumerate(vals):
        s.groups[k] = _lib.GsrAdamGroup(*t)
    with torch.cuda.device(dev):
        check(lib().gsr_adam_update(C.byref(s), _stream(dev)))


def adamUpdate(param, param_grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M):
    """Upstream's ``_C.adamUpdate`` (the ``3dgs_accel`` rasterizer's sparse Adam), positional signature kept: one group of
    ``N`` Gaussians x ``M`` floats through :func:`adam_update_groups`."""
    adam_update_groups([{"param": param, "grad": param_grad, "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq, "lr": lr,
                         "beta1": b1, "beta2": b2, "eps": eps, "M": M}], visible, N)


def densification_stats(radii, grad_means2D, grad_accum, denom, max_radii2D=None, binding: str = "auto") -> None:
    """``gsr_densification_stats`` (include/gsr.h): for every Gaussian with ``radii > 0``, ``grad_accum += |grad_means2D[:, :2]|``,
    ``denom += 1`` and, when given, ``max_radii2D = max(max_radii2D, radii)`` -- in place, on the current stream, without the
    compaction and the host read of ``(radii > 0).nonzero()``.  ``radii`` int32 ``(N,)``; ``grad_means2D`` float32 ``(N, 3)``
    (made contiguous if it is not); the accumulators contiguous float32 with ``N`` elements."""
    if not isinstance(radii, torch.Tensor) or radii.dtype != torch.int32:
        raise RuntimeError("radii must be an int32 tensor")
    _require_gpu(radii, "radii")
    dev, N = radii.device, radii.numel()
    radii = radii.contiguous()
    if isinstance(grad_means2D, torch.Tensor) and grad_means2D.is_cuda:
        grad_means2D = grad_means2D.contiguous()
    g = _dense_f32(grad_means2D, "grad_means2D", 3 * N, dev)
    acc = _dense_f32(grad_accum, "grad_accum", N, dev)
    den = _dense_f32(denom, "denom", N, dev)
    mx = _dense_f32(max_radii2D, "max_radii2D", N, dev) if max_radii2D is not None else None
    if N == 0:
        return
    ptrs = (radii.data_ptr(), g.data_ptr(), acc.data_ptr(), den.data_ptr(), mx.data_ptr() if mx is not None else 0)
    if _use_ext(binding, "densification_stats"):
        _ext.densification_stats(dev.index if dev.index is not None else torch.cuda.current_device(), N, *ptrs)
        return
    with torch.cuda.device(dev):
        check(lib().gsr_densification_stats(N, *(C.c_void_p(p or None) for p in ptrs), _stream(dev)))


# ---- densify-and-prune (include/gsr.h gsr_densify_plan / gsr_densify_apply) -------------------------------------------
def densify_workspace_bytes(N: int) -> int:
    """``gsr_densify_workspace_bytes``: the workspace ``densify_plan`` fills for ``densify_apply`` (a multiple of 256)."""
    return int(lib().gsr_densify_workspace_bytes(int(N)))


def densify_plan(grad_accum, denom, scaling, opacity, *, grad_threshold, min_opacity, dense_limit, world_limit,
                 prune_world_size, counts=None, workspace=None, binding: str = "auto"):
    """``gsr_densify_plan`` (include/gsr.h holds the definition): the decisions of upstream's ``densify_and_prune`` for every
    Gaussian -- kept, cloned, split into two children, pruned -- from the accumulated statistics and the raw ``scaling`` (N, 3)
    and ``opacity`` (N elements).  -> ``(counts, workspace)``: ``counts`` int32 (4,) on the device (kept, clones, split, N_out),
    ``workspace`` the uint8 tensor ``densify_apply`` reads; both are allocated when not given.  The four scalars are passed as
    binary32 values.  Three launches on the current stream, no synchronisation; N = 0 launches nothing (counts is zeroed)."""
    if not isinstance(scaling, torch.Tensor):
        raise RuntimeError("scaling must be a tensor")
    _require_gpu(scaling, "scaling")
    dev = scaling.device
    N = scaling.numel() // 3
    if N > _lib.DENSIFY_MAX_N:
        raise RuntimeError(f"densify_plan: N = {N} exceeds 2^30")
    sc = _dense_f32(scaling, "scaling", 3 * N, dev)
    acc = _dense_f32(grad_accum, "grad_accum", N, dev)
    den = _dense_f32(denom, "denom", N, dev)
    op = _dense_f32(opacity, "opacity", N, dev)
    nbytes = densify_workspace_bytes(N)
    if workspace is None:
        workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    elif (not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8
          or not workspace.is_contiguous() or workspace.numel() < nbytes):
        raise RuntimeError(f"workspace must be a contiguous uint8 tensor of at least {nbytes} bytes on {dev}")
    if counts is None:
        counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    elif (not isinstance(counts, torch.Tensor) or counts.device != dev or counts.dtype != torch.int32
          or not counts.is_contiguous() or counts.numel() != 4):
        raise RuntimeError(f"counts must be a contiguous int32 tensor of 4 elements on {dev}")
    if N == 0:
        counts.zero_()
        return counts, workspace
    thr, mop, dl, wl = (float(np.float32(x)) for x in (grad_threshold, min_opacity, dense_limit, world_limit))
    if _use_ext(binding, "densify_plan"):
        _ext.densify_plan(dev.index if dev.index is not None else torch.cuda.current_device(), N, acc.data_ptr(),
                          den.data_ptr(), sc.data_ptr(), op.data_ptr(), thr, mop, dl, wl, bool(prune_world_size),
                          counts.data_ptr(), workspace.data_ptr(), workspace.numel())
        return counts, workspace
    s = _lib.GsrDensifyPlan()
    s.struct_size, s.N = C.sizeof(_lib.GsrDensifyPlan), N
    s.grad_accum, s.denom, s.scaling, s.opacity = acc.data_ptr(), den.data_ptr(), sc.data_ptr(), op.data_ptr()
    s.grad_threshold, s.min_opacity, s.dense_limit, s.world_limit = thr, mop, dl, wl
    s.prune_world_size = int(bool(prune_world_size))
    s.counts, s.workspace, s.workspace_bytes = counts.data_ptr(), workspace.data_ptr(), workspace.numel()
    with torch.cuda.device(dev):
        check(lib().gsr_densify_plan(C.byref(s), _stream(dev)))
    return counts, workspace


DENSIFY_ROLES = {"copy": _lib.DENSIFY_COPY, "xyz": _lib.DENSIFY_XYZ, "scaling": _lib.DENSIFY_SCALING}


def densify_apply(N: int, N_out: int, workspace, xyz, scaling, rotation, noise, groups, parent,
                  binding: str = "auto") -> None:
    """``gsr_densify_apply`` (include/gsr.h): ONE launch that writes the ``N_out`` output rows of every group -- kept rows with
    their moments, clones and children with zero moments, children of the ``"xyz"`` / ``"scaling"`` roles computed -- and
    ``parent`` (int32, ``N_out``).  ``groups``: up to 8 dicts with ``src`` and ``dst``, each ``(param, exp_avg, exp_avg_sq)``
    with both moments None for a group without state, and optionally ``M`` and ``role`` ("copy", "xyz", "scaling").  ``N``,
    ``workspace``: the plan's; ``N_out``: what the caller read from the plan's ``counts[3]``; ``noise`` (N, 2, 3) standard
    normals indexed by parent.  Enqueued on the current stream, no synchronisation."""
    N, N_out = int(N), int(N_out)
    if len(groups) > _lib.ADAM_MAX_GROUPS:
        raise RuntimeError(f"densify_apply: at most {_lib.ADAM_MAX_GROUPS} groups per call, got {len(groups)}")
    if not 0 <= N <= _lib.DENSIFY_MAX_N or not 0 <= N_out <= 2 * N:
        raise RuntimeError(f"densify_apply: N = {N}, N_out = {N_out}")
    if not isinstance(xyz, torch.Tensor):
        raise RuntimeError("xyz must be a tensor")
    _require_gpu(xyz, "xyz")
    dev = xyz.device
    x = _dense_f32(xyz, "xyz", 3 * N, dev)
    sc = _dense_f32(scaling, "scaling", 3 * N, dev)
    rot = _dense_f32(rotation, "rotation", 4 * N, dev)
    nz = _dense_f32(noise, "noise", 6 * N, dev)
    if (not isinstance(parent, torch.Tensor) or parent.device != dev or parent.dtype != torch.int32
            or not parent.is_contiguous() or parent.numel() != N_out):
        raise RuntimeError(f"parent must be a contiguous int32 tensor of {N_out} elements on {dev}")
    if (not isinstance(workspace, torch.Tensor) or workspace.device != dev or workspace.dtype != torch.uint8
            or not workspace.is_contiguous()):
        raise RuntimeError(f"workspace must be the contiguous uint8 tensor of densify_plan on {dev}")
    vals = []
    for k, g in enumerate(groups):
        sp = g["src"][0]
        M = int(g["M"]) if g.get("M") is not None else (sp.numel() // N if N else 1)
        if not 1 <= M <= _lib.ADAM_MAX_M:
            raise RuntimeError(f"group {k}: M = {M} floats per Gaussian (1 .. {_lib.ADAM_MAX_M})")
        moments = g["src"][1] is not None
        if any((t is not None) != moments for t in (g["src"][2], g["dst"][1], g["dst"][2])):
            raise RuntimeError(f"group {k}: exp_avg, exp_avg_sq and their outputs are all given or all None")
        ptrs = []
        for side, rows in (("src", N), ("dst", N_out)):
            for name, t in zip(("param", "exp_avg", "exp_avg_sq"), g[side]):
                ptrs.append(0 if t is None else _dense_f32(t, f"group {k}: {side} {name}", rows * M, dev).data_ptr())
        vals.append((*ptrs, M, DENSIFY_ROLES[g.get("role", "copy")]))
    if N == 0 or N_out == 0:
        return
    if _use_ext(binding, "densify_apply"):
        _ext.densify_apply(dev.index if dev.index is not None else torch.cuda.current_device(), N, N_out,
                           workspace.data_ptr(), workspace.numel(), x.data_ptr(), sc.data_ptr(), rot.data_ptr(),
                           nz.data_ptr(), parent.data_ptr(), vals)
        return
    s = _lib.GsrDensifyApply()
    s.struct_size, s.N, s.N_out, s.num_groups = C.sizeof(_lib.GsrDensifyApply), N, N_out, len(vals)
    s.workspace, s.workspace_bytes = workspace.data_ptr(), workspace.numel()
    s.xyz, s.scaling, s.rotation, s.noise, s.parent = x.data_ptr(), sc.data_ptr(), rot.data_ptr(), nz.data_ptr(), parent.data_ptr()
    for k, t in enumerate(vals):
        s.groups[k] = _lib.GsrDensifyGroup(*(v or None for v in t[:6]), t[6], t[7])
    with torch.cuda.device(dev):
        check(lib().gsr_densify_apply(C.byref(s), _stream(dev)))


# ---- the fused training loss (include/gsr.h gsr_train_loss / gsr_train_loss_backward) -----------------------------------
def train_loss_scratch_floats(H: int, W: int) -> int:
    return int(lib().gsr_train_loss_scratch_floats(int(H), int(W)))


def train_loss_scratch_needed(H: int, W: int, exposure: bool, alpha_mask: bool) -> int:
    """``gsr_train_loss_scratch_needed``: the floats of scratch a call of this size with / without an exposure and an alpha
    mask needs (host arithmetic; at most ``train_loss_scratch_floats(H, W)``)."""
    a = _lib.GsrTrainLoss(struct_size=C.sizeof(_lib.GsrTrainLoss), H=int(H), W=int(W), exposure=8 if exposure else None,
                          alpha_mask=8 if alpha_mask else None)  # (presence only: nothing is dereferenced)
    return int(lib().gsr_train_loss_scratch_needed(C.byref(a)))


_TRAIN_LOSS_PTRS = frozenset((3, 4, 5, 6, 7, 8, 9, 12, 14, 15, 16, 17, 18, 19))  # positions of the pointers in `vals`


def train_loss(vals, device, backward: bool = False, binding: str = "auto") -> None:
    """One ``gsr_train_loss`` (or ``_backward``) on the current stream of ``device``.  ``vals``: the fields of ``GsrTrainLoss``
    behind ``struct_size`` in the header's order, buffers as device addresses (0 = NULL); gsworld_amd/ssim.py has checked
    dtype, device and layout.  No synchronisation."""
    if _use_ext(binding, "train_loss"):
        _ext.train_loss(device.index if device.index is not None else torch.cuda.current_device(), bool(backward), tuple(vals))
        return
    a = _lib.GsrTrainLoss(C.sizeof(_lib.GsrTrainLoss), *(v or None if k in _TRAIN_LOSS_PTRS else v for k, v in enumerate(vals)))
    with torch.cuda.device(device):
        check((lib().gsr_train_loss_backward if backward else lib().gsr_train_loss)(C.byref(a), _stream(device)))
