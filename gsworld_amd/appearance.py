"""Per-environment appearance randomization of the splatted scene (visual domain randomization).

Every Gaussian's colour -- what preprocess evaluates from its SH coefficients, ``max(sh + 0.5, 0)``, or a precomputed
colour -- goes through the 3 x 4 affine ``[M | t]`` of its appearance group inside preprocess (include/gsr.h
``GsrInputs.appearance``):

    c'_j = max(((M[j][0] r + M[j][1] g) + M[j][2] b) + t[j], 0)      j = r, g, b

in round-to-nearest binary32 multiplies and adds in exactly this order (:func:`apply_table` restates it in NumPy bit for
bit).  A group is a set of semantic labels (a table, an object); group 0 is everything else.
:class:`gsworld_amd.closed_loop.ClosedLoopRenderer` keeps one table per environment (``appearance=`` /
:meth:`~gsworld_amd.closed_loop.ClosedLoopRenderer.set_appearance`).

The helpers below build the affines (float64 ``(3, 4)`` arrays) on the host; :class:`AppearanceRandomizer` draws a table
per environment at reset from a seeded generator.  The kernel only applies what it is handed.
"""
from __future__ import annotations

import math

import numpy as np

LUMA = (0.299, 0.587, 0.114)  # ITU-R BT.601 weights (what torchvision's rgb_to_grayscale uses)


def _affine(M, t=(0.0, 0.0, 0.0)) -> np.ndarray:
    A = np.zeros((3, 4), np.float64)
    A[:, :3] = np.asarray(M, np.float64)
    A[:, 3] = np.asarray(t, np.float64)
    return A


def identity() -> np.ndarray:
    return _affine(np.eye(3))


def brightness(b: float) -> np.ndarray:
    """``c' = b c``."""
    return _affine(float(b) * np.eye(3))


def contrast(k: float) -> np.ndarray:
    """``c' = k (c - 0.5) + 0.5``: contrast about mid-grey 0.5 -- NOT about the image's mean as torchvision's
    ``adjust_contrast`` does (a per-Gaussian transform does not know the image)."""
    k = float(k)
    return _affine(k * np.eye(3), (0.5 * (1.0 - k),) * 3)


def saturation(s: float) -> np.ndarray:
    """``c' = s c + (1 - s) luma(c)`` with the luma weights ``(0.299, 0.587, 0.114)``: 0 gives the luma on every channel,
    1 the identity."""
    s = float(s)
    L = np.tile(np.asarray(LUMA, np.float64), (3, 1))
    return _affine(s * np.eye(3) + (1.0 - s) * L)


def hue(theta: float) -> np.ndarray:
    """Rotation by ``theta`` radians about the grey axis (1, 1, 1) / sqrt(3) (Rodrigues).  A LINEAR hue shift: it keeps grey
    and the channel sum fixed and cycles r -> g -> b at 2 pi / 3 -- not the HSV hue of torchvision's ``adjust_hue``."""
    c, s = math.cos(float(theta)), math.sin(float(theta))
    k = np.full(3, 1.0 / math.sqrt(3.0))
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return _affine(c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k))


def gain(rgb) -> np.ndarray:
    """Per-channel gains: ``c'_j = rgb[j] c_j``."""
    g = np.asarray(rgb, np.float64).reshape(3)
    return _affine(np.diag(g))


def compose(*ops) -> np.ndarray:
    """The affine that applies ``ops`` LEFT TO RIGHT: ``compose(a, b)(c) = b(a(c))``."""
    M, t = np.eye(3), np.zeros(3)
    for op in ops:
        A = np.asarray(op, np.float64).reshape(3, 4)
        M, t = A[:, :3] @ M, A[:, :3] @ t + A[:, 3]
    return _affine(M, t)


def apply_table(table, colours) -> np.ndarray:
    """NumPy float32 restatement of the kernel's transform: ``table`` (3, 4), ``colours`` (N, 3) -> (N, 3) float32."""
    T = np.asarray(table, np.float32).reshape(3, 4)
    c = np.asarray(colours, np.float32).reshape(-1, 3)
    r, g, b = c[:, 0], c[:, 1], c[:, 2]
    out = np.empty_like(c)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(3):
            out[:, j] = np.maximum(((T[j, 0] * r + T[j, 1] * g) + T[j, 2] * b) + T[j, 3], np.float32(0.0))
    return out


def _range(name, v, default):
    if v is None:
        return default
    lo, hi = (float(x) for x in v)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo > hi:
        raise ValueError(f"{name}: expected (lo, hi) with lo <= hi, got {v!r}")
    return lo, hi


class AppearanceRandomizer:
    """Draws per-environment appearance tables from a seeded ``numpy.random.Generator``.

    Every parameter is a ``(lo, hi)`` uniform range (None: fixed at the identity): ``brightness`` and ``contrast`` factors,
    ``saturation`` factor, ``hue`` angle in radians, ``gain`` per-channel factors (one range for all three channels, drawn
    independently).  A group's affine is ``compose(brightness, contrast, saturation, hue, gain)``.  ``per_group=True``: each
    group draws its own; False: one draw per environment for every group.  ``background``: ``(lo_rgb, hi_rgb)`` per-channel
    range of the background colour, or None (black).  Draws are deterministic per seed; the kernel applies them."""

    def __init__(self, num_groups: int, brightness=None, contrast=None, saturation=None, hue=None, gain=None,
                 background=None, per_group: bool = True, seed: int = 0):
        self.G = int(num_groups)
        if not 1 <= self.G <= 64:
            raise ValueError(f"num_groups must be 1..64, got {num_groups}")
        self.brightness = _range("brightness", brightness, (1.0, 1.0))
        self.contrast = _range("contrast", contrast, (1.0, 1.0))
        self.saturation = _range("saturation", saturation, (1.0, 1.0))
        self.hue = _range("hue", hue, (0.0, 0.0))
        self.gain = _range("gain", gain, (1.0, 1.0))
        if background is not None:
            lo, hi = (np.asarray(x, np.float64).reshape(3) for x in background)
            if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
                raise ValueError(f"background: expected (lo_rgb, hi_rgb) with lo <= hi, got {background!r}")
            self.background = (lo, hi)
        else:
            self.background = None
        self.per_group = bool(per_group)
        self.rng = np.random.default_rng(seed)

    def _one(self) -> np.ndarray:
        u = self.rng.uniform
        return compose(brightness(u(*self.brightness)), contrast(u(*self.contrast)), saturation(u(*self.saturation)),
                       hue(u(*self.hue)), gain(u(self.gain[0], self.gain[1], size=3)))

    def sample(self, n: int):
        """-> ``(tables (n, G, 3, 4) float32, backgrounds (n, 3) float32)`` for ``n`` environments."""
        tables = np.empty((int(n), self.G, 3, 4), np.float32)
        for e in range(int(n)):
            if self.per_group:
                for g in range(self.G):
                    tables[e, g] = self._one()
            else:
                tables[e, :] = self._one()
        if self.background is None:
            bgs = np.zeros((int(n), 3), np.float32)
        else:
            lo, hi = self.background
            bgs = self.rng.uniform(lo, hi, size=(int(n), 3)).astype(np.float32)
        return tables, bgs


def check_groups(groups: dict, semantics=None):
    """The loop's ``appearance={name: labels}`` -> (names, lut (int32 numpy), number of groups G = len + 1).  Labels are
    integers in [0, 65535], each named by one group; with ``semantics`` (the model's labels) every label must occur in the
    model.  ``ValueError`` otherwise."""
    if not isinstance(groups, dict) or not groups:
        raise ValueError("appearance must be a non-empty dict {group name: label or labels}")
    if len(groups) + 1 > 64:
        raise ValueError(f"appearance: at most 63 named groups (group 0 is the rest), got {len(groups)}")
    owner, names = {}, list(groups.keys())
    for k, name in enumerate(names):
        labs = groups[name]
        labs = list(labs) if isinstance(labs, (list, tuple, np.ndarray)) else [labs]
        if not labs:
            raise ValueError(f"appearance group {name!r} names no label")
        for lab in labs:
            if isinstance(lab, (bool, np.bool_)) or float(lab) != int(lab) or not 0 <= int(lab) <= 65535:
                raise ValueError(f"appearance group {name!r}: label {lab!r} is not an integer in [0, 65535]")
            if int(lab) in owner:
                raise ValueError(f"appearance: label {int(lab)} is named by {owner[int(lab)]!r} and {name!r}")
            owner[int(lab)] = name
    if semantics is not None:
        present = set(int(x) for x in np.unique(np.asarray(semantics, np.float64).reshape(-1)) if np.isfinite(x))
        missing = sorted(l for l in owner if l not in present)
        if missing:
            raise ValueError(f"appearance: labels {missing} do not occur in the model's semantics")
    lut = np.zeros(max(owner) + 1, np.int32)
    for lab, name in owner.items():
        lut[lab] = names.index(name) + 1
    return names, lut, len(names) + 1


def check_tables(tables, backgrounds, env_ids, num_envs: int, G: int):
    """Arguments of :meth:`ClosedLoopRenderer.set_appearance` -> (tables (n, G, 3, 4) float32 tensor, backgrounds (n, 3)
    float32 tensor | None, env_ids list of n).  Host and device tensors / arrays are accepted; nothing is copied to a device
    here.  ``ValueError`` for wrong shapes or environments out of range."""
    import torch

    if env_ids is None:
        ids = list(range(int(num_envs)))
    else:
        ids = [int(e) for e in (env_ids.tolist() if hasattr(env_ids, "tolist") else env_ids)]
        if not ids or any(not 0 <= e < num_envs for e in ids) or len(set(ids)) != len(ids):
            raise ValueError(f"env_ids must be distinct environments in [0, {num_envs}), got {ids}")
    n = len(ids)
    t = tables if isinstance(tables, torch.Tensor) else torch.as_tensor(np.asarray(tables, np.float32))
    if tuple(t.shape) != (n, G, 3, 4):
        raise ValueError(f"appearance tables: expected shape ({n}, {G}, 3, 4), got {tuple(t.shape)}")
    t = t.to(torch.float32)
    b = None
    if backgrounds is not None:
        b = backgrounds if isinstance(backgrounds, torch.Tensor) else torch.as_tensor(np.asarray(backgrounds, np.float32))
        if tuple(b.shape) != (n, 3):
            raise ValueError(f"appearance backgrounds: expected shape ({n}, 3), got {tuple(b.shape)}")
        b = b.to(torch.float32)
    return t, b, ids
