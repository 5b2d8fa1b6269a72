"""The optimizer side of a training iteration on the device: ``SparseGaussianAdam`` -- the sparse Adam of upstream's
``3dgs_accel`` rasterizer (``adamUpdateCUDA``) -- and the densification statistics, both without the
``(radii > 0).nonzero()`` compaction and host read upstream's loop does every iteration.

    forward -> photometric_loss -> backward -> densification_stats(radii, ...) -> optimizer.step(radii, N)

The optimizer lives HERE, not in the drop-in ``diff_gaussian_rasterization`` package: GSWorld probes that package for the
name to pick its ``separate_sh`` call signature (gs_world_wrapper.py:22-26), which this project does not offer.  A training
script imports it from ``gsworld_amd.optim``.

``densify_and_prune`` is the half that runs every ``densification_interval`` iterations: upstream's clone / split / prune
sequence in four launches with one host read (the new model size).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _C


class SparseGaussianAdam(torch.optim.Adam):
    """Adam that updates only the Gaussians a frame saw, and leaves parameter and moments of the others bit for bit alone
    (their moments do not decay: upstream's semantics, not an approximation of dense Adam).  No bias correction; betas
    (0.9, 0.999).  One parameter tensor per group, ``(N, ...)`` contiguous float32 on a HIP device; every group with a
    gradient goes into ONE kernel launch (include/gsr.h ``gsr_adam_update`` is the definition).  State keys are upstream's
    (``step``, ``exp_avg``, ``exp_avg_sq``), so ``state_dict`` / ``load_state_dict`` and code that prunes or extends the
    moments work as with ``torch.optim.Adam``."""

    def __init__(self, params, lr, eps):
        super().__init__(params=params, lr=lr, eps=eps)

    @torch.no_grad()
    def step(self, visibility, N):
        """``visibility``: None (every Gaussian), a bool / uint8 ``(N,)`` mask, or the int32 ``radii`` of the forward
        (> 0 = visible), read on the device."""
        N = int(N)
        groups = []
        for group in self.param_groups:
            assert len(group["params"]) == 1, "more than one tensor in group"
            param = group["params"][0]
            if param.grad is None:
                continue
            if not param.is_cuda:
                raise RuntimeError(f"parameter {group.get('name', len(groups))!r} is on {param.device}: SparseGaussianAdam has "
                                   "no CPU path (tensors must live on a HIP device)")
            state = self.state[param]
            if len(state) == 0:
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            groups.append({"param": param, "grad": param.grad, "exp_avg": state["exp_avg"],
                           "exp_avg_sq": state["exp_avg_sq"], "lr": group["lr"], "beta1": 0.9, "beta2": 0.999,
                           "eps": group["eps"], "M": (param.numel() // N) if N else 1})
        # (gsr_adam_update takes 8 groups; a model with more parameter tensors takes one launch per 8)
        for k in range(0, len(groups), 8):
            _C.adam_update_groups(groups[k:k + 8], visibility, N)


def densification_stats(radii, viewspace_grad, xyz_gradient_accum, denom, max_radii2D=None):
    """For every Gaussian with ``radii > 0``: ``xyz_gradient_accum += norm(viewspace_grad[:, :2])``, ``denom += 1`` and, when
    given, ``max_radii2D = max(max_radii2D, radii)`` -- upstream's per-iteration bookkeeping in one launch, in place, with
    ``radii`` (int32 ``(N,)``, as the forward returns it) read on the device (include/gsr.h ``gsr_densification_stats``).
    The accumulators are float32 with N elements (``(N,)`` or ``(N, 1)``)."""
    _C.densification_stats(radii, viewspace_grad, xyz_gradient_accum, denom, max_radii2D)


DENSIFY_GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


@torch.no_grad()
def densify_and_prune(params, optimizer, grad_accum, denom, *, grad_threshold, min_opacity, extent, percent_dense,
                      prune_world_size, noise=None, generator=None):
    """Upstream's ``densify_and_prune`` -- clone the small hot Gaussians, split the large hot ones in two, prune the
    transparent and (``prune_world_size``: upstream's ``if max_screen_size:``) the oversized ones -- on the device, with ONE
    host read: plan (three launches) -> read ``counts`` -> allocate ``N_out`` rows -> apply (one launch for the six
    parameters and their moments).  include/gsr.h ``gsr_densify_plan`` / ``gsr_densify_apply`` hold the definition; the rows
    come out in upstream's order (kept | clones | first children | second children, each ascending).

    ``params`` maps upstream's group names (``xyz``, ``f_dc``, ``f_rest``, ``opacity``, ``scaling``, ``rotation``) to the
    ``(N, ...)`` contiguous float32 tensors; ``optimizer`` (``torch.optim.Adam``, ``SparseGaussianAdam`` or None) has them as
    its groups' single parameters.  Each group's tensor is replaced by a fresh ``nn.Parameter`` of ``N_out`` rows and its
    state re-keyed: ``step`` survives, the moments are carried (zero on new rows) where there were any.  ``noise``:
    ``(N, 2, 3)`` standard normals indexed by PARENT, drawn here (``generator``) when not given.

    -> ``(new_params: dict, counts: (kept, clones, split, N_out) as ints, parent: int32 (N_out,))``; ``parent[r]`` is the
    input row of output row ``r``, for carrying side arrays (labels, semantics) along."""
    missing = [n for n in DENSIFY_GROUPS if n not in params]
    if missing:
        raise RuntimeError(f"densify_and_prune: params lacks {missing}")
    for n in DENSIFY_GROUPS:
        if not params[n].is_cuda:
            raise RuntimeError(f"parameter {n!r} is on {params[n].device}: densify_and_prune has no CPU path (tensors must "
                               "live on a HIP device)")
    dev = params["xyz"].device
    N = params["xyz"].shape[0]
    if noise is None:
        noise = torch.randn((N, 2, 3), dtype=torch.float32, device=dev, generator=generator)
    f32 = np.float32
    counts_dev, workspace = _C.densify_plan(
        grad_accum, denom, params["scaling"].detach(), params["opacity"].detach(), grad_threshold=grad_threshold,
        min_opacity=min_opacity, dense_limit=f32(percent_dense) * f32(extent), world_limit=f32(0.1) * f32(extent),
        prune_world_size=bool(prune_world_size))
    counts = tuple(int(c) for c in counts_dev.tolist())  # the one host read
    N_out = counts[3]
    by_name = {g["name"]: g for g in optimizer.param_groups} if optimizer is not None else {}
    groups, fresh = [], {}
    for n in DENSIFY_GROUPS:
        old = params[n]
        if optimizer is not None and (n not in by_name or by_name[n]["params"][0] is not old):
            raise RuntimeError(f"densify_and_prune: params[{n!r}] is not the parameter of the optimizer's group {n!r}")
        state = optimizer.state.get(old) if optimizer is not None else None
        moments = state is not None and "exp_avg" in state
        shape = (N_out,) + tuple(old.shape[1:])
        new = torch.empty(shape, dtype=torch.float32, device=dev)
        src = (old.detach(), state["exp_avg"] if moments else None, state["exp_avg_sq"] if moments else None)
        dst = (new, torch.empty_like(new) if moments else None, torch.empty_like(new) if moments else None)
        groups.append({"src": src, "dst": dst, "M": math.prod(old.shape[1:]), "role": n if n in ("xyz", "scaling") else "copy"})
        fresh[n] = dst
    parent = torch.empty((N_out,), dtype=torch.int32, device=dev)
    _C.densify_apply(N, N_out, workspace, params["xyz"].detach(), params["scaling"].detach(), params["rotation"].detach(),
                     noise, groups, parent)
    out = {}
    for n in DENSIFY_GROUPS:
        old, (new, m, v) = params[n], fresh[n]
        prm = torch.nn.Parameter(new.requires_grad_(True))
        if optimizer is not None:
            state = optimizer.state.pop(old, None)
            by_name[n]["params"][0] = prm
            if state is not None:
                if m is not None:
                    state["exp_avg"], state["exp_avg_sq"] = m, v
                optimizer.state[prm] = state
        out[n] = prm
    return out, counts, parent
