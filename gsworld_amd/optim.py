"""The optimizer side of a training iteration on the device: ``SparseGaussianAdam`` -- the sparse Adam of upstream's
``3dgs_accel`` rasterizer (``adamUpdateCUDA``) -- and the densification statistics, both without the
``(radii > 0).nonzero()`` compaction and host read upstream's loop does every iteration.

    forward -> photometric_loss -> backward -> densification_stats(radii, ...) -> optimizer.step(radii, N)

The optimizer lives HERE, not in the drop-in ``diff_gaussian_rasterization`` package: GSWorld probes that package for the
name to pick its ``separate_sh`` call signature (gs_world_wrapper.py:22-26), which this project does not offer.  A training
script imports it from ``gsworld_amd.optim``.
"""
from __future__ import annotations

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
