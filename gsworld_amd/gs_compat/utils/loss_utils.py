"""``utils.loss_utils`` of the 3DGS python layer: the pieces upstream's train.py composes its loss from.  ``ssim`` is this
package's ``fused_ssim`` (the HIP kernels of gsworld_amd/csrc/ssim.hip); the whole loss as one node is
``gsworld_amd.ssim.training_loss``."""
import torch


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def l2_loss(network_output, gt):
    return ((network_output - gt) ** 2).mean()


def ssim(img1, img2, window_size=11, size_average=True):
    from gsworld_amd.ssim import fused_ssim

    if window_size != 11 or not size_average:
        raise NotImplementedError("ssim: the 11 x 11 window and the mean are what the HIP kernels compute")
    if img1.dim() == 3:
        img1, img2 = img1[None], img2[None]
    return fused_ssim(img1, img2)
