"""``utils.general_utils`` helpers of the 3DGS python layer that GaussianModel needs."""
import torch


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def build_rotation(r):
    q = r / r.norm(dim=1, keepdim=True)
    w, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def build_scaling_rotation(s, r):
    return build_rotation(r) * s[:, None, :]


def strip_symmetric(L):
    return torch.stack((L[:, 0, 0], L[:, 0, 1], L[:, 0, 2], L[:, 1, 1], L[:, 1, 2], L[:, 2, 2]), 1)


def PILtoTorch(pil_image, resolution):
    import numpy as np

    resized = pil_image.resize(resolution)
    img = torch.from_numpy(np.array(resized)) / 255.0
    return img.permute(2, 0, 1) if img.dim() == 3 else img.unsqueeze(-1).permute(2, 0, 1)


def get_expon_lr_func(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """Upstream's schedule: log-linear from ``lr_init`` (step 0) to ``lr_final`` (step ``max_steps``), optionally eased in
    over the first ``lr_delay_steps`` steps from ``lr_delay_mult`` times the value; 0 before step 0 and when both ends are 0."""
    import numpy as np

    def helper(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        if lr_delay_steps > 0:
            delay_rate = lr_delay_mult + (1 - lr_delay_mult) * np.sin(0.5 * np.pi * np.clip(step / lr_delay_steps, 0, 1))
        else:
            delay_rate = 1.0
        t = np.clip(step / max_steps, 0, 1)
        return delay_rate * np.exp(np.log(lr_init) * (1 - t) + np.log(lr_final) * t)

    return helper


def safe_state(silent):
    """Seeds python, numpy and torch with 0; with ``silent`` the training script's prints are dropped (upstream stamps
    them with the time instead: not reproduced)."""
    import random
    import sys

    import numpy as np

    if silent:
        class _Quiet:
            def __init__(self, out):
                self._out = out

            def write(self, s):
                pass

            def flush(self):
                self._out.flush()

        sys.stdout = _Quiet(sys.stdout)
    random.seed(0)
    np.random.seed(0)
    torch.manual_seed(0)
    if torch.cuda.is_available():
        torch.cuda.set_device(torch.device("cuda:0"))
