"""Pins the backward oracle (gso_render_backward + gso_preprocess_backward): its gradients must equal torch
autograd (float64) through the independently written PyTorch restatement of the forward pass."""
import numpy as np
import pytest
import torch

from gsworld_amd import scenes
from oracle import gs_oracle as go
from oracle import torch_cpu_render as tcr
from tests import helpers as hp
from tests import helpers_bwd as hb


@pytest.mark.parametrize("aa,deg", [(False, 3), (True, 3), (False, 1)])
def test_backward_oracle_matches_float64_autograd(aa, deg):
    n, W, H = 300, 48, 32
    raw = scenes.random_scene_camera_frame(n, seed=31, near_fraction=0.0)
    raw.scaling += 0.7  # larger splats: every pixel blends several Gaussians
    cam = scenes.identity_camera(W, H, 60.0)
    inp = hp.np_inputs(raw, cam)
    st = hp.oracle_settings(cam, antialiasing=aa, sh_degree=deg)
    bg = np.float32([0.3, 0.1, 0.6])
    fwd = hp.oracle_forward(inp, st, bg, border_eps=0.0)
    gen = torch.Generator().manual_seed(1)
    dLc = torch.randn(3, H, W, generator=gen)
    dLd = torch.randn(1, H, W, generator=gen)
    gr = go.backward(st, fwd, inp, bg, dLc.numpy(), dLd.numpy())
    means, shs, op, sc, rot = [t.double().requires_grad_(True) for t in raw.activated()]
    out = tcr.render(means, shs, op, sc, rot, cam.world_view_transform.double(), cam.full_proj_transform.double(),
                     cam.camera_center.double(), torch.from_numpy(bg).double(), H, W, cam.tanfovx, cam.tanfovy,
                     sh_degree=deg, antialiasing=aa)
    assert float((out["color"].detach().float() - torch.from_numpy(fwd["color"])).abs().max()) < 1e-5
    ((out["color"] * dLc.double()).sum() + (out["invdepth"] * dLd.double()).sum()).backward()
    for name, t, g in (("means3D", means, gr["dL_dmeans3D"]), ("sh", shs, gr["dL_dsh"]),
                       ("opacity", op, gr["dL_dopacity"]), ("scales", sc, gr["dL_dscales"]),
                       ("rotations", rot, gr["dL_drotations"])):
        ref = t.grad.numpy().reshape(g.shape)
        scale = np.abs(ref).max()
        assert scale > 0, name
        err = np.abs(ref - g) / (np.abs(ref) + 1e-3 * scale)
        assert err.max() < 2e-3, (name, err.max())
        assert np.median(err) < 1e-5, (name, np.median(err))


def _autograd_reference(raw, cam, inp, st, bg, fwd, dLc, dLd):
    """float64 autograd through oracle/torch_cpu_render.py of sum(color * dLc) + sum(invdepth * dLd)."""
    M, H, W = st.sh_coeffs, st.image_height, st.image_width
    means, shs, op, sc, rot = [t.double() for t in raw.activated()]
    leaves = [t.contiguous().requires_grad_(True) for t in (means, shs[:, :M], op, sc, rot)]
    out = tcr.render(*leaves, cam.world_view_transform.double(), cam.full_proj_transform.double(),
                     cam.camera_center.double(), torch.from_numpy(bg).double(), H, W, cam.tanfovx, cam.tanfovy,
                     sh_degree=st.sh_degree, scale_modifier=st.scale_modifier, antialiasing=st.antialiasing)
    assert float((out["color"].detach().float() - torch.from_numpy(fwd["color"])).abs().max()) < 1e-5
    assert torch.equal(out["radii"] > 0, torch.from_numpy(fwd["geom"]["radii"] > 0))
    loss = (out["color"] * torch.from_numpy(dLc).double()).sum() + (out["invdepth"] * torch.from_numpy(dLd).double()).sum()
    loss.backward()
    return dict(zip(("means3D", "sh", "opacity", "scales", "rotations"), (t.grad.numpy() for t in leaves)))


def _normalised_errors(ref, got):
    ref = ref.reshape(got.shape)
    scale = np.abs(ref).max()
    assert scale > 0
    return np.abs(ref - got) / (np.abs(ref) + 1e-3 * scale)


@pytest.mark.parametrize("scale_modifier", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("M,deg", [(16, 3), (16, 1), (9, 2), (4, 1), (4, 0), (1, 0)])
def test_backward_oracle_under_a_rotated_camera(M, deg, aa, scale_modifier):
    """The same pin where tests/test_backward_edges_gpu.py leans on the oracle: the rotated, off-origin camera with
    unequal fields of view of ``helpers_bwd.rotated_camera``, every SH layout size with ``shs[:, :M]`` and
    ``sh_coeffs = M``, antialiasing, and ``scale_modifier`` != 1, on ``helpers_bwd.edge_scene`` (culled Gaussians,
    clamped colours, saturated pixels) without the two kinds of Gaussian for which upstream's backward is not the
    derivative autograd computes (``upstream_branches`` there).

    dL_dscales: the oracle follows upstream's convention (oracle/gs_oracle.c) -- its value is the derivative with
    respect to ``scale_modifier * scale``, NOT multiplied by ``scale_modifier`` -- whereas autograd differentiates with
    respect to the ``scales`` tensor itself.  So ``oracle * scale_modifier`` is compared with autograd, and the
    un-multiplied value is asserted to be off by the factor: a "fix" of the convention on either side alone fails here."""
    n, W, H = 384, 48, 32
    case = hb.edge_case(n, W, H, aa=aa, deg=deg, M=M, scale_modifier=scale_modifier, upstream_branches=False)
    gr = case["ref"]
    ref = _autograd_reference(case["raw"], case["cam"], case["inp"], case["st"], case["bg"], case["fwd"], case["dLc"],
                              case["dLd"])
    for name, g in (("means3D", gr["dL_dmeans3D"]), ("sh", gr["dL_dsh"]), ("opacity", gr["dL_dopacity"]),
                    ("scales", gr["dL_dscales"] * np.float32(scale_modifier)), ("rotations", gr["dL_drotations"])):
        err = _normalised_errors(ref[name], g)
        assert err.max() < 2e-3, (name, err.max())
        assert np.median(err) < 1e-5, (name, np.median(err))
    assert not gr["dL_dsh"][:, (deg + 1) ** 2:].any() and not ref["sh"][:, (deg + 1) ** 2:].any()
    if scale_modifier != 1.0:
        # without the factor every entry is off by 1 / scale_modifier - 1 (relative to autograd's value)
        big = np.abs(ref["scales"]) > 1e-2 * np.abs(ref["scales"]).max()
        ratio = gr["dL_dscales"].astype(np.float64)[big] / ref["scales"][big]
        assert np.abs(ratio - 1.0 / scale_modifier).max() < 5e-3, (ratio.min(), ratio.max())
        assert _normalised_errors(ref["scales"], gr["dL_dscales"]).max() > 0.2
