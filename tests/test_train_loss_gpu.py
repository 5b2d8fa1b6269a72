"""``gsworld_amd.ssim.training_loss`` (gsr_train_loss / gsr_train_loss_backward, include/gsr.h) against binary64 autograd of
its definition -- exposure affine, clamp, alpha mask, L1 + ssim (oracle/ssim_ref.py) and the inverse-depth term -- on the
smallest shapes at which it can go wrong: one ssim window (16 x 16), an odd size that is no multiple of any tile (37 x 53),
several workgroups of every kernel (64 x 80).

Tolerances are those ``photometric_loss`` is held to (tests/test_knn_ssim_gpu.py): the value within 2e-6, an image gradient
within 2e-5 of the reference's largest entry; each of the twelve exposure gradients -- a sum over pixels of terms that each
carry the image-gradient tolerance -- within 2e-5 of the reference's sum of the absolute per-pixel contributions to it."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import ssim_ref

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (37, 53), (64, 80)]
LAM = 0.2
DEPTH_WEIGHT = 0.7
GUARD, SENTINEL = 64, -7.25


def make_inputs(H, W, exposure, alpha, depth, seed=0):
    """CPU float32 inputs: the image leaves [0, 1] in places, sits exactly on 0 and 1 in others and equals the target in
    others; a non-identity exposure pushes further pixels over the clamp; alpha and depth_mask have exact zeros;
    invdepth == mono at some pixels."""
    gen = torch.Generator().manual_seed(1000 * H + W + seed)
    t = torch.rand(3, H, W, generator=gen)
    img = t + 0.2 * torch.randn(3, H, W, generator=gen)
    img.view(-1)[::7] = t.view(-1)[::7]
    img.view(-1)[3::11] = 1.0
    img.view(-1)[5::13] = 0.0
    d = {"color": img, "target": t}
    if exposure:
        E = torch.tensor([[1.10, 0.05, -0.03, 0.02], [-0.04, 0.90, 0.06, -0.01], [0.03, -0.02, 1.20, 0.04]])
        d["exposure"] = E
    if alpha:
        a = torch.rand(1, H, W, generator=gen)
        a.view(-1)[::5] = 0.0
        a.view(-1)[1::9] = 1.0
        d["alpha_mask"] = a
    if depth:
        inv = torch.rand(1, H, W, generator=gen) + 0.1
        mono = inv + 0.3 * torch.randn(1, H, W, generator=gen)
        mono.view(-1)[::6] = inv.view(-1)[::6]
        m = (torch.rand(1, H, W, generator=gen) > 0.3).float()
        m.view(-1)[2::4] = 0.0
        d.update(invdepth=inv, mono_invdepth=mono, depth_mask=m)
    return d


def reference(d, lam=LAM, depth_weight=DEPTH_WEIGHT, grad_loss=2.0):
    """binary64 autograd of the definition.  -> value, terms (4), gradients, the clamp's gate, and for the exposure the
    sum over pixels of the absolute per-pixel contributions to each entry."""
    color = d["color"].double().requires_grad_(True)
    t = d["target"].double()
    E = d["exposure"].double().requires_grad_(True) if "exposure" in d else None
    if E is not None:
        y = torch.matmul(color.permute(1, 2, 0), E[:3, :3]).permute(2, 0, 1) + E[:3, 3, None, None]
    else:
        y = color
    y.retain_grad()
    x = y.clamp(0, 1)
    if "alpha_mask" in d:
        x = x * d["alpha_mask"].double()
    l1 = (x - t).abs().mean()
    ss = ssim_ref.ssim(x[None], t[None], "same")
    total = (1 - lam) * l1 + lam * (1 - ss)
    inv = None
    dl1 = torch.zeros((), dtype=torch.float64)
    if "invdepth" in d:
        inv = d["invdepth"].double().requires_grad_(True)
        dl1 = ((inv - d["mono_invdepth"].double()) * d["depth_mask"].double()).abs().mean()
        total = total + depth_weight * dl1
    (grad_loss * total).backward()
    parts = [float(v.detach()) for v in (total, l1, ss, dl1)]
    out = {"value": parts[0], "terms": parts, "dcolor": color.grad,
           "dinv": inv.grad if inv is not None else None, "dexp": E.grad if E is not None else None,
           "outside": ((y < 0) | (y > 1)).detach()}
    if E is not None:
        gy = y.grad  # (3,H,W): dL/dy, zero outside the clamp
        scale = torch.zeros(3, 4, dtype=torch.float64)
        for i in range(3):
            for c in range(3):
                scale[i, c] = (color.detach()[i] * gy[c]).abs().sum()
            scale[i, 3] = gy[i].abs().sum()
        out["dexp_scale"] = scale
    return out


_REF = {}


def case(H, W, exposure, alpha, depth):
    """The inputs and their reference, computed once per case and shared (never modified)."""
    key = (H, W, exposure, alpha, depth)
    if key not in _REF:
        d = make_inputs(H, W, exposure, alpha, depth)
        _REF[key] = (d, reference(d))
    return _REF[key]


def run(d, dev, lam=LAM, depth_weight=DEPTH_WEIGHT, grad_loss=2.0, backward=True):
    from gsworld_amd.ssim import training_loss

    g = {k: v.to(dev) for k, v in d.items()}
    for k in ("color", "exposure", "invdepth"):
        if k in g and backward:
            g[k].requires_grad_(True)
    loss = training_loss(g["color"], g["target"], lam, exposure=g.get("exposure"), alpha_mask=g.get("alpha_mask"),
                         invdepth=g.get("invdepth"), mono_invdepth=g.get("mono_invdepth"), depth_mask=g.get("depth_mask"),
                         depth_weight=depth_weight if "invdepth" in g else 0.0)
    if backward:
        (grad_loss * loss).backward()
    return loss, g


@pytest.mark.parametrize("exposure,alpha,depth", list(itertools.product([False, True], repeat=3)))
@pytest.mark.parametrize("shape", SHAPES)
def test_training_loss_against_binary64_autograd(cuda_device, shape, exposure, alpha, depth):
    H, W = shape
    d, ref = case(H, W, exposure, alpha, depth)
    loss, g = run(d, cuda_device)
    terms = loss.terms.cpu().double()
    g_color = g["color"].grad.cpu().double()
    err_c = float((g_color - ref["dcolor"]).abs().max())
    print(f"value {float(loss):.9f} want {ref['value']:.9f}; dcolor err {err_c:.3e} of max {float(ref['dcolor'].abs().max()):.3e}")
    assert loss.shape == () and abs(float(loss) - ref["value"]) < 2e-6
    assert loss.terms.is_cuda and float(terms[0]) == float(loss)
    for k in (1, 2, 3):
        assert abs(float(terms[k]) - ref["terms"][k]) < 2e-6, k
    assert err_c <= 2e-5 * float(ref["dcolor"].abs().max())
    # the clamp stops the gradient outside [0, 1]: with an exposure every input channel feeds a stopped output channel, so
    # the exact zeros are those of the pixels whose three outputs are all outside; without one, channel by channel
    out = ref["outside"]
    dead = out.all(0, keepdim=True).expand_as(out) if exposure else out
    if alpha:
        zero_a = (d["alpha_mask"] == 0).expand_as(out)
        assert zero_a.any()
        dead = dead | zero_a
    assert out.any()
    if dead.any():
        assert float(g_color[dead].abs().max()) == 0.0
    if depth:
        g_inv = g["invdepth"].grad.cpu().double()
        err_d = float((g_inv - ref["dinv"]).abs().max())
        print(f"dinvdepth err {err_d:.3e} of max {float(ref['dinv'].abs().max()):.3e}")
        assert err_d <= 2e-5 * float(ref["dinv"].abs().max())
        off = (d["depth_mask"] == 0) | (d["invdepth"] == d["mono_invdepth"])
        assert (d["depth_mask"] == 0).any() and (d["invdepth"] == d["mono_invdepth"]).any()
        assert float(g_inv[off].abs().max()) == 0.0
    if exposure:
        g_e = g["exposure"].grad.cpu().double()
        assert g_e.shape == (3, 4)
        err_e = (g_e - ref["dexp"]).abs()
        print("dexposure err / scale:", (err_e / ref["dexp_scale"]).max().item())
        assert bool((err_e <= 2e-5 * ref["dexp_scale"]).all())


@pytest.mark.parametrize("shape", SHAPES)
def test_plain_and_identity_exposure_are_photometric_loss_bit_for_bit(cuda_device, shape):
    from gsworld_amd.ssim import photometric_loss

    H, W = shape
    d, _ = case(H, W, False, False, False)
    x = d["color"].to(cuda_device).requires_grad_(True)
    want = photometric_loss(x, d["target"].to(cuda_device), LAM, clamp01=True)
    (2.0 * want).backward()
    loss, g = run(d, cuda_device)
    assert torch.equal(loss.detach(), want.detach()) and torch.equal(g["color"].grad, x.grad)
    ident = dict(d, exposure=torch.eye(3, 4))
    loss_i, g_i = run(ident, cuda_device)
    assert torch.equal(loss_i.detach(), want.detach()) and torch.equal(g_i["color"].grad, x.grad)


@pytest.mark.parametrize("shape", SHAPES)
def test_dead_depth_term_gives_the_depth_free_bits(cuda_device, shape):
    H, W = shape
    d, _ = case(H, W, True, True, True)
    free = {k: v for k, v in d.items() if k not in ("invdepth", "mono_invdepth", "depth_mask")}
    want, gw = run(free, cuda_device)
    for variant in (dict(d, depth_mask=torch.zeros_like(d["depth_mask"])), None):
        if variant is None:
            loss, g = run(d, cuda_device, depth_weight=0.0)
        else:
            loss, g = run(variant, cuda_device)
        assert torch.equal(loss.detach(), want.detach())
        assert torch.equal(g["color"].grad, gw["color"].grad) and torch.equal(g["exposure"].grad, gw["exposure"].grad)
        assert float(g["invdepth"].grad.abs().max()) == 0.0


def test_two_calls_give_identical_bits(cuda_device):
    d, _ = case(37, 53, True, True, True)
    a, ga = run(d, cuda_device)
    b, gb = run(d, cuda_device)
    assert torch.equal(a.detach(), b.detach()) and torch.equal(a.terms, b.terms)
    for k in ("color", "exposure", "invdepth"):
        assert torch.equal(ga[k].grad, gb[k].grad), k


def _carve(n, dev, fill=None):
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[GUARD:GUARD + n]
    if fill is not None:
        view.copy_(fill.reshape(-1))
    return view, buf


def _intact(buf, n):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == np.float32(SENTINEL)).all() and (b[GUARD + n:] == np.float32(SENTINEL)).all())


@pytest.mark.parametrize("binding", ["ctypes", "ext"])
def test_guards_intact_and_both_bindings(cuda_device, binding):
    """Every buffer of a call carved with 64 guard floats on each side (the scratch included): guards come back intact, and
    the outputs are those of ``training_loss``, through either binding."""
    from gsworld_amd import _C

    H, W = 37, 53
    d, _ = case(H, W, True, True, True)
    want, gw = run(d, cuda_device, grad_loss=1.0)
    dev = torch.device(cuda_device)
    ins = {k: _carve(v.numel(), dev, v.to(dev)) for k, v in d.items()}
    nf = _C.train_loss_scratch_floats(H, W)
    outs = {"scratch": _carve(nf, dev), "loss": _carve(1, dev), "terms": _carve(4, dev), "dcolor": _carve(3 * H * W, dev),
            "dinv": _carve(H * W, dev), "dexp": _carve(12, dev)}
    p = lambda k: (ins.get(k) or outs[k])[0].data_ptr()  # noqa: E731
    vals = [H, W, LAM, p("color"), p("target"), p("exposure"), p("alpha_mask"), p("invdepth"), p("mono_invdepth"),
            p("depth_mask"), DEPTH_WEIGHT, 1, p("scratch"), nf, p("loss"), p("terms"), 0, 0, 0, 0]
    _C.train_loss(vals, dev, binding=binding)
    vals[17:20] = [p("dcolor"), p("dinv"), p("dexp")]
    _C.train_loss(vals, dev, backward=True, binding=binding)
    for k, (view, buf) in {**ins, **outs}.items():
        assert _intact(buf, view.numel()), k
    for k, v in d.items():
        assert torch.equal(ins[k][0].cpu(), v.reshape(-1)), f"{k} is read-only"
    assert torch.equal(outs["loss"][0][0], want.detach()) and torch.equal(outs["terms"][0], want.terms)
    assert torch.equal(outs["dcolor"][0], gw["color"].grad.reshape(-1))
    assert torch.equal(outs["dinv"][0], gw["invdepth"].grad.reshape(-1))
    assert torch.equal(outs["dexp"][0], gw["exposure"].grad.reshape(-1))


def test_refusals(cuda_device):
    from gsworld_amd.ssim import training_loss

    t = torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training_loss(t, t)
    g = t.to(cuda_device)
    with pytest.raises(RuntimeError, match="no CPU path"):
        training_loss(g, g, alpha_mask=torch.ones(1, 16, 16))
    with pytest.raises(RuntimeError, match="together"):
        training_loss(g, g, invdepth=g[:1])
    with pytest.raises(RuntimeError, match="shape"):
        training_loss(g, g, alpha_mask=g)
    # no gradient asked for: the forward alone
    assert training_loss(g, g).shape == ()
