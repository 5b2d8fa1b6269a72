"""gsr_backward against the backward oracle where tests/test_backward_gpu.py does not go: a rotated, off-origin camera
with unequal fields of view, every SH layout (the three variants of sh_backward_kernel), Gaussian counts around the
workgroup and float4 boundaries, the raw parameter space, precomputed colours / covariances -- all on gradient buffers
the test owns, filled with NaN between guard floats, so that "the kernels write every element" is asserted.

Scenes: ``helpers_bwd.edge_scene`` (what they hold is asserted on the CPU by tests/test_backward_scenes_cpu.py); the
oracle is pinned on them against float64 autograd by tests/test_backward_oracle.py.

Tolerance: ``helpers_bwd.SUITE_TOLERANCES`` for every case -- 99.95 % of a gradient's entries within 2e-3 relative (+1e-3
of the tensor's largest entry as the floor), the worst entry within 5e-3.  Zeros (rows of culled Gaussians, SH
coefficients above the active degree) and the floats around the arrays are compared as bits.  No entry is left out.
The last test prints the worst normalised error of every case (profiles/backward_edges/worst_errors.txt)."""
import numpy as np
import pytest

from tests import helpers_bwd as hb

pytestmark = pytest.mark.gpu

# name -> (M, split, SH arrays this many floats past a 16-byte boundary); the variant of sh_backward_kernel it takes
LAYOUTS = {
    "packed16": (16, False, 0),       # <48>
    "split16": (16, True, 0),         # <45>
    "packed1": (1, False, 0),         # <0> from here on
    "packed4": (4, False, 0),
    "packed9": (9, False, 0),
    "split4": (4, True, 0),
    "split9": (9, True, 0),
    "packed16_misaligned": (16, False, None),  # (None: 1, 2 or 3 floats, by degree / size)
    "split16_misaligned": (16, True, None),
}
MAX_DEGREE = {1: 0, 4: 1, 9: 2, 16: 3}
ARRANGEMENTS = ("arena", "scattered")
TAIL_SIZES = (1, 2, 3, 255, 256, 257, 515, 1022, 2049)


def run(cuda_device, case, layout="packed16", arrangement="arena", misalign=1, label=None, seed=0, raw=False):
    M, split, mis = LAYOUTS[layout]
    mis = misalign if mis is None else mis
    got, visible, R, color = hb.gsr_backward_owned(
        case, cuda_device, split=split, arrangement=arrangement, sh_misalign=mis, seed=seed,
        param_space=7 if raw else 0, raw_params=case["raw_params"] if raw else None)
    assert R == case["fwd"]["binning"]["num_rendered"]
    assert np.abs(color - case["fwd"]["color"]).max() < 1e-3
    return hb.check_owned(case, got, visible, split=split, label=label, ref=case["ref_raw"] if raw else None,
                          **hb.SUITE_TOLERANCES)


# ---- 1. rotated camera, canonical parameter space ----------------------------------------------------------------------
@pytest.mark.parametrize("scale_modifier", [1.0, 0.7])
@pytest.mark.parametrize("with_invdepth", [True, False])
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("W,H", hb.IMAGE_SIZES)
def test_rotated_camera(cuda_device, request, W, H, aa, with_invdepth, scale_modifier):
    """All eight gradients.  dL_dscales is the oracle's as it stands: both sides follow upstream's convention (the
    derivative with respect to scale_modifier * scale; tests/test_backward_oracle.py pins it against autograd)."""
    case = hb.edge_case(3000, W, H, aa=aa, scale_modifier=scale_modifier, with_invdepth=with_invdepth)
    rep = run(cuda_device, case, label=request.node.name)
    assert set(rep) == set(hb.GRAD_NAMES)


@pytest.mark.parametrize("aa", [False, True])
def test_rotated_camera_many_staging_rounds(cuda_device, request, aa):
    rep = run(cuda_device, hb.edge_case(3000, 48, 32, aa=aa, deep=True), label=request.node.name)
    assert set(rep) == set(hb.GRAD_NAMES)


# ---- 2. + 4. every SH layout at every active degree, on poisoned buffers in both arrangements ----------------------------
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("layout,deg", [(name, d) for name, (M, _, _) in LAYOUTS.items() for d in range(MAX_DEGREE[M] + 1)])
def test_sh_layouts(cuda_device, request, layout, deg, arrangement):
    case = hb.edge_case(3000, 48, 32, deg=deg, M=LAYOUTS[layout][0])
    rep = run(cuda_device, case, layout, arrangement, misalign=1 + deg % 3, label=request.node.name, seed=deg)
    assert "dL_dsh" in rep and ("dL_dsh_rest" in rep) == (LAYOUTS[layout][1] and deg > 0)


# ---- 3. + 4. Gaussian counts around the workgroup (256) and float4 boundaries ---------------------------------------------
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("layout", ["split16", "packed16", "split9", "packed4", "packed16_misaligned", "split16_misaligned"])
@pytest.mark.parametrize("P", TAIL_SIZES)
def test_gaussian_count_tails(cuda_device, request, P, layout, arrangement):
    """P mod 4 takes every value, P mod 256 is 0, 1 and 255 among others: the last workgroup's tail loads and stores of
    sh_backward_kernel<45> (P * 45 floats is a multiple of 4 only when P is), the per-thread bound of every kernel, and
    -- through the guard floats -- a store past the end."""
    M = LAYOUTS[layout][0]
    case = hb.edge_case(P, 48, 32, deg=MAX_DEGREE[M], M=M)
    run(cuda_device, case, layout, arrangement, misalign=1 + P % 3, label=request.node.name, seed=P)


# ---- 4. nothing to render, and the NULL gradient pointers of precomputed inputs -------------------------------------------
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("layout", ["packed16", "split16", "split9", "packed16_misaligned"])
@pytest.mark.parametrize("P", [257, 1024])
def test_every_gaussian_culled(cuda_device, P, layout, arrangement):
    """num_rendered == 0 with P > 0: no kernel runs, every gradient comes back zero through gsr_backward's memsets --
    adjacent arrays fused into one (the arena: all of them when P is a multiple of 4) or one per array (scattered)."""
    M = LAYOUTS[layout][0]
    case = hb.edge_case(P, 48, 32, deg=MAX_DEGREE[M], M=M, all_culled=True)
    assert not case["visible"].any() and case["fwd"]["binning"]["num_rendered"] == 0
    rep = run(cuda_device, case, layout, arrangement, misalign=3)
    assert rep == {}  # (compare_grads: every reference gradient is all-zero, and so was every result)


# ---- 6. precomputed colours and covariances -----------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("W,H", [(48, 32), (17, 9)])
def test_precomputed_colors_and_cov(cuda_device, request, W, H, arrangement):
    """Under the rotated camera, with antialiasing and dL_dinvdepth; dL_dsh / dL_dscales / dL_drots are NULL."""
    case = hb.edge_case(3000, W, H, aa=True, precomp=True)
    rep = run(cuda_device, case, arrangement=arrangement, label=request.node.name)
    assert set(rep) == {"dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D"}


# ---- 5. raw parameter space against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True])
@pytest.mark.parametrize("layout", ["split16", "split4"])
def test_raw_parameter_space(cuda_device, request, layout, aa):
    """param_space = 7 with split SH: raw opacity logits, log scales and quaternions of length 0.2 to 5 go in, the gradients
    come back with respect to them.  Reference: the oracle on the canonical float32 activations, then the chain rule in
    binary64 (``helpers_bwd.edge_case``) -- not the GPU's own canonical path."""
    M = LAYOUTS[layout][0]
    case = hb.edge_case(3000, 48, 32, aa=aa, deg=MAX_DEGREE[M], M=M, raw_space=True)
    lengths = np.linalg.norm(case["raw_params"][2], axis=1)
    assert lengths.min() < 0.3 and lengths.max() > 4.0
    rep = run(cuda_device, case, layout, label=request.node.name, raw=True)
    assert {"dL_dopacity", "dL_dscales", "dL_drotations", "dL_dsh", "dL_dsh_rest"} <= set(rep)


def test_worst_errors():
    """(Runs last: prints what the cases above observed.)"""
    for label in sorted(hb.WORST):
        err, name = hb.WORST[label]
        print(f"{label}: worst normalised error {err:.2e} ({name})")
    assert all(err <= hb.SUITE_TOLERANCES["max_norm_err"] for err, _ in hb.WORST.values())
