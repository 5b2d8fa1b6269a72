"""Appearance randomization without a GPU: the op algebra of gsworld_amd.appearance, the seeded randomizer, the NumPy
restatement of the kernel's colour contract, the loop's argument checks and the GsrInputs layout against include/gsr.h."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from gsworld_amd import _lib
from gsworld_amd import appearance as ap
from gsworld_amd import closed_loop as cl
from gsworld_amd import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C3 = np.random.default_rng(0).uniform(0.0, 1.0, size=(50, 3))


def _apply64(A, c):
    return c @ np.asarray(A)[:, :3].T + np.asarray(A)[:, 3]


def test_op_algebra():
    assert np.array_equal(ap.identity(), np.eye(3, 4))
    assert np.allclose(_apply64(ap.brightness(1.5), C3), 1.5 * C3)
    assert np.allclose(_apply64(ap.contrast(2.0), np.full((1, 3), 0.5)), 0.5)
    assert np.allclose(_apply64(ap.gain((1, 2, 3)), C3), C3 * [1, 2, 3])
    # compose applies left to right
    a, b = ap.brightness(2.0), ap.contrast(0.5)
    assert np.allclose(_apply64(ap.compose(a, b), C3), _apply64(b, _apply64(a, C3)))
    assert not np.allclose(_apply64(ap.compose(a, b), C3), _apply64(a, _apply64(b, C3)))
    # saturation 0: the luma on every channel
    luma = C3 @ np.array(ap.LUMA)
    assert np.allclose(_apply64(ap.saturation(0.0), C3), luma[:, None].repeat(3, 1))
    assert np.allclose(_apply64(ap.saturation(1.0), C3), C3)
    # hue: 2 pi / 3 cycles the channels, grey and the channel sum stay
    assert np.allclose(_apply64(ap.hue(2 * math.pi / 3), C3), C3[:, [2, 0, 1]])
    for th in (0.3, -1.1, 2.5):
        H = _apply64(ap.hue(th), C3)
        assert np.allclose(H.sum(1), C3.sum(1))
        assert np.allclose(_apply64(ap.hue(th), np.full((1, 3), 0.37)), 0.37)


def test_randomizer_is_seeded_and_respects_its_ranges():
    kw = dict(brightness=(0.5, 1.5), background=((0.1, 0.2, 0.3), (0.2, 0.4, 0.6)), seed=5)
    t1, b1 = ap.AppearanceRandomizer(3, **kw).sample(4)
    t2, b2 = ap.AppearanceRandomizer(3, **kw).sample(4)
    t3, _ = ap.AppearanceRandomizer(3, **{**kw, "seed": 6}).sample(4)
    assert t1.shape == (4, 3, 3, 4) and t1.dtype == np.float32 and b1.shape == (4, 3) and b1.dtype == np.float32
    assert np.array_equal(t1, t2) and np.array_equal(b1, b2) and not np.array_equal(t1, t3)
    # brightness only: b I with b in range, no offset
    diag = t1[..., [0, 1, 2], [0, 1, 2]]
    assert np.all(diag >= 0.5 - 1e-6) and np.all(diag <= 1.5 + 1e-6)
    assert np.allclose(diag, diag[..., :1]) and np.all(t1[..., 3] == 0)
    assert np.all(b1 >= [0.1, 0.2, 0.3]) and np.all(b1 <= [0.2, 0.4, 0.6])
    # per_group=False: one draw for every group of an environment
    t4, _ = ap.AppearanceRandomizer(3, hue=(-1, 1), per_group=False, seed=1).sample(2)
    assert np.array_equal(t4[:, 0], t4[:, 2]) and not np.array_equal(t4[0], t4[1])
    with pytest.raises(ValueError):
        ap.AppearanceRandomizer(3, brightness=(2.0, 1.0))
    with pytest.raises(ValueError):
        ap.AppearanceRandomizer(0)


def test_restatement_of_the_colour_contract():
    T = np.array([[1.5, -0.25, 0.1, -0.2], [0.0, 1.0, 0.0, 0.0], [0.3, 0.3, 0.3, -0.5]], np.float32)
    c = np.array([[0.2, 0.4, 0.6], [0.0, 0.0, 0.0], [1.0, 0.5, 0.25]], np.float32)
    got = ap.apply_table(T, c)
    assert got.dtype == np.float32
    for i in range(3):
        for j in range(3):
            x = np.float32(np.float32(np.float32(np.float32(T[j, 0] * c[i, 0]) + np.float32(T[j, 1] * c[i, 1])) +
                                      np.float32(T[j, 2] * c[i, 2])) + T[j, 3])
            assert got[i, j].view(np.uint32) == np.float32(max(x, np.float32(0))).view(np.uint32)
    assert got[1, 0] == 0 and got[1, 2] == 0  # (the clamp at 0)
    # identity: bit-identical for c >= 0
    cc = np.random.default_rng(1).uniform(0, 3, size=(1000, 3)).astype(np.float32)
    assert np.array_equal(ap.apply_table(np.eye(3, 4), cc).view(np.uint32), cc.view(np.uint32))


def test_loop_argument_checks_raise_before_device_work():
    raw = scenes.tabletop_scene("xarm6_align", n=5000, seed=1)
    cams = {"c": scenes.identity_camera(64, 64)}
    for bad in ({"robot": [999]}, {"a": [1], "b": [1]}, {"a": [1.5]}, {}, {"a": []}):
        with pytest.raises(ValueError):
            cl.ClosedLoopRenderer(raw, {"link": 1}, cams, device="cpu", appearance=bad)
    with pytest.raises(ValueError):
        cl.ClosedLoopRenderer(raw, {"link": 1}, cams, device="cpu", appearance={"robot": [1]},
                              background=torch.zeros(3, 3), num_envs=2)
    with pytest.raises(ValueError, match="appearance"):
        cl.PipelinedClosedLoop(raw, {"link": 1}, cams, device="cpu", appearance={"robot": [1]})
    names, lut, G = ap.check_groups({"robot": list(range(1, 17)), "obj": [17, 18]}, raw.semantics.numpy())
    assert names == ["robot", "obj"] and G == 3 and lut[0] == 0 and lut[5] == 1 and lut[18] == 2
    t, b, ids = ap.check_tables(np.zeros((2, 3, 3, 4)), None, [0, 3], 4, 3)
    assert t.shape == (2, 3, 3, 4) and b is None and ids == [0, 3]
    for args in ((np.zeros((4, 2, 3, 4)), None, None), (np.zeros((4, 3, 3, 3)), None, None),
                 (np.zeros((1, 3, 3, 4)), None, [4]), (np.zeros((1, 3, 3, 4)), None, [-1]),
                 (np.zeros((2, 3, 3, 4)), None, [1, 1]), (np.zeros((4, 3, 3, 4)), np.zeros((4, 4)), None)):
        with pytest.raises(ValueError):
            ap.check_tables(*args, 4, 3)


def _header_fields():
    """The GsrInputs members from include/gsr.h, in order."""
    src = open(os.path.join(ROOT, "include", "gsr.h")).read()
    body = re.search(r"typedef struct GsrInputs \{(.*?)\} GsrInputs;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names.append(re.findall(r"\w+", decl)[-1])
    return names


def test_ctypes_inputs_match_the_header():
    names = [n for n, _ in _lib.GsrInputs._fields_]
    assert names == _header_fields()
    for n in ("appearance", "appearance_lut", "appearance_lut_size", "appearance_groups", "appearance_versions",
              "appearance_labels"):
        assert n in names
    # offsets as a C compiler lays them out
    prog = "#include <stdio.h>\n#include <stddef.h>\n#include \"gsr.h\"\nint main(void){\n"
    for n in names:
        prog += f'printf("%zu\\n", offsetof(GsrInputs, {n}));\n'
    prog += 'printf("%zu\\n", sizeof(GsrInputs)); return 0; }\n'
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "o.c"), os.path.join(d, "o")
        open(c, "w").write(prog)
        cc = os.environ.get("CC", "cc")
        try:
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        except (OSError, subprocess.CalledProcessError):
            pytest.fail("no host C compiler to lay out GsrInputs")
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [getattr(_lib.GsrInputs, n).offset for n in names] + [C.sizeof(_lib.GsrInputs)]
    assert got == want
