"""Point clouds (csrc/pointcloud.hip) at the shapes where the kernels' edge branches fire: views whose pixel counts end in a
partial 256-pixel block, anisotropic cameras, 64 views (the limit) with environments of 0, 1, K-1, K, K+1 and more than
fps_candidates points, fps_candidates around the 1024-thread rounds and the <8> / <16> instances, crop faces exactly on a
point and exclusion of -1 / 32767.  Held to the float32 restatement (tests/test_pointcloud_cpu.py) bit for bit, to the
binary64 unprojection (tests/ref_observations.py cloud_f64) within CROP_TOL (1 + |q|), and to fps_check in binary64."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from gsworld_amd import scenes
from gsworld_amd.camera import look_at_view
from gsworld_amd.pointcloud import PointCloudSpec, render_pointcloud, sim_from_scene
from gsworld_amd.renderer import FrameRenderer
from tests import ref_observations as ro
from tests.test_pointcloud_cpu import unproject
from tests.test_pointcloud_gpu import _against_restatement, _rigid

pytestmark = pytest.mark.gpu

F32 = np.float32
SENTINEL = dict(xyzw=-3.25, rgb=77, segmentation=555, count=-9)


def _cam(W, H, k=0):
    # anisotropic on purpose: tanfovx / tanfovy != W / H
    return look_at_view([0.05 - 0.02 * k, -0.03, 0.0], [0.0, 0.02 * k, 3.0], [0, -1, 0], 1.1, 0.55 + 0.1 * k, W, H)


def _synthetic(dev, sizes, E, seed, zero=0.1):
    gen = torch.Generator().manual_seed(seed)
    cams, depth, labels, frames = {}, {}, {}, {}
    for k, (W, H) in enumerate(sizes):
        name = f"c{k}"
        cams[name] = _cam(W, H, k)
        cams[name].world_view_transform = cams[name].world_view_transform.to(dev)
        d = 1.5 + 3.0 * torch.rand((E, H, W, 1), generator=gen)
        d[torch.rand((E, H, W, 1), generator=gen) < zero] = 0.0
        depth[name] = d.to(dev)
        labels[name] = torch.randint(-1, 24, (E, H, W, 1), generator=gen, dtype=torch.int16).to(dev)
        frames[name] = torch.randint(0, 256, (E, H, W, 3), generator=gen, dtype=torch.uint8).to(dev)
    return cams, depth, labels, frames


def _rendered(dev, sizes, ds):
    """Maps of real frames (random scene, one environment) for cameras of these sizes."""
    raw = scenes.random_scene_camera_frame(20_000, seed=5, near_fraction=0.0)
    means, shs, op, sc, rot = raw.to(dev).activated()
    labs = (torch.arange(means.shape[0], device=dev) % 997).to(torch.float32)
    cams, depth, labels = {}, {}, {}
    for k, (W, H) in enumerate(sizes):
        name = f"r{k}"
        cam = _cam(W, H, k)
        r = FrameRenderer(dev)
        r.render(cam, means, op, shs=shs, scales=sc, rotations=rot, exact=True)
        lab, dep = r.render_maps(labs, ds)
        cams[name], depth[name], labels[name] = cam, dep.view(1, H, W, 1), lab.view(1, H, W, 1)
        cam.world_view_transform = cam.world_view_transform.to(dev)
    return cams, depth, labels


def _prefilled(E, S, dev):
    return {"xyzw": torch.full((E, S, 4), SENTINEL["xyzw"], device=dev),
            "rgb": torch.full((E, S, 3), SENTINEL["rgb"], dtype=torch.uint8, device=dev),
            "segmentation": torch.full((E, S, 1), SENTINEL["segmentation"], dtype=torch.int16, device=dev),
            "count": torch.full((E,), SENTINEL["count"], dtype=torch.int32, device=dev)}


def _f64_views(depth, labels, cams, e):
    return [dict(depth=depth[n][e].reshape(c.image_height, c.image_width).cpu().numpy(),
                 label=None if labels is None else labels[n][e].reshape(c.image_height, c.image_width).cpu().numpy(),
                 viewmatrix=c.world_view_transform.cpu().numpy().reshape(-1), tanfovx=F32(c.tanfovx), tanfovy=F32(c.tanfovy))
            for n, c in cams.items()]


def _q32(views, spec, ds):
    A = np.asarray(spec.affine(), F32)
    return np.concatenate([unproject(v["depth"], v["viewmatrix"], v["tanfovx"], v["tanfovy"], ds, A)[0] for v in views])


def _picks(cand32, out):
    """Candidate indices of the GPU's picks, found by their float32 coordinates (-1: no candidate has them)."""
    pos = {}
    for i, row in enumerate(cand32.view(np.uint32)):
        pos.setdefault(row.tobytes(), i)
    return [pos.get(np.ascontiguousarray(r, F32).view(np.uint32).tobytes(), -1) for r in out]


def _against_f64(got, depth, labels, cams, spec, ds, what):
    """The cloud against the binary64 unprojection: every environment's count, the selected points within CROP_TOL (1 + |q|)
    (STRIDE / DENSE; off borderline points, whose crop decision may differ), fps_check on every FPS environment.
    -> the largest point error seen."""
    torch.cuda.synchronize()
    E = got["count"].shape[0]
    K = spec.num_points

    def one(e):
        views = _f64_views(depth, labels, cams, e)
        ref = ro.cloud_f64(views, spec, ds)
        cnt = int(got["count"][e])
        xyzw = got["xyzw"][e].cpu().numpy()
        if ref["border"].any():
            return None  # (a point within the tolerance of a crop face: n itself may differ; the restatement still holds)
        if K is None:
            assert cnt == ref["n"], f"{what} env {e}: count {cnt} != {ref['n']}"
            ok = xyzw[:, 3] == 1.0
            assert np.array_equal(ok, ref["valid"]), f"{what} env {e}: valid points differ"
            q = ref["q"][ok]
            g = xyzw[ok, :3]
        elif spec.sample == "stride":
            assert cnt == ref["sel"].size, f"{what} env {e}: count {cnt} != {ref['sel'].size}"
            q = ref["q"][ref["sel"]]
            g = xyzw[:cnt, :3]
        else:
            M = ref["sel"].size
            assert cnt == min(M, K), f"{what} env {e}: count {cnt} != min({M}, {K})"
            cand32 = _q32(views, spec, ds)[ref["sel"]]
            ro.fps_check(cand32.astype(np.float64), _picks(cand32, xyzw[:cnt, :3]))
            q = ref["q"][ref["sel"]]
            g = cand32
        if q.size == 0:
            return 0.0
        err = np.abs(g.astype(np.float64) - q) / (1.0 + np.abs(q))
        assert err.max() <= ro.CROP_TOL, f"{what} env {e}: point error {err.max():.2e}"
        return float(err.max())

    with ThreadPoolExecutor(ro.THREADS) as ex:
        errs = [x for x in ex.map(one, range(E)) if x is not None]
    assert errs, f"{what}: every environment has a point on a crop face: nothing was compared"
    print(f"{what}: max point error {max(errs):.2e} (1 + |q|) against binary64, {E - len(errs)} environments skipped")
    return max(errs)


SPECS = [PointCloudSpec(out_from_scene=sim_from_scene(_rigid(), 1.3)),
         PointCloudSpec(num_points=300, sample="stride", crop=((-9.0, -9.0, -9.0), (9.0, 9.0, 2.5)), exclude_labels=(3,)),
         PointCloudSpec(num_points=200, sample="fps", fps_candidates=1500, out_from_scene=sim_from_scene(_rigid(), 0.8))]


@pytest.mark.parametrize("spec", SPECS, ids=["dense", "stride", "fps"])
@pytest.mark.parametrize("sizes", [((33, 17), (70, 50)), ((9, 5), (200, 48))], ids=["33x17+70x50", "9x5+200x48"])
def test_partial_blocks_and_anisotropic_cameras(cuda_device, sizes, spec):
    dev = cuda_device
    ds = 1.5
    cams, depth, labels, frames = _synthetic(dev, sizes, E=3, seed=sum(sizes[0]))
    got = render_pointcloud(depth, labels, frames, cams, spec, depth_scale=ds)
    what = f"{sizes} {spec.sample if spec.num_points else 'dense'}"
    _against_restatement(got, depth, labels, frames, cams, spec, ds, what)
    _against_f64(got, depth, labels, cams, spec, ds, what)
    # maps of real frames, in the simulator frame
    rc, rd, rl = _rendered(dev, sizes, ds)
    spec_sim = PointCloudSpec(num_points=spec.num_points, sample=spec.sample, fps_candidates=spec.fps_candidates,
                              out_from_scene=sim_from_scene(_rigid(), 1.3))
    got = render_pointcloud(rd, rl, None, rc, spec_sim, depth_scale=ds)
    _against_restatement(got, rd, rl, None, rc, spec_sim, ds, what + " rendered")
    _against_f64(got, rd, rl, rc, spec_sim, ds, what + " rendered")
    assert int(got["count"][0]) > 0


# two cameras whose pixel counts end in partial blocks; 64 views in all
LIMIT_SIZES = ((201, 97), (33, 17))
LIMIT_E = 32


def _limit_inputs(dev, counts, seed):
    """E = 32 environments whose valid-point counts are ``counts`` (spread over both cameras at random pixels)."""
    gen = np.random.default_rng(seed)
    cams = {f"c{k}": _cam(W, H, k) for k, (W, H) in enumerate(LIMIT_SIZES)}
    for c in cams.values():
        c.world_view_transform = c.world_view_transform.to(dev)
    npx = [W * H for W, H in LIMIT_SIZES]
    total = sum(npx)
    flat = np.zeros((LIMIT_E, total), F32)
    for e, n in enumerate(counts):
        pix = gen.choice(total, size=min(n, total), replace=False)
        flat[e, pix] = (1.5 + 3.0 * gen.random(pix.size)).astype(F32)
    depth, labels, off = {}, {}, 0
    for (name, c), n in zip(cams.items(), npx):
        d = flat[:, off:off + n].reshape(LIMIT_E, c.image_height, c.image_width, 1)
        depth[name] = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
        labels[name] = torch.from_numpy(gen.integers(0, 50, d.shape).astype(np.int16)).to(dev)
        off += n
    return cams, depth, labels, total


def _limit_counts(K, M, total, seed):
    want = [0, 1, K - 1, K, K + 1, M - 1, M, M + 1, total]
    rng = np.random.default_rng(seed)
    extra = list(rng.integers(0, 300, LIMIT_E - len(want)))  # (small: the binary64 FPS check is a host pass per pick)
    return [int(min(max(n, 0), total)) for n in want + extra]


def _check_unused(got, dense):
    """Every slot without a point (DENSE: invalid pixels; else the slots past count) reads 0 / 0 / -1, not the sentinel."""
    torch.cuda.synchronize()
    S = got["xyzw"].shape[1]
    for e, c in enumerate(got["count"].cpu().numpy()):
        empty = got["xyzw"][e, :, 3] != 1.0 if dense else torch.arange(S, device=got["xyzw"].device) >= int(c)
        assert bool((got["xyzw"][e][empty] == 0).all()) and bool((got["rgb"][e][empty] == 0).all()) and \
            bool((got["segmentation"][e][empty] == -1).all()), f"env {e} (count {c}): empty slots are not 0 / 0 / -1"


LIMIT_CASES = [("dense", None, None), ("stride", 1, None), ("stride", 1024, None), ("stride", 8192, None)]
for _M in (1, 1023, 1024, 1025, 8192, 8193, 16384):
    for _K in sorted({1, min(_M, 8192), min(_M + 1, 8192)}):
        LIMIT_CASES.append(("fps", _K, _M))


@pytest.mark.parametrize("mode,K,M", LIMIT_CASES)
def test_counts_at_the_limits(cuda_device, mode, K, M):
    dev = cuda_device
    total = sum(W * H for W, H in LIMIT_SIZES)
    counts = _limit_counts(K or 1, M or K or 1, total, seed=(K or 0) + (M or 0))
    cams, depth, labels, _ = _limit_inputs(dev, counts, seed=(K or 0) * 7 + (M or 0))
    spec = PointCloudSpec() if mode == "dense" else PointCloudSpec(num_points=K, sample=mode, fps_candidates=M or 8192)
    S = total if K is None else K
    out = _prefilled(LIMIT_E, S, dev)
    got = render_pointcloud(depth, labels, None, cams, spec, out=out)
    _check_unused(got, mode == "dense")
    cnt = got["count"].cpu().numpy()
    for e, n in enumerate(counts):
        want = n if mode == "dense" else min(n, K) if mode == "stride" else min(n, M, K)
        assert cnt[e] == want, f"env {e} (n = {n}): count {cnt[e]} != {want}"
    what = f"E=32 C=2 {mode} K={K} M={M}"
    if mode != "fps" or M <= 1025:  # (the restatement's float32 FPS is one host pass per pick: the small cases only)
        _against_restatement(got, depth, labels, None, cams, spec, 1.0, what)
    _against_f64(got, depth, labels, cams, spec, 1.0, what)


def test_sixty_five_views_are_refused_before_any_device_work(cuda_device):
    dev = cuda_device
    cams, depth, labels, _ = _synthetic(dev, ((9, 5), (7, 3)), E=33, seed=1)
    out = _prefilled(33, 64, dev)
    with pytest.raises(ValueError):
        render_pointcloud(depth, labels, None, cams, PointCloudSpec(num_points=64, sample="fps"), out=out)
    torch.cuda.synchronize()
    assert bool((out["count"] == SENTINEL["count"]).all()) and bool((out["xyzw"] == SENTINEL["xyzw"]).all())


def test_crop_faces_on_a_point_and_excluded_extreme_labels(cuda_device):
    dev = cuda_device
    cams, depth, labels, frames = _synthetic(dev, ((33, 17), (70, 50)), E=2, seed=9)
    # labels -1 and 32767 on some pixels: both must go
    for n in cams:
        lab = labels[n]
        lab[:, ::3] = 32767
        lab[:, 1::5] = -1
    A = sim_from_scene(_rigid(), 1.3)
    dense = render_pointcloud(depth, labels, frames, cams, PointCloudSpec(out_from_scene=A))
    torch.cuda.synchronize()
    xyzw = dense["xyzw"][0].cpu().numpy()
    seg0 = dense["segmentation"][0, :, 0].cpu().numpy()
    assert {-1, 32767} <= set(seg0[xyzw[:, 3] == 1.0].tolist())
    ok =np.flatnonzero((xyzw[:, 3] == 1.0) & ~np.isin(seg0, [-1, 32767]))
    a, b = ok[len(ok) // 3], ok[2 * len(ok) // 3]
    # a box of one point (every face on it), and a wide box whose lo.x passes through a and hi.z through b
    boxes = [(xyzw[a, :3].tolist(), xyzw[a, :3].tolist()),
             ([float(xyzw[a, 0]), -50.0, -50.0], [50.0, 50.0, float(xyzw[b, 2])])]
    for crop in boxes:
        for spec in (PointCloudSpec(out_from_scene=A, crop=crop, exclude_labels=(-1, 32767)),
                     PointCloudSpec(out_from_scene=A, crop=crop),
                     PointCloudSpec(num_points=400, sample="stride", out_from_scene=A, crop=crop,
                                    exclude_labels=(-1, 32767))):
            what = f"crop {crop} exclude {spec.exclude_labels}"
            got = render_pointcloud(depth, labels, frames, cams, spec)
            _against_restatement(got, depth, labels, frames, cams, spec, 1.0, what)
            seg = got["segmentation"][..., 0].cpu().numpy()
            w = got["xyzw"][..., 3].cpu().numpy()
            if spec.num_points is None:
                assert w[0, a] == 1.0 and (crop is boxes[0] or w[0, b] == 1.0), f"{what}: a point on a face was dropped"
            if spec.exclude_labels:
                assert not np.isin(seg[w == 1.0], [-1, 32767]).any(), what
            elif crop is boxes[1]:
                assert np.isin(seg[w == 1.0], [-1, 32767]).any(), what


def test_fps_within_one_round_of_the_thread_count(cuda_device):
    # the candidate count just past a 1024-thread round with every environment full: picks of the second register row
    dev = cuda_device
    cams, depth, labels, frames = _synthetic(dev, ((40, 26), (9, 5)), E=4, seed=2, zero=0.0)
    for M, K in ((1025, 1025), (1023, 512)):
        spec = PointCloudSpec(num_points=K, sample="fps", fps_candidates=M)
        got = render_pointcloud(depth, labels, frames, cams, spec)
        _against_restatement(got, depth, labels, frames, cams, spec, 1.0, f"fps M={M} K={K}")
        _against_f64(got, depth, labels, cams, spec, 1.0, f"fps M={M} K={K}")
        assert bool((got["count"] == min(M, K)).all()) and math.isfinite(float(got["xyzw"].sum()))
