"""hgs_hull_visibility (csrc/hgs_visibility.hip) and hgs_lift_moments_gated (csrc/hgs_lift.hip) against the numpy paths of
utils/visibility.py and utils/lift.py, word for word and bit for bit: every grid, density and knob of tests/visibility_cases.py at
the point and view counts around the wavefront, the workgroup and the word boundaries; the hand-written rays with their expected bits;
repeatability; the refusals by their text; the analytic scene's words; and the init_cloud.py --visibility driver on both devices."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import carve_cases as CC
from tests import lift_cases as LC
from tests import visibility_cases as VC
from tests import visibility_reference as VR

pytestmark = pytest.mark.gpu

LIFT_NS = (0, 1, 63, 64, 65, 1000)
LIFT_VS = (1, 2, 33)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _device(pts, C, occ):
    return torch.from_numpy(pts).cuda(), torch.from_numpy(C).cuda(), torch.from_numpy(occ).cuda()


# ---- 1. the kernel equals the numpy path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", VC.DENSITIES)
@pytest.mark.parametrize("dims", VC.GRIDS)
def test_kernel_equals_the_numpy_path(dims, density):
    from utils import visibility
    occ = VC.random_occ(dims, density, seed=sum(dims))
    pts, C = VC.equality_inputs(dims)
    p, c, o = _device(pts, C, occ)
    for skip in VC.SKIPS:
        for max_blocked in VC.MAX_BLOCKED:
            # (a pair's bit depends on nothing but its point, its centre and the grid: the numpy path runs once, at the largest size)
            full = visibility.unpack_bits(visibility.visibility_numpy(pts, C, occ, VC.ORIGIN, VC.H, skip, max_blocked), C.shape[0])
            for N in VC.NS:
                for V in VC.VS:
                    got = visibility.visibility_device(p[:N], c[:V], o, VC.ORIGIN, VC.H, skip, max_blocked)
                    assert got.dtype == torch.int32 and tuple(got.shape) == (N, (V + 31) // 32)
                    assert _bits(got.cpu().numpy(), visibility.pack_bits(full[:N, :V])), (skip, max_blocked, N, V)
    host = visibility.hull_visibility(pts, C, occ, VC.ORIGIN, VC.H, 1, 0, device="cuda")
    assert _bits(host, visibility.visibility_numpy(pts, C, occ, VC.ORIGIN, VC.H, 1, 0))


@pytest.mark.parametrize("case", VC.hand_cases(), ids=lambda c: c[0])
def test_hand_written_rays(case):
    from utils import visibility
    _, pts, C, occ, origin, h, skip, max_blocked, want = case
    got = visibility.visibility_device(*_device(pts, C, occ), origin, h, skip, max_blocked)
    assert _bits(got.cpu().numpy(), VR.words_of(want))


def test_repeatable_and_stream_independent():
    from utils import visibility
    dims = VC.GRIDS[-1]
    pts, C = VC.equality_inputs(dims)
    p, c, o = _device(pts, C, VC.random_occ(dims, 0.3, seed=sum(dims)))

    def run():
        return visibility.visibility_device(p, c, o, VC.ORIGIN, VC.H, 1, 0)
    a, b = run(), run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s = run()
    side.synchronize()
    assert _bits(a.cpu().numpy(), b.cpu().numpy()) and _bits(a.cpu().numpy(), s.cpu().numpy())


def test_quality_scene_words_equal_the_hosts():
    from utils import visibility
    s = VC.quality_scene()
    for skip in (0, 1):
        got = visibility.hull_visibility(s["points"], s["centres"], s["occ"], s["origin"], s["h"], skip, device="cuda")
        assert _bits(got, visibility.visibility_numpy(s["points"], s["centres"], s["occ"], s["origin"], s["h"], skip))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    import hgs_runtime as rt
    from utils import visibility
    dims = (5, 4, 3)
    pts, C = VC.equality_inputs(dims)
    p, c, o = _device(pts[:8], C[:3], VC.random_occ(dims, 0.3))
    words = torch.zeros((8, 1), dtype=torch.int32, device="cuda")
    origin = np.ascontiguousarray(VC.ORIGIN)
    L, st = rt.lib(), rt.current_stream()
    good = dict(N=8, points=rt.ptr(p), V=3, centres=rt.ptr(c), occ=rt.ptr(o), origin=origin.ctypes.data, h=VC.H, nx=5, ny=4, nz=3, skip=1,
                max_blocked=0, visible=rt.ptr(words))

    def call(**change):
        a = dict(good, **change)
        return L.hgs_hull_visibility(st, a["N"], a["points"], a["V"], a["centres"], a["occ"], a["origin"], a["h"], a["nx"], a["ny"], a["nz"],
                                     a["skip"], a["max_blocked"], a["visible"])
    nan_origin = np.array([0.0, np.nan, 0.0])
    inf_origin = np.array([np.inf, 0.0, 0.0])
    bad = [(dict(N=-1), "N = -1 points"), (dict(V=0), "V = 0 views (1 to 4096)"), (dict(V=4097), "V = 4097 views (1 to 4096)"),
           (dict(nx=0), "a grid of 0 x 4 x 3 voxels (1 to 1024 per axis)"), (dict(ny=1025), "a grid of 5 x 1025 x 3 voxels"),
           (dict(nz=-2), "a grid of 5 x 4 x -2 voxels"), (dict(skip=-1), "skip = -1 (0 to 1024)"), (dict(skip=1025), "skip = 1025 (0 to 1024)"),
           (dict(max_blocked=-1), "max_blocked = -1 (0 to 3072)"), (dict(max_blocked=3073), "max_blocked = 3073 (0 to 3072)"),
           (dict(h=0.0), "voxel size h = 0"), (dict(h=-1.0), "voxel size h = -1"), (dict(h=float("inf")), "voxel size h = inf"),
           (dict(h=float("nan")), "nan (h and 1/h finite and positive)"), (dict(h=1e-320), "h and 1/h finite and positive"),
           (dict(origin=nan_origin.ctypes.data), "the origin is not finite"), (dict(origin=inf_origin.ctypes.data), "the origin is not finite")]
    bad += [({k: None}, "null argument") for k in ("points", "centres", "occ", "origin", "visible")]
    for change, text in bad:
        assert call(**change) != 0, change
        message = L.hgs_last_error().decode()
        assert message.startswith("hgs_hull_visibility: ") and text in message, (change, message)
    torch.cuda.synchronize()
    assert not words.any()                                       # nothing was launched
    assert call(N=0, points=None, visible=None) == 0 and call() == 0
    # the wrapper raises, and checks what the kernel trusts
    with pytest.raises(rt.HgsError, match="occ holds 59 bytes"):
        rt.visibility_check((5, 4, 3), o.reshape(-1)[:-1].contiguous(), p, c, words)
    with pytest.raises(rt.HgsError, match=r"visible of shape \(8, 2\)"):
        rt.visibility_check((5, 4, 3), o, p, c, torch.zeros((8, 2), dtype=torch.int32, device="cuda"))
    with pytest.raises(rt.HgsError, match="visible must be torch.int32"):
        rt.visibility_check((5, 4, 3), o, p, c, words.long())
    with pytest.raises(rt.HgsError, match="centres of shape"):
        rt.visibility_check((5, 4, 3), o, p, c.reshape(-1), words)
    with pytest.raises(rt.HgsError, match="points must be contiguous"):
        rt.visibility_check((5, 4, 3), o, torch.zeros((3, 8), dtype=torch.float64, device="cuda").t(), c, words)
    with pytest.raises(rt.HgsError, match="1 to 1024 per axis"):
        rt.visibility_check((5, 4, 1025), o, p, c, words)
    for change in (dict(points=p.cpu()), dict(points=p.float()), dict(centres=c.cpu()), dict(occ=o.cpu()), dict(occ=o.int()), dict(occ=o[0]),
                   dict(skip=-1), dict(max_blocked=3073), dict(h=0.0), dict(origin=nan_origin), dict(centres=c[:0])):
        with pytest.raises(rt.HgsError):
            visibility.visibility_device(**dict(dict(points=p, centres=c, occ=o, origin=VC.ORIGIN, h=VC.H, skip=1, max_blocked=0), **change))
    with pytest.raises(rt.HgsError, match="not finite"):
        visibility.upload_centres(np.array([[0.0, np.nan, 0.0]]), "cuda")


# ---- 3. the gated moments --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lift_inputs():
    """{V: (views, planes, Packed, points, prev, bool [N, V])} at the largest N; a smaller N is a prefix."""
    from utils import lift
    out = {}
    for V in LIFT_VS:
        views = LC.equality_views(V)
        planes = LC.random_planes(views, seed=V)
        out[V] = (views, planes, lift.pack(views, *planes, "cuda"), LC.equality_points(max(LIFT_NS)), LC.unit_prev(max(LIFT_NS)),
                  VC.random_visible(max(LIFT_NS), V, seed=V))
    return out


@pytest.mark.parametrize("N", LIFT_NS)
def test_gated_moments_equal_the_numpy_path(lift_inputs, N):
    from utils import lift, visibility
    s2 = lift.sin2(10.0)
    for V in LIFT_VS:
        views, planes, packed, pts, prev, vis = lift_inputs[V]
        words = visibility.pack_bits(vis[:N])
        dev, w = torch.from_numpy(pts[:N]).cuda(), torch.from_numpy(words).cuda()
        ones = torch.from_numpy(visibility.all_visible(N, V)).cuda()
        for pv in (None, prev[:N]):
            pd = None if pv is None else torch.from_numpy(pv).cuda()
            got = lift.moments_device(dev, packed, pd, s2, visible=w)
            want = lift.moments_numpy(pts[:N], views, *planes, pv, s2, visible=words)
            assert got[0].shape == (N, 6) and got[2].dtype == torch.int32
            assert all(_bits(g.cpu().numpy(), x) for g, x in zip(got, want)), (V, pv is not None)
            plain = lift.moments_device(dev, packed, pd, s2)
            assert all(_bits(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(lift.moments_device(dev, packed, pd, s2, visible=ones), plain)), V
            if N == max(LIFT_NS):
                assert not _bits(got[0].cpu().numpy(), plain[0].cpu().numpy()) and want[2].sum() > 0
    if N:                                                        # the host-array entry points
        views, planes, packed, pts, prev, vis = lift_inputs[2]
        words = visibility.pack_bits(vis[:N])
        host = lift.lift_moments(pts[:N], views, *planes, prev[:N], s2, device="cuda", visible=words)
        assert all(_bits(a, b) for a, b in zip(host, lift.moments_numpy(pts[:N], views, *planes, prev[:N], s2, visible=words)))


def test_gated_moments_refusals(lift_inputs):
    import hgs_runtime as rt
    from utils import lift, visibility
    views, planes, packed, pts, prev, vis = lift_inputs[33]
    dev = torch.from_numpy(pts[:8]).cuda()
    w = torch.from_numpy(visibility.pack_bits(vis[:8])).cuda()
    M = torch.zeros((8, 6), dtype=torch.float64, device="cuda")
    wsum = torch.zeros(8, dtype=torch.float64, device="cuda")
    count = torch.zeros(8, dtype=torch.int32, device="cuda")
    L, st = rt.lib(), rt.current_stream()

    def call(visible, words, V=33, min_conf=1):
        return L.hgs_lift_moments_gated(st, 8, rt.ptr(dev), V, rt.ptr(packed.carve.views_dev), rt.ptr(packed.carve.masks_dev),
                                        rt.ptr(packed.orients_dev), rt.ptr(packed.confs_dev), rt.ptr(packed.tab_dev), None, 0.0, min_conf, visible,
                                        words, rt.ptr(M), rt.ptr(wsum), rt.ptr(count))
    for args, text in (((None, 2), "null argument"), ((rt.ptr(w), 1), "words = 1, 33 views take 2"), ((rt.ptr(w), 3), "words = 3"),
                       ((rt.ptr(w), 2, 0), "V = 0 views"), ((rt.ptr(w), 2, 33, 256), "min_conf = 256")):
        assert call(*args) != 0, args
        message = L.hgs_last_error().decode()
        assert message.startswith("hgs_lift_moments_gated: ") and text in message, message
    torch.cuda.synchronize()
    assert not M.any() and not wsum.any() and not count.any()    # nothing was launched
    assert call(rt.ptr(w), 2) == 0
    for bad in (w[:, :1].contiguous(), w[:7].contiguous(), w.long(), w.cpu(), torch.zeros((2, 8), dtype=torch.int32, device="cuda").t()):
        with pytest.raises(rt.HgsError, match="visible"):
            lift.moments_device(dev, packed, visible=bad)


# ---- 4. the driver on both devices ---------------------------------------------------------------------------------------------
def test_driver_agrees_on_both_devices_and_the_scene_loads(tmp_path, capsys):
    import init_cloud
    from data.dataset_readers import fetchPly
    from scene import Scene
    from utils import carve, lift, visibility
    bins, normals, reports = {}, {}, {}
    for device in ("cuda", "cpu"):
        src = str(tmp_path / device)
        views, masks, _, _ = CC.build_scene(src)
        orients, confs, _ = LC.smooth_orientations(src, views)
        n = init_cloud.main(["-s", src, "--device", device, "--grid", "24", "--min_views", "6", "--min_percent", "100", "--directions",
                             "--visibility"])
        sparse = os.path.join(src, "sparse", "0")
        with open(os.path.join(sparse, "points3D.bin"), "rb") as fh:
            bins[device] = fh.read()
        normals[device] = fetchPly(os.path.join(sparse, "points3D.ply")).normals
        reports[device] = [line for line in capsys.readouterr().out.splitlines() if line.startswith("visibility")]
        assert n > 100 and normals[device].shape == (n, 3)
    assert bins["cuda"] == bins["cpu"] and reports["cuda"] == reports["cpu"] and len(reports["cpu"]) == 1
    # the same words on both devices, and through them the same directions under the solvers' rule
    xyz = CC.read_points(os.path.join(str(tmp_path / "cpu"), "sparse", "0", "points3D.bin"))[0]
    lo, hi = carve.auto_bounds(views, masks, 6, 100)
    origin, h, dims = carve.fine_grid(lo, hi, 24)
    occ = carve.carve_grid(origin, h, dims, views, masks, 6, 100)
    C = visibility.camera_centres(views)
    words = visibility.hull_visibility(xyz, C, occ, origin, h)
    assert _bits(words, visibility.hull_visibility(xyz, C, occ, origin, h, device="cuda"))
    assert 0 < (~visibility.unpack_bits(words, len(views))).sum()
    host = lift.lift_directions(xyz, views, masks, orients, confs, visible=words)
    dev = lift.lift_directions(xyz, views, masks, orients, confs, device="cuda", visible=words)
    assert np.array_equal(normals["cpu"], host[0].astype(np.float32)) and np.array_equal(normals["cuda"], dev[0].astype(np.float32))
    prev = lift.lift_directions(xyz, views, masks, orients, confs, rounds=2, visible=words)[0]
    M = lift.lift_moments(xyz, views, masks, orients, confs, prev, lift.sin2(10.0), visible=words)[0]      # the last round's matrices
    below = LC.compare_solves(M, dev[:2], host[:2])
    live = int(host[0].any(axis=1).sum())
    print(f"{below} of {live} directions below the gap")
    assert live > n // 2 and below <= 0.01 * live
    args = SimpleNamespace(source_path=str(tmp_path / "cuda"), model_path=str(tmp_path / "model"), images="images", sh_degree=0, resolution=-1,
                           data_device="cuda", eval=False, init_directions=True, direction_stretch=3.0)
    scene = Scene(args, shuffle=False)
    assert scene.gaussians.get_xyz.shape[0] == n
    got = scene.gaussians.get_orientation.detach()
    want = torch.from_numpy(normals["cuda"]).cuda()
    has = want.any(dim=1)
    err = torch.minimum((got - want).abs().amax(dim=1), (got + want).abs().amax(dim=1))
    assert float(err[has].max()) <= 1e-5
