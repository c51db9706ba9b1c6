"""The hull's ray march (utils/visibility.py) and the gated lift (utils/lift.py) on the host: the numpy path against the loop
restatement of tests/visibility_reference.py, word for word, over the grids, densities, knobs and the point and view counts around the
word boundaries; the hand-written rays with their expected bits; the refusals; the gated moments against the gated restatement, bit
for bit; what the gate is worth on the analytic scene of tests/visibility_cases.py; and the init_cloud.py --visibility driver."""
import os

import numpy as np
import pytest

from tests import carve_cases as CC
from tests import lift_cases as LC
from tests import visibility_cases as VC
from tests import visibility_reference as VR


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. the numpy path equals the loop -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", VC.DENSITIES)
@pytest.mark.parametrize("dims", VC.GRIDS)
def test_numpy_path_equals_the_loop(dims, density):
    from utils import visibility
    blocked = 0
    for skip in VC.SKIPS:
        for max_blocked in VC.MAX_BLOCKED:
            occ, pts, C, want = VC.loop_truth(dims, density, skip, max_blocked)
            blocked += int((~want).sum())
            for N in VC.NS:
                for V in VC.VS:
                    got = visibility.visibility_numpy(pts[:N], C[:V], occ, VC.ORIGIN, VC.H, skip, max_blocked)
                    assert got.shape == (N, (V + 31) // 32) and _bits(got, VR.words_of(want[:N, :V])), (skip, max_blocked, N, V)
                    if V % 32 and N:
                        assert not (got[:, -1].view(np.uint32) >> np.uint32(V % 32)).any()   # the bits at and above V are 0
    assert blocked > 100 or max(dims) < 5                        # (the two small grids may have nothing in a ray's way)
    assert not (VC.loop_truth(dims, density, 0, 0)[3] & ~VC.loop_truth(dims, density, 3, 2)[3]).any()   # looser knobs block no more
    occ, pts, C, want = VC.loop_truth(dims, density, 1, 0)
    host = visibility.hull_visibility(pts, C, occ, VC.ORIGIN, VC.H)
    assert _bits(host, VR.words_of(want))
    assert np.array_equal(visibility.unpack_bits(host, C.shape[0]), want) and _bits(visibility.pack_bits(want), host)
    assert np.array_equal(visibility.unpack_bits(visibility.all_visible(5, 33), 33), np.ones((5, 33), bool))


@pytest.mark.parametrize("case", VC.hand_cases(), ids=lambda c: c[0])
def test_hand_written_rays(case):
    from utils import visibility
    _, pts, C, occ, origin, h, skip, max_blocked, want = case
    assert np.array_equal(VR.visible_loop(pts, C, occ, origin, h, skip, max_blocked), want)
    assert _bits(visibility.visibility_numpy(pts, C, occ, origin, h, skip, max_blocked), VR.words_of(want))


def test_refusals():
    from utils import visibility
    occ, pts, C, _ = VC.loop_truth((2, 2, 2), 0.3, 1, 0)
    good = dict(points=pts, centres=C, occ=occ, origin=VC.ORIGIN, h=VC.H, skip=1, max_blocked=0)
    bad = [dict(skip=-1), dict(skip=1025), dict(skip=0.5), dict(max_blocked=-1), dict(max_blocked=3073), dict(h=0.0), dict(h=-1.0),
           dict(h=float("inf")), dict(h=float("nan")), dict(h=1e-320), dict(origin=[0.0, float("nan"), 0.0]), dict(origin=[0.0, 0.0]),
           dict(occ=occ.astype(np.int32)), dict(occ=occ[0]), dict(occ=np.zeros((1, 1, 1025), np.uint8)), dict(centres=np.zeros((0, 3))),
           dict(centres=np.zeros((4097, 3))), dict(centres=np.zeros((3, 2))), dict(centres=np.array([[0.0, float("inf"), 0.0]]))]
    for change in bad:
        with pytest.raises(ValueError):
            visibility.visibility_numpy(**dict(good, **change))
    with pytest.raises(ValueError, match="view 1 is not finite"):
        visibility.camera_centres([CC.identity_view(4, 4), CC.identity_view(4, 4)._replace(t=np.array([0.0, np.nan, 0.0]))])
    assert np.array_equal(visibility.camera_centres(CC.ring_views(3)), np.stack([-v.R.T @ v.t for v in CC.ring_views(3)]))
    with pytest.raises(ValueError, match="device"):
        visibility.hull_visibility(pts, C, occ, VC.ORIGIN, VC.H, device="cpu")


# ---- 2. the gated moments ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_prev", (False, True))
def test_gated_moments_equal_the_gated_restatement(with_prev):
    from utils import lift, visibility
    N, V = 80, 8
    views = LC.equality_views(V)
    planes = LC.random_planes(views, seed=V)
    pts = LC.equality_points(N)
    prev, s2 = (LC.unit_prev(N), lift.sin2(10.0)) if with_prev else (None, 0.0)
    vis = VC.random_visible(N, V, seed=2)
    words = visibility.pack_bits(vis)
    got = lift.moments_numpy(pts, views, *planes, prev, s2, visible=words)
    want = VC.gated_moments_loop(pts, views, *planes, lift.table(), vis, prev, s2)
    assert all(_bits(g, w) for g, w in zip(got, want))
    plain = lift.moments_numpy(pts, views, *planes, prev, s2)
    assert all(_bits(a, b) for a, b in zip(lift.moments_numpy(pts, views, *planes, prev, s2, visible=visibility.all_visible(N, V)), plain))
    assert not _bits(got[0], plain[0]) and (got[2] <= plain[2]).all() and not got[2][1] and _bits(got[0][:1], plain[0][:1])
    host = lift.lift_moments(pts, views, *planes, prev, s2, visible=words)
    assert all(_bits(a, b) for a, b in zip(host, got))
    with pytest.raises(ValueError, match="visible"):
        lift.moments_numpy(pts, views, *planes, visible=words[:, :0])
    with pytest.raises(ValueError, match="visible"):
        lift.moments_numpy(pts, views, *planes, visible=words.astype(np.int64))


def test_gated_directions_zero_a_point_with_too_few_views():
    from utils import lift, visibility
    views, pts, d = LC.rig(6, 40)
    orient, inside = LC.image_angle_bytes(views, pts, d)
    assert inside.all()
    used, conf = np.ones(orient.shape, bool), np.full(orient.shape, 255, np.uint8)
    vis = np.ones((40, 6), bool)
    vis[0, 1:] = False                                           # one view left: no direction, and no fallback to the ungated fit
    vis[1, 2:] = False                                           # two views: a direction
    M, _, count = lift.moments_from_samples(pts, views, used, orient, conf, visible=visibility.pack_bits(vis))
    got, _ = lift.solve_numpy(M, count)
    assert count[0] == 1 and count[1] == 2 and not got[0].any() and got[1:].any(axis=1).all()


# ---- 3. what the gate is worth ---------------------------------------------------------------------------------------------------
def test_quality_on_the_analytic_scene():
    """Measured on this scene (the numpy path; the figures DESIGN.md section 8 quotes): 792 points, 9504 pairs; skip 0 sets the bit of
    no pair with another first hit at all; skip 1 sets it for 35 such pairs, the longest chord 1.45 voxels; the plain lift's median
    error is 7.63 degrees after round 0 and 1.76 after three re-weighted rounds, the gated lift's 0.17 after round 0 and 0.17 after
    three rounds, an oracle gate's 0.13; 768 of 792 points keep a direction."""
    from utils import visibility
    s = VC.quality_scene()
    pts, h = s["points"], s["h"]
    assert pts.shape == (792, 3)
    words = {k: visibility.visibility_numpy(pts, s["centres"], s["occ"], s["origin"], h, skip=k) for k in (0, 1)}
    vis = {k: visibility.unpack_bits(w, VC.Q_VIEWS) for k, w in words.items()}
    far = s["chord"] > 1e-6 * h                                  # (the point's own hit comes back to a few ulp, not to zero)
    for k in (0, 1):
        wrong = vis[k] & far
        print(f"skip {k}: {int(vis[k].sum())} of {vis[k].size} pairs visible, {int(wrong.sum())} of them with another first hit, the longest "
              f"chord {float((s['chord'][wrong] / h).max()) if wrong.any() else 0.0:.2f} voxels")
    assert not (vis[0] & (s["chord"] > h)).any()
    assert not (vis[1] & (s["chord"] > 3.0 * h)).any()
    plain0, plain3 = (np.median(LC.angle_deg(VC.quality_lift(s, None, r), s["truth"])) for r in (0, 3))
    d0, d3 = VC.quality_lift(s, words[1], 0), VC.quality_lift(s, words[1], 3)
    gated0, gated3 = (np.median(LC.angle_deg(d, s["truth"])) for d in (d0, d3))          # (over all points: a zero direction counts 90)
    oracle = np.median(LC.angle_deg(VC.quality_lift(s, visibility.pack_bits(~far), 0), s["truth"]))
    kept = int(d0.any(axis=1).sum())
    print(f"median error, degrees: plain {plain0:.2f} after round 0 and {plain3:.2f} after three rounds; gated {gated0:.2f} and {gated3:.2f}; "
          f"oracle gate {oracle:.2f}; {kept} of {pts.shape[0]} points keep a direction")
    assert gated0 < plain3
    assert gated0 < 3.0 * LC.STEP_DEG
    assert kept >= 0.9 * pts.shape[0]


# ---- 4. the driver -----------------------------------------------------------------------------------------------------------------
def _hull_args(extra=()):
    return ["--device", "cpu", "--grid", "24", "--min_views", "6", "--min_percent", "100", *extra]


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_driver_gates_the_directions_and_the_loader_reads_them(tmp_path, capsys):
    import init_cloud
    from data.colmap import write_points3D_arrays
    from data.dataset_readers import fetchPly, readColmapSceneInfo, storePly
    from utils import carve, lift, visibility
    src = str(tmp_path / "scene")
    views, masks, images, _ = CC.build_scene(src)
    orients, confs, _ = LC.smooth_orientations(src, views)
    sparse = os.path.join(src, "sparse", "0")
    n = init_cloud.main(["-s", src, *_hull_args(["--directions", "--visibility"])])
    out = capsys.readouterr().out
    assert "visibility (skip 1, max_blocked 0):" in out and "lost their direction to the gate" in out
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin", "points3D.colmap.bin", "points3D.ply"]
    gated_bin = _read(os.path.join(sparse, "points3D.bin"))
    xyz, rgb, _ = CC.read_points(os.path.join(sparse, "points3D.bin"))
    # the words the driver must have used: the solid grid over the automatic bounds, marched from the written points
    lo, hi = carve.auto_bounds(views, masks, 6, 100)
    origin, h, dims = carve.fine_grid(lo, hi, 24)
    occ = carve.carve_grid(origin, h, dims, views, masks, 6, 100)
    words = visibility.hull_visibility(xyz, visibility.camera_centres(views), occ, origin, h)
    vis = visibility.unpack_bits(words, len(views))
    assert 0 < (~vis).sum() < vis.size
    d, _, count = lift.lift_directions(xyz, views, masks, orients, confs, visible=words)
    pcd = fetchPly(os.path.join(sparse, "points3D.ply"))
    assert n == len(xyz) and np.array_equal(pcd.normals, d.astype(np.float32)) and d.any(axis=1).sum() > n // 2
    on_mask, seen = visibility.pair_counts(xyz, views, masks, words)
    plain_d, _, plain_count = lift.lift_directions(xyz, views, masks, orients, confs)
    lost = int(((plain_count >= 2) & (count < 2)).sum())
    assert f"{on_mask} (point, view) pair(s) in frame and on the mask, {seen} of them visible; {lost} point(s) lost" in out
    assert 0 < seen < on_mask
    loaded = readColmapSceneInfo(src).point_cloud
    assert np.array_equal(loaded.normals, d.astype(np.float32)) and loaded.points.shape == (n, 3)
    # the knobs reach the march
    init_cloud.main(["-s", src, *_hull_args(["--directions", "--visibility", "--vis_skip", "3", "--vis_max_blocked", "2", "--overwrite"])])
    w2 = visibility.hull_visibility(xyz, visibility.camera_centres(views), occ, origin, h, 3, 2)
    assert not _bits(w2, words)
    d2 = lift.lift_directions(xyz, views, masks, orients, confs, visible=w2)[0]
    assert np.array_equal(fetchPly(os.path.join(sparse, "points3D.ply")).normals, d2.astype(np.float32))
    # without the flag: the files of the ungated calls, byte for byte
    capsys.readouterr()
    init_cloud.main(["-s", src, *_hull_args(["--directions", "--overwrite"])])
    assert "visibility" not in capsys.readouterr().out
    assert _read(os.path.join(sparse, "points3D.bin")) == gated_bin
    write_points3D_arrays(xyz, rgb, np.zeros(n), str(tmp_path / "want.bin"))
    storePly(str(tmp_path / "want.ply"), xyz, rgb, plain_d)
    assert _read(os.path.join(sparse, "points3D.bin")) == _read(str(tmp_path / "want.bin"))
    assert _read(os.path.join(sparse, "points3D.ply")) == _read(str(tmp_path / "want.ply"))


def test_driver_mode_both_leaves_outside_points_unoccluded(tmp_path):
    import init_cloud
    from data.dataset_readers import fetchPly
    from utils import carve, lift, visibility
    src = str(tmp_path / "scene")
    views, masks, _, _ = CC.build_scene(src)
    orients, confs, _ = LC.smooth_orientations(src, views)
    n = init_cloud.main(["-s", src, *_hull_args(["--mode", "both", "--min_views", "1", "--min_percent", "0", "--bounds", "-0.5", "-0.5", "-0.5",
                                                 "0.5", "0.5", "0.5", "--directions", "--visibility"])])
    sparse = os.path.join(src, "sparse", "0")
    xyz = CC.read_points(os.path.join(sparse, "points3D.bin"))[0]
    origin, h, dims = carve.fine_grid([-0.5] * 3, [0.5] * 3, 24)
    occ = carve.carve_grid(origin, h, dims, views, masks, 1, 0)
    words = visibility.hull_visibility(xyz, visibility.camera_centres(views), occ, origin, h)
    outside = (np.abs(xyz) > 0.5).any(axis=1)
    assert outside.sum() > 10 and _bits(words[outside], visibility.all_visible(int(outside.sum()), len(views)))
    d = lift.lift_directions(xyz, views, masks, orients, confs, visible=words)[0]
    assert n == len(xyz) and np.array_equal(fetchPly(os.path.join(sparse, "points3D.ply")).normals, d.astype(np.float32))


def test_driver_refusals(tmp_path):
    import init_cloud
    src = str(tmp_path / "scene")
    views, _, _, _ = CC.build_scene(src)
    LC.smooth_orientations(src, views)
    with pytest.raises(SystemExit, match=r"init_cloud.py: --visibility gates the votes of --directions"):
        init_cloud.main(["-s", src, *_hull_args(["--visibility"])])
    with pytest.raises(SystemExit, match=r"init_cloud.py: --visibility marches the carved grid, and --mode filter carves none"):
        init_cloud.main(["-s", src, *_hull_args(["--mode", "filter", "--directions", "--visibility"])])
    for extra in (["--vis_skip", "-1"], ["--vis_skip", "1025"], ["--vis_max_blocked", "-1"], ["--vis_max_blocked", "3073"]):
        with pytest.raises(SystemExit, match="--vis_skip"):
            init_cloud.main(["-s", src, *_hull_args(["--directions", "--visibility", *extra])])
    sparse = os.path.join(src, "sparse", "0")                     # a refused run leaves the points where they were
    assert sorted(os.listdir(sparse)) == ["cameras.bin", "images.bin", "points3D.bin"]


# ---- 5. binding ------------------------------------------------------------------------------------------------------------------
def test_binding_loads():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    for name, n_args in (("hgs_hull_visibility", 14), ("hgs_lift_moments_gated", 17), ("hgs_lift_moments", 15)):
        assert hasattr(L, name) and len(rt.SIGNATURES[name][1]) == n_args
