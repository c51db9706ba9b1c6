"""utils/scalp.py on the CPU: the numpy path against the loop restatement of tests/scalp_reference.py (equal arrays), the depth maps'
edge cases against hand-computed expectations, a labelled cap and an occluder on a unit head, surface_samples, the init_scalp.py
driver, the Stage-II workflow it opens, and the binding's refusals."""
import ctypes
import os

import numpy as np
import pytest

from tests import carve_cases as CC
from tests import scalp_cases as SC
from tests import scalp_reference as REF

INF = float("inf")


@pytest.fixture(scope="module")
def cap():
    """The labelled cap: head, views, masks and label_scalp's result with the issue's knobs."""
    from utils import scalp
    verts, faces = SC.icosphere(3)
    views = SC.cap_views()
    masks = [SC.cap_mask(v) for v in views]
    points, vis, hits, kept = scalp.label_scalp(verts, faces, views, masks, 0.0, SC.MIN_COS, SC.DEPTH_TOL, 1, 70)
    return dict(verts=verts, faces=faces, views=views, masks=masks, points=points, vis=vis, hits=hits, kept=kept)


# ---- depth maps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.edge_faces(), ids=lambda c: c[0])
def test_depth_edge_cases(case):
    from utils import scalp
    name, _, want = case
    view = CC.identity_view(45, 31)
    verts, faces = SC.edge_mesh([name])
    (Z,), dropped = scalp.depth_maps(verts, faces, [view])
    (Zr,), dropped_r = REF.depth_maps(verts, faces, [view])
    assert Z.dtype == np.float64 and Z.shape == (31, 45)
    assert np.array_equal(Z, Zr) and dropped == dropped_r
    (Zf,), dropped_f = scalp.depth_maps(*SC.edge_mesh([name], flip=True), [view])      # the other winding
    assert np.array_equal(Z, Zf) and dropped == dropped_f
    if want == ("dropped",):
        assert dropped == 1 and np.isinf(Z).all()
        return
    assert dropped == 0
    if want == "row":
        ys, xs = np.nonzero(np.isfinite(Z))
        assert set(ys) == {4} and xs.size > 20 and (Z[ys, xs] == 2.0).all()
    elif "frame" in want:
        assert (Z == want["frame"]).all()
    else:
        expected = np.full((31, 45), INF)
        for (py, px), z in want.items():
            expected[py, px] = z
        assert np.array_equal(Z, expected)


def test_shared_edge_keeps_the_minimum_and_order_does_not_matter():
    from utils import scalp
    view = CC.identity_view(8, 6)
    verts, faces = SC.edge_mesh(["shared edge, near side", "shared edge, far side"])
    (Z,), _ = scalp.depth_maps(verts, faces, [view])
    expected = np.full((6, 8), INF)
    for py in range(4):
        for px in range(4):
            expected[py, px] = 2.0 if px >= py else 4.0                              # the diagonal's centres lie on both faces
    assert np.array_equal(Z, expected)
    (Z2,), _ = scalp.depth_maps(verts, faces[::-1], [view])
    assert np.array_equal(Z, Z2)


def test_slanted_face_interpolates_the_plane():
    """The plane z = 2 + 0.1 x meets the ray of the pixel centre (cx, cy) at z = 2/(1 - 0.1 cx)."""
    from utils import scalp
    view = CC.identity_view(8, 6)
    tri = [(u * 2.0 / (1.0 - 0.1 * u), v * 2.0 / (1.0 - 0.1 * u), 2.0 / (1.0 - 0.1 * u)) for u, v in ((-1.0, -1.0), (9.5, -1.0), (-1.0, 20.0))]
    (Z,), dropped = scalp.depth_maps(np.array(tri), np.array([[0, 1, 2]]), [view])
    (Zr,), _ = REF.depth_maps(np.array(tri), np.array([[0, 1, 2]]), [view])
    assert dropped == 0 and np.array_equal(Z, Zr)
    want = np.broadcast_to(2.0 / (1.0 - 0.1 * (np.arange(8) + 0.5)), (6, 8))
    inside = np.isfinite(Z)
    assert inside[:3, :4].all() and np.allclose(Z[inside], want[inside], rtol=1e-12, atol=0)


@pytest.mark.parametrize("V", [1, 3])
def test_numpy_path_equals_the_restatement(V):
    """All edge cases and random faces in one mesh, ring views of two sizes and the identity view; then the votes over its depth maps."""
    from utils import scalp
    views = CC.ring_views(V) + [CC.identity_view(45, 31)]
    verts, faces = SC.join(SC.edge_mesh(), SC.random_faces(40, seed=V), SC.random_faces(20, seed=7, centre=(40.0, 28.0, 2.0), spread=12.0, size=3.0))
    maps, dropped = scalp.depth_maps(verts, faces, views)
    maps_r, dropped_r = REF.depth_maps(verts, faces, views)
    assert dropped == dropped_r and dropped >= 4
    for a, b in zip(maps, maps_r):
        assert np.array_equal(a, b)
    assert all(np.isfinite(m).any() for m in maps)
    masks = CC.random_masks(views, 0.6, seed=3)
    border, _ = CC.border_points(45, 31)
    pts = np.concatenate([border, CC.cloud(60, seed=2, spread=0.8)])
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=pts.shape)
    nrm[::7] = 0.0
    nrm[3::11] = np.nan
    for min_cos, tol in ((0.0, 0.0), (0.25, 0.02), (1.0, 0.02)):
        vis, hits = scalp.scalp_votes(pts, nrm, views, masks, maps, min_cos, tol)
        vis_r, hits_r = REF.scalp_votes(pts, nrm, views, masks, maps, min_cos, tol)
        assert vis.dtype == np.int32 and np.array_equal(vis, vis_r) and np.array_equal(hits, hits_r)
        assert (vis[::7] == 0).all()                                                  # a zero normal faces nothing
        if min_cos == 0.0:
            assert vis.max() > 0 and hits.max() > 0 and (hits <= vis).all()


def test_bad_meshes_and_knobs_are_refused():
    from utils import scalp
    view = CC.identity_view(8, 6)
    tri = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    for verts, faces in ((tri, np.array([[0, 1, 3]])), (tri, np.array([[0, -1, 2]])), (tri, np.array([[0.0, 1.0, 2.0]])), (tri, np.array([0, 1, 2])),
                         (tri[:, :2], np.array([[0, 1, 2]])), (tri, np.zeros((1, 4), np.int64))):
        with pytest.raises(ValueError):
            scalp.depth_maps(verts, faces, [view])
        with pytest.raises(ValueError):
            scalp.surface_samples(verts, faces, 0.0)
    maps, dropped = scalp.depth_maps(tri, np.zeros((0, 3), np.int64), [view])       # no face: +inf
    assert dropped == 0 and np.isinf(maps[0]).all()
    mask = [np.ones((6, 8), np.uint8)]
    for min_cos, tol in ((-0.1, 0.0), (1.5, 0.0), (float("nan"), 0.0), (0.5, -1.0), (0.5, INF), (0.5, float("nan"))):
        with pytest.raises(ValueError):
            scalp.scalp_votes(tri, tri, [view], mask, maps, min_cos, tol)
    with pytest.raises(ValueError):
        scalp.scalp_votes(tri, tri, [view], mask, [maps[0][:, :4]], 0.5, 0.0)
    with pytest.raises(ValueError):
        scalp.depth_maps(tri, np.array([[0, 1, 2]]), [view], device="cpu")          # None or "cuda": nothing else
    assert scalp.view_batches([view] * 5, 8 * 48 * 2) == [(0, 2), (2, 4), (4, 5)]
    assert scalp.view_batches([view] * 3, 1) == [(0, 1), (1, 2), (2, 3)] and scalp.view_batches([view] * 3) == [(0, 3)]


# ---- labelled cap and occluder ---------------------------------------------------------------------------------------
def test_labelled_cap(cap):
    z = cap["verts"][:, 2]
    kept = cap["kept"]
    assert cap["verts"].shape == (642, 3) and cap["faces"].shape == (1280, 3)
    assert kept.any() and not (z[kept] < 0.15).any()
    assert kept[z > 0.35].all() and (z > 0.35).sum() > 100
    assert (cap["vis"] == 0).any()                                                   # (the underside: no camera looks up at it)
    assert np.array_equal(cap["points"], cap["verts"][kept])
    print(f"labelled cap: {int(kept.sum())} kept, {int((z > 0.35).sum())} above 0.35, {int((cap['vis'] == 0).sum())} never visible")


def test_occluder_hides_what_lies_behind_it(cap):
    from utils import scalp
    verts, faces, n_head = SC.head_and_ball()
    views = CC.ring_views(8, radius=3, sizes=((96, 80), (128, 96)), f_scale=1.1)
    masks = [np.full((v.H, v.W), 255, np.uint8) for v in views]
    head_v, head_f = cap["verts"], cap["faces"]
    r = SC.BALL_RADIUS
    hidden_by_ball = clear = 0
    for v, m in zip(views, masks):
        with_ball, _ = scalp.depth_maps(verts, faces, [v])
        alone, _ = scalp.depth_maps(head_v, head_f, [v])
        vis_b, _ = scalp.scalp_votes(head_v, head_v, [v], [m], with_ball, SC.MIN_COS, SC.DEPTH_TOL)
        vis_a, _ = scalp.scalp_votes(head_v, head_v, [v], [m], alone, SC.MIN_COS, SC.DEPTH_TOL)
        C = -(v.R.T @ v.t)
        seg = C - head_v                                                            # sample -> camera centre
        s = np.clip(((SC.BALL_CENTRE - head_v) * seg).sum(axis=1) / (seg * seg).sum(axis=1), 0.0, 1.0)
        dist = np.linalg.norm(head_v + s[:, None] * seg - SC.BALL_CENTRE, axis=1)
        assert not (vis_b[dist < 0.85 * r] != 0).any()
        assert not ((vis_a != 0) & (vis_b == 0) & (dist > 1.15 * r)).any()
        assert (vis_b <= vis_a).all()
        hidden_by_ball += int(((vis_a != 0) & (vis_b == 0)).sum())
        clear += int(((dist < 0.85 * r) & (vis_a != 0)).sum())
    assert hidden_by_ball > 0 and clear > 0
    print(f"occluder: {clear} clearly hidden (sample, view) pairs, {hidden_by_ball} pairs hidden by the ball alone")


# ---- surface samples -------------------------------------------------------------------------------------------------
def test_surface_samples(cap):
    from utils import scalp
    verts, faces = cap["verts"], cap["faces"]
    p0, n0 = scalp.surface_samples(verts, faces, 0.0)
    assert np.array_equal(p0, verts) and n0.shape == verts.shape
    assert ((n0 * verts).sum(axis=1) > 0).all()                                      # outwards, not normalised
    edges = np.linalg.norm(verts[faces] - verts[np.roll(faces, 1, axis=1)], axis=2)
    longest = edges.max(axis=1)
    F = faces.shape[0]
    for spacing, m in ((longest.max() * 1.01, 1), (longest.max() * 0.51, 2)):
        want_m = np.minimum(64, np.ceil(longest / spacing)).astype(int)
        assert (want_m == m).all()                                                   # (an icosphere's edges differ by a fifth at most)
        p, n = scalp.surface_samples(verts, faces, spacing)
        assert p.shape[0] == verts.shape[0] + int((want_m * want_m).sum()) and np.array_equal(p[:verts.shape[0]], verts)
        assert np.array_equal(n[:verts.shape[0]], n0)
    p1, n1 = scalp.surface_samples(verts, faces, longest.max() * 1.01)
    assert p1.shape[0] == verts.shape[0] + F
    assert np.allclose(p1[verts.shape[0]:], verts[faces].mean(axis=1), rtol=0, atol=1e-15)
    assert np.array_equal(n1[verts.shape[0]:], np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]]))
    # one face, m = 2 and the cap of 64: the centroids lie on the face, inside it, in the stated order
    tri = np.array([[0.0, 0.0, 1.0], [4.0, 0.0, 1.0], [0.0, 2.0, 3.0]])
    one = np.array([[0, 1, 2]])
    p2, n2 = scalp.surface_samples(tri, one, 2.3)                                    # longest edge sqrt(24) = 4.9: m = 3
    assert p2.shape[0] == 3 + 9
    p2, n2 = scalp.surface_samples(tri, one, 2.5)                                    # m = 2
    want = [(1 / 6, 1 / 6), (1 / 6, 4 / 6), (4 / 6, 1 / 6), (2 / 6, 2 / 6)]
    assert p2.shape[0] == 3 + 4
    assert np.allclose(p2[3:], [tri[0] + a * (tri[1] - tri[0]) + b * (tri[2] - tri[0]) for a, b in want], rtol=0, atol=1e-15)
    p64, n64 = scalp.surface_samples(tri, one, 1e-6)
    assert p64.shape[0] == 3 + 64 * 64
    normal = np.cross(tri[1] - tri[0], tri[2] - tri[0])
    assert (n64[3:] == normal).all()
    rel = p64[3:] - tri[0]
    assert np.abs(rel @ normal).max() < 1e-12                                        # on the plane
    ab = np.linalg.lstsq(np.stack([tri[1] - tri[0], tri[2] - tri[0]], axis=1), rel.T, rcond=None)[0]
    assert (ab > 0).all() and (ab.sum(axis=0) < 1).all()                             # strictly inside
    assert np.unique(np.round(p64[3:], 9), axis=0).shape[0] == 64 * 64
    assert np.allclose(p64[3:].mean(axis=0), tri.mean(axis=0), atol=1e-12)
    # a degenerate face adds nothing
    pd, _ = scalp.surface_samples(np.array([[0.0, 0.0, 0.0]]), np.array([[0, 0, 0]]), 0.1)
    assert pd.shape[0] == 1


# ---- driver ----------------------------------------------------------------------------------------------------------
def _args(extra=()):
    return ["--device", "cpu", "--min_views", "1", *extra]


def test_driver_writes_the_roots_file(tmp_path, capsys):
    import init_scalp
    from data.head_reconstruction_data import load_head_reconstruction_data_npz
    from utils import scalp
    src = str(tmp_path / "ply")
    views, masks, verts, faces = SC.build_scene(src)
    result = os.path.join(src, "head_reconstruction_data.npz")
    n = init_scalp.main(["-s", src, *_args()])
    out = capsys.readouterr().out
    assert "never visible" in out and "kept" in out and "dropped" in out and f"{n} scalp point(s)" in out
    with np.load(result) as d:
        assert sorted(d.files) == ["head_verts", "scalp_verts"]                     # what Scene loads
    head = load_head_reconstruction_data_npz(result)
    assert np.array_equal(head.head_verts, verts) and head.scalp_verts.shape == (n, 3) and n > 10
    diag = float(np.linalg.norm(verts.max(axis=0) - verts.min(axis=0)))
    want, _, _, kept = scalp.label_scalp(verts, faces, views, masks, 0.0, 0.25, 0.01 * diag, 1, 70)
    assert np.array_equal(head.scalp_verts, want)
    assert not (head.scalp_verts[:, 2] < 0.1).any() and kept[verts[:, 2] > 0.4].all()
    assert sorted(f for f in os.listdir(src) if f.startswith("head_rec")) == ["head_reconstruction_data.npz"]
    # a second run is refused; --overwrite keeps the first file once
    first = open(result, "rb").read()
    with pytest.raises(SystemExit, match="--overwrite"):
        init_scalp.main(["-s", src, *_args()])
    n2 = init_scalp.main(["-s", src, "--overwrite", "--max_points", "7", *_args(["--spacing", "0.2"])])
    assert n2 == 7 and load_head_reconstruction_data_npz(result).scalp_verts.shape == (7, 3)
    backup = os.path.join(src, "head_reconstruction_data.orig.npz")
    assert open(backup, "rb").read() == first
    init_scalp.main(["-s", src, "--overwrite", *_args(["--dilate", "1", "--depth_tol", "0.05"])])
    assert open(backup, "rb").read() == first                                        # written once
    # the same mesh as an OBJ gives the same points
    obj = str(tmp_path / "obj")
    SC.build_scene(obj, mesh="obj")
    with pytest.raises(SystemExit, match="head_mesh.ply is missing"):
        init_scalp.main(["-s", obj, *_args()])
    assert init_scalp.main(["-s", obj, "--mesh", os.path.join(obj, "head_mesh.obj"), *_args()]) == n
    other = load_head_reconstruction_data_npz(os.path.join(obj, "head_reconstruction_data.npz"))
    assert np.array_equal(other.scalp_verts, head.scalp_verts) and np.array_equal(other.head_verts, head.head_verts)


def test_driver_refusals(tmp_path):
    import init_scalp
    a, b = str(tmp_path / "opencv"), str(tmp_path / "empty")
    SC.build_scene(a, model="OPENCV")
    with pytest.raises(SystemExit, match="OPENCV.*undistort.py"):
        init_scalp.main(["-s", a, *_args()])
    views, masks, verts, faces = SC.build_scene(b)
    from PIL import Image as PILImage
    for v in views:
        PILImage.fromarray(np.zeros((v.H, v.W), np.uint8)).save(os.path.join(b, "masks", v.name))
    with pytest.raises(SystemExit, match="no sample is scalp.*--min_percent 70.*--min_cos"):
        init_scalp.main(["-s", b, *_args()])
    os.remove(os.path.join(b, "masks", "axis_2.png"))
    with pytest.raises(SystemExit, match="axis_2.png is missing"):
        init_scalp.main(["-s", b, *_args()])
    with pytest.raises(SystemExit, match="min_cos"):
        init_scalp.main(["-s", a, "--min_cos", "2", *_args()])
    for scene in (a, b):
        assert not os.path.exists(os.path.join(scene, "head_reconstruction_data.npz"))


# ---- workflow --------------------------------------------------------------------------------------------------------
def test_labelled_scalp_orients_the_strands(cap):
    """Strands rooted on the cap, every other one stored tip first: without roots compute_strands_info refuses, with the labelled scalp
    as ref_strand_root it walks every strand root -> tip."""
    from scene.hair_gaussian_model import HairGaussianModel
    roots = cap["verts"][cap["verts"][:, 2] > 0.5][::4]
    S, n = roots.shape[0], 5
    strands = roots[:, None, :] * (1.0 + 0.05 * np.arange(n))[None, :, None]        # straight out of the head
    strands[1::2] = strands[1::2, ::-1]
    m = HairGaussianModel.from_strands(strands.astype(np.float32), device="cpu")
    m.ref_strand_root = np.empty(0)                                                  # a capture without head_reconstruction_data.npz
    with pytest.raises(ValueError, match="ref_strand_root is not set"):
        m.compute_strands_info()
    m.ref_strand_root = cap["points"]
    m.compute_strands_info()
    info = m.strands_info
    assert info.n_strands == S
    first = info.rows[info.offsets[:-1], 0]                                          # every strand's first endpoint
    last = info.rows[info.offsets[1:] - 1, 1]
    ep = m._endpoints.detach().numpy()
    assert np.allclose(np.linalg.norm(ep[first], axis=1), 1.0, atol=1e-5)            # on the head
    assert np.allclose(np.linalg.norm(ep[last], axis=1), 1.2, atol=1e-5)             # the tips


# ---- binding ---------------------------------------------------------------------------------------------------------
def test_binding_symbols_and_refusals():
    import hgs_runtime as rt
    rt.build()
    L = rt.lib()
    assert len(rt.SIGNATURES["hgs_scalp_depth"][1]) == 9 and len(rt.SIGNATURES["hgs_scalp_votes"][1]) == 12
    assert hasattr(L, "hgs_scalp_depth") and hasattr(L, "hgs_scalp_votes")
    assert rt.ABI_VERSION == 15 and L.hgs_abi_version() == 15
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                                        # (never dereferenced: every call below is refused first)

    def depth(NV=3, verts=p, F=1, faces=p, V=1, views=p, out=p, dropped=p):
        assert L.hgs_scalp_depth(None, NV, verts, F, faces, V, views, out, dropped) != 0
        return L.hgs_last_error().decode()

    def votes(N=4, points=p, normals=p, V=1, views=p, masks=p, dep=p, min_cos=0.25, tol=0.0, vis=p, hits=p):
        assert L.hgs_scalp_votes(None, N, points, normals, V, views, masks, dep, min_cos, tol, vis, hits) != 0
        return L.hgs_last_error().decode()
    for kw in (dict(V=0), dict(V=4097)):
        assert depth(**kw).startswith("hgs_scalp_depth: V = ") and votes(**kw).startswith("hgs_scalp_votes: V = ")
    assert depth(NV=(1 << 24) + 1).startswith("hgs_scalp_depth: NV = ") and depth(NV=-1).startswith("hgs_scalp_depth: NV = ")
    assert depth(F=(1 << 24) + 1).startswith("hgs_scalp_depth: F = ") and depth(F=-1).startswith("hgs_scalp_depth: F = ")
    assert depth(NV=0).startswith("hgs_scalp_depth: F = 1 faces of no vertex")
    for kw in (dict(verts=None), dict(faces=None), dict(views=None), dict(out=None), dict(dropped=None)):
        assert depth(**kw) == "hgs_scalp_depth: null argument"
    assert votes(N=-1).startswith("hgs_scalp_votes: N = ")
    for c in (-0.01, 1.01, float("nan")):
        assert votes(min_cos=c).startswith("hgs_scalp_votes: min_cos = ")
    for t in (-1.0, INF, float("nan")):
        assert votes(tol=t).startswith("hgs_scalp_votes: depth_tol = ")
    for kw in (dict(points=None), dict(normals=None), dict(views=None), dict(masks=None), dict(dep=None), dict(vis=None), dict(hits=None)):
        assert votes(**kw) == "hgs_scalp_votes: null argument"
    assert L.hgs_scalp_votes(None, 0, None, None, 1, None, None, None, 0.25, 0.0, None, None) == 0    # N == 0 launches nothing
