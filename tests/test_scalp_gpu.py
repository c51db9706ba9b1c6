"""hgs_scalp_depth and hgs_scalp_votes (csrc/hgs_scalp.hip) against the numpy path of utils/scalp.py: equal arrays, no tolerance, at the
smallest shapes where the kernels can go wrong -- face and sample counts around the 64-lane wavefront, 1 / 3 / 7 views of two sizes,
every edge case of the depth maps, one face over the whole frame and one over a single pixel row, permuted faces -- and label_scalp
and the init_scalp.py driver, whose result is the same on both devices and under any batching of the views."""
import os

import numpy as np
import pytest
import torch

from tests import carve_cases as CC
from tests import scalp_cases as SC

pytestmark = pytest.mark.gpu


def _depth_views(V):
    """V - 1 ring views (45 x 31 and 64 x 48 in turn) and the identity view that the edge cases are made for."""
    return CC.ring_views(V - 1) + [CC.identity_view(*CC.SIZES[(V - 1) % 2])] if V > 1 else [CC.identity_view(64, 48)]


def _depth_mesh(F):
    """F faces: the edge cases first, then small random faces around the ring's centre and in front of the identity view."""
    edge = SC.edge_mesh()
    n = max(0, F - edge[1].shape[0])
    verts, faces = SC.join(edge, SC.random_faces(n - n // 3, seed=F), SC.random_faces(n // 3, seed=F + 1, centre=(40.0, 28.0, 2.0), spread=12.0, size=3.0))
    faces = faces[:F]
    return verts, faces


@pytest.fixture(scope="module")
def depth_reference():
    """{(F, V): (verts, faces, views, maps, dropped)} of the numpy path, computed once."""
    from utils import scalp
    out = {}
    for F in (0, 1, 63, 64, 65, 1000):
        for V in (1, 3, 7):
            verts, faces = _depth_mesh(F)
            views = _depth_views(V)
            out[F, V] = (verts, faces, views) + scalp.depth_numpy(verts, faces, views)
    return out


def _device_maps(verts, faces, views):
    from utils import carve, scalp
    packed = carve.pack(views, [np.zeros((v.H, v.W), np.uint8) for v in views], None, "cuda")
    depth, dropped = scalp.depth_device(torch.from_numpy(verts).cuda(), torch.from_numpy(faces.astype(np.int32)).cuda(), packed)
    assert depth.dtype == torch.float64 and depth.numel() == sum(v.W * v.H for v in views)
    return scalp._split(depth, packed.records), dropped


@pytest.mark.parametrize("V", [1, 3, 7])
@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 1000])
def test_depth_equals_the_numpy_path(depth_reference, F, V):
    verts, faces, views, want, want_dropped = depth_reference[F, V]
    got, dropped = _device_maps(verts, faces, views)
    assert dropped == want_dropped
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (k, int((g != w).sum()))
    if F == 0:
        assert all(np.isinf(g).all() for g in got) and dropped == 0
    if F >= 63:
        assert dropped > 0 and np.isfinite(want[-1]).all()                           # (the identity view: one face covers its frame)
        assert all(np.isfinite(w).any() and (V == 1 or np.isinf(w).any()) for w in want[:-1] or want)
    # the same faces in another order: the same maps
    perm = np.random.default_rng(F + V).permutation(faces.shape[0])
    again, dropped2 = _device_maps(verts, faces[perm], views)
    assert dropped2 == want_dropped and all(np.array_equal(a, w) for a, w in zip(again, want))


def test_whole_frame_and_single_row():
    from utils import scalp
    view = CC.identity_view(64, 48)
    for name in ("larger than the frame", "one pixel row"):
        verts, faces = SC.edge_mesh([name])
        (want,), _ = scalp.depth_numpy(verts, faces, [view])
        (got,), dropped = _device_maps(verts, faces, [view])
        assert dropped == 0 and np.array_equal(got, want)
        if name == "one pixel row":
            assert set(np.nonzero(np.isfinite(got))[0]) == {4}
        else:
            assert (got == 2.0).all()


def _vote_inputs():
    """Views of both sizes with the identity view of the border cases, a mesh that hides part of the samples, and 1000 samples: the
    border points, NaN / Inf points and points behind a camera first; some normals zero or NaN."""
    views = CC.ring_views(3) + [CC.identity_view(45, 31)]
    verts, faces = SC.join(SC.icosphere(1, 0.6), SC.random_faces(30, seed=3, centre=(20.0, 14.0, 3.0), spread=6.0, size=4.0))
    border, _ = CC.border_points(45, 31)
    behind = np.array([[4.0, 0.0, 0.0], [0.0, 5.0, 0.2], [-6.0, 1.0, 0.3]])
    sphere, _ = SC.icosphere(2, 0.6)
    pts = np.concatenate([border, behind, sphere, CC.cloud(1000, seed=8)])[:1000]
    nrm = np.random.default_rng(9).normal(size=pts.shape)
    k = border.shape[0] + 3
    nrm[:border.shape[0]] = (0.0, 0.0, -1.0)                                         # towards the identity camera
    nrm[k:k + sphere.shape[0]] = sphere                                              # the sphere's own normals
    nrm[5::13] = 0.0
    nrm[6::17] = np.nan
    return views, verts, faces, np.ascontiguousarray(pts), np.ascontiguousarray(nrm)


@pytest.fixture(scope="module")
def vote_reference():
    from utils import scalp
    views, verts, faces, pts, nrm = _vote_inputs()
    maps, _ = scalp.depth_numpy(verts, faces, views)
    masks = {d: CC.random_masks(views, d, seed=5) for d in (0.3, 0.9)}
    want = {(d, c, t): scalp.votes_numpy(pts, nrm, views, masks[d], maps, c, t) for d in masks for c in (0.0, 0.25, 1.0) for t in (0.0, 0.02)}
    return views, maps, masks, pts, nrm, want


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 1000])
def test_votes_equal_the_numpy_path(vote_reference, N):
    from utils import carve, scalp
    views, maps, masks, pts, nrm, want = vote_reference
    p, n = torch.from_numpy(pts[:N]).cuda(), torch.from_numpy(nrm[:N]).cuda()
    depth = torch.from_numpy(np.concatenate([m.reshape(-1) for m in maps])).cuda()
    some_vis = some_fewer = 0
    for density in (0.3, 0.9):
        packed = carve.pack(views, masks[density], None, "cuda")
        for min_cos in (0.0, 0.25, 1.0):
            for tol in (0.0, 0.02):
                vis, hits = scalp.votes_device(p, n, packed, depth, min_cos, tol)
                w_vis, w_hits = want[density, min_cos, tol]
                assert vis.dtype == torch.int32 and hits.dtype == torch.int32 and vis.shape == (N,)
                assert np.array_equal(vis.cpu().numpy(), w_vis[:N]) and np.array_equal(hits.cpu().numpy(), w_hits[:N]), (density, min_cos, tol)
                some_vis += int(w_vis[:N].sum())
                some_fewer += int((want[density, 0.0, 0.02][0][:N] > w_vis[:N]).sum())
    if N >= 63:
        assert some_vis > 0 and some_fewer > 0
    if N == 1000:                                                                     # the cases discriminate
        a, b = want[0.3, 0.0, 0.0], want[0.9, 0.0, 0.02]
        assert (a[0] != b[0]).any() and (a[1] < a[0]).any() and (want[0.3, 0.25, 0.02][0] != want[0.3, 1.0, 0.02][0]).any()


def test_entry_points_and_refusals():
    from utils import carve, scalp
    import hgs_runtime as rt
    views = CC.ring_views(3)
    masks = CC.random_masks(views, 0.5, seed=1)
    verts, faces = SC.icosphere(1, 0.7)
    maps, dropped = scalp.depth_maps(verts, faces, views, device="cuda")
    want, want_dropped = scalp.depth_maps(verts, faces, views)
    assert dropped == want_dropped and all(np.array_equal(a, b) for a, b in zip(maps, want))
    tiny, _ = scalp.depth_maps(verts, faces, views, device="cuda", budget=1)         # one view per batch
    assert all(np.array_equal(a, b) for a, b in zip(tiny, want))
    got = scalp.scalp_votes(verts, verts, views, masks, maps, 0.25, 0.02, device="cuda", budget=8 * 64 * 48)
    ref = scalp.scalp_votes(verts, verts, views, masks, want, 0.25, 0.02)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and ref[0].max() > 0
    packed = carve.pack(views, masks, None, "cuda")
    v_dev, f_dev = torch.from_numpy(verts).cuda(), torch.from_numpy(faces.astype(np.int32)).cuda()
    depth, _ = scalp.depth_device(v_dev, f_dev, packed)
    bad = f_dev.clone()
    bad[3, 1] = verts.shape[0]
    with pytest.raises(rt.HgsError, match="out of range"):
        scalp.depth_device(v_dev, bad, packed)
    with pytest.raises(rt.HgsError):
        scalp.depth_device(v_dev.float(), f_dev, packed)
    with pytest.raises(rt.HgsError):
        scalp.depth_device(v_dev, f_dev.long(), packed)
    with pytest.raises(rt.HgsError, match="depth"):                                  # a depth buffer shorter than offset + W*H
        scalp.votes_device(v_dev, v_dev, packed, depth[:-1].contiguous(), 0.25, 0.02)
    with pytest.raises(rt.HgsError, match="hgs_scalp_votes: min_cos"):
        scalp.votes_device(v_dev, v_dev, packed, depth, 1.5, 0.02)
    with pytest.raises(rt.HgsError, match="hgs_scalp_votes: depth_tol"):
        scalp.votes_device(v_dev, v_dev, packed, depth, 0.5, -1.0)
    with pytest.raises(rt.HgsError):
        scalp.votes_device(v_dev, v_dev[:-1].contiguous(), packed, depth, 0.5, 0.0)


@pytest.fixture(scope="module")
def cap_inputs():
    verts, faces = SC.icosphere(3)
    views = SC.cap_views()
    return verts, faces, views, [SC.cap_mask(v) for v in views]


@pytest.mark.parametrize("case", ["cap", "occluder", "spacing"])
def test_label_scalp_equals_the_numpy_path(cap_inputs, case):
    from utils import scalp
    verts, faces, views, masks = cap_inputs
    spacing, min_views = 0.0, 1
    if case == "occluder":
        verts, faces, _ = SC.head_and_ball()
        views = views[:8]
        masks = [np.full((v.H, v.W), 255, np.uint8) for v in views]
    if case == "spacing":
        spacing, min_views = 0.08, 2
    want = scalp.label_scalp(verts, faces, views, masks, spacing, SC.MIN_COS, SC.DEPTH_TOL, min_views, 70)
    stats = {}
    got = scalp.label_scalp(verts, faces, views, masks, spacing, SC.MIN_COS, SC.DEPTH_TOL, min_views, 70, device="cuda", stats=stats)
    three = scalp.label_scalp(verts, faces, views, masks, spacing, SC.MIN_COS, SC.DEPTH_TOL, min_views, 70, device="cuda", budget=3 * 8 * 128 * 96)
    single = scalp.label_scalp(verts, faces, views, masks, spacing, SC.MIN_COS, SC.DEPTH_TOL, min_views, 70, device="cuda", budget=1)
    for g, t, s, w in zip(got, three, single, want):
        assert g.dtype == w.dtype and np.array_equal(g, w) and np.array_equal(t, w) and np.array_equal(s, w)
    assert stats["dropped"] == 0 and want[3].any() and not want[3].all()
    assert 3 <= len(scalp.view_batches(views, 3 * 8 * 128 * 96)) < len(views) == len(scalp.view_batches(views, 1))


def test_driver_writes_the_same_file_on_both_devices(tmp_path):
    import init_scalp
    files = {}
    for device in ("cuda", "cpu"):
        src = str(tmp_path / device)
        SC.build_scene(src)
        n = init_scalp.main(["-s", src, "--device", device, "--min_views", "1", "--spacing", "0.2", "--dilate", "1"])
        path = os.path.join(src, "head_reconstruction_data.npz")
        with open(path, "rb") as fh:
            files[device] = fh.read()
        with np.load(path) as d:
            assert n > 10 and d["scalp_verts"].shape == (n, 3) and d["scalp_verts"].dtype == np.float64
    assert files["cuda"] == files["cpu"]                     # (np.savez stamps its members 1980-01-01, not the clock: the bytes repeat)
