"""Point-cloud normals on the GPU (csrc/hgs_normals.hip through utils.normals) against the host path and plain numpy / scipy
restatements (tests/normals_fixtures.py).  Only test_reproducible compares the device code with itself, and says so.

Conditions (caps, not measurements): a point is TIED when the K-th and (K+1)-th distances of cKDTree.query(k=K+1) are within
1e-12 relative, FRAGILE IN SIGN when a non-self neighbour has |proj| <= 1e-12 sqrt(l2) under the host normal.  Tied points are
left out of the neighbour-set and normal comparisons, fragile ones out of the sign comparison; on the five non-lattice inputs
the reference excludes NO point, which every test asserts first.  Direction: |n_dev x n_host| <= 1e-14 / g, g = (l1 - l0) /
(l0 + l1 + l2) of the host-order covariance of the reference neighbours (eigenvector perturbation = matrix error / gap; two
independent float64 statements of the algorithm differ by 3.1e-16 / g on these inputs; the factor ~32 allows for another sweep
count and reduction shape).  Length: | |n| - 1 | <= 4 * 2^-52 everywhere."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import normals_fixtures as F

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(inp, K, shift=False):
    p = F.cloud(inp)
    if shift:
        p = (p.astype(np.float64) + np.array([100.0, -50.0, 25.0])).astype(np.float32)
    return F.reference(p, K)


def _device(p, K=50, neighbors=True):
    import torch
    from utils.normals import estimate_pointcloud_normals_device
    out = estimate_pointcloud_normals_device(torch.from_numpy(np.ascontiguousarray(p)).cuda(), K, return_neighbors=neighbors)
    torch.cuda.synchronize()
    if neighbors:
        return out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.int64)
    return out.cpu().numpy()


def _check_unit(n):
    assert np.isfinite(n).all()
    err = np.abs(np.linalg.norm(n, axis=1) - 1.0).max() if n.shape[0] else 0.0
    print(f"  largest | |n| - 1 | = {err:.3e}")
    assert err <= F.UNIT_TOL


def _check_rows(ref, nb, K, expect_no_exclusion=True):
    p, N = ref["p"], ref["p"].shape[0]
    excluded = int(ref["tied"].sum())
    print(f"  tied (excluded) points: {excluded} of {N}")
    if expect_no_exclusion:
        assert excluded == 0
    else:
        assert excluded <= 1e-4 * N
    keep = ~ref["tied"]
    assert nb.shape == (N, K) and nb.min() >= 0 and nb.max() < N
    assert np.array_equal(np.sort(nb, axis=1)[keep], np.sort(ref["nb"][:, :K], axis=1)[keep])
    assert np.array_equal(nb[:, 0], np.arange(N))
    d2 = F.d2_rule1(p[:, None, :], p[nb])
    assert (np.diff(d2, axis=1) >= 0).all()


def _check_normals(ref, n, K):
    N = n.shape[0]
    keep = ~ref["tied"]
    assert int(ref["tied"].sum()) == 0 and int(ref["fragile"].sum()) == 0, (int(ref["tied"].sum()), int(ref["fragile"].sum()))
    _check_unit(n)
    cross = np.linalg.norm(np.cross(n, ref["n_host"]), axis=1)
    worst = (cross * ref["g"])[keep].max()
    print(f"  K = {K}: largest |n_dev x n_host| * g = {worst:.3e} (bound {F.DIRECTION_TOL:.0e}); smallest g = {ref['g'].min():.3e}")
    assert (cross[keep] <= F.DIRECTION_TOL / ref["g"][keep]).all()
    if K % 2 == 0:
        ok = keep & ~ref["fragile"]
        flipped = int(((n * ref["n_host"]).sum(axis=1)[ok] <= 0).sum())
        print(f"  sign mismatches: {flipped} of {int(ok.sum())}")
        assert flipped == 0
    c32 = int((n.astype(np.float32) != ref["n_host"].astype(np.float32)).sum())
    print(f"  float32-cast components that differ from the host path: {c32} of {3 * N}")


CASES = [(i, 50) for i in F.FIVE] + [("strands-50k", 3), ("strands-50k", 16), ("strands-50k", 64)]


@pytest.mark.parametrize("inp,K", CASES, ids=[f"{i}-K{k}" for i, k in CASES])
def test_neighbour_sets(inp, K):
    ref = _ref(inp, K)
    _, nb = _device(F.cloud(inp), K)
    _check_rows(ref, nb, K)


@pytest.mark.parametrize("K", [50, 7])
def test_ties_on_a_lattice(K):
    """The row of every point equals the (d2, index)-ordered brute force: its largest d2 is the K-th smallest, everything
    nearer is in it, at the K-th distance it holds the lowest indices, and equal distances stand in ascending index order."""
    p = F.cloud("lattice")
    n, nb = _device(p, K)
    want = F.brute_force_rows(p, K)
    p64 = p.astype(np.float64)
    d2 = F.d2_rule1(p64[:, None, :], p64[nb])
    d2w = F.d2_rule1(p64[:, None, :], p64[want])
    assert np.array_equal(d2[:, -1], d2w[:, -1])
    assert np.array_equal(nb, want)
    _check_unit(n)


NORMAL_CASES = [(i, 50) for i in F.FIVE] + [("strands-50k", 16), ("strands-50k", 64)]


@pytest.mark.parametrize("inp,K", NORMAL_CASES, ids=[f"{i}-K{k}" for i, k in NORMAL_CASES])
def test_normals(inp, K):
    ref = _ref(inp, K)
    n = _device(F.cloud(inp), K, neighbors=False)
    _check_normals(ref, n, K)


def test_reproducible():
    """The device path against itself: two calls are bitwise equal, and a permutation of the input permutes the output."""
    ref = _ref("cloud", 50)
    assert ref["distinct"].all()          # (reference side: no two of a point's K + 1 smallest distances are equal)
    p = F.cloud("cloud")
    n1, nb1 = _device(p)
    n2, nb2 = _device(p)
    assert n1.tobytes() == n2.tobytes() and np.array_equal(nb1, nb2)
    s = np.random.default_rng(7).permutation(p.shape[0])
    ns, nbs = _device(p[s])
    assert ns.tobytes() == n1[s].tobytes()
    assert np.array_equal(s[nbs], nb1[s])


@pytest.mark.parametrize("N", [0, 1, 2, 7, 64, 4097])
def test_small_and_odd_sizes(N):
    K = 64 if N == 64 else 50
    p = (np.random.default_rng(N).normal(size=(N, 3)) * 0.1).astype(np.float32)
    n, nb = _device(p, K)
    Kc = min(K, N)
    assert n.shape == (N, 3) and nb.shape == (N, Kc)
    _check_unit(n)
    if N:
        assert np.array_equal(nb, F.brute_force_rows(p, Kc))
    if N == 7:
        assert np.array_equal(np.sort(nb, axis=1), np.tile(np.arange(7), (7, 1)))


def test_far_from_the_origin():
    ref = _ref("cloud", 50, True)
    p = ref["p"].astype(np.float32)
    assert np.array_equal(p.astype(np.float64), ref["p"])
    n, nb = _device(p)
    _check_rows(ref, nb, 50)
    _check_unit(n)


def test_duplicated_points():
    """cloud[:5000] and 500 exact copies of its point 0: every copy's row is the 50 lowest indices of the copies."""
    base = F.cloud("cloud")[:5000]
    p = np.concatenate([base, np.repeat(base[:1], 500, axis=0)], axis=0)
    n, nb = _device(p)
    _check_unit(n)
    copies = np.concatenate([[0], np.arange(5000, 5500)])
    assert np.array_equal(nb[copies], np.tile(copies[:50], (copies.shape[0], 1)))
    assert np.array_equal(nb, F.brute_force_rows(p, 50))


def test_errors_before_any_launch(monkeypatch):
    import hgs_runtime as rt
    import torch
    from utils.normals import estimate_pointcloud_normals, estimate_pointcloud_normals_device
    L = rt.lib()
    p = torch.from_numpy(F.cloud("cloud")[:1000]).cuda()

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")
    with monkeypatch.context() as m:
        m.setattr(rt, "lib", lambda: NoLaunch())
        with pytest.raises(ValueError):
            estimate_pointcloud_normals_device(p, 65)
        with pytest.raises(ValueError):
            estimate_pointcloud_normals_device(p[:, :2])
        for bad in (float("nan"), float("inf")):
            q = p.clone()
            q[3, 2] = bad
            with pytest.raises(ValueError):
                estimate_pointcloud_normals_device(q)
            with pytest.raises(ValueError):
                estimate_pointcloud_normals(q.cpu().numpy(), device="cuda")
        with pytest.raises(TypeError):
            estimate_pointcloud_normals_device(p.cpu())
        assert estimate_pointcloud_normals_device(p[:0]).shape == (0, 3)
    # the C entry itself
    p64 = p.double().contiguous()
    out = torch.full((1000, 3), 7.0, dtype=torch.float64, device="cuda")
    nbytes = int(L.hgs_pointcloud_normals_scratch_bytes(1000, 50))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    s = rt.current_stream()

    def refused(N, K, pts, nrm, scr, size, word):
        assert L.hgs_pointcloud_normals(s, N, K, pts, nrm, None, scr, size) != 0
        assert word in L.hgs_last_error().decode()
    refused(1000, 65, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch), nbytes, "K = 65")
    refused(1000, 0, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch), nbytes, "K = 0")
    refused(40, 50, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch), nbytes, "exceeds")
    refused(-1, 50, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch), nbytes, "N = -1")
    refused(1000, 50, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch), nbytes - 256, "scratch")
    refused(1000, 50, rt.ptr(p64), rt.ptr(out), rt.ptr(scratch) + 8, nbytes, "scratch")
    refused(1000, 50, None, rt.ptr(out), rt.ptr(scratch), nbytes, "null")
    assert L.hgs_pointcloud_normals(s, 0, 50, None, None, None, None, ctypes.c_size_t(0)) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_hair_loader(tmp_path):
    from data.hair_data import load_hair_from_usc_dataset
    from tests.synth_fixtures import write_usc
    path = str(tmp_path / "strands.data")
    write_usc(path, n_long=200, seed=2)
    host = load_hair_from_usc_dataset(path, normal_required=True)
    dev = load_hair_from_usc_dataset(path, normal_required=True, normals_device="cuda")
    assert np.array_equal(host.verts, dev.verts) and dev.normals.dtype == np.float64 and dev.normals.shape == host.normals.shape
    ref = F.reference(host.verts, 50)
    assert np.array_equal(ref["n_host"], host.normals)
    N = host.verts.shape[0]
    excluded = int((ref["tied"] | ref["fragile"]).sum())
    print(f"  loader: {excluded} of {N} point(s) tied or fragile")
    assert excluded <= 1e-4 * N
    keep = ~ref["tied"]
    _check_unit(dev.normals)
    cross = np.linalg.norm(np.cross(dev.normals, host.normals), axis=1)
    print(f"  loader: largest |n_dev x n_host| * g = {(cross * ref['g'])[keep].max():.3e}")
    assert (cross[keep] <= F.DIRECTION_TOL / ref["g"][keep]).all()
    ok = keep & ~ref["fragile"]
    assert ((dev.normals * host.normals).sum(axis=1)[ok] > 0).all()


def _synth(tmp_path, normals, W=128, H=96, cams=4):
    import synthesize
    from tests.synth_fixtures import sphere_mesh, write_obj, write_usc
    hair, head = tmp_path / "strands.data", tmp_path / "head.obj"
    if not hair.exists():
        write_usc(str(hair), n_long=200, seed=2)
        v, f, n = sphere_mesh()
        write_obj(str(head), v, f, n)
    out = tmp_path / f"scene_{normals}"
    synthesize.main(["--dataset", "usc_hair_salon", "--hair", str(hair), "--head", str(head), "-o", str(out), "--pct_strands", "2",
                     "--cameras", str(cams), "--height", str(H), "--width", str(W), "--cam_z", "0.45", "--device", "cuda",
                     "--normals", normals])
    return out


def test_driver_device_normals(tmp_path, capsys):
    from PIL import Image as PILImage
    from data.hair_data import load_hair_from_usc_dataset
    host = _synth(tmp_path, "host")
    assert "normals: host" in capsys.readouterr().out
    dev = _synth(tmp_path, "device")
    assert "normals: device" in capsys.readouterr().out
    names = sorted(os.listdir(host / "masks"))
    assert names == sorted(os.listdir(dev / "masks")) and len(names) == 4
    for n in names:
        assert (host / "masks" / n).read_bytes() == (dev / "masks" / n).read_bytes(), n
    for n in ("sparse/0/cameras.bin", "sparse/0/images.bin", "sparse/0/points3D.bin", "hair_eval_data.npz",
              "head_reconstruction_data.npz"):
        assert (host / n).read_bytes() == (dev / n).read_bytes(), n
    differing = total = 0
    for n in sorted(os.listdir(host / "images")):
        a = np.asarray(PILImage.open(host / "images" / n)).astype(np.int32)
        b = np.asarray(PILImage.open(dev / "images" / n)).astype(np.int32)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1, n
        differing += int((a != b).sum())
        total += a.size
    path = str(tmp_path / "strands.data")
    hn = load_hair_from_usc_dataset(path, normal_required=True, pct_strands=2).normals.astype(np.float32)
    dn = load_hair_from_usc_dataset(path, normal_required=True, pct_strands=2, normals_device="cuda").normals.astype(np.float32)
    c32 = int((hn != dn).sum())
    print(f"  images: {differing} of {total} byte(s) differ; float32 normal components: {c32} of {hn.size} differ")
    assert c32 <= 1e-4 * hn.size
