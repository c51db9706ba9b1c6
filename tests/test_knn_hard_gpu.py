"""The four neighbour searches of csrc/hgs_knn.hip on the degenerate clouds of tests/knn_cases.py, through the public wrappers,
against the brute forces of tests/knn_reference.py: distCUDA2, knn3_self and the radius pairs bit for bit against the float32
statement (and within the derived 9 u / 6 u of float64), nearest_distance bit for bit against float64.  No comparison carries an
exclusion.  tests/test_knn_hard_cpu.py checks the references against each other."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hgs_oracle as O
from tests import knn_cases as KC
from tests import knn_reference as KR

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dist2_twice(p):
    """distCUDA2 called twice on the same cloud: the cell table is built with atomics and has to be order-independent."""
    from simple_knn._C import distCUDA2
    t = torch.from_numpy(p).cuda()
    a = distCUDA2(t).cpu().numpy()
    b = distCUDA2(t).cpu().numpy()
    assert np.array_equal(_bits(a), _bits(b)), "two calls differ"
    return a


# ---- distCUDA2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.NAMES)
def test_dist2_on_every_family(name):
    p = KC.small(name)
    got = _dist2_twice(p)
    b32 = KR.brute_dist2_f32(p)
    b64 = KR.brute_dist2_f64(p)
    diff = int((_bits(got) != _bits(b32)).sum())
    fin = np.isfinite(b64) & (b64 > 0)
    worst = float((np.abs(got[fin].astype(np.float64) - b64[fin]) / b64[fin]).max() / KR.U) if fin.any() else 0.0
    print(f"KNN_GPU dist2 {name} P={p.shape[0]} differing words={diff} worst vs float64={worst:.3f} u")
    assert diff == 0
    assert KR.within(got, b64, 9).all() and np.array_equal(got == 0, b64 == 0)


@pytest.mark.parametrize("P", KC.LARGE_SIZES)
@pytest.mark.parametrize("name", KC.LARGE_FAMILIES)
def test_dist2_where_the_grid_level_changes(name, P):
    p = KC.large(name, P)
    got = _dist2_twice(p)
    ref = O.dist2(p)
    diff = int((_bits(got) != _bits(ref)).sum())
    print(f"KNN_GPU dist2 {name} P={P} differing words={diff}")
    assert diff == 0


def test_dist2_on_the_margin_cloud():
    """A third neighbour in the next cell, one rounding beyond the unpadded radius (tests/knn_cases.py margin_cloud)."""
    p = KC.margin_cloud()
    got = _dist2_twice(p)
    assert np.array_equal(_bits(got), _bits(KR.brute_dist2_f32(p)))


def test_dist2_non_finite_points_are_invisible():
    p = KC.small("non_finite")
    rows = list(KC.NON_FINITE_ROWS)
    got = _dist2_twice(p)
    assert np.array_equal(_bits(got), _bits(O.dist2(p)))
    keep = np.ones(p.shape[0], bool)
    keep[rows] = False
    sub = _dist2_twice(np.ascontiguousarray(p[keep]))
    assert np.array_equal(_bits(got[keep]), _bits(sub))
    assert np.isposinf(got[rows]).all()


def test_dist2_refuses_bad_scratch_before_any_launch():
    """hgs_launch_dist2 checks the scratch size and alignment before its first launch: a stated size one byte short and a pointer
    4 bytes off are refused with a message, and nothing is written.  (The buffers are as large as a good call needs.)"""
    import hgs_runtime as rt
    L = rt.lib()
    P = 1000
    pts = torch.from_numpy(KC.octants(P, 1)).cuda()
    need = L.hgs_dist2_scratch_bytes(P)
    scratch = torch.zeros((need + 512,), dtype=torch.uint8, device="cuda")
    base = (scratch.data_ptr() + 255) & ~255
    out = torch.full((P,), -7.0, dtype=torch.float32, device="cuda")
    with torch.cuda.device(pts.device):
        st = L.hgs_dist2(rt.current_stream(), P, rt.ptr(pts), rt.ptr(out), C.c_void_p(base), need - 1)
        assert st != 0
        msg = L.hgs_last_error().decode()
        assert "hgs_dist2" in msg and str(need) in msg and str(need - 1) in msg
        st = L.hgs_dist2(rt.current_stream(), P, rt.ptr(pts), rt.ptr(out), C.c_void_p(base + 4), need)
        assert st != 0 and "aligned" in L.hgs_last_error().decode()
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((scratch == 0).all())
        rt.check(L.hgs_dist2(rt.current_stream(), P, rt.ptr(pts), rt.ptr(out), C.c_void_p(base), need))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(O.dist2(pts.cpu().numpy())))


# ---- knn3_self ------------------------------------------------------------------------------------------------------------
def _knn3_check(p):
    from loss.losses import knn3_self
    d2, idx = knn3_self(torch.from_numpy(p).cuda())
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    rd2, ridx = KR.brute_knn3_f32(p)
    d64, _ = KR.brute_knn3_f64(p)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(_bits(d2), _bits(rd2))
    assert KR.within(d2, d64, 6).all() and np.array_equal(d2 == 0, d64 == 0)
    return d2, idx


@pytest.mark.parametrize("n", KC.KNN3_SIZES)
@pytest.mark.parametrize("name", KC.KNN3_FAMILIES)
def test_knn3_on_the_hard_families(name, n):
    p = KC.knn3_case(name, n)
    d2, idx = _knn3_check(p)
    if name == "non_finite":
        bad = KC.knn3_non_finite_rows(n)
        assert len(bad) >= 4 and not np.isfinite(p[bad]).all(axis=1).any()
        assert (idx[bad] == -1).all() and np.isposinf(d2[bad]).all()      # the documented row of a non-finite point
        assert not np.isin(idx, bad).any()                                # and it is nobody's neighbour
        rest = np.delete(np.arange(n), bad)
        assert (idx[rest] >= 0).all() and np.isfinite(d2[rest]).all()


def test_knn3_ties_across_tile_boundaries():
    p = KC.knn3_tile_ties()
    d2, idx = _knn3_check(p)
    assert idx[254:259].tolist() == [[254, 255, 256]] * 5 and idx[510:515].tolist() == [[510, 511, 512]] * 5


# ---- the radius pairs ---------------------------------------------------------------------------------------------------------
_PAIR_REF = {}


def _pair_ref(name):
    if name not in _PAIR_REF:
        pos, dirs, r, min_cos, bidir, _ = KC.pair_cases()[name]
        _PAIR_REF[name] = KR.brute_pairs_f32(pos, dirs, r, min_cos, bidir)
    return _PAIR_REF[name]


def _abi_pairs(pos, dirs, r, min_cos, bidir, sorted_by_x):
    """hgs_radius_pairs called directly on positions sorted by x here (a stable numpy sort), with the callers' capacity rule:
    (pairs in the caller's indices, a < b, in lexicographic order; the kernel's distances in that order; launches)."""
    import hgs_runtime as rt
    order = np.argsort(pos[:, 0], kind="stable")
    ps, ds = torch.from_numpy(pos[order]).cuda(), torch.from_numpy(dirs[order]).cuda()
    n = pos.shape[0]
    cap, launches = max(4 * n, 1024), 0
    while True:
        pairs = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((cap,), dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt.check(rt.lib().hgs_radius_pairs(rt.current_stream(), n, rt.ptr(ps), rt.ptr(ds), float(r), float(min_cos), int(bidir), cap,
                                           rt.ptr(pairs), rt.ptr(dist), rt.ptr(count), int(sorted_by_x)))
        launches += 1
        found = int(count.item())
        if found <= cap:
            break
        cap = found
    pr = order[pairs[:found].cpu().numpy().astype(np.int64)].reshape(-1, 2)
    pr = np.stack([pr.min(axis=1), pr.max(axis=1)], 1)
    o = np.lexsort((pr[:, 1], pr[:, 0]))
    return pr[o], dist[:found].cpu().numpy()[o], launches


@pytest.mark.parametrize("name", KC.PAIR_NAMES)
def test_radius_pairs_equal_the_float32_statement(name):
    from scene.hair_topology import HairTopologyMixin
    pos, dirs, r, min_cos, bidir, _ = KC.pair_cases()[name]
    want, want_d = _pair_ref(name)
    a, b = HairTopologyMixin._radius_pairs_gpu(torch.from_numpy(pos).cuda(), torch.from_numpy(dirs).cuda(), r, min_cos, bidir)
    got = np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], 1).reshape(-1, 2)
    got = got[np.lexsort((got[:, 1], got[:, 0]))]
    print(f"KNN_GPU pairs {name} N={pos.shape[0]} want={len(want)} got={len(got)}")
    assert np.array_equal(got, want)
    for sorted_by_x in (1, 0):                 # the early exit on and off: the same pairs, the same distances
        pr, d, launches = _abi_pairs(pos, dirs, r, min_cos, bidir, sorted_by_x)
        assert np.array_equal(pr, want), sorted_by_x
        assert np.array_equal(_bits(d), _bits(want_d)), sorted_by_x
        assert launches == (2 if len(want) > max(4 * pos.shape[0], 1024) else 1)


def test_merge_of_a_dense_cluster_gpu_model_equals_cpu_model(monkeypatch):
    """64 strand tips within a quarter of merge_dist_th of one point: 2016 candidate pairs against the first capacity of 1024 in
    _merge_candidates_device, so its second launch runs (counted here); the GPU model merges what the CPU model merges."""
    import hgs_runtime as rt
    from arguments import OptimizationParams
    from scene.hair_gaussian_model import HairGaussianModel
    pts, roots = KC.merge_cluster_strands()
    L = rt.lib()
    real, calls = L.hgs_radius_pairs, []

    def counted(*args):
        calls.append(args[7])                       # the capacity of this launch
        return real(*args)
    monkeypatch.setattr(L, "hgs_radius_pairs", counted)
    out = {}
    for dev in ("cpu", "cuda"):
        m = HairGaussianModel.from_strands(pts, device=dev, ref_strand_root=roots)
        opt = OptimizationParams()
        opt.bidirectional_merge = True
        m.training_setup(opt)
        m.compute_strands_info()
        # the premise, from the model's own thresholds: every pair of tips is a candidate, more than the first capacity holds
        tips = pts[:, 2]
        dirs = pts[:, 1] - tips
        dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
        cand, _ = KR.brute_pairs_f32(tips, dirs, float(m.merge_dist_th), np.cos(np.deg2rad(m.merge_angle_th)), True)
        assert len(cand) == 2016 > max(4 * 2 * pts.shape[0], 1024)
        out[dev] = m.compute_endpoint_pair_to_merge().cpu().numpy()
    assert len(calls) == 2 and calls[0] == 1024 and calls[1] >= 2016, calls      # the cap = found rerun of the device path
    assert out["cpu"].shape[0] >= 10
    assert sorted(map(tuple, np.sort(out["cpu"], 1).tolist())) == sorted(map(tuple, np.sort(out["cuda"], 1).tolist()))


# ---- nearest_distance ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", KC.NEAREST_M)
@pytest.mark.parametrize("N", KC.NEAREST_N)
def test_nearest_distance_around_the_lds_tile(N, M):
    from scene.hair_gaussian_model import nearest_distance
    pts, refs = KC.nearest_case(N, M)
    got = nearest_distance(torch.from_numpy(pts).cuda(), torch.from_numpy(refs).cuda()).cpu().numpy()
    want = KR.brute_nearest_f64(pts, refs)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert (want == 0).sum() >= (1 if N > 1 else 0)                 # exact copies among the references (N = 1: the far point alone)
    far = np.arange(0, N, 5)[-1]
    assert abs(want[far] - 0.01) < 1e-10                            # a point near 1e4: the runner-up is 1e-9 farther
