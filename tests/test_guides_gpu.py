"""The guide selection on the GPU (csrc/hgs_guides.hip through scene/strand_guides.py): the three kernels in their loop and
select_guides(device="cuda") against the numpy path and the loop restatement (tests/guides_reference.py) bit for bit on every case of
tests/guides_cases.py; each kernel alone against the matching numpy statement on handed-in centroids and labels; a second run; the
wrapper's checks; the C entry points' refusals on device buffers; and the driver on both devices."""
import numpy as np
import pytest
import torch

from tests import guides_cases as GC
from tests import guides_reference as GR
from tests.test_guides_cpu import assert_same, numpy_result, reference

pytestmark = pytest.mark.gpu


def _device(name):
    from scene.strand_guides import guides_device
    pts, off, k, samples, iters = GC.cases()[name]
    return guides_device(torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda"), k, samples, iters)


@pytest.mark.parametrize("name", GC.NAMES)
def test_kernels_match_the_numpy_path_and_the_restatement(name):
    from scene.strand_guides import select_guides
    got = _device(name)
    assert_same(got, numpy_result(name), name + " (numpy)")
    assert_same(got, reference(name), name + " (loop)")
    pts, off, k, samples, iters = GC.cases()[name]
    strands = GC.as_export(pts, off)
    host, dev = select_guides(strands, k, samples, iters), select_guides(strands, k, samples, iters, device="cuda")
    for a, b in zip(host[0], dev[0]):
        assert GR.same_bytes(a, b), name
    assert set(host[1]) == set(dev[1]) and all(GR.same_bytes(host[1][key], dev[1][key]) for key in host[1]), name
    assert host[2] == dev[2], (host[2], dev[2])


# ---- each kernel alone -------------------------------------------------------------------------------------------------------------
# (N, M, samples, K): S = 2 and 16 (registers, 128 strands a workgroup), 17 (LDS, tiles of 16) and 64 (LDS, tiles of 8); more than one
# workgroup; K below, at and above a tile edge
ALONE = ((1, 2, 2, 1), (130, 3, 2, 257), (257, 17, 16, 63), (257, 17, 16, 64), (129, 17, 16, 130), (65, 17, 64, 16), (130, 20, 32, 33),
         (65, 100, 64, 8), (130, 70, 64, 19))


def _alone(N, M, samples, K, seed):
    """Strands with three that are not finite, centroids that are NOT their seeds -- some of them twice (ties), one far from all
    (empty) -- and a previous labelling."""
    from scene.strand_guides import sample_joints
    rng = np.random.default_rng(seed)
    strands = GC.blob(N, M, seed)
    if N > 8:
        strands = GC.with_bad(strands, {(2, M - 1, 0): np.nan, (N - 1, 0, 1): np.inf, (N // 2, M // 2, 2): np.nan})
    pts, off = GC.pack(strands)
    S = min(samples, M)
    x = pts.reshape(N, M, 3)[:, sample_joints(M, S)].astype(np.float64)
    cent = rng.uniform(-1.0, 1.0, (K, S, 3))
    if K > 4:
        cent[1] = x[4]                                                              # strand 4 sits on centroid 1 ...
        cent[K - 1] = cent[1]                                                       # ... and on K - 1: a tie, 1 wins
        cent[3] = 50.0                                                              # no strand comes here
        cent[2] = np.nan_to_num(x[0], nan=0.0, posinf=0.0, neginf=0.0)              # strand 0 sits on centroid 2
    status = (~np.isfinite(pts.reshape(N, -1)).all(axis=1)).astype(np.int32)
    prev = rng.integers(0, K, N).astype(np.int32)
    return pts, off, S, x, cent, status, prev


@pytest.mark.parametrize("N,M,samples,K", ALONE)
def test_assign_alone(N, M, samples, K):
    from scene import strand_guides as SG
    pts, off, S, x, cent, status, prev = _alone(N, M, samples, K, 100 + K)
    E = np.nonzero(status == 0)[0]
    want_l, want_d = np.full(N, -1, np.int32), np.full(N, np.inf)
    want_l[E], want_d[E] = SG.assign_numpy(x[E], cent)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    changed = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    label, d2 = SG.assign_device(dev(pts), N, M, S, dev(status), dev(cent), dev(prev), changed)
    assert GR.same_bytes(label.cpu().numpy(), want_l) and GR.same_bytes(d2.cpu().numpy(), want_d)
    assert int(changed) == 5 + int((want_l != prev).sum())                          # added to what was there
    again, d2_again = SG.assign_device(dev(pts), N, M, S, dev(status), dev(cent))   # no previous assignment: nothing is counted
    assert GR.same_bytes(again.cpu().numpy(), want_l) and GR.same_bytes(d2_again.cpu().numpy(), want_d)
    if K > 4 and N > 8:
        assert want_l[4] == 1 and want_d[4] == 0.0 and (want_l == K - 1).sum() == 0 and (want_l == 3).sum() == 0
        assert want_l[0] == 2 and want_d[0] == 0.0 and want_l[2] == -1 and len(set(want_l.tolist())) > 3


@pytest.mark.parametrize("N,M,samples,K", ALONE)
def test_update_and_pick_alone(N, M, samples, K):
    from scene import strand_guides as SG
    pts, off, S, x, cent, status, _ = _alone(N, M, samples, K, 200 + K)
    rng = np.random.default_rng(300 + K)
    E = np.nonzero(status == 0)[0]
    lab_E = rng.integers(0, K, E.shape[0]).astype(np.int32)
    if K > 4:
        lab_E[lab_E == 3] = 0                                                       # cluster 3 is empty
    d_E = rng.integers(0, 4, E.shape[0]).astype(np.float64)                         # many ties: the smaller i wins
    labels, dist2 = np.full(N, -1, np.int32), np.full(N, np.inf)
    labels[E], dist2[E] = lab_E, d_E
    want_c, want_n = SG.update_numpy(x[E], lab_E, cent)
    want_g, want_n2 = SG.pick_numpy(E, lab_E, d_E, K)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    order, start = SG.member_list(dev(labels), K)
    assert order.shape[0] == E.shape[0] and start.shape[0] == K + 1
    cent_d = dev(cent)
    count = SG.update_device(dev(pts), N, M, S, order, start, cent_d)
    assert GR.same_bytes(cent_d.cpu().numpy(), want_c) and GR.same_bytes(count.cpu().numpy(), want_n)
    guide = SG.pick_device(N, K, order, start, dev(dist2))
    assert GR.same_bytes(guide.cpu().numpy(), want_g) and np.array_equal(want_n, want_n2)
    if K > 4:
        assert want_g[3] == -1 and want_n[3] == 0 and GR.same_bytes(want_c[3], cent[3])


def test_two_runs_and_a_side_stream_give_equal_bytes():
    from scene.strand_guides import guides_device
    first = _device("n129_m17_k65")
    assert_same(_device("n129_m17_k65"), first, "second run")
    pts, off, k, samples, iters = GC.cases()["n129_m17_k65"]
    stream = torch.cuda.Stream()
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        side = guides_device(pts_d, off_d, k, samples, iters)
    stream.synchronize()
    assert_same(side, first, "side stream")


def test_device_wrapper_checks_its_tensors():
    import hgs_runtime as rt
    from scene.strand_guides import guides_device
    pts, off = GC.cases()["n63_m3_k2"][:2]
    pts_d, off_d = torch.as_tensor(pts, device="cuda"), torch.as_tensor(off, device="cuda")
    with pytest.raises(rt.HgsError):
        guides_device(torch.as_tensor(pts), off_d, 2)                              # a host tensor is not moved to the GPU behind the caller's back
    with pytest.raises(rt.HgsError):
        guides_device(pts_d, off_d.to(torch.int32), 2)
    with pytest.raises(rt.HgsError):
        guides_device(pts_d.to(torch.float64), off_d, 2)
    for params, words in GC.REFUSED:
        with pytest.raises(rt.HgsError, match=words):
            guides_device(pts_d, off_d, *params)
    for bad_pts, bad_off in (GC.ragged(), GC.one_point()):
        with pytest.raises(rt.HgsError, match="same number M >= 2 of points"):
            guides_device(torch.as_tensor(bad_pts, device="cuda"), torch.as_tensor(bad_off, device="cuda"), 2)
    with pytest.raises(rt.HgsError, match="tile the points"):
        guides_device(pts_d[:-3], off_d, 2)


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    """On device buffers: every refusal returns 1 with a message and leaves the output buffers as they were."""
    import hgs_runtime as rt
    from scene import strand_guides as SG
    L = rt.lib()
    N, M, samples, K = 130, 20, 32, 33
    pts, off, S, x, cent, status, prev = _alone(N, M, samples, K, 7)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    pts_d, st_d, cent_d, prev_d = dev(pts), dev(status), dev(cent), dev(prev)
    label = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    changed = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    count = torch.full((K,), -7, dtype=torch.int32, device="cuda")
    guide = torch.full((K,), -7, dtype=torch.int64, device="cuda")
    order, start = SG.member_list(prev_d, K)
    P = N * M

    def assign(N_=N, M_=M, S_=S, P_=P, p=pts_d.data_ptr(), s=st_d.data_ptr(), K_=K, c=cent_d.data_ptr(), pv=prev_d.data_ptr(), l=label.data_ptr(),
               d=d2.data_ptr(), ch=changed.data_ptr()):
        return L.hgs_guides_assign(rt.current_stream(), N_, M_, S_, P_, p, s, K_, c, pv, l, d, ch)

    def update(N_=N, M_=M, S_=S, P_=P, p=pts_d.data_ptr(), K_=K, o=order.data_ptr(), n=order.shape[0], st=start.data_ptr(), c=cent_d.data_ptr(),
               cn=count.data_ptr()):
        return L.hgs_guides_update(rt.current_stream(), N_, M_, S_, P_, p, K_, o, n, st, c, cn)

    def pick(N_=N, K_=K, o=order.data_ptr(), n=order.shape[0], st=start.data_ptr(), d=d2.data_ptr(), g=guide.data_ptr()):
        return L.hgs_guides_pick(rt.current_stream(), N_, K_, o, n, st, d, g)

    strands = (dict(N_=-1), dict(P_=-1), dict(M_=1), dict(S_=1), dict(S_=65), dict(S_=M + 1), dict(P_=P - 1), dict(N_=2 ** 31 - 1, M_=2 ** 31 - 1),
               dict(K_=0), dict(K_=65537), dict(p=None))
    for kw in strands + (dict(s=None), dict(c=None), dict(l=None), dict(d=None), dict(ch=None), dict(l=prev_d.data_ptr()), dict(l=st_d.data_ptr())):
        assert assign(**kw) == 1 and b"hgs_guides_assign" in L.hgs_last_error(), kw
    for kw in strands + (dict(n=-1), dict(n=N + 1), dict(o=None), dict(st=None), dict(c=None), dict(cn=None)):
        assert update(**kw) == 1 and b"hgs_guides_update" in L.hgs_last_error(), kw
    for kw in (dict(N_=-1), dict(K_=0), dict(K_=65537), dict(n=-1), dict(n=N + 1), dict(o=None), dict(st=None), dict(d=None), dict(g=None)):
        assert pick(**kw) == 1 and b"hgs_guides_pick" in L.hgs_last_error(), kw
    assert assign(N_=0, P_=0) == 0
    torch.cuda.synchronize()
    assert bool((label == -7).all()) and bool((d2 == -7.0).all()) and int(changed) == -7 and bool((count == -7).all()) and bool((guide == -7).all())
    assert GR.same_bytes(cent_d.cpu().numpy(), cent)
    # and the same buffers with good arguments
    assert assign() == 0
    torch.cuda.synchronize()
    E = np.nonzero(status == 0)[0]
    want_l, want_d = np.full(N, -1, np.int32), np.full(N, np.inf)
    want_l[E], want_d[E] = SG.assign_numpy(x[E], cent)
    assert GR.same_bytes(label.cpu().numpy(), want_l) and GR.same_bytes(d2.cpu().numpy(), want_d) and int(changed) == -7 + int((want_l != prev).sum())


def test_driver_on_the_device_writes_the_host_files(tmp_path):
    """export_strands.py --select_guides with --device cuda and with --device cpu, behind --interpolate: the same bytes in every file."""
    import export_strands
    from tests.test_groom_cpu import driver_model
    model, _ = driver_model(tmp_path)
    common = ["-m", str(model), "--points", "9", "--format", "hair", "--format", "usc", "--interpolate", "--select_guides", "6", "--select_samples", "5"]
    _, dp = export_strands.main(common + ["-o", str(tmp_path / "dev"), "--device", "cuda"])
    _, hp = export_strands.main(common + ["-o", str(tmp_path / "host"), "--device", "cpu"])
    assert set(dp) == set(hp) == {"hair", "usc", "hair_guides", "usc_guides", "guide_binding"}
    for key in ("hair", "usc", "hair_guides", "usc_guides"):
        d, h = open(dp[key], "rb").read(), open(hp[key], "rb").read()
        assert len(d) == len(h) > 0 and d == h, key
    with np.load(dp["guide_binding"]) as zd, np.load(hp["guide_binding"]) as zh:
        assert set(zd.files) == set(zh.files) and all(GR.same_bytes(zd[k], zh[k]) for k in zd.files)
        assert 1 <= zd["guide_strand"].shape[0] <= 6
