"""hgs_oriented_match and hgs_strand_votes (csrc/hgs_metrics.hip) per point and per strand against the brute-force statements
of tests/metrics_reference.py on the hard clouds of tests/metrics_cases.py.  Everything compared is an integer: equality.

The kernels are called through the C ABI with ctypes, as loss/metrics.py calls them.  Every device array lives inside a larger
allocation with sentinel bytes on both sides (checked after the launches); masks and best rows start as a sentinel pattern,
the overflow list as -1."""
import numpy as np
import pytest
import torch

from tests import metrics_cases as MC
from tests import metrics_reference as R

pytestmark = pytest.mark.gpu

GUARD = 256                      # sentinel bytes on either side (keeps the payload's 256-byte alignment)
FILL = 0xA5
MASK_FILL = np.uint32(0xA5A5A5A5)
BEST_FILL = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
DEVICE = "cuda"
NAMES = MC.case_names()
STRAND_NAMES = [n for n in NAMES if MC.get(n).has_strands]
# through compute_metrics: finite points (the host recount of an overflowing strand uses the tree), both directions within the
# cell limit; all_pairs has its own test, with a 33rd pair
METRIC_NAMES = [n for n in STRAND_NAMES if MC.get(n).cpu_comparable and MC.get(n).reversible and MC.get(n).angles is not None and n != "all_pairs"]


class Dev:
    """A host array's bytes on the device between two runs of sentinel bytes; `offset` bytes in front shift the payload off
    its alignment."""

    def __init__(self, host, offset=0):
        host = np.ascontiguousarray(host)
        self.shape, self.dtype, n = host.shape, host.dtype, host.nbytes
        pad = (-(n + offset)) % 16
        self.buf = torch.full((GUARD + offset + n + pad + GUARD,), FILL, dtype=torch.uint8, device=DEVICE)
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.set(host)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo

    def set(self, host):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        assert host.nbytes == self.hi - self.lo
        if host.nbytes:
            self.buf[self.lo:self.hi] = torch.from_numpy(host.reshape(-1).view(np.uint8).copy()).to(DEVICE)

    def get(self):
        return self.buf[self.lo:self.hi].cpu().numpy().view(self.dtype).reshape(self.shape).copy()

    def intact(self):
        return bool((self.buf[:self.lo] == FILL).all()) and bool((self.buf[self.hi:] == FILL).all())


class Pool:
    def __init__(self):
        self.items = []

    def put(self, host, offset=0):
        self.items.append(Dev(host, offset))
        return self.items[-1]

    def check(self):
        torch.cuda.synchronize()
        for k, d in enumerate(self.items):
            assert d.intact(), f"array {k} {d.shape}: a sentinel byte was overwritten"


def _rt():
    import hgs_runtime as rt
    return rt, rt.lib()


class Side:
    """A case's arrays on the device, uploaded once per test."""

    def __init__(self, c, pool):
        self.c, self.pool = c, pool
        self.a_pts, self.a_dirs = pool.put(c.a_pts), pool.put(c.a_dirs)
        self.b_pts, self.b_dirs = pool.put(c.b_pts), pool.put(c.b_dirs)
        self.nA, self.nB = len(c.a_pts), len(c.b_pts)
        rt, L = _rt()
        self.scratch_bytes = int(L.hgs_oriented_match_scratch_bytes(self.nB))
        self.thr = np.ascontiguousarray(c.thresholds, np.float64)
        if c.has_strands:
            self.offsets, self.b_strand = pool.put(np.asarray(c.offsets, np.int64)), pool.put(np.asarray(c.b_strand, np.int32))

    def match(self, bidir, box=None, stream=None):
        """One hgs_oriented_match into a fresh sentinel-filled mask and a fresh scratch -> (mask Dev, scratch Dev, box)."""
        rt, L = _rt()
        box = np.ascontiguousarray(self.c.box if box is None else box, np.float64)
        mask = self.pool.put(np.full(self.nA, MASK_FILL, np.uint32))
        scratch = self.pool.put(np.full(self.scratch_bytes, FILL, np.uint8))
        rt.check(L.hgs_oriented_match(rt.current_stream() if stream is None else stream, self.nA, self.nB, self.c.K, self.a_pts.ptr,
                                      self.a_dirs.ptr, self.b_pts.ptr, self.b_dirs.ptr, self.thr.ctypes.data, int(bidir), box.ctypes.data,
                                      mask.ptr, scratch.ptr, self.scratch_bytes))
        return mask, scratch, box

    def votes(self, bidir, scratch, box, cap, stream=None):
        """One hgs_strand_votes after the match call that left `scratch` -> (best [K][S], overflow [S], n_overflow)."""
        rt, L = _rt()
        S = len(self.c.offsets) - 1
        best = self.pool.put(np.full((self.c.K, S), BEST_FILL, np.int32))
        over, n_over = self.pool.put(np.full(S, -1, np.int32)), self.pool.put(np.zeros(1, np.int32))
        rt.check(L.hgs_strand_votes(rt.current_stream() if stream is None else stream, S, self.nB, self.c.K, self.a_pts.ptr, self.a_dirs.ptr,
                                    self.offsets.ptr, self.b_strand.ptr, self.thr.ctypes.data, int(bidir), box.ctypes.data, scratch.ptr,
                                    int(cap), best.ptr, over.ptr, n_over.ptr))
        return best, over, n_over


def _assert_masks(name, what, got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{name} {what}: {bad.size} of {len(want)} points differ; first: point {int(bad[0])} expected "
                           f"{int(want[bad[0]]):#034b} got {int(got[bad[0]]):#034b}")


@pytest.mark.parametrize("name", NAMES)
def test_oriented_match_equals_brute_force_per_point(name):
    c = MC.get(name)
    pool = Pool()
    side = Side(c, pool)
    for bidir in c.bidirectional:
        want = MC.expected_masks(name, bidir)
        for t, box in enumerate((None,) + tuple(c.extra_boxes)):
            mask, _, _ = side.match(bidir, box)
            pool.check()
            _assert_masks(name, f"bidirectional={int(bidir)} box {t}", mask.get(), want)


def _assert_votes(name, what, c, cap, best, over, n_over, want_best, entries):
    S = len(entries)
    n = int(n_over.get()[0])
    over = over.get()
    want_over = np.flatnonzero(entries > cap)
    assert n == len(want_over), f"{name} {what}: n_overflow {n}, {len(want_over)} strands have more than {cap} entries"
    assert sorted(over[:n].tolist()) == want_over.tolist(), f"{name} {what}: overflow list {sorted(over[:n].tolist())[:8]}.. expected {want_over.tolist()[:8]}.."
    assert (over[n:] == -1).all(), f"{name} {what}: the overflow list was written beyond n_overflow"
    best = best.get()
    fits = np.ones(S, bool)
    fits[want_over] = False
    assert (best[:, ~fits] == BEST_FILL).all(), f"{name} {what}: the best row of an overflowing strand was written"
    bad = np.argwhere(best[:, fits] != want_best[:, fits])
    if bad.size:
        k, s = int(bad[0][0]), int(np.flatnonzero(fits)[bad[0][1]])
        raise AssertionError(f"{name} {what}: {len(bad)} best entries differ; first: pair {k} strand {s} ({int(entries[s])} entries) "
                             f"expected {int(want_best[k, s])} got {int(best[k, s])}")


@pytest.mark.parametrize("name", STRAND_NAMES)
def test_strand_votes_equal_brute_force_per_strand(name):
    c = MC.get(name)
    pool = Pool()
    side = Side(c, pool)
    for bidir in c.bidirectional:
        want_best, entries = MC.expected_votes(name, bidir)
        mask, scratch, box = side.match(bidir)
        for cap in c.capacities:
            best, over, n_over = side.votes(bidir, scratch, box, cap)
            pool.check()
            _assert_votes(name, f"bidirectional={int(bidir)} capacity={cap}", c, cap, best, over, n_over, want_best, entries)
        _assert_masks(name, f"bidirectional={int(bidir)}", mask.get(), MC.expected_masks(name, bidir))


@pytest.mark.parametrize("name,cap", [("vote_shapes[mixed]", 64), ("vote_shapes[mixed]", 2048), ("vote_strand_numbers[order1]", 4),
                                      ("vote_shapes[S=3000]", 1)])
def test_strand_votes_give_the_same_bytes_twice_and_on_a_side_stream(name, cap):
    c = MC.get(name)
    pool = Pool()
    side = Side(c, pool)
    mask, scratch, box = side.match(True)
    runs = [side.votes(True, scratch, box, cap), side.votes(True, scratch, box, cap)]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        mask2, scratch2, _ = side.match(True, stream=stream.cuda_stream)
        runs.append(side.votes(True, scratch2, box, cap, stream=stream.cuda_stream))
    stream.synchronize()
    pool.check()
    assert mask.get().tobytes() == mask2.get().tobytes()
    first = runs[0]
    for best, over, n_over in runs[1:]:
        n = int(n_over.get()[0])
        assert n == int(first[2].get()[0]) and best.get().tobytes() == first[0].get().tobytes()
        assert set(over.get()[:n].tolist()) == set(first[1].get()[:n].tolist()) and (over.get()[n:] == -1).all()


def _same(a, b):
    assert a.keys() == b.keys(), (a.keys(), b.keys())
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (k, a[k], b[k])


@pytest.mark.parametrize("name", METRIC_NAMES)
def test_compute_metrics_equals_the_brute_force_integers(name):
    """compute_metrics(device="cuda") from the kernels' integers against metrics_from_counts of the brute-force integers, byte
    for byte; at vote_capacity 4 most strands are recounted on the host, and that recount is held to brute force too."""
    from loss.metrics import HairEvalData, compute_metrics
    c = MC.get(name)
    gt, pred = HairEvalData(c.a_pts.copy(), c.a_dirs.copy(), c.a_strand), HairEvalData(c.b_pts.copy(), c.b_dirs.copy(), c.b_strand)
    sizes = np.diff(c.offsets)
    keep = sizes > 0
    for bidir in c.bidirectional:
        best, _ = MC.expected_votes(name, bidir)
        want = R.metrics_from_counts(R.counts(MC.expected_reverse_masks(name, bidir), c.K), len(c.b_pts),
                                     R.counts(MC.expected_masks(name, bidir), c.K), len(c.a_pts), best[:, keep], sizes[keep], bidir)
        for cap in (2048, 4):
            got, _ = compute_metrics(pred, gt, dist_ths=list(c.thresholds[:, 0]), angle_ths=list(c.angles), bidirectional=bidir,
                                     device="cuda", vote_capacity=cap)
            _same(got, want)


def test_thirty_three_pairs_take_two_passes():
    from loss.metrics import HairEvalData, compute_metrics
    c = MC.get("all_pairs")
    gt, pred = HairEvalData(c.a_pts.copy(), c.a_dirs.copy(), c.a_strand), HairEvalData(c.b_pts.copy(), c.b_dirs.copy(), c.b_strand)
    radii, angles = list(MC.ALL_RADII) + [2e-3], list(MC.ALL_ANGLES) + [45.0]
    for bidir in (False, True):
        want = R.reference_metrics(pred, gt, radii, angles, bidir)
        for cap in (2048, 4):
            got, _ = compute_metrics(pred, gt, dist_ths=radii, angle_ths=angles, bidirectional=bidir, device="cuda", vote_capacity=cap)
            _same(got, want)
            assert len(got["recall" + ("(b)" if bidir else "")]) == 33


def test_refusals_leave_the_buffers_untouched():
    rt, L = _rt()
    c = MC.get("cell_limit")
    pool = Pool()
    side = Side(c, pool)
    st = rt.current_stream()
    mask = pool.put(np.full(side.nA, MASK_FILL, np.uint32))
    scratch = pool.put(np.full(side.scratch_bytes + 64, FILL, np.uint8))
    box = np.ascontiguousarray(c.box)

    def match(K=c.K, thr=side.thr, box=box, b_pts=side.b_pts, scratch_ptr=scratch.ptr, nbytes=side.scratch_bytes):
        return L.hgs_oriented_match(st, side.nA, side.nB, K, side.a_pts.ptr, side.a_dirs.ptr, b_pts.ptr, side.b_dirs.ptr, thr.ctypes.data, 0,
                                    box.ctypes.data, mask.ptr, scratch_ptr, nbytes)

    def refused(status, who):
        assert status != 0
        msg = L.hgs_last_error().decode()
        assert msg.startswith(who), msg
        torch.cuda.synchronize()
        assert (mask.get() == MASK_FILL).all() and (scratch.get() == FILL).all(), msg
        return msg

    # one cell too many on x
    b_wide = MC.cell_limit_points(1)[2]
    wide = np.ascontiguousarray(np.concatenate([b_wide.min(0), b_wide.max(0)]))
    msg = refused(match(box=wide, b_pts=pool.put(b_wide)), "hgs_oriented_match")
    assert "2^21" in msg
    thr33 = np.ascontiguousarray(np.tile(side.thr[:1], (33, 1)))
    refused(match(K=0), "hgs_oriented_match")
    refused(match(K=33, thr=thr33), "hgs_oriented_match")
    for r in (0.0, -1e-3, np.inf, np.nan):
        bad = side.thr.copy()
        bad[1, 0] = r
        assert "radius 1" in refused(match(thr=bad), "hgs_oriented_match")
    refused(match(nbytes=side.scratch_bytes - 1), "hgs_oriented_match")
    refused(match(scratch_ptr=scratch.ptr + 16), "hgs_oriented_match")
    # the vote call: after a good match, capacities that are no power of two in [1, 2048]
    good, good_scratch, _ = side.match(False)
    S = len(c.offsets) - 1
    best, over, n_over = pool.put(np.full((c.K, S), BEST_FILL, np.int32)), pool.put(np.full(S, -1, np.int32)), pool.put(np.zeros(1, np.int32))

    def votes(cap, K=c.K, thr=side.thr, scratch_ptr=good_scratch.ptr):
        return L.hgs_strand_votes(st, S, side.nB, K, side.a_pts.ptr, side.a_dirs.ptr, side.offsets.ptr, side.b_strand.ptr, thr.ctypes.data, 0,
                                  box.ctypes.data, scratch_ptr, cap, best.ptr, over.ptr, n_over.ptr)

    for status in (votes(0), votes(3), votes(4096), votes(-4), votes(4, K=0), votes(4, K=33, thr=thr33), votes(4, scratch_ptr=good_scratch.ptr + 16)):
        assert status != 0 and L.hgs_last_error().decode().startswith("hgs_strand_votes")
        torch.cuda.synchronize()
        assert (best.get() == BEST_FILL).all() and (over.get() == -1).all() and n_over.get()[0] == 0
    pool.check()
    _assert_masks("cell_limit", "after the refusals", good.get(), MC.expected_masks("cell_limit", False))


def test_empty_sides_return_zero_and_write_what_the_header_says():
    rt, L = _rt()
    c = MC.get("flat_boxes[single]")
    pool = Pool()
    side = Side(c, pool)
    st = rt.current_stream()
    box = np.ascontiguousarray(c.box)
    mask = pool.put(np.full(side.nA, MASK_FILL, np.uint32))
    scratch = pool.put(np.full(side.scratch_bytes, FILL, np.uint8))
    S = len(c.offsets) - 1
    best, over, n_over = pool.put(np.full((c.K, S), BEST_FILL, np.int32)), pool.put(np.full(S, -1, np.int32)), pool.put(np.zeros(1, np.int32))
    # nA = 0: nothing to write
    rt.check(L.hgs_oriented_match(st, 0, side.nB, c.K, side.a_pts.ptr, side.a_dirs.ptr, side.b_pts.ptr, side.b_dirs.ptr, side.thr.ctypes.data, 0,
                                  box.ctypes.data, mask.ptr, scratch.ptr, side.scratch_bytes))
    # S = 0: nothing to write
    rt.check(L.hgs_strand_votes(st, 0, side.nB, c.K, side.a_pts.ptr, side.a_dirs.ptr, side.offsets.ptr, side.b_strand.ptr, side.thr.ctypes.data, 0,
                                box.ctypes.data, scratch.ptr, 2048, best.ptr, over.ptr, n_over.ptr))
    pool.check()
    assert (mask.get() == MASK_FILL).all() and (scratch.get() == FILL).all() and (best.get() == BEST_FILL).all() and (over.get() == -1).all()
    # nB = 0: no point of A is matched, no strand has a vote; no scratch is needed
    rt.check(L.hgs_oriented_match(st, side.nA, 0, c.K, side.a_pts.ptr, side.a_dirs.ptr, None, None, side.thr.ctypes.data, 0, box.ctypes.data,
                                  mask.ptr, None, 0))
    rt.check(L.hgs_strand_votes(st, S, 0, c.K, side.a_pts.ptr, side.a_dirs.ptr, side.offsets.ptr, None, side.thr.ctypes.data, 0, box.ctypes.data,
                                None, 2048, best.ptr, over.ptr, n_over.ptr))
    pool.check()
    assert (mask.get() == 0).all() and (best.get() == 0).all() and (over.get() == -1).all() and n_over.get()[0] == 0
