"""Host-side helpers of round 5 that need no GPU: the endpoint adjacency tables of the gather-mode backward, the degree
table the topology operators ask in place of torch.unique + torch.isin, the first-occurrence mask of
remove_duplicate_endpoint_rows, and the tile-order view of a capacity-mode binning buffer used by the parity tests."""
import numpy as np
import pytest
import torch


def test_adjacency_lists_every_role_once():
    from hgs_runtime.strand_step import _adjacency
    pairs = torch.tensor([[0, 1], [1, 2], [2, 3], [5, 4]])          # a chain of three segments and a lone one
    table = _adjacency(pairs.reshape(-1), 2, 6, 2)
    assert table.shape == (6, 2) and table.dtype == torch.int32
    # code = 2 * segment + (which end): endpoint 1 is the second end of segment 0 and the first of segment 1
    assert sorted(table[1].tolist()) == [1, 2] and sorted(table[2].tolist()) == [3, 4]
    assert table[0].tolist() == [0, -1] and table[3].tolist() == [5, -1]
    assert table[5].tolist() == [6, -1] and table[4].tolist() == [7, -1]
    # an endpoint of degree three does not fit a two-slot table
    assert _adjacency(torch.tensor([0, 1, 0, 2, 0, 3]), 2, 4, 2) is None


def test_degree_table_answers_what_unique_and_isin_answered():
    from scene.hair_gaussian_model import HairGaussianModel
    rng = np.random.default_rng(0)
    pts = np.cumsum(rng.normal(size=(7, 6, 3)) * 0.01, axis=1).astype(np.float32)
    m = HairGaussianModel.from_strands(pts, device="cpu")
    m.endpoint_pairs = torch.cat([m.endpoint_pairs, torch.tensor([[3, 40], [41, 41]])])      # a branch and a degenerate segment
    deg = m._endpoint_degree_table()
    u, c = torch.unique(m.endpoint_pairs, return_counts=True)
    assert deg.shape[0] == int(m.endpoint_pairs.max()) + 1
    assert torch.equal(torch.nonzero(deg == 1).squeeze(1), u[c == 1])
    assert torch.equal(deg[m.endpoint_pairs] != 1, torch.isin(m.endpoint_pairs, u[c != 1]))
    assert torch.equal(deg[m.endpoint_pairs] == 1, torch.isin(m.endpoint_pairs, u[c == 1]))
    assert m._endpoint_degree_table() is deg                      # remembered while endpoint_pairs is the same tensor
    m.endpoint_pairs = m.endpoint_pairs[:-1]
    assert m._endpoint_degree_table() is not deg


def test_first_occurrence_mask_equals_the_reference_form():
    from scene.hair_gaussian_model import HairGaussianModel
    m = HairGaussianModel(sh_degree=0, device="cpu")
    rng = np.random.default_rng(1)
    for n in (1, 7, 200):
        rows = torch.as_tensor(rng.integers(0, max(3, n // 2), (n, 2)))
        kept, mask = m.remove_duplicate_endpoint_rows(rows, return_mask=True)
        flat = rows.flatten()
        want = torch.zeros(flat.shape[0], dtype=torch.bool)
        want[m.get_first_occurence_index(flat)] = True                 # the reference's statements (:712-728, :772-784)
        want = want.reshape(-1, 2)
        want = want[:, 0] & want[:, 1]
        assert torch.equal(mask, want) and torch.equal(kept, rows[want])
    empty, mask = m.remove_duplicate_endpoint_rows(torch.zeros((0, 2), dtype=torch.long), return_mask=True)
    assert empty.shape == (0, 2) and mask.shape == (0,)


def test_in_tile_order_relays_an_allocated_layout():
    import importlib.util, os, sys
    # (tests.gpu_util imports the GPU binding at module level; the helper itself is numpy: load it without that import)
    src = open(os.path.join(os.path.dirname(__file__), "gpu_util.py")).read()
    body = src[src.index("def in_tile_order"):src.index("def run_backward")]
    ns = {"np": np}
    exec(body, ns)
    in_tile_order = ns["in_tile_order"]
    # four tiles; the allocation put tile 2's list first, then tile 0's, then tile 3's; tile 1 is empty
    ranges = np.array([[3, 5], [0, 0], [0, 3], [5, 9]], np.uint32)
    point_list = np.array([20, 21, 22, 0, 1, 30, 31, 32, 33], np.uint32)
    keys = point_list.astype(np.uint64) + 100
    r, pl, ks = in_tile_order(dict(ranges=ranges, point_list=point_list, keys_sorted=keys), 9)
    assert r.tolist() == [[0, 2], [0, 0], [2, 5], [5, 9]]
    assert pl.tolist() == [0, 1, 20, 21, 22, 30, 31, 32, 33] and ks.tolist() == (pl.astype(np.uint64) + 100).tolist()
    import pytest
    with pytest.raises(AssertionError):                              # overlapping segments are not a partition
        in_tile_order(dict(ranges=np.array([[0, 3], [2, 5]], np.uint32), point_list=point_list[:5], keys_sorted=keys[:5]), 5)


def test_bucket_capacity_keeps_four_significant_bits():
    """diff_gaussian_rasterization._C.bucket_capacity (round 6): >= n, at most 12.5 % above it, monotone, idempotent -- successive
    captures of a slowly growing model then ask the allocator for the same workspace sizes."""
    from diff_gaussian_rasterization._C import bucket_capacity as b
    prev = 0
    for n in list(range(0, 70)) + [100, 4095, 4096, 4097, 173000, 1 << 20, (1 << 20) + 1, 2437617, (1 << 31) - 5]:
        c = b(n)
        assert c >= n and c <= n + max(n // 8, 1) and b(c) == c and c >= prev
        assert n <= 16 or bin(c).rstrip("0").count("1") <= 4 and len(bin(c).rstrip("0")) - 2 <= 4
        prev = c
    assert len({b(n) for n in range(100000, 112000)}) <= 2


@pytest.fixture
def raster_word():
    """(diff_gaussian_rasterization._C in blocking mode with no capacity and nothing pending, a CPU int32 tensor as its sticky word)."""
    from diff_gaussian_rasterization import _C as raster
    cap = raster.capacity()
    raster.set_async(False)
    raster.reset_capacity(0)
    word = raster._max_rendered(torch.device("cpu"))
    raster.discard_pending()
    yield raster, word
    raster.set_async(False)
    raster.discard_pending()
    raster.reset_capacity(cap)


def test_capacity_growth_rule(raster_word):
    """raise_capacity is the one growth rule: bucket_capacity(int(worst * slack) + 4096), never shrinking; check_async() applies it
    with the mode's slack whether or not a pass overflowed, and records the worst count as the last exact one."""
    raster, word = raster_word
    raster.set_async(True, slack=1.5)
    raster._mark_pending(1 << 20)
    word.fill_(100000)
    assert raster.check_async() == [100000]                       # no overflow, and still ...
    assert raster.capacity() == raster.bucket_capacity(154096) == 163840
    assert raster.last_exact_rendered() == 100000
    raster._mark_pending(1 << 20)
    word.fill_(50000)
    assert raster.check_async() == [50000] and raster.capacity() == 163840      # a smaller worst leaves it
    assert raster.raise_capacity(10) == 163840
    assert raster.raise_capacity(100000, 2.0) == raster.bucket_capacity(204096) == raster.capacity() > 163840
    raster.reset_capacity(0)
    assert raster.capacity() == 0                                 # forgotten
    assert raster.raise_capacity(100000) == 163840                # slack None: the mode's
    raster.reset_capacity(64)
    assert raster.capacity() == 64                                # forced


def test_check_async_overflow_is_worst_above_the_smallest_capacity_used(raster_word):
    raster, word = raster_word
    raster.set_async(True, slack=1.5)
    assert raster.check_async() == []                             # nothing pending: the word is not even looked at
    word.fill_(77)
    assert raster.check_async() == [] and int(word.item()) == 77
    word.zero_()
    for worst, overflows in ((100000, False), (100001, True)):
        raster.reset_capacity(0)
        raster._mark_pending(200000)
        raster._mark_pending(100000)                              # the smallest capacity used counts
        raster._mark_pending(150000)
        word.fill_(worst)
        if overflows:
            with pytest.raises(raster.HgsCapacityOverflow, match="needed 100001 instances .capacity 100000."):
                raster.check_async()
        else:
            assert raster.check_async() == [worst]
        assert raster.capacity() == raster.bucket_capacity(int(worst * 1.5) + 4096)     # raised either way
        assert raster.last_exact_rendered() == worst
        assert int(word.item()) == 0 and raster.check_async() == []                    # word zeroed, marks cleared


def test_timeout_sentinel_is_an_error_and_never_a_capacity(raster_word):
    """HGS_WAIT_TIMED_OUT (include/hgs.h) in a sticky word: HgsError from every reader, the word zeroed, the capacity as it was."""
    import hgs_runtime as rt
    raster, word = raster_word
    raster.set_async(True)
    raster.reset_capacity(4096)
    raster._mark_pending(4096)
    word.fill_(-1)                                                # int32 -1 == 0xFFFFFFFF
    with pytest.raises(rt.HgsError, match="inter-workgroup wait"):
        raster.check_async()
    assert raster.capacity() == 4096 and int(word.item()) == 0
    assert raster.check_async() == []                             # the marks were cleared before it raised
    own = torch.full((1,), -1, dtype=torch.int32)                 # a caller's own word (FrameRenderer's)
    with pytest.raises(rt.HgsError, match="inter-workgroup wait"):
        raster.read_max_rendered(own)
    assert int(own.item()) == 0 and raster.capacity() == 4096
    word.fill_(-1)                                                # GraphedStep.headroom's read
    with pytest.raises(rt.HgsError, match="inter-workgroup wait"):
        raster.read_max_rendered()
    assert int(word.item()) == 0 and raster.capacity() == 4096
    own.fill_(-2)                                                 # the word is unsigned: a count above 2^31 is a count
    assert raster.read_max_rendered(own) == 0xFFFFFFFE


def test_discard_pending_and_the_headroom_read(raster_word):
    """What GraphedStep.capture ends with and what GraphedStep.headroom reads."""
    raster, word = raster_word
    raster.set_async(True, slack=1.5)
    raster.reset_capacity(8192)
    assert raster.discard_pending() is None                       # no pass since the last check
    raster._mark_pending(8192)
    raster._mark_pending(6144)
    word.fill_(999999)                                            # (would be an overflow if it were read)
    assert raster.discard_pending() == 6144
    assert int(word.item()) == 0 and raster.check_async() == [] and raster.capacity() == 8192
    # the headroom read: the worst count, the word zeroed -- capacity, pending marks and last exact count untouched
    exact = raster.last_exact_rendered()
    raster._mark_pending(8192)
    word.fill_(7000)
    assert raster.read_max_rendered() == 7000 and int(word.item()) == 0
    assert raster.capacity() == 8192 and raster.last_exact_rendered() == exact
    word.fill_(9000)
    with pytest.raises(raster.HgsCapacityOverflow):                # still pending, still against 8192
        raster.check_async()


def test_async_mode_restores_mode_slack_and_marks_and_keeps_the_capacity(raster_word):
    raster, word = raster_word
    fuses = lambda: raster.will_fuse_hair(16, 16)                 # (capacity mode and a learnt capacity)
    for before in (False, True):
        raster.reset_capacity(8192)
        raster.set_async(before, slack=3.0)
        raster._mark_pending(8192)
        try:
            with raster.async_mode(not before, slack=1.5):
                assert fuses() is (not before)
                raster._mark_pending(16)                          # (a pass of the body's; its mark goes with the body)
                assert raster.raise_capacity(100000) == 163840    # the body's slack
                raise KeyError("body")
        except KeyError:
            pass
        assert fuses() is before and raster.capacity() == 163840   # the mode is back, the capacity learnt inside is kept
        assert raster.raise_capacity(100000) == raster.bucket_capacity(304096)       # the slack is back
        word.fill_(8192)
        assert raster.check_async() == [8192]                     # pending as before, against 8192 and not 16
        with raster.async_mode(True):                             # no slack given: the mode's stays
            assert fuses() and raster.raise_capacity(200000) == raster.bucket_capacity(604096)
        assert fuses() is before and raster.check_async() == []


def test_set_async_keeps_the_capacity_and_clears_the_marks(raster_word):
    raster, word = raster_word
    raster.set_async(True, slack=1.5)
    raster.reset_capacity(12288)
    raster._mark_pending(64)
    raster.set_async(True, slack=2.0)
    assert raster.capacity() == 12288 and raster.check_async() == []
    raster.set_async(False)
    assert raster.capacity() == 12288 and not raster.will_fuse_hair(16, 16)


def test_training_event_log_and_visible_gpus_need_no_gpu():
    """train._EventInfo is what the operators take as `training_info`; bench.visible_gpus() counts devices without a HIP call."""
    import importlib.util
    import os
    from train import _EventInfo
    info = _EventInfo()
    info.densification_info["clone"] = 3
    assert info.densification_info == {"clone": 3}
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(__file__)), "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    n = m.visible_gpus()
    assert n is None or n >= 0
    if not os.path.isdir("/sys/class/kfd"):
        assert n == 0


def test_greedy_partner_filter_equals_the_in_order_walk():
    """HairTopologyMixin._keep_rows_whose_strand_partners_are_free (stage 2 of compute_endpoint_pair_to_merge resolved in vectorised
    rounds) against the reference's walk (scene/hair_gaussian_model.py:1331-1362: a set of blocked ids, rows in order) on random
    tables: strands of two ends each, candidate rows pairing ends of different strands, every id in at most one row, long
    dependency chains included (row k pairs the far end of strand k with the near end of strand k + 1)."""
    from scene.hair_topology import HairTopologyMixin
    rng = np.random.default_rng(5)
    for trial in range(200):
        n_strands = int(rng.integers(2, 400))
        n_ids = 2 * n_strands + int(rng.integers(0, 5))
        ids = rng.permutation(n_ids)[:2 * n_strands]
        partner = -np.ones(n_ids, np.int32)
        partner[ids[0::2]], partner[ids[1::2]] = ids[1::2], ids[0::2]
        if trial % 3 == 0:      # a chain: every row depends on the one in front of it
            cand = np.stack([ids[1:-1:2], ids[2::2]], 1)
        else:
            free = rng.permutation(ids)
            k = int(rng.integers(1, n_strands + 1))
            cand = free[:2 * k].reshape(k, 2)
            cand = cand[partner[cand[:, 0]] != cand[:, 1]]          # (the two ends of one strand are never a candidate row)
        if trial % 2:
            cand = cand[rng.permutation(cand.shape[0])]
        cand = cand.astype(np.int64)
        blocked, keep = set(), []
        for (p, q) in cand.tolist():
            if p in blocked or q in blocked:
                keep.append(False)
                continue
            blocked.add(int(partner[p])); blocked.add(int(partner[q])); keep.append(True)
        got = HairTopologyMixin._keep_rows_whose_strand_partners_are_free(cand, partner)
        np.testing.assert_array_equal(got, np.asarray(keep, bool), err_msg=f"trial {trial}")
