"""The block plan of a strand model (hgs_runtime.strand_step._block_plan, include/hgs.h HgsBlockPlan) on hand-made topologies:
the partition of the segments into chunks that own whole strands, which lets the backward's per-Gaussian launch be the
endpoint gather too.  Host code only: no GPU."""
import numpy as np
import pytest
import torch

LENS = (1, 2, 63, 64, 65, 127, 128, 255)      # 705 segments (705 % 64 = 1), 713 endpoints
LIMIT = 256


def _chains(lens, loose=0):
    """endpoint_pairs [P,2] of open chains stored strand after strand (+ `loose` endpoints no segment names), and E."""
    pairs, e = [], 0
    for n in lens:
        pairs += [(e + k, e + k + 1) for k in range(n)]
        e += n + 1
    return torch.tensor(pairs, dtype=torch.int64), e + loose


def _plan(pairs, E):
    from hgs_runtime.strand_step import _adjacency, _block_plan
    adj = _adjacency(pairs.reshape(-1), 2, E, 2)
    assert adj is not None
    return adj, _block_plan(adj, pairs.shape[0])


def _check(pairs, E, adj, plan):
    """The properties include/hgs.h states: each segment and each endpoint exactly once, both limits, every segment an
    endpoint names inside that endpoint's chunk."""
    assert plan is not None
    chunks, ep_list = plan[0].numpy().astype(np.int64), plan[1].numpy().astype(np.int64)
    assert plan[0].dtype == torch.int32 and plan[1].dtype == torch.int32 and plan[0].is_contiguous()
    P = pairs.shape[0]
    s0, ns, e0, ne = chunks.T
    assert (ns >= 1).all() and (ns <= LIMIT).all() and (ne >= 0).all() and (ne <= LIMIT).all()
    # consecutive runs that tile [0, P) and [0, E)
    assert s0[0] == 0 and (s0[1:] == (s0 + ns)[:-1]).all() and s0[-1] + ns[-1] == P
    assert e0[0] == 0 and (e0[1:] == (e0 + ne)[:-1]).all() and e0[-1] + ne[-1] == E
    assert sorted(ep_list.tolist()) == list(range(E))
    chunk_of_ep = np.empty(E, np.int64)
    chunk_of_ep[ep_list] = np.repeat(np.arange(len(chunks)), ne)
    codes = adj.numpy().astype(np.int64)
    for col in range(2):
        named = codes[:, col] >= 0
        seg = codes[named, col] >> 1
        c = chunk_of_ep[named]
        assert (seg >= s0[c]).all() and (seg < s0[c] + ns[c]).all()
    return chunks


@pytest.mark.parametrize("loose", [0, 5, 200])
def test_mixed_strand_lengths(loose):
    pairs, E = _chains(LENS, loose)
    assert pairs.shape[0] == 705 and pairs.shape[0] % 64 == 1
    adj, plan = _plan(pairs, E)
    chunks = _check(pairs, E, adj, plan)
    # greedy to the furthest allowed cut: 1 + 2 + 63 + 64 + 65 = 195 segments (127 more would pass 256), then 127 (with 128: 257
    # endpoints), 128, and the 255-segment strand -- 256 endpoints -- alone
    assert chunks[:, 0].tolist() == [0, 195, 322, 450] and chunks[:, 1].tolist() == [195, 127, 128, 255]
    assert chunks[-1, 1] == 255 and chunks[-1, 3] == 256
    # the endpoints no segment names went where there was room
    assert int(chunks[:, 3].sum()) == E and chunks[:, 3].tolist()[0] == min(256, 200 + loose)


def test_cuts_are_strand_boundaries_only():
    pairs, E = _chains((100,) * 7)
    adj, plan = _plan(pairs, E)
    chunks = _check(pairs, E, adj, plan)
    assert chunks[:, 1].tolist() == [200, 200, 200, 100] and chunks[:, 3].tolist() == [202, 202, 202, 101]


def test_a_strand_that_fits_no_chunk_gives_none():
    pairs, E = _chains((3, 256, 3))          # 256 segments have 257 endpoints
    assert _plan(pairs, E)[1] is None
    pairs, E = _chains((255,))
    adj, plan = _plan(pairs, E)
    assert _check(pairs, E, adj, plan).tolist() == [[0, 255, 0, 256]]


def test_storage_that_is_not_strand_ordered_gives_none():
    pairs, E = _chains(LENS)
    perm = torch.randperm(pairs.shape[0], generator=torch.Generator().manual_seed(0))
    assert _plan(pairs[perm], E)[1] is None


def test_more_loose_endpoints_than_room_gives_none():
    pairs, E = _chains((255,), loose=1)
    assert _plan(pairs, E)[1] is None


def test_single_segments_and_reversed_pairs():
    """Strands of one segment pack 128 to a chunk (256 endpoints); which end of a segment is stored first does not matter."""
    pairs, E = _chains((1,) * 300)
    adj, plan = _plan(pairs.flip(1), E)
    chunks = _check(pairs.flip(1), E, adj, plan)
    assert chunks[:, 1].tolist() == [128, 128, 44]
