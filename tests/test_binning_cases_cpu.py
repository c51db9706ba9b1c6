"""The binning edge cases (tests/binning_cases.py) and the statements they are graded by (tests/binning_reference.py), checked on
the CPU oracle: every case produces the lists / rectangles / block sums it is named for, the numpy statement of the lists equals
the oracle's arrays, and the two checkers accept what follows their rules and reject each planted defect."""
import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import binning_cases as BN
from tests import binning_reference as BR

_oracle = {}


def _ref(name):
    if name not in _oracle:
        _oracle[name] = O.forward(BN.case(name), render=False)
    return _oracle[name]


def _lengths(o):
    return o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0]


@pytest.mark.parametrize("name", list(BN.CASES))
def test_case_is_what_it_prescribes(name):
    s, o = BN.case(name), _ref(name)
    rect = s["rects"]
    np.testing.assert_array_equal(o["tiles_touched"], (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1]))
    np.testing.assert_array_equal(BR.get_rect(o["radii"], o["means2D"], s["W"], s["H"]), rect)
    np.testing.assert_array_equal(_lengths(o), s["lengths"])
    np.testing.assert_array_equal(o["radii"] > 0, s["live"])
    assert s["edges"]


@pytest.mark.parametrize("name", list(BN.CASES))
def test_numpy_lists_equal_the_oracle(name):
    s, o = BN.case(name), _ref(name)
    got = BR.lists(o["radii"], o["means2D"], o["depths"], s["W"], s["H"])
    assert got["num_rendered"] == o["num_rendered"]
    for k in ("tiles_touched", "point_offsets", "ranges", "point_list", "keys_sorted"):
        np.testing.assert_array_equal(got[k], o[k], err_msg=k)


@pytest.mark.parametrize("name", BN.LIST_CASES)
def test_lists_have_depth_ties_and_ids_out_of_depth_order(name):
    s, o = BN.case(name), _ref(name)
    for t in s["long_tiles"]:
        a, e = o["ranges"][t]
        d = o["keys_sorted"][a:e] & np.uint64(0xFFFFFFFF)
        tied = np.zeros(e - a, bool)
        tied[1:] |= d[1:] == d[:-1]
        tied[:-1] |= d[1:] == d[:-1]
        assert tied.mean() >= 0.5, (t, tied.mean())
        ids = o["point_list"][a:e].astype(np.int64)
        same = d[1:] == d[:-1]
        assert (np.diff(ids)[same] > 0).all()                 # inside a tie group: by id
        assert (np.diff(ids)[~same] < 0).mean() > 0.25        # across groups: id order is not depth order


def test_named_lengths():
    assert tuple(sorted(BN.case("list_edges")["lengths"][BN.case("list_edges")["lengths"] > 0])) == BN.LIST_EDGE_LENGTHS[1:]
    assert (BN.case("list_edges")["lengths"] == 0).any()
    assert sorted(BN.case("items_do_not_fit")["lengths"]) == [0, 7, 1025, 1025]
    cl = BN.case("chunk_limit")["lengths"]
    assert (cl == 63 * 512).sum() == 1 and (cl == 63 * 512 + 1).sum() == 1 and (cl == 8064).sum() == 17 and len(cl) >= 63
    assert sorted(BN.case("split_edges_128")["lengths"])[-6:] == [192, 193, 256, 257, 8064, 8065]
    assert sorted(BN.case("split_edges_1024")["lengths"])[-4:] == [1536, 1537, 2048, 2049]
    assert BN.split_of(8065, 128) == (43, 192) and BN.split_of(8064, 128) == (63, 128) and BN.split_of(193, 128) == (2, 128)
    for name, T in (("candidate_limit_4096", 4160), ("candidate_limit_wide_4097", 8280), ("huge_frame_split", 17545), ("huge_frame_short", 17545)):
        assert len(BN.case(name)["lengths"]) == T
    assert BN.uses_shared_builder(4160) and BN.uses_shared_builder(16384) and not BN.uses_shared_builder(17545)
    assert (BN.case("candidate_limit_4096")["lengths"] == 193).sum() == 4096
    assert (BN.case("candidate_limit_4097")["lengths"] == 193).sum() == 4097
    assert (BN.case("candidate_limit_wide_4096")["lengths"] == 193).sum() == 4096
    assert (BN.case("candidate_limit_wide_4097")["lengths"] == 193).sum() == 4097 and BN.uses_shared_builder(8280)
    hs = BN.case("huge_frame_split")["lengths"]
    assert hs[-1] == 193 and hs[9000] == 8065 and hs[0] == 3 and BN.case("huge_frame_short")["lengths"].max() == 3


def test_split_outcomes_the_cases_are_named_for():
    for name, S, want in (("split_capacity_1024", 128, (True, 17, 1024)), ("split_capacity_1025", 128, (False, 17, 1025)),
                          ("candidate_limit_4096", 128, (False, 4096, 8192)), ("candidate_limit_4097", 128, (False, 4097, 8194)),
                          ("candidate_limit_wide_4096", 128, (True, 4096, 8192)), ("candidate_limit_wide_4097", 128, (False, 4097, 8194)),
                          ("huge_frame_split", 128, (True, 2, 45)), ("huge_frame_short", 128, (False, 0, 0))):
        s = BN.case(name)
        assert BR.expected_split(s["lengths"], len(s["lengths"]), S, int(s["lengths"].sum())) == want, name


def test_rect_edges_rectangles():
    s, o = BN.case("rect_edges"), _ref("rect_edges")
    gx, gy = BN.grid(s["W"], s["H"])
    assert s["W"] % 16 and s["H"] % 16
    # (rows are stored shuffled: find each named rectangle by its clipped corners)
    rect = BR.get_rect(o["radii"], o["means2D"], s["W"], s["H"])
    have = {tuple(r) for r in rect.tolist()}
    want = {"area16_4x4": (3, 2, 7, 6), "area20_4x5": (5, 8, 9, 13), "area20_5x4": (1, 12, 6, 16), "w1_left_17": (0, 1, 1, 18),
            "w2_left_18": (0, 5, 2, 14), "w1_right_19": (12, 0, 13, 19), "w3_right_18": (10, 5, 13, 11),
            "w3_bottom_right_18_mark_T": (10, 13, 13, 19), "top_8x4": (3, 0, 11, 4), "top_5x3": (4, 0, 9, 3), "bottom_8x4": (2, 15, 10, 19),
            "corner_tl_16": (0, 0, 4, 4), "corner_tr_12": (10, 0, 13, 4), "corner_bl_16": (0, 15, 4, 19), "whole_frame": (0, 0, gx, gy)}
    for k, r in want.items():
        assert r in have, k
    areas = set(o["tiles_touched"].tolist())
    assert {16, 17, 18, 19, 20, gx * gy} <= areas


def test_block_edges_sums():
    for live in BN.BLOCK_LAST_LIVE:
        s, o = BN.case(f"block_edges_{live}"), _ref(f"block_edges_{live}")
        tt = o["tiles_touched"].astype(np.int64)
        P = len(tt)
        assert P == 8 * BN.BLOCK + live and int((o["radii"][8 * BN.BLOCK:] > 0).sum()) == live
        got = {}
        for b, (name, total, dealt, distinct) in enumerate(s["blocks"]):
            blk = tt[b * BN.BLOCK:(b + 1) * BN.BLOCK]
            assert (int(blk.sum()), int(blk[blk > BN.TH_MAX_AREA].sum())) == (total, dealt), name
            got[name] = (total, dealt, distinct)
        assert got["sum_4096"][0] == BN.SC_PART and got["sum_4100"][0] > BN.SC_PART and got["sum_9216"][0] > 2 * BN.SC_PART
        assert got["dealt_2048"][1] == BN.PPF_DIRECT and got["dealt_2049"][1] == BN.PPF_DIRECT + 1
        assert got["table_overflow"][2] > BN.TH_SLOTS and got["table_overflow"][1] <= BN.PPF_DIRECT
        assert got["culled"][0] == 0 and got["last"][0] == live
        assert o["num_rendered"] >= BN.SC_HELPER_MIN_MEAN * P         # the scatter launch has helper workgroups


# ---- the checkers: accept what follows the rules, reject each planted defect ---------------------------------------------
WL_CASES = ("list_edges", "split_edges_128", "split_capacity_1024", "split_capacity_1025", "candidate_limit_4096",
            "candidate_limit_4097", "candidate_limit_wide_4096", "candidate_limit_wide_4097", "huge_frame_split", "huge_frame_short")


def _wl(name):
    s, o = BN.case(name), _ref(name)
    S = s["S"] or BN.segment_length(o["num_rendered"])
    T = len(s["lengths"])
    st, wl = BR.synth_work_list(s["lengths"], T, S, o["num_rendered"])
    return s, o, S, T, st, wl


@pytest.mark.parametrize("name", WL_CASES)
def test_check_work_list_accepts_its_own_rules(name):
    s, o, S, T, st, wl = _wl(name)
    split = BR.check_work_list(st, wl, o["ranges"], T, S)
    want_split = BR.expected_split(s["lengths"], T, S, o["num_rendered"])[0]
    assert bool(split) == want_split
    if name == "list_edges":
        assert BR.check_work_list(st, wl, o["ranges"], T, BN.SEG_POLICY) == split


def test_check_work_list_rejects_planted_defects():
    s, o, S, T, st, wl = _wl("split_edges_128")
    nsplit, nwork = int(st[5]), int(st[7])
    bad = wl.copy()                                            # a tile listed twice (another one dropped)
    bad[nwork - 1] = bad[nwork - 2]
    with pytest.raises(AssertionError):
        BR.check_work_list(st, bad, o["ranges"], T, S)
    bad, st2 = np.delete(wl, 1), st.copy()                     # a missing segment
    st2[5], st2[7] = nsplit - 1, nwork - 1
    with pytest.raises(AssertionError):
        BR.check_work_list(st2, bad, o["ranges"], T, S)
    bad = wl.copy()                                            # segments out of order
    bad[0], bad[1] = wl[1], wl[0]
    with pytest.raises(AssertionError):
        BR.check_work_list(st, bad, o["ranges"], T, S)
    st2 = st.copy()                                            # the work-item count off by one
    st2[7] += 1
    with pytest.raises(AssertionError):
        BR.check_work_list(st2, wl, o["ranges"], T, S)
    bad = wl.copy()                                            # unsplit tiles not in descending length
    bad[nsplit], bad[nwork - 1] = wl[nwork - 1], wl[nsplit]
    with pytest.raises(AssertionError):
        BR.check_work_list(st, bad, o["ranges"], T, S)
    # a list split in a frame where none may be: the work list of the same lengths as if the capacity were one larger
    s, o, S, T, st, wl = _wl("split_capacity_1025")
    n = s["lengths"]
    items = [int(t) | (k << 24) for t in np.flatnonzero(n > 192) for k in range(BN.split_of(int(n[t]), S)[0])]
    rest = sorted((t for t in range(T) if n[t] <= 192), key=lambda t: -min(int(n[t]), 511))
    st2, bad = st.copy(), wl.copy()
    st2[5], st2[7] = len(items), len(items) + len(rest)
    bad[:len(items) + len(rest)] = items + rest
    with pytest.raises(AssertionError):
        BR.check_work_list(st2, bad, o["ranges"], T, S)
    # ... and none split where all must be
    s, o, S, T, st, wl = _wl("split_capacity_1024")
    st2, bad = st.copy(), wl.copy()
    whole = sorted(range(T), key=lambda t: -min(int(s["lengths"][t]), 511))
    st2[5], st2[7] = 0, T
    bad[:T] = whole
    with pytest.raises(AssertionError):
        BR.check_work_list(st2, bad, o["ranges"], T, S)


def _synth_records(s, o, channels):
    """Records, sorted and placed keys written from check_records' own rules on the oracle's lists."""
    W, H = s["W"], s["H"]
    gx, _ = BN.grid(W, H)
    ref = BR.lists(o["radii"], o["means2D"], o["depths"], W, H)
    R = o["num_rendered"]
    pos, tile = BR._positions(o["ranges"])
    assert np.array_equal(pos, np.arange(R))
    ids = o["point_list"].astype(np.int64)
    mask = BR.quadrants_needed(tile, ids, o["means2D"], o["conic_opacity"], W, H)
    f = [o["means2D"][ids], o["conic_opacity"][ids], s["colors_precomp"][ids]] + ([s["extra4"][ids]] if channels == 7 else [])
    fl = np.ascontiguousarray(np.concatenate(f, 1).astype(np.float32)).view(np.uint32)
    tail = np.stack([ids.astype(np.uint32), mask, ref["slots"]], 1)
    rec = np.concatenate([fl, tail], 1)
    assert rec.shape[1] == (12 if channels == 3 else 16)
    ks = ((o["keys_sorted"] & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | (ids.astype(np.uint64) << np.uint64(4)) | mask.astype(np.uint64)
    ku = ks.copy()
    rng = np.random.default_rng(0)
    for a, e in o["ranges"]:                                  # the scatter kernel places a tile's keys in any order
        ku[a:e] = rng.permutation(ku[a:e])
    return rec, ks, ku, mask


def _check_records(s, o, channels, rec, ks, ku):
    BR.check_records(rec.reshape(-1), channels, o["ranges"], o["point_list"], ks, ku, o["point_offsets"], o["means2D"], o["conic_opacity"],
                     s["colors_precomp"], s["extra4"], o["radii"], s["W"], s["H"])


@pytest.mark.parametrize("name,channels", [("rect_edges", 3), ("rect_edges", 7), ("list_edges", 3), ("block_edges_255", 7)])
def test_check_records_accepts_its_own_rules(name, channels):
    s, o = BN.case(name), _ref(name)
    rec, ks, ku, mask = _synth_records(s, o, channels)
    assert 0 < int((mask != 0xF).sum()) and (mask == 0).any() and (mask == 0xF).any()
    _check_records(s, o, channels, rec, ks, ku)


@pytest.mark.parametrize("channels", [3, 7])
def test_check_records_rejects_planted_defects(channels):
    s, o = BN.case("rect_edges"), _ref("rect_edges")
    rec, ks, ku, mask = _synth_records(s, o, channels)
    words = rec.shape[1]
    k = int(np.flatnonzero(mask == 0xF)[5])

    def planted(col, value, keys=None):
        bad = rec.copy()
        bad[k, col] = value
        with pytest.raises(AssertionError):
            _check_records(s, o, channels, bad, ks if keys is None else keys, ku)

    planted(words - 1, rec[k, words - 1] + 1)                  # a slot off by one
    planted(words - 3, rec[k, words - 3] ^ 1)                  # another Gaussian's id
    planted(3, rec[k, 3] ^ 1)                                  # one bit of a float
    planted(words - 4, rec[k, words - 4] ^ 1)                  # ... of the last colour / extra channel
    planted(words - 2, 0xE)                                    # a mask that is not the key's
    # a cleared quadrant bit that float64 needs, in the record and in both keys alike
    ks2, ku2 = ks.copy(), ku.copy()
    ks2[k] &= ~np.uint64(4)
    a, e = next((a, e) for a, e in o["ranges"] if a <= k < e)     # (the same key may stand in other tiles)
    ku2[a + np.flatnonzero(ku[a:e] == ks[k])[0]] &= ~np.uint64(4)
    bad = rec.copy()
    bad[k, words - 2] &= ~np.uint32(4)
    with pytest.raises(AssertionError, match="quadrant float64 needs"):
        _check_records(s, o, channels, bad, ks2, ku2)
    # two slots swapped: each wrong, still a permutation
    bad = rec.copy()
    bad[[k, k + 1], words - 1] = rec[[k + 1, k], words - 1]
    with pytest.raises(AssertionError):
        _check_records(s, o, channels, bad, ks, ku)
    # a placed key that the sort lost
    ku3 = ku.copy()
    ku3[0] ^= np.uint64(1 << 40)
    with pytest.raises(AssertionError):
        _check_records(s, o, channels, rec, ks, ku3)
