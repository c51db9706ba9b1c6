"""The integer machinery between preprocess and blend -- the rectangle counting of preprocess_fwd_body, scan_kernel, scatter_kernel,
sort_tiles_kernel and its two work-list builders (csrc/hgs_preprocess.hip, csrc/hgs_binning.hip) -- on the scenes of
tests/binning_cases.py, which sit on every size at which that code takes another path.  Everything compared is an integer (or the
bits of a float), for exact equality, with no exemption: against tests/binning_reference.py fed the kernel's own radii, means2D and
depths, against the CPU oracle, and through check_work_list / check_records.  Every case also asserts, from the status words and
the buffers, that the path it is named for was taken.  (The cases, the reference and the checkers are validated without a GPU in
tests/test_binning_cases_cpu.py.)"""
import contextlib
import itertools

import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import binning_cases as BN
from tests import binning_reference as BR

pytestmark = pytest.mark.gpu

SEVEN = ("radii", "tiles_touched", "point_offsets", "num_rendered", "ranges", "point_list", "keys_sorted")
_oracle, _reference = {}, {}


def _align(v):
    return (v + 255) & ~255


def _binning_layout(R, channels):
    """Byte offsets inside the binning buffer of a pass with `channels` planes (csrc/hgs_common.h hgs_binning_carve; the library's
    hgs_binning_layout states the 3-channel form, which this is checked against)."""
    import hgs_runtime as rt
    lay = {"keys": 0, "point_list": _align(8 * R)}
    lay["packed"] = _align(lay["point_list"] + 4 * R)
    lay["inv"] = _align(lay["packed"] + 16 * (R * (3 if channels == 3 else 4) + 4))
    lay["keys_sorted"] = _align(lay["inv"] + 4 * R)
    if channels == 3:
        assert lay == {k: rt.layout("binning", R)[k] for k in lay}
    return lay


def _run(s, channels):
    """One forward pass through the drop-in module (tile culling off: the reference's lists) and typed views of what it left."""
    import hgs_runtime as rt
    from tests import gpu_util as G
    from tests.test_gpu_raster import _forward7
    W, H, P = s["W"], s["H"], s["means3D"].shape[0]
    gx, gy = BN.grid(W, H)
    T = gx * gy
    if channels == 3:
        fw = G.run_forward(s)
        planes = fw["color"].cpu().numpy()
    else:
        fw = _forward7(s, G.to_dev(s["extra4"]), s["bg7"], cull=False)
        planes = fw["planes"].cpu().numpy()
    R = int(fw["R"])
    g, im = rt.layout("geom", P), rt.layout("image", W, H)
    o = dict(R_cap=R, planes=planes, radii=fw["radii"].cpu().numpy())
    for k, dt, n in (("depths", np.float32, P), ("means2D", np.float32, 2 * P), ("conic_opacity", np.float32, 4 * P),
                     ("tiles_touched", np.uint32, P), ("point_offsets", np.uint32, P)):
        o[k] = G._view(fw["geom"], g[k], n, dt)
    o["means2D"], o["conic_opacity"] = o["means2D"].reshape(P, 2), o["conic_opacity"].reshape(P, 4)
    o["ranges"] = G._view(fw["img"], im["ranges"], 2 * T, np.uint32).reshape(T, 2)
    o["status"] = G._view(fw["img"], im["status"], 16, np.uint32)
    o["work_list"] = G.blend_work_list(s, fw)
    # (the chunk work items of the sort, HgsImage.sort_items: T words in front of the work list, both on 256-byte boundaries)
    o["sort_items"] = G._view(fw["img"], im["tile_order"] - _align(4 * T), T, np.uint32)
    o["num_rendered"] = int(o["status"][0])
    lay = _binning_layout(R, channels)
    o["point_list"] = G._view(fw["binning"], lay["point_list"], R, np.uint32)
    o["keys_raw"] = G._view(fw["binning"], lay["keys_sorted"], R, np.uint64)       # depth << 32 | id << 4 | quadrant mask
    o["keys_placed"] = G._view(fw["binning"], lay["keys"], R, np.uint64)
    o["packed"] = G._view(fw["binning"], lay["packed"], R * (12 if channels == 3 else 16), np.uint32)
    pos, tile = BR._positions(o["ranges"])
    ks = np.zeros(R, np.uint64)
    ks[pos] = (tile.astype(np.uint64) << np.uint64(32)) | (o["keys_raw"][pos] >> np.uint64(32))
    o["keys_sorted"] = ks                                                          # the reference's format: tile << 32 | depth bits
    return o


@contextlib.contextmanager
def _settings(S):
    """The segment policy of a case pinned (S) or at its default; every mode setter and the policy back at the defaults after."""
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    L = rt.lib()
    cap = _C.capacity()
    try:
        if S:
            rt.check(L.hgs_set_segment_policy(S, S, 1))
        yield
    finally:
        _C.set_async(False)
        _C.reset_capacity(cap)
        _C.set_row_runs(None)
        _C.set_lazy_records(None)
        rt.check(L.hgs_set_segment_policy(*BN.SEG_POLICY))


def _oracle_of(name):
    if name not in _oracle:
        _oracle[name] = O.forward(BN.case(name), render=False)
    return _oracle[name]


def _reference_of(name, p):
    """binning_reference.lists of the kernel's own radii, means2D and depths: computed from the case's first pass; every later pass
    must have left the same bits of the three, and is then held to the same lists."""
    s = BN.case(name)
    if name not in _reference:
        _reference[name] = (BR.lists(p["radii"], p["means2D"], p["depths"], s["W"], s["H"]), p["radii"], p["means2D"], p["depths"])
    ref, radii, means2D, depths = _reference[name]
    vis = radii > 0
    np.testing.assert_array_equal(p["radii"], radii)
    np.testing.assert_array_equal(p["means2D"][vis].view(np.uint32), means2D[vis].view(np.uint32))
    np.testing.assert_array_equal(p["depths"][vis].view(np.uint32), depths[vis].view(np.uint32))
    return ref


def _expected_sort_items(n):
    """status[4]: chunk work items of the lists longer than one chunk and of at most HGS_MAX_PARTS chunks (hgs_emit_sort_items)."""
    nch = -(-n // BN.SORT_CAP)
    return int(nch[(n > BN.SORT_CAP) & (nch <= BN.MAX_PARTS)].sum())


def _check_pass(name, p, capacity_mode, lazy, channels, what):
    from tests import gpu_util as G
    s, o = BN.case(name), _oracle_of(name)
    T = len(s["lengths"])
    st = p["status"]
    # a set timeout word is a failure to report, not a reason to run again
    assert st[1] == 0 and st[8] == 0, (what, "overflow / wait timeout", st[1], st[8])
    assert st[14] == int(lazy), what
    n = p["num_rendered"]
    assert p["R_cap"] >= n and (capacity_mode or p["R_cap"] == n)
    ref = _reference_of(name, p)
    got = dict(p)
    if capacity_mode:        # the tiles' segments lie in the order they were allocated: compared tile by tile
        got["ranges"], got["point_list"], got["keys_sorted"] = G.in_tile_order(p, n)
    else:
        got["point_list"], got["keys_sorted"] = p["point_list"][:n], p["keys_sorted"][:n]
    for against, r in (("reference", ref), ("oracle", o)):
        for k in SEVEN:
            if k == "radii" and against == "reference":      # (the reference is fed the kernel's radii)
                continue
            if k == "num_rendered":
                assert got[k] == r[k], (what, against, k)
            else:
                np.testing.assert_array_equal(got[k], r[k], err_msg=f"{what}: {k} against the {against}")
    BR.check_work_list(st, p["work_list"], p["ranges"], T, s["S"] or BN.SEG_POLICY, R_cap=p["R_cap"])
    if not lazy:
        BR.check_records(p["packed"], channels, p["ranges"], p["point_list"], p["keys_raw"], p["keys_placed"], p["point_offsets"],
                         p["means2D"], p["conic_opacity"], s["colors_precomp"], s["extra4"], p["radii"], s["W"], s["H"])
    _check_reached(name, s, p, T, capacity_mode)


def _check_reached(name, s, p, T, capacity_mode):
    """The path the case is named for was taken: read off the status words and the buffers."""
    st = p["status"]
    lens = (p["ranges"][:, 1].astype(np.int64) - p["ranges"][:, 0])
    np.testing.assert_array_equal(lens, s["lengths"])
    np.testing.assert_array_equal(BR.get_rect(p["radii"], p["means2D"], s["W"], s["H"]), s["rects"])
    assert st[4] == _expected_sort_items(lens), (st[4], _expected_sort_items(lens))
    items = p["sort_items"][:min(int(st[4]), T)]
    S = s["S"] or BN.segment_length(p["num_rendered"])
    assert st[6] == S
    split_all, nc, nitems = BR.expected_split(lens, T, S, p["R_cap"])
    assert (st[5], st[7]) == ((nitems, nitems + T - nc) if split_all else (0, T))
    if name == "list_edges":
        assert st[4] == 2 + 2 + 2 + 3 + 3 + 4 and (items != 0xFFFFFFFF).all() and S == 128
        assert st[5] == sum(BN.split_of(v, 128)[0] for v in BN.LIST_EDGE_LENGTHS if v > BN.SPLIT_MIN_LEN)
    elif name == "items_do_not_fit":
        # two lists of three chunk items each for T = 4 slots: the one that reserved first has its three, the other's first (the only
        # one inside the array) says "none", and its own workgroup merged it (the lists are the reference's: asserted above)
        assert st[4] == 6 > T and len(items) == 4
        kept = items[items != 0xFFFFFFFF]
        assert len(kept) == 3 and len(set((kept & 0xFFFFFF).tolist())) == 1 and int(kept[0] & 0xFFFFFF) in (0, 1)
        assert sorted((kept >> 24).tolist()) == [0, 1, 2]
    elif name == "chunk_limit":
        assert st[4] == BN.MAX_PARTS + 17 * 16 <= T and (items != 0xFFFFFFFF).all()
        tiles = set((items & 0xFFFFFF).tolist())
        assert int(np.flatnonzero(lens == BN.MAX_PARTS * BN.SORT_CAP)[0]) in tiles            # the largest cooperative merge
        assert int(np.flatnonzero(lens == BN.MAX_PARTS * BN.SORT_CAP + 1)[0]) not in tiles    # 64 chunks: its own workgroup, serially
        assert int(((items & 0xFFFFFF) == np.flatnonzero(lens == BN.MAX_PARTS * BN.SORT_CAP)[0]).sum()) == BN.MAX_PARTS
    elif name.startswith("split_edges"):
        assert split_all and st[5] == sum(BN.split_of(v, S)[0] for v in BN.split_lengths(S)[1:])
    elif name.startswith("split_capacity"):
        assert split_all == name.endswith("1024") and nitems == int(name.rsplit("_", 1)[1]) and (st[5] != 0) == split_all
    elif name.startswith("candidate_limit"):
        assert BN.uses_shared_builder(T) and nc == int(name.rsplit("_", 1)[1])
        assert split_all == (name == "candidate_limit_wide_4096") and (st[5] != 0) == split_all
        if "wide" in name:
            assert nitems <= T                       # the capacity would hold them: the candidate limit decides
    elif name.startswith("huge_frame"):
        assert T > 16384 and not BN.uses_shared_builder(T)
        assert (st[5] == 2 + 43) if name == "huge_frame_split" else (st[5] == 0 and nc == 0)
    elif name.startswith("block_edges"):
        tt = p["tiles_touched"].astype(np.int64)
        for b, (bname, total, dealt, _) in enumerate(s["blocks"]):
            blk = tt[b * BN.BLOCK:(b + 1) * BN.BLOCK]
            assert (int(blk.sum()), int(blk[blk > BN.TH_MAX_AREA].sum())) == (total, dealt), bname
        sums = {b[0]: b for b in s["blocks"]}
        assert sums["sum_4096"][1] == BN.SC_PART < sums["sum_4100"][1] and sums["sum_9216"][1] > 2 * BN.SC_PART
        assert sums["dealt_2048"][2] == BN.PPF_DIRECT == sums["dealt_2049"][2] - 1 and sums["table_overflow"][3] > BN.TH_SLOTS
        assert p["R_cap"] >= BN.SC_HELPER_MIN_MEAN * len(tt)             # the scatter launch had helper workgroups
    elif name == "rect_edges":
        assert {16, 17, 18, 19, 20, T} <= set(p["tiles_touched"].tolist())


def _passes(name, mode, combos):
    """Runs `combos` of (row_runs, lazy, channels) on the case in blocking or capacity mode and checks every pass."""
    from diff_gaussian_rasterization import _C
    s = BN.case(name)
    with _settings(s["S"]):
        if mode == "capacity":
            _C.reset_capacity(0)                   # (a capacity learnt on another scene would be kept)
            _C.set_async(True)
            _C.set_lazy_records(False)
            first = _run(s, 3)                     # the first pass of the mode learns the capacity (it blocks)
            assert first["status"][1] == 0 and first["status"][8] == 0
        for row_runs, lazy, channels in combos:
            what = f"{name} {mode} row_runs={row_runs} lazy={lazy} channels={channels}"
            _C.set_row_runs(row_runs)
            _C.set_lazy_records(lazy)
            p = _run(s, channels)
            if mode == "capacity":
                assert p["R_cap"] == _C.capacity() and _C.check_async() == [p["num_rendered"]], what
            _check_pass(name, p, mode == "capacity", lazy, channels, what)


@pytest.mark.parametrize("mode", ["blocking", "capacity"])
@pytest.mark.parametrize("name", BN.SMALL)
def test_small_cases_in_every_mode(name, mode):
    """The cross product on the small cases: row runs off / on x packed / lazy records x the 3- and the 7-channel pass."""
    _passes(name, mode, list(itertools.product((False, True), (False, True), (3, 7))))


@pytest.mark.parametrize("mode", ["blocking", "capacity"])
@pytest.mark.parametrize("name", BN.BIG)
def test_big_cases(name, mode):
    """candidate_limit and chunk_limit: each mode once with packed and once with lazy records."""
    _passes(name, mode, [(False, False, 3), (False, True, 3)])


@pytest.mark.parametrize("name", ["list_edges", "chunk_limit"])
def test_two_runs_give_the_same_bits(name):
    s = BN.case(name)
    with _settings(s["S"]):
        a, b = _run(s, 3), _run(s, 3)
    assert a["status"][1] == 0 and a["status"][8] == 0 and b["status"][1] == 0 and b["status"][8] == 0
    for k in ("point_list", "keys_sorted", "keys_raw", "ranges"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["planes"].view(np.uint32), b["planes"].view(np.uint32))
