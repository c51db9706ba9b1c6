"""Plain numpy statements of what the binning kernels must produce (csrc/hgs_preprocess.hip: rectangle counting, scatter_kernel;
csrc/hgs_binning.hip: scan_kernel, sort_tiles_kernel, the blend work list).  tests/test_binning_cases_cpu.py validates each against
the C oracle and shows that the two checkers can fail; tests/test_binning_edges_gpu.py holds the kernels to them."""
import numpy as np

from tests import binning_cases as BN

ALPHA_MIN = 1.0 / 255.0 * (1.0 + 1e-4)      # a pixel "needs" a Gaussian from here on (check_records: the mask may be generous, never short)
ORDER_CAP = 511                             # csrc/hgs_common.h HGS_WL_BUCKETS - 1: list lengths the work list's order tells apart


def get_rect(radii, means2D, W, H):
    """The reference's getRect (CR/auxiliary.h:46-56) in its fp32 arithmetic: [P, 4] (x0, y0, x1, y1), zeros where radii <= 0."""
    gx, gy = BN.grid(W, H)
    r = np.asarray(radii).astype(np.float32)
    c16, c1 = np.float32(16), np.float32(1)
    out = np.zeros((len(r), 4), np.int64)
    for k, g in ((0, gx), (1, gy)):
        c = np.asarray(means2D)[:, k].astype(np.float32)
        with np.errstate(invalid="ignore"):
            lo = np.trunc((c - r) / c16)
            hi = np.trunc((((c + r) + c16) - c1) / c16)
        out[:, k] = np.clip(np.nan_to_num(lo), 0, g).astype(np.int64)
        out[:, 2 + k] = np.clip(np.nan_to_num(hi), 0, g).astype(np.int64)
    out[np.asarray(radii) <= 0] = 0
    return out


def lists(radii, means2D, depths, W, H):
    """duplicateWithKeys + the stable sort by (tile, depth bits) + identifyTileRanges (CR/rasterizer_impl.cu:70-138, :300-317) as ONE
    lexsort by (tile, depth bits, id).  Returns tiles_touched, point_offsets (inclusive), ranges, point_list, keys_sorted
    (tile << 32 | depth bits), and for check_records `rects` and `slots` (the Gaussian-major position of every sorted entry)."""
    gx, gy = BN.grid(W, H)
    T, P = gx * gy, len(radii)
    rect = get_rect(radii, means2D, W, H)
    w, h = rect[:, 2] - rect[:, 0], rect[:, 3] - rect[:, 1]
    tt = w * h
    off = np.cumsum(tt)
    R = int(off[-1]) if P else 0
    ids = np.repeat(np.arange(P, dtype=np.int64), tt)
    local = np.arange(R, dtype=np.int64) - np.repeat(off - tt, tt)
    wr = np.maximum(np.repeat(w, tt), 1)
    tile = (np.repeat(rect[:, 1], tt) + local // wr) * gx + np.repeat(rect[:, 0], tt) + local % wr
    dbits = np.ascontiguousarray(depths, np.float32).view(np.uint32).astype(np.int64)[ids]
    order = np.lexsort((ids, dbits, tile))
    count = np.bincount(tile, minlength=T).astype(np.int64)
    start = np.cumsum(count) - count
    ranges = np.stack([start, start + count], 1)
    ranges[count == 0] = 0
    keys = (tile[order].astype(np.uint64) << np.uint64(32)) | dbits[order].astype(np.uint64)
    return dict(tiles_touched=tt.astype(np.uint32), point_offsets=off.astype(np.uint32), num_rendered=R, ranges=ranges.astype(np.uint32),
                point_list=ids[order].astype(np.uint32), keys_sorted=keys, rects=rect, slots=order.astype(np.uint32))


def expected_split(n, T, S, R_cap):
    """The all-or-none rule of the work-list builders: (split_all, candidates, their segments).  A list is a candidate above
    1.5 S; all candidates are split unless their segments exceed min(segment arrays of the pass, HGS_SPLIT_CAPACITY(T)) or -- in
    work_list_shared, whose candidate list is an array -- they number more than HGS_WL_MAX_CAND."""
    seg_cap = min(R_cap // (BN.SEG_MIN_LEN // 2) + 2 if R_cap else 0, max(T, BN.SPLIT_PER_TILE_MIN_T))
    cand = (n > int(BN.SPLIT_FACTOR * S)) if seg_cap else np.zeros(len(n), bool)
    nc = int(cand.sum())
    nitems = int(sum(BN.split_of(int(v), S)[0] for v in n[cand]))
    ok = nc != 0 and nitems <= seg_cap and (nc <= BN.WL_MAX_CAND or not BN.uses_shared_builder(T))
    return ok, nc, nitems


def check_work_list(status, work_list, ranges, T, S_policy, R_cap=None):
    """The blend kernels' work list (sort_tiles_kernel; status = the image buffer's status words, work_list = HgsImage.tile_order):
    split lists as consecutive ascending segments that tile the list exactly and number hgs_split_of's, every other tile exactly
    once with list lengths (capped at 511) non-increasing; all long lists split or none, as expected_split says; status[7] =
    segments + unsplit tiles.  S_policy: the pinned segment length, or the (min, max, target) policy.  R_cap: the instance
    capacity the pass's binning buffer was carved for (default: its instance count).  Returns {split tile: segments}."""
    st = np.asarray(status)
    n_split_items, seg_len, n_work = int(st[5]), int(st[6]), int(st[7])
    assert st[8] == 0 and 128 <= seg_len <= 1024 and seg_len % 64 == 0
    ranges = np.asarray(ranges)
    n = (ranges[:, 1].astype(np.int64) - ranges[:, 0])
    S = BN.segment_length(int(st[0]), S_policy) if isinstance(S_policy, tuple) else int(S_policy)
    assert seg_len == S, (seg_len, S)
    split_all, nc, nitems = expected_split(n, T, S, int(st[0]) if R_cap is None else int(R_cap))
    assert n_split_items == (nitems if split_all else 0), (n_split_items, split_all, nc, nitems)
    assert n_work == n_split_items + T - (nc if split_all else 0), (n_work, n_split_items, T, nc)
    order = work_list[n_split_items:n_work]
    assert (order >> 24 == 0).all()
    split_tiles = {}
    if n_split_items:
        work = work_list[:n_split_items]
        assert (work != 0xFFFFFFFF).all()
        for pos, item in enumerate(work.tolist()):
            split_tiles.setdefault(item & 0xFFFFFF, []).append((pos, item >> 24))
        for t, segs in split_tiles.items():
            pos, idx = zip(*segs)
            assert list(idx) == list(range(len(idx))) and list(pos) == list(range(pos[0], pos[0] + len(pos))), t
            assert n[t] > seg_len + seg_len // 2 and len(idx) <= 63
            step = seg_len if -(-n[t] // seg_len) <= 63 else ((-(-n[t] // 63) + 63) // 64) * 64
            assert len(idx) == -(-n[t] // step), (t, n[t], len(idx), step)
            assert (len(idx), step) == BN.split_of(int(n[t]), seg_len)
    assert sorted(order.tolist() + list(split_tiles)) == list(range(T))
    if split_all or nc == 0:
        assert (n[order] <= seg_len + seg_len // 2).all()
    else:                                   # none may be split: every tile once, whole
        assert not split_tiles and len(order) == T
    L = np.minimum(n, ORDER_CAP)[order]
    assert (np.diff(L) <= 0).all()
    return {t: len(v) for t, v in split_tiles.items()}


def _positions(ranges):
    """List positions of all tiles in tile order, and the tile of each."""
    r = np.asarray(ranges).astype(np.int64)
    n = r[:, 1] - r[:, 0]
    tile = np.repeat(np.arange(len(r)), n)
    pos = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n) + np.repeat(r[:, 0], n)
    return pos, tile


def quadrants_needed(tile, ids, means2D, conic_opacity, W, H, only=None, chunk=1 << 15):
    """[n] masks: bit w set where a float64 evaluation of alpha = opacity exp(power) (CR/forward.cu:340-358, power > 0 skipped)
    finds a pixel of quadrant w (8 x 8 pixels: bit 0 = x, bit 1 = y) of `tile`, inside the frame, with alpha >= ALPHA_MIN.
    only: [n] masks of the quadrants to evaluate (the others read as not needed)."""
    gx, _ = BN.grid(W, H)
    xy, co = np.asarray(means2D, np.float64), np.asarray(conic_opacity, np.float64)
    need = np.zeros(len(ids), np.uint32)
    jy, jx = np.mgrid[0:8, 0:8]
    for w in range(4):
        sel = np.flatnonzero((co[ids, 3] >= ALPHA_MIN) & (True if only is None else ((only >> w) & 1) != 0))
        for a in range(0, len(sel), chunk):
            k = sel[a:a + chunk]
            g = ids[k]
            px = ((tile[k] % gx) * 16 + (w & 1) * 8)[:, None] + jx.reshape(1, -1)
            py = ((tile[k] // gx) * 16 + (w >> 1) * 8)[:, None] + jy.reshape(1, -1)
            dx, dy = xy[g, 0, None] - px, xy[g, 1, None] - py
            power = -0.5 * (co[g, 0, None] * dx * dx + co[g, 2, None] * dy * dy) - co[g, 1, None] * dx * dy
            alpha = np.where((power > 0) | (px >= W) | (py >= H), 0.0, co[g, 3, None] * np.exp(np.minimum(power, 0.0)))
            need[k[(alpha >= ALPHA_MIN).any(1)]] |= np.uint32(1 << w)
    return need


def check_records(packed, channels, ranges, point_list, keys_sorted_raw, keys_unsorted, point_offsets, means2D, conic_opacity, rgb,
                  extra4, radii, W, H):
    """The packed per-instance records the sort kernel writes for the blend kernels (csrc/hgs_binning.hip emit_instance): 48 bytes
    (xy, conic, opacity, rgb, id, quadrant mask, slot) for 3 channels, 64 (... rgb, 4 extra channels, id, mask, slot) for 7.
    packed: the record array as uint32 words; keys_*_raw: the pass's 64-bit keys depth << 32 | id << 4 | mask, sorted and as the
    scatter kernel placed them; point_offsets: inclusive."""
    words = 12 if channels == 3 else 16
    gx, _ = BN.grid(W, H)
    pos, tile = _positions(ranges)
    R = len(pos)
    rec = np.asarray(packed).view(np.uint32)[:words * (int(pos.max()) + 1 if R else 0)].reshape(-1, words)[pos]
    ids = np.asarray(point_list)[pos].astype(np.int64)
    np.testing.assert_array_equal(rec[:, words - 3], ids, err_msg="record id")
    f = [np.asarray(means2D, np.float32)[ids], np.asarray(conic_opacity, np.float32)[ids], np.asarray(rgb, np.float32)[ids]]
    if channels == 7:
        f.append(np.asarray(extra4, np.float32)[ids])
    want = np.ascontiguousarray(np.concatenate(f, 1)).view(np.uint32)
    got = np.concatenate([rec[:, :8], rec[:, 8:9]], 1) if channels == 3 else np.concatenate([rec[:, :12], rec[:, 12:13]], 1)
    np.testing.assert_array_equal(got, want, err_msg="record floats")
    rect = get_rect(radii, means2D, W, H)
    excl = np.asarray(point_offsets).astype(np.int64) - (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    slot = excl[ids] + (tile // gx - rect[ids, 1]) * (rect[ids, 2] - rect[ids, 0]) + (tile % gx - rect[ids, 0])
    np.testing.assert_array_equal(rec[:, words - 1], slot, err_msg="record slot")
    np.testing.assert_array_equal(np.sort(rec[:, words - 1]), np.arange(R), err_msg="slots are a permutation")
    ks, ku = np.asarray(keys_sorted_raw)[pos], np.asarray(keys_unsorted)[pos]
    np.testing.assert_array_equal((ks & np.uint64(0xFFFFFFFF)) >> np.uint64(4), ids, err_msg="sorted key id")
    np.testing.assert_array_equal(ku[np.lexsort((ku, tile))], ks, err_msg="sorted keys are the placed keys, tile by tile")
    qmask = rec[:, words - 2]
    np.testing.assert_array_equal(qmask, (ks & np.uint64(0xF)).astype(np.uint32), err_msg="record quadrant mask")
    need = quadrants_needed(tile, ids, means2D, conic_opacity, W, H, only=~qmask & 0xF)
    short = np.flatnonzero(need & ~qmask)
    assert len(short) == 0, f"{len(short)} records lack a quadrant float64 needs, first: position {pos[short[0]]}, id {ids[short[0]]}"


def synth_work_list(n, T, S, R_cap, rng=None):
    """(status, work_list) built from the rules check_work_list states (the CPU test's positive control)."""
    n = np.asarray(n, np.int64)
    split_all, nc, nitems = expected_split(n, T, S, R_cap)
    items = []
    if split_all:
        for t in np.flatnonzero(n > int(BN.SPLIT_FACTOR * S)):
            items += [int(t) | (k << 24) for k in range(BN.split_of(int(n[t]), S)[0])]
    rest = [t for t in range(T) if not (split_all and n[t] > int(BN.SPLIT_FACTOR * S))]
    rest.sort(key=lambda t: -min(int(n[t]), ORDER_CAP))
    st = np.zeros(16, np.uint32)
    st[0], st[5], st[6], st[7] = int(n.sum()), len(items), S, len(items) + len(rest)
    wl = np.full(T + max(T, 1024), 0xFFFFFFFF, np.uint32)
    wl[:len(items) + len(rest)] = items + rest
    return st, wl
