"""Seeded scenes for the integer machinery between preprocess and blend (csrc/hgs_preprocess.hip: the rectangle counting of
preprocess_fwd_body and scatter_kernel; csrc/hgs_binning.hip: scan_kernel, sort_tiles_kernel and its two work-list builders):
scenes whose per-tile list LENGTHS, tile RECTANGLES and per-block INSTANCE SUMS are what the case says, so that every size at which
that code takes another path is hit on purpose.  numpy only; tests/binning_reference.py states what the kernels must produce,
tests/test_binning_cases_cpu.py asserts on the CPU oracle what each case below is listed for, tests/test_binning_edges_gpu.py runs them.

Construction (tests/blend_cases.py, vectorised).  A narrow camera (10 degrees) looks down +z; a Gaussian is an isotropic
`cov3D_precomp` at a chosen pixel position.  A "single" has sigma in [1.4, 1.8) pixels (radius 5 or 6) and its centre in
[7.5, 9.5)^2 of a tile: it touches that tile only.  A "rectangle" Gaussian has its radius and centre chosen so that the
reference's getRect gives a wanted tile rectangle (_rect_rows).  Depths come in groups of TIE Gaussians with identical depth
bits (inside a group a list is ordered by id), and the rows of a list scene are stored in shuffled order: id order is not depth
order.  Every scene carries `edges` (what it is for), `bg7`, `extra4`, and what it prescribes: `lengths` [T] and / or `rects`
[P, 4] (x0, y0, x1, y1 in tiles, clipped to the frame; zeros for a culled row) and `blocks`.
"""
import numpy as np

from tests import scenes

# ---- the constants of the code under test, restated once (a changed define makes the reachability assertions of the GPU test
# fail instead of quietly un-testing an edge)
WAVE_SORT_MAX = 128        # csrc/hgs_binning.hip WAVE_SORT_MAX: lists up to this length are sorted by one wavefront
SORT_CAP = 512             # csrc/hgs_common.h HGS_SORT_CAP: keys of one LDS sort chunk
MAX_PARTS = 63             # csrc/hgs_common.h HGS_MAX_PARTS: chunks / segments of one list that cooperate
WL_MAX_CAND = 4096         # csrc/hgs_common.h HGS_WL_MAX_CAND: long lists a frame can have split (work_list_shared)
SC_PART = 4096             # csrc/hgs_preprocess.hip HGS_SC_PART: instances of a block of 256 Gaussians one scatter workgroup places
SC_HELPER_MIN_MEAN = 8     # csrc/hgs_preprocess.hip hgs_launch_scatter: helper workgroups exist from this many instances per Gaussian
PPF_DIRECT = 2048          # csrc/hgs_preprocess.hip HGS_PPF_DIRECT: dealt instances of a block beyond which the LDS tile table is bypassed
TH_MAX_AREA = 16           # csrc/hgs_preprocess.hip TH_MAX_AREA: rectangles of more tiles are dealt across the block
TH_SLOTS = 1024            # csrc/hgs_preprocess.hip TH_LOG: slots of the preprocess kernel's tile table (the scatter kernel's has 512)
SPLIT_FACTOR = 1.5         # csrc/hgs_common.h HGS_SPLIT_QUARTERS / 4: a list longer than this many segment lengths is split
SEG_MIN_LEN = 128          # csrc/hgs_common.h HGS_SEG_MIN_LEN: the shortest segment length
SPLIT_MIN_LEN = int(SPLIT_FACTOR * SEG_MIN_LEN)   # lists up to this length are never split
SEG_POLICY = (128, 1024, 2048)                     # csrc/hgs_binning.hip g_seg_policy: the default of hgs_set_segment_policy
SPLIT_PER_TILE_MIN_T = 1024                        # csrc/hgs_common.h HGS_SPLIT_CAPACITY(T) = max(T, 1024) segment work items
WL_SHARED_MAX_SHARE = 2048                         # csrc/hgs_binning.hip sort_tiles_kernel: tiles per builder that work_list_shared keeps in LDS
WL_BUILDERS = 8                                    # csrc/hgs_common.h HGS_WL_BUILDERS
BLOCK = 256                                        # csrc/hgs_common.h HGS_BLOCK: Gaussians per workgroup of the per-Gaussian kernels

FOV_DEG = 10.0
DEPTH0 = 2.0
TIE = 4                    # Gaussians per group of identical depth bits


def split_of(n, S):
    """(number of segments, segment length) of a list of n entries at segment length S: csrc/hgs_common.h hgs_split_of."""
    if n <= S * 6 // 4:
        return 1, n
    seglen, nseg = S, -(-n // S)
    if nseg > MAX_PARTS:
        seglen = ((-(-n // MAX_PARTS)) + 63) & ~63
        nseg = -(-n // seglen)
    return nseg, seglen


def segment_length(R, policy=SEG_POLICY):
    """csrc/hgs_common.h hgs_segment_length: R / target rounded up to 64, clamped to [min_len, max_len]."""
    lo, hi, target = policy
    return min(max(((R // target) + 63) & ~63, lo), hi)


def uses_shared_builder(T):
    """Does sort_tiles_kernel build this frame's work list with work_list_shared (else: work_list_block, one builder)?"""
    share = -(-(-(-T // WL_BUILDERS)) // BLOCK) * BLOCK
    return share <= WL_SHARED_MAX_SHARE


def grid(W, H):
    return (W + 15) // 16, (H + 15) // 16


def _camera(W, H):
    return scenes.make_camera(eye=(0.0, 0.0, -DEPTH0), target=(0, 0, 0), W=W, H=H, fovx_deg=FOV_DEG)


def _single_rows(W, H, rng, tile_of):
    """(px, py, sigma, rect) of one single-tile Gaussian per entry of `tile_of`."""
    gx, _ = grid(W, H)
    n = len(tile_of)
    tx, ty = tile_of % gx, tile_of // gx
    px, py = 16.0 * tx + rng.uniform(7.5, 9.5, n), 16.0 * ty + rng.uniform(7.5, 9.5, n)
    return px, py, rng.uniform(1.4, 1.8, n), np.stack([tx, ty, tx + 1, ty + 1], 1)


def _axis(t0, n, r):
    """A centre coordinate c (pixels) with int((c - r) / 16) == t0 and int((c + r + 15) / 16) == t0 + n -- the two ends of
    getRect before clipping --, in the middle of the interval that allows, which is at least two pixels wide."""
    lo, hi = max(0.0, 16.0 * n - 2 * r - 15), min(16.0, 16.0 * n - 2 * r + 1)
    assert hi - lo >= 2.0, (n, r)
    return 16.0 * t0 + 0.5 * (lo + hi) + r


def _rect_rows(W, H, cam, rects):
    """(px, py, sigma, rect) of Gaussians whose getRect rectangle, before clipping to the frame, is (x0, y0, w, h) tiles for every
    row of `rects` (|w - h| <= 1: the footprint is a square of 2 r pixels).  The radius is r = ceil(3 sqrt(lambda)) with lambda =
    sigma^2 (1 + tx^2 + ty^2) + 0.3 (an isotropic covariance through the projection's Jacobian at the ray (tx, ty), which the
    reference clamps to 1.3 tan(fov / 2)): sigma is chosen so that 3 sqrt(lambda) = r - 0.5."""
    gx, gy = grid(W, H)
    px, py, sg, out = [], [], [], []
    for x0, y0, w, h in rects:
        lo, hi = 16 * max(w, h) - 29, 16 * min(w, h) - 1
        r = max(3, (lo + hi) // 4)
        assert abs(w - h) <= 1 and lo <= 2 * r <= hi and r >= 3, (w, h)
        cx, cy = _axis(x0, w, r), _axis(y0, h, r)
        tx = np.clip(((2 * cx + 1) / W - 1) * cam["tanfovx"], -1.3 * cam["tanfovx"], 1.3 * cam["tanfovx"])
        ty = np.clip(((2 * cy + 1) / H - 1) * cam["tanfovy"], -1.3 * cam["tanfovy"], 1.3 * cam["tanfovy"])
        px.append(cx)
        py.append(cy)
        sg.append(np.sqrt((((r - 0.5) / 3.0) ** 2 - 0.3) / (1.0 + tx * tx + ty * ty)))
        out.append((min(max(x0, 0), gx), min(max(y0, 0), gy), min(max(x0 + w, 0), gx), min(max(y0 + h, 0), gy)))
    return np.array(px), np.array(py), np.array(sg), np.array(out, np.int64).reshape(-1, 4)


def _scene(name, W, H, seed, px, py, sigma, rect, edges, live=None, order=None, **more):
    """The scene dict of Gaussians at pixel positions (px, py), `sigma` pixels wide, in the order given: row k lies in depth group
    k // TIE.  live[k] False: the row is behind the camera (culled).  order: the permutation the rows are stored in."""
    cam = _camera(W, H)
    rng = np.random.default_rng(seed + 7919)
    P = len(px)
    live = np.ones(P, bool) if live is None else live
    groups = np.arange(P) // TIE
    step = min(1e-3, 0.9 / max(1, int(groups.max(initial=0)) + 1))
    z = DEPTH0 + step * groups
    fx = W / (2.0 * cam["tanfovx"])
    xyz = np.stack([((2.0 * px + 1.0) / W - 1.0) * z * cam["tanfovx"], ((2.0 * py + 1.0) / H - 1.0) * z * cam["tanfovy"],
                    np.where(live, z - DEPTH0, -DEPTH0 - 1.0)], 1)
    s2 = (sigma * z / fx) ** 2
    zero = np.zeros(P)
    cov = np.stack([s2, zero, zero, s2, zero, s2], 1)
    opac = rng.uniform(0.02, 0.3, P)
    opac[rng.uniform(size=P) < 0.03] = 0.002             # below 1 / 255: blended nowhere, quadrant mask 0
    rect = np.where(live[:, None], rect, 0)
    col, extra = rng.uniform(-1.0, 1.0, (P, 3)), rng.uniform(-1.0, 1.0, (P, 4))
    if order is not None:
        xyz, cov, opac, rect, col, extra, live = (a[order] for a in (xyz, cov, opac, rect, col, extra, live))
    gx, gy = grid(W, H)
    # per-tile list lengths the rectangles prescribe (a 2-D difference array: +1 over every rectangle)
    d = np.zeros((gy + 1, gx + 1), np.int64)
    np.add.at(d, (rect[:, 1], rect[:, 0]), 1)
    np.add.at(d, (rect[:, 1], rect[:, 2]), -1)
    np.add.at(d, (rect[:, 3], rect[:, 0]), -1)
    np.add.at(d, (rect[:, 3], rect[:, 2]), 1)
    lengths = d.cumsum(0).cumsum(1)[:gy, :gx].reshape(-1)
    s = dict(cam)
    s.update(name=name, means3D=xyz.astype(np.float32), opacities=opac.astype(np.float32), cov3D_precomp=cov.astype(np.float32),
             colors_precomp=col.astype(np.float32), shs=None, scales=None, rotations=None, sh_degree=0, scale_modifier=1.0,
             bg7=np.array([0.3, -0.2, 0.7, 0.5, -0.4, 0.25, 0.6], np.float32), extra4=extra.astype(np.float32),
             rects=rect, live=live, lengths=lengths, edges=tuple(edges), S=None)
    s["bg"] = s["bg7"][:3].copy()
    s.update(more)
    return s


def _list_scene(name, W, H, seed, lens, edges, tiles=None, **more):
    """Single-tile Gaussians only: tile tiles[k] (default: a seeded choice among all tiles) gets a list of lens[k] entries."""
    rng = np.random.default_rng(seed)
    gx, gy = grid(W, H)
    lens = np.asarray(lens, np.int64)
    assert len(lens) <= gx * gy
    tiles = rng.permutation(gx * gy)[:len(lens)] if tiles is None else np.asarray(tiles, np.int64)
    tile_of = np.repeat(tiles, lens)
    px, py, sg, rect = _single_rows(W, H, rng, tile_of)
    s = _scene(name, W, H, seed, px, py, sg, rect, edges, order=rng.permutation(len(tile_of)), **more)
    want = np.zeros(gx * gy, np.int64)
    want[tiles] = lens
    assert np.array_equal(s["lengths"], want)
    s["long_tiles"] = tiles[lens > WAVE_SORT_MAX]
    return s


LIST_EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 511, 512, 513, 1023, 1024, 1025, 1536, 1537)


def list_edges():
    return _list_scene("list_edges", 96, 64, 31, LIST_EDGE_LENGTHS,
                       ["WAVE_SORT_MAX 127/128/129", "HGS_SORT_CAP 511/512/513 and two full chunks 1023/1024/1025",
                        "three full chunks 1536/1537", "empty, one and two entries", "HGS_SEG_MIN_LEN x 1.5: 192/193"])


def items_do_not_fit():
    return _list_scene("items_do_not_fit", 32, 32, 32, [1025, 1025, 0, 7],
                       ["hgs_emit_sort_items: the chunk items of the second long list do not fit the T slots (HGS_ITEM_NONE)"],
                       tiles=[0, 1, 2, 3])


CHUNK_LIMIT_LENGTHS = (MAX_PARTS * SORT_CAP, MAX_PARTS * SORT_CAP + 1) + (8064,) * 17


def chunk_limit():
    """22 x 16 = 352 tiles: the 63 + 17 x 16 = 335 chunk items all fit the T slots of the sort's work list, whichever list reserves
    first, so the 63-chunk list is merged cooperatively on every run."""
    return _list_scene("chunk_limit", 352, 248, 33, CHUNK_LIMIT_LENGTHS,
                       ["HGS_MAX_PARTS x HGS_SORT_CAP = 32256: the largest cooperative merge", "32257: 64 chunks, the serial fallback"])


def split_lengths(S):
    full = (int(SPLIT_FACTOR * S), int(SPLIT_FACTOR * S) + 1, 2 * S, 2 * S + 1, MAX_PARTS * S, MAX_PARTS * S + 1)
    return full if S == 128 else full[:4]


def split_edges(S):
    return _list_scene(f"split_edges_{S}", 64, 48, 34 + S, split_lengths(S),
                       [f"hgs_split_of at S = {S}: 1.5 S, 1.5 S + 1, 2 S, 2 S + 1" + (", 63 S, 63 S + 1 (re-cut)" if S == 128 else "")], S=S)


def split_capacity(over):
    """S = 128, T = 72 <= 1024: the work list holds 1024 segment items.  16 lists of 63 segments and one of 16 (over: 17)."""
    S = 128
    lens = [MAX_PARTS * S] * 16 + [16 * S + (1 if over else 0)] + [5, 1, 100, 192]
    nseg = sum(split_of(n, S)[0] for n in lens if n > SPLIT_FACTOR * S)
    assert nseg == SPLIT_PER_TILE_MIN_T + (1 if over else 0)
    return _list_scene(f"split_capacity_{nseg}", 144, 128, 36 + over, lens,
                       [f"HGS_SPLIT_CAPACITY(T) = 1024: {nseg} segments, " + ("none split" if over else "all split")], S=S)


def candidate_limit(over, wide=False):
    """HGS_WL_MAX_CAND lists of 193 entries (two segments each at S = 128), or one more.  At 1040 x 1024 (T = 4160) their 8192 / 8194
    segments exceed HGS_SPLIT_CAPACITY(T) = 4160 either way: none is split, and it is the capacity that decides.  `wide`: 1840 x 1152,
    T = 8280 >= 8194 -- the capacity holds both, so the candidate limit decides: 4096 all split, 4097 none.  Both frames are
    work_list_shared's."""
    n = WL_MAX_CAND + (1 if over else 0)
    W, H = (1840, 1152) if wide else (1040, 1024)
    T = grid(W, H)[0] * grid(W, H)[1]
    what = ("none split" if over else "all split") + ": the candidate limit decides" if wide else "none split: HGS_SPLIT_CAPACITY(T) = 4160 decides"
    return _list_scene(f"candidate_limit_{'wide_' if wide else ''}{n}", W, H, 38 + over + 2 * wide, [SPLIT_MIN_LEN + 1] * n + [5] * (T - n),
                       [f"HGS_WL_MAX_CAND: {n} lists of 193 entries at T = {T}, {what} (work_list_shared)"], S=128)


def huge_frame(split):
    """2320 x 1936: 17545 tiles, work_list_block with one builder that places everything from memory."""
    lens = ([SPLIT_MIN_LEN + 1, MAX_PARTS * 128 + 1, 3] if split else [3]) + [1] * 50
    gx, gy = grid(2320, 1936)
    first = [gx * gy - 1, 9000, 0] if split else [gx * gy - 1]      # the long lists: the frame's last tile, a middle one, the first
    rest = np.random.default_rng(40).permutation(np.setdiff1d(np.arange(gx * gy), first))
    tiles = np.concatenate([first, rest[:len(lens) - len(first)]])
    return _list_scene("huge_frame_split" if split else "huge_frame_short", 2320, 1936, 40 + split, lens,
                       ["T = 17545 > 16384: work_list_block, one builder, " + ("place_long and bucket_mem with split lists" if split else "no long list")],
                       tiles=tiles, S=128)


# ---- rectangles ----------------------------------------------------------------------------------------------------------
RECT_W, RECT_H = 200, 300          # 13 x 19 tiles, neither side a multiple of 16
RECT_EDGE_RECTS = {                # name: (x0, y0, w, h) before clipping
    "area16_4x4": (3, 2, 4, 4), "area20_4x5": (5, 8, 4, 5), "area20_5x4": (1, 12, 5, 4), "area9_3x3": (8, 1, 3, 3),
    "area1": (6, 6, 1, 1), "area2_1x2": (2, 9, 1, 2), "area2_2x1": (9, 9, 2, 1), "area4": (10, 14, 2, 2),
    "w1_left_17": (-16, 1, 17, 17), "w2_left_18": (-7, 5, 9, 9), "w1_right_19": (12, -1, 20, 20),
    "w3_right_18": (10, 5, 6, 6), "w3_bottom_right_18_mark_T": (10, 13, 6, 6),
    "top_8x4": (3, -4, 8, 8), "top_5x3": (4, -2, 5, 5), "bottom_8x4": (2, 15, 8, 8),
    "corner_tl_16": (-2, -2, 6, 6), "corner_tr_12": (10, -3, 7, 7), "corner_bl_16": (-3, 15, 7, 7),
    "whole_frame": (-3, -1, 20, 20),
}


def rect_edges():
    cam = _camera(RECT_W, RECT_H)
    rng = np.random.default_rng(41)
    names = list(RECT_EDGE_RECTS) * 3                                    # every rectangle at three depths
    px, py, sg, rect = _rect_rows(RECT_W, RECT_H, cam, [RECT_EDGE_RECTS[n] for n in names])
    gx, gy = grid(RECT_W, RECT_H)
    spx, spy, ssg, srect = _single_rows(RECT_W, RECT_H, rng, rng.integers(0, gx * gy, 300))
    px, py, sg, rect = (np.concatenate(p) for p in ((px, spx), (py, spy), (sg, ssg), (rect, srect)))
    return _scene("rect_edges", RECT_W, RECT_H, 41, px, py, sg, rect,
                  ["TH_MAX_AREA: rectangle areas 16, 17, 18, 19, 20", "row runs of width 1, 2 (direct) and 3 (marked)",
                   "clipped by every frame edge and corner", "a run that ends on the right edge; on the last row: the mark on entry T",
                   "one rectangle covers the frame", "W, H no multiples of 16"],
                  order=rng.permutation(len(px)), rect_names=names)


BLOCK_W, BLOCK_H = 648, 488        # 41 x 31 = 1271 tiles (more than the tile table's 1024 slots), neither side a multiple of 16
BLOCK_LAST_LIVE = (1, 255, 256)


def block_edges(last_live):
    """Blocks of 256 consecutive Gaussians (one workgroup of the preprocess and scatter kernels each) with controlled instance
    sums; `blocks` lists (name, instance sum, dealt instances = those of rectangles above TH_MAX_AREA, distinct tiles)."""
    W, H = BLOCK_W, BLOCK_H
    cam = _camera(W, H)
    gx, gy = grid(W, H)
    rng = np.random.default_rng(42)

    def inner(n, w, h):
        return [(int(rng.integers(0, gx - w + 1)), int(rng.integers(0, gy - h + 1)), w, h) for _ in range(n)]

    plan = [("singles", [], 256, True),
            ("sum_4096", inner(256, 4, 4), 0, True),
            ("culled", [], 256, False),
            ("sum_4100", inner(255, 4, 4) + inner(1, 4, 5), 0, True),
            ("dealt_2048", inner(32, 8, 8), 224, True),
            ("dealt_2049", inner(16, 8, 8) + inner(41, 5, 5), 199, True),
            ("table_overflow", [(-1, -6, 43, 43)], 255, True),
            ("sum_9216", inner(256, 6, 6), 0, True),
            ("last", [], last_live, True)]
    parts, blocks = [], []
    for name, rects, n_single, alive in plan:
        rp = _rect_rows(W, H, cam, rects) if rects else (np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 4), np.int64))
        sp = _single_rows(W, H, rng, rng.integers(0, gx * gy, n_single))
        rows = [np.concatenate(p) for p in zip(rp, sp)]
        n = len(rows[0])
        assert n == BLOCK or name == "last"
        o = rng.permutation(n)
        parts.append([r[o] for r in rows] + [np.full(n, alive)])
        area = (rows[3][:, 2] - rows[3][:, 0]) * (rows[3][:, 3] - rows[3][:, 1]) if alive else np.zeros(n, np.int64)
        cover = np.zeros((gy, gx), bool)
        for x0, y0, x1, y1 in (rows[3] if alive else ()):
            cover[y0:y1, x0:x1] = True
        blocks.append((name, int(area.sum()), int(area[area > TH_MAX_AREA].sum()), int(cover.sum())))
    px, py, sg, rect, live = (np.concatenate([p[k] for p in parts]) for k in range(5))
    return _scene(f"block_edges_{last_live}", W, H, 42, px, py, sg, rect,
                  ["HGS_SC_PART: block sums 4096 (one part), 4100 (owner + helper), 9216 (three parts)",
                   "HGS_PPF_DIRECT: 2048 and 2049 dealt instances", "a block touching more than 1024 distinct tiles: the tile table overflows",
                   f"the last block holds {last_live} live rows", "a block of culled rows"], live=live, blocks=blocks)


CASES = {"list_edges": list_edges, "items_do_not_fit": items_do_not_fit, "chunk_limit": chunk_limit,
         "split_edges_128": lambda: split_edges(128), "split_edges_1024": lambda: split_edges(1024),
         "split_capacity_1024": lambda: split_capacity(0), "split_capacity_1025": lambda: split_capacity(1),
         "candidate_limit_4096": lambda: candidate_limit(0), "candidate_limit_4097": lambda: candidate_limit(1),
         "candidate_limit_wide_4096": lambda: candidate_limit(0, True), "candidate_limit_wide_4097": lambda: candidate_limit(1, True),
         "huge_frame_split": lambda: huge_frame(1), "huge_frame_short": lambda: huge_frame(0), "rect_edges": rect_edges,
         "block_edges_1": lambda: block_edges(1), "block_edges_255": lambda: block_edges(255), "block_edges_256": lambda: block_edges(256)}
BIG = ("candidate_limit_4096", "candidate_limit_4097", "candidate_limit_wide_4096", "candidate_limit_wide_4097", "chunk_limit")        # run in fewer modes (tests/test_binning_edges_gpu.py)
SMALL = tuple(n for n in CASES if n not in BIG)
LIST_CASES = tuple(n for n in CASES if not n.startswith(("rect_", "block_")))   # prescribed list lengths, single-tile Gaussians only
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]
