"""The resampling contract of the strand export (scene/strand_export.py, csrc/hgs_export.hip) restated as a plain float64 loop, one
strand and one sample at a time with a sequential `cum`, and the strand models the export tests share.  Nothing here is shared
with the product code: the restatement reads the model's strand tables, endpoints and attribute table and nothing else.

Bounds of the comparisons (tests/test_strand_export_cpu.py, tests/test_strand_export_gpu.py): a float64 result rounded once to
float32 is within half a unit of its own last place, and a last place of a value no larger than X is at most 2^-23 X -- positions
within 2^-23 max|coordinate of the strand|, attributes within 2^-23 max|attr column|."""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -23


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def strand_tables(model):
    """(offsets, rows, segment rows of the whole table, endpoints float32, attr float32) of a model, on the host."""
    from scene.strand_export import export_attributes
    si = model.strands_info
    offsets = np.asarray(si.offsets, np.int64)
    rows = np.asarray(si.rows, np.int64).reshape(-1, 2)
    fg = np.nonzero(model.compute_foreground_mask().cpu().numpy())[0]
    seg = fg[np.asarray(si.segment_rows, np.int64)] if rows.shape[0] else np.zeros(0, np.int64)
    return offsets, rows, seg, model._endpoints.detach().cpu().numpy().astype(np.float32), export_attributes(model).cpu().numpy()


def reference_strand(rows, seg, ep, attr, M):
    """One strand (its rows [n,2], segment rows [n]): (points [M or n+1, 3] float32, attrs [.., C] float32, L float64)."""
    n, C = rows.shape[0], attr.shape[1]
    v = [[float(x) for x in ep[rows[i, 0]]] for i in range(n)] + [[float(x) for x in ep[rows[n - 1, 1]]]]
    length, cum = [], [0.0]
    for i in range(n):
        dx, dy, dz = v[i + 1][0] - v[i][0], v[i + 1][1] - v[i][1], v[i + 1][2] - v[i][2]
        length.append(math.sqrt((dx * dx + dy * dy) + dz * dz))
        cum.append(cum[i] + length[i])
    L = cum[n]
    a = []
    for i in range(n + 1):
        if i == 0:
            a.append([float(x) for x in attr[seg[0]]])
        elif i == n:
            a.append([float(x) for x in attr[seg[n - 1]]])
        else:
            a.append([0.5 * (float(attr[seg[i - 1], c]) + float(attr[seg[i], c])) for c in range(C)])
    if M == 0:
        return np.array(v, np.float64).astype(np.float32), np.array(a, np.float64).astype(np.float32), L
    pts, att = [], []
    for j in range(M):
        if j == 0:
            pts.append(v[0]); att.append(a[0])
            continue
        if j == M - 1:
            pts.append(v[n]); att.append(a[n])
            continue
        t = (j / (M - 1)) * L
        i = 0
        for q in range(n + 1):
            if cum[q] <= t:
                i = q
        i = min(i, n - 1)
        w = (t - cum[i]) / length[i] if length[i] > 0 else 0.0
        pts.append([v[i][c] + w * (v[i + 1][c] - v[i][c]) for c in range(3)])
        att.append([a[i][c] + w * (a[i + 1][c] - a[i][c]) for c in range(C)])
    return np.array(pts, np.float64).astype(np.float32), np.array(att, np.float64).astype(np.float32), L


def reference_export(model, M, kept=None):
    """The restatement over the strands `kept` (default: all): (points, attrs, offsets, length [K])."""
    offsets, rows, seg, ep, attr = strand_tables(model)
    S = len(offsets) - 1
    kept = np.arange(S) if kept is None else np.asarray(kept)
    P, A, Ls, off = [], [], [], [0]
    for s in kept:
        o0, o1 = offsets[s], offsets[s + 1]
        p, a, L = reference_strand(rows[o0:o1], seg[o0:o1], ep, attr, M)
        P.append(p); A.append(a); Ls.append(L); off.append(off[-1] + p.shape[0])
    C = attr.shape[1]
    return (np.concatenate(P) if P else np.zeros((0, 3), np.float32), np.concatenate(A) if A else np.zeros((0, C), np.float32),
            np.asarray(off, np.int64), np.asarray(Ls, np.float64))


def assert_close(res, ref, model, attr_strands=None, what=""):
    """res (StrandExport) against reference_export's tuple under the bounds of the module docstring; attributes only on the strands
    `attr_strands` (positions in the kept list; default all).  End samples bit for bit.  Prints the largest differences first."""
    pts, att, off, _ = ref
    assert np.array_equal(res.offsets, off), what
    assert res.points.dtype == np.float32 and res.attrs.dtype == np.float32 and res.points.shape == pts.shape and res.attrs.shape == att.shape, what
    col_max = np.abs(strand_tables(model)[4]).max(axis=0) if att.shape[0] else np.zeros(att.shape[1])
    K = len(off) - 1
    worst_p = worst_a = 0.0
    for k in range(K):
        a, b = off[k], off[k + 1]
        scale = float(np.abs(pts[a:b]).max())
        dp = float(np.abs(res.points[a:b].astype(np.float64) - pts[a:b].astype(np.float64)).max())
        worst_p = max(worst_p, dp / (EPS32 * scale) if scale else dp)
        assert dp <= EPS32 * scale, (what, "positions", k, dp, scale)
        for e in (a, b - 1):
            assert res.points[e].tobytes() == pts[e].tobytes() and res.attrs[e].tobytes() == att[e].tobytes(), (what, "end sample", k)
        if attr_strands is None or k in attr_strands:
            da = np.abs(res.attrs[a:b].astype(np.float64) - att[a:b].astype(np.float64)).max(axis=0)
            worst_a = max(worst_a, float((da / (EPS32 * col_max)).max()))
            assert np.all(da <= EPS32 * col_max), (what, "attributes", k, da, col_max)
    print(f"{what}: {K} strands, worst position difference {worst_p:.3f} units, worst attribute difference {worst_a:.3f} units")


# ---- models ------------------------------------------------------------------------------------------------------------------------
def polyline(rng, n, root=None):
    """n segments of uneven lengths (0.1 to 6 mm, log-uniform) on a jittered walk from a root on a 10 cm sphere."""
    if root is None:
        root = rng.normal(size=3)
        root = 0.1 * root / np.linalg.norm(root)
    d = root / np.linalg.norm(root)
    pts = [root]
    for _ in range(n):
        d = d + rng.normal(size=3) * 0.2
        d = d / np.linalg.norm(d)
        pts.append(pts[-1] + d * 1e-4 * 60.0 ** rng.uniform())
    return np.asarray(pts, np.float32)


def model_from_polylines(lines, device="cpu", seed=0, sh_degree=0, background=False):
    """A strand model of polylines of ANY lengths (HairGaussianModel.from_strands takes one length): consecutive vertices share an
    endpoint; distinct raw attributes per segment, every segment in the foreground; the strand roots are the first vertices."""
    from scene.hair_gaussian_model import HairGaussianModel
    from torch import nn
    rng = np.random.default_rng(1000 + seed)
    m = HairGaussianModel(sh_degree=sh_degree, device=device)
    ep = np.concatenate(lines, axis=0).astype(np.float32) if lines else np.zeros((0, 3), np.float32)
    pairs, start = [], 0
    for ln in lines:
        ids = np.arange(start, start + ln.shape[0])
        pairs.append(np.stack([ids[:-1], ids[1:]], axis=1))
        start += ln.shape[0]
    pairs = np.concatenate(pairs).astype(np.int64) if pairs else np.zeros((0, 2), np.int64)
    P = pairs.shape[0]
    f32 = lambda a: nn.Parameter(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device).requires_grad_(True))
    m._endpoints = f32(ep)
    m.endpoint_pairs = torch.from_numpy(pairs).to(device)
    m._features_dc = f32(rng.normal(size=(P, 1, 3)) * 1.2)              # (some colours leave [0, 1]: the clamp is part of the table)
    m._features_rest = f32(np.zeros((P, (sh_degree + 1) ** 2 - 1, 3)))
    m._opacity = f32(rng.normal(size=(P, 1)) + 1.5)
    m._mask = f32(rng.uniform(1.0, 3.0, size=(P, 1)) if not background else np.full((P, 1), -5.0))   # (background: no strand at all)
    m._width = f32(np.log(1e-4) + rng.normal(size=(P, 1)) * 0.3)
    m.ref_strand_root = np.stack([ln[0] for ln in lines]).astype(np.float64) if lines else np.zeros((0, 3))
    m.strand_root_endpoint_idx = torch.zeros(0, dtype=torch.long, device=device)
    m.active_sh_degree = sh_degree
    if P:
        m.compute_strands_info()
    return m


def uniform_model(S, n_seg=12, device="cpu", seed=0):
    """S strands of n_seg segments; S = 0: one polyline whose segments are all in the background, so the model has no strand."""
    rng = np.random.default_rng(seed)
    m = model_from_polylines([polyline(rng, n_seg) for _ in range(max(S, 1))], device=device, seed=seed, background=(S == 0))
    assert m.strands_info.n_strands == S
    return m


def mixed_model(ns, device="cpu", seed=0):
    """One strand per entry of ns, of that many segments."""
    rng = np.random.default_rng(seed)
    m = model_from_polylines([polyline(rng, n) for n in ns], device=device, seed=seed)
    assert m.strands_info.n_strands == len(ns)
    assert sorted((m.strands_info.offsets[1:] - m.strands_info.offsets[:-1]).tolist()) == sorted(ns)
    return m


def collapsed_model(S, n_seg=12, device="cpu", seed=0):
    """tests/test_growth_gpu.py _strand_model's pattern: the last segment collapsed on strands 1::7, the last four on strands 2::7;
    strand 2 collapsed altogether.  Returns (model, the strands with a collapsed segment: a boolean per strand of the model)."""
    rng = np.random.default_rng(seed)
    pts = np.stack([polyline(rng, n_seg) for _ in range(S)]) if S else np.zeros((0, n_seg + 1, 3), np.float32)
    pts[1::7, -1] = pts[1::7, -2]
    pts[2::7, -4:] = pts[2::7, -5:-4]
    if S > 2:
        pts[2, :] = pts[2, :1]
    m = model_from_polylines(list(pts), device=device, seed=seed)
    assert m.strands_info.n_strands == S
    offsets, rows, _, ep, _ = strand_tables(m)
    d = ep[rows[:, 1]] - ep[rows[:, 0]]
    zero = ~np.any(d != 0, axis=1)
    has = np.array([bool(zero[offsets[s]:offsets[s + 1]].any()) for s in range(S)], bool)
    # (strand s of the model is polyline s: the walk numbers strands by their smaller end id, and the roots are the first vertices)
    first = rows[offsets[:-1], 0]
    assert np.array_equal(ep[first], pts[:, 0])
    return m, has
