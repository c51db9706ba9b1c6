"""The parameter kernels (hgs_strands.hip, hgs_strand_fwd.h, hgs_strand_bwd.h), the smoothness term (hgs_smooth.h) and Adam
(hgs_adam.h, hgs_optim.hip) against float64 statements on the rows of tests/param_cases.py, with no row exempt.

Everything goes through the C ABI with ctypes.  Every array lives inside a larger allocation with sentinel bytes on both
sides (checked after the launches: a byte written outside stays written), every output starts as NaN.  The bar of every
comparison is per CLASS of rows (tests/param_reference.py): `max|x_hip - x64| <= K * max(e_ref, 4 ulp * scale)`, e_ref the
fp32 CPU statements' own distance from float64 on the class, exactly 0 where the float64 class is exactly 0.
K comes from the table in DESIGN.md section 2 by the rule written there: twice the worst ratio measured on the MI355X over
all classes, rounded up to a power of two, never above 8.  `pytest -s` prints one row per class.  No such run is recorded
yet: K is the ceiling.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import param_cases as PC
from tests import param_reference as R

pytestmark = pytest.mark.gpu

K = 8.0
GUARD = 256                      # sentinel bytes on either side (keeps the payload's 256-byte alignment)
FILL = 0xA5
FS = (PC.F_DEFAULT, 1.0)
SIZES = ("all", 1, 255, 256, 257)
DEVICE = "cuda"


class Dev:
    """A host array's bytes on the device between two runs of sentinel bytes; `offset` bytes in front shift the payload off
    its 16-byte alignment."""

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

    def out(self, *shape, offset=0):
        return self.put(np.full(shape, np.nan, dtype=np.float32), offset)

    def check(self):
        torch.cuda.synchronize()
        for k, d in enumerate(self.items):
            assert d.intact(), f"array {k} {d.shape}: a sentinel byte was overwritten"


def _rt():
    import hgs_runtime as rt
    return rt, rt.lib(), rt.current_stream()


def _judge(title, x, x64, x32, labels, k=K):
    ratios = R.class_ratios(x, x64, x32, labels)
    R.table(title, ratios)
    bad = {n: v for n, v in ratios.items() if not v[1] <= k}
    assert not bad, (title, bad)


# ---- a. strand forward ------------------------------------------------------------------------------------------------------------------------
def _strand_forward(rows, f, pool):
    """hgs_strand_geometry_forward and hgs_params_forward(HGS_PARAMS_HAIR) on the same rows -> (geometry dict, hair dict)."""
    rt, L, st = _rt()
    P = len(rows.pairs)
    ep, pairs, width = pool.put(rows.endpoints), pool.put(rows.pairs), pool.put(rows.width)
    o_raw, m_raw = pool.put(rows.opacity_raw), pool.put(rows.mask_raw)
    g = {"xyz": pool.out(P, 3), "scale": pool.out(P, 3), "quat": pool.out(P, 4), "dir": pool.out(P, 3)}
    rt.check(L.hgs_strand_geometry_forward(st, P, ep.ptr, pairs.ptr, width.ptr, f, g["xyz"].ptr, g["scale"].ptr, g["quat"].ptr,
                                           g["dir"].ptr))
    h = {"xyz": pool.out(P, 3), "scale": pool.out(P, 3), "quat": pool.out(P, 4), "opacity": pool.out(P, 1), "extra4": pool.out(P, 4)}
    pf = rt.ParamForward()
    pf.kind, pf.endpoints, pf.endpoint_pairs, pf.width, pf.dist_to_scale_factor = rt.PARAMS_HAIR, ep.ptr, pairs.ptr, width.ptr, f
    pf.opacity_raw, pf.mask_raw = o_raw.ptr, m_raw.ptr
    pf.means3D, pf.scale, pf.quat, pf.opacity, pf.extra4 = (h[k].ptr for k in ("xyz", "scale", "quat", "opacity", "extra4"))
    rt.check(L.hgs_params_forward(st, P, C.byref(pf), None))
    pool.check()
    dev = {"ep": ep, "pairs": pairs, "width": width, "opacity": h["opacity"], "extra4": h["extra4"]}
    return {k: v.get() for k, v in g.items()}, {k: v.get() for k, v in h.items()}, dev


@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("f", FS, ids=["f_default", "f_1"])
def test_strand_forward_against_float64(f, which):
    """a. Mean, scale, quaternion, direction and the two activations, per class; both entry points give the same bits; the
    collapsed rows are the identity and the half-turn rows (0, 0, 0, 1) bit for bit; |q| = 1 and R(q) x_hat = d."""
    rows, _, r64, r32 = R.strand_reference(f, which, None)
    g, h, _ = _strand_forward(rows, rows.f, Pool())
    for k in ("xyz", "scale", "quat"):
        assert np.array_equal(g[k].view(np.uint32), h[k].view(np.uint32)), k
    assert np.array_equal(g["dir"].view(np.uint32), h["extra4"][:, 1:].view(np.uint32))
    for k in ("xyz", "scale", "quat", "dir"):
        _judge(f"strand fwd {which} f={f:.2g} {k}", g[k], r64[k], r32[k], rows.seg_class)
    _judge(f"strand fwd {which} f={f:.2g} opacity", h["opacity"], r64["opacity"], r32["opacity"], rows.act_class)
    _judge(f"strand fwd {which} f={f:.2g} mask", h["extra4"][:, :1], r64["mask"], r32["mask"], rows.act_class)
    live, rot = r64["live"], r64["rot"]
    assert np.array_equal(g["quat"][~live], np.tile(np.float32([1, 0, 0, 0]), ((~live).sum(), 1)))
    assert np.array_equal(g["dir"][~live], np.tile(np.float32([1, 0, 0]), ((~live).sum(), 1)))
    assert np.array_equal(g["quat"][live & ~rot], np.tile(np.float32([0, 0, 0, 1]), ((live & ~rot).sum(), 1)))
    if which == "all":
        assert (~live).sum() >= 2 * PC.ROWS and (live & ~rot).sum() >= PC.ROWS
    # |q| = 1 within the class's quaternion bar; R(q) x_hat = d within 6 of them plus the direction's own (a column of R is
    # quadratic in q: |d col| <= 4 sqrt(2) |dq|)
    q, d = g["quat"].astype(np.float64), g["dir"].astype(np.float64)
    col = np.stack([1 - 2 * (q[:, 2] ** 2 + q[:, 3] ** 2), 2 * (q[:, 1] * q[:, 2] + q[:, 0] * q[:, 3]),
                    2 * (q[:, 1] * q[:, 3] - q[:, 0] * q[:, 2])], axis=1)
    for c in dict.fromkeys(rows.seg_class):
        s = (rows.seg_class == c) & live
        if not s.any():
            continue
        bar = K * max(np.abs(r32["quat"][s] - r64["quat"][s]).max(), R.ULP4)
        bar_d = K * max(np.abs(r32["dir"][s] - r64["dir"][s]).max(), R.ULP4)
        assert np.abs(np.linalg.norm(q[s], axis=1) - 1).max() <= 2 * bar, c
        assert np.abs(col[s] - d[s]).max() <= 6 * bar + bar_d, c


# ---- b. strand backward -----------------------------------------------------------------------------------------------------------------------
def _adjacency_dev(pool, ids, roles, E, degree):
    from hgs_runtime.strand_step import _adjacency
    t = _adjacency(torch.tensor(np.asarray(ids).reshape(-1), device=DEVICE), roles, E, degree)
    assert t is not None
    return pool.put(t.cpu().numpy())


def _hair_backward(rows, up, mode, fusion=None, f=None):
    """hgs_hair_params_backward on the outputs of hgs_params_forward, the direction's gradient through g_extra4 (what
    training does).  mode: "scatter" | "gather"."""
    rt, L, st = _rt()
    pool = Pool()
    P, E = len(rows.pairs), len(rows.endpoints)
    _, _, dev = _strand_forward(rows, rows.f, pool)
    gx, gs, gq = pool.put(up["xyz"]), pool.put(up["scale"]), pool.put(up["quat"])
    go, ge = pool.put(up["opacity"]), pool.put(np.concatenate([up["mask"], up["dir"]], axis=1))
    d_ep, d_w, d_o, d_m = pool.out(E, 3), pool.out(P), pool.out(P), pool.out(P)
    fu = fusion(pool, rt) if fusion else rt.StrandFusion()
    if mode == "gather":
        fu.ep_segments, fu.n_endpoints = _adjacency_dev(pool, rows.pairs, 2, E, 2).ptr, E
    rt.check(L.hgs_hair_params_backward(st, P, E, dev["ep"].ptr, dev["pairs"].ptr, dev["width"].ptr, rows.f if f is None else f,
                                        dev["opacity"].ptr, dev["extra4"].ptr, gx.ptr, gs.ptr, gq.ptr, None, go.ptr, ge.ptr, 0,
                                        d_ep.ptr, d_w.ptr, d_o.ptr, d_m.ptr, C.byref(fu)))
    pool.check()
    return {"d_endpoints": d_ep.get(), "d_width": d_w.get(), "d_opacity_raw": d_o.get(), "d_mask_raw": d_m.get()}


def _geometry_backward(rows, up, f=None):
    rt, L, st = _rt()
    pool = Pool()
    P, E = len(rows.pairs), len(rows.endpoints)
    ep, pairs, width = pool.put(rows.endpoints), pool.put(rows.pairs), pool.put(rows.width)
    g = [pool.put(up[k]) for k in ("xyz", "scale", "quat", "dir")]
    d_ep, d_w = pool.out(E, 3), pool.out(P)
    rt.check(L.hgs_strand_geometry_backward(st, P, E, ep.ptr, pairs.ptr, width.ptr, rows.f if f is None else f, g[0].ptr, g[1].ptr,
                                            g[2].ptr, g[3].ptr, d_ep.ptr, d_w.ptr))
    pool.check()
    return {"d_endpoints": d_ep.get(), "d_width": d_w.get()}


def _judge_backward(title, got, rows, r64, r32):
    labels = {"d_endpoints": rows.ep_class, "d_width": rows.seg_class, "d_opacity_raw": rows.act_class, "d_mask_raw": rows.act_class}
    for k, x in got.items():
        _judge(f"{title} {k}", x, r64[k], r32[k], labels[k])


UPSTREAMS = ("xyz", "scale", "quat", "dir", "opacity", "mask", None)


@pytest.mark.parametrize("only", UPSTREAMS, ids=lambda o: o or "together")
@pytest.mark.parametrize("f", FS, ids=["f_default", "f_1"])
def test_strand_backward_against_float64_no_row_exempt(f, only):
    """b. Every class and topology (chains, the star, unreferenced endpoints), one upstream gradient at a time and all
    together: hgs_strand_geometry_backward (g_dir) and hgs_hair_params_backward in scatter mode (g_extra4 / g_opacity)."""
    rows, up, r64, r32 = R.strand_reference(f, "all", only)
    if only not in ("opacity", "mask"):
        _judge_backward(f"geometry bwd f={f:.2g} {only}", _geometry_backward(rows, up), rows, r64, r32)
    _judge_backward(f"hair bwd scatter f={f:.2g} {only}", _hair_backward(rows, up, "scatter"), rows, r64, r32)


@pytest.mark.parametrize("only", UPSTREAMS, ids=lambda o: o or "together")
def test_strand_backward_gather_equals_scatter_on_chains(only):
    """b. Gather mode (no atomics; the table from hgs_runtime.strand_step._adjacency) on the independent segments and the
    chains: within the bars, and bit for bit the scatter mode's result (two-term sums commute)."""
    rows, up, r64, r32 = R.strand_reference(PC.F_DEFAULT, "chains", only)
    ga, sc = _hair_backward(rows, up, "gather"), _hair_backward(rows, up, "scatter")
    _judge_backward(f"hair bwd gather {only}", ga, rows, r64, r32)
    for k in ga:
        # (+0 and -0 are the same gradient: an endpoint's first atomic lands on the +0 of the memset)
        assert np.array_equal(ga[k], sc[k]) and np.isfinite(ga[k]).all(), k


@pytest.mark.parametrize("P", SIZES[1:])
@pytest.mark.parametrize("mode", ["scatter", "gather"])
def test_strand_backward_sizes(mode, P):
    """b. P in {1, 255, 256, 257}: one lane, the last lane of a workgroup, a second workgroup of one lane."""
    rows, up, r64, r32 = R.strand_reference(PC.F_DEFAULT, P, None)
    _judge_backward(f"hair bwd {mode} P={P}", _hair_backward(rows, up, mode), rows, r64, r32)
    _judge_backward(f"geometry bwd P={P}", _geometry_backward(rows, up), rows, r64, r32)


def test_no_segments_zero_the_endpoint_gradient():
    """b. P = 0 with E > 0: d_endpoints is zeroed by all three forms."""
    rt, L, st = _rt()
    pool = Pool()
    E = 257
    ep = pool.put(np.zeros((E, 3), np.float32))
    one, pairs = pool.put(np.zeros(4, np.float32)), pool.put(np.zeros((1, 2), np.int64))
    table = pool.put(np.full((E, 2), -1, np.int32))
    d = [pool.out(E, 3) for _ in range(3)]
    rt.check(L.hgs_strand_geometry_backward(st, 0, E, ep.ptr, pairs.ptr, one.ptr, 0.5, None, None, None, None, d[0].ptr, one.ptr))
    for k, gather in ((1, False), (2, True)):
        fu = rt.StrandFusion()
        if gather:
            fu.ep_segments, fu.n_endpoints = table.ptr, E
        rt.check(L.hgs_hair_params_backward(st, 0, E, ep.ptr, pairs.ptr, one.ptr, 0.5, one.ptr, one.ptr, None, None, None, None,
                                            one.ptr, one.ptr, 0, d[k].ptr, one.ptr, one.ptr, one.ptr, C.byref(fu)))
    pool.check()
    for x in d:
        assert not x.get().any() and np.isfinite(x.get()).all()


# ---- c. smoothness ----------------------------------------------------------------------------------------------------------------------------
def _cos(th):
    return float(np.cos(th * np.pi / 180))


def _smooth_standalone(rows, th, eps):
    rt, L, st = _rt()
    pool = Pool()
    N, E = len(rows.pairs), len(rows.endpoints)
    nb = L.hgs_smoothness_num_blocks(N)
    ep, idx, partials = pool.put(rows.endpoints), pool.put(rows.pairs), pool.out(nb, 2)
    rt.check(L.hgs_smoothness_forward(st, N, ep.ptr, idx.ptr, _cos(th), eps, partials.ptr))
    pool.check()
    part = partials.get().astype(np.float64)
    assert np.isfinite(part).all()
    total, count = part[:, 0].sum(), part[:, 1].sum()
    g_loss, cnt, d_ep = pool.put(np.float32([1.0])), pool.put(np.float32([count])), pool.out(E, 3)
    rt.check(L.hgs_smoothness_backward(st, N, E, ep.ptr, idx.ptr, _cos(th), eps, g_loss.ptr, cnt.ptr, d_ep.ptr))
    pool.check()
    return total / max(count, 1.0), count, d_ep.get()


def _smooth_segments(rows):
    """The strand segments under the pairs: the distinct (a0, a1) / (b0, b1) rows."""
    return np.ascontiguousarray(np.unique(rows.pairs.reshape(-1, 2), axis=0))


def _smooth_through_params(rows, th, eps, count, form):
    """The same pairs as the smoothness group of the parameter launches, every rasterizer gradient zero.  form: "scatter" |
    "gather" (hgs_hair_params_backward) | "pair_grads" (hgs_params_forward leaves the pairs' unit gradients, then
    hgs_hair_endpoint_gather reads them)."""
    rt, L, st = _rt()
    seg = _smooth_segments(rows)
    P, E, N = len(seg), len(rows.endpoints), len(rows.pairs)
    z = lambda *s: np.zeros(s, np.float32)
    srows = types.SimpleNamespace(endpoints=rows.endpoints, pairs=seg, width=z(P), opacity_raw=z(P), mask_raw=z(P), f=PC.F_DEFAULT)
    up = {"xyz": z(P, 3), "scale": z(P, 3), "quat": z(P, 4), "dir": z(P, 3), "opacity": z(P, 1), "mask": z(P, 1)}
    head = np.zeros(16, np.float32)
    head[rt.HEAD_OUT.index("g_smooth")], head[rt.HEAD_OUT.index("smooth_count")] = 1.0, count

    def group(pool, rt_):
        fu = rt_.StrandFusion()
        fu.smooth_pairs, fu.n_smooth, fu.cos_threshold, fu.eps = pool.put(rows.pairs).ptr, N, _cos(th), eps
        fu.head_out, fu.grad_out = pool.put(head).ptr, pool.put(np.float32([1.0])).ptr
        if form != "scatter":
            fu.ep_pairs = _adjacency_dev(pool, rows.pairs, 4, E, 4).ptr
        return fu

    if form in ("scatter", "gather"):
        return _hair_backward(srows, up, form, fusion=group)["d_endpoints"]
    pool = Pool()
    fu = group(pool, rt)
    ep, pairs, zero_p = pool.put(rows.endpoints), pool.put(seg), pool.put(z(P))
    nb = L.hgs_smoothness_num_blocks(N)
    partials, pair_grads = pool.out(nb, 2), pool.out(N, 2, 4)
    outs = [pool.out(P, c) for c in (3, 3, 4, 1, 4)]
    pf = rt.ParamForward()
    pf.kind, pf.endpoints, pf.endpoint_pairs, pf.width, pf.dist_to_scale_factor = rt.PARAMS_HAIR, ep.ptr, pairs.ptr, zero_p.ptr, PC.F_DEFAULT
    pf.opacity_raw, pf.mask_raw = zero_p.ptr, zero_p.ptr
    pf.means3D, pf.scale, pf.quat, pf.opacity, pf.extra4 = (o.ptr for o in outs)
    fu.smooth_partials, fu.smooth_pair_grads = partials.ptr, pair_grads.ptr
    rt.check(L.hgs_params_forward(st, P, C.byref(pf), C.byref(fu)))
    pool.check()
    part = partials.get().astype(np.float64)
    assert part[:, 1].sum() == count and np.isfinite(pair_grads.get()).all()
    contrib, d_ep = pool.put(z(P, 2, 4)), pool.out(E, 3)
    fu.ep_segments = _adjacency_dev(pool, seg, 2, E, 2).ptr
    rt.check(L.hgs_hair_endpoint_gather(st, E, contrib.ptr, ep.ptr, d_ep.ptr, C.byref(fu), None))
    pool.check()
    return d_ep.get()


@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("th", PC.THRESHOLDS)
def test_smoothness_against_float64(th, which):
    """c. Value within max(K |v32 - v64|, 4 ulp), the count exact; the gradient per bend class through the stand-alone
    kernels and the three forms the parameter launches run it in -- exactly 0 on the unselected and the saturated classes
    and on the zero-length pair (class scale 0)."""
    rows, s64, s32 = R.smooth_reference(which, th)
    value, count, d_ep = _smooth_standalone(rows, th, PC.SMOOTH_EPS)
    print(f"value | smooth th={th:g} {which} | {abs(value - s64.value):.1e} | {abs(s32.value - s64.value):.1e} | count {count:.0f}")
    assert count == s64.count
    assert abs(value - s64.value) <= max(K * abs(s32.value - s64.value), R.ULP4 * s64.value)
    _judge(f"smooth bwd th={th:g} {which}", d_ep, s64.d_endpoints, s32.d_endpoints, rows.ep_class)
    assert not d_ep[rows.ep_class == "zero_length"].any()
    for form in ("scatter", "gather", "pair_grads"):
        g = _smooth_through_params(rows, th, PC.SMOOTH_EPS, count, form)
        _judge(f"smooth {form} th={th:g} {which}", g, s64.d_endpoints, s32.d_endpoints, rows.ep_class)


# ---- d. the endpoint gather alone -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_endpoint_gather_sums_its_slots_in_table_order(E):
    """d. hgs_hair_endpoint_gather with synthetic contributions: d_endpoints[i] is the fp32 sum of its slots in table order,
    bit for bit; endpoints with 0, 1 and 2 segments."""
    rt, L, st = _rt()
    rng = np.random.default_rng(E)
    P = E
    codes = rng.permutation(2 * P)
    table, k = np.full((E, 2), -1, np.int32), 0
    for i in range(E):
        deg = (i + 2) % 3
        table[i, :deg] = codes[k:k + deg]
        k += deg
    contrib = rng.standard_normal((2 * P, 4)).astype(np.float32)
    want = np.zeros((E, 3), np.float32)
    for s in range(2):
        has = table[:, s] >= 0
        want[has] = want[has] + contrib[table[has, s], :3]
    pool = Pool()
    ep, d_ep = pool.put(rng.standard_normal((E, 3)).astype(np.float32)), pool.out(E, 3)
    fu = rt.StrandFusion()
    fu.ep_segments = pool.put(table).ptr
    rt.check(L.hgs_hair_endpoint_gather(st, E, pool.put(contrib).ptr, ep.ptr, d_ep.ptr, C.byref(fu), None))
    pool.check()
    assert np.array_equal(d_ep.get().view(np.uint32), want.view(np.uint32))


# ---- e. Stage-I cloud -------------------------------------------------------------------------------------------------------------------------
def _cloud(rows, up):
    rt, L, st = _rt()
    pool = Pool()
    P = len(rows.opacity_raw)
    s, r, o, m = (pool.put(a) for a in (rows.scaling_raw, rows.rotation_raw, rows.opacity_raw, rows.mask_raw))
    scale, quat, opac, ex = pool.out(P, 3), pool.out(P, 4), pool.out(P, 1), pool.out(P, 4)
    pf = rt.ParamForward()
    pf.kind, pf.scaling_raw, pf.rotation_raw, pf.opacity_raw, pf.mask_raw = rt.PARAMS_CLOUD, s.ptr, r.ptr, o.ptr, m.ptr
    pf.scale, pf.quat, pf.opacity, pf.extra4 = scale.ptr, quat.ptr, opac.ptr, ex.ptr
    rt.check(L.hgs_params_forward(st, P, C.byref(pf), None))
    pool.check()
    out = {"scale": scale.get(), "quat": quat.get(), "opacity": opac.get(), "mask": ex.get()[:, :1], "dir": ex.get()[:, 1:]}
    if up is not None:
        gs, gq, go = pool.put(up["scale"]), pool.put(up["quat"]), pool.put(up["opacity"])
        ge = pool.put(np.concatenate([up["mask"], up["dir"]], axis=1))
        d = {"d_scaling_raw": pool.out(P, 3), "d_rotation_raw": pool.out(P, 4), "d_opacity_raw": pool.out(P), "d_mask_raw": pool.out(P)}
        rt.check(L.hgs_cloud_params_backward(st, P, s.ptr, r.ptr, opac.ptr, ex.ptr, gs.ptr, gq.ptr, go.ptr, ge.ptr,
                                             d["d_scaling_raw"].ptr, d["d_rotation_raw"].ptr, d["d_opacity_raw"].ptr,
                                             d["d_mask_raw"].ptr, None))
        pool.check()
        out.update({k: v.get() for k, v in d.items()})
    return out


@pytest.mark.parametrize("P", PC.CLOUD_P)
def test_cloud_against_float64(P):
    """e. hgs_params_forward(HGS_PARAMS_CLOUD) and hgs_cloud_params_backward with every upstream gradient, per class; on ties
    of the scales the direction is the column of the FIRST largest axis, as torch.argmax takes it."""
    rows, up, c64, c32 = R.cloud_reference(P, None)
    got = _cloud(rows, up)
    for k, x in got.items():
        _judge(f"cloud P={P} {k}", x, c64[k], c32[k], rows.row_class)
    from utils.transform import build_rotation
    Rm = build_rotation(torch.tensor(rows.rotation_raw, dtype=torch.float64)).numpy()
    axis = np.abs(Rm - got["dir"].astype(np.float64)[:, :, None]).max(axis=1).argmin(axis=1)
    assert np.array_equal(axis, c64["axis"])
    if P == 1000:
        for nm, first in (("tie_01", 0), ("tie_02", 0), ("tie_12", 1), ("tie_012", 0)):
            assert (c64["axis"][rows.row_class == nm] == first).all()


@pytest.mark.parametrize("only", PC.CLOUD_OUTPUTS)
def test_cloud_backward_one_upstream_at_a_time(only):
    rows, up, c64, c32 = R.cloud_reference(1000, only)
    got = _cloud(rows, up)
    for k in ("d_scaling_raw", "d_rotation_raw", "d_opacity_raw", "d_mask_raw"):
        _judge(f"cloud bwd {only} {k}", got[k], c64[k], c32[k], rows.row_class)


# ---- f. Adam ----------------------------------------------------------------------------------------------------------------------------------
def _adam(prob, offset=0, own_tickets=True, beta1=PC.BETA1, beta2=PC.BETA2, eps=PC.ADAM_EPS, lr_factor=1.0):
    """prob.T launches per call of hgs_adam_step; after every launch every step counter has advanced by exactly 1 and the
    ticket words are back to 0; the sentinels are read once at the end (a byte written outside by any launch stays written).
    offset: bytes in front of p / g / m / v (4: the scalar path).  -> list of (p, m, v)."""
    rt, L, st = _rt()
    pool = Pool()
    ts = prob.tensors
    n = len(ts)
    steps, lrs = pool.put(np.float32([t.step0 for t in ts])), pool.put(np.float32([PC.adam_lr(t, 1) * lr_factor for t in ts]))
    tickets = pool.put(np.zeros(rt.ADAM_MAX_TENSORS, np.uint32)) if own_tickets else None
    arr = [{"p": pool.put(t.p0, offset), "g": pool.put(np.zeros(t.n, np.float32), offset), "m": pool.put(t.m0, offset),
            "v": pool.put(t.v0, offset)} for t in ts]
    index = {id(t): k for k, t in enumerate(ts)}
    calls = []
    for call in prob.calls:
        ks = [index[id(t)] for t in call]
        vec = lambda f: (C.c_void_p * len(ks))(*[f(k) for k in ks])
        calls.append((len(ks), vec(lambda k: arr[k]["p"].ptr), vec(lambda k: arr[k]["g"].ptr), vec(lambda k: arr[k]["m"].ptr),
                      vec(lambda k: arr[k]["v"].ptr), vec(lambda k: lrs.ptr + 4 * k), vec(lambda k: steps.ptr + 4 * k),
                      (C.c_longlong * len(ks))(*[ts[k].n for k in ks]), ks))
    for step in range(1, prob.T + 1):
        for k, t in enumerate(ts):
            arr[k]["g"].set(PC.adam_gradient(t.stream, t.n, step, t.seed))
        lrs.set(np.float32([PC.adam_lr(t, step) * lr_factor for t in ts]))
        for nt, p, g, m, v, lr, sp, numel, ks in calls:
            before = steps.get()
            rt.check(L.hgs_adam_step(st, nt, p, g, m, v, lr, sp, numel, beta1, beta2, eps, tickets.ptr if tickets else None))
            torch.cuda.synchronize()
            after = steps.get()
            want = before.copy()
            want[ks] += 1.0
            assert np.array_equal(after, want), (step, before, after)
            if tickets:
                assert not tickets.get().any()
    pool.check()
    return [tuple(a[k].get().astype(np.float64) for k in ("p", "m", "v")) for a in arr]


def _adam_ratios(got, ref, against="abi"):
    """tensor k, array j -> ratio against float64 Adam (`abi`: the betas as the C ABI receives them; `dec`: decimal); the
    yardstick is fp32 torch's distance from its own float64 statement (`dec`)."""
    want = getattr(ref, against)
    out = {}
    for k, t in enumerate(ref.prob.tensors):
        for j, name in enumerate("pmv"):
            if not np.isfinite(got[k][j]).all():
                out[(t.n, name)] = float("inf")
                continue
            e_ref, scale = np.abs(ref.t32[k][j] - ref.dec[k][j]).max(), np.abs(want[k][j]).max()
            bar = max(e_ref, R.ULP4 * scale)
            d = np.abs(got[k][j] - want[k][j]).max()
            out[(t.n, name)] = d / bar if bar > 0 else (0.0 if d == 0 else float("inf"))
    return out


def _adam_judge(title, got, ref):
    abi, dec = _adam_ratios(got, ref, "abi"), _adam_ratios(got, ref, "dec")
    for t in ref.prob.tensors:
        print(f"ratio | {title} | n={t.n} {t.stream} | p {abi[(t.n, 'p')]:.2f} | m {abi[(t.n, 'm')]:.2f} | v {abi[(t.n, 'v')]:.2f} |"
              f" p vs decimal betas {dec[(t.n, 'p')]:.2f} |")
    assert max(abi.values()) <= K, {k: v for k, v in abi.items() if v > K}
    assert max(v for (_, name), v in dec.items() if name == "p") <= K


def _v_contract(got, ref):
    """exp_avg_sq against decimal-beta Adam: off by (1 - fl(0.999)) / 0.001 - 1 relative, to 1e-6 -- the kernel weights g^2 with
    the float the C ABI hands it.  (Elements above 1e-30: below, fp32 has no 1e-6.)"""
    for k in range(len(got)):
        big = ref.dec[k][2] > 1e-30
        if big.any():
            rel = got[k][2][big] / ref.dec[k][2][big] - 1.0
            assert np.abs(rel - R.V_CONTRACT).max() <= 1e-6, (k, rel.min(), rel.max(), R.V_CONTRACT)


@pytest.mark.parametrize("offset,own", [(0, True), (4, True), (0, False), (4, False)], ids=["aligned-own", "scalar-own", "aligned-null", "scalar-null"])
def test_adam_small_sizes_against_float64(offset, own):
    """f. The 13 sizes around the float4 trip, the 1024-element trip and the 4096-element workgroup, 10 steps, one learning
    rate changed in device memory half way: aligned arrays and arrays one float off (the scalar path), an owned ticket
    buffer and tickets = NULL."""
    ref = R.adam_reference("small", 10)
    got = _adam(ref.prob, offset, own)
    _adam_judge(f"adam small T=10 off={offset} own={own}", got, ref)
    _v_contract(got, ref)


@pytest.mark.parametrize("T,offset,own", [(1, 0, True), (1, 4, False), (300, 0, True), (300, 4, False)])
def test_adam_one_and_many_steps(T, offset, own):
    ref = R.adam_reference("small", T)
    got = _adam(ref.prob, offset, own)
    _adam_judge(f"adam small T={T} off={offset}", got, ref)
    if T == 1:
        _v_contract(got, ref)


def test_adam_above_six_mi_elements():
    """f. One call of 8 tensors above 6 * 2^20 elements: 8192 elements per workgroup, 769 workgroups on one ticket."""
    ref = R.adam_reference("big", 3)
    _adam_judge("adam big T=3", _adam(ref.prob), ref)


def test_adam_late_joiner_takes_its_own_bias_corrections():
    """f. One tensor at step 0 beside seven at step 100 (with their moments) in one launch."""
    ref = R.adam_reference("late", 10)
    _adam_judge("adam late T=10", _adam(ref.prob), ref)


# ---- g. the bar sees a wrong constant ---------------------------------------------------------------------------------------------------------
def test_the_bar_sees_a_wrong_scale_factor():
    """g. f is an argument of the C ABI: with f * (1 + 1e-4) the scale and the scale's gradient must FAIL the comparator
    against the unperturbed float64 reference."""
    rows, up, r64, r32 = R.strand_reference(PC.F_DEFAULT, "all", "scale")
    rt, L, st = _rt()
    for f, ok in ((rows.f, True), (float(np.float32(rows.f * (1 + 1e-4))), False)):
        g, _, _ = _strand_forward(rows, f, Pool())
        assert R.accepts(g["scale"], r64["scale"], r32["scale"], rows.seg_class, K) == ok
        for got in (_geometry_backward(rows, up, f), _hair_backward(rows, up, "scatter", f=f)):
            assert R.accepts(got["d_endpoints"], r64["d_endpoints"], r32["d_endpoints"], rows.ep_class, K) == ok


@pytest.mark.parametrize("what", ["beta1", "lr"])
def test_the_bar_sees_a_wrong_adam_constant(what):
    """g. beta1 * (1 + 1e-4) (an argument) and lr * (1 + 1e-4) (device memory): rejected; unperturbed: accepted."""
    ref = R.adam_reference("small", 10)
    assert max(_adam_ratios(_adam(ref.prob), ref).values()) <= K
    kw = {"beta1": float(np.float32(PC.BETA1 * (1 + 1e-4)))} if what == "beta1" else {"lr_factor": 1 + 1e-4}
    worst = max(_adam_ratios(_adam(ref.prob, **kw), ref).values())
    print(f"wrong constant | adam {what} | {worst:.1f} |")
    assert worst > K


def test_the_bar_sees_a_wrong_smoothness_eps():
    """g. eps = 2e-6 saturates the clamp on the 179.9-degree classes (1 + dot = 1.5e-6): their gradient must fail the bar."""
    rows, s64, s32 = R.smooth_reference("all", 30.0)
    for eps, ok in ((PC.SMOOTH_EPS, True), (2e-6, False)):
        _, _, d_ep = _smooth_standalone(rows, 30.0, eps)
        ratios = R.class_ratios(d_ep, s64.d_endpoints, s32.d_endpoints, rows.ep_class)
        for c in ("bend_179.9_5e-3", "bend_179.9_mixed"):
            assert (ratios[c][1] <= K) == ok, (c, ratios[c])
