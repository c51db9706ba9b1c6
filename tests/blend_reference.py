"""float64 reference, fp32 statements and comparator for blend_fwd_kernel / blend_bwd_kernel (csrc/hgs_blend.hip).

The reference ISOLATES the blend: it is the float64 walk (oracle/raster_oracle.c, -DORACLE_F64: hgs_oracle_render_f64 and
hgs_oracle_render_backward_f64) of the fp32 2-D state -- means2D, conic_opacity, colours, ranges, point_list, which the GPU
tests show to be the kernel's bit for bit -- widened to double.  Its backward runs on its OWN final_T and n_contrib; the
kernel's runs on the kernel's own: a forward transmittance error is not handed across and cannot cancel.

Clear pixels.  fp32 and float64 may take a threshold decision differently, so the float64 walk (restated here in numpy,
pinned against the C build by tests/test_blend_f64_cpu.py) marks a pixel CLEAR when every entry it evaluates before its stop
keeps |alpha 255 - 1| >= 1e-4, |power| >= 1e-5 and, for an entry that passes the alpha test, |T (1 - alpha) / 1e-4 - 1| >=
max(1e-3, 8 m 2^-24) with m the entries blended so far.  Forward comparisons cover clear pixels, where n_contrib must EQUAL
the float64 walk's; dL_dpix is zeroed elsewhere on every side (each term is linear in its pixel's dL_dpix).

Yardstick: the distance of fp32 statements of the same blend from float64 on the same input, floored;
the bar is K yardsticks.  The statements, all numpy float32 with one rounding per operation, vectorised over a tile's pixels:
  oracle    the oracle's order of operations (bit for bit O.forward / O.backward);
  segments  the kernel's association (hgs_blend.hip's header): per-segment local transmittance scaled by the product in front,
            c (alpha T_local) T_in, a re-walk of the stop segment, colours summed back to front, the backward started from the
            transmittance and the suffix colour the forward left, T * rcp(1 - alpha), the scalar colour dot product and the
            moments of u = G dL/dalpha that preprocess_bwd_kernel combines once per Gaussian;
  exp_ulp   `oracle` with each exp result moved by a seeded -1, 0 or +1 ulp (v_exp_f32 against libm);
  rcp_ulp   `segments` with each reciprocal of 1 - alpha moved by a seeded -1, 0 or +1 ulp (v_rcp_f32, 1 ulp, against a
            division): the backward rebuilds T by one such multiplication per entry, so the error walks along a segment --
            added because the MI355X showed it: at segment length 1024 the kernel sat 8.4 yardsticks of the first three
            statements from float64, its error growing from a segment's back to its front.
e_ref is the envelope (largest distance) over them.

Forward bars, per tile over its clear pixels: max |x - x64| <= K max(e_ref, 4 x 2^-23 x scale), with scale = the tile's largest
sum_k |c_k| alpha_k T_k + T |bg| for out_color and 1 for final_T, whose error is RELATIVE, |T / T64 - 1|.
Gradient bars, per row and column: |g - g64| <= K max(e_ref, 2^-24 (8 + t_i) S_i): S_i the float64 sum of the magnitudes of
the row's per-(pixel, entry) terms (the oracle's `acc_abs`), 8 = the 6 butterfly levels over 64 lanes + the 2 of the four-wave
combine, t_i = the tiles the Gaussian touches (its per-tile rows are summed serially).  dL_dmeans2D is NOT summed term by
term by the kernel: it sums the moments u dx and u dy and forms sx (-a S(u dx) - b S(u dy)) once per Gaussian, so its S_i is
sx (|a| S|u dx| + |b| S|u dy|) (never below the oracle's term sum) and two more roundings (the 8 becomes 10).
"""
import ctypes as C

import numpy as np

from oracle import hgs_oracle as O
from tests import blend_cases as BC

K_CEILING = 8
STATEMENTS = ("oracle", "segments", "exp_ulp", "rcp_ulp")
SEGMENTED = ("segments", "rcp_ulp")     # the statements that depend on the segment length
TENSORS3 = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors")
TENSORS7 = ("dL_dmeans2D_rgb", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dextra")
FLAWS = ("final_T_scaled", "stop_on_T", "no_clamp", "no_bg_term", "seam_product", "seam_suffix", "outside_live")


def _exp(x):
    """libm's exp on an array, in the array's precision (numpy's float32 exp is not expf bit for bit)."""
    x = np.ascontiguousarray(x)
    out = np.empty_like(x)
    f = O.lib().hgs_oracle_exp_f64 if x.dtype == np.float64 else O.lib().hgs_oracle_exp_f32
    f(C.c_int64(x.size), O._p(x), O._p(out))
    return out


def passes(scene, st, form):
    """The blend passes of a form as (features [P, 3], bg [3], dL_dpix [3, H, W], bg is NULL for the backward): one for the
    3-channel forms; the reference's three for the 7-channel single pass (RGB, mask, direction), whose image planes are
    [0:3] of the first, [0] of the second and [0:3] of the third and whose gradients are summed."""
    rgb = scene["colors_precomp"] if scene["colors_precomp"] is not None else st["rgb"]
    d7, bg7, ex = scene["dpix7"], scene["bg7"], scene["extra4"]
    z = np.zeros_like(d7[0])
    if form == "bg":
        return [(rgb, bg7[:3], d7[:3], False)]
    if form == "black":
        return [(rgb, np.zeros(3, np.float32), d7[:3], True)]
    assert form == "seven"
    return [(rgb, bg7[:3], d7[:3], False),
            (np.repeat(ex[:, 0:1], 3, axis=1), np.repeat(bg7[3:4], 3), np.stack([d7[3], z, z]), False),
            (np.ascontiguousarray(ex[:, 1:4]), bg7[4:7], d7[4:7], False)]


def planes_of(form, outs):
    """[C, H, W] image of a form from its passes' [3, H, W] images."""
    return outs[0] if form != "seven" else np.concatenate([outs[0], outs[1][0:1], outs[2]], axis=0)


# ---------------------------------------------------------------------------------------------------------------------------
# one tile, vectorised over its 256 pixels


class _Tile:
    def __init__(self, st, t, dt, exp_mode="libm", no_clamp=False, outside_live=False, seed=0):
        W, H = st["W"], st["H"]
        gx = (W + 15) // 16
        lx, ly = np.tile(np.arange(16), 16), np.repeat(np.arange(16), 16)
        self.px, self.py = (t % gx) * 16 + lx, (t // gx) * 16 + ly
        self.really_inside = (self.px < W) & (self.py < H)
        self.inside = np.ones(256, bool) if outside_live else self.really_inside
        self.flat = self.py * W + self.px                    # (a lane outside the image: where a live lane would read)
        r0, r1 = (int(v) for v in st["ranges"][t])
        self.ids = st["point_list"][r0:r1].astype(np.int64)
        self.n = n = r1 - r0
        m2, co = st["means2D"][self.ids].astype(dt), st["conic_opacity"][self.ids].astype(dt)
        self.a, self.b, self.c, self.op = (co[:, k:k + 1] for k in range(4))
        self.dx = m2[:, 0:1] - self.px.astype(dt)[None, :]
        self.dy = m2[:, 1:2] - self.py.astype(dt)[None, :]
        dx, dy = self.dx, self.dy
        self.power = dt(-0.5) * (self.a * dx * dx + self.c * dy * dy) - self.b * dx * dy
        self.G = _exp(self.power)
        if exp_mode == "ulp":
            step = np.random.default_rng(seed * 7919 + t).integers(-1, 2, size=self.G.shape)
            up, dn = np.nextafter(self.G, dt(np.inf)), np.nextafter(self.G, dt(-np.inf))
            self.G = np.where(step > 0, up, np.where(step < 0, dn, self.G))
        raw = self.op * self.G
        self.alpha = raw if no_clamp else np.minimum(dt(0.99), raw)
        self.ok = (self.power <= 0) & (self.alpha >= dt(1.0) / dt(255.0))


def _fwd_walk(tl, s, e, T, alive, rule="ref", margins=None):
    """The reference's walk (forward.cu:309-362) over entries [s, e) from transmittance T on the `alive` pixels.  Returns
    (T, stopped, last, add [e-s, 256], Tb [e-s, 256] = the transmittance in front of each entry).  margins: None, or a dict
    {"clear": bool[256], "m": int[256], "stop_pos": int[256]} updated with the float64 margins of the module docstring."""
    dt = T.dtype.type
    one, thr = dt(1.0), dt(0.0001)
    n = e - s
    add_all, Tb = np.zeros((n, 256), bool), np.zeros((n, 256), T.dtype)
    last = np.zeros(256, np.int64)
    stopped = np.zeros(256, bool)
    alive = alive.copy()
    T = T.copy()
    for k in range(s, e):
        a = tl.alpha[k]
        ok = tl.ok[k] & alive
        test = T * (one - a)
        stop = ok & ((T if rule == "T" else test) < thr)
        add = ok & ~stop
        if margins is not None:
            p = tl.power[k]
            near = np.abs(p) < 1e-5
            near |= (p <= 0) & (np.abs(a * 255.0 - 1.0) < 1e-4)
            m = margins["m"] + 1
            near |= ok & (np.abs(test / 1e-4 - 1.0) < np.maximum(1e-3, 8.0 * m * 2.0 ** -24))
            margins["clear"] &= ~(near & alive)
            margins["m"] = np.where(add, m, margins["m"])
            margins["stop_pos"] = np.where(stop, k + 1, margins["stop_pos"])
        add_all[k - s], Tb[k - s] = add, T
        T = np.where(add, test, T)
        last = np.where(add, k + 1, last)
        stopped |= stop
        alive &= ~stop
    return T, stopped, last, add_all, Tb


def _colour(contrib):
    """Sequential sum over entries (axis 0) from zero, in the array's precision."""
    return np.add.accumulate(contrib, axis=0)[-1] if contrib.shape[0] else np.zeros(contrib.shape[1:], contrib.dtype)


def _segments(n, S):
    if S is None:
        return [(0, n)]
    nseg, seglen = BC.split_of(n, S)
    return [(j * seglen, min(n, (j + 1) * seglen)) for j in range(nseg)]


def _forward_tile(tl, feats, bg, dt, S=None, kernel_form=False, rule="ref", flaw=None, want_margins=False):
    """One pass's forward on one tile.  Returns dict(T [256], last [256], C [3, 256], scale [256] (float64 runs), clear,
    and for the kernel form the per-segment state the backward starts from: segs, seg_T [nseg, 256], suffix [nseg, 3, 256])."""
    f = feats[tl.ids].astype(dt)
    one = dt(1.0)
    T0 = np.ones(256, dt)
    out = {}
    segs = _segments(tl.n, S) if kernel_form else [(0, tl.n)]
    if len(segs) <= 2:
        # one workgroup walks the list serially (a list of two segments too: its colours are summed per segment, back to front)
        margins = {"clear": tl.inside.copy(), "m": np.zeros(256, np.int64), "stop_pos": np.zeros(256, np.int64)} if want_margins else None
        T, alive, last = T0, tl.inside.copy(), np.zeros(256, np.int64)
        Cs, seg_T = [], []
        mags = np.zeros((3, 256))
        for (s, e) in segs:
            seg_T.append(T.copy())
            T, stopped, l2, add, Tb = _fwd_walk(tl, s, e, T, alive, rule, margins)
            alive = alive & ~stopped
            last = np.maximum(last, l2)
            al = tl.alpha[s:e]
            w = [np.where(add, (f[s:e, ch:ch + 1] * (al * Tb)) if kernel_form else (f[s:e, ch:ch + 1] * al) * Tb, dt(0)) for ch in range(3)]
            Cs.append(np.stack([_colour(x) for x in w]))
            if dt == np.float64 and e > s:
                mags = mags + np.stack([np.abs(x).sum(axis=0) for x in w])
        Csum = Cs[-1].copy()
        suffix = [None] * len(segs)
        suffix[-1] = Cs[-1]
        for j in range(len(segs) - 2, -1, -1):
            Csum = Csum + Cs[j]
            suffix[j] = Csum.copy()
        out.update(T=T, last=last, C=Csum, segs=segs, seg_T=np.stack(seg_T), suffix=np.stack(suffix))
        if want_margins:
            out["clear"], out["stop_pos"] = margins["clear"] & tl.really_inside, margins["stop_pos"]
        if dt == np.float64:
            out["scale"] = np.max(mags + np.abs(T)[None, :] * np.abs(bg.astype(np.float64))[:, None], axis=0)
        return out
    # ---- three and more segments: pass A from a transmittance of 1, the products in front, pass B for the pixels that stop inside
    nseg = len(segs)
    A = []
    for (s, e) in segs:
        T, stopped, last, add, Tb = _fwd_walk(tl, s, e, T0, tl.inside, rule)
        w = [np.where(add, f[s:e, ch:ch + 1] * (tl.alpha[s:e] * Tb), dt(0)) for ch in range(3)]
        P = np.where(stopped, dt(0), T)
        if flaw == "seam_product" and e > s:          # the product published without the segment's last entry
            P = np.where(stopped, dt(0), np.where(add[-1], Tb[-1], T))
        Clast = np.stack([x[-1] for x in w]) if e > s else np.zeros((3, 256), dt)
        A.append(dict(T=T, stopped=stopped, last=last, C=np.stack([_colour(x) for x in w]), P=P, Clast=Clast))
    seg_T, Tout, neg, lasts, Cs, Cs_sfx = [], [], [], [], [], []
    T_in = T0.copy()
    for j, (s, e) in enumerate(segs):
        if j > 0:
            T_in = T_in * A[j - 1]["P"]
        seg_T.append(T_in.copy())
        a = A[j]
        first = j == 0
        dead = tl.inside & (not first) & (T_in < dt(0.0001))
        through = tl.inside & ~dead & (first | (~a["stopped"] & (T_in * a["T"] >= dt(0.00010002))))
        redo = tl.inside & ~dead & ~through
        T = np.where(through, a["T"] if first else a["T"] * T_in, T_in)
        ng = dead | (through & a["stopped"])
        last = np.where(through, a["last"], 0)
        Cj = np.where(through[None, :], a["C"] if first else a["C"] * T_in[None, :], dt(0))
        if redo.any():
            T2, st2, l2, add, Tb = _fwd_walk(tl, s, e, T_in, redo, rule)
            w = [np.where(add, f[s:e, ch:ch + 1] * (tl.alpha[s:e] * Tb), dt(0)) for ch in range(3)]
            C2 = np.stack([_colour(x) for x in w])
            T, ng, last = np.where(redo, T2, T), np.where(redo, st2, ng), np.where(redo, l2, last)
            Cj = np.where(redo[None, :], C2, Cj)
        Tout.append(T), neg.append(ng), lasts.append(last), Cs.append(Cj)
        # (planted flaw: what the suffix sums take of a segment a pixel passes through misses the segment's last entry)
        Cs_sfx.append(Cj - np.where(through[None, :], a["Clast"] if first else a["Clast"] * T_in[None, :], dt(0)))
    Tfin, nc = T0.copy(), np.zeros(256, np.int64)
    stopped = np.zeros(256, bool)
    lastseg = np.full(256, nseg - 1)
    for j in range(nseg):
        live = ~stopped
        nc = np.where(live, np.maximum(nc, lasts[j]), nc)
        Tfin = np.where(live, Tout[j], Tfin)
        lastseg = np.where(live & neg[j], j, lastseg)
        stopped |= live & neg[j]
    acc = np.zeros((3, 256), dt)
    suffix = [None] * nseg
    for j in range(nseg - 1, -1, -1):
        Cj = Cs_sfx[j] if flaw == "seam_suffix" else Cs[j]
        acc = acc + np.where((j <= lastseg)[None, :], Cj, dt(0))
        suffix[j] = acc.copy()
    Cimg = np.zeros((3, 256), dt)
    for j in range(nseg - 1, -1, -1):
        Cimg = Cimg + np.where((j <= lastseg)[None, :], Cs[j], dt(0))
    return dict(T=Tfin, last=nc, C=Cimg, segs=segs, seg_T=np.stack(seg_T), suffix=np.stack(suffix))


def _backward_tile_ref(tl, feats, bg, dpx, T_final, last, dt, W, H, no_bg_term=False):
    """The oracle's backward walk (backward_distwar.cu:855-1014) of one tile: per-entry sums over the tile's pixels of the nine
    terms [n, 9] (float64 sums of `dt` terms), of their magnitudes, and of |u dx|, |u dy| [n, 2]."""
    n = tl.n
    one = dt(1.0)
    f = feats[tl.ids].astype(dt)
    T = T_final.copy()
    Tk, AR, valid = np.zeros((n, 256), T.dtype), np.zeros((n, 3, 256), T.dtype), np.zeros((n, 256), bool)
    accum, last_color, last_alpha = np.zeros((3, 256), T.dtype), np.zeros((3, 256), T.dtype), np.zeros(256, T.dtype)
    for k in range(n - 1, -1, -1):
        v = tl.ok[k] & (k < last) & tl.inside
        if not v.any():
            continue
        a = tl.alpha[k]
        T = np.where(v, T / (one - a), T)
        accum = np.where(v[None, :], last_alpha[None, :] * last_color + (one - last_alpha)[None, :] * accum, accum)
        last_color = np.where(v[None, :], f[k][:, None], last_color)
        last_alpha = np.where(v, a, last_alpha)
        Tk[k], AR[k], valid[k] = T, accum, v
    al, G, dx, dy = tl.alpha, tl.G, tl.dx, tl.dy
    dcd = al * Tk
    dLa = np.zeros((n, 256), T.dtype)
    cols = []
    for ch in range(3):
        dLa = dLa + (f[:, ch:ch + 1] - AR[:, ch]) * dpx[ch][None, :]
        cols.append(dcd * dpx[ch][None, :])
    dLa = dLa * Tk
    bgd = np.zeros(256, T.dtype)
    for ch in range(3):
        bgd = bgd + dt(bg[ch]) * dpx[ch]
    if not no_bg_term:
        dLa = dLa + (-T_final[None, :] / (one - al)) * bgd[None, :]
    dLdG = tl.op * dLa
    gdx, gdy = G * dx, G * dy
    ddx, ddy = -gdx * tl.a - gdy * tl.b, -gdy * tl.c - gdx * tl.b
    v = [dLdG * ddx * dt(0.5 * W), dLdG * ddy * dt(0.5 * H), dt(-0.5) * gdx * dx * dLdG, dt(-0.5) * gdx * dy * dLdG,
         dt(-0.5) * gdy * dy * dLdG, G * dLa] + cols
    terms = np.stack([np.where(valid, x, dt(0)).astype(np.float64) for x in v], axis=-1)      # [n, 256, 9]
    u = np.where(valid, G * dLa, dt(0)).astype(np.float64)
    mom = np.stack([np.abs(u * dx).sum(axis=1), np.abs(u * dy).sum(axis=1)], axis=-1)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1), mom


def _backward_tile_kernel(tl, feats, bg, dpx, T_final, last, fw, dt, black, rcp_seed=None):
    """The kernel's backward (blend_bwd_kernel) of one tile, segment by segment: per-entry sums over the pixels of the moments
    [u dx, u dy, u dx dx, u dx dy, u dy dy, u, dcolour 0..2]."""
    n = tl.n
    one = dt(1.0)
    f = feats[tl.ids].astype(dt)
    bgd = np.zeros(256, T_final.dtype)
    if not black:
        for ch in range(3):
            bgd = bgd + dt(bg[ch]) * dpx[ch]
    U, Tk = np.zeros((n, 256), T_final.dtype), np.zeros((n, 256), T_final.dtype)
    valid = np.zeros((n, 256), bool)
    segs = fw["segs"]
    rcp_step = None if rcp_seed is None else np.random.default_rng(rcp_seed).integers(-1, 2, size=(n, 256))
    col_dot_all = (f[:, 0:1] * dpx[0][None, :] + f[:, 1:2] * dpx[1][None, :]) + f[:, 2:3] * dpx[2][None, :]
    for j, (s, e) in enumerate(segs):
        T, acc_dot = T_final.copy(), np.zeros(256, T_final.dtype)
        if len(segs) > 1 and j + 1 < len(segs):
            behind = last > e
            Tn = fw["seg_T"][j + 1]
            sfx = fw["suffix"][j + 1]
            d = (sfx[0] * dpx[0] + sfx[1] * dpx[1]) + sfx[2] * dpx[2]
            inv = np.where(Tn > 0, one / np.where(Tn > 0, Tn, one), dt(0))
            T, acc_dot = np.where(behind, Tn, T), np.where(behind, d * inv, acc_dot)
        for k in range(e - 1, s - 1, -1):
            v = tl.ok[k] & (k < last) & tl.inside
            if not v.any():
                continue
            a = np.where(v, tl.alpha[k], dt(0))
            inv = one / (one - a)
            if rcp_step is not None:
                inv = np.where(rcp_step[k] > 0, np.nextafter(inv, dt(np.inf)), np.where(rcp_step[k] < 0, np.nextafter(inv, dt(0)), inv))
            T = T * inv
            cd = col_dot_all[k]
            dLa = (cd - acc_dot) * T
            if not black:
                dLa = dLa + (-T_final * inv) * bgd
            U[k] = np.where(v, tl.G[k], dt(0)) * dLa
            Tk[k], valid[k] = T, v
            acc_dot = a * cd + (one - a) * acc_dot
    ux, uy = U * tl.dx, U * tl.dy
    dcd = np.where(valid, tl.alpha * Tk, dt(0))
    v = [ux, uy, ux * tl.dx, ux * tl.dy, uy * tl.dy, U] + [dcd * dpx[ch][None, :] for ch in range(3)]
    return np.stack([x.astype(np.float64).sum(axis=1) for x in v], axis=-1)


# ---------------------------------------------------------------------------------------------------------------------------
# whole image


def _tiles(st):
    return ((st["W"] + 15) // 16) * ((st["H"] + 15) // 16)


def tile_of_pixel(W, H):
    gx = (W + 15) // 16
    y, x = np.mgrid[0:H, 0:W]
    return (y // 16) * gx + x // 16


def _gather(st, dpix, tl):
    """dL_dpix of a tile's 256 lanes [3, 256]: zero outside the image -- or, for a tile built with outside_live, what a lane that
    believes itself inside reads at py * W + px."""
    flat = dpix.reshape(3, -1)
    idx = np.where(tl.flat < flat.shape[1], tl.flat, 0)
    return np.where((tl.inside & (tl.flat < flat.shape[1]))[None, :], flat[:, idx], 0)


def run(st, pss, dt, clear=None, statement="oracle", S=None, flaw=None, want_margins=False, backward=True):
    """All passes `pss` of one statement over the whole image in precision `dt`.  Returns dict(out [npass][3, H, W], final_T,
    n_contrib, acc [npass][P, 9] float64 (oracle layout), abs [npass][P, 9], mom [npass][P, 2], and with want_margins clear,
    scale [npass][H, W])."""
    W, H, P = st["W"], st["H"], st["means2D"].shape[0]
    dtt = np.dtype(dt).type
    kernel_form = statement in ("segments", "rcp_ulp") or flaw in ("seam_product", "seam_suffix")
    exp_mode = {"exp_ulp": "ulp"}.get(statement, "libm")
    res = dict(out=[np.zeros((3, H, W), dt) for _ in pss], final_T=np.zeros((H, W), dt), n_contrib=np.zeros((H, W), np.uint32),
               acc=[np.zeros((P, 9)) for _ in pss], abs=[np.zeros((P, 9)) for _ in pss], mom=[np.zeros((P, 2)) for _ in pss],
               scale=[np.zeros((H, W)) for _ in pss])
    if want_margins:
        res["clear"], res["stop_pos"] = np.zeros((H, W), bool), np.zeros((H, W), np.int64)   # stop_pos: 1-based list position of the stop, 0: none
    co = st["conic_opacity"].astype(dt)
    for t in range(_tiles(st)):
        tl = _Tile(st, t, dtt, exp_mode, no_clamp=flaw == "no_clamp", outside_live=flaw == "outside_live", seed=17)
        ins = tl.really_inside
        yy, xx = tl.py[ins], tl.px[ins]
        for pi, (feats, bg, dpix, black) in enumerate(pss):
            fw = _forward_tile(tl, feats, bg.astype(dt), dtt, S=S, kernel_form=kernel_form, rule="T" if flaw == "stop_on_T" else "ref",
                               flaw=flaw, want_margins=want_margins and pi == 0)
            img = fw["C"] + fw["T"][None, :] * bg.astype(dt)[:, None]
            res["out"][pi][:, yy, xx] = img[:, ins]
            if "scale" in fw:
                res["scale"][pi][yy, xx] = fw["scale"][ins]
            if pi == 0:
                res["final_T"][yy, xx] = fw["T"][ins]
                res["n_contrib"][yy, xx] = fw["last"][ins]
                if want_margins:
                    res["clear"][yy, xx] = fw["clear"][ins]
                    res["stop_pos"][yy, xx] = fw["stop_pos"][ins]
            if not backward or tl.n == 0:
                continue
            dpm = dpix if clear is None else dpix * clear[None]
            dpx = _gather(st, dpm.astype(dt), tl).astype(dt)
            T_final = np.where(tl.inside, fw["T"], dtt(0))
            if flaw == "final_T_scaled":
                T_final = T_final * dtt(1.0 + 2e-5)
            last = np.where(tl.inside, fw["last"], 0)
            if kernel_form:
                mo = _backward_tile_kernel(tl, feats, bg, dpx, T_final, last, fw, dtt, black,
                                           rcp_seed=104729 * (t + 1) + pi if statement == "rcp_ulp" else None)
                np.add.at(res["acc"][pi], tl.ids, mo)           # (moments: combined per Gaussian below)
            else:
                tm, ab, mo = _backward_tile_ref(tl, feats, bg, dpx, T_final, last, dtt, W, H, no_bg_term=flaw == "no_bg_term")
                np.add.at(res["acc"][pi], tl.ids, tm)
                np.add.at(res["abs"][pi], tl.ids, ab)
                np.add.at(res["mom"][pi], tl.ids, mo)
    if kernel_form and backward:
        # preprocess_bwd_kernel: dmean2D and dconic from the Gaussian's summed moments, in fp32
        for pi in range(len(pss)):
            m = res["acc"][pi].astype(dt)
            a, b, c, op = (co[:, k] for k in range(4))
            sx, sy, h = dtt(0.5) * dtt(W) * op, dtt(0.5) * dtt(H) * op, dtt(-0.5) * op
            out = m.copy()
            out[:, 0] = sx * (-a * m[:, 0] - b * m[:, 1])
            out[:, 1] = sy * (-c * m[:, 1] - b * m[:, 0])
            out[:, 2], out[:, 3], out[:, 4] = m[:, 2] * h, m[:, 3] * h, m[:, 4] * h
            res["acc"][pi] = out.astype(np.float64)
    return res


def grads_of(form, accs):
    """{tensor: [P, k] float64} of a form from its passes' [P, 9] accumulators (sums of the passes where autograd would sum)."""
    a0 = accs[0]
    if form != "seven":
        return {"dL_dmeans2D": a0[:, 0:2], "dL_dconic": a0[:, 2:5], "dL_dopacity": a0[:, 5:6], "dL_dcolors": a0[:, 6:9]}
    tot = accs[0] + accs[1] + accs[2]
    return {"dL_dmeans2D_rgb": a0[:, 0:2], "dL_dconic": tot[:, 2:5], "dL_dopacity": tot[:, 5:6], "dL_dcolors": a0[:, 6:9],
            "dL_dextra": np.concatenate([accs[1][:, 6:7], accs[2][:, 6:9]], axis=1)}


def oracle_f64(st, pss, clear):
    """The C oracle's float64 blend of the widened fp32 state: forward per pass, and the backward on ITS OWN final_T / n_contrib
    with dL_dpix zeroed outside `clear` (None: forward only).  Returns dict(out, final_T, n_contrib, acc, abs)."""
    L = O.lib()
    W, H, P = st["W"], st["H"], st["means2D"].shape[0]
    m2, co = st["means2D"].astype(np.float64), st["conic_opacity"].astype(np.float64)
    res = dict(out=[], acc=[], abs=[])
    for pi, (feats, bg, dpix, black) in enumerate(pss):
        f64, bg64 = np.ascontiguousarray(feats, np.float64), bg.astype(np.float64)
        out, fT, nc = np.zeros((3, H, W)), np.zeros((H, W)), np.zeros((H, W), np.uint32)
        L.hgs_oracle_render_f64(C.c_int(W), C.c_int(H), O._p(st["ranges"]), O._p(st["point_list"]), O._p(m2), O._p(f64), O._p(co),
                                O._p(bg64), O._p(fT), O._p(nc), O._p(out))
        res["out"].append(out)
        if pi == 0:
            res["final_T"], res["n_contrib"] = fT, nc
        if clear is None:
            continue
        d64 = np.ascontiguousarray(dpix.astype(np.float64) * clear[None])
        acc, aabs = np.zeros((P, 9)), np.zeros((P, 9))
        L.hgs_oracle_render_backward_f64(C.c_int(P), C.c_int(W), C.c_int(H), O._p(st["ranges"]), O._p(st["point_list"]), O._p(bg64),
                                         O._p(m2), O._p(co), O._p(f64), O._p(fT), O._p(nc), O._p(d64), O._p(acc), None, None, None,
                                         O._p(aabs))
        res["acc"].append(acc)
        res["abs"].append(aabs)
    return res


_ref_cache = {}


def reference(scene, form, S=None, statements=STATEMENTS):
    """Everything the comparator needs for (scene, form) at segment length S (None: no list is split).  Cached; the float64 side
    and the statements that do not depend on S are computed once per (scene, form)."""
    key = (scene["name"], form)
    if key not in _ref_cache:
        st = O.forward(scene)
        st["W"], st["H"] = scene["W"], scene["H"]
        pss = passes(scene, st, form)
        w64 = run(st, pss, np.float64, want_margins=True, backward=False)
        clear = w64["clear"]
        w64 = run(st, pss, np.float64, clear=clear, want_margins=True)
        c64 = oracle_f64(st, pss, clear)
        base = dict(st=st, pss=pss, clear=clear, walk64=w64, c64=c64, stm={})
        _ref_cache[key] = base
    base = _ref_cache[key]
    st, pss, clear, w64, c64 = (base[k] for k in ("st", "pss", "clear", "walk64", "c64"))
    for name in statements:
        k2 = (name, S if name in SEGMENTED else None)
        if k2 not in base["stm"]:
            base["stm"][k2] = run(st, pss, np.float32, clear=clear, statement=name, S=k2[1])
    stm = {name: base["stm"][(name, S if name in SEGMENTED else None)] for name in statements}
    return assemble(scene, form, base, stm)


def assemble(scene, form, base, stm):
    st, pss, clear, w64, c64 = (base[k] for k in ("st", "pss", "clear", "walk64", "c64"))
    W, H, P = st["W"], st["H"], st["means2D"].shape[0]
    ref = dict(st=st, pss=pss, clear=clear, form=form, statements=stm, walk64=w64, c64=c64)
    ref["out64"] = planes_of(form, c64["out"])
    ref["T64"], ref["n64"] = c64["final_T"], c64["n_contrib"]
    ref["scale_out"] = np.max(np.stack(w64["scale"]), axis=0)
    ref["x64"] = grads_of(form, c64["acc"])
    # magnitudes: the oracle's term sums, and for dL_dmeans2D the kernel's moment form (module docstring)
    co = st["conic_opacity"].astype(np.float64)
    absn = [a.copy() for a in c64["abs"]]
    for pi in range(len(pss)):
        mx, my = w64["mom"][pi][:, 0], w64["mom"][pi][:, 1]
        absn[pi][:, 0] = np.maximum(absn[pi][:, 0], 0.5 * W * co[:, 3] * (np.abs(co[:, 0]) * mx + np.abs(co[:, 1]) * my))
        absn[pi][:, 1] = np.maximum(absn[pi][:, 1], 0.5 * H * co[:, 3] * (np.abs(co[:, 2]) * my + np.abs(co[:, 1]) * mx))
    S_i = grads_of(form, absn)
    t_i = st["tiles_touched"].astype(np.float64)[:, None]
    ref["S"] = S_i
    ref["floor"] = {k: 2.0 ** -24 * ((10.0 if k.startswith("dL_dmeans2D") else 8.0) + t_i) * v for k, v in S_i.items()}
    ref["e_grad"] = {k: np.max(np.stack([np.abs(grads_of(form, s["acc"])[k] - ref["x64"][k]) for s in stm.values()]), axis=0)
                     for k in ref["x64"]}
    top = tile_of_pixel(W, H)
    nT = _tiles(st)
    e_out, e_T = np.zeros(nT), np.zeros(nT)
    for s in stm.values():
        fe = forward_errors(ref, planes_of(form, s["out"]), s["final_T"])
        e_out, e_T = np.maximum(e_out, fe["out_color"]), np.maximum(e_T, fe["final_T"])
    ref["e_fwd"] = {"out_color": e_out, "final_T": e_T}
    sc = np.zeros(nT)
    np.maximum.at(sc, top[clear], ref["scale_out"][clear])
    ref["yard_fwd"] = {"out_color": np.maximum(e_out, 4 * 2.0 ** -23 * sc), "final_T": np.maximum(e_T, 4 * 2.0 ** -23)}
    ref["yard_grad"] = {k: np.maximum(ref["e_grad"][k], ref["floor"][k]) for k in ref["x64"]}
    return ref


def forward_errors(ref, planes, final_T):
    """Per tile, over its clear pixels: max |out_color - out64| and max |final_T / T64 - 1|."""
    st, clear = ref["st"], ref["clear"]
    top = tile_of_pixel(st["W"], st["H"])
    nT = _tiles(st)
    eo, eT = np.zeros(nT), np.zeros(nT)
    d = np.abs(planes.astype(np.float64) - ref["out64"]).max(axis=0)
    np.maximum.at(eo, top[clear], d[clear])
    r = np.abs(final_T.astype(np.float64)[clear] / ref["T64"][clear] - 1.0)
    np.maximum.at(eT, top[clear], r)
    return {"out_color": eo, "final_T": eT}


def _ratio(err, yard):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, np.where(yard > 0, err / np.where(yard > 0, yard, 1.0), np.inf))


def grade(ref, planes, final_T, n_contrib, grads, label=None):
    """Ratios in yardsticks of one implementation's outputs (grads: {tensor: [P, k]} or None).  Returns {name: worst ratio} plus
    "n_contrib": the clear pixels whose count differs; prints one table row per tensor with `label`."""
    out = {}
    fe = forward_errors(ref, planes, final_T)
    for k in ("out_color", "final_T"):
        out[k] = float(_ratio(fe[k], ref["yard_fwd"][k]).max())
    out["n_contrib"] = int((np.asarray(n_contrib)[ref["clear"]] != ref["n64"][ref["clear"]]).sum())
    if grads is not None:
        for k, x in ref["x64"].items():
            g = np.asarray(grads[k], np.float64).reshape(x.shape)
            assert np.isfinite(g).all(), f"{k}: NaN / Inf (an element nobody wrote?)"
            out[k] = float(_ratio(np.abs(g - x), ref["yard_grad"][k]).max()) if x.size else 0.0
    if label is not None:
        for k, v in out.items():
            print(f"BLEND64 {label:<34s} {k:<16s} {v:10.3f}")
    return out


def failures(report, K):
    return [(k, v) for k, v in report.items() if (v != 0 if k == "n_contrib" else not v <= K)]


def statement_outputs(ref, s):
    """(planes, final_T, n_contrib, grads) of a run() result, as grade() takes them."""
    return planes_of(ref["form"], s["out"]), s["final_T"], s["n_contrib"], grads_of(ref["form"], s["acc"])


def flawed(scene, form, flaw, S=None):
    """The `oracle` statement (the `segments` one for the two seam flaws) with one planted flaw, on the reference's mask."""
    ref = reference(scene, form, S=S)
    base = _ref_cache[(scene["name"], form)]
    return ref, run(base["st"], base["pss"], np.float32, clear=base["clear"], flaw=flaw, S=S,
                    statement="segments" if flaw.startswith("seam") else "oracle")
