"""The comparator of the per-Gaussian backward (preprocess_bwd_kernel) against float64, row by row.

The chain is isolated from the blend: both builds of the oracle's hgs_oracle_preprocess_backward (oracle/raster_oracle.c) are
called on an UPSTREAM that is given -- the dL_dmeans2D, dL_dconic and dL_dcolors the kernel summed and then used (float32,
hence exact in float64), or, without a GPU, the fp32 oracle's own -- with the given `radii` and `clamped` and with `cov3D` from
their own forward.  Their dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales and dL_drotations are the two statements x32 and x64.

Per row i and tensor:  s_i = max|x64_i|;  the yardstick E_i = max |x32_i - x64_i| over the base inputs and J copies of them with
means3D, scales and rotations moved by -1, 0 or +1 ulp (zeros left alone; both statements at the SAME inputs);  the bar is
    max|x_i - x64_i| <= K * max(E_i, 4 * 2^-23 * s_i),
exactly 0 wherever x64 is exactly 0, NaN / Inf never.  CAP is the condition that keeps the bar from being vacuous:
E_i <= 1e-2 * s_i on every graded row.
"""
import ctypes as C

import numpy as np

from oracle import hgs_oracle as O

UPSTREAM = ("dL_dmeans2D", "dL_dconic", "dL_dcolors")
TENSORS = ("dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
FLOOR = 4.0 * 2.0 ** -23
CAP = 1e-2
J = 16


def cov3d(scene, f64):
    """cov3D of the statement's own forward (computeCov3D at this precision), or the precomputed one.  It depends on scales,
    rotations and the modifier only, so the forward is run with every mean at the world point the camera looks at: a row the
    forward would cull at its own mean (near_cut, or a jittered copy of its neighbour) still has its covariance."""
    dt = np.float64 if f64 else np.float32
    P = scene["means3D"].shape[0]
    if scene["cov3D_precomp"] is not None:
        return np.ascontiguousarray(scene["cov3D_precomp"], dtype=dt).reshape(P, 6)
    s = dict(scene)
    V = np.asarray(scene["viewmatrix"], np.float64)
    s["means3D"] = np.tile(np.linalg.inv(V)[3, :3] + 1.2 * V[:3, 2], (P, 1)).astype(np.float32)
    f = O.forward(s, f64=f64, render=False)
    assert P == 0 or (f["cov3D"] != 0).any(axis=1).all()
    return f["cov3D"]


def grad_mul(scene, f64):
    """(x_grad_mul != 0, y_grad_mul != 0) per row as the statement of this precision decides them (CR/backward_distwar.cu:
    186-190): transformPoint4x3 and the two divisions in the oracle's operation order."""
    dt = np.float64 if f64 else np.float32
    m, V = np.asarray(scene["means3D"]).astype(dt), np.asarray(scene["viewmatrix"]).astype(dt).reshape(16)
    t = [V[k] * m[:, 0] + V[4 + k] * m[:, 1] + V[8 + k] * m[:, 2] + V[12 + k] for k in range(3)]
    limx, limy = dt(1.3) * dt(scene["tanfovx"]), dt(1.3) * dt(scene["tanfovy"])
    with np.errstate(divide="ignore", invalid="ignore"):
        txtz, tytz = t[0] / t[2], t[1] / t[2]
    assert txtz.dtype == dt
    return ~((txtz < -limx) | (txtz > limx)), ~((tytz < -limy) | (tytz > limy))


def _means_f64(scene, edge_rows):
    """means3D in float64.  On `edge_rows` (clamp_edge: fp32 t.x / t.z within ulps of the clamp) the float64 statement is
    graded against the fp32 statement's DECISION: where the two precisions decide x_grad_mul differently, the row's x is moved
    (by at most those few float32 ulps) to 1.3 tan_fovx t.z (1 -+ 1e-12), the side fp32 took.  Everything but the decision is
    continuous in x, and the move is inside the yardstick: x32 is compared with x64 at exactly these means."""
    m = np.asarray(scene["means3D"]).astype(np.float64)
    if edge_rows is None or len(edge_rows) == 0:
        return m
    in32, _ = grad_mul(scene, False)
    in64, _ = grad_mul(scene, True)
    rows = np.asarray(edge_rows)[in32[edge_rows] != in64[edge_rows]]
    if len(rows):
        V = np.asarray(scene["viewmatrix"], np.float64).reshape(16)
        assert V[0] == 1.0 and V[4] == 0.0 and V[8] == 0.0 and V[2] == 0.0 and V[6] == 0.0   # (axis-aligned: view x = world x + V[12])
        tz = V[10] * m[rows, 2] + V[14]
        lim = 1.3 * float(scene["tanfovx"])
        m[rows, 0] = np.sign(m[rows, 0] + V[12]) * lim * tz * np.where(in32[rows], 1.0 - 1e-12, 1.0 + 1e-12) - V[12]
        moved = dict(scene, means3D=m)
        assert np.array_equal(grad_mul(moved, True)[0][rows], in32[rows])
    return m


def chain(scene, upstream, radii, clamped, f64, edge_rows=None, cov=None):
    """The oracle's preprocess backward at one precision on a given upstream: {tensor: array} for TENSORS (dL_dmeans3D is the
    sum of the cov2D, projection and SH parts, as the kernel returns it)."""
    dt, cr, sfx = O._real(f64)
    n = O.normalize_inputs(scene, f64)
    if f64:
        n["means3D"] = np.ascontiguousarray(_means_f64(scene, edge_rows))
    P, M = n["P"], n["M"]
    cov = cov3d(scene, f64) if cov is None else cov
    up = {k: np.ascontiguousarray(np.asarray(upstream[k]).reshape(P, -1), dtype=dt) for k in UPSTREAM}
    assert up["dL_dmeans2D"].shape[1] == 3 and up["dL_dconic"].shape[1] == 4 and up["dL_dcolors"].shape[1] == 3
    g = {"dL_dmeans3D": np.zeros((P, 3), dt), "dL_dcov3D": np.zeros((P, 6), dt), "dL_dsh": np.zeros((P, M, 3), dt),
         "dL_dscales": np.zeros((P, 3), dt), "dL_drotations": np.zeros((P, 4), dt)}
    if P:
        p = O._p
        getattr(O.lib(), "hgs_oracle_preprocess_backward" + sfx)(
            C.c_int(P), C.c_int(n["sh_degree"]), C.c_int(M), C.c_int(int(scene["W"])), C.c_int(int(scene["H"])), p(n["means3D"]),
            p(np.ascontiguousarray(radii, dtype=np.int32)), p(n["shs"]), p(np.ascontiguousarray(clamped, dtype=np.uint8)),
            p(n["scales"]), p(n["rotations"]), cr(n["scale_modifier"]), p(np.ascontiguousarray(cov, dtype=dt)), p(n["viewmatrix"]),
            p(n["projmatrix"]), cr(n["tanfovx"]), cr(n["tanfovy"]), p(n["campos"]), p(up["dL_dmeans2D"]), p(up["dL_dconic"]),
            p(g["dL_dmeans3D"]), p(up["dL_dcolors"]), p(g["dL_dcov3D"]), p(g["dL_dsh"]), p(g["dL_dscales"]), p(g["dL_drotations"]))
    return g


def jitter(scene, rng):
    """A copy of the scene with every element of means3D, scales and rotations moved by -1, 0 or +1 float32 ulp (zeros left alone)."""
    s = dict(scene)
    for k in ("means3D", "scales", "rotations"):
        a = scene.get(k)
        if a is None:
            continue
        a = np.asarray(a, np.float32)
        step = rng.integers(-1, 2, a.shape)
        up, down = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))
        s[k] = np.where(a == 0, a, np.where(step > 0, up, np.where(step < 0, down, a))).astype(np.float32)
    return s


def _rows(a):
    return np.asarray(a, np.float64).reshape(a.shape[0], -1)


def yardstick(scene, upstream, radii, clamped, edge_rows=None, copies=J, seed=0):
    """(x64 at the base inputs {tensor: float64 array}, E {tensor: [P]}, s {tensor: [P]})."""
    rng = np.random.default_rng(seed)
    x64 = chain(scene, upstream, radii, clamped, True, edge_rows)
    P = scene["means3D"].shape[0]
    E = {k: np.zeros(P) for k in TENSORS}
    for j in range(copies + 1):
        sj = scene if j == 0 else jitter(scene, rng)
        a = chain(sj, upstream, radii, clamped, False)
        b = x64 if j == 0 else chain(sj, upstream, radii, clamped, True, edge_rows)
        for k in TENSORS:
            if a[k].size:
                E[k] = np.maximum(E[k], np.abs(_rows(a[k]) - _rows(b[k])).max(axis=1))
    s = {k: (np.abs(_rows(x64[k])).max(axis=1) if x64[k].size else np.zeros(P)) for k in TENSORS}
    return x64, E, s


def ratios(x, x64, E, s):
    """{tensor: (ratio [P], ok_zero [P], finite [P])}: the row's error in units of its bar at K = 1 (0 where the row has no
    float64 gradient at all), whether it is exactly 0 wherever x64 is, and whether it is finite."""
    out = {}
    for k in TENSORS:
        b = _rows(x64[k])
        a = np.asarray(x[k], np.float64).reshape(b.shape)
        P = b.shape[0]
        if b.size == 0:
            out[k] = (np.zeros(P), np.ones(P, bool), np.ones(P, bool))
            continue
        finite = np.isfinite(a).all(axis=1)
        ok_zero = ((b != 0) | (a == 0)).all(axis=1)
        err = np.abs(np.where(np.isfinite(a), a, 0.0) - b).max(axis=1)
        bar = np.maximum(E[k], FLOOR * s[k])
        out[k] = (np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), 0.0), ok_zero, finite)
    return out


def failures(x, x64, E, s, K, classes):
    """[(class, tensor, worst ratio, rows outside the bar, rows not exactly 0 where float64 is, rows with NaN / Inf)] for
    every class and tensor that misses the bar; [] when the comparator passes."""
    bad = []
    r = ratios(x, x64, E, s)
    for c, idx in classes.items():
        if len(idx) == 0:
            continue
        for k in TENSORS:
            ratio, ok_zero, finite = (v[idx] for v in r[k])
            if (ratio > K).any() or not ok_zero.all() or not finite.all():
                bad.append((c, k, float(ratio.max()), int((ratio > K).sum()), int((~ok_zero).sum()), int((~finite).sum())))
    return bad


def table(x, x64, E, s, classes, label):
    """One printed row per class and tensor: worst E_i / s_i and worst ratio (the figures DESIGN.md section 2 records).
    Returns (worst E_i / s_i, worst ratio) over everything."""
    r = ratios(x, x64, E, s)
    worst_e, worst_r = 0.0, 0.0
    for c, idx in classes.items():
        if len(idx) == 0:
            continue
        cells = []
        for k in TENSORS:
            if x64[k].size == 0:
                continue
            live = s[k][idx] > 0
            e = float((E[k][idx][live] / s[k][idx][live]).max()) if live.any() else 0.0
            q = float(r[k][0][idx].max())
            worst_e, worst_r = max(worst_e, e), max(worst_r, q)
            cells.append(f"{k[3:]} {e:.1e} {q:.2f}")
        print(f"F64ROW {label} {c:13s} (E/s, ratio) " + " | ".join(cells))
    print(f"F64ROW {label} worst E/s {worst_e:.2e} worst ratio {worst_r:.3f}")
    return worst_e, worst_r


def cap_violations(E, s, classes):
    """[(class, tensor, worst E_i / s_i)] of the classes that break the cap E_i <= CAP * s_i on a row with a gradient."""
    out = []
    for c, idx in classes.items():
        for k in TENSORS:
            live = s[k][idx] > 0
            if live.any():
                e = float((E[k][idx][live] / s[k][idx][live]).max())
                if e > CAP:
                    out.append((c, k, e))
    return out
