"""Float64 statements of the parameter kernels, the smoothness term and Adam; the yardsticks and the comparator built on them
(tests/test_params_f64_cpu.py, tests/test_params_f64_gpu.py).

Every function takes a torch dtype: float64 is the reference, float32 (CPU) the yardstick -- the same statements at the
kernels' precision, `e_ref = max|x32 - x64|` per class.  The strand quaternion is the closed form of the header comment of
csrc/hgs_strands.hip, normalize(1 + d.x, 0, -d.z, d.y); tests/test_params_f64_cpu.py ties it to
utils.transform.calculate_rotation_from_vectors in float64, so no arithmetic is trusted that the reference does not state.
The fp32 yardstick of the quaternion is the fp32 CLOSED FORM, not the fp32 getters: R = I + K + K^2 / (1 + c) cancels near
d = -x_hat, which is a property of that formula in fp32, not of the rotation.
"""
import functools
import types

import numpy as np
import torch
import torch.nn.functional as F

from tests import param_cases as PC

ULP4 = 4.0 * 2.0 ** -23            # four fp32 ulps of the class's scale: the floor under the reference's own error
MINV = PC.MINV


def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(grad)


# ---- strand geometry ------------------------------------------------------------------------------------------------------------------------
def strand_statements(ep, pairs, width, o_raw, m_raw, f, mutant=None):
    """mean, scale, quaternion, direction, sigmoid(opacity), sigmoid(mask) of every segment, in the dtype of `ep`; branches are
    decided on this dtype's own L and 1 + v.x (csrc/hgs_strands.hip header).  -> dict of outputs + `live`, `rot` (bool)."""
    e0, e1 = ep[pairs[:, 0]], ep[pairs[:, 1]]
    delta = e1 - e0
    Lsq = (delta * delta).sum(dim=1, keepdim=True)
    L = torch.where(Lsq > 0, torch.sqrt(torch.where(Lsq > 0, Lsq, torch.ones_like(Lsq))), torch.zeros_like(Lsq))
    live = L > MINV
    half_f = f if mutant == "scale_f" else f / 2
    s0 = torch.clamp(L * half_f, min=MINV)
    sw = torch.exp(width).reshape(-1, 1)
    v = delta / torch.where(live, L, torch.ones_like(L))
    if mutant == "no_projection":       # the direction as if |delta| were a constant: (I - v v^T) dropped from its gradient
        v = delta / torch.where(live, L, torch.ones_like(L)).detach()
    xhat = torch.zeros_like(v)
    xhat[:, 0] = 1.0
    d = torch.where(live, v, xhat)
    n0 = 1 + v[:, :1]
    rot = live & (n0 > MINV)
    q2 = v[:, 2:3] if mutant == "q2_sign" else -v[:, 2:3]
    qr = torch.cat([n0, torch.zeros_like(n0), q2, v[:, 1:2]], dim=1)
    qsq = (qr * qr).sum(dim=1, keepdim=True)
    qc = qr / torch.sqrt(torch.where(rot, qsq, torch.ones_like(qsq)))
    ident, halfturn = torch.zeros_like(qc), torch.zeros_like(qc)
    ident[:, 0] = 1.0
    halfturn[:, 3] = 1.0
    quat = torch.where(rot, qc, torch.where(live, halfturn, ident))
    return {"xyz": (e0 + e1) / 2, "scale": torch.cat([s0, sw, sw], dim=1), "quat": quat, "dir": d,
            "opacity": torch.sigmoid(o_raw).reshape(-1, 1), "mask": torch.sigmoid(m_raw).reshape(-1, 1),
            "live": live.reshape(-1), "rot": rot.reshape(-1), "L": L.detach().reshape(-1), "n0": n0.detach().reshape(-1)}


def strand_run(rows, upstream, dtype, f=None, mutant=None):
    """Outputs and the gradients of sum(output * upstream) w.r.t. endpoints, width, raw opacity, raw mask (numpy float64)."""
    ep, w = _t(rows.endpoints, dtype, True), _t(rows.width, dtype, True)
    o, m = _t(rows.opacity_raw, dtype, True), _t(rows.mask_raw, dtype, True)
    f = rows.f if f is None else f
    out = strand_statements(ep, torch.tensor(rows.pairs), w, o, m, float(f), mutant)
    res = {k: out[k].detach().double().numpy() for k in PC.STRAND_OUTPUTS}
    res.update(live=out["live"].numpy(), rot=out["rot"].numpy(), L=out["L"].double().numpy(), n0=out["n0"].double().numpy())
    if upstream is not None:
        loss = sum((out[k] * _t(upstream[k], dtype)).sum() for k in PC.STRAND_OUTPUTS)
        gs = torch.autograd.grad(loss, (ep, w, o, m), allow_unused=True)
        for name, g, like in zip(("d_endpoints", "d_width", "d_opacity_raw", "d_mask_raw"), gs, (ep, w, o, m)):
            res[name] = (torch.zeros_like(like) if g is None else g).double().numpy()
    return res


@functools.lru_cache(maxsize=None)
def strand_reference(f, which, only):
    """-> (rows, upstream, r64, r32) for PC.strand_rows(f, which) and PC.strand_upstream(P, only); shared, never modified."""
    rows = PC.strand_rows(f, which)
    up = PC.strand_upstream(len(rows.pairs), only)
    return rows, up, strand_run(rows, up, torch.float64), strand_run(rows, up, torch.float32)


# ---- smoothness -----------------------------------------------------------------------------------------------------------------------------
def smooth_run(rows, threshold_deg, eps, dtype):
    """loss.losses.angle_smoothness_loss's statements (the torch.where form) on `dtype` tensors.  Pairs with a zero-length
    segment are left out of the graph: the reference never selects them (0 / 0 direction, NaN <= cos is false) and the fused
    kernel skips them; inside the graph they would turn every gradient into NaN.
    -> namespace(value, count, sel [N] bool, d_endpoints [E,3])."""
    ep = _t(rows.endpoints, dtype, True)
    idx = torch.tensor(rows.pairs).reshape(-1, 2, 2)
    cos_th = float(np.cos(threshold_deg * np.pi / 180))
    pos = ep[idx]
    d = pos[:, :, 1] - pos[:, :, 0]
    ok = (d.detach().abs().sum(dim=2) > 0).all(dim=1)
    d = d[ok]
    d = d / torch.norm(d, dim=2, keepdim=True)
    dot = torch.sum(d[:, 0] * d[:, 1], dim=1)
    sel_ok = dot <= cos_th
    ang2 = torch.acos(torch.clamp(dot, -1 + eps, 1 - eps)) ** 2
    value = torch.where(sel_ok, ang2, torch.zeros_like(ang2)).sum() / sel_ok.sum().clamp(min=1)
    g = torch.autograd.grad(value, ep)[0] if bool(sel_ok.any()) else torch.zeros_like(ep)
    sel = torch.zeros(len(rows.pairs), dtype=torch.bool)
    sel[ok] = sel_ok
    dots = torch.full((len(rows.pairs),), float("nan"), dtype=torch.float64)
    dots[ok] = dot.detach().double()
    return types.SimpleNamespace(value=float(value.detach()), count=int(sel_ok.sum()), sel=sel.numpy(), dot=dots.numpy(),
                                 d_endpoints=g.double().numpy())


@functools.lru_cache(maxsize=None)
def smooth_reference(which, threshold_deg, eps=PC.SMOOTH_EPS):
    rows = PC.smooth_rows(which)
    return rows, smooth_run(rows, threshold_deg, eps, torch.float64), smooth_run(rows, threshold_deg, eps, torch.float32)


# ---- Stage-I cloud --------------------------------------------------------------------------------------------------------------------------
def cloud_run(rows, upstream, dtype):
    """exp, F.normalize, sigmoid and the build_rotation column of the first largest scale (scene/gaussian_model.py)."""
    from utils.transform import build_rotation
    s, r = _t(rows.scaling_raw, dtype, True), _t(rows.rotation_raw, dtype, True)
    o, m = _t(rows.opacity_raw, dtype, True), _t(rows.mask_raw, dtype, True)
    scale = torch.exp(s)
    axis = torch.argmax(scale, dim=1)
    onehot = torch.zeros_like(scale)
    onehot.scatter_(1, axis[:, None], 1.0)
    out = {"scale": scale, "quat": F.normalize(r), "opacity": torch.sigmoid(o).reshape(-1, 1), "mask": torch.sigmoid(m).reshape(-1, 1),
           "dir": torch.bmm(build_rotation(r), onehot.unsqueeze(2)).squeeze(-1)}
    res = {k: out[k].detach().double().numpy() for k in PC.CLOUD_OUTPUTS}
    res["axis"] = axis.numpy()
    if upstream is not None:
        loss = sum((out[k] * _t(upstream[k], dtype)).sum() for k in PC.CLOUD_OUTPUTS)
        gs = torch.autograd.grad(loss, (s, r, o, m))
        for name, g in zip(("d_scaling_raw", "d_rotation_raw", "d_opacity_raw", "d_mask_raw"), gs):
            res[name] = g.double().numpy()
    return res


@functools.lru_cache(maxsize=None)
def cloud_reference(P, only):
    rows = PC.cloud_rows(P)
    up = PC.cloud_upstream(P, only)
    return rows, up, cloud_run(rows, up, torch.float64), cloud_run(rows, up, torch.float32)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
def adam_f64(prob, beta1, beta2, eps, lr_factor=1.0):
    """float64 Adam with torch's update rule (m as a lerp; p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)) on the
    fp32 inputs widened.  betas / eps as given: np.float32 values for the C ABI's contract, decimal ones for torch's.
    -> list of (p, m, v) float64, in the order of prob.tensors."""
    b1, b2, eps = float(beta1), float(beta2), float(eps)
    out = []
    for t in prob.tensors:
        p, m, v = (np.asarray(a, dtype=np.float64).copy() for a in (t.p0, t.m0, t.v0))
        for k in range(1, prob.T + 1):
            g = PC.adam_gradient(t.stream, t.n, k, t.seed).astype(np.float64)
            step = t.step0 + k
            lr = float(np.float32(PC.adam_lr(t, k))) * lr_factor
            m += (g - m) * (1 - b1)
            v *= b2
            v += (1 - b2) * g * g
            p -= lr / (1 - b1 ** step) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps))
        out.append((p, m, v))
    return out


def adam_torch32(prob):
    """The yardstick: torch.optim.Adam(foreach=False), fp32, CPU, decimal betas."""
    out = []
    for t in prob.tensors:
        p = torch.tensor(t.p0).requires_grad_(True)
        opt = torch.optim.Adam([p], lr=PC.adam_lr(t, 1), betas=(PC.BETA1, PC.BETA2), eps=PC.ADAM_EPS, foreach=False)
        if t.step0:
            opt.state[p] = {"step": torch.tensor(float(t.step0)), "exp_avg": torch.tensor(t.m0), "exp_avg_sq": torch.tensor(t.v0)}
        for k in range(1, prob.T + 1):
            p.grad = torch.tensor(PC.adam_gradient(t.stream, t.n, k, t.seed))
            opt.param_groups[0]["lr"] = PC.adam_lr(t, k)
            opt.step()
        st = opt.state[p]
        out.append(tuple(a.detach().double().numpy() for a in (p, st["exp_avg"], st["exp_avg_sq"])))
    return out


def adam_kernel_emulation(prob, beta1=PC.BETA1, beta2=PC.BETA2, eps=PC.ADAM_EPS, lr_factor=1.0):
    """hgs_adam_coef / hgs_adam_one operation by operation in numpy fp32 (the C ABI's float betas): what stands in for the
    kernel on a machine without a GPU."""
    f = np.float32
    b1, b2, eps = f(beta1), f(beta2), f(eps)
    out = []
    for t in prob.tensors:
        p, m, v = t.p0.copy(), t.m0.copy(), t.v0.copy()
        for k in range(1, prob.T + 1):
            g = PC.adam_gradient(t.stream, t.n, k, t.seed)
            step = f(t.step0 + k)
            lr = f(f(PC.adam_lr(t, k)) * f(lr_factor))
            bc1, bc2 = f(1) - f(np.power(b1, step, dtype=f)), f(1) - f(np.power(b2, step, dtype=f))
            step_size, inv = f(lr / bc1), f(f(1) / np.sqrt(bc2, dtype=f))
            m = m + (g - m) * (f(1) - b1)
            v = b2 * v + (f(1) - b2) * g * g
            p = p - step_size * (m / (np.sqrt(v) * inv + eps))
        out.append(tuple(a.astype(np.float64) for a in (p, m, v)))
    return out


@functools.lru_cache(maxsize=None)
def adam_reference(kind, T):
    """-> namespace(prob, abi: float64 Adam with the betas as the C ABI receives them, dec: with the decimal betas,
    t32: fp32 torch).  Yardstick of tensor k, array j: max|t32 - dec| -- torch's own distance from ITS float64 statement."""
    prob = PC.adam_problem(kind, T)
    f = np.float32
    return types.SimpleNamespace(prob=prob, abi=adam_f64(prob, f(PC.BETA1), f(PC.BETA2), f(PC.ADAM_EPS)),
                                 dec=adam_f64(prob, PC.BETA1, PC.BETA2, PC.ADAM_EPS), t32=adam_torch32(prob))


# the contract of exp_avg_sq: g^2 is weighted with 1 - fl(0.999), torch weights it with 0.001
V_CONTRACT = (1.0 - float(np.float32(PC.BETA2))) / (1.0 - PC.BETA2) - 1.0


# ---- the comparator ---------------------------------------------------------------------------------------------------------------------------
def class_ratios(x, x64, x32, labels):
    """Per class of `labels` (one per row of the arrays) and under "*" globally:
    name -> (e_ref / scale, max|x - x64| / max(e_ref, 4 ulp scale)).  Where a class's float64 values are all exactly 0 (clamped
    branch, saturated clamp, unreferenced endpoint, unselected pair) `x` must be exactly 0 there: ratio 0, else inf.
    A NaN / Inf in `x` gives inf."""
    x, x64, x32 = (np.asarray(a, dtype=np.float64).reshape(len(labels), -1) for a in (x, x64, x32))
    assert np.isfinite(x64).all() and np.isfinite(x32).all(), "the reference itself is not finite"
    out = {}
    groups = [("*", np.ones(len(labels), dtype=bool))] + [(c, labels == c) for c in dict.fromkeys(labels)]
    for name, sel in groups:
        a, b, c = x[sel], x64[sel], x32[sel]
        scale = float(np.abs(b).max()) if b.size else 0.0
        if not np.isfinite(a).all():
            out[name] = (0.0, float("inf"))
        elif scale == 0.0:
            out[name] = (0.0, float("inf") if a.any() else 0.0)
        else:
            e_ref = float(np.abs(c - b).max())
            out[name] = (e_ref / scale, float(np.abs(a - b).max()) / max(e_ref, ULP4 * scale))
    return out


def worst(ratios):
    return max(r for _, r in ratios.values())


def accepts(x, x64, x32, labels, K):
    return worst(class_ratios(x, x64, x32, labels)) <= K


def table(title, ratios):
    """One row per class for `pytest -s`: class, e_ref / scale, ratio."""
    for name, (e, r) in ratios.items():
        print(f"ratio | {title} | {name} | {e:.1e} | {r:.2f} |")
