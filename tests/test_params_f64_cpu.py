"""The float64 reference of the parameter kernels, the smoothness term and Adam, and what keeps the bars built on it honest
(no GPU).

tests/test_params_f64_gpu.py holds the HIP kernels to `K * max(e_ref, 4 ulp * scale)` per class of rows, e_ref being the
fp32 CPU statements' own distance from float64.  Shown here: the closed-form quaternion of the reference IS
calculate_rotation_from_vectors in float64 (value and gradient); fp32 and float64 take the same branch on every row and
select the same smoothness pairs; every class has the property it is listed for; no yardstick can grow silently (caps);
the comparator rejects mutants of the fp32 statements at the ceiling K = 8; and with the fp32 statements standing in for
the kernels every comparator of the GPU file passes.
"""
import types

import numpy as np
import pytest
import torch

from tests import param_cases as PC
from tests import param_reference as R

K_MAX = 8.0
FS = (PC.F_DEFAULT, 1.0)
SIZES = ("all", 1, 255, 256, 257)

# e_ref <= cap * scale per class ("*": every class not named).  Each cap is 4 x the worst value measured on the CPU (fp32
# torch against float64; strand: both f, every upstream; smoothness: both thresholds; cloud: every upstream), rounded up to
# one digit; a class whose fp32 statement gives 0 where float64 is 1e-9 .. 1e-44 (sigmoid at +-100, its derivative at 20)
# has e_ref = scale, cap 1.  Measured values: the table in DESIGN.md section 2.
CAPS = {
    "strand/xyz": {"*": 3e-07},
    "strand/scale": {"*": 5e-07},
    "strand/quat": {"*": 4e-06, "theta_0.03": 2e-05, "theta_0.01": 4e-05, "theta_0.003": 0.0002, "theta_0.001": 0.0004},
    "strand/dir": {"*": 5e-07},
    "strand/opacity": {"*": 4e-07, "act_-100": 1.0},
    "strand/mask": {"*": 4e-07, "act_-100": 1.0},
    "strand/d_endpoints": {"*": 6e-06, "theta_0.03": 1e-05, "theta_0.01": 4e-05, "theta_0.003": 0.0002, "theta_0.001": 0.0003},
    "strand/d_width": {"*": 5e-07},
    "strand/d_opacity_raw": {"*": 2e-06, "act_-100": 1.0, "act_20": 1.0},
    "strand/d_mask_raw": {"*": 9e-07, "act_-100": 1.0, "act_20": 1.0},
    "smooth/d_endpoints": {"*": 6e-06, "bend_3.1_5e-3": 2e-05, "bend_179_5e-3": 0.002, "bend_179.9_5e-3": 0.2, "bend_3.1_mixed": 2e-05, "bend_5_mixed": 1e-05, "bend_179_mixed": 0.002, "bend_179.9_mixed": 0.2},
    "cloud/scale": {"*": 3e-07},
    "cloud/quat": {"*": 5e-07},
    "cloud/opacity": {"*": 4e-07, "act_-100": 1.0},
    "cloud/mask": {"*": 4e-07, "act_-100": 1.0},
    "cloud/dir": {"*": 2e-06},
    "cloud/d_scaling_raw": {"*": 4e-07},
    "cloud/d_rotation_raw": {"*": 2e-06},
    "cloud/d_opacity_raw": {"*": 2e-06, "act_-100": 1.0, "act_20": 1.0},
    "cloud/d_mask_raw": {"*": 3e-06, "act_-100": 1.0, "act_20": 1.0},
}


def _strand_labels(rows):
    return {"xyz": rows.seg_class, "scale": rows.seg_class, "quat": rows.seg_class, "dir": rows.seg_class, "opacity": rows.act_class,
            "mask": rows.act_class, "d_endpoints": rows.ep_class, "d_width": rows.seg_class, "d_opacity_raw": rows.act_class,
            "d_mask_raw": rows.act_class}


def _stand_in(group, x64, x32, labels, keys):
    """The fp32 statements in the kernels' place: every class ratio <= 1 by construction, every yardstick under its cap."""
    for k in keys:
        ratios = R.class_ratios(x32[k], x64[k], x32[k], labels[k])
        assert R.worst(ratios) <= 1.0, (k, ratios)
        caps = CAPS[f"{group}/{k}"]
        for c, (e, _) in ratios.items():
            if c != "*":
                assert e <= caps.get(str(c), caps["*"]), (group, k, c, e)


# ---- the closed form is the reference's statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FS)
def test_closed_form_quaternion_is_calculate_rotation_from_vectors_in_float64(f):
    """Value and gradient to 1e-8 relative on every class with 1 + d.x >= 5e-7 (every row of the rotation branch; measured
    2e-10)."""
    from utils.transform import calculate_rotation_from_vectors
    rows = PC.strand_rows(f, "all")
    r64 = R.strand_run(rows, None, torch.float64)
    rot = r64["rot"]
    assert r64["n0"][rot].min() >= 4.98e-7
    pairs = torch.tensor(rows.pairs[rot])
    g = torch.tensor(PC.strand_upstream(len(rows.pairs))["quat"][rot], dtype=torch.float64)
    res = {}
    for form in ("closed", "reference"):
        ep = torch.tensor(rows.endpoints, dtype=torch.float64, requires_grad=True)
        delta = ep[pairs[:, 1]] - ep[pairs[:, 0]]
        if form == "closed":
            z = torch.zeros(len(pairs), dtype=torch.float64)
            q = R.strand_statements(ep, pairs, z, z, z, float(rows.f))["quat"]
        else:
            xhat = torch.zeros_like(delta)
            xhat[:, 0] = 1.0
            q = calculate_rotation_from_vectors(xhat, delta, representation="quat")
        res[form] = (q.detach().numpy(), torch.autograd.grad((q * g).sum(), ep)[0].numpy())
    assert np.abs(res["closed"][0] - res["reference"][0]).max() <= 1e-8
    for c in dict.fromkeys(rows.ep_class):
        s = rows.ep_class == c
        scale = np.abs(res["reference"][1][s]).max()
        assert np.abs(res["closed"][1][s] - res["reference"][1][s]).max() <= 1e-8 * scale, c


# ---- same branches, same pairs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("f", FS)
def test_fp32_and_float64_take_the_same_strand_branches(f, which):
    rows, _, r64, r32 = R.strand_reference(f, which, None)
    assert np.array_equal(r64["live"], r32["live"]) and np.array_equal(r64["rot"], r32["rot"])
    clamped64, clamped32 = r64["scale"][:, 0] == PC.MINV, r32["scale"][:, 0] == np.float64(np.float32(PC.MINV))
    assert np.array_equal(clamped64, clamped32)
    # never at a threshold: L, 1 + v.x and L / 2 * f stay 20 % away from 1e-7 (exact zeros aside)
    for v in (r64["L"], r64["n0"][r64["live"]], r64["L"] / 2 * rows.f):
        v = v[v > 1e-12]
        assert not ((v > 0.8e-7) & (v < 1.25e-7)).any()


@pytest.mark.parametrize("which", SIZES)
@pytest.mark.parametrize("th", PC.THRESHOLDS)
def test_fp32_and_float64_select_the_same_smoothness_pairs(th, which):
    rows, s64, s32 = R.smooth_reference(which, th)
    assert np.array_equal(s64.sel, s32.sel) and s64.count == s32.count
    assert np.isfinite(s64.d_endpoints).all() and np.isfinite(s32.d_endpoints).all()


@pytest.mark.parametrize("P", PC.CLOUD_P)
def test_fp32_and_float64_pick_the_same_cloud_axis(P):
    rows, _, c64, c32 = R.cloud_reference(P, None)
    assert np.array_equal(c64["axis"], c32["axis"])
    assert np.isfinite(c64["d_rotation_raw"]).all()


# ---- every class has the property it is listed for -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", FS)
def test_strand_classes_have_their_properties(f):
    rows, _, r64, _ = R.strand_reference(f, "all", None)
    cls = lambda c: rows.seg_class == c
    counts = {c: int(cls(c).sum()) for c in dict.fromkeys(rows.seg_class)}
    assert all(n >= PC.ROWS for c, n in counts.items() if c != "star") and counts["star"] == 5
    for th in PC.THETAS:                                  # 1 + d.x in its decade: within 2 % of 1 - cos(theta)
        n0 = r64["n0"][cls(f"theta_{th:g}")]
        assert np.abs(n0 / (1 - np.cos(th)) - 1).max() <= 0.02 and r64["rot"][cls(f"theta_{th:g}")].all()
    assert r64["n0"][cls("theta_0.001")].max() <= 5.1e-7 and r64["n0"][cls("theta_3")].min() >= 1.9
    assert (r64["live"] & ~r64["rot"])[cls("dir_-x")].all() and not (r64["live"] & ~r64["rot"])[~cls("dir_-x")].any()
    for name, ax in PC.AXES.items():
        assert np.array_equal(r64["dir"][cls(name)], np.tile(np.float64(ax), (PC.ROWS, 1)))
    assert not r64["L"][cls("L_0")].any() and (rows.pairs[cls("L_0")][:, 0] == rows.pairs[cls("L_0")][:, 1]).sum() == PC.ROWS // 2
    assert not r64["live"][cls("L_0") | cls("L_half")].any() and r64["live"][~(cls("L_0") | cls("L_half"))].all()
    for name, L in PC.tiny_lengths(f).items():
        assert np.abs(r64["L"][cls(name)] / L - 1).max() <= 0.04, name
    s0 = r64["scale"][:, 0]
    for name in ("L_2x", "sclamp_lo"):                    # alive, scale clamped (its gradient off)
        assert (s0[cls(name)] == PC.MINV).all() and r64["live"][cls(name)].all()
    assert (s0[cls("sclamp_hi")] > 1.8 * PC.MINV).all()
    for L in (1e-5, 1e-2, 1e3):
        assert np.abs(np.log(r64["L"][cls(f"L_{L:g}")] / L)).max() <= 0.25
    assert np.abs(rows.endpoints[rows.ep_class == "offset_100"]).min() >= 99.0
    for name, w in (("w_-20", -20.0), ("w_0", 0.0), ("w_5", 5.0)):
        assert (rows.width[cls(name)] == w).all()
    # topologies: independent endpoints are referenced once, inner chain vertices twice, the star's centre 5 times, 7 never
    deg = np.bincount(rows.pairs.reshape(-1), minlength=len(rows.endpoints))
    assert sorted(deg[rows.ep_class == "star"]) == [1] * 5 + [5]
    assert sorted(set(deg[rows.ep_class == "chain"])) == [1, 2] and (deg[rows.ep_class == "chain"] == 2).sum() == 80
    assert (deg[rows.ep_class == "unreferenced"] == 0).all() and (rows.ep_class == "unreferenced").sum() == 7
    # with the scale's gradient alone: clamped classes have exactly no endpoint gradient in float64, the others have one
    _, _, g64, _ = R.strand_reference(f, "all", "scale")
    for c in dict.fromkeys(rows.ep_class):
        dead = c in ("L_0", "L_half", "L_2x", "sclamp_lo", "unreferenced")
        assert bool(g64["d_endpoints"][rows.ep_class == c].any()) != dead, c
    # ... and the direction's gradient is alive where the scale's is off
    _, _, g64, _ = R.strand_reference(f, "all", "dir")
    for c in ("L_2x", "sclamp_lo", "dir_-x"):
        assert g64["d_endpoints"][rows.ep_class == c].any()


@pytest.mark.parametrize("th", PC.THRESHOLDS)
def test_smoothness_classes_have_their_properties(th):
    rows, s64, _ = R.smooth_reference("all", th)
    deg = 180 / np.pi * np.arccos(np.clip(s64.dot, -1, 1))
    for c in dict.fromkeys(rows.pair_class):
        p, e = rows.pair_class == c, rows.ep_class == c
        assert p.sum() >= PC.ROWS
        bend = PC.bend_of(c)
        if c == "zero_length":
            assert not s64.sel[p].any() and not s64.d_endpoints[e].any() and np.isnan(s64.dot[p]).all()
        elif bend is not None:
            assert np.abs(deg[p] - bend).max() <= (0.05 if bend < 179.5 else 0.01), c
            assert (s64.sel[p] == (bend >= th)).all(), c
            saturated = 1 + np.cos(np.deg2rad(bend)) < PC.SMOOTH_EPS or bend == 0
            assert bool(s64.d_endpoints[e].any()) == (bend >= th and not saturated), c
            if bend == 179.9:
                assert (1 + s64.dot[p]).min() > 1.2e-6 and (1 + s64.dot[p]).max() < 1.9e-6     # alive at eps = 1e-6, off at 2e-6
    roles = np.bincount(rows.pairs.reshape(-1), minlength=len(rows.endpoints))
    assert roles[rows.ep_class == "walk"].max() == 4


def test_cloud_classes_have_their_properties():
    rows, _, c64, _ = R.cloud_reference(1000, None)
    cls = lambda c: rows.row_class == c
    assert all(cls(c).sum() >= PC.ROWS for c in dict.fromkeys(rows.row_class)) and len(rows.row_class) == 1000
    n = np.linalg.norm(rows.rotation_raw.astype(np.float64), axis=1)
    assert n.min() > 0
    for name, v in (("qnorm_1e-3", 1e-3), ("qnorm_1", 1.0), ("qnorm_1e3", 1e3)):
        assert np.abs(n[cls(name)] / v - 1).max() <= 1e-6
    q = np.abs(rows.rotation_raw[cls("q_dominant")])
    assert (np.sort(q, axis=1)[:, -1] == 1).all() and np.sort(q, axis=1)[:, -2].max() < 1e-3
    assert not rows.rotation_raw[cls("q_w0"), 0].any()
    s = rows.scaling_raw
    for name, tied, first in (("tie_01", (0, 1), 0), ("tie_02", (0, 2), 0), ("tie_12", (1, 2), 1), ("tie_012", (0, 1, 2), 0)):
        r = s[cls(name)]
        assert (r[:, list(tied)] == r[:, [tied[0]]]).all() and (r.max(axis=1) == r[:, tied[0]]).all()
        assert (c64["axis"][cls(name)] == first).all()
    assert s[cls("scale_range")].min() < -14 and s[cls("scale_range")].max() > 2
    for v in (-100.0, -20.0, 0.0, 20.0, 100.0):
        assert (rows.opacity_raw[cls(f"act_{v:g}")] == v).all() and (rows.mask_raw[cls(f"act_{v:g}")] == v).all()


def test_adam_problems_cover_the_listed_paths():
    small, big, late = (PC.adam_problem(k, 10) for k in ("small", "big", "late"))
    assert tuple(t.n for t in small.tensors) == PC.ADAM_SIZES and all(len(c) <= 8 for c in small.calls)
    assert len(big.calls) == 1 and len(big.calls[0]) == 8 and sum(t.n for t in big.tensors) > 6 * 2 ** 20
    assert [t.step0 for t in late.tensors] == [0] + [100] * 7
    assert {t.stream for t in small.tensors} == set(PC.ADAM_STREAMS) and {t.lr0 for t in small.tensors} == set(PC.ADAM_LRS)
    assert sum(t.change_at is not None for t in small.tensors) == 1
    g = PC.adam_gradient("sparse", 4096, 3, 1)
    assert 0.85 <= (g == 0).mean() <= 0.95
    assert abs(R.V_CONTRACT + 1.287e-5) < 1e-8


# ---- the fp32 statements in the kernels' place; caps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("only", (None,) + PC.STRAND_OUTPUTS, ids=lambda o: o or "together")
@pytest.mark.parametrize("f", FS)
def test_fp32_strand_statements_pass_every_comparator(f, only):
    for which in (SIZES if only is None else ("all", "chains")):
        rows, _, r64, r32 = R.strand_reference(f, which, only)
        _stand_in("strand", r64, r32, _strand_labels(rows), list(_strand_labels(rows)))


@pytest.mark.parametrize("th", PC.THRESHOLDS)
def test_fp32_smoothness_statements_pass_every_comparator(th):
    for which in SIZES:
        rows, s64, s32 = R.smooth_reference(which, th)
        _stand_in("smooth", {"d_endpoints": s64.d_endpoints}, {"d_endpoints": s32.d_endpoints}, {"d_endpoints": rows.ep_class}, ["d_endpoints"])
        assert abs(s32.value - s64.value) <= 2e-5 * max(s64.value, 1e-30)        # 4 x the worst measured, 4.3e-6 (N = 255: a fifth of the pairs at 179.9 degrees)


@pytest.mark.parametrize("only", (None,) + PC.CLOUD_OUTPUTS, ids=lambda o: o or "together")
def test_fp32_cloud_statements_pass_every_comparator(only):
    for P in (PC.CLOUD_P if only is None else (1000,)):
        rows, _, c64, c32 = R.cloud_reference(P, only)
        keys = [k for k in c64 if k != "axis"]
        _stand_in("cloud", c64, c32, {k: rows.row_class for k in keys}, keys)


def _adam_worst(got, ref, against="abi", arrays="pmv"):
    want, worst = getattr(ref, against), 0.0
    for k in range(len(got)):
        for j, name in enumerate("pmv"):
            if name in arrays:
                e_ref, scale = np.abs(ref.t32[k][j] - ref.dec[k][j]).max(), np.abs(want[k][j]).max()
                d, bar = np.abs(got[k][j] - want[k][j]).max(), max(e_ref, R.ULP4 * scale)
                worst = max(worst, d / bar if bar > 0 else (0.0 if d == 0 else float("inf")))
    return worst


@pytest.mark.parametrize("kind,T", [("small", 1), ("small", 10), ("late", 10)])
def test_adam_contract_on_the_cpu(kind, T):
    """fp32 torch is within its own yardstick by construction; an fp32 emulation of hgs_adam_coef / hgs_adam_one (float betas)
    passes against float64 Adam with the betas as the C ABI receives them, and on p against the decimal betas; its
    exp_avg_sq is off the decimal-beta one by (1 - fl(0.999)) / 0.001 - 1, which is 27 yardsticks: the contract the GPU file
    states."""
    ref = R.adam_reference(kind, T)
    assert _adam_worst(ref.t32, ref, "dec") <= 1.0
    em = R.adam_kernel_emulation(ref.prob)
    assert _adam_worst(em, ref, "abi") <= 2.0 and _adam_worst(em, ref, "dec", "p") <= 2.0      # measured 0.6 and 1.1
    if kind == "small":
        for k in range(len(em)):                     # (elements above 1e-30: below, fp32 has no 1e-6)
            big = ref.dec[k][2] > 1e-30
            assert not big.any() or np.abs(em[k][2][big] / ref.dec[k][2][big] - 1 - R.V_CONTRACT).max() <= 1e-6
        assert _adam_worst(em, ref, "dec", "v") > K_MAX


# ---- the comparator rejects mutants of the fp32 statements at K = 8 -----------------------------------------------------------------------
@pytest.mark.parametrize("mutant,only,key,label", [("no_projection", "dir", "d_endpoints", "ep_class"), ("q2_sign", None, "quat", "seg_class"),
                                                   ("q2_sign", "quat", "d_endpoints", "ep_class"), ("scale_f", None, "scale", "seg_class"),
                                                   ("scale_f", "scale", "d_endpoints", "ep_class")])
def test_comparator_rejects_strand_mutants(mutant, only, key, label):
    rows, up, r64, r32 = R.strand_reference(PC.F_DEFAULT, "all", only)
    bad = R.strand_run(rows, up, torch.float32, mutant=mutant)
    assert R.accepts(r32[key], r64[key], r32[key], getattr(rows, label), K_MAX)
    assert not R.accepts(bad[key], r64[key], r32[key], getattr(rows, label), K_MAX)


def test_comparator_rejects_a_wrong_scale_factor_and_a_doubled_eps():
    rows, up, r64, r32 = R.strand_reference(PC.F_DEFAULT, "all", "scale")
    bad = R.strand_run(rows, up, torch.float32, f=float(np.float32(rows.f * (1 + 1e-4))))
    assert not R.accepts(bad["scale"], r64["scale"], r32["scale"], rows.seg_class, K_MAX)
    assert not R.accepts(bad["d_endpoints"], r64["d_endpoints"], r32["d_endpoints"], rows.ep_class, K_MAX)
    for th in PC.THRESHOLDS:
        rows, s64, s32 = R.smooth_reference("all", th)
        bad = R.smooth_run(rows, th, 2 * PC.SMOOTH_EPS, torch.float32)
        ratios = R.class_ratios(bad.d_endpoints, s64.d_endpoints, s32.d_endpoints, rows.ep_class)
        assert ratios["bend_179.9_5e-3"][1] > K_MAX and ratios["bend_179.9_mixed"][1] > K_MAX
        assert max(r for c, (_, r) in ratios.items() if not str(c).startswith("bend_179.9") and c != "*") <= 1.0


@pytest.mark.parametrize("kw", [{"beta1": float(np.float32(PC.BETA1 * (1 + 1e-4)))}, {"lr_factor": 1 + 1e-4}], ids=["beta1", "lr"])
def test_comparator_rejects_adam_mutants(kw):
    ref = R.adam_reference("small", 10)
    assert _adam_worst(R.adam_kernel_emulation(ref.prob, **kw), ref, "abi") > K_MAX
    late = R.adam_reference("late", 10)          # every tensor taking the bias corrections of step 100: rejected too
    wrong = PC.adam_problem("late", 10)
    shifted = [types.SimpleNamespace(**{**vars(t), "step0": 100}) for t in wrong.tensors]
    em = R.adam_kernel_emulation(types.SimpleNamespace(tensors=shifted, T=10))
    assert _adam_worst(em, late, "abi") > K_MAX
