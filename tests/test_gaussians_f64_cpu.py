"""No GPU: what tests/gaussian_cases.py promises of its classes, the conditions under which tests/gaussian_reference.py's
row-by-row bar means something (every row graded, the yardstick capped at 1e-2 of the row's own gradient), and that the
comparator passes the fp32 statement and REJECTS it when one argument is subtly wrong.  Upstream here: the fp32 oracle's own
blend backward on the smooth dL_dpix, zeroed on the near-threshold pixels (tests/test_gaussians_f64_gpu.py feeds the kernel's)."""
import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import gaussian_cases as GC
from tests import gaussian_reference as GR

K = 8   # the ceiling of DESIGN.md section 2's rule; the GPU file holds the measured constant
VARIANTS = {"sh0": dict(form="sh0"), "sh3": dict(form="sh3"), "colors_precomp": dict(form="colors_precomp"),
            "cov3D_precomp": dict(form="cov3D_precomp"), "scale_modifier": dict(form="sh3", scale_modifier=0.6),
            "far_origin": dict(form="sh3", far_origin=True)}
MASK_MAX_SHARE_OF_BLENDED = 0.05
_STATE = {}


def _state(variant):
    if variant not in _STATE:
        s = GC.hard_scene(**VARIANTS[variant])
        f32, f64 = O.forward(s), O.forward(s, f64=True)
        mask = O.fragile_pixels(s, f32)
        g = O.backward(s, f32, GC.smooth_dpix() * ~mask)
        up = {k: g[k] for k in GR.UPSTREAM}
        assert all(up[k].dtype == np.float32 for k in up)
        edge = s["classes"].get("clamp_edge")
        x64, E, sc = GR.yardstick(s, up, f32["radii"], f32["clamped"], edge)
        x32 = GR.chain(s, up, f32["radii"], f32["clamped"], False)
        _STATE[variant] = dict(s=s, f32=f32, f64=f64, mask=mask, g=g, up=up, edge=edge, x64=x64, E=E, sc=sc, x32=x32)
    return _STATE[variant]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_classes_are_what_they_are_listed_for(variant):
    st = _state(variant)
    s, f32, f64, g = st["s"], st["f32"], st["f64"], st["g"]
    cl = s["classes"]
    names = [c for c in GC.CLASSES if not (variant == "far_origin" and c in GC.GRID_CLASSES)]
    assert list(cl) == names and all(len(cl[c]) >= 64 for c in names)
    assert sum(len(v) for v in cl.values()) == s["means3D"].shape[0]
    vis = f32["radii"] > 0
    culled = np.flatnonzero(~vis)
    if "near_cut" in cl:        # the culled rows are the even rows of near_cut and nothing else
        np.testing.assert_array_equal(culled, cl["near_cut"][0::2])
        lo, hi, zlo, zhi = GC.near_cut_depths(s)
        assert zlo <= np.float32(0.2) < zhi and hi == np.nextafter(lo, np.float32(1.0)) and zhi - zlo <= np.float32(2.0 ** -22)
        np.testing.assert_array_equal(s["means3D"][cl["near_cut"][0::2], 2], lo)
        np.testing.assert_array_equal(s["means3D"][cl["near_cut"][1::2], 2], hi)
        np.testing.assert_array_equal(s["means3D"][cl["near_cut"][0::2], :2], s["means3D"][cl["near_cut"][1::2], :2])
    else:
        assert culled.size == 0
    # every non-culled row has an upstream gradient in each of the three tensors the chain starts from
    acc = g["acc"]
    for what, sl in (("dL_dmeans2D", slice(0, 2)), ("dL_dconic", slice(2, 5)), ("dL_dcolors", slice(6, 9))):
        none = vis & ~(np.abs(acc[:, sl]).max(axis=1) > 0)
        assert not none.any(), (what, np.flatnonzero(none))
    # the fp32 and the float64 forward take the same decisions on every row but clamp_edge
    in32, in64 = GR.grad_mul(s, False), GR.grad_mul(s, True)
    other = np.ones(len(vis), bool)
    if st["edge"] is not None:
        other[st["edge"]] = False
    np.testing.assert_array_equal(f32["radii"], f64["radii"])
    np.testing.assert_array_equal(f32["clamped"][vis], f64["clamped"][vis])
    for a, b in zip(in32, in64):
        np.testing.assert_array_equal(a[other], b[other])
    # which decisions
    for c in names:
        x_in, y_in = in32[0][cl[c]], in32[1][cl[c]]
        if c == "clamp_edge":
            assert x_in.any() and not x_in.all() and y_in.all()       # both sides of the x clamp
            m = s["means3D"][cl[c]]
            ratio = np.abs(m[:, 0].astype(np.float64) / (m[:, 2].astype(np.float64) + float(s["viewmatrix"][3, 2])))
            lim = float(np.float32(1.3) * np.float32(s["tanfovx"]))
            assert (np.abs(ratio / lim - 1.0) <= 4 * 2.0 ** -23).all()
        else:
            assert (x_in == (c not in ("clamp_x", "clamp_xy"))).all() and (y_in == (c not in ("clamp_y", "clamp_xy"))).all(), c
    diag = float(np.hypot(s["W"], s["H"]))
    assert (f32["radii"][np.concatenate([cl["clamp_x"], cl["clamp_y"], cl["clamp_xy"]])] > diag).any()
    # depths, scales, quaternions, colours
    V = s["viewmatrix"].astype(np.float64)
    zv = s["means3D"].astype(np.float64) @ V[:3, 2] + V[3, 2]
    for c in ("near", "near_needle"):
        assert ((zv[cl[c]] > 0.2004) & (zv[cl[c]] < 0.2301)).all()
    if s["scales"] is not None:
        sm = s["scale_modifier"]
        assert np.allclose(s["scales"][cl["tiny"]] * sm, 1e-7, rtol=1e-6)
        for c, (lo_, hi_) in (("needle_side", (0.02, 0.08)), ("needle_diag", (0.02, 0.05)), ("needle_endon", (0.02, 0.08)),
                              ("near_needle", (0.003, 0.01))):
            sc_ = s["scales"][cl[c]].astype(np.float64) * sm
            assert ((sc_[:, 0] >= lo_ * (1 - 1e-6)) & (sc_[:, 0] <= hi_ * (1 + 1e-6))).all() and np.allclose(sc_[:, 1:], 1e-4, rtol=1e-6)
        qn = np.linalg.norm(s["rotations"].astype(np.float64), axis=1)
        assert ((qn[cl["qnorm"]] >= 0.3 - 1e-6) & (qn[cl["qnorm"]] <= 3 + 1e-6)).all() and np.ptp(qn[cl["qnorm"]]) > 1.5
        assert np.allclose(np.delete(qn, cl["qnorm"]), 1.0, atol=1e-6)
    if s["shs"] is not None:
        n_cl = f32["clamped"][cl["sh_clamped"]].sum(axis=1)
        assert ((n_cl == 1) | (n_cl == 2)).all() and (n_cl == 1).any() and (n_cl == 2).any()
        rgb64 = f64["rgb"][cl["sh_clamped"]]      # (clamped channels read 0; the channel just above 0 is the smallest positive)
        just = np.where(rgb64 > 0, rgb64, np.inf).min(axis=1)
        assert ((just >= 1e-4) & (just <= 1e-3)).all()
    assert ((s["opacities"] >= 0.01) & (s["opacities"] <= 0.04)).all()
    # the mask
    blended = f32["n_contrib"] > 0
    print(f"HARD {variant}: P {len(vis)} visible {int(vis.sum())} instances {f32['num_rendered']} min final_T {f32['final_T'].min():.3f} "
          f"masked {int(st['mask'].sum())} of {int(blended.sum())} blended pixels")
    assert int(st["mask"].sum()) <= MASK_MAX_SHARE_OF_BLENDED * int(blended.sum())
    assert float(f32["final_T"].min()) > 0.05           # nothing saturates: far from the T < 1e-4 stop


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "colors_precomp"])
def test_sh_clamped_margin_below_zero(variant):
    """The clamped channels of sh_clamped lie below 0 by at least 1e-4 (float64 evaluation of the stored float32 coefficients)."""
    s = GC.hard_scene(**VARIANTS[variant])
    r = s["classes"]["sh_clamped"]
    d = s["means3D"][r].astype(np.float64) - s["campos"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    res = GC.SH_C0 * s["shs"][r, 0, :].astype(np.float64) + 0.5
    if s["sh_degree"] == 3:
        res = res + GC.sh_rest(d, s["shs"][r])
    assert ((res <= -1e-4) | ((res >= 1e-4) & (res <= 1e-3)) | (res >= 0.1)).all()
    assert ((res <= -1e-4).sum(axis=1) >= 1).all() and (((res >= 1e-4) & (res <= 1e-3)).sum(axis=1) == 1).all()


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_row_is_graded_and_the_fp32_statement_passes(variant):
    st = _state(variant)
    s, x64, E, sc = st["s"], st["x64"], st["E"], st["sc"]
    worst_e, worst_r = GR.table(st["x32"], x64, E, sc, s["classes"], "cpu:" + variant)
    vis = st["f32"]["radii"] > 0
    for k in GR.TENSORS:                                   # no row is exempt: every visible row has a float64 gradient to be held to
        if x64[k].size == 0 or (k in ("dL_dscales", "dL_drotations") and s["scales"] is None):
            assert not np.asarray(x64[k]).any()
            continue
        assert (sc[k][vis] > 0).all(), (k, np.flatnonzero(vis & ~(sc[k] > 0)))
        assert not (sc[k][~vis] > 0).any()
        assert np.isfinite(E[k]).all()
    assert GR.cap_violations(E, sc, s["classes"]) == []    # the cap: E_i <= 1e-2 s_i
    assert worst_e <= GR.CAP
    assert GR.failures(st["x32"], x64, E, sc, 1.0, s["classes"]) == []    # ratio <= 1 by construction (the base copy is in E)
    # an independent jittered fp32 sample (inputs the yardstick has not seen), against float64 at ITS inputs (far_origin: one
    # ulp of a coordinate of 100 moves the Gaussian by 8e-6; clamp_edge: one ulp of x is the other decision), stays within the
    # ceiling of the yardsticks taken at the base inputs
    sj = GR.jitter(s, np.random.default_rng(991))
    xj = GR.chain(sj, st["up"], st["f32"]["radii"], st["f32"]["clamped"], False)
    xj64 = GR.chain(sj, st["up"], st["f32"]["radii"], st["f32"]["clamped"], True, st["edge"])
    r = GR.ratios(xj, xj64, E, sc)
    print("INDEPENDENT", variant, {k[3:]: f"{float(r[k][0].max()):.2f}" for k in GR.TENSORS})
    assert GR.failures(xj, xj64, E, sc, K, s["classes"]) == []
    # the float64 statement has the exact zeros the kernel is held to
    if "near_cut" in s["classes"]:
        for k in GR.TENSORS:
            assert not np.asarray(x64[k])[s["classes"]["near_cut"][0::2]].any()
    if s["shs"] is not None:
        r = s["classes"]["sh_clamped"]
        flags = st["f32"]["clamped"][r].astype(bool)
        dsh = np.asarray(x64["dL_dsh"])[r]
        assert not dsh[np.broadcast_to(flags[:, None, :], dsh.shape)].any() and (np.abs(dsh[:, 0, :])[~flags] > 0).all()


def _mutant(st, name):
    """(class the mutation is aimed at, the fp32 statement with one argument wrong)."""
    s, up, f32 = st["s"], st["up"], st["f32"]
    radii, clamped = f32["radii"], f32["clamped"]
    if name == "scale_modifier":
        return "plain", GR.chain(dict(s, scale_modifier=float(np.float32(s["scale_modifier"] * (1 + 1e-4)))), up, radii, clamped, False)
    if name == "tan_fovx":
        return "clamp_x", GR.chain(dict(s, tanfovx=s["tanfovx"] * 1.2), up, radii, clamped, False)
    if name == "clamped_flag":
        flipped = clamped.copy()
        flipped[s["classes"]["sh_clamped"]] ^= 1
        return "sh_clamped", GR.chain(s, up, radii, flipped, False)
    if name == "dL_dconic_y":
        up2 = dict(up, dL_dconic=up["dL_dconic"].copy())
        up2["dL_dconic"][:, 1] *= np.float32(1 + 1e-4)
        return "plain", GR.chain(s, up2, radii, clamped, False)
    if name == "quaternion_normalised":
        q = s["rotations"].astype(np.float64)
        return "qnorm", GR.chain(dict(s, rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)), up, radii, clamped, False)
    if name == "cov3D_of_the_other_form":
        # (a precomputed covariance ignores the modifier: at 0.6 the other form's cov3D is 1 / 0.36 of this one's)
        other = GC.hard_scene("cov3D_precomp", scale_modifier=s["scale_modifier"])
        return "plain", GR.chain(s, up, radii, clamped, False, cov=other["cov3D_precomp"])
    raise KeyError(name)


@pytest.mark.parametrize("name", ["scale_modifier", "tan_fovx", "clamped_flag", "dL_dconic_y", "quaternion_normalised",
                                  "cov3D_of_the_other_form"])
def test_the_comparator_rejects_a_subtly_wrong_argument(name):
    st = _state("scale_modifier" if name in ("scale_modifier", "cov3D_of_the_other_form") else "sh3")
    aimed, x = _mutant(st, name)
    bad = GR.failures(x, st["x64"], st["E"], st["sc"], K, st["s"]["classes"])
    print("MUTANT", name, "aimed at", aimed, "->", [(c, k, f"{r:.3g}", n, z, f) for c, k, r, n, z, f in bad if c == aimed])
    assert any(c == aimed for c, *_ in bad), (name, bad)
    if name == "scale_modifier":       # also at modifier 1
        st1 = _state("sh3")
        _, x1 = _mutant(st1, name)
        assert any(c == aimed for c, *_ in GR.failures(x1, st1["x64"], st1["E"], st1["sc"], K, st1["s"]["classes"]))
    if name == "clamped_flag":         # through the exact-zero rule as well as through the bar
        assert any(c == aimed and k == "dL_dsh" and z > 0 for c, k, _, _, z, _ in bad)


def test_subsets_keep_their_classes():
    for n in (1, 255, 256, 257):
        s = GC.hard_scene("sh3", rows=GC.spread_rows(n))
        assert s["means3D"].shape[0] == n and sum(len(v) for v in s["classes"].values()) == n
        full = GC.hard_scene("sh3")
        for c, idx in s["classes"].items():
            for i in idx[:2]:
                assert any(np.array_equal(s["means3D"][i], full["means3D"][j]) for j in full["classes"][c])
