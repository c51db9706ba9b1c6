"""What the float64 check of the blend kernels (tests/test_blend_f64_gpu.py) rests on, without a GPU: the cases hold the classes
they are listed for, the clear-pixel mask hides little, the numpy statements are what they claim to be, and the comparator
passes the fp32 statements and rejects planted flaws -- the first of which the old gradient bar cannot see."""
import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import blend_cases as BC
from tests import blend_reference as BR
from tests.test_blend_f64_gpu import K

CASES = list(BC.CASES)


def _ref(name, form="bg", S=None):
    return BR.reference(BC.case(name), form, S=S)


def _tile_pixels(s, tiles):
    top = BR.tile_of_pixel(s["W"], s["H"]).reshape(-1)
    return np.flatnonzero(np.isin(top, tiles))


def _entries(ref, pix):
    """The float64 (power, opacity x G, alpha, passes-the-tests) of every entry of pixel `pix`'s tile list at that pixel."""
    st = ref["st"]
    W = st["W"]
    y, x = divmod(int(pix), W)
    t = (y // 16) * ((W + 15) // 16) + x // 16
    tl = BR._Tile(st, t, np.float64)
    lane = (y % 16) * 16 + x % 16
    return tl.power[:, lane], (tl.op * tl.G)[:, lane], tl.alpha[:, lane], tl.ok[:, lane]


def _lists(ref):
    r = ref["st"]["ranges"].astype(np.int64)
    return r[:, 1] - r[:, 0]


# ---- the classes ------------------------------------------------------------------------------------------------------------

def test_batch_edges_lists_have_the_listed_lengths_and_nothing_stops():
    s, ref = BC.case("batch_edges"), _ref("batch_edges")
    n = _lists(ref)
    for cnt in BC.BATCH_COUNTS:
        assert n[s["classes"][f"n{cnt}"][0]] == cnt
    assert (ref["st"]["tiles_touched"] == 1).all()                  # footprints stay inside one tile
    assert not ref["walk64"]["stop_pos"].any()
    assert (ref["n64"].reshape(-1)[_tile_pixels(s, s["classes"]["n129"])] == 129).any()


def test_stop_pixels_stop_where_listed():
    s, ref = BC.case("stop"), _ref("stop")
    sp, T = ref["walk64"]["stop_pos"].reshape(-1), ref["T64"].reshape(-1)
    cl = s["classes"]
    for p in (3, 4, 63, 64, 65):
        assert (sp[cl[f"stop_at_{p}"]] == p).all(), p
    assert _lists(ref)[5] == 40 and (sp[cl["stop_at_last"]] == 40).all()
    assert ((T[cl["tiny_final_T"]] >= 1e-4) & (T[cl["tiny_final_T"]] <= 1e-3)).all()
    assert (sp[cl["quadrants_stop"]] > 0).all()
    assert not sp[cl["quadrants_never"]].any() and (ref["n64"].reshape(-1)[cl["quadrants_never"]] > 0).any()


def test_clamp_pixels_sit_on_and_just_under_the_clamp():
    s, ref = BC.case("clamp"), _ref("clamp")
    for pix in s["classes"]["clamped"]:
        _, raw, alpha, ok = _entries(ref, pix)
        assert (ok & (raw > 0.99) & (alpha == 0.99)).any()
    for pix in s["classes"]["just_under"]:
        _, raw, alpha, ok = _entries(ref, pix)
        assert (ok & (alpha >= 0.97) & (alpha < 0.99)).any()          # alpha / (1 - alpha) from 32 to 99


def test_faint_pixels_blend_faint_entries_between_rejected_ones():
    s, ref = BC.case("faint"), _ref("faint")
    assert np.abs(s["colors_precomp"]).max() > 9 and (s["colors_precomp"] < -5).any() and (s["colors_precomp"] > 5).any()
    for pix in s["classes"]["faint"][::17]:
        power, raw, alpha, ok = _entries(ref, pix)
        assert ok.sum() >= 10 and (alpha[ok] * 255 >= 1.2).all() and (alpha[ok] * 255 <= 3.0).all()
        assert ((power <= 0) & (alpha * 255 < 0.9)).sum() >= 10      # below the threshold
        assert (power > 1e-3).sum() >= 10                            # an indefinite conic: power > 0
        kinds = np.where(ok, 0, np.where(power > 0, 2, 1))
        assert (np.diff(kinds) != 0).sum() >= 20                     # interleaved


def test_split_lists_split_as_listed_and_pixels_stop_where_listed():
    s, ref = BC.case("split"), _ref("split")
    n, cl = _lists(ref), s["classes"]
    for key, (t, cnt) in BC.SPLIT_TILES.items():
        assert cl[key][0] == t and n[t] == cnt
    nseg = {S: [BC.split_of(cnt, S)[0] for _, cnt in BC.SPLIT_TILES.values()] for S in BC.SPLIT_S}
    assert nseg == {128: [2, 3, 18], 256: [1, 1, 9], 1024: [1, 1, 3]}     # unsplit, two, three, many
    sp = ref["walk64"]["stop_pos"].reshape(-1)
    idx = {k: int(sp[cl[k][0]]) - 1 for k in BC.SPLIT_PLANTS}           # list index of the entry that stops the pixel
    assert idx == {k: v[0][2] for k, v in BC.SPLIT_PLANTS.items()}
    for S in BC.SPLIT_S:
        ns, L = BC.split_of(2200, S)
        assert idx["stop_first_seg"] // L == 0 and idx["stop_last_seg"] // L == ns - 1
        assert idx["stop_seg_last_entry"] % L == L - 1 and idx["stop_seg_first_entry"] % L == 0
    assert 0 < idx["stop_middle_seg"] // 128 < 17 and 0 < idx["stop_middle_seg"] // 256 < 8
    assert not sp[cl["never"]].any()
    assert (s["bg7"] != 0).all()


@pytest.mark.parametrize("name", ["border_37x21", "border_7x5"])
def test_border_tiles_are_cut_and_gaussians_sit_on_the_last_row_and_column(name):
    s, ref = BC.case(name), _ref(name)
    W, H = s["W"], s["H"]
    assert W % 16 and H % 16
    m2 = ref["st"]["means2D"]
    assert (np.isclose(m2[:, 0], W - 1, atol=0.2) | np.isclose(m2[:, 1], H - 1, atol=0.2)).all()
    sp = ref["walk64"]["stop_pos"].reshape(-1)
    assert (sp[s["classes"]["edge"]] > 0).any() and (sp[s["classes"]["edge"]] == 0).any()


def test_needles_are_thin_and_their_power_cancels():
    s, ref = BC.case("needles"), _ref("needles")
    st = ref["st"]
    co = st["conic_opacity"].astype(np.float64)[st["radii"] > 0]
    mid, det = 0.5 * (co[:, 0] + co[:, 2]), co[:, 0] * co[:, 2] - co[:, 1] ** 2
    root = np.sqrt(np.maximum(mid * mid - det, 0))
    assert np.median((mid + root) / (mid - root)) > 10                 # the conic's eigenvalue ratio
    assert (st["tiles_touched"] > 1).any()
    worst = 0.0
    for t in range(len(st["ranges"])):
        tl = BR._Tile(st, t, np.float64)
        if tl.n:
            terms = np.abs(tl.a * tl.dx * tl.dx) + np.abs(tl.c * tl.dy * tl.dy) + 2 * np.abs(tl.b * tl.dx * tl.dy)
            worst = max(worst, float((terms / np.maximum(2 * np.abs(tl.power), 1e-30))[tl.ok].max(initial=0.0)))
    assert worst > 10                                                  # a blended entry whose power is a difference of terms ten times its size


# ---- the mask ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_the_mask_hides_little(name):
    """At most 5 % of a case's blended pixels are not clear; every class keeps 90 % of its pixels (a class of tiles: of those
    tiles' blended pixels); 90 % of the Gaussians with a gradient keep one, in every form."""
    s, ref = BC.case(name), _ref(name)
    clear, blended = ref["clear"].reshape(-1), ref["n64"].reshape(-1) > 0
    share = float((blended & ~clear).sum()) / max(1, int(blended.sum()))
    print(f"BLEND64 MASK {name:<14s} not clear: {int((blended & ~clear).sum())} of {int(blended.sum())} blended pixels = {100 * share:.2f} %")
    assert share <= 0.05
    for key, idx in s["classes"].items():
        tiles = key.startswith(("n", "list_")) and name in ("batch_edges", "split") and key != "never"
        pix = _tile_pixels(s, idx) if tiles else idx
        pix = pix[blended[pix]] if tiles or key in ("all", "edge", "quadrants_never") else pix
        assert clear[pix].sum() >= 0.9 * len(pix), (key, int(clear[pix].sum()), len(pix))
    for form in BC.FORMS:
        r = _ref(name, form)
        full = BR.oracle_f64(r["st"], r["pss"], np.ones_like(r["clear"]))
        for k, x in BR.grads_of(form, full["acc"]).items():
            had, has = np.abs(x).max(axis=1) > 0, np.abs(r["x64"][k]).max(axis=1) > 0
            assert (had & has).sum() >= 0.9 * had.sum(), (form, k, int((had & has).sum()), int(had.sum()))


# ---- the statements ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", CASES)
def test_numpy_statement_one_is_the_oracle_bit_for_bit(name):
    s, ref = BC.case(name), _ref(name)
    st, stm = ref["st"], ref["statements"]["oracle"]
    fw = O.forward(dict(s, bg=ref["pss"][0][1]))
    for k, x in (("out_color", stm["out"][0]), ("final_T", stm["final_T"])):
        np.testing.assert_array_equal(fw[k].view(np.uint32), x.view(np.uint32), err_msg=k)
    np.testing.assert_array_equal(fw["n_contrib"], stm["n_contrib"])
    g = O.backward(dict(s, bg=ref["pss"][0][1]), fw, ref["pss"][0][2] * ref["clear"][None])
    acc = stm["acc"][0].astype(np.float32)
    for k, x in (("dL_dmeans2D", g["dL_dmeans2D"][:, :2]), ("dL_dconic", g["dL_dconic"][:, [0, 1, 3]]), ("dL_dopacity", g["dL_dopacity"]),
                 ("dL_dcolors", g["dL_dcolors"])):
        np.testing.assert_array_equal(x.view(np.uint32), np.ascontiguousarray(BR.grads_of("bg", [acc])[k]).view(np.uint32), err_msg=k)


@pytest.mark.parametrize("name", CASES)
def test_float64_walk_is_the_oracles_float64_build(name):
    ref = _ref(name)
    w, c = ref["walk64"], ref["c64"]
    np.testing.assert_array_equal(w["n_contrib"], c["n_contrib"])
    assert np.abs(w["final_T"] - c["final_T"]).max() <= 1e-12
    assert np.abs(w["out"][0] - c["out"][0]).max() <= 1e-12 * max(1.0, np.abs(c["out"][0]).max())
    # the fp32 oracle takes every decision of a clear pixel the way the float64 walk does
    fw = O.forward(dict(BC.case(name), bg=ref["pss"][0][1]))
    np.testing.assert_array_equal(fw["n_contrib"][ref["clear"]], c["n_contrib"][ref["clear"]])


def test_acc_abs_is_the_sum_of_the_terms_magnitudes():
    for form in ("bg", "seven"):
        ref = _ref("border_7x5", form)
        for a, b, x in zip(ref["walk64"]["abs"], ref["c64"]["abs"], ref["c64"]["acc"]):
            assert b.max() > 0 and (b >= np.abs(x) * (1 - 1e-12)).all()
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    s = BC.case("border_7x5")
    fw = O.forward(s)
    g = O.backward(s, fw, s["dpix7"][:3], acc_abs=True)                # the fp32 build's, through the front-end
    assert (g["acc_abs"] >= np.abs(g["acc"]) * (1 - 1e-6)).all() and g["acc_abs"].max() > 0


# ---- the comparator ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("name", CASES)
def test_comparator_passes_every_fp32_statement(name, form):
    for S in (BC.SPLIT_S if name == "split" else (None,)):
        ref = _ref(name, form, S)
        for stname, stm in ref["statements"].items():
            rep = BR.grade(ref, *BR.statement_outputs(ref, stm))
            assert BR.failures(rep, K) == [], (name, form, S, stname, rep)


PLANTED = [("final_T_scaled", "batch_edges", "bg", None), ("final_T_scaled", "needles", "black", None), ("final_T_scaled", "split", "bg", 1024), ("stop_on_T", "stop", "bg", None),
           ("no_clamp", "clamp", "bg", None), ("no_bg_term", "clamp", "bg", None), ("no_bg_term", "stop", "seven", None),
           ("seam_product", "split", "bg", 128), ("seam_suffix", "split", "bg", 128), ("outside_live", "border_37x21", "bg", None),
           ("outside_live", "border_7x5", "black", None)]


@pytest.mark.parametrize("flaw,name,form,S", PLANTED)
def test_comparator_rejects_planted_flaw(flaw, name, form, S):
    ref, bad = BR.flawed(BC.case(name), form, flaw, S)
    rep = BR.grade(ref, *BR.statement_outputs(ref, bad))
    print(f"BLEND64 FLAW {flaw:<15s} {name:<13s} {form:<6s}", {k: (v if k == "n_contrib" else float(f"{v:.3g}")) for k, v in rep.items()})
    assert BR.failures(rep, K) != [], rep
    if flaw == "stop_on_T":
        assert rep["n_contrib"] > 0
    if flaw in ("final_T_scaled", "no_bg_term", "seam_suffix", "outside_live"):      # a backward flaw: the image is untouched
        assert rep["out_color"] <= 1 and rep["final_T"] <= 1 and rep["n_contrib"] == 0
        assert max(v for k, v in rep.items() if k.startswith("dL_")) > K


def test_the_old_gradient_bar_cannot_see_a_scaled_final_T():
    """final_T (1 + 2e-5) handed to the backward passes test_gpu_raster._grad_check_strict against the same float64 reference
    (and fails this comparator: test_comparator_rejects_planted_flaw)."""
    from tests.test_gpu_raster import _grad_check_strict
    for name, form in (("batch_edges", "bg"), ("needles", "black")):
        ref, bad = BR.flawed(BC.case(name), form, "final_T_scaled")
        g = BR.grads_of(form, bad["acc"])
        report = _grad_check_strict(g, ref["x64"], keys=BR.TENSORS3, label=f"scaled final_T, {name}")
        assert max(v[0] for v in report.values()) > 2e-6           # (it does move the gradients: by a fifth of that bar or less)
