"""Independent checks of the (reference-unpinned) oracle arithmetic:
fp64 central finite differences of the backward, a brute-force 3-NN for distCUDA2, and the per-pixel mask of near-threshold
decisions that the strict GPU gradient checks zero dL_dpix on (tests/test_gpu_raster.py _grad_check_strict)."""
import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import scenes


def _loss(s, dpix):
    f = O.forward(s, f64=True)
    return float((f["out_color"] * dpix).sum()), f


@pytest.mark.parametrize("variant", ["sh3_scalerot", "precomp_color_cov", "sh0_bg"])
def test_backward_matches_finite_differences(variant):
    kw = dict(P=60, W=48, H=32, seed=3, behind_frac=0.0, scale_lo=0.02, scale_hi=0.08)
    if variant == "sh3_scalerot":
        s = scenes.random_scene(sh_degree=3, bg=(0.2, 0.1, 0.3), **kw)
    elif variant == "precomp_color_cov":
        s = scenes.random_scene(use_colors_precomp=True, use_cov3D_precomp=True, neg_colors=True, bg=(0.5, 0.5, 0.1), **kw)
    else:
        s = scenes.random_scene(sh_degree=0, bg=(1.0, 1.0, 1.0), **kw)
    for k in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp", "viewmatrix",
              "projmatrix", "campos", "bg"):
        if s.get(k) is not None:
            s[k] = np.asarray(s[k], np.float64)
    rng = np.random.default_rng(7)
    dpix = rng.normal(size=(3, s["H"], s["W"]))
    _fd_check(s, dpix, rng)
    # the same with dpix zeroed on the pixels that hold a near-threshold decision (what the strict GPU gradient check feeds
    # both sides): the masked loss is a loss the oracle differentiates correctly too
    mask = O.fragile_pixels(s, O.forward(s, f64=True), f64=True)
    assert mask.shape == (s["H"], s["W"]) and mask.dtype == bool
    print(variant, "masked pixels", int(mask.sum()), "of", mask.size)
    _fd_check(s, dpix * ~mask, np.random.default_rng(8))


def _fd_check(s, dpix, rng):
    """Analytic f64 backward of sum(out_color * dpix) against central differences on sampled elements of every input."""
    L0, f = _loss(s, dpix)
    g = O.backward(s, f, dpix, f64=True)
    pairs = [("means3D", "dL_dmeans3D"), ("opacities", "dL_dopacity"), ("shs", "dL_dsh"),
             ("colors_precomp", "dL_dcolors"), ("scales", "dL_dscales"), ("rotations", "dL_drotations"),
             ("cov3D_precomp", "dL_dcov3D")]
    h = 1e-6
    checked = 0
    for name, gname in pairs:
        if s.get(name) is None:
            continue
        x = s[name]
        flat_idx = rng.choice(x.size, size=min(12, x.size), replace=False)
        for fi in flat_idx:
            idx = np.unravel_index(fi, x.shape)
            old = x[idx]
            x[idx] = old + h
            Lp, fp = _loss(s, dpix)
            x[idx] = old - h
            Lm, fm = _loss(s, dpix)
            x[idx] = old
            # skip samples where a hard threshold (n_contrib / radius / culling) changed across the stencil
            if not (np.array_equal(fp["n_contrib"], fm["n_contrib"]) and np.array_equal(fp["radii"], fm["radii"])
                    and np.array_equal(fp["point_list"], fm["point_list"])):
                continue
            fd = (Lp - Lm) / (2 * h)
            an = g[gname].reshape(x.shape)[idx] if gname != "dL_dopacity" else g[gname][idx[0], 0]
            # cov3D off-diagonals: the kernel's gradient is w.r.t. the 6 stored entries -- same as FD on them
            assert abs(fd - an) <= 2e-4 * max(1.0, abs(fd), abs(an)), (name, idx, fd, an)
            checked += 1
    assert checked >= 20


def test_means2D_grad_is_pixel_grad_times_half_extent():
    """dL_dmeans2D = dL/d(pixel pos) * (0.5 W, 0.5 H) (CR/backward_distwar.cu:917-918,1002-1003)."""
    s = scenes.random_scene(P=40, W=48, H=32, seed=5, behind_frac=0.0, scale_lo=0.03, scale_hi=0.08)
    rng = np.random.default_rng(1)
    dpix = rng.normal(size=(3, s["H"], s["W"]))
    f = O.forward(s, f64=True)
    g = O.backward(s, f, dpix, f64=True)
    C = O.C
    L = O.lib()
    # FD on means2D through the blend only
    h = 1e-6
    n = O.normalize_inputs(s, True)
    tested = 0
    for i in np.nonzero(f["radii"] > 0)[0][:10]:
        for ax in range(2):
            vals = []
            for sgn in (+1, -1):
                m2 = f["means2D"].copy()
                m2[i, ax] += sgn * h
                out = np.zeros_like(f["out_color"]); fT = np.zeros_like(f["final_T"]); nc = np.zeros_like(f["n_contrib"])
                L.hgs_oracle_render_f64(C.c_int(s["W"]), C.c_int(s["H"]), O._p(f["ranges"]), O._p(f["point_list"]),
                                        O._p(m2), O._p(f["features"]), O._p(f["conic_opacity"]), O._p(n["bg"]),
                                        O._p(fT), O._p(nc), O._p(out))
                vals.append(((out * dpix).sum(), nc))
            if not np.array_equal(vals[0][1], vals[1][1]):
                continue
            fd = (vals[0][0] - vals[1][0]) / (2 * h)
            scale = 0.5 * (s["W"] if ax == 0 else s["H"])
            an = g["dL_dmeans2D"][i, ax]
            assert abs(fd * scale - an) <= 2e-4 * max(1.0, abs(an)), (i, ax, fd * scale, an)
            tested += 1
    assert tested >= 8


def _brute_dist2(p):
    p = p.astype(np.float32)
    out = np.zeros(p.shape[0], np.float32)
    for i in range(p.shape[0]):
        d = p - p[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d2[i] = np.inf
        b = np.sort(d2)[:3]
        out[i] = ((b[0] + b[1]) + b[2]) / np.float32(3.0)
    return out


@pytest.mark.parametrize("P", [4, 17, 1024, 1025, 3000])
def test_dist2_oracle_equals_bruteforce(P):
    rng = np.random.default_rng(P)
    pts = (rng.normal(size=(P, 3)) * 0.3 + np.array([0.5, -0.2, 1.0])).astype(np.float32)
    if P == 3000:
        pts[:100] = pts[100:200]  # exact duplicates -> zero distances
    got = O.dist2(pts)
    np.testing.assert_array_equal(got, _brute_dist2(pts))


def test_binning_is_sorted_and_stable():
    s = scenes.random_scene(P=3000, W=200, H=120, seed=11, depth_levels=6, scale_lo=0.01, scale_hi=0.06)
    f = O.forward(s, render=False)
    k, v = f["keys_sorted"], f["point_list"]
    assert f["num_rendered"] == k.shape[0] == int(f["tiles_touched"].sum())
    assert (np.diff(k.astype(np.uint64)) >= 0).all()
    same = k[1:] == k[:-1]
    assert same.sum() > 50  # the scene really has exact (tile, depth) ties
    assert (v[1:][same] > v[:-1][same]).all()  # ties keep Gaussian-index order (stable LSD sort)
    T = f["ranges"].shape[0]
    tiles = (k >> np.uint64(32)).astype(np.int64)
    for t in np.unique(tiles):
        a, b = f["ranges"][t]
        assert (tiles[a:b] == t).all() and (a == 0 or tiles[a - 1] != t) and (b == len(k) or tiles[b] != t)
    empty = np.setdiff1d(np.arange(T), np.unique(tiles))
    assert (f["ranges"][empty] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# The mask of near-threshold decisions (oracle/raster_oracle.c pixel_mask, O.fragile_pixels).  The strict GPU gradient
# checks zero dL_dpix on it and then hold EVERY Gaussian to 1e-4 of scale; these tests pin what the mask means and that
# masking cannot hide a scene: few pixels go, (almost) every graded Gaussian stays graded.
MASK_MAX_SHARE_OF_BLENDED = 0.05
MASK_MIN_GRADED_KEPT = 0.90
_STATE = {}


def _scene_state(name):
    """(scene, oracle forward, mask, unmasked backward with mask) of a scene of scenes.ALL; dL_dpix from seed 123."""
    if name not in _STATE:
        _STATE.clear()                                    # (one scene at a time: many_tiles holds 4.5 M pixels)
        s = scenes._scene(name)
        f = O.forward(s)
        dpix = np.random.default_rng(123).normal(size=(3, s["H"], s["W"])).astype(np.float32)
        g = O.backward(s, f, dpix, pixel_mask=True)
        _STATE[name] = (s, f, dpix, g)
    return _STATE[name]


def _walk_masks(s, f):
    """Independent restatement, pixel by pixel in numpy: (mask [H, W], fragile [P], touched [P]) from ranges, point_list,
    n_contrib, means2D and conic_opacity.  power in the oracle's fp32 operation order; exp taken in double and rounded (where
    libm expf is correctly rounded that is the same number; a last-bit difference moves alpha x 255 by 6e-8 of a 1e-4 window)."""
    W, H = s["W"], s["H"]
    gx = (W + 15) // 16
    m2, co = f["means2D"], f["conic_opacity"]
    P = m2.shape[0]
    mask, fragile, touched = np.zeros((H, W), bool), np.zeros(P, bool), np.zeros(P, bool)
    half = np.float32(-0.5)
    for py in range(H):
        for px in range(W):
            r0 = int(f["ranges"][(py // 16) * gx + px // 16, 0])
            ids = f["point_list"][r0:r0 + int(f["n_contrib"][py, px])]
            if ids.size == 0:
                continue
            dx, dy = m2[ids, 0] - np.float32(px), m2[ids, 1] - np.float32(py)
            c = co[ids]
            power = half * (c[:, 0] * dx * dx + c[:, 2] * dy * dy) - c[:, 1] * dx * dy
            assert power.dtype == np.float32
            G = np.exp(np.minimum(power, 0).astype(np.float64)).astype(np.float32)
            alpha = np.minimum(np.float32(0.99), c[:, 3] * G)
            p64, a64 = power.astype(np.float64), alpha.astype(np.float64)
            near = np.where(power > 0, p64 < 1e-5, (np.abs(a64 * 255.0 - 1.0) < 1e-4) | (np.abs(p64) < 1e-5))
            if near.any():
                mask[py, px] = True
                fragile[ids[near]] = True
                touched[ids[(power <= 0) & (alpha >= np.float32(1.0) / np.float32(255.0))]] = True
    return mask, fragile, touched | fragile


@pytest.mark.parametrize("name", scenes.ALL)
def test_fragile_pixel_mask_semantics(name):
    s, f, dpix, g = _scene_state(name)
    mask = g["fragile_pixels"]
    assert mask.shape == (s["H"], s["W"]) and mask.dtype == bool
    np.testing.assert_array_equal(O.fragile_pixels(s, f), mask)          # the convenience call; no dL_dpix involved
    assert "fragile_pixels" not in O.backward(s, f, dpix)                # only when asked
    assert not (g["fragile"] & ~g["touched"]).any()
    assert mask.any() == g["fragile"].any()
    assert not mask[f["n_contrib"] == 0].any()                            # a pixel that evaluates nothing decides nothing
    if name in ("tiny_image", "sh1_M16", "strands_precomp"):
        m_ref, fragile_ref, touched_ref = _walk_masks(s, f)
        np.testing.assert_array_equal(mask, m_ref)
        np.testing.assert_array_equal(g["fragile"], fragile_ref)
        np.testing.assert_array_equal(g["touched"], touched_ref)
    # linearity: every term a pixel contributes is linear in that pixel's dL_dpix, so the two halves add up to the whole --
    # the same fp32 terms, summed in double in another order
    g_out = O.backward(s, f, dpix * ~mask)
    g_in = O.backward(s, f, dpix * mask)
    scale = np.abs(g["acc"]).max(axis=0)
    diff = np.abs(g_out["acc"] + g_in["acc"] - g["acc"]).max(axis=0) if g["acc"].size else scale
    assert (diff <= 1e-10 * scale).all(), (diff, scale)
    # a Gaussian that is not touched gets nothing from the masked pixels
    assert not g_in["acc"][~g["touched"]].any()


@pytest.mark.parametrize("name", scenes.ALL)
def test_fragile_pixel_mask_hides_nothing(name):
    """The conditions under which zeroing dL_dpix on the mask leaves a check of the whole scene: at most 5 % of the blended
    pixels masked (one_huge_tile blends 8 pixels: at most 1), at least 90 % of the Gaussians with a gradient keep one.
    Measured: worst 2.15 % (dense_long_lists) and 96.8 % (one_huge_tile).  A scene added to scenes.ALL must meet them too."""
    s, f, dpix, g = _scene_state(name)
    mask = g["fragile_pixels"]
    blended = f["n_contrib"] > 0
    g_m = O.backward(s, f, dpix * ~mask)
    graded = np.abs(g["acc"]).max(axis=1) > 0
    kept = graded & (np.abs(g_m["acc"]).max(axis=1) > 0)
    print(f"MASK {name}: masked {int(mask.sum())} of {int(blended.sum())} blended pixels ({mask.size} pixels), graded "
          f"{int(graded.sum())}, still graded {int(kept.sum())}, fragile {int(g['fragile'].sum())}, touched {int(g['touched'].sum())}")
    if name == "one_huge_tile":
        assert int(mask.sum()) <= 1
    else:
        assert int(mask.sum()) <= MASK_MAX_SHARE_OF_BLENDED * int(blended.sum())
    assert int(kept.sum()) >= MASK_MIN_GRADED_KEPT * int(graded.sum())
    if name != "all_culled":
        assert graded.any() and blended.any()
