"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle on identical seeded inputs.

Bars (BASELINE.json north_star): tile/depth key ordering bit-exact; rendered RGB and per-parameter gradients within
1e-4 relative (fp32).  Everything the preprocess stage produces is checked BIT-EXACT as well (same fp32 operation
order, no contraction on either side).  The blend uses the hardware exp (v_exp_f32) where the oracle uses libm expf,
so a pixel whose alpha lands within an ulp of the 1/255 or T<1e-4 thresholds may take the other branch: such pixels
are counted and bounded (the reference on NVIDIA hardware has the same property against any CPU restatement).
"""
import os

import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import scenes
from tests.binning_cases import SEG_POLICY, SPLIT_MIN_LEN   # (lists up to SPLIT_MIN_LEN entries are never split across workgroups)
from tests.scenes import ALL, VARIANTS, _scene  # noqa: F401

pytestmark = pytest.mark.gpu

def _forward(s, cull):
    """Forward pass with tile culling (include/hgs.h HGS_TILE_CULL) on or off; the module default is restored."""
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    was = _C.set_tile_cull(cull)
    try:
        return G.run_forward(s)
    finally:
        _C.set_tile_cull(was)


def _long_tile_pixels(ranges, W, H):
    """[H, W] bool: pixels of tiles whose list (the given ranges) is long enough for the segment-parallel blend, which
    multiplies the transmittance segment by segment: the product associates differently when the list length changes
    (culling on/off), so such tiles agree to rounding instead of bit for bit."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    L = (ranges[:, 1].astype(np.int64) - ranges[:, 0]).reshape(gy, gx) > SPLIT_MIN_LEN
    return np.repeat(np.repeat(L, 16, 0), 16, 1)[:H, :W]


def _assert_same_image(a, b, ranges):
    """Bit-identical outside long tiles, 2e-6 absolute inside (see _long_tile_pixels; `ranges` = the longer lists)."""
    H, W = a.shape[-2:]
    lt = _long_tile_pixels(ranges, W, H)
    a2, b2 = a.reshape(-1, H, W), b.reshape(-1, H, W)
    np.testing.assert_array_equal(a2[:, ~lt].view(np.uint32), b2[:, ~lt].view(np.uint32))
    if lt.any():
        assert float(np.abs(a2[:, lt].astype(np.float64) - b2[:, lt]).max()) <= 2e-6


def _check_forward(name):
    return _check_forward_scene(_scene(name))


def _check_forward_scene(s):
    """_check_forward on a scene dict (tests/test_gaussians_f64_gpu.py runs it on every input form of `hard_gaussians`)."""
    from tests import gpu_util as G
    ref = O.forward(s)
    # the reference's own entry point with its 19 arguments (no culling): the tile lists are the reference's, every binning
    # stage is compared bit for bit.  render() and the training step cull instances that no pixel blends;
    # test_tile_cull_changes_no_output shows that nothing else changes.
    fw = G.run_forward(s)
    got = G.intermediates(s, fw)
    vis = ref["radii"] > 0
    assert got["status"][1] == 0 and got["status"][8] == 0   # no capacity overflow, no cooperative-wait timeout
    # ---- bit-exact stages
    np.testing.assert_array_equal(got["radii"], ref["radii"])
    np.testing.assert_array_equal(got["tiles_touched"], ref["tiles_touched"])
    np.testing.assert_array_equal(got["point_offsets"], ref["point_offsets"])
    assert got["num_rendered"] == ref["num_rendered"]
    for k in ("depths", "means2D", "conic_opacity"):
        np.testing.assert_array_equal(got[k][vis].view(np.uint32), ref[k][vis].view(np.uint32), err_msg=k)
    if s["cov3D_precomp"] is None:
        np.testing.assert_array_equal(got["cov3D"][vis].view(np.uint32), ref["cov3D"][vis].view(np.uint32))
    if s["colors_precomp"] is None:
        np.testing.assert_array_equal(got["rgb"][vis].view(np.uint32), ref["rgb"][vis].view(np.uint32))
        np.testing.assert_array_equal(got["clamped"][vis], ref["clamped"][vis])
    np.testing.assert_array_equal(got["ranges"], ref["ranges"])
    np.testing.assert_array_equal(got["point_list"], ref["point_list"])
    np.testing.assert_array_equal(got["keys_sorted"], ref["keys_sorted"])
    # ---- blend: tolerance + bounded threshold flips
    npix = s["W"] * s["H"]
    flips = int((got["n_contrib"] != ref["n_contrib"]).sum())
    assert flips <= max(2, npix // 2000), f"n_contrib differs on {flips}/{npix} pixels"
    same = got["n_contrib"] == ref["n_contrib"]
    err = np.abs(got["out_color"] - ref["out_color"])
    tol = 1e-4 * np.maximum(np.abs(ref["out_color"]), 1.0)
    bad = (err > tol)
    # pixels may exceed the tolerance only through a threshold flip (alpha~1/255 contributes <= 0.4% of full scale)
    nbad = int(bad.any(0).sum())
    assert nbad <= max(2, npix // 2000), f"{nbad} pixels outside 1e-4"
    assert err.max() <= 2e-2
    assert (np.abs(got["final_T"] - ref["final_T"])[same] <= 1e-4).all()
    return s, ref, fw, got


@pytest.mark.parametrize("name", ALL)
def test_forward_matches_oracle(name):
    _check_forward(name)


@pytest.mark.parametrize("name", ["strands", "dense_long_lists", "medium_lists", "many_tiles", "qhd_tiles", "all_culled", "one_huge_tile"])
def test_blend_work_list_covers_every_tile_once(name):
    """The blend kernels' work list (sort_tiles_kernel): split lists as consecutive ascending segments that tile the list
    exactly, every other tile exactly once in tile_order with list lengths (capped at 511) non-increasing."""
    from tests import binning_reference as BR
    from tests import gpu_util as G
    s = _scene(name)
    fw = G.run_forward(s)
    W, H = s["W"], s["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    got = G.intermediates(s, fw)
    split_tiles = BR.check_work_list(got["status"], G.blend_work_list(s, fw), got["ranges"], T, SEG_POLICY)
    if name in ("dense_long_lists", "medium_lists", "one_huge_tile"):
        assert split_tiles


def test_two_segment_lists_walked_by_one_workgroup():
    """Lists of exactly TWO segments (round 4: the forward's first segment workgroup walks both serially, the backward still
    runs two workgroups on what it left -- the transmittance in front of the second segment, the segments' colours and their
    suffix sum).  hgs_set_segment_policy pins the segment length so that tiles of `medium_lists` land in (1.5 S, 2 S]: against
    the unsplit walk of the same lists n_contrib and final_T are bit-identical and the image agrees to the association of one
    sum per pixel; the backward agrees with the oracle at the usual bar."""
    import hgs_runtime as rt
    from tests import gpu_util as G
    s = _scene("medium_lists")
    L = rt.lib()
    try:
        rt.check(L.hgs_set_segment_policy(1024, 1024, 1))          # lists up to 1536 entries: one workgroup per tile
        fw0 = G.run_forward(s)
        got0 = G.intermediates(s, fw0)
        n = (got0["ranges"][:, 1].astype(np.int64) - got0["ranges"][:, 0])
        assert n.max() <= 1536
        S = next(S for S in range(128, 1025, 64) if ((n > S + S // 2) & (n <= 2 * S)).any())
        two = np.flatnonzero((n > S + S // 2) & (n <= 2 * S))
        rt.check(L.hgs_set_segment_policy(S, S, 1))
        fw = G.run_forward(s)
        got = G.intermediates(s, fw)
        assert got["status"][6] == S and got["status"][8] == 0
        items = G.blend_work_list(s, fw)[:int(got["status"][5])]
        for t in two:
            assert sorted((items[(items & 0xFFFFFF) == t] >> 24).tolist()) == [0, 1]
        # on the two-segment tiles the transmittance is carried through both walks: the serial walk's bits (tiles of three and
        # more segments multiply per-segment products: rounding, like every split list)
        gx, gy = (s["W"] + 15) // 16, (s["H"] + 15) // 16
        tmask = np.zeros(gx * gy, bool)
        tmask[two] = True
        pm = np.repeat(np.repeat(tmask.reshape(gy, gx), 16, 0), 16, 1)[:s["H"], :s["W"]]
        assert pm.any()
        np.testing.assert_array_equal(got["n_contrib"][pm], got0["n_contrib"][pm])
        np.testing.assert_array_equal(got["final_T"][pm].view(np.uint32), got0["final_T"][pm].view(np.uint32))
        assert float(np.abs(got["final_T"].astype(np.float64) - got0["final_T"]).max()) <= 2e-6
        assert float(np.abs(got["out_color"].astype(np.float64) - got0["out_color"]).max()) <= 2e-6
        ref = O.forward(s)
        ref_state = dict(ref)
        ref_state["n_contrib"], ref_state["final_T"] = got["n_contrib"].copy(), got["final_T"].copy()
        dpix = np.random.default_rng(5).normal(size=(3, s["H"], s["W"])).astype(np.float32)
        gref = O.backward(s, ref_state, dpix)
        _grad_check(G.run_backward(s, fw, dpix), gref, ref)
        _strict_masked_backward(s, fw, ref_state, dpix, "two_segment medium_lists", gref)
    finally:
        rt.check(L.hgs_set_segment_policy(128, 1024, 2048))


GRAD_KEYS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations")
# Gradient bar (BASELINE.json north_star: "per-param grads within 1e-4 rel fp32"), enforced on EVERY element:
#   |got - ref| <= 1e-4 x max|ref tensor|       for every Gaussian the oracle does not mark fragile (measured: 1e-5 at
#       north_star, 6e-5 at C4 -- thin strands make `power` a difference of large terms, and the blend kernels contract
#       it into FMAs like nvcc does for the reference while the oracle rounds every operation)
#   |got - ref| <= 1e-4 x max(|ref|, 1e-2 x max|ref tensor|)  on all but NOISE_FRAC of the elements (the oracle sums in
#       double, the GPU in fp32: an element that cancels to ~0 sits at the fp32 noise of its terms, not at 1e-4 of itself)
# Fragile Gaussians (oracle/raster_oracle.c: a (pixel, entry) decision within 1e-4 of the alpha >= 1/255 threshold or
# 1e-5 of power > 0, where v_exp_f32 and libm expf may branch differently) are enumerated.  Their number is bounded by
# what the geometry predicts -- the pixels of a Gaussian whose power lies in a window of width dp cover an area of
# 2 pi sqrt(det cov2D) dp (uniform in power), so a Gaussian is fragile with probability ~ min(1, 2 pi dp / sqrt(det
# conic)) per view -- and their error is bounded too (single pixels with alpha ~ 1/255).
GRAD_MAX_OF_SCALE = 1e-4
GRAD_NOISE_FRAC = 2e-3
FRAGILE_MAX_OF_SCALE = 2e-2


def _expected_fragile(fwd_ref):
    """Expected number of Gaussians with a pixel inside the oracle's threshold windows (see above), from the preprocessed
    2D state: visible, opacity above 1/255, ring area 2 pi sqrt(det cov2D) x (2e-4 + 1e-5)."""
    co = fwd_ref["conic_opacity"].astype(np.float64)
    vis = (fwd_ref["radii"] > 0) & (co[:, 3] > 1.0 / 255.0)
    det = co[vis, 0] * co[vis, 2] - co[vis, 1] ** 2
    ring = 2.0 * np.pi / np.sqrt(np.maximum(det, 1e-30)) * 2.1e-4
    return float(np.minimum(1.0, ring).sum())


def _grad_check(g, gref, fwd_ref, skip=()):
    """Asserts the gradient bar above for every tensor; returns {name: (max error / tensor scale, fraction outside the
    element-wise tolerance, fragile Gaussians)} for the log."""
    fragile = gref["fragile"]
    P = fragile.shape[0]
    expected = _expected_fragile(fwd_ref)
    assert int(fragile.sum()) <= 3.0 * expected + 8, f"{int(fragile.sum())} of {P} Gaussians near a blend threshold, {expected:.1f} expected"
    report = {}
    for k in GRAD_KEYS:
        if k in skip or gref[k].size == 0:
            continue
        b = gref[k].astype(np.float64).reshape(P, -1)
        a = g[k].astype(np.float64).reshape(b.shape)
        scale = float(np.abs(b).max())
        if scale == 0.0:
            assert np.abs(a).max() == 0.0, k
            continue
        err = np.abs(a - b)
        solid = err[~fragile]
        worst = float(solid.max()) / scale if solid.size else 0.0
        frac = float((solid > 1e-4 * np.maximum(np.abs(b[~fragile]), 1e-2 * scale)).mean()) if solid.size else 0.0
        report[k] = (worst, frac, int(fragile.sum()))
        assert worst <= GRAD_MAX_OF_SCALE, (k, report[k])
        assert frac <= GRAD_NOISE_FRAC, (k, report[k])
        if fragile.any():
            assert float(err[fragile].max()) / scale <= FRAGILE_MAX_OF_SCALE, (k, float(err[fragile].max()) / scale)
    return report


KEYS7 = ("dL_dmeans2D_rgb", "dL_dcolors", "dL_dextra", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
         "dL_drotations")


def _grad_check_strict(g, gref, keys=GRAD_KEYS, label=None):
    """The gradient bar with NO exemption: every tensor of `keys`, every Gaussian, every element --
      |got - ref| <= GRAD_MAX_OF_SCALE x max|ref tensor|, and at most GRAD_NOISE_FRAC of the elements outside
      1e-4 x max(|ref|, 1e-2 x max|ref tensor|)
    (the constants of _grad_check; no `fragile` branch, no `touched` branch).  For gradients of a dL_dpix that is ZERO on the oracle's near-threshold pixels (O.fragile_pixels of the state the oracle
    walks): every term a pixel contributes to any gradient is linear in that pixel's dL_dpix, so a decision the GPU's v_exp_f32
    takes the other way there contributes nothing on either side, and nobody needs a wider bar (tests/test_oracle_checks.py:
    the mask is <= 2.2 % of a scene's blended pixels and un-grades no more than 3.2 % of its Gaussians).  The oracle's own fp32
    against fp64 build under the mask: <= 3.2e-5 of scale on every scene it can be measured on.
    Prints the figures (with `label`) BEFORE asserting; returns {name: (worst error / scale, fraction outside)}."""
    report, failed = {}, []
    for k in keys:
        ref = gref[k]
        if ref.size == 0:
            assert g[k].size == 0, k
            continue
        b = ref.astype(np.float64).reshape(ref.shape[0], -1)
        a = g[k].astype(np.float64).reshape(b.shape)
        scale = float(np.abs(b).max())
        if scale == 0.0:
            report[k] = (float(np.abs(a).max()), 0.0)
            if report[k][0] != 0.0:
                failed.append(k)
            continue
        err = np.abs(a - b)
        report[k] = (float(err.max()) / scale, float((err > 1e-4 * np.maximum(np.abs(b), 1e-2 * scale)).mean()))
        if not (report[k][0] <= GRAD_MAX_OF_SCALE and report[k][1] <= GRAD_NOISE_FRAC):
            failed.append(k)
    if label is not None:
        print("STRICT", label, "exempt 0", {k: (f"{v[0]:.1e}", f"{v[1]:.1e}") for k, v in report.items()})
    assert not failed, (label, {k: report[k] for k in failed})
    return report


def _exempt_share(gref, which):
    """(exempt, graded): the Gaussians with any gradient from the blend (the oracle's accumulators), and those of them that
    _grad_check (`fragile`) / _grad_check7 (`touched`) hold to a wider bar than 1e-4."""
    graded = np.abs(gref["acc"]).max(axis=1) > 0 if gref["acc"].size else np.zeros(0, bool)
    return int((gref[which] & graded).sum()), int(graded.sum())


def _strict_masked_backward(s, fw, ref_state, dpix, label, gref_unmasked=None):
    """The second backward of the 3-channel oracle tests: dL_dpix zeroed on the near-threshold pixels of the state the oracle
    backward walks (the GPU's n_contrib / final_T on the reference's lists), the same masked dL_dpix to both sides, every
    Gaussian at the strict bar.  Returns the line it prints as a dict."""
    from tests import gpu_util as G
    mask = O.fragile_pixels(s, ref_state)
    dpix_m = dpix * ~mask
    assert dpix_m.dtype == np.float32
    report = _grad_check_strict(G.run_backward(s, fw, dpix_m), O.backward(s, ref_state, dpix_m), label=label)
    line = {"masked_pixels": int(mask.sum()), "blended_pixels": int((ref_state["n_contrib"] > 0).sum()), "pixels": int(mask.size),
            "strict_worst_of_scale": {k: v[0] for k, v in report.items()}}
    if gref_unmasked is not None:
        line["exempt_in_grad_check"], line["graded"] = _exempt_share(gref_unmasked, "fragile")
    print("STRICT_SHARES", label, {k: v for k, v in line.items() if k != "strict_worst_of_scale"})
    return line


def _grad_percentiles(g, gref):
    """Per-element error distribution of every gradient against the oracle (the measured bar):
    err / max|ref tensor| and the RELATIVE error err / max(|ref|, 1e-3 max|ref tensor|) -- an element that cancels to ~0 has
    no relative error of its own -- at p50 / p99 / p99.9 / max, over the Gaussians the oracle does not mark fragile and over all."""
    fragile = gref["fragile"]
    P = fragile.shape[0]
    out = {}
    for k in GRAD_KEYS:
        if gref[k].size == 0:
            continue
        b = gref[k].astype(np.float64).reshape(P, -1)
        a = g[k].astype(np.float64).reshape(b.shape)
        scale = float(np.abs(b).max())
        if scale == 0.0:
            continue
        nz = np.abs(b).max(axis=1) > 0            # Gaussians with a gradient at all (culled ones are exact zeros on both sides)
        row = {}
        for tag, sel in (("solid", nz & ~fragile), ("all", nz)):
            if not sel.any():
                continue
            err = np.abs(a[sel] - b[sel]).reshape(-1)
            rel = err / np.maximum(np.abs(b[sel]).reshape(-1), 1e-3 * scale)
            q = lambda v: [float(x) for x in np.percentile(v, [50, 99, 99.9, 100])]
            row[tag] = {"of_scale": q(err / scale), "relative": q(rel), "n": int(err.size)}
        out[k] = row
    return out


@pytest.mark.parametrize("name", [n for n in ALL if n not in ("all_culled",)])
def test_backward_matches_oracle(name):
    from tests import gpu_util as G
    s, ref, fw, got = _check_forward(name)
    rng = np.random.default_rng(123)
    dpix = rng.normal(size=(3, s["H"], s["W"])).astype(np.float32)
    # evaluate the oracle backward on the GPU's own forward state (n_contrib / final_T), so a forward threshold
    # flip does not masquerade as a backward error
    ref_state = dict(ref)
    ref_state["n_contrib"] = got["n_contrib"].copy()
    ref_state["final_T"] = got["final_T"].copy()
    gref = O.backward(s, ref_state, dpix)
    g = G.run_backward(s, fw, dpix)
    _grad_check(g, gref, ref)
    _strict_masked_backward(s, fw, ref_state, dpix, name, gref)
    # culled Gaussians receive exactly zero everywhere (trap 4)
    inv = ref["radii"] == 0
    for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacity", "dL_dcolors"):
        assert (g[k].reshape(len(inv), -1)[inv] == 0).all()


@pytest.mark.parametrize("name", ALL)
def test_tile_cull_changes_no_output(name):
    """Tile culling on (the default) against off (the reference's tile lists): fewer instances, and bit-identical image,
    radii, transmittance and gradients -- every dropped (Gaussian, tile) instance is one that no pixel of the tile
    blends (alpha < 1/255 on all 256 pixels, checked here in float64 from the preprocessed 2D state)."""
    from tests import gpu_util as G
    s = _scene(name)
    fw_on, fw_off = _forward(s, True), _forward(s, False)
    on, off = G.intermediates(s, fw_on), G.intermediates(s, fw_off)
    assert on["status"][1] == 0 and off["status"][1] == 0
    assert on["num_rendered"] <= off["num_rendered"]
    if name in ("strands", "strands_precomp", "sh0"):
        assert on["num_rendered"] < off["num_rendered"]
    np.testing.assert_array_equal(on["radii"], off["radii"])
    _assert_same_image(on["out_color"], off["out_color"], off["ranges"])
    _assert_same_image(on["final_T"], off["final_T"], off["ranges"])
    if off["num_rendered"] == 0:
        return
    assert (on["tiles_touched"] <= off["tiles_touched"]).all()
    # ---- the kept list of every tile is the reference's list minus dropped entries, in the same order; dropped
    # entries cannot pass the alpha test anywhere in the tile
    W, H = s["W"], s["H"]
    gx = (W + 15) // 16
    xy, co = off["means2D"].astype(np.float64), off["conic_opacity"].astype(np.float64)
    py, px = np.mgrid[0:16, 0:16]
    worst = 0.0
    for t in range(len(off["ranges"])):
        a0, a1 = off["ranges"][t]
        b0, b1 = on["ranges"][t]
        full, kept = off["point_list"][a0:a1], on["point_list"][b0:b1]
        keep = np.isin(full, kept)
        np.testing.assert_array_equal(full[keep], kept)
        if keep.all():
            continue
        ids = full[~keep]
        dx = xy[ids, 0, None, None] - ((t % gx) * 16 + px)[None]
        dy = xy[ids, 1, None, None] - ((t // gx) * 16 + py)[None]
        power = -0.5 * (co[ids, 0, None, None] * dx * dx + co[ids, 2, None, None] * dy * dy) - co[ids, 1, None, None] * dx * dy
        alpha = np.where(power > 0, 0.0, co[ids, 3, None, None] * np.exp(np.minimum(power, 0)))
        worst = max(worst, float(alpha.max()))
    assert worst < 1.0 / 255.0, worst
    if name == "all_culled":
        return
    dpix = np.random.default_rng(77).normal(size=(3, H, W)).astype(np.float32)
    g_on, g_off = G.run_backward(s, fw_on, dpix), G.run_backward(s, fw_off, dpix)
    if not _long_tile_pixels(off["ranges"], W, H).any():
        # Bit for bit -- except where the per-Gaussian sum of the instance rows is taken by the whole wavefront (round 6,
        # hgs_stream_rows: wavefronts of 64 consecutive Gaussians one of which has more than HGS_PPB_LIGHT_MAX = 32 instances):
        # there a Gaussian's rows are added 16 at a time as they fall into the run's chunks, and dropping instances moves them
        # (the same terms, associated differently: rounding).
        P = len(on["tiles_touched"])
        pad = (-P) % 64
        wave_max = lambda n: np.repeat(np.concatenate([n, np.zeros(pad, n.dtype)]).reshape(-1, 64).max(1), 64)[:P]
        streamed = (wave_max(on["tiles_touched"]) > 32) | (wave_max(off["tiles_touched"]) > 32)
        for k in g_on:
            if g_off[k].size == 0:
                assert g_on[k].size == 0
                continue
            a, b = g_on[k].reshape(P, -1), g_off[k].reshape(P, -1)
            np.testing.assert_array_equal(a[~streamed].view(np.uint32), b[~streamed].view(np.uint32), err_msg=k)
            scale = float(np.abs(b).max())
            assert float(np.abs(a.astype(np.float64) - b).max()) <= 2e-5 * max(scale, 1e-30), k
    else:   # split lists: the same terms, transmittance products associated per segment
        for k in g_on:
            if g_off[k].size == 0:      # (dL_dsh of a pass with precomputed colours: nothing to compare)
                assert g_on[k].size == 0
                continue
            scale = float(np.abs(g_off[k]).max())
            assert float(np.abs(g_on[k].astype(np.float64) - g_off[k]).max()) <= 2e-5 * max(scale, 1e-30), k


def test_backward_is_bitwise_reproducible():
    from tests import gpu_util as G
    s = _scene("strands")
    fw = G.run_forward(s)
    dpix = np.random.default_rng(5).normal(size=(3, s["H"], s["W"])).astype(np.float32)
    g1 = G.run_backward(s, fw, dpix)
    g2 = G.run_backward(s, fw, dpix)
    for k in g1:
        np.testing.assert_array_equal(g1[k].view(np.uint32), g2[k].view(np.uint32), err_msg=k)


def test_wait_timeout_word_is_not_silent():
    """HGS_WAIT_TIMED_OUT (include/hgs.h): a pass whose workgroups gave up a bounded inter-workgroup wait raises the
    caller's sticky maximum to 0xFFFFFFFF; the host's next validation turns that into an error, not into a capacity."""
    import torch
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C as raster
    from tests import gpu_util as G
    cap_at_entry = raster.capacity()
    raster.set_async(True)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        s = _scene("sh0")
        G.run_forward(s)                    # (learns a capacity if there is none)
        G.run_forward(s)                    # a capacity-mode pass: pending until the next check
        word = raster._max_rendered(dev)
        word.fill_(-1)                      # int32 -1 == 0xFFFFFFFF, what hgs_wait_parts leaves behind
        cap_before = raster.capacity()
        with pytest.raises(rt.HgsError, match="inter-workgroup wait"):
            raster.check_async()
        assert raster.capacity() == cap_before and int(word.item()) == 0
        assert raster.check_async() == []   # the marks went with the error
    finally:
        raster.set_async(False)
        raster.reset_capacity(cap_at_entry)


def test_capacity_overflow_gives_zero_gradients_not_garbage(monkeypatch):
    """A pass whose binning capacity is too small (capacity mode) drops instances: it is flagged (status[1], the host
    raises HgsCapacityOverflow at its next check) and its backward must return EXACTLY ZERO for every gradient -- never
    rows of the uninitialised scratch (poisoned with NaN here), whatever a graph replay does with them before the host
    looks."""
    import torch
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    monkeypatch.setenv("HGS_POISON_SCRATCH", "1")
    # (both forms of the blend kernels' records: a lazy pass builds a record THROUGH its sorted key -- the keys of a void pass may
    # never have been written, so its lists must read as empty; round 6's first build followed a stray id out of the buffer)
    was = _C.set_lazy_records(None)
    try:
        for name, lazy in (("strands", None), ("dense_long_lists", None), ("strands", True), ("dense_long_lists", True),
                           ("dense_long_lists", False)):
            _C.set_lazy_records(lazy)
            s = _scene(name)
            full = G.run_forward(s)
            dpix = np.random.default_rng(4).normal(size=(3, s["H"], s["W"])).astype(np.float32)
            try:
                _C.set_async(True)
                _C.reset_capacity(max(64, full["R"] // 3))
                fw = G.run_forward(s)
                assert fw["R"] == _C.capacity() and G.intermediates(s, fw)["status"][1] == 1
                g = G.run_backward(s, fw, dpix)
                for k, v in g.items():
                    assert np.isfinite(v).all() and (v == 0).all(), k
                with pytest.raises(_C.HgsCapacityOverflow):
                    _C.check_async()
                assert _C.capacity() > full["R"]
            finally:
                _C.set_async(False)
                _C.reset_capacity(0)
            # and the same scene right after, with enough capacity, is unaffected
            g2 = G.run_backward(s, full, dpix)
            assert any((v != 0).any() for v in g2.values())
    finally:
        _C.set_lazy_records(was)


def test_empty_inputs():
    import torch
    from diff_gaussian_rasterization import _C
    s = scenes.random_scene(P=10, W=40, H=24, seed=1, bg=(0.25, 0.5, 0.75))
    from tests.gpu_util import to_dev
    e = torch.empty(0, device="cuda")
    R, color, radii, *_ = _C.rasterize_gaussians(to_dev(s["bg"]), torch.empty((0, 3), device="cuda"), e, e, e, e, 1.0, e,
                                                 to_dev(s["viewmatrix"]), to_dev(s["projmatrix"]), s["tanfovx"],
                                                 s["tanfovy"], s["H"], s["W"], e, 0, to_dev(s["campos"]), False, False)
    assert R == 0 and radii.numel() == 0
    exp = np.broadcast_to(np.array(s["bg"], np.float32)[:, None, None], (3, s["H"], s["W"]))
    np.testing.assert_array_equal(color.cpu().numpy(), exp)


def test_mark_visible():
    import torch
    from diff_gaussian_rasterization import _C
    from tests.gpu_util import to_dev
    s = scenes.random_scene(P=2000, W=64, H=64, seed=21, behind_frac=0.3)
    got = _C.mark_visible(to_dev(s["means3D"]), to_dev(s["viewmatrix"]), to_dev(s["projmatrix"])).cpu().numpy()
    np.testing.assert_array_equal(got, O.mark_visible(s["means3D"], s["viewmatrix"]))
    assert 0 < got.sum() < len(got)


@pytest.mark.parametrize("name", ["sh0", "strands", "dense_long_lists", "tiny_image", "many_tiles", "c3_full_size"])
def test_capacity_mode_binning_equals_blocking_mode(name):
    """Capacity (async) mode: hgs_forward_preprocess launches no scan, the scatter kernel scans the tile counts itself
    ("fused scan"; many_tiles exceeds its LDS and c3_full_size -- 200 k Gaussians -- the Gaussian count up to which that
    pays: both keep the scan launch).  Ranges, sorted lists, image and the reported instance count have to be what the
    blocking mode produces."""
    import torch
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    s = _workload_scene("c3") if name == "c3_full_size" else _scene(name)
    ref_fw = G.run_forward(s)
    ref = G.intermediates(s, ref_fw)
    try:
        _C.reset_capacity(0)                   # (a capacity learnt on another scene would be kept)
        _C.set_async(True)
        G.run_forward(s)                       # the first pass of the mode learns the capacity (it blocks)
        fw = G.run_forward(s)                  # capacity mode
        worst = _C.check_async()
        assert worst == [ref["num_rendered"]]
        got = G.intermediates(s, fw)           # (the pass returns its CAPACITY: the buffer is carved for that many)
    finally:
        _C.set_async(False)
    n = ref["num_rendered"]
    assert fw["R"] >= n and got["status"][0] == n and got["status"][1] == 0
    for k in ("tiles_touched", "point_offsets", "n_contrib"):
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    # Where the scatter kernel allocates the tiles' segments itself (round 5: one atomic per wavefront of 64 tiles instead of
    # a scan in tile order) the segments sit in the order those atomics arrived: compared tile by tile -- every tile's range
    # length, list and sorted keys are the blocking mode's, the segments partition [0, n).  (many_tiles and every frame of
    # more than 8192 tiles keep the scan kernel, i.e. the reference's layout, which in_tile_order leaves as it is.)
    ranges, point_list, keys_sorted = G.in_tile_order(got, n)
    np.testing.assert_array_equal(ranges, ref["ranges"], err_msg="ranges")
    np.testing.assert_array_equal(point_list, ref["point_list"], err_msg="point_list")
    np.testing.assert_array_equal(keys_sorted, ref["keys_sorted"], err_msg="keys_sorted")
    np.testing.assert_array_equal(got["out_color"].view(np.uint32), ref["out_color"].view(np.uint32))
    dpix = np.random.default_rng(3).normal(size=(3, s["H"], s["W"])).astype(np.float32)
    g1, g0 = G.run_backward(s, fw, dpix), G.run_backward(s, ref_fw, dpix)
    for k in g0:
        np.testing.assert_array_equal(g1[k].view(np.uint32), g0[k].view(np.uint32), err_msg=k)


def _workload_scene(workload, view=0):
    """One view of a BASELINE.json workload (synthetic.WORKLOADS) as an oracle scene dict."""
    import math
    import torch
    from synthetic import build_workload
    model, cams, _ = build_workload(workload, device="cuda", seed=0, with_targets=False, n_views=2)
    cam = cams[view]
    with torch.no_grad():
        return dict(means3D=model.get_xyz.cpu().numpy(), opacities=model.get_opacity.cpu().numpy().reshape(-1),
                    scales=model.get_scaling.cpu().numpy(), rotations=model.get_rotation.cpu().numpy(), cov3D_precomp=None,
                    viewmatrix=cam.world_view_transform.cpu().numpy(), projmatrix=cam.full_proj_transform.cpu().numpy(),
                    campos=cam.camera_center.cpu().numpy(), bg=np.zeros(3, np.float32),
                    tanfovx=float(math.tan(cam.FoVx * 0.5)), tanfovy=float(math.tan(cam.FoVy * 0.5)), W=cam.image_width,
                    H=cam.image_height, sh_degree=model.active_sh_degree, scale_modifier=1.0,
                    shs=model.get_features.cpu().numpy(), colors_precomp=None)


# BASELINE.json configs[1..4] + north_star, each at its full size (one view; the 8-GPU part of C5 is view-parallel, every
# rank runs exactly this): C2 = Stage-I cloud 50k @ 800x800 (tile lists of 1000-3000 entries: the multi-chunk sort and the
# segment-parallel blend), C3 = 200k strands, C4 = 1M curly strands (2.5M instances), C5 = 500k strands, all @ 1080p.
@pytest.mark.parametrize("workload", ["north_star", "c2", "c3", "c4", "c5"])
def test_full_size_forward_and_backward_against_oracle(workload):
    """The library's default path (tile culling on) against the CPU oracle at the BASELINE.json sizes: image to 2e-5
    absolute (PSNR > 110 dB); with culling off `ranges`, `point_list` and the sorted keys bit-exact (the reference's
    lists, CR/rasterizer_impl.cu:300-317); every gradient to the bar of _grad_check (CR/backward_distwar.cu:855-1014), and a
    second backward with dL_dpix zeroed on the oracle's near-threshold pixels at the strict bar (_grad_check_strict: no
    Gaussian exempt)."""
    import math
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    s = _workload_scene(workload)
    ref = O.forward(s)
    fw = _forward(s, True)                                   # what render() and the training step run: culling on
    img = fw["color"].cpu().numpy()
    err = np.abs(img - ref["out_color"])
    mse = float(np.mean(err.astype(np.float64) ** 2))
    flips = err > 1e-4                                       # (a threshold flip moves a pixel by <= alpha ~ 1/255)
    assert int(flips.any(0).sum()) <= max(2, err[0].size // 20000), int(flips.any(0).sum())
    assert np.median(err) <= 1e-6 and float(err[~flips].max()) <= 1e-4 and (mse == 0 or 10 * math.log10(1.0 / mse) > 110.0), (
        float(err.max()), mse)
    assert fw["R"] <= ref["num_rendered"]                    # fewer instances than the reference's lists ...
    np.testing.assert_array_equal(fw["radii"].cpu().numpy(), ref["radii"])   # ... same radii
    # the reference's lists (culling off): binning bit-exact at size; its per-pixel state feeds the oracle backward
    # (bit-identical image and transmittance, list positions in the reference's numbering)
    was = _C.set_tile_cull(False)
    try:
        got_ref_lists = G.intermediates(s, G.run_forward(s))
    finally:
        _C.set_tile_cull(was)
    assert got_ref_lists["status"][1] == 0 and got_ref_lists["num_rendered"] == ref["num_rendered"]
    for k in ("ranges", "point_list", "keys_sorted", "tiles_touched", "point_offsets"):
        np.testing.assert_array_equal(got_ref_lists[k], ref[k], err_msg=k)
    _assert_same_image(got_ref_lists["out_color"], img, got_ref_lists["ranges"])
    ref["n_contrib"], ref["final_T"] = got_ref_lists["n_contrib"], got_ref_lists["final_T"]
    dpix = np.random.default_rng(9).normal(size=(3, s["H"], s["W"])).astype(np.float32)
    gref = O.backward(s, ref, dpix)
    g = G.run_backward(s, fw, dpix)
    report = _grad_check(g, gref, ref)
    print(workload, {k: (f"{v[0]:.1e}", f"{v[1]:.1e}", v[2]) for k, v in report.items()})
    strict = _strict_masked_backward(s, fw, ref, dpix, workload, gref)
    # the measured error distribution, every tensor (dL_dcov3D included), for DESIGN.md's table: printed, and written where a
    # collecting run asks for it (HGS_GRAD_REPORT_DIR)
    pct = _grad_percentiles(g, gref)
    print("GRAD_PERCENTILES", workload, {k: {t: ["%.1e" % x for x in v[t]["relative"]] for t in v} for k, v in pct.items()})
    if os.environ.get("HGS_GRAD_REPORT_DIR"):
        import json
        with open(os.path.join(os.environ["HGS_GRAD_REPORT_DIR"], f"grad_parity_{workload}.json"), "w") as fh:
            json.dump({"workload": workload, "fragile_gaussians": int(gref["fragile"].sum()), "gaussians": int(gref["fragile"].shape[0]),
                       "percentiles_p50_p99_p99.9_max": pct, "strict_masked": strict}, fh, indent=1)


# ---------------------------------------------------------------------------------------------------------------------
# The kernels the training step runs -- blend_fwd_kernel<7>, blend_bwd_kernel<7, BLACK>, preprocess_bwd_kernel<DC_ONLY, 0/1/2>
# -- against the oracle at every BASELINE size.  The reference renders three times per iteration (SH RGB: train.py:146;
# colors_precomp = mask x 3: loss/losses.py:246-249; colors_precomp = orientation: :311-312) and autograd sums the three
# backward passes (CR/backward_distwar.cu:855-1014); the densification statistics read the screen-space gradient of the RGB
# pass alone (train.py:170).  So the oracle is called three times on the same scene and its gradients are summed.
BG7_NONZERO = np.array([0.1, 0.2, 0.3, 0.05, 0.2, -0.1, 0.3], np.float32)


def _workload_scene7(workload, view=0):
    """_workload_scene + the four extra per-Gaussian channels of the single pass (mask, world-space direction) and the model."""
    import torch
    from synthetic import build_workload
    model, cams, _ = build_workload(workload, device="cuda", seed=0, with_targets=False, n_views=2)
    s = _scene_of(model, cams[view])
    with torch.no_grad():
        extra = torch.cat((model.get_mask, model.get_orientation), dim=1).contiguous()
    return s, extra, model, cams[view]


def _scene_of(model, cam):
    import math
    import torch
    with torch.no_grad():
        return dict(means3D=model.get_xyz.cpu().numpy(), opacities=model.get_opacity.cpu().numpy().reshape(-1),
                    scales=model.get_scaling.cpu().numpy(), rotations=model.get_rotation.cpu().numpy(), cov3D_precomp=None,
                    viewmatrix=cam.world_view_transform.cpu().numpy(), projmatrix=cam.full_proj_transform.cpu().numpy(),
                    campos=cam.camera_center.cpu().numpy(), bg=np.zeros(3, np.float32),
                    tanfovx=float(math.tan(cam.FoVx * 0.5)), tanfovy=float(math.tan(cam.FoVy * 0.5)), W=cam.image_width,
                    H=cam.image_height, sh_degree=model.active_sh_degree, scale_modifier=1.0,
                    shs=model.get_features.cpu().numpy(), colors_precomp=None)


def _forward7(s, extra, bg7, cull):
    """hgs_forward_render (n_extra 4) through the drop-in module; bg7: a [7] array.  Colour source (SH or colors_precomp),
    covariance source (scales + rotations or cov3D_precomp), scale_modifier, SH degree and M are the scene dict's."""
    import torch
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    d = G.to_dev
    was = _C.set_tile_cull(cull)
    try:
        R, planes, radii, geom, binning, img = _C.rasterize_gaussians_multi(
            d(bg7), d(s["means3D"]), d(s["colors_precomp"]), extra, d(s["opacities"]).reshape(-1, 1), d(s["scales"]),
            d(s["rotations"]), float(s["scale_modifier"]), d(s["cov3D_precomp"]), d(s["viewmatrix"]), d(s["projmatrix"]), float(s["tanfovx"]), float(s["tanfovy"]), int(s["H"]), int(s["W"]),
            d(s["shs"]), int(s["sh_degree"]), d(s["campos"]), False, False)
    finally:
        _C.set_tile_cull(was)
    torch.cuda.synchronize()
    W, H = s["W"], s["H"]
    T = ((W + 15) // 16) * ((H + 15) // 16)
    im = rt_layout_image(W, H)
    return dict(R=R, planes=planes, radii=radii, geom=geom, binning=binning, img=img,
                final_T=G._view(img, im["final_T"], W * H, np.float32).reshape(H, W),
                n_contrib=G._view(img, im["n_contrib"], W * H, np.uint32).reshape(H, W),
                ranges=G._view(img, im["ranges"], 2 * T, np.uint32).reshape(T, 2),
                status=G._view(img, im["status"], 16, np.uint32))


def rt_layout_image(W, H):
    import hgs_runtime as rt
    return rt.layout("image", W, H)


def _oracle_three_passes(s, extra_np, bg7):
    """The reference's three render() calls as three oracle forwards on the same scene: (rgb, mask, orientation) results.
    The RGB pass keeps the scene's own colour source (SH of its degree and M, or colors_precomp); all three keep its covariance
    source and scale_modifier."""
    s_rgb = dict(s, bg=bg7[0:3])
    s_mask = dict(s, shs=None, sh_degree=0, colors_precomp=np.repeat(extra_np[:, 0:1], 3, axis=1), bg=np.repeat(bg7[3:4], 3))
    s_ori = dict(s, shs=None, sh_degree=0, colors_precomp=np.ascontiguousarray(extra_np[:, 1:4]), bg=bg7[4:7])
    return [(sc, O.forward(sc)) for sc in (s_rgb, s_mask, s_ori)]


def _check_image7(planes, refs, npix):
    """Seven planes against the three oracle images: <= 1e-4 (x max(|ref|, 1)) except on the few pixels a threshold flip moves."""
    ref7 = np.concatenate([refs[0][1]["out_color"], refs[1][1]["out_color"][0:1], refs[2][1]["out_color"]], axis=0)
    err = np.abs(planes - ref7)
    bad = err > 1e-4 * np.maximum(np.abs(ref7), 1.0)
    nbad = int(bad.any(0).sum())
    assert nbad <= max(2, npix // 20000), f"{nbad} pixels outside 1e-4"
    assert float(err.max()) <= 2e-2 and float(np.median(err)) <= 1e-6
    return float(err[~bad].max()) if (~bad).any() else 0.0


def _fragile_pixels7(refs, state):
    """O.fragile_pixels of the state the three oracle backwards walk (the decisions do not depend on the colours: one mask)."""
    st = dict(refs[0][1])
    st["n_contrib"], st["final_T"] = state["n_contrib"].copy(), state["final_T"].copy()
    return O.fragile_pixels(refs[0][0], st)


def _oracle_backward7(refs, state, dplanes):
    """Sum of the three oracle backward passes (what autograd accumulates over the reference's three render() calls) on the
    given per-pixel state (n_contrib / final_T in the reference's list numbering).  Returns the summed gradient dict in the
    key set of GRAD_KEYS (+ dL_dextra [P,4], the RGB pass's own dL_dmeans2D as dL_dmeans2D_rgb, fragile = union)."""
    out = None
    for k, ((sc, fw), dp) in enumerate(zip(refs, (dplanes[0:3], np.stack([dplanes[3], 0 * dplanes[3], 0 * dplanes[3]]), dplanes[4:7]))):
        st = dict(fw)
        st["n_contrib"], st["final_T"] = state["n_contrib"].copy(), state["final_T"].copy()
        g = O.backward(sc, st, np.ascontiguousarray(dp, dtype=np.float32))
        if k == 0:
            out = {n: g[n].astype(np.float64) for n in GRAD_KEYS}
            out["dL_dmeans2D_rgb"] = g["dL_dmeans2D"].astype(np.float64)
            out["fragile"] = g["fragile"].copy()
            out["touched"] = g["touched"].copy()
            out["acc"] = g["acc"]          # (which Gaussians the blend grades at all: the same set in all three passes' walks)
            P = g["fragile"].shape[0]
            out["dL_dextra"] = np.zeros((P, 4))
        else:
            for n in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"):
                out[n] = out[n] + g[n]
            out["fragile"] |= g["fragile"]
            out["touched"] |= g["touched"]
            if k == 1:
                out["dL_dextra"][:, 0] = g["dL_dcolors"][:, 0]
            else:
                out["dL_dextra"][:, 1:4] = g["dL_dcolors"]
    return out


def _backward7(s, extra, fw, bg7, dplanes):
    import torch
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    d = G.to_dev
    dp = d(dplanes)
    out = _C.rasterize_gaussians_multi_backward(
        None if bg7 is None else d(bg7), d(s["means3D"]), fw["radii"], d(s["colors_precomp"]), d(s["scales"]), d(s["rotations"]),
        float(s["scale_modifier"]), d(s["cov3D_precomp"]), d(s["viewmatrix"]), d(s["projmatrix"]), float(s["tanfovx"]), float(s["tanfovy"]), [dp[k] for k in range(7)], d(s["shs"]),
        int(s["sh_degree"]), d(s["campos"]), fw["geom"], fw["R"], fw["binning"], fw["img"], False)
    torch.cuda.synchronize()
    names = ["dL_dmeans2D_rgb", "dL_dcolors", "dL_dextra", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
             "dL_drotations"]
    return {n: t.cpu().numpy() for n, t in zip(names, out)}


TOUCHED_MAX_OF_SCALE = 4e-3   # one decision taken the other way moves what its pixel contributes to the Gaussians it blends by <= alpha ~ 1/255


def _grad_check7(g, gref, fwd_ref, report_name=None):
    """_grad_check's bar for the tensors the 7-channel backward returns (the summed geometry gradients, dL_dcolors / dL_dsh of the
    RGB pass, dL_dextra of the other two, the RGB-only screen-space gradient), with the exemption enumerated one step further:
      every element of a Gaussian that shares NO pixel with a near-threshold decision: 1e-4 of the tensor's scale, and the
          element-wise bound 1e-4 x max(|ref|, 1e-2 scale) on all but 0.2 %;
      `touched` Gaussians (oracle/raster_oracle.c: blended at a pixel where some entry's alpha lies within 1e-4 of 1/255 -- if the
          GPU's v_exp_f32 takes that decision the other way, the transmittance in front of / the colour behind every entry of
          that pixel moves by that alpha): 4e-3 of scale;
      `fragile` Gaussians (the ones whose own decision it is): 2e-2 of scale.
    Both sets are bounded in number by what the geometry predicts (_expected_fragile; touched <= fragile x the longest walk)."""
    fragile, touched = gref["fragile"], gref["touched"]
    P = fragile.shape[0]
    expected = _expected_fragile(fwd_ref)
    assert int(fragile.sum()) <= 3.0 * expected + 8
    assert int(touched.sum()) <= int(fragile.sum()) * max(1, int(fwd_ref["n_contrib"].max()))
    report = {}
    for k in ("dL_dmeans2D_rgb", "dL_dcolors", "dL_dextra", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
              "dL_drotations"):
        if k not in g or gref[k].size == 0:
            continue
        b = gref[k].astype(np.float64).reshape(P, -1)
        a = g[k].astype(np.float64).reshape(b.shape)
        scale = float(np.abs(b).max())
        if scale == 0.0:
            assert np.abs(a).max() == 0.0, k
            continue
        err = np.abs(a - b)
        solid = err[~touched]
        worst = float(solid.max()) / scale if solid.size else 0.0
        frac = float((solid > 1e-4 * np.maximum(np.abs(b[~touched]), 1e-2 * scale)).mean()) if solid.size else 0.0
        near = touched & ~fragile
        worst_touched = float(err[near].max()) / scale if near.any() else 0.0
        worst_fragile = float(err[fragile].max()) / scale if fragile.any() else 0.0
        report[k] = (worst, frac, int(fragile.sum()), int(touched.sum()), worst_touched, worst_fragile)
        assert worst <= GRAD_MAX_OF_SCALE, (k, report[k])
        assert frac <= GRAD_NOISE_FRAC, (k, report[k])
        assert worst_touched <= TOUCHED_MAX_OF_SCALE, (k, report[k])
        assert worst_fragile <= FRAGILE_MAX_OF_SCALE, (k, report[k])
    return report


@pytest.mark.parametrize("workload", ["north_star", "c2", "c3", "c4", "c5"])
def test_seven_channel_pass_against_oracle(workload):
    """hgs_forward_render + hgs_backward with n_extra 4 (the 7-channel instantiations bench.py times) against three oracle passes
    at the BASELINE sizes: seven image planes, n_contrib / final_T, every gradient as the sum of the three oracle backwards at
    _grad_check's bar, the RGB-only dL_dmeans2D (what densification reads) as the RGB pass's alone.  Twice: bg = NULL (the
    black-background specialisation blend_bwd_kernel<7, true>: the training step's) and a non-zero 7-channel background.  Each
    time a second backward with dL_dpix zeroed on the oracle's near-threshold pixels holds every Gaussian to the strict bar."""
    import torch
    s, extra, _, _ = _workload_scene7(workload)
    extra_np = extra.cpu().numpy()
    npix = s["W"] * s["H"]
    rng = np.random.default_rng(17)
    dplanes = rng.normal(size=(7, s["H"], s["W"])).astype(np.float32)
    for tag, bg7 in (("black", np.zeros(7, np.float32)), ("bg7", BG7_NONZERO)):
        refs = _oracle_three_passes(s, extra_np, bg7)
        # the reference's three passes share one geometry: same lists, same per-pixel walk
        for _, r in refs[1:]:
            np.testing.assert_array_equal(r["n_contrib"], refs[0][1]["n_contrib"])
            np.testing.assert_array_equal(r["point_list"], refs[0][1]["point_list"])
        fw = _forward7(s, extra, bg7, True)                       # the training step's form: tile culling on
        fw_ref_lists = _forward7(s, extra, bg7, False)            # the reference's lists: per-pixel state in its numbering
        assert fw["status"][1] == 0 and fw["status"][8] == 0 and fw_ref_lists["status"][1] == 0
        planes = fw["planes"].cpu().numpy()
        worst_img = _check_image7(planes, refs, npix)
        _assert_same_image(fw_ref_lists["planes"].cpu().numpy(), planes, fw_ref_lists["ranges"])
        np.testing.assert_array_equal(fw["radii"].cpu().numpy(), refs[0][1]["radii"])
        ref0 = refs[0][1]
        flips = int((fw_ref_lists["n_contrib"] != ref0["n_contrib"]).sum())
        assert flips <= max(2, npix // 2000), f"n_contrib differs on {flips}/{npix} pixels"
        same = fw_ref_lists["n_contrib"] == ref0["n_contrib"]
        # (an entry in the MIDDLE of a pixel's walk whose alpha sits within rounding of 1/255 is blended by one side only: the
        # last contributor stays, the transmittance moves by that alpha -- counted like the image's threshold flips)
        dT = np.abs(fw_ref_lists["final_T"] - ref0["final_T"])[same]
        assert int((dT > 1e-4).sum()) <= max(2, npix // 20000) and float(dT.max(initial=0.0)) <= 5e-3, (int((dT > 1e-4).sum()), float(dT.max()))
        gref = _oracle_backward7(refs, fw_ref_lists, dplanes)
        g = _backward7(s, extra, fw, None if tag == "black" else bg7, dplanes)
        report = _grad_check7(g, gref, ref0)
        mask = _fragile_pixels7(refs, fw_ref_lists)
        dmasked = dplanes * ~mask
        gref_m = _oracle_backward7(refs, fw_ref_lists, dmasked)
        _grad_check_strict(_backward7(s, extra, fw, None if tag == "black" else bg7, dmasked), gref_m, KEYS7, f"SEVEN {workload} {tag}")
        print("STRICT_SHARES", f"SEVEN {workload} {tag}", dict(masked_pixels=int(mask.sum()), pixels=npix,
              exempt_in_grad_check7=_exempt_share(gref, "touched"), exempt_in_grad_check=_exempt_share(gref, "fragile")))
        if tag == "black":
            # the same pass with the per-Gaussian row sums taken by row_reduce_kernel (include/hgs.h HGS_ROWS_REDUCE: what
            # a pass with many instances per Gaussian runs by default) and with the sums inside the per-Gaussian launch
            from diff_gaussian_rasterization import _C
            was = _C.set_row_reduce(True)
            try:
                g_rr = _backward7(s, extra, fw, None, dplanes)
                _grad_check7(g_rr, gref, ref0)
                _grad_check_strict(_backward7(s, extra, fw, None, dmasked), gref_m, KEYS7, f"SEVEN {workload} rows_reduce")
                _C.set_row_reduce(False)
                g_in = _backward7(s, extra, fw, None, dplanes)
                _grad_check7(g_in, gref, ref0)
                _grad_check_strict(_backward7(s, extra, fw, None, dmasked), gref_m, KEYS7, f"SEVEN {workload} rows_inline")
            finally:
                _C.set_row_reduce(was)
            for k in g_rr:
                if g_in[k].size:
                    scale = float(np.abs(g_in[k]).max())
                    assert float(np.abs(g_rr[k].astype(np.float64) - g_in[k]).max()) <= 2e-5 * max(scale, 1e-30), k
        print("SEVEN", workload, tag, f"image {worst_img:.1e}", {k: (f"{v[0]:.1e}", f"{v[1]:.1e}", v[2], v[3], f"{v[4]:.1e}", f"{v[5]:.1e}") for k, v in report.items()})
        if os.environ.get("HGS_GRAD_REPORT_DIR"):
            import json
            gg = dict(g)
            gg["dL_dmeans2D"] = None
            pct = {}
            fragile, touched = gref["fragile"], gref["touched"]
            for k in report:
                b = gref[k].astype(np.float64).reshape(fragile.shape[0], -1)
                a = g[k].astype(np.float64).reshape(b.shape)
                scale = float(np.abs(b).max())
                nz = np.abs(b).max(axis=1) > 0
                row = {}
                for t2, sel in (("solid", nz & ~touched), ("touched_not_fragile", nz & touched & ~fragile), ("all", nz)):
                    if sel.any():
                        err = np.abs(a[sel] - b[sel]).reshape(-1)
                        rel = err / np.maximum(np.abs(b[sel]).reshape(-1), 1e-3 * scale)
                        q = lambda v: [float(x) for x in np.percentile(v, [50, 99, 99.9, 100])]
                        row[t2] = {"of_scale": q(err / scale), "relative": q(rel), "n": int(err.size)}
                pct[k] = row
            with open(os.path.join(os.environ["HGS_GRAD_REPORT_DIR"], f"grad_parity7_{workload}_{tag}.json"), "w") as fh:
                json.dump({"workload": workload, "pass": "7-channel, " + tag, "fragile_gaussians": int(fragile.sum()),
                           "touched_gaussians": int(touched.sum()), "gaussians": int(fragile.shape[0]), "image_max_err_outside_flips": worst_img,
                           "percentiles_p50_p99_p99.9_max": pct}, fh, indent=1)
        del fw, fw_ref_lists
        torch.cuda.empty_cache()


def _assert_bit_identical(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=f"{what}: {k}")


@pytest.mark.parametrize("name", ALL)
def test_seven_channel_variants_against_oracle(name):
    """The 7-channel pass (blend_fwd_kernel<7>, blend_bwd_kernel<7, BLACK>, preprocess_bwd_kernel<*, 0>, row_reduce_kernel) on the
    adversarial scenes, which until now met the oracle through the 3-channel entry points only: lists of ~3000 entries in 24
    segments, one tile of 140 k entries, saturation, depth ties, 17 545 tiles, a 7 x 5 image, SH degree 1-3 with M above the
    active degree, negative precomputed colours, a precomputed covariance, scale_modifier 0.6, a rotated camera, everything
    culled.  `extra` is uniform in [-1, 1].  Forward as in test_seven_channel_pass_against_oracle; backward as the sum of three
    oracle passes, once at _grad_check7's bars and once with dL_dpix zeroed on the near-threshold pixels at the strict bar, no
    Gaussian exempt -- with both row-sum forms, packed against lazy records bit for bit, and two runs bit for bit."""
    import torch
    from diff_gaussian_rasterization import _C
    s = _scene(name)
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    npix = W * H
    rng = np.random.default_rng(7000 + ALL.index(name))
    extra_np = rng.uniform(-1, 1, size=(P, 4)).astype(np.float32)
    extra = torch.from_numpy(extra_np).cuda()
    dplanes = rng.normal(size=(7, H, W)).astype(np.float32)
    for tag, bg7 in (("black", np.zeros(7, np.float32)), ("bg7", BG7_NONZERO)):
        bg_arg = None if tag == "black" else bg7
        refs = _oracle_three_passes(s, extra_np, bg7)
        ref0 = refs[0][1]
        for _, r in refs[1:]:
            np.testing.assert_array_equal(r["n_contrib"], ref0["n_contrib"])
            np.testing.assert_array_equal(r["point_list"], ref0["point_list"])
        fw = _forward7(s, extra, bg7, True)
        fw_ref_lists = _forward7(s, extra, bg7, False)
        assert fw["status"][1] == 0 and fw["status"][8] == 0 and fw_ref_lists["status"][1] == 0 and fw_ref_lists["status"][8] == 0
        planes = fw["planes"].cpu().numpy()
        worst_img = _check_image7(planes, refs, npix)
        _assert_same_image(fw_ref_lists["planes"].cpu().numpy(), planes, fw_ref_lists["ranges"])
        np.testing.assert_array_equal(fw["radii"].cpu().numpy(), ref0["radii"])
        flips = int((fw_ref_lists["n_contrib"] != ref0["n_contrib"]).sum())
        assert flips <= max(2, npix // 2000), f"n_contrib differs on {flips}/{npix} pixels"
        same = fw_ref_lists["n_contrib"] == ref0["n_contrib"]
        dT = np.abs(fw_ref_lists["final_T"] - ref0["final_T"])[same]
        assert int((dT > 1e-4).sum()) <= max(2, npix // 20000) and float(dT.max(initial=0.0)) <= 5e-3, (int((dT > 1e-4).sum()), float(dT.max()))
        g = _backward7(s, extra, fw, bg_arg, dplanes)
        if name == "all_culled":
            # nothing on screen: the planes are the background's bits and every gradient, dL_dextra included, is exactly zero
            assert fw["R"] == 0 and fw_ref_lists["R"] == 0
            np.testing.assert_array_equal(planes, np.broadcast_to(bg7[:, None, None], planes.shape))
            for k, v in g.items():
                assert v.shape[0] == P and not v.any(), k
            continue
        # ---- the unmasked run at the bars of _grad_check7 (what the workload test asserts), and how many Gaussians that exempts
        gref = _oracle_backward7(refs, fw_ref_lists, dplanes)
        exempt7, graded = _exempt_share(gref, "touched")
        exempt3, _ = _exempt_share(gref, "fragile")
        mask = _fragile_pixels7(refs, fw_ref_lists)
        print("STRICT_SHARES", f"SEVEN {name} {tag}", dict(masked_pixels=int(mask.sum()), blended_pixels=int((fw_ref_lists["n_contrib"] > 0).sum()),
              pixels=npix, graded=graded, exempt_in_grad_check7=exempt7, exempt_in_grad_check=exempt3, image=f"{worst_img:.1e}"))
        report = _grad_check7(g, gref, ref0)
        print("SEVEN", name, tag, {k: (f"{v[0]:.1e}", f"{v[1]:.1e}", v[2], v[3], f"{v[4]:.1e}", f"{v[5]:.1e}") for k, v in report.items()})
        # ---- dL_dpix zeroed on the near-threshold pixels, the same planes to both sides: every Gaussian at 1e-4 of scale
        dmasked = dplanes * ~mask
        gref_m = _oracle_backward7(refs, fw_ref_lists, dmasked)
        g_m = _backward7(s, extra, fw, bg_arg, dmasked)
        _grad_check_strict(g_m, gref_m, KEYS7, f"SEVEN {name} {tag}")
        _assert_bit_identical(g_m, _backward7(s, extra, fw, bg_arg, dmasked), "second run")
        if tag != "black":
            continue
        # ---- both forms of the per-Gaussian row sums (include/hgs.h HGS_ROWS_REDUCE / HGS_ROWS_INLINE), each at the strict bar
        was = _C.set_row_reduce(True)
        try:
            _grad_check_strict(_backward7(s, extra, fw, None, dmasked), gref_m, KEYS7, f"SEVEN {name} rows_reduce")
            _C.set_row_reduce(False)
            _grad_check_strict(_backward7(s, extra, fw, None, dmasked), gref_m, KEYS7, f"SEVEN {name} rows_inline")
        finally:
            _C.set_row_reduce(was)
        # ---- packed against lazy records (include/hgs.h HGS_RECORDS_*) in the blocking mode: the same bits
        runs = {}
        was = _C.set_lazy_records(None)
        try:
            for lazy in (0, 1):
                _C.set_lazy_records(lazy)
                f2 = _forward7(s, extra, bg7, True)
                assert f2["status"][14] == lazy and f2["status"][1] == 0
                runs[lazy] = (dict(planes=f2["planes"].cpu().numpy(), final_T=f2["final_T"], n_contrib=f2["n_contrib"]),
                              _backward7(s, extra, f2, None, dmasked))
                del f2
        finally:
            _C.set_lazy_records(was)
        _assert_bit_identical(runs[0][0], runs[1][0], "lazy records, forward")
        _assert_bit_identical(runs[0][1], runs[1][1], "lazy records, backward")
        del fw, fw_ref_lists
        torch.cuda.empty_cache()


def test_seven_channel_pass_without_gaussians():
    """P = 0 with n_extra 4: the planes are the background, every gradient tensor is empty (nothing to launch over)."""
    import torch
    s = scenes.random_scene(P=10, W=40, H=24, seed=1)
    for k in ("means3D", "opacities", "scales", "rotations", "shs"):
        s[k] = s[k][:0]
    extra = torch.empty((0, 4), device="cuda")
    for bg7 in (np.zeros(7, np.float32), BG7_NONZERO):
        fw = _forward7(s, extra, bg7, True)
        assert fw["R"] == 0 and fw["radii"].numel() == 0
        planes = fw["planes"].cpu().numpy()
        np.testing.assert_array_equal(planes, np.broadcast_to(bg7[:, None, None], planes.shape))
        dplanes = np.random.default_rng(2).normal(size=(7, s["H"], s["W"])).astype(np.float32)
        for k, v in _backward7(s, extra, fw, bg7, dplanes).items():
            assert v.shape[0] == 0 and v.size == 0, k


def _chain_rule_reference(model, kind, gref):
    """The parameters' gradients by torch autograd through the model's own getters (the reference's statements,
    scene/hair_gaussian_model.py:134-201 / scene/gaussian_model.py:81-113) from the ORACLE's Gaussian-space gradients."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    chain = ((model.get_xyz * t(gref["dL_dmeans3D"])).sum() + (model.get_scaling * t(gref["dL_dscales"])).sum() +
             (model.get_rotation * t(gref["dL_drotations"])).sum() + (model.get_opacity * t(gref["dL_dopacity"])).sum() +
             (model.get_mask * t(gref["dL_dextra"][:, 0:1])).sum() + (model.get_orientation * t(gref["dL_dextra"][:, 1:4])).sum())
    if kind == "hair":
        params = [model._endpoints, model._width, model._opacity, model._mask]
    else:
        params = [model._xyz, model._scaling, model._rotation, model._opacity, model._mask]
    return [x.detach().cpu().numpy() for x in torch.autograd.grad(chain, params)]


@pytest.mark.parametrize("workload", ["north_star", "c2"])
def test_seven_channel_parameter_backward_against_oracle(workload):
    """hgs_backward_multi_params (the backward the captured iteration runs: preprocess_bwd_kernel<true, 1> for strands + the
    endpoint gather, <true, 2> for the Stage-I cloud) at BASELINE size against the oracle's three backward passes pushed
    through the model's getters by torch autograd: every parameter gradient at _grad_check's bar, dL_dsh, the RGB-only
    screen-space gradient and the densification statistics it feeds (scene/hair_gaussian_model.py:1401-1408, train.py:170).
    The `touched` rows get their wider bars in that run only: a second run with dL_dpix zeroed on the oracle's near-threshold
    pixels holds every row of every parameter gradient, dL_dsh, the screen-space gradient and the accumulated statistic to
    _grad_check_strict's bar."""
    import ctypes as C
    import torch
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from hgs_runtime.strand_step import _adjacency
    from tests import gpu_util as G
    s, extra, model, cam = _workload_scene7(workload)
    from scene.hair_gaussian_model import HairGaussianModel
    kind = "hair" if isinstance(model, HairGaussianModel) else "cloud"
    extra_np = extra.cpu().numpy()
    bg7 = np.zeros(7, np.float32)
    refs = _oracle_three_passes(s, extra_np, bg7)
    fw = _forward7(s, extra, bg7, True)
    fw_ref_lists = _forward7(s, extra, bg7, False)
    dplanes = np.random.default_rng(23).normal(size=(7, s["H"], s["W"])).astype(np.float32)
    gref = _oracle_backward7(refs, fw_ref_lists, dplanes)
    ref_params = _chain_rule_reference(model, kind, gref)
    d = G.to_dev
    P = s["means3D"].shape[0]
    f32 = dict(dtype=torch.float32, device="cuda")
    xyz, scales, rots = d(s["means3D"]), d(s["scales"]), d(s["rotations"])

    def product(planes_np):
        """One launch for the Gaussians' gradients AND the parameters' backward (+ the endpoint gather for strands)."""
        dp = d(planes_np)
        pb = rt.ParamBackward()
        g_means2D = torch.empty((P, 3), **f32)
        d_o, d_m = torch.empty((P, 1), **f32), torch.empty((P, 1), **f32)
        max_radii, accum, denom = torch.zeros(P, **f32), torch.zeros((P, 1), **f32), torch.zeros((P, 1), **f32)
        pb.extra4, pb.d_opacity_raw, pb.d_mask_raw, pb.dL_dmeans2D_rgb = rt.ptr(extra), rt.ptr(d_o), rt.ptr(d_m), rt.ptr(g_means2D)
        pb.max_radii2D, pb.grad_accum, pb.denom = rt.ptr(max_radii), rt.ptr(accum), rt.ptr(denom)
        if kind == "hair":
            E = model._endpoints.shape[0]
            pairs = model.endpoint_pairs.contiguous()
            seg_contrib, d_w, d_ep = torch.empty((P, 2, 4), **f32), torch.empty((P, 1), **f32), torch.empty((E, 3), **f32)
            pb.kind, pb.endpoints, pb.endpoint_pairs = rt.PARAMS_HAIR, rt.ptr(model._endpoints.detach()), rt.ptr(pairs)
            pb.dist_to_scale_factor = float(model.dist_to_scale_factor)
            pb.seg_contrib, pb.d_width = rt.ptr(seg_contrib), rt.ptr(d_w)
        else:
            rot_raw = model._rotation.detach().contiguous()
            g3, d_s, d_r = torch.empty((P, 3), **f32), torch.empty((P, 3), **f32), torch.empty((P, 4), **f32)
            pb.kind, pb.rotation_raw = rt.PARAMS_CLOUD, rt.ptr(rot_raw)
            pb.d_means3D, pb.d_scaling_raw, pb.d_rotation_raw = rt.ptr(g3), rt.ptr(d_s), rt.ptr(d_r)
        g_sh = _C.rasterize_gaussians_multi_backward_params(
            None, xyz, fw["radii"], scales, rots, d(s["viewmatrix"]), d(s["projmatrix"]), float(s["tanfovx"]), float(s["tanfovy"]),
            [dp[k] for k in range(7)], d(s["shs"]), int(s["sh_degree"]), d(s["campos"]), fw["geom"], fw["R"], fw["binning"], fw["img"], pb)
        if kind == "hair":
            fu = rt.StrandFusion()
            adj = _adjacency(pairs.reshape(-1), 2, E, 2)
            assert adj is not None
            fu.ep_segments, fu.n_endpoints = adj.data_ptr(), E
            rt.check(rt.lib().hgs_hair_endpoint_gather(rt.current_stream(), E, rt.ptr(seg_contrib), rt.ptr(model._endpoints.detach()),
                                                       rt.ptr(d_ep), C.byref(fu), None))
            got = [d_ep, d_w, d_o, d_m]
        else:
            got = [g3, d_s, d_r, d_o, d_m]
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in got], g_sh.cpu().numpy(), g_means2D.cpu().numpy(), accum, denom, max_radii

    got_params, g_sh, g_means2D, accum, denom, max_radii = product(dplanes)
    if kind == "hair":
        names = ["endpoints", "width", "opacity_raw", "mask_raw"]
        pr = model.endpoint_pairs.cpu().numpy()
        frag_e = np.zeros(model._endpoints.shape[0], bool)
        frag_e[pr[gref["touched"]].reshape(-1)] = True
        frag_rows = [frag_e, gref["touched"], gref["touched"], gref["touched"]]
    else:
        names = ["xyz", "scaling_raw", "rotation_raw", "opacity_raw", "mask_raw"]
        frag_rows = [gref["touched"]] * 5
    # ---- the same with dL_dpix zeroed on the near-threshold pixels: every parameter row, every Gaussian, at the strict bar
    mask = _fragile_pixels7(refs, fw_ref_lists)
    dmasked = dplanes * ~mask
    gref_m = _oracle_backward7(refs, fw_ref_lists, dmasked)
    m_params, m_sh, m_means2D, m_accum, _, _ = product(dmasked)
    want_m = dict(zip(names, _chain_rule_reference(model, kind, gref_m)), dL_dsh=gref_m["dL_dsh"], dL_dmeans2D_rgb=gref_m["dL_dmeans2D_rgb"])
    vis_m = refs[0][1]["radii"] > 0
    want_m["grad_accum"] = np.where(vis_m, np.linalg.norm(gref_m["dL_dmeans2D_rgb"][:, :2], axis=1), 0.0).reshape(-1, 1)
    got_m = dict(zip(names, m_params), dL_dsh=m_sh, dL_dmeans2D_rgb=m_means2D, grad_accum=m_accum.cpu().numpy())
    _grad_check_strict(got_m, want_m, tuple(want_m), f"SEVEN_PARAMS {workload}")
    print("STRICT_SHARES", f"SEVEN_PARAMS {workload}", dict(masked_pixels=int(mask.sum()), pixels=int(mask.size),
          exempt_in_unmasked_run=_exempt_share(gref, "touched")))
    report = {}
    for name, got, ref, frag in zip(names, got_params, ref_params, frag_rows):
        a = got.astype(np.float64).reshape(ref.shape[0], -1)
        b = ref.astype(np.float64).reshape(ref.shape[0], -1)
        scale = float(np.abs(b).max())
        assert scale > 0, name
        err = np.abs(a - b)
        worst = float(err[~frag].max()) / scale
        frac = float((err[~frag] > 1e-4 * np.maximum(np.abs(b[~frag]), 1e-2 * scale)).mean())
        report[name] = (worst, frac)
        assert worst <= GRAD_MAX_OF_SCALE and frac <= GRAD_NOISE_FRAC, (name, report[name])
        if frag.any():
            assert float(err[frag].max()) / scale <= FRAGILE_MAX_OF_SCALE, name
    rasters = {"dL_dsh": g_sh, "dL_dmeans2D_rgb": g_means2D}
    report.update(_grad_check7(rasters, gref, refs[0][1]))
    # ---- the densification statistics of this one pass, from the oracle's RGB-only screen-space gradient
    vis = refs[0][1]["radii"] > 0
    np.testing.assert_array_equal(denom.cpu().numpy().reshape(-1), vis.astype(np.float32))
    np.testing.assert_array_equal(max_radii.cpu().numpy(), np.where(vis, refs[0][1]["radii"], 0).astype(np.float32))
    want = np.where(vis, np.linalg.norm(gref["dL_dmeans2D_rgb"][:, :2], axis=1), 0.0)
    got_acc = accum.cpu().numpy().reshape(-1).astype(np.float64)
    solid = ~gref["touched"]
    assert float(np.abs(got_acc - want)[solid].max()) <= 1e-4 * float(want.max())
    print("SEVEN_PARAMS", workload, {k: tuple(f"{x:.1e}" for x in v[:2]) for k, v in report.items()})


@pytest.mark.parametrize("name", ["strands", "dense_long_lists", "medium_lists", "many_tiles", "sh3_bg", "tiny_image"])
def test_row_reduce_kernel_equals_the_in_kernel_row_sums(name):
    """row_reduce_kernel (round 6: the per-Gaussian sums of the instance rows as a launch balanced by rows -- runs of 512 rows per
    wavefront, segments found by the Gaussian id blend_bwd_kernel<7> leaves in every row's sixteenth float, partial sums for the
    segments that cross a run) against the sums taken inside preprocess_bwd_kernel: the same terms, so every gradient of the
    7-channel backward agrees to rounding (2e-5 of the tensor's scale); each form is bitwise reproducible; and a scratch
    poisoned with NaN shows that no row or partial that nobody wrote is ever read."""
    import torch
    import hgs_runtime as rt
    s = _scene(name)
    P = s["means3D"].shape[0]
    rng = np.random.default_rng(31)
    extra = torch.from_numpy(rng.uniform(-1, 1, size=(P, 4)).astype(np.float32)).cuda()
    fw = _forward7(s, extra, np.zeros(7, np.float32), True)
    dplanes = rng.normal(size=(7, s["H"], s["W"])).astype(np.float32)
    from diff_gaussian_rasterization import _C
    was = _C.set_row_reduce(False)
    os.environ["HGS_POISON_SCRATCH"] = "1"
    try:
        g_in = _backward7(s, extra, fw, None, dplanes)
        _C.set_row_reduce(True)
        g_rr = _backward7(s, extra, fw, None, dplanes)
        g_rr2 = _backward7(s, extra, fw, None, dplanes)
    finally:
        _C.set_row_reduce(was)
        os.environ.pop("HGS_POISON_SCRATCH", None)
    assert fw["R"] > 0
    for k in g_in:
        if g_in[k].size == 0:
            continue
        assert np.isfinite(g_rr[k]).all() and np.isfinite(g_in[k]).all(), k
        np.testing.assert_array_equal(g_rr[k].view(np.uint32), g_rr2[k].view(np.uint32), err_msg=k)
        scale = float(np.abs(g_in[k]).max())
        assert float(np.abs(g_rr[k].astype(np.float64) - g_in[k]).max()) <= 2e-5 * max(scale, 1e-30), k
    assert any(float(np.abs(v).max()) > 0 for v in g_in.values() if v.size)


@pytest.mark.parametrize("name", ALL + ["c2_full_size"])
def test_row_run_counting_changes_nothing(name):
    """HGS_COUNT_ROW_RUNS (include/hgs.h: tile rectangles of more than 16 tiles counted by their tile rows -- two marks per row,
    summed up by tile_delta_kernel -- instead of tile by tile): every buffer of the pass is what the tile-by-tile form gives, bit
    for bit, in the blocking mode and in the capacity mode, and the marks are left at zero (passes on a caller-cleared image
    buffer, which rely on that: tests/test_gpu_train.py::test_row_run_counting_in_the_fused_iterations).  c2_full_size: BASELINE config 2, a Stage-I cloud whose Gaussians cover ~40 tiles each;
    many_tiles: 17 545 tiles, three rounds of the summing workgroup; rectangles that end at the frame's right edge close on the
    next row's first entry (one running sum over all tiles)."""
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    s = _workload_scene("c2") if name == "c2_full_size" else _scene(name)
    was = _C.set_row_runs(False)
    try:
        ref_fw = G.run_forward(s)
        ref = G.intermediates(s, ref_fw)
        _C.set_row_runs(True)
        fw = G.run_forward(s)
        got = G.intermediates(s, fw)
        for k in ("radii", "tiles_touched", "point_offsets", "ranges", "point_list", "keys_sorted", "n_contrib"):
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
        assert got["num_rendered"] == ref["num_rendered"] and got["status"][1] == 0
        np.testing.assert_array_equal(got["out_color"].view(np.uint32), ref["out_color"].view(np.uint32))
        lay = G.rt.layout("image", s["W"], s["H"])
        n_marks = (((s["W"] + 15) // 16) * ((s["H"] + 15) // 16) + 2) & ~1
        marks = G._view(fw["img"], lay["tile_cursor"] - 4 * n_marks, n_marks, np.int32)
        assert not marks.any()
        if ref["num_rendered"] == 0:
            return
        try:
            _C.reset_capacity(0)
            _C.set_async(True)
            G.run_forward(s)
            for _ in range(2):
                fw2 = G.run_forward(s)
                assert _C.check_async() == [ref["num_rendered"]]
                got2 = G.intermediates(s, fw2)
                ranges, point_list, keys_sorted = G.in_tile_order(got2, ref["num_rendered"])
                np.testing.assert_array_equal(ranges, ref["ranges"], err_msg="ranges")
                np.testing.assert_array_equal(point_list, ref["point_list"], err_msg="point_list")
                np.testing.assert_array_equal(keys_sorted, ref["keys_sorted"], err_msg="keys_sorted")
                np.testing.assert_array_equal(got2["out_color"].view(np.uint32), ref["out_color"].view(np.uint32))
        finally:
            _C.set_async(False)
    finally:
        _C.set_row_runs(was)


@pytest.mark.parametrize("name", ["strands", "dense_long_lists", "medium_lists", "many_tiles", "one_huge_tile", "sh3_bg", "tiny_image",
                                  "strands_precomp", "c2_full_size", "c3_full_size"])
def test_lazy_records_change_nothing(name):
    """_C.set_lazy_records (include/hgs.h HGS_RECORDS_*): the blend kernels building an entry's record from its Gaussian's template through the
    sorted key, against streaming the records the sort kernel packs -- image, contributor counts, final transmittance and every
    gradient of the 3-channel pass bit for bit, in the blocking and (the 7-channel pass too: tests/test_gpu_train.py) the capacity
    mode; split lists (dense_long_lists, one_huge_tile, C2 at size), 17 545 tiles, precomputed colours."""
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    s = _workload_scene(name[:2]) if name.endswith("_full_size") else _scene(name)
    dpix = np.random.default_rng(11).normal(size=(3, s["H"], s["W"])).astype(np.float32)
    runs = {}
    was = _C.set_lazy_records(None)
    try:
        for lazy in (0, 1):
            _C.set_lazy_records(lazy)
            fw = G.run_forward(s)
            got = G.intermediates(s, fw)
            assert got["status"][14] == lazy and got["status"][1] == 0
            runs[lazy] = (got, G.run_backward(s, fw, dpix))
        for k in ("out_color", "final_T"):
            np.testing.assert_array_equal(runs[0][0][k].view(np.uint32), runs[1][0][k].view(np.uint32), err_msg=k)
        for k in ("n_contrib", "ranges", "point_list", "keys_sorted", "tile_maxc"):
            np.testing.assert_array_equal(runs[0][0][k], runs[1][0][k], err_msg=k)
        for k in runs[0][1]:
            np.testing.assert_array_equal(runs[0][1][k].view(np.uint32), runs[1][1][k].view(np.uint32), err_msg=k)
        if runs[0][0]["num_rendered"] == 0:
            return
        _C.reset_capacity(0)
        _C.set_async(True)
        G.run_forward(s)
        for lazy in (0, 1):
            _C.set_lazy_records(lazy)
            fw = G.run_forward(s)
            assert _C.check_async() == [runs[0][0]["num_rendered"]]
            np.testing.assert_array_equal(fw["color"].cpu().numpy().view(np.uint32), runs[0][0]["out_color"].view(np.uint32))
            g = G.run_backward(s, fw, dpix)
            for k in g:
                np.testing.assert_array_equal(g[k].view(np.uint32), runs[0][1][k].view(np.uint32), err_msg=k)
    finally:
        _C.set_async(False)
        _C.set_lazy_records(was)
