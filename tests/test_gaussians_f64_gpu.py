"""preprocess_bwd_kernel (csrc/hgs_preprocess.hip) against float64 on the Gaussians of tests/gaussian_cases.py, ROW BY ROW
with each row's own yardstick (tests/gaussian_reference.py; conditions and comparator checked without a GPU in
tests/test_gaussians_f64_cpu.py).  The chain is fed the kernel's own upstream -- the dL_dmeans2D, dL_dconic and dL_dcolors it
summed and then used -- so no blend threshold and no pixel sum enters; through the C ABI, every output starts as NaN."""
import ctypes as C

import numpy as np
import pytest

from oracle import hgs_oracle as O
from tests import gaussian_cases as GC
from tests import gaussian_reference as GR

pytestmark = pytest.mark.gpu

# DESIGN.md section 2's rule: twice the worst ratio measured on the MI355X over all classes and tensors, rounded up to a power
# of two, never above 8.  Measured (table in DESIGN.md): 1.000 on every form, variant and size -- the kernel gives the fp32
# statement's bits, so its distance from float64 is the yardstick's base copy.
K = 2

OUTPUTS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
           "dL_drotations")


def _backward_nan(s, fw, dpix, scale_modifier=None, tanfovx=None):
    """hgs_backward on the forward `fw` of scene `s`, as diff_gaussian_rasterization._C._backward calls it, but into outputs
    that start as NaN; `scale_modifier` / `tanfovx` override what the ABI is told (the forward ran with the scene's)."""
    import torch
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    (bg, means3D, colors, _, scales, rotations, sm, cov3D, view, proj, tfx, tfy, H, W, sh, degree, campos, _, _) = fw["args"]
    L = rt.lib()
    P, R = means3D.shape[0], int(fw["R"])
    M = sh.shape[1] if sh.numel() else 0
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=means3D.device)   # noqa: E731
    grads = [nan(P, 3), nan(P, 2, 2), nan(P, 1), nan(P, 3), nan(P, 3), nan(P, 6), nan(P, M, 3), nan(P, 3), nan(P, 4)]
    scratch = _C._scratch(L.hgs_backward_scratch_bytes(P, R, 3), means3D.device)
    planes = [p.contiguous() for p in G.to_dev(dpix).unbind(0)]
    plane_ptrs = (C.c_void_p * 3)(*[p.data_ptr() for p in planes])
    rt.check(L.hgs_backward(rt.current_stream(), P, int(degree), M, R, int(W), int(H), 0, _C._row_reduce_flags(P, R), rt.ptr(bg),
                            rt.ptr(means3D), rt.ptr(sh), rt.ptr(colors), rt.ptr(scales),
                            float(sm if scale_modifier is None else scale_modifier), rt.ptr(rotations), rt.ptr(cov3D),
                            rt.ptr(view), rt.ptr(proj), rt.ptr(campos), float(tfx if tanfovx is None else tanfovx), float(tfy),
                            rt.ptr(fw["radii"]), rt.ptr(fw["geom"]), rt.ptr(fw["binning"]), rt.ptr(fw["img"]), plane_ptrs,
                            rt.ptr(scratch), None, *[rt.ptr(g) for g in grads]))
    torch.cuda.synchronize()
    g = {k: t.cpu().numpy() for k, t in zip(OUTPUTS, grads)}
    g["dL_dconic"] = g["dL_dconic"].reshape(P, 4)
    return g


def _run(s, **overrides):
    """Forward (every preprocess stage bit-exact with the fp32 oracle: the stage comparisons of test_gpu_raster._check_forward),
    backward on the smooth dL_dpix zeroed on the near-threshold pixels, and the float64 statement with its yardsticks on the
    kernel's own upstream.  Returns (kernel outputs, x64, E, s_i, oracle forward)."""
    from tests.test_gpu_raster import _check_forward_scene
    _, ref, fw, got = _check_forward_scene(s)
    ref_state = dict(ref)
    ref_state["n_contrib"], ref_state["final_T"] = got["n_contrib"].copy(), got["final_T"].copy()
    mask = O.fragile_pixels(s, ref_state)
    assert int(mask.sum()) <= 0.05 * max(1, int((got["n_contrib"] > 0).sum())) or s["means3D"].shape[0] < 64
    dpix = GC.smooth_dpix() * ~mask
    assert dpix.dtype == np.float32
    g = _backward_nan(s, fw, dpix, **overrides)
    for k in OUTPUTS:
        assert np.isfinite(g[k]).all(), f"{k}: NaN / Inf (an element nobody wrote?)"
    clamped = got["clamped"] if s["shs"] is not None else np.zeros((len(got["radii"]), 3), np.uint8)
    up = {k: g[k] for k in GR.UPSTREAM}
    assert np.array_equal(g["dL_dconic"][:, 2], np.zeros(len(got["radii"]), np.float32))
    x64, E, sc = GR.yardstick(s, up, got["radii"], clamped, s["classes"].get("clamp_edge"))
    culled = got["radii"] == 0
    for k in OUTPUTS:                                      # a culled Gaussian gets exact zeros everywhere
        assert not g[k].reshape(len(culled), -1)[culled].any(), k
    # the kernel against the fp32 statement itself, on the same upstream: elements that differ at all, and by how much of s_i
    x32 = GR.chain(s, up, got["radii"], clamped, False)
    diff = {k[3:]: (int((g[k].reshape(x32[k].shape) != x32[k]).sum()),
                    float((np.abs(g[k].reshape(len(culled), -1).astype(np.float64) - x32[k].reshape(len(culled), -1)).max(axis=1)
                           / np.where(sc[k] > 0, sc[k], 1.0)).max()) if x32[k].size else 0.0) for k in GR.TENSORS}
    print("F64ROW kernel vs fp32 statement (elements that differ, worst |diff| / s_i):", {k: (n, f"{d:.1e}") for k, (n, d) in diff.items()})
    return g, x64, E, sc, ref


def _assert_passes(s, g, x64, E, sc, label):
    worst_e, worst_r = GR.table(g, x64, E, sc, s["classes"], label)      # the figures first
    assert GR.cap_violations(E, sc, s["classes"]) == []
    bad = GR.failures(g, x64, E, sc, K, s["classes"])
    assert bad == [], (label, bad)


@pytest.mark.parametrize("form", GC.FORMS)
def test_per_gaussian_backward_against_float64(form):
    """a. every class, every row, every tensor, in each of the four input forms (sh0: the DC_ONLY instantiation)."""
    s = GC.hard_scene(form)
    g, x64, E, sc, ref = _run(s)
    vis = ref["radii"] > 0
    np.testing.assert_array_equal(np.flatnonzero(~vis), s["classes"]["near_cut"][0::2])
    for k in GR.TENSORS:                                   # no row is exempt
        if x64[k].size and not (k in ("dL_dscales", "dL_drotations") and s["scales"] is None):
            assert (sc[k][vis] > 0).all(), k
    _assert_passes(s, g, x64, E, sc, form)


@pytest.mark.parametrize("variant", ["scale_modifier", "far_origin"])
def test_per_gaussian_backward_against_float64_variants(variant):
    """The whole scene again at scale_modifier 0.6, and with world and camera shifted by (100, -50, 25)."""
    s = GC.hard_scene("sh3", scale_modifier=0.6) if variant == "scale_modifier" else GC.hard_scene("sh3", far_origin=True)
    g, x64, E, sc, _ = _run(s)
    _assert_passes(s, g, x64, E, sc, variant)


@pytest.mark.parametrize("what", ["scale_modifier", "tanfovx"])
def test_the_bar_sees_a_wrong_abi_argument(what):
    """b. the kernel itself must FAIL the comparator, in the class the change is aimed at, when the C ABI is told a
    scale_modifier off by 1e-4, or tan_fovx times 1.2 (which unclamps the clamp_x rows), against the reference at the true value."""
    s = GC.hard_scene("sh3")
    if what == "scale_modifier":
        aimed, over = "plain", dict(scale_modifier=float(np.float32(s["scale_modifier"] * (1 + 1e-4))))
    else:
        aimed, over = "clamp_x", dict(tanfovx=s["tanfovx"] * 1.2)
    g, x64, E, sc, _ = _run(s, **over)
    bad = GR.failures(g, x64, E, sc, K, s["classes"])
    print("WRONG_ABI", what, [(c, k, f"{r:.3g}", n) for c, k, r, n, _, _ in bad if c == aimed])
    assert any(c == aimed for c, *_ in bad), bad


@pytest.mark.parametrize("form", ["sh3", "sh0"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sizes_around_the_workgroup(n, form):
    """c. 1, 255, 256 and 257 rows of the concatenation: the lanes of the last workgroup that are past P."""
    s = GC.hard_scene(form, rows=GC.spread_rows(n))
    assert s["means3D"].shape[0] == n
    g, x64, E, sc, _ = _run(s)
    _assert_passes(s, g, x64, E, sc, f"{form}:{n}")
