"""blend_fwd_kernel / blend_bwd_kernel (csrc/hgs_blend.hip) against the float64 walk of the SAME fp32 2-D state, on the tiles
of tests/blend_cases.py, with the yardsticks of tests/blend_reference.py (cases, mask, statements and comparator are checked
without a GPU in tests/test_blend_f64_cpu.py).  The forward's preprocess and binning stages are compared bit for bit first
(test_gpu_raster._check_forward_scene), so only the blend can differ.  The float64 backward runs on the float64 forward's own
final_T and n_contrib, the kernel's on the kernel's own: nothing is handed across, so a transmittance error cannot cancel.
Through the C ABI; every gradient buffer starts as NaN."""
import ctypes as C

import numpy as np
import pytest

from tests import blend_cases as BC
from tests import blend_reference as BR

pytestmark = pytest.mark.gpu

# DESIGN.md section 2's rule: twice the worst ratio measured on the MI355X over all cases, forms and tensors, rounded up to a
# power of two, never above 8.  Measured (table in DESIGN.md): 4.24, `split` at segment length 1024 (dL_dextra; 2.7 at the
# shorter segments, <= 2.2 on every other case): twice that rounds up to 16, so the ceiling holds.
K = 8

OUTPUTS = ("dL_dextra", "dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
           "dL_drotations")


def _forward(scene, form):
    """The kernel's forward of a form: the 3-channel pass through _check_forward_scene (every stage in front of the blend bit for
    bit the fp32 oracle's), and for `seven` the single pass on the same lists.  Returns the pass's buffers and blend outputs."""
    from tests import gpu_util as G
    from tests.test_gpu_raster import _check_forward_scene, _forward7
    import hgs_runtime as rt
    s3 = dict(scene, bg=np.zeros(3, np.float32) if form == "black" else scene["bg7"][:3].copy())
    _, oref, fw, got = _check_forward_scene(s3)
    out = dict(s=s3, S=int(got["status"][6]), lazy=int(got["status"][14]), tile_maxc=got["tile_maxc"])
    if form != "seven":
        out.update(n_extra=0, planes=got["out_color"], final_T=got["final_T"], n_contrib=got["n_contrib"],
                   **{k: fw[k] for k in ("R", "radii", "geom", "binning", "img")})
        return out
    f7 = _forward7(s3, G.to_dev(scene["extra4"]), scene["bg7"], cull=False)
    assert f7["status"][1] == 0 and f7["status"][8] == 0 and f7["R"] == fw["R"]
    np.testing.assert_array_equal(f7["ranges"], oref["ranges"])
    if f7["R"]:
        pl = G._view(f7["binning"], rt.layout("binning", f7["R"])["point_list"], f7["R"], np.uint32)
        np.testing.assert_array_equal(pl, oref["point_list"])
    out.update(n_extra=4, planes=f7["planes"].cpu().numpy(), final_T=f7["final_T"], n_contrib=f7["n_contrib"], S=int(f7["status"][6]),
               lazy=int(f7["status"][14]), **{k: f7[k] for k in ("R", "radii", "geom", "binning", "img")})
    return out


def _backward(scene, form, f, planes, bg="own"):
    """hgs_backward on the forward `f` with the [C, H, W] upstream `planes`, into outputs that start as NaN.  bg: what the ABI is
    told -- "own": the forward's (NULL, the black-background specialisation, for the `black` form), or an array."""
    import torch
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    from tests import gpu_util as G
    s, n_extra = f["s"], f["n_extra"]
    d = lambda x: _C._f32(G.to_dev(x), "input")                          # noqa: E731
    means3D = G.to_dev(s["means3D"])
    P, R, W, H = means3D.shape[0], int(f["R"]), int(s["W"]), int(s["H"])
    M = 0 if s["shs"] is None else int(s["shs"].shape[1])
    if isinstance(bg, str):
        bg = None if form == "black" else (scene["bg7"] if n_extra else scene["bg7"][:3])
    bg_, sh_, col_, sc_, rot_, cov_ = d(bg), d(s["shs"]), d(s["colors_precomp"]), d(s["scales"]), d(s["rotations"]), d(s["cov3D_precomp"])
    view_, proj_, cam_ = d(s["viewmatrix"]), d(s["projmatrix"]), d(s["campos"])
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=means3D.device)   # noqa: E731
    grads = [nan(P, 4) if n_extra else None, nan(P, 3), nan(P, 2, 2), nan(P, 1), nan(P, 3), nan(P, 3), nan(P, 6), nan(P, M, 3), nan(P, 3),
             nan(P, 4)]
    L = rt.lib()
    scratch = _C._scratch(L.hgs_backward_scratch_bytes(P, R, 3 + n_extra), means3D.device)
    pl = [p.contiguous() for p in G.to_dev(np.ascontiguousarray(planes, np.float32)).unbind(0)]
    plane_ptrs = (C.c_void_p * (3 + n_extra))(*[p.data_ptr() for p in pl])
    rt.check(L.hgs_backward(rt.current_stream(), P, int(s["sh_degree"]), M, R, W, H, n_extra, _C._row_reduce_flags(P, R), rt.ptr(bg_),
                            rt.ptr(means3D), rt.ptr(sh_), rt.ptr(col_), rt.ptr(sc_), float(s["scale_modifier"]), rt.ptr(rot_),
                            rt.ptr(cov_), rt.ptr(view_), rt.ptr(proj_), rt.ptr(cam_), float(s["tanfovx"]), float(s["tanfovy"]),
                            rt.ptr(f["radii"]), rt.ptr(f["geom"]), rt.ptr(f["binning"]), rt.ptr(f["img"]), plane_ptrs, rt.ptr(scratch),
                            *[rt.ptr(g) for g in grads]))
    torch.cuda.synchronize()
    raw = {k: t.cpu().numpy() for k, t in zip(OUTPUTS, grads) if t is not None}
    for k, v in raw.items():
        assert np.isfinite(v).all(), f"{k}: NaN / Inf (an element nobody wrote?)"
    conic = raw["dL_dconic"].reshape(P, 4)
    assert not conic[:, 2].any()
    g = {"dL_dconic": conic[:, [0, 1, 3]], "dL_dopacity": raw["dL_dopacity"], "dL_dcolors": raw["dL_dcolors"]}
    if n_extra:
        g["dL_dmeans2D_rgb"], g["dL_dextra"] = raw["dL_dmeans2D"][:, :2], raw["dL_dextra"]
    else:
        g["dL_dmeans2D"] = raw["dL_dmeans2D"][:, :2]
    g["raw"] = raw
    return g


def _masked_planes(scene, form, ref):
    d7 = scene["dpix7"] * ref["clear"][None]
    assert d7.dtype == np.float32
    return d7 if form == "seven" else d7[:3]


def _run(name, form, label, bg="own"):
    """Forward, reference at the segment length the forward used, backward on the masked upstream; prints the table rows."""
    scene = BC.case(name)
    f = _forward(scene, form)
    ref = BR.reference(scene, form, S=f["S"])
    g = _backward(scene, form, f, _masked_planes(scene, form, ref), bg=bg)
    rep = BR.grade(ref, f["planes"], f["final_T"], f["n_contrib"], g, label=label)
    # a Gaussian with no clear pixel gets exact zeros
    for k, x in ref["x64"].items():
        none = ref["S"][k].max(axis=1) == 0
        assert not np.asarray(g[k])[none].any(), k
    return rep, f, g, ref


@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("name", list(BC.CASES))
def test_blend_against_float64(name, form):
    """a. every case and form at the library's own segment policy: forward bars per tile, n_contrib equal on clear pixels,
    gradient bars per row and column."""
    rep, *_ = _run(name, form, f"{name}:{form}")
    assert BR.failures(rep, K) == [], rep


@pytest.mark.parametrize("form", BC.FORMS)
@pytest.mark.parametrize("S", BC.SPLIT_S)
def test_split_lists_against_float64_at_pinned_segment_lengths(S, form):
    """b. `split` with the segment length pinned: the same lists unsplit, as two, three and many segments."""
    import hgs_runtime as rt
    L = rt.lib()
    try:
        rt.check(L.hgs_set_segment_policy(S, S, 1))
        rep, f, _, _ = _run("split", form, f"split:S{S}:{form}")
        assert f["S"] == S
        assert BR.failures(rep, K) == [], rep
    finally:
        rt.check(L.hgs_set_segment_policy(128, 1024, 2048))


@pytest.mark.parametrize("name,form", [("clamp", "bg"), ("stop", "seven")])
def test_the_bar_sees_a_wrong_background_at_the_abi(name, form):
    """c. the backward is told a background that differs by 1e-3 in one channel from the forward's: the kernel must FAIL the
    comparator on dL_dopacity, against the reference at the true background."""
    scene = BC.case(name)
    bg = (scene["bg7"] if form == "seven" else scene["bg7"][:3]).copy()
    bg[1] += np.float32(1e-3)
    rep, *_ = _run(name, form, f"WRONG_BG {name}:{form}", bg=bg)
    assert rep["dL_dopacity"] > K, rep
    assert rep["out_color"] <= K and rep["final_T"] <= K and rep["n_contrib"] == 0


@pytest.mark.parametrize("form", ["bg", "seven"])
def test_lazy_records_give_the_same_bits_on_split(form):
    """d. records built lazily through the sorted key against records the sort kernel packs: images and gradients bit for bit,
    at a pinned segment length (many segments) and at the library's policy."""
    import hgs_runtime as rt
    from diff_gaussian_rasterization import _C
    scene = BC.case("split")
    L = rt.lib()
    was = _C.set_lazy_records(None)
    try:
        for policy in ((128, 128, 1), (128, 1024, 2048)):
            rt.check(L.hgs_set_segment_policy(*policy))
            runs = []
            for lazy in (0, 1):
                _C.set_lazy_records(lazy)
                f = _forward(scene, form)
                assert f["lazy"] == lazy
                g = _backward(scene, form, f, scene["dpix7"] if form == "seven" else scene["dpix7"][:3])
                runs.append((f, g))
            (f0, g0), (f1, g1) = runs
            for k in ("planes", "final_T"):
                np.testing.assert_array_equal(f0[k].view(np.uint32), f1[k].view(np.uint32), err_msg=k)
            np.testing.assert_array_equal(f0["n_contrib"], f1["n_contrib"])
            for k in g0["raw"]:
                np.testing.assert_array_equal(g0["raw"][k].view(np.uint32), g1["raw"][k].view(np.uint32), err_msg=k)
    finally:
        _C.set_lazy_records(was)
        rt.check(L.hgs_set_segment_policy(128, 1024, 2048))
