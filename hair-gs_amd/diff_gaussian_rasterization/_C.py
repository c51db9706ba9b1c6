"""Drop-in for the reference's pybind11 module `diff_gaussian_rasterization._C`
(submodules/diff-gaussian-rasterization/ext.cpp:15-19): same three functions, same argument order, same
return tuples -- implemented over the C ABI of libhgs.so (include/hgs.h) with ctypes."""
import contextlib
import ctypes as C
import os

import torch

import hgs_runtime as rt

# ---- capacity mode: its bookkeeping lives in this module and nowhere else ---------------------------------------------
# Default (blocking mode) = the reference's behaviour: every forward waits once for `num_rendered`
# (cuda_rasterizer/rasterizer_impl.cu:280-281) to size the binning buffer exactly.  After set_async(True) only the first pass
# does, and learns a CAPACITY from it (raise_capacity); later passes size the buffer from the capacity (their `num_rendered`)
# and never wait: the library keeps a sticky maximum of the true counts in one int32 word per device (hgs_forward_preprocess
# max_rendered).  A pass on this module's word sets the pending mark (`dirty`) and lowers `cap_used` to its capacity;
# check_async() clears the marks and judges those passes, set_async() and discard_pending() clear them without a verdict.
# A pass given the caller's own `max_rendered` word sets no mark: that caller reads its word (read_max_rendered) and judges.
IMAGE_PREZEROED = 2   # include/hgs.h HGS_IMAGE_PREZEROED (flag in `prefiltered`)
COUNT_ROW_RUNS = 4    # include/hgs.h HGS_COUNT_ROW_RUNS
TILE_CULL = 8         # include/hgs.h HGS_TILE_CULL
RECORDS_PACKED, RECORDS_LAZY = 16, 32   # include/hgs.h HGS_RECORDS_* (flags of hgs_forward_render)
ROWS_INLINE, ROWS_REDUCE = 64, 128      # include/hgs.h HGS_ROWS_* (flags of hgs_backward)
_state = {"async": False, "slack": 1.5, "cap": 0, "dirty": False, "cap_used": None,   # (cap 0: none learnt yet; cap_used: the smallest a pending pass ran with)
          "max_R": {}, "last_exact_R": 0, "last_counts_clean": False,                   # device -> sticky word; side results of the last pass / check
          "cull": None, "row_reduce": None, "lazy_records": None, "row_runs": None}   # the tri-state mode setters


class HgsCapacityOverflow(RuntimeError):
    pass


def bucket_capacity(n):
    """A binning capacity of at least `n` instances with four significant bits (m x 2^e, 8 <= m < 16: at most 12.5 % above n).
    The workspaces carved for a capacity are the largest allocations of a pass (~330 B per instance); a model that grows by a few
    per cent per topology event would otherwise ask for a slightly larger block at every re-capture, which no cached block can
    serve -- the caching allocator then holds one retired block per event (tools/dev/recapture_memory.py).  In buckets, successive
    captures ask for the same sizes and take the blocks the dropped graph has freed."""
    n = int(n)
    if n <= 16:
        return max(n, 0)
    e = n.bit_length() - 4
    return ((n + (1 << e) - 1) >> e) << e


def set_tile_cull(enabled=True):
    """Tile culling (include/hgs.h HGS_TILE_CULL: drop the (Gaussian, tile) instances no pixel can blend) for ALL entry points
    of this module: True / False, or None for the per-entry-point defaults:
      rasterize_gaussians         OFF -- the reference's own function: `num_rendered`, the tile lists in the returned
                                  buffers and `n_contrib` are the reference's, entry for entry;
      rasterize_gaussians_culled  (what diff_gaussian_rasterization.GaussianRasterizer, i.e. render(), calls) and
      rasterize_gaussians_multi   ON -- callers that only see the image, the radii and the gradients.
    Image, radii and final_T are bit-identical with and without; so are the gradients, except those of Gaussians whose rows the
    backward streams or row_reduce_kernel sums (the same terms, associated differently).  Tiles long enough to be blended in
    segments agree to rounding.  Returns the previous setting."""
    was = _state["cull"]
    _state["cull"] = None if enabled is None else bool(enabled)
    return was


def _pinned(mode, env):
    """`mode`, unless the A/B aid `env` (HGS_ROW_REDUCE, HGS_ROW_RUNS, HGS_LAZY_RECORDS) = 0 / 1 pins it for the whole process."""
    v = os.environ.get(env)
    return v == "1" if v in ("0", "1") else mode


def set_row_reduce(mode):
    """How the single-pass backward sums the instance rows per Gaussian (include/hgs.h HGS_ROWS_REDUCE / HGS_ROWS_INLINE): True /
    False, or None = decide per call -- from the exact instance count of a blocking-mode pass (R >= 4 P), from the library's
    capacity rule otherwise.  train.GraphedStep.capture() sets it from the instance counts its warm-up passes measured, so that the form
    follows the MODEL (and with it every replay and every eager iteration until the next capture), not the capacity a run
    happens to hold: a run that rolls back and raises its capacity keeps the arithmetic of one that never overflowed."""
    was = _state["row_reduce"]
    _state["row_reduce"] = None if mode is None else bool(mode)
    return was


def _row_reduce_flags(P, R):
    mode = _pinned(_state["row_reduce"], "HGS_ROW_REDUCE")
    if mode is None and not _state["async"]:
        mode = R >= 4 * P
    return 0 if mode is None else (ROWS_REDUCE if mode else ROWS_INLINE)   # (None: the library's rule, R >= 8 P)


def set_lazy_records(mode):
    """How the blend kernels of the following passes (and of their backwards) get the per-entry records (include/hgs.h
    HGS_RECORDS_LAZY / HGS_RECORDS_PACKED): True = built from the Gaussians' templates through the sorted keys, False = packed
    by the sort kernel, None = the library's rule (lazy from 128 entries per tile).  Images and gradients are the same bits
    either way.  Returns the previous setting."""
    was = _state["lazy_records"]
    _state["lazy_records"] = None if mode is None else bool(mode)
    return was


def _records_flags():
    lazy = _pinned(_state["lazy_records"], "HGS_LAZY_RECORDS")
    return 0 if lazy is None else (RECORDS_LAZY if lazy else RECORDS_PACKED)   # (None: the library's rule)


def set_row_runs(mode):
    """How the preprocess launch counts tile rectangles of more than 16 tiles (include/hgs.h HGS_COUNT_ROW_RUNS): True = by tile
    rows plus a one-workgroup launch, False = tile by tile, None = decide per pass from the instances per Gaussian seen so far
    (capacity mode: the capacity; blocking mode: the previous pass's exact count) -- the counts are the same integers either way."""
    was = _state["row_runs"]
    _state["row_runs"] = None if mode is None else bool(mode)
    return was


def _row_runs_flag(P, use_async):
    mode = _pinned(_state["row_runs"], "HGS_ROW_RUNS")
    if mode is None:
        mode = (_state["cap"] if use_async else _state["last_exact_R"]) >= 8 * P
    return COUNT_ROW_RUNS if (mode and P > 0) else 0


def set_async(enabled=True, slack=1.5):
    """Capacity mode on / off (see the top of the module); clears the pending marks, keeps the learnt capacity."""
    _state["async"], _state["slack"] = bool(enabled), float(slack)
    _state["dirty"], _state["cap_used"] = False, None


@contextlib.contextmanager
def async_mode(enabled, slack=None):
    """Run the body in capacity mode (at `slack`, if given) or blocking mode; mode, slack and pending marks are then put back, a capacity learnt inside stays."""
    saved = {k: _state[k] for k in ("async", "slack", "dirty", "cap_used")}
    _state["async"], _state["slack"] = bool(enabled), _state["slack"] if slack is None else float(slack)
    try:
        yield
    finally:
        _state.update(saved)


def capacity():
    """The learnt binning capacity (0: none yet)."""
    return _state["cap"]


def reset_capacity(n=0):
    """Forget the learnt capacity (the next capacity-mode pass blocks once and learns it anew), or force it to `n`."""
    _state["cap"] = int(n)


def raise_capacity(worst, slack=None):
    """THE growth rule: the capacity covers slack x `worst` instances (None: the mode's slack) and never shrinks.  Returns it."""
    slack = _state["slack"] if slack is None else slack
    _state["cap"] = max(_state["cap"], bucket_capacity(int(worst * slack) + 4096))
    return _state["cap"]


def last_exact_rendered():
    """The instance COUNT (not a capacity) of the last blocking pass or check_async(): what set_row_reduce's callers decide by."""
    return _state["last_exact_R"]


def last_counts_clean():
    """Did the last pass leave the per-tile instance counters of its image buffer at zero?  (see _forward)"""
    return _state["last_counts_clean"]


def _max_rendered(dev):
    if dev not in _state["max_R"]:
        _state["max_R"][dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return _state["max_R"][dev]


def read_max_rendered(word=None):
    """THE read of a sticky word (None: the worst over this module's, one per device), which it zeroes; nothing else changes."""
    worst = 0
    for t in _state["max_R"].values() if word is None else (word,):
        worst = max(worst, int(t.item()) & 0xFFFFFFFF)   # (.item() synchronises the stream the passes ran on; the word is unsigned)
        t.zero_()
    if worst == 0xFFFFFFFF:   # include/hgs.h HGS_WAIT_TIMED_OUT: an error (every word is zeroed by now), never a count
        raise rt.HgsError("a raster pass gave up an inter-workgroup wait (status word 8): its frame is invalid")
    return worst


def _mark_pending(cap):
    _state["dirty"], _state["cap_used"] = True, cap if _state["cap_used"] is None else min(_state["cap_used"], cap)


def discard_pending():
    """Zero every word unread and clear the marks; returns the smallest capacity a pass since the last check ran with (or None)."""
    cap, _state["dirty"], _state["cap_used"] = _state["cap_used"], False, None
    for t in _state["max_R"].values():
        t.zero_()
    return cap


def check_async():
    """Synchronise once and validate every pass issued since the last check against the capacity it ran with; returns
    [largest num_rendered seen] ([] if no pass was issued).  Raises HgsCapacityOverflow after raising the capacity."""
    if not _state["dirty"]:
        return []
    cap, _state["dirty"], _state["cap_used"] = _state["cap_used"], False, None
    worst = _state["last_exact_R"] = read_max_rendered()
    raised = raise_capacity(worst)
    if cap is not None and worst > cap:
        raise HgsCapacityOverflow(f"a raster pass needed {worst} instances (capacity {cap}): capacity raised to {raised}, repeat the step")
    return [worst]


def _f32(t, name):
    if t is None or t.numel() == 0:
        return None
    return rt.require_gpu_tensor(t, name, torch.float32)


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, debug):
    """RasterizeGaussiansCUDA (rasterize_points.cu:35-115).
    Returns (num_rendered, out_color[3,H,W], radii[P], geomBuffer, binningBuffer, imgBuffer); the tile lists are the
    reference's (see set_tile_cull)."""
    return _forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                    None, False)


def rasterize_gaussians_culled(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                               viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                               prefiltered, debug):
    """rasterize_gaussians with tile culling on (this module's extension; what GaussianRasterizer / render() call): fewer
    instances in the buffers; the same image, radii and final_T bit for bit, and gradients as set_tile_cull states."""
    return _forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                    None, True)


def rasterize_gaussians_multi(background7, means3D, colors, extra4, opacity, scales, rotations, scale_modifier,
                              cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh,
                              degree, campos, prefiltered, debug, image_buffer=None, hair=None):
    """Single-pass 7-channel forward (hgs_forward_render, n_extra 4): RGB + `extra4` [P,4] unclamped channels blended with
    the same weights.  Returns (num_rendered, out_color[7,H,W], radii, geomBuffer, binningBuffer, imgBuffer).
    image_buffer: a uint8 tensor of hgs_image_bytes(W, H) whose counters the caller has cleared on this stream
    (hgs_iteration_prologue): used as the imgBuffer, and the pass skips its own clearing launch."""
    return _forward(background7, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug,
                    extra4, True, image_buffer, None, hair)


class _ParamSource:
    """The model's raw parameters behind means3D / scales / rotations / opacity (/ extra4) of a pass: those tensors are then
    OUTPUTS (a cloud's means3D: its own parameter), written by the pass's first launch.  In capacity mode that launch is
    hgs_params_forward_preprocess (parameters -> Gaussians -> preprocess in one kernel, `fusion`'s riders beside it); otherwise, or
    with fuse=False, hgs_params_forward runs in front of the ordinary preprocess launch.  `fusion`: hgs_runtime.StrandFusion (or
    None); `fill(fused)` is called once the form is known and must put the iteration prologue (if one rides) into `fusion` with
    the matching zero range (hgs_runtime.strand_step.ViewTable.carry_prologue).
    Holds `params`, an hgs_runtime.ParamForward filled in except for the output pointers, and `inputs`, the validated
    contiguous tensors it points to."""

    def __init__(self, kind, fusion, fill, fuse, **inputs):
        self.params, self.fusion, self.fill, self.fuse = rt.ParamForward(kind=kind), fusion, fill, bool(fuse)
        self.inputs = {k: rt.require_gpu_tensor(t, k, torch.int64) if k == "endpoint_pairs" else _f32(t, k) for k, t in inputs.items()}
        for k, t in self.inputs.items():
            setattr(self.params, k, rt.ptr(t))


class HairSource(_ParamSource):
    """The strand parameters of a pass (include/hgs.h HGS_PARAMS_HAIR)."""

    def __init__(self, endpoints, pairs, width, factor, opacity_raw, mask_raw, fusion=None, fill=None, fuse=True):
        super().__init__(rt.PARAMS_HAIR, fusion, fill, fuse, endpoints=endpoints, endpoint_pairs=pairs, width=width,
                         opacity_raw=opacity_raw, mask_raw=mask_raw)
        self.params.dist_to_scale_factor = float(factor)


class CloudSource(_ParamSource):
    """The Stage-I counterpart: a cloud's raw scaling / rotation / opacity / mask parameters (HGS_PARAMS_CLOUD)."""

    def __init__(self, scaling_raw, rotation_raw, opacity_raw, mask_raw, fusion=None, fill=None, fuse=True):
        super().__init__(rt.PARAMS_CLOUD, fusion, fill, fuse, scaling_raw=scaling_raw, rotation_raw=rotation_raw,
                         opacity_raw=opacity_raw, mask_raw=mask_raw)


def will_fuse_hair(W, H):
    """Would a pass with a HairSource / CloudSource (fuse=True) at this size run the one-launch form now?  (capacity mode with a learnt capacity,
    at most HGS_FUSED_PREPROCESS_MAX_TILES tiles)"""
    return (_state["async"] and _state["cap"] > 0 and os.environ.get("HGS_FUSE_PREPROCESS", "1") != "0"
            and ((int(W) + 15) // 16) * ((int(H) + 15) // 16) <= rt.FUSED_PREPROCESS_MAX_TILES)


def rasterize_gaussians_prezeroed(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                                  viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                                  image_buffer, max_rendered=None, hair=None):
    """rasterize_gaussians_culled on an image buffer whose counters the caller has cleared on this stream (see
    rasterize_gaussians_multi); max_rendered: an int32[1] device tensor of the caller's that receives the sticky maximum of
    num_rendered in capacity mode instead of this module's (gaussian_renderer.frames validates its own frames with it)."""
    return _forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                    projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, False, False,
                    None, True, image_buffer, max_rendered, hair)


def _forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
             projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug, extra4,
             cull, image_buffer=None, max_rendered=None, hair=None):
    if means3D.ndim != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")  # rasterize_points.cu:57-59
    L = rt.lib()
    means3D = rt.require_gpu_tensor(means3D, "means3D", torch.float32)
    dev = means3D.device
    P, H, W = means3D.shape[0], int(image_height), int(image_width)
    M = sh.shape[1] if (sh is not None and sh.numel() != 0) else 0
    n_ch = 3 if extra4 is None else 7
    extra_ = None if extra4 is None else rt.require_gpu_tensor(extra4, "extra4", torch.float32)
    out_color = torch.empty((n_ch, H, W), dtype=torch.float32, device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    u8 = dict(dtype=torch.uint8, device=dev)
    geom = torch.empty((L.hgs_geom_bytes(P),), **u8)
    cull = _state["cull"] if _state["cull"] is not None else cull
    flags = int(bool(prefiltered)) | (TILE_CULL if cull else 0)
    if image_buffer is not None:
        if image_buffer.numel() != L.hgs_image_bytes(W, H) or image_buffer.dtype != torch.uint8 or image_buffer.device != dev:
            raise RuntimeError("image_buffer: need a uint8 tensor of hgs_image_bytes(W, H) on the inputs' device")
        img, flags = image_buffer, flags | IMAGE_PREZEROED
    else:
        img = torch.empty((L.hgs_image_bytes(W, H),), **u8)
    bg = _f32(background, "bg")
    colors_, opacity_, scales_, rots_, cov_, sh_ = (_f32(colors, "colors_precomp"), _f32(opacity, "opacities"),
                                                     _f32(scales, "scales"), _f32(rotations, "rotations"),
                                                     _f32(cov3D_precomp, "cov3D_precomp"), _f32(sh, "sh"))
    view, proj, cam = _f32(viewmatrix, "viewmatrix"), _f32(projmatrix, "projmatrix"), _f32(campos, "campos")
    stream = rt.current_stream()
    with torch.cuda.device(dev):
        use_async = _state["async"] and _state["cap"] > 0 and P > 0
        flags |= _row_runs_flag(P, use_async)
        n_host = C.c_int(0)
        fused_hair = hair is not None and hair.fuse and use_async and will_fuse_hair(W, H)
        mr_ = rt.ptr(max_rendered if max_rendered is not None else _max_rendered(dev)) if use_async else None
        if hair is not None:
            if scale_modifier != 1.0 or colors_ is not None or cov_ is not None or sh_ is None:
                raise RuntimeError("a HairSource / CloudSource pass renders SH colours at scale_modifier 1")
            if hair.fill is not None:
                hair.fill(fused_hair)
            ex_out = extra_ if extra_ is not None else torch.empty((P, 4), dtype=torch.float32, device=dev)
            pf = hair.params
            pf.means3D, pf.scale, pf.quat, pf.opacity, pf.extra4 = (rt.ptr(means3D), rt.ptr(scales_), rt.ptr(rots_),
                                                                    rt.ptr(opacity_), rt.ptr(ex_out))
            fu_ = None if hair.fusion is None else C.byref(hair.fusion)
            if fused_hair:
                rt.check(L.hgs_params_forward_preprocess(stream, P, int(degree), M, W, H, C.byref(pf), rt.ptr(sh_), rt.ptr(view),
                                                         rt.ptr(proj), rt.ptr(cam), float(tan_fovx), float(tan_fovy), flags,
                                                         rt.ptr(geom), rt.ptr(img), rt.ptr(radii), mr_, fu_))
            else:
                rt.check(L.hgs_params_forward(stream, P, C.byref(pf), fu_))
        if not fused_hair:
            rt.check(L.hgs_forward_preprocess(stream, P, int(degree), M, W, H, rt.ptr(means3D), rt.ptr(sh_), rt.ptr(colors_),
                                              rt.ptr(opacity_), rt.ptr(scales_), float(scale_modifier), rt.ptr(rots_),
                                              rt.ptr(cov_), rt.ptr(view), rt.ptr(proj), rt.ptr(cam), float(tan_fovx),
                                              float(tan_fovy), flags, rt.ptr(geom), rt.ptr(img),
                                              rt.ptr(radii), None if use_async else C.addressof(n_host), mr_))
        # the scan of a capacity-mode pass (scatter kernel) leaves the per-tile instance counters of `img` at zero; a blocking
        # pass leaves its counts there (hgs_runtime.strand_step.ViewTable.counts_clean follows this)
        if P > 0:
            _state["last_counts_clean"] = bool(use_async and ((W + 15) // 16) * ((H + 15) // 16) <= rt.FUSED_PREPROCESS_MAX_TILES)
        if use_async:
            R = _state["cap"]
        else:
            R = int(n_host.value)
            _state["last_exact_R"] = R
            if _state["async"]:  # first call: learn the scale of the scene with one blocking read
                raise_capacity(R)
        binning = torch.empty((L.hgs_binning_bytes(R, n_ch),), **u8)
        rt.check(L.hgs_forward_render(stream, P, W, H, R, n_ch - 3, _records_flags(), rt.ptr(bg), rt.ptr(colors_),
                                      rt.ptr(extra_), rt.ptr(geom), rt.ptr(binning), rt.ptr(img), rt.ptr(out_color)))
        if use_async and max_rendered is None:
            _mark_pending(R)
        if debug:
            torch.cuda.synchronize(dev)  # surface asynchronous faults here, like CHECK_CUDA (auxiliary.h:166-173)
    return R, out_color, radii, geom, binning, img


def _scratch(nbytes, dev):
    """Backward scratch (per-instance partial-gradient rows).  It is deliberately NOT cleared by the library; with
    HGS_POISON_SCRATCH=1 (tests) it is filled with NaN so that any read of a row nobody wrote shows up."""
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    if os.environ.get("HGS_POISON_SCRATCH") == "1" and nbytes >= 4:
        buf[:nbytes // 4 * 4].view(torch.float32).fill_(float("nan"))
    return buf


def _backward(n_extra, background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
              projmatrix, tan_fovx, tan_fovy, planes, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug=False,
              params=None, plan=None):
    """hgs_backward of a pass with 3 + n_extra channels (`planes`: one [H,W] gradient tensor per channel), or with `params`
    hgs_backward_multi_params (with `plan`, a filled hgs_runtime.BlockPlan: hgs_backward_multi_params_planned).  Returns the gradients in hgs_backward's order -- dL_dextra (None for 3 channels), dL_dmeans2D,
    dL_dconic, dL_dopacity, dL_dcolors, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations --, or dL_dsh alone with
    `params`."""
    L = rt.lib()
    means3D = rt.require_gpu_tensor(means3D, "means3D", torch.float32)
    dev, P = means3D.device, means3D.shape[0]
    H, W = int(planes[0].shape[-2]), int(planes[0].shape[-1])
    M = sh.shape[1] if (params is not None or (sh is not None and sh.numel() != 0)) else 0   # (the parameter form has SH colours)
    f32 = dict(dtype=torch.float32, device=dev)
    new = torch.empty if P > 0 else torch.zeros  # the kernel writes every element when P > 0
    if params is None:
        grads = [new((P, 4), **f32) if n_extra else None, new((P, 3), **f32), new((P, 2, 2), **f32), new((P, 1), **f32),
                 new((P, 3), **f32), new((P, 3), **f32), new((P, 6), **f32), new((P, M, 3), **f32), new((P, 3), **f32),
                 new((P, 4), **f32)]
        if P == 0:
            return grads
    else:
        grads = new((P, M, 3), **f32)
    scratch = _scratch(L.hgs_backward_scratch_bytes(P, int(R), 3 + n_extra), dev)
    # keep every (possibly freshly made contiguous) input alive in a local until the launch has been enqueued:
    # a temporary released early would hand its block to the next temporary of the same size
    planes = [rt.require_gpu_tensor(g, "dL_dpix plane", torch.float32) for g in planes]
    plane_ptrs = (C.c_void_p * (3 + n_extra))(*[g.data_ptr() for g in planes])
    bg_, sh_, colors_, scales_, rots_, cov_ = (_f32(background, "bg"), _f32(sh, "sh"), _f32(colors, "colors_precomp"),
                                               _f32(scales, "scales"), _f32(rotations, "rotations"),
                                               _f32(cov3D_precomp, "cov3D_precomp"))
    view_, proj_, cam_ = _f32(viewmatrix, "viewmatrix"), _f32(projmatrix, "projmatrix"), _f32(campos, "campos")
    radii_ = rt.require_gpu_tensor(radii, "radii", torch.int32)
    flags = _row_reduce_flags(P, int(R))
    with torch.cuda.device(dev):
        if params is None:
            rt.check(L.hgs_backward(rt.current_stream(), P, int(degree), M, int(R), W, H, n_extra, flags, rt.ptr(bg_),
                                    rt.ptr(means3D), rt.ptr(sh_), rt.ptr(colors_), rt.ptr(scales_), float(scale_modifier),
                                    rt.ptr(rots_), rt.ptr(cov_), rt.ptr(view_), rt.ptr(proj_), rt.ptr(cam_), float(tan_fovx),
                                    float(tan_fovy), rt.ptr(radii_), rt.ptr(geomBuffer), rt.ptr(binningBuffer),
                                    rt.ptr(imageBuffer), plane_ptrs, rt.ptr(scratch), *[rt.ptr(g) for g in grads]))
        else:
            rt.check(L.hgs_backward_multi_params_planned(
                rt.current_stream(), P, int(degree), M, int(R), W, H, flags, rt.ptr(bg_), rt.ptr(means3D), rt.ptr(sh_),
                rt.ptr(scales_), rt.ptr(rots_), rt.ptr(view_), rt.ptr(proj_), rt.ptr(cam_), float(tan_fovx), float(tan_fovy),
                rt.ptr(radii_), rt.ptr(geomBuffer), rt.ptr(binningBuffer), rt.ptr(imageBuffer), plane_ptrs, rt.ptr(scratch),
                rt.ptr(grads), C.byref(params), None if plan is None else C.byref(plan)))
        if debug:
            torch.cuda.synchronize(dev)
    return grads


def rasterize_gaussians_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                                 viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos,
                                 geomBuffer, R, binningBuffer, imageBuffer, debug):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196).
    Returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)."""
    _, dmeans2D, dconic, dopacity, dcolors, dmeans3D, dcov3D, dsh, dscales, drotations = _backward(
        0, background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        tan_fovx, tan_fovy, dL_dout_color.unbind(0), sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug)
    rasterize_gaussians_backward.last_dL_dconic = dconic  # kept for the parity tests
    return dmeans2D, dcolors, dopacity, dmeans3D, dcov3D, dsh, dscales, drotations


def rasterize_gaussians_multi_backward(background7, means3D, radii, colors, scales, rotations, scale_modifier,
                                       cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, grad_planes, sh,
                                       degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug):
    """Backward of the single-pass mode (hgs_backward, n_extra 4).  `grad_planes`: list of 7 contiguous [H,W] tensors (views
    into larger gradient tensors are fine).  `background7=None` declares an all-zero background (include/hgs.h: selects the
    black-background specialisation of the blend backward; same gradients).  Returns (dL_dmeans2D_rgb, dL_dcolors, dL_dextra4, dL_dopacity,
    dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations)."""
    dextra, dmeans2D, _, dopacity, dcolors, dmeans3D, dcov3D, dsh, dscales, drotations = _backward(
        4, background7, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        tan_fovx, tan_fovy, grad_planes, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, debug)
    return dmeans2D, dcolors, dextra, dopacity, dmeans3D, dcov3D, dsh, dscales, drotations


def rasterize_gaussians_multi_backward_params(background7, means3D, radii, scales, rotations, viewmatrix, projmatrix, tan_fovx,
                                              tan_fovy, grad_planes, sh, degree, campos, geomBuffer, R, binningBuffer,
                                              imageBuffer, params, plan=None):
    """hgs_backward_multi_params: the single-pass backward whose per-Gaussian launch also applies the parameters' backward
    (`params`: a filled hgs_runtime.ParamBackward; its output tensors are the caller's).  `plan` (a filled hgs_runtime.BlockPlan,
    strand models): that launch is also the endpoint gather (hgs_backward_multi_params_planned).  Returns dL_dsh [P,M,3]."""
    return _backward(4, background7, means3D, radii, None, scales, rotations, 1.0, None, viewmatrix, projmatrix, tan_fovx,
                     tan_fovy, grad_planes, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer, params=params, plan=plan)


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:198-217) -> bool[P]."""
    means3D = rt.require_gpu_tensor(means3D, "means3D", torch.float32)
    P = means3D.shape[0]
    present = torch.zeros((P,), dtype=torch.bool, device=means3D.device)
    if P:
        view_, proj_ = _f32(viewmatrix, "viewmatrix"), _f32(projmatrix, "projmatrix")
        with torch.cuda.device(means3D.device):
            rt.check(rt.lib().hgs_mark_visible(rt.current_stream(), P, rt.ptr(means3D), rt.ptr(view_), rt.ptr(proj_),
                                               rt.ptr(present)))
    return present
