"""Loader of libhgs.so (the hand-written HIP kernels behind a C ABI, include/hgs.h).

There is NO fallback: if the library is missing or fails to load, every op raises.  The library is built
in-tree by `hgs_runtime.build()` (hipcc --offload-arch=gfx950, cross-compiles without a GPU) and travels
with the source tree.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("HGS_LIB") or os.path.join(_PKG_ROOT, "libhgs.so")   # HGS_LIB: another build of the same ABI (A/B runs, tools/)
CSRC = os.path.join(_PKG_ROOT, "csrc")
_lib = None

vp, ci, cf, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); mirrors include/hgs.h one to one (tests/test_abi.py checks the header against this)
SIGNATURES = {
    "hgs_abi_version": (ci, []),
    "hgs_last_error": (C.c_char_p, []),
    "hgs_geom_bytes": (sz, [ci]),
    "hgs_image_bytes": (sz, [ci, ci]),
    "hgs_binning_bytes": (sz, [ci, ci]),
    "hgs_backward_scratch_bytes": (sz, [ci, ci, ci]),
    "hgs_forward_preprocess": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, cf, cf, ci,
                                    vp, vp, vp, vp, vp]),
    "hgs_forward_render": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_backward": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, cf, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp,
                          vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_param_backward_bytes": (sz, []),
    "hgs_backward_multi_params": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp, vp,
                                       vp, vp, vp]),
    "hgs_block_plan_bytes": (sz, []),
    "hgs_backward_multi_params_planned": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, cf, cf, vp, vp, vp, vp,
                                               vp, vp, vp, vp, vp]),
    "hgs_hair_endpoint_gather": (ci, [vp, ci, vp, vp, vp, vp, vp]),
    "hgs_mark_visible": (ci, [vp, ci, vp, vp, vp, vp]),
    "hgs_dist2_scratch_bytes": (sz, [ci]),
    "hgs_dist2": (ci, [vp, ci, vp, vp, vp, sz]),
    "hgs_ssim_l1_scratch_floats": (sz, [ci, ci, ci]),
    "hgs_ssim_l1_num_blocks": (ci, [ci, ci, ci]),
    "hgs_ssim_l1_forward": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "hgs_ssim_l1_backward": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_orientation_loss_num_blocks": (ci, [ci, ci]),
    "hgs_orientation_loss_forward": (ci, [vp, ci, ci, vp, vp, vp, cf, vp, vp, vp, vp]),
    "hgs_orientation_loss_backward": (ci, [vp, ci, ci, vp, vp, vp, cf, vp, vp, vp, vp, vp, vp]),
    "hgs_adam_step": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp, cf, cf, cf, vp]),
    "hgs_smoothness_num_blocks": (ci, [ci]),
    "hgs_smoothness_forward": (ci, [vp, ci, vp, vp, cf, cf, vp]),
    "hgs_smoothness_backward": (ci, [vp, ci, ci, vp, vp, cf, cf, vp, vp, vp]),
    "hgs_strand_geometry_forward": (ci, [vp, ci, vp, vp, vp, cf, vp, vp, vp, vp]),
    "hgs_strand_geometry_backward": (ci, [vp, ci, ci, vp, vp, vp, cf, vp, vp, vp, vp, vp, vp]),
    "hgs_view_targets_bytes": (sz, []),
    "hgs_head_params_bytes": (sz, []),
    "hgs_strand_fusion_bytes": (sz, []),
    "hgs_select_view": (ci, [vp, vp, ci, vp, cf, vp]),
    "hgs_iteration_prologue": (ci, [vp, vp, ci, vp, cf, vp, vp, sz, vp]),
    "hgs_adam_prep_bytes": (sz, []),
    "hgs_adam_inline_bytes": (sz, []),
    "hgs_image_zero_range": (ci, [ci, ci, vp, vp]),
    "hgs_graph_find_prologue": (ci, [vp, vp]),
    "hgs_graph_find_prologues": (ci, [vp, ci, vp, vp, vp]),
    "hgs_graph_set_prologue": (ci, [vp, vp, vp, ci, vp, cf, vp, vp, sz]),
    "hgs_set_view_queue": (ci, [vp, vp, ci, vp, cf, vp]),
    "hgs_select_view_queued": (ci, [vp, vp, ci, vp, vp, vp, vp]),
    "hgs_param_forward_bytes": (sz, []),
    "hgs_params_forward": (ci, [vp, ci, vp, vp]),
    "hgs_params_forward_preprocess": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, cf, cf, ci, vp, vp, vp, vp, vp]),
    "hgs_hair_params_backward": (ci, [vp, ci, ci, vp, vp, vp, cf, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp]),
    "hgs_cloud_params_backward": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_loss_head_scratch_floats": (sz, [vp]),
    "hgs_loss_head_tail": (ci, [vp, vp, vp, vp]),
    "hgs_loss_head_forward": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_loss_head_backward": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp]),
    "hgs_densify_stats": (ci, [vp, ci, vp, vp, ci, vp, vp, vp]),
    "hgs_radius_pairs": (ci, [vp, ci, vp, vp, cf, cf, ci, ci, vp, vp, vp, ci]),
    "hgs_knn3": (ci, [vp, ci, vp, vp, vp]),
    "hgs_nearest_distance_f64": (ci, [vp, ci, ci, vp, vp, vp]),
    "hgs_magnet_scratch_bytes": (sz, [ci, ci]),
    "hgs_magnet_forward": (ci, [vp, ci, ci, vp, vp, vp, vp, cf, vp, sz, vp, vp, vp, vp, vp]),
    "hgs_magnet_backward": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, sz, vp]),
    "hgs_set_magnet_search": (ci, [ci]),
    "hgs_pointcloud_normals_scratch_bytes": (sz, [ci, ci]),
    "hgs_pointcloud_normals": (ci, [vp, ci, ci, vp, vp, vp, vp, sz]),
    "hgs_strand_walk_ends": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp]),
    "hgs_strand_walk_fill": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_strand_grow_plan": (ci, [vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, cf, vp, vp, vp]),
    "hgs_strand_grow_fill": (ci, [vp, ci, vp, vp, vp, ci, vp, vp, vp, ci, vp, ci, cf, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp,
                                  vp, vp]),
    "hgs_strand_arclen": (ci, [vp, ci, vp, vp, C.c_longlong, vp, ci, vp, vp, vp]),
    "hgs_strand_resample": (ci, [vp, ci, vp, vp, vp, C.c_longlong, vp, ci, vp, ci, ci, vp, ci, vp, ci, vp, C.c_longlong, vp, vp]),
    "hgs_groom_neighbours": (ci, [vp, ci, vp, ci, ci, vp, ci, C.c_double, C.c_double, vp, vp, vp, vp]),
    "hgs_groom_blend": (ci, [vp, ci, ci, ci, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp]),
    "hgs_undistort_images": (ci, [vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci]),
    "hgs_rescale_images": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp, ci]),
    "hgs_rescale_orientation": (ci, [vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp]),
    "hgs_carve_view_bytes": (sz, []),
    "hgs_carve_votes": (ci, [vp, C.c_longlong, vp, ci, vp, vp, vp, vp, vp, vp]),
    "hgs_carve_grid": (ci, [vp, vp, C.c_double, ci, ci, ci, ci, vp, vp, ci, ci, vp]),
    "hgs_carve_shell": (ci, [vp, ci, ci, ci, vp, vp]),
    "hgs_lift_moments": (ci, [vp, C.c_longlong, vp, ci, vp, vp, vp, vp, vp, vp, C.c_double, ci, vp, vp, vp]),
    "hgs_lift_solve": (ci, [vp, C.c_longlong, vp, vp, ci, vp, vp]),
    "hgs_lift_moments_gated": (ci, [vp, C.c_longlong, vp, ci, vp, vp, vp, vp, vp, vp, C.c_double, ci, vp, ci, vp, vp, vp]),
    "hgs_hull_visibility": (ci, [vp, C.c_longlong, vp, ci, vp, vp, vp, C.c_double, ci, ci, ci, ci, ci, vp]),
    "hgs_scalp_depth": (ci, [vp, ci, vp, ci, vp, ci, vp, vp, vp]),
    "hgs_scalp_votes": (ci, [vp, C.c_longlong, vp, vp, ci, vp, vp, vp, C.c_double, C.c_double, vp, vp]),
    "hgs_mesh_sdf": (ci, [vp, ci, vp, C.c_double, C.c_double, C.c_double, C.c_double, ci, ci, ci, vp, vp]),
    "hgs_head_penalty_num_blocks": (ci, [ci]),
    "hgs_head_penalty_forward": (ci, [vp, ci, vp, vp, ci, ci, ci, cf, cf, cf, cf, cf, vp, vp, vp, vp, vp]),
    "hgs_head_penalty_backward": (ci, [vp, ci, vp, vp, vp]),
    "hgs_direction_loss_num_blocks": (ci, [ci]),
    "hgs_direction_loss_forward": (ci, [vp, ci, vp, vp, vp, ci, ci, ci, cf, cf, cf, cf, cf, vp, vp, vp, vp, vp]),
    "hgs_direction_loss_backward": (ci, [vp, ci, ci, vp, vp, vp, vp, vp]),
    "hgs_strand_collide": (ci, [vp, ci, vp, C.c_longlong, vp, vp, ci, ci, ci, cf, cf, cf, cf, cf, cf, ci, vp, vp, vp]),
    "hgs_root_attach": (ci, [vp, ci, vp, C.c_longlong, vp, vp, ci, ci, ci, cf, cf, cf, cf, vp, vp, ci, ci, ci, C.c_double, C.c_double,
                             C.c_double, C.c_double, C.c_double, cf, cf, C.c_double, ci, ci, C.c_double, C.c_double, C.c_double, vp, vp, vp,
                             vp]),
    "hgs_strand_rejoin": (ci, [vp, ci, vp, C.c_longlong, vp, vp, ci, vp, ci, vp, vp, ci, vp, C.c_longlong, vp, vp]),
    "hgs_strand_smooth": (ci, [vp, ci, vp, C.c_longlong, vp, ci, ci, C.c_double, C.c_double, ci, C.c_double, vp, vp, vp]),
    "hgs_strand_simplify": (ci, [vp, ci, vp, C.c_longlong, vp, ci, C.c_double, vp, vp, vp]),
    "hgs_guides_assign": (ci, [vp, ci, ci, ci, C.c_longlong, vp, vp, ci, vp, vp, vp, vp, vp]),
    "hgs_guides_update": (ci, [vp, ci, ci, ci, C.c_longlong, vp, ci, vp, C.c_longlong, vp, vp, vp]),
    "hgs_guides_pick": (ci, [vp, ci, ci, vp, C.c_longlong, vp, vp, vp]),
    "hgs_dedupe_count": (ci, [vp, ci, ci, C.c_longlong, vp, C.c_double, vp]),
    "hgs_dedupe_fill": (ci, [vp, ci, ci, C.c_longlong, vp, C.c_double, vp, C.c_longlong, vp]),
    "hgs_dedupe_resolve": (ci, [vp, ci, vp, C.c_longlong, vp, vp, vp, ci, vp, vp, vp]),
    "hgs_field_splat": (ci, [vp, ci, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, ci, ci, ci, C.c_double, vp, vp]),
    "hgs_field_solve": (ci, [vp, ci, ci, ci, vp, vp, vp]),
    "hgs_strand_trace": (ci, [vp, ci, vp, vp, vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, ci, ci, ci, C.c_double, ci,
                              C.c_double, C.c_double, ci, vp, vp, vp]),
    "hgs_field_fill": (ci, [vp, ci, ci, ci, vp, vp, ci, vp, vp, ci]),
    "hgs_oriented_match_scratch_bytes": (sz, [ci]),
    "hgs_oriented_match": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, sz]),
    "hgs_strand_votes": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, vp, vp, ci, vp, vp, vp]),
    "hgs_orientation_scratch_bytes": (sz, [ci, ci, ci, ci, ci]),
    "hgs_orientation_field": (ci, [vp, ci, ci, ci, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz]),
    "hgs_orientation_confidence": (ci, [vp, ci, ci, ci, vp, vp, vp]),
    "hgs_view_stats_num_blocks": (ci, [ci, ci]),
    "hgs_view_stats": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, cf, vp, vp, vp, vp, cf, vp, vp]),
    "hgs_raster_model_bytes": (sz, []),
    "hgs_raster_vertex_bytes": (sz, []),
    "hgs_raster_tiles": (ci, [ci, ci]),
    "hgs_raster_vertices": (ci, [vp, ci, ci, ci, ci, vp, vp, vp, vp]),
    "hgs_raster_count": (ci, [vp, ci, ci, ci, ci, vp, C.c_longlong, vp, ci, vp, vp, vp]),
    "hgs_raster_fill": (ci, [vp, ci, ci, ci, ci, vp, C.c_longlong, vp, ci, vp, vp, vp, vp, vp]),
    "hgs_raster_resolve": (ci, [vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hgs_set_segment_policy": (ci, [ci, ci, ci]),
    "hgs_debug_set_wg_trace": (ci, [vp, vp]),
    "hgs_prof_enable": (ci, [ci]),
    "hgs_prof_bracket_overhead_ms": (C.c_double, []),
    "hgs_prof_collect": (ci, [vp, vp]),
    "hgs_prof_kernel_name": (C.c_char_p, [ci]),
    "hgs_geom_layout": (ci, [ci, vp]),
    "hgs_image_layout": (ci, [ci, ci, vp]),
    "hgs_binning_layout": (ci, [ci, vp]),
}
GEOM_FIELDS = ["depths", "clamped", "means2D", "cov3D", "conic_opacity", "rgb", "tiles_touched", "point_offsets", "rect",
               "block_sums"]
IMG_FIELDS = ["final_T", "n_contrib", "ranges", "tile_count", "tile_cursor", "tile_maxc", "status", "tile_order"]
BIN_FIELDS = ["keys", "point_list", "packed", "inv", "keys_sorted"]
PACKED_FLOATS = 12
INST_GRAD_FLOATS = 12


class HgsError(RuntimeError):
    pass


class ViewTargets(C.Structure):
    """include/hgs.h HgsViewTargets (184 bytes)."""
    _fields_ = [("image", vp), ("float_mask", vp), ("orientation", vp), ("confidence", vp), ("mask", vp),
                ("viewmatrix", cf * 16), ("projmatrix", cf * 16), ("campos", cf * 3), ("mask_count", cf)]


class HeadParams(C.Structure):
    """include/hgs.h HgsHeadParams."""
    _fields_ = [("H", ci), ("W", ci), ("lambda_dssim", cf), ("lambda_mask", cf), ("lambda_orientation", cf),
                ("lambda_smooth", cf), ("bg", cf * 3), ("min_val", cf), ("window", cf * 11), ("n_smooth", ci),
                ("cos_threshold", cf), ("eps", cf), ("n_endpoints", ci), ("defer_tail", ci), ("tile_used", vp),
                ("tiles_x", ci), ("tiles_y", ci)]


class HeadTail(C.Structure):
    """include/hgs.h HgsHeadTail."""
    _fields_ = [("pix_partials", vp), ("nb_pix", ci), ("out", vp), ("inv_hw", cf), ("l_mask", cf), ("l_ori", cf),
                ("l_smooth", cf), ("bce", ci), ("ori", ci), ("smooth", ci)]


class Prologue(C.Structure):
    """include/hgs.h HgsPrologue."""
    _fields_ = [("table", vp), ("view", ci), ("slot", vp), ("lr", cf), ("lr_dst", vp), ("zero_ptr", vp), ("zero_bytes", sz),
                ("adam_prep", vp)]


ADAM_MAX_TENSORS = 8


class AdamSlot(C.Structure):
    """include/hgs.h HgsAdamSlot."""
    _fields_ = [("p", vp), ("m", vp), ("v", vp), ("coef", vp)]


class AdamPrep(C.Structure):
    """include/hgs.h HgsAdamPrep (lives in device memory: built here, uploaded as bytes)."""
    _fields_ = [("n", ci), ("lr", vp * ADAM_MAX_TENSORS), ("step", vp * ADAM_MAX_TENSORS), ("beta1", cf), ("beta2", cf), ("coef", vp)]


class RasterModel(C.Structure):
    """include/hgs.h HgsRasterModel (an array of them lives in device memory: built here, uploaded as bytes)."""
    _fields_ = [("draw_base", C.c_longlong), ("idx_offset", C.c_longlong), ("n_prims", ci), ("kind", ci), ("width", ci), ("lit", ci),
                ("ka", C.c_double), ("kd", C.c_double)]


class CarveView(C.Structure):
    """include/hgs.h HgsCarveView (152 bytes; an array of them lives in device memory: built by utils/carve.py, uploaded as bytes)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("W", C.c_int32), ("H", C.c_int32), ("mask_offset", C.c_int64), ("image_offset", C.c_int64)]


_CARVE_VIEW = np.dtype(CarveView)   # (a numpy view of a record array: _planes)


class AdamInline(C.Structure):
    """include/hgs.h HgsAdamInline."""
    _fields_ = [("slot", AdamSlot * 6), ("beta1", cf), ("beta2", cf), ("eps", cf)]


class StrandFusion(C.Structure):
    """include/hgs.h HgsStrandFusion."""
    _fields_ = [("smooth_pairs", vp), ("n_smooth", ci), ("cos_threshold", cf), ("eps", cf), ("smooth_partials", vp),
                ("smooth_pair_grads", vp), ("head_out", vp), ("grad_out", vp), ("radii", vp), ("dmean2D", vp), ("dmean2D_stride", ci),
                ("max_radii2D", vp), ("grad_accum", vp), ("denom", vp), ("ep_segments", vp), ("ep_pairs", vp),
                ("n_endpoints", ci), ("head_tail", HeadTail), ("prologue", Prologue)]


class ParamForward(C.Structure):
    """include/hgs.h HgsParamForward."""
    _fields_ = [("kind", ci), ("endpoints", vp), ("endpoint_pairs", vp), ("width", vp), ("dist_to_scale_factor", cf),
                ("scaling_raw", vp), ("rotation_raw", vp), ("opacity_raw", vp), ("mask_raw", vp), ("means3D", vp), ("scale", vp),
                ("quat", vp), ("opacity", vp), ("extra4", vp)]


class ParamBackward(C.Structure):
    """include/hgs.h HgsParamBackward."""
    _fields_ = [("kind", ci), ("endpoints", vp), ("endpoint_pairs", vp), ("dist_to_scale_factor", cf), ("seg_contrib", vp),
                ("d_width", vp), ("rotation_raw", vp), ("d_means3D", vp), ("d_scaling_raw", vp), ("d_rotation_raw", vp),
                ("extra4", vp), ("d_opacity_raw", vp), ("d_mask_raw", vp), ("dL_dmeans2D_rgb", vp), ("max_radii2D", vp),
                ("grad_accum", vp), ("denom", vp), ("head_tail", HeadTail), ("adam", AdamInline)]


class BlockPlan(C.Structure):
    """include/hgs.h HgsBlockPlan."""
    _fields_ = [("n_chunks", ci), ("chunks", vp), ("ep_list", vp), ("n_segments", ci), ("n_endpoints", ci), ("ep_segments", vp),
                ("ep_pairs", vp), ("smooth_pair_grads", vp), ("n_smooth", ci), ("head_out", vp), ("grad_out", vp),
                ("d_endpoints", vp), ("ep_adam", AdamSlot), ("beta1", cf), ("beta2", cf), ("eps", cf)]


PARAMS_HAIR, PARAMS_CLOUD = 1, 2
HEAD_SKIP_PIXELS, HEAD_SKIP_SMOOTH = 1, 2
VIEW_QUEUE_MAX = 16   # include/hgs.h HGS_VIEW_QUEUE_MAX
DEDUPE_PARTS = 8      # include/hgs.h HGS_DEDUPE_PARTS
HEAD_OUT = ["total", "l1", "dssim", "mask", "orientation", "smooth", "ori_count", "smooth_count", "g_ssim", "g_l1", "g_mask",
            "g_ori", "g_smooth", "total_fwd"]
HEAD_NOUT = 16
FUSED_PREPROCESS_MAX_TILES = 8192   # include/hgs.h HGS_FUSED_PREPROCESS_MAX_TILES
ABI_VERSION = 15   # include/hgs.h HGS_ABI_VERSION: bumped whenever a struct, a signature or a buffer layout changes


def build(verbose=False):
    """Compile csrc/*.hip into libhgs.so for gfx950 (no GPU needed)."""
    subprocess.check_call(["make", "-s", "-j8", "-C", CSRC], stdout=None if verbose else subprocess.DEVNULL)
    import c_utils
    c_utils.build()   # the host-side native helper (CPython extension, gcc)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HgsError(f"{LIB_PATH} not found: run hgs_runtime.build() (hipcc --offload-arch=gfx950). "
                           "There is no CPU fallback.")
        # torch first: its wheel carries its own libamdhip64; the process must end up with ONE HIP runtime, and it has to
        # be the one that owns the tensors' memory.  Loading libhgs.so before torch binds it to /opt/rocm's copy, and a
        # later kernel launch on torch's memory then fails with "no ROCm-capable device is detected".
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        # a stale library called through newer struct layouts corrupts memory: refuse it (version AND struct sizes)
        if L.hgs_abi_version() != ABI_VERSION:
            raise HgsError(f"{LIB_PATH}: ABI version {L.hgs_abi_version()}, this binding needs {ABI_VERSION}: "
                           "rebuild with hgs_runtime.build()")
        for fn, st in (("hgs_view_targets_bytes", ViewTargets), ("hgs_head_params_bytes", HeadParams),
                       ("hgs_strand_fusion_bytes", StrandFusion), ("hgs_param_forward_bytes", ParamForward),
                       ("hgs_param_backward_bytes", ParamBackward), ("hgs_block_plan_bytes", BlockPlan),
                       ("hgs_adam_prep_bytes", AdamPrep), ("hgs_adam_inline_bytes", AdamInline),
                       ("hgs_raster_model_bytes", RasterModel), ("hgs_carve_view_bytes", CarveView)):
            if getattr(L, fn)() != C.sizeof(st):
                raise HgsError(f"{LIB_PATH}: {fn}() = {getattr(L, fn)()} but the binding's struct has {C.sizeof(st)} bytes: "
                               "rebuild with hgs_runtime.build()")
        _lib = L
    return _lib


def check(status):
    if status != 0:
        raise HgsError(lib().hgs_last_error().decode())


def ptr(t):
    """Device pointer of a tensor; None / empty tensors map to NULL (the reference passes 0-element tensors)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def current_stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_gpu_tensor(t, name, dtype=None):
    import torch
    if not t.is_cuda:
        raise HgsError(f"{name} must be a CUDA(HIP) tensor: libhgs.so only runs on the GPU, there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise HgsError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def require_device_buffer(t, name, dtype):
    """A contiguous device tensor of `dtype`, as it is: nothing is copied or converted on the way to a kernel."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HgsError(f"{name} must be a CUDA(HIP) tensor: libhgs.so only runs on the GPU, there is no CPU path")
    if t.dtype != dtype:
        raise HgsError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise HgsError(f"{name} must be contiguous")
    return t


def _planes(records):
    """[(mask_offset, W, H, image_offset)] of the view records as plain integers, read once through a numpy view of the array: a
    field of a ctypes record costs far more than the comparison it feeds, and these checks run in front of every launch."""
    a = np.frombuffer(records, dtype=_CARVE_VIEW)
    return list(zip(a["mask_offset"].tolist(), a["W"].tolist(), a["H"].tolist(), a["image_offset"].tolist()))


def _planes_inside(planes, buf, what, where):
    """Every view's plane, W*H elements from its mask_offset, lies inside the device buffer `buf`; the refusal names the plane
    (`what`) and the buffer (`where`)."""
    n = buf.numel()
    for k, (offset, W, H, _) in enumerate(planes):
        if offset < 0 or offset + W * H > n:
            raise HgsError(f"view {k}: its {what} (offset {offset}, {W} x {H}) does not lie inside the {where}")


def _carve_planes(records, views_dev, masks, images):
    """carve_check; returns _planes(records) for the checks that extend it."""
    import torch
    V = len(records)
    if not 1 <= V <= 4096:
        raise HgsError(f"{V} views (1 to 4096)")
    require_device_buffer(views_dev, "views", torch.uint8)
    require_device_buffer(masks, "masks", torch.uint8)
    if images is not None:
        require_device_buffer(images, "images", torch.uint8)
    if views_dev.numel() != V * C.sizeof(CarveView):
        raise HgsError(f"the view buffer holds {views_dev.numel()} bytes, {V} views take {V * C.sizeof(CarveView)}")
    planes = _planes(records)
    for k, (_, W, H, _) in enumerate(planes):
        if W < 1 or H < 1:
            raise HgsError(f"view {k}: {W} x {H} pixels")
    _planes_inside(planes, masks, "mask", f"mask buffer of {masks.numel()} bytes")
    for k, (_, W, H, image_offset) in enumerate(planes):
        if image_offset >= 0 and (images is None or image_offset + 3 * W * H > images.numel()):
            raise HgsError(f"view {k}: its image (offset {image_offset}, {W} x {H} x 3) does not lie inside the image buffer")
    return planes


def carve_check(records, views_dev, masks, images=None):
    """What hgs_carve_* may not be called without (include/hgs.h): `records`, the host copy (a CarveView array) of the view records in
    views_dev, name a mask -- and, where image_offset >= 0, an image -- that lies inside its buffer; every buffer is a contiguous
    uint8 device tensor.  Returns the number of views."""
    return len(_carve_planes(records, views_dev, masks, images))


def lift_check(records, views_dev, masks, orients, confs, tab, images=None, visible=None, N=None):
    """What hgs_lift_moments may not be called without (include/hgs.h): carve_check's guarantee for the masks, extended to the
    orientation and confidence buffers (addressed by the same mask_offset), and a float64 table of 256 x 2 entries.  `images`: the
    image buffer of records that name one (the lift does not read it).  `visible` (hgs_lift_moments_gated): the word buffer, an
    int32 device tensor of exactly [N, ceil(V/32)].  Returns the number of views."""
    import torch
    planes = _carve_planes(records, views_dev, masks, images)
    for name, buf in (("orients", orients), ("confs", confs)):
        require_device_buffer(buf, name, torch.uint8)
        _planes_inside(planes, buf, "plane", f"{name} buffer of {buf.numel()} bytes")
    require_device_buffer(tab, "tab", torch.float64)
    if tab.numel() != 512:
        raise HgsError(f"the sine / cosine table holds {tab.numel()} values, 256 x 2 expected")
    if visible is not None:
        _words_check(visible, N, len(planes))
    return len(planes)


def _words_check(visible, N, V):
    """The visibility words of N points and V views: a contiguous int32 device tensor [N, ceil(V/32)]."""
    import torch
    require_device_buffer(visible, "visible", torch.int32)
    if tuple(visible.shape) != (int(N), (V + 31) // 32):
        raise HgsError(f"visible of shape {tuple(visible.shape)}: [{int(N)}, {(V + 31) // 32}] expected for {V} views")


def visibility_check(shape, occ, points, centres, visible):
    """What hgs_hull_visibility trusts beyond its own argument checks, in front of every launch: occ is a contiguous uint8 device tensor
    of exactly the grid's voxels, points and centres float64 [N, 3] and [V, 3], visible int32 [N, ceil(V/32)].  Returns (N, V)."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if min(nx, ny, nz) < 1 or max(nx, ny, nz) > 1024:
        raise HgsError(f"a grid of {nx} x {ny} x {nz} voxels (1 to 1024 per axis)")
    require_device_buffer(occ, "occ", torch.uint8)
    if occ.numel() != nx * ny * nz:
        raise HgsError(f"occ holds {occ.numel()} bytes, a grid of {nx} x {ny} x {nz} voxels takes {nx * ny * nz}")
    for t, name in ((points, "points"), (centres, "centres")):
        require_device_buffer(t, name, torch.float64)
        if t.dim() != 2 or t.shape[1] != 3:
            raise HgsError(f"{name} of shape {tuple(t.shape)}: [{'N' if name == 'points' else 'V'}, 3] expected")
    N, V = points.shape[0], centres.shape[0]
    if not 1 <= V <= 4096:
        raise HgsError(f"{V} views (1 to 4096)")
    _words_check(visible, N, V)
    return N, V


def scalp_check(records, views_dev, masks, depth, faces=None, n_verts=None):
    """What hgs_scalp_* may not be called without (include/hgs.h): carve_check's guarantee for the masks, extended to the float64 depth
    buffer (addressed by the same mask_offset, in elements), views of fewer than 2^31 pixels and, with `faces` (an int32 device tensor
    [F, 3]), indices inside the n_verts vertices.  Returns the number of views."""
    import torch
    planes = _carve_planes(records, views_dev, masks, None)
    require_device_buffer(depth, "depth", torch.float64)
    for k, (_, W, H, _) in enumerate(planes):
        if W * H >= 1 << 31:
            raise HgsError(f"view {k}: {W} x {H} pixels (fewer than 2^31)")
    _planes_inside(planes, depth, "depth map", f"depth buffer of {depth.numel()} values")
    if faces is not None:
        require_device_buffer(faces, "faces", torch.int32)
        if faces.numel() and (int(faces.min()) < 0 or int(faces.max()) >= int(n_verts)):
            raise HgsError(f"a face index is out of range of the {n_verts} vertices")
    return len(planes)


def trace_check(acc=None, shape=None, skipped=None, dir=None, conf=None):
    """What the hgs_field_* / hgs_strand_trace kernels trust beyond their own argument checks: the node arrays they index by the grid's
    shape are contiguous device tensors of exactly that many nodes."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > 1024 or nx * ny * nz > (1 << 26):
        raise HgsError(f"a grid of {nx} x {ny} x {nz} nodes (2 to 1024 an axis, at most 2^26 in all)")
    nodes = nx * ny * nz
    for t, name, dtype, per in ((acc, "acc", torch.int64, 7), (skipped, "skipped", torch.int32, None), (dir, "dir", torch.float64, 3),
                                (conf, "conf", torch.float64, 1)):
        if t is None:
            continue
        require_device_buffer(t, name, dtype)
        want = 1 if per is None else nodes * per
        if t.numel() != want:
            raise HgsError(f"{name} holds {t.numel()} values, a grid of {nx} x {ny} x {nz} nodes takes {want}")


def fill_check(shape, kind, a, b, free_index):
    """What hgs_field_fill trusts beyond its own argument checks: kind, a and b are contiguous device tensors of exactly the grid's
    nodes (a and b six planes of them, two buffers), and free_index is an int32 device tensor of node indices in range.  Returns F."""
    import torch
    nx, ny, nz = (int(n) for n in shape)
    if min(nx, ny, nz) < 2 or max(nx, ny, nz) > 1024 or nx * ny * nz > (1 << 26):
        raise HgsError(f"a grid of {nx} x {ny} x {nz} nodes (2 to 1024 an axis, at most 2^26 in all)")
    nodes = nx * ny * nz
    for t, name, dtype, per in ((kind, "kind", torch.uint8, 1), (a, "a", torch.float64, 6), (b, "b", torch.float64, 6)):
        require_device_buffer(t, name, dtype)
        if t.numel() != nodes * per:
            raise HgsError(f"{name} holds {t.numel()} values, a grid of {nx} x {ny} x {nz} nodes takes {nodes * per}")
    if a.data_ptr() == b.data_ptr():
        raise HgsError("a and b are one buffer: the sweep reads one and writes the other")
    require_device_buffer(free_index, "free_index", torch.int32)
    F = free_index.numel()
    if free_index.dim() != 1 or F > nodes:
        raise HgsError(f"free_index of shape {tuple(free_index.shape)}: [F] with F at most the {nodes} nodes expected")
    if F and (int(free_index.min()) < 0 or int(free_index.max()) >= nodes):
        raise HgsError(f"a free index is out of range of the {nodes} nodes")
    return F


KERNEL_COUNT = 18


def prof_enable(on=True):
    lib().hgs_prof_enable(int(bool(on)))


def prof_collect():
    """{kernel name: (total_ms, launches)} since the last collect (synchronises the recorded events)."""
    ms = (C.c_double * KERNEL_COUNT)()
    n = (C.c_longlong * KERNEL_COUNT)()
    check(lib().hgs_prof_collect(ms, n))
    return {lib().hgs_prof_kernel_name(i).decode(): (ms[i], n[i]) for i in range(KERNEL_COUNT)}


def layout(kind, *dims):
    n = {"geom": len(GEOM_FIELDS), "image": len(IMG_FIELDS), "binning": len(BIN_FIELDS)}[kind]
    arr = (C.c_size_t * n)()
    getattr(lib(), f"hgs_{kind}_layout")(*dims, arr)
    names = {"geom": GEOM_FIELDS, "image": IMG_FIELDS, "binning": BIN_FIELDS}[kind]
    return dict(zip(names, list(arr)))
