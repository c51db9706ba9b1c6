/*
 * hgs.h -- C ABI of libhgs.so, the MI355X (gfx950) rasterizer + distCUDA2 library.
 *
 * This is the drop-in boundary for the reference's native layer.  Every entry point names the
 * reference interface it replaces (paths relative to /root/reference/submodules/):
 *
 *   hgs_forward_preprocess + hgs_forward_render
 *        <-> RasterizeGaussiansCUDA            diff-gaussian-rasterization/rasterize_points.cu:35-115
 *            CudaRasterizer::Rasterizer::forward  .../cuda_rasterizer/rasterizer_impl.cu:198-336
 *            (split at the one point where the reference needs `num_rendered` on the host, :280-285)
 *   hgs_backward
 *        <-> RasterizeGaussiansBackwardCUDA    diff-gaussian-rasterization/rasterize_points.cu:117-196
 *            CudaRasterizer::Rasterizer::backward .../cuda_rasterizer/rasterizer_impl.cu:340-434
 *   hgs_mark_visible
 *        <-> markVisible                       diff-gaussian-rasterization/rasterize_points.cu:198-217
 *   hgs_dist2
 *        <-> distCUDA2 / SimpleKNN::knn        simple-knn/spatial.cu:15-26, simple-knn/simple_knn.cu:186-222
 *   hgs_geom_bytes / hgs_image_bytes / hgs_binning_bytes
 *        <-> required<GeometryState|ImageState|BinningState>()  .../cuda_rasterizer/rasterizer_impl.h:67-71
 *            (the reference grows torch byte tensors through resize callbacks, rasterize_points.cu:27-33;
 *             here the caller asks for the size and allocates)
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch), fp32/int32 contiguous, unless
 *     the name ends in _host;  "absent" optional inputs are NULL (the reference passes 0-element tensors);
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work,
 *     except hgs_forward_preprocess which waits for the instance count when num_rendered_host != NULL;
 *   - return value 0 = ok, non-zero = error, message in hgs_last_error() (thread-local);
 *   - matrices are the reference's row-vector (transposed) 4x4s, read as m[0],m[4],m[8],m[12] per row
 *     (cuda_rasterizer/auxiliary.h:58-77);
 *   - the three opaque buffers play the roles of geomBuffer / imgBuffer / binningBuffer
 *     (rasterize_points.cu:72-78): written by forward, handed back unchanged to backward.
 *   - not re-entrant on the same buffers; distinct buffers + distinct streams may overlap.
 */
#ifndef HGS_H_INCLUDED
#define HGS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* bumped with every incompatible change of a struct, a signature or a buffer layout (round 1: 1, round 2: 2, round 3: 3, then 4 with the one-launch parameters + preprocess entry points;
 * 5, round 5: hgs_backward_multi_params / hgs_hair_endpoint_gather, HgsPrologue.adam_prep and the in-lane Adam update, and the contract that HgsHeadParams.tile_used also limits
 * what hgs_loss_head_forward writes of d_extra_unit -- a caller of version 4 that read those planes everywhere must not;
 * 6, round 6: tile_delta in the image buffer; 7: every image-buffer field behind tile_cursor starts on a 256-byte boundary, and a
 * misaligned HgsHeadParams.tile_used is an error of hgs_loss_head_forward; 8: hgs_strand_grow_plan / hgs_strand_grow_fill;
 * 9: tile culling, the record form and the row sums are flag bits of each call instead of process-wide setters, and one render,
 * backward and size function each serves 3 and 7 channels; 10: hgs_pointcloud_normals / hgs_pointcloud_normals_scratch_bytes;
 * 11: one parameter-source struct for the forward, HgsParamForward; 12: hgs_strand_arclen / hgs_strand_resample; 13: hgs_magnet_*;
 * 14: hgs_undistort_images; 15: hgs_carve_votes / hgs_carve_grid / hgs_carve_shell and HgsCarveView);
 * the Python binding refuses a library whose version or struct sizes differ from its own */
#define HGS_ABI_VERSION 15
#define HGS_TILE 16 /* cuda_rasterizer/config.h:16-17 */

int hgs_abi_version(void);
const char* hgs_last_error(void);

/* ---- workspace sizes (bytes).  Layout is private; hgs_*_layout() exposes it for tests.  `channels`: 3, or 7 for the
 * single-pass mode (n_extra = 4, hgs_forward_render); any other value gives 0. ---- */
size_t hgs_geom_bytes(int P);
size_t hgs_image_bytes(int W, int H);
size_t hgs_binning_bytes(int R, int channels);
size_t hgs_backward_scratch_bytes(int P, int R, int channels);

/* Forward, part 1: per-Gaussian preprocess (cull, cov3D, EWA cov2D, conic, radius, tile rect, SH->RGB)
 * + per-tile instance counts + scans.  Writes radii[P].  If num_rendered_host != NULL the call blocks
 * until R = num_rendered is known and stores it there (reference: rasterizer_impl.cu:280-281);
 * with NULL nothing blocks and R stays on the device (pass a capacity to hgs_forward_render).
 * max_rendered (device, may be NULL): raised atomically to R -- a sticky maximum over all calls since the caller last
 * cleared it, which is what a captured HIP graph needs to validate its capacity after any number of replays without a
 * per-iteration device-to-host copy.  With num_rendered_host == NULL and max_rendered != NULL the scans are left to the
 * scatter kernel of hgs_forward_render (no one-workgroup scan launch in between): R and its maximum are then on the
 * device once THAT call has run on the stream; max_rendered has to stay valid until then.
 * prefiltered: bit 0 = the reference's flag (accepted, ignored); bit 1 (HGS_IMAGE_PREZEROED) = the caller has already
 * cleared the counters of image_buf on this stream (hgs_iteration_prologue over hgs_image_zero_range): the call's own
 * clearing launch is skipped; bit 2 (HGS_COUNT_ROW_RUNS) = count the tile rectangles of more than 16 tiles by their tile
 * ROWS (two marks per row, which the pass's scan turns into counts) instead of tile by tile: the same counts; pays
 * where Gaussians cover many tiles each (a Stage-I cloud at 1080p, a merged strand
 * model: callers set it from the instances per Gaussian they have seen -- diff_gaussian_rasterization/_C.py); bit 3
 * (HGS_TILE_CULL) = tile culling, below. */
#define HGS_IMAGE_PREZEROED 2
#define HGS_COUNT_ROW_RUNS 4
/* Tile culling.  The reference gives every Gaussian the tiles of its 3-sigma square (forward.cu:229-235, auxiliary.h:46-56)
 * although a pixel only blends it where opacity * exp(power) >= 1/255 (forward.cu:358): with HGS_TILE_CULL the preprocess keeps
 * only the tiles that the bounding box of that ellipse reaches, so num_rendered, the tile lists and n_contrib count fewer
 * entries than the reference's -- the dropped ones are skipped by every pixel there too.  out_color, radii and final_T are
 * bit-identical with and without; so are the gradients, except those of Gaussians whose wavefront of the per-Gaussian backward
 * streams its rows (one of its 64 Gaussians has more than 32 instances) or whose rows row_reduce_kernel sums (HGS_ROWS_REDUCE):
 * there the terms are the same, associated differently.  (Tiles whose list is long enough to be blended in segments,
 * hgs_set_segment_policy, associate their transmittance products per segment: there image and gradients agree to rounding.)
 * Without the bit the lists are the reference's exactly (the parity tests of the binning stages use that).  The backward
 * takes no such bit: the buffers carry the rectangles. */
#define HGS_TILE_CULL 8
/* Value a max_rendered word takes when a workgroup of a pass gave up waiting for another one of the same launch (bounded
 * spins of the list-parallel sort / blend: never observed; would mean the dispatcher kept a predecessor from running).
 * The frame of that pass is invalid. */
#define HGS_WAIT_TIMED_OUT 0xFFFFFFFFu
int hgs_forward_preprocess(void* stream, int P, int D, int M, int W, int H,
                           const float* means3D, const float* shs, const float* colors_precomp,
                           const float* opacities, const float* scales, float scale_modifier,
                           const float* rotations, const float* cov3D_precomp,
                           const float* viewmatrix, const float* projmatrix, const float* campos,
                           float tan_fovx, float tan_fovy, int prefiltered,
                           void* geom_buf, void* image_buf, int* radii, int* num_rendered_host,
                           unsigned int* max_rendered);

/* Forward, part 2: instance scatter (tile binning), per-tile depth sort, front-to-back blend.
 * `R_capacity` = number of instances binning_buf was sized for (== num_rendered in the blocking mode).
 * n_extra = 0: bg is [3], out_color [3,H,W].  n_extra = 4, the single-pass mode: RGB + 4 extra unclamped
 * per-Gaussian channels `extra` [P,4] (16-byte aligned; the reference's mask value and world-space direction) composited with
 * the same weights in ONE traversal -- what the reference obtains from three separate render() calls per iteration
 * (train.py:146, loss/losses.py:247 and :312); bg and out_color then have 7 channels.  Workspaces are sized for 3 + n_extra
 * channels.  flags: how the blend kernels of the pass (and of its backward) get the per-entry records --
 * HGS_RECORDS_PACKED: the sort kernel writes a 48- / 64-byte record per instance which they stream (rounds 1-5);
 * HGS_RECORDS_LAZY: the sort kernel orders keys only and they build an entry's record from its Gaussian's template through the
 * sorted key (nothing is written for the entries behind a tile's last contributor: two thirds of a dense Stage-I frame's);
 * neither: lazy for passes with at least 128 entries per tile by R_capacity.  Images and gradients are the same bits either way.
 * Fails (status in hgs_read_status) if the scene needs more than R_capacity. */
#define HGS_RECORDS_PACKED 16
#define HGS_RECORDS_LAZY 32
int hgs_forward_render(void* stream, int P, int W, int H, int R_capacity, int n_extra, int flags,
                       const float* bg, const float* colors_precomp, const float* extra,
                       void* geom_buf, void* binning_buf, void* image_buf, float* out_color);

/* Backward of a pass of hgs_forward_render with the same n_extra.  bg == NULL means a BLACK background (the same gradients as a
 * zero vector; the background terms of the blend backward are compiled out -- what a training step on a black background,
 * train.py:94, should pass).  dL_dpix_planes is a HOST array of 3 + n_extra device pointers, one [H,W] gradient plane per
 * output channel (the planes need not be adjacent: the losses produce them separately).
 * All gradient outputs are fully written by the call (zeros for culled Gaussians):
 * the caller does not need to zero-fill them (reference zero-allocates, rasterize_points.cu:151-159).
 * dL_dextra is [P,4] (NULL when n_extra is 0); dL_dconic is [P,2,2] (element [1,0] is written as 0); dL_dmeans2D is [P,3]
 * (z = 0), the screen-space gradient of the RGB channels alone (the only one the reference's densification statistics see);
 * dL_dmeans3D uses all channels.  `scratch` >= hgs_backward_scratch_bytes(P, R, 3 + n_extra) bytes.  viewmatrix, projmatrix
 * and campos are REQUIRED whatever the colour source (the kernel reads them at entry; NULL is refused).
 * flags, with n_extra = 4 (ignored otherwise): the per-Gaussian sums of the instance rows are taken inside the per-Gaussian
 * launch -- whose wavefronts wait for their longest Gaussian -- (HGS_ROWS_INLINE) or by a launch of their own that is balanced
 * by ROWS (HGS_ROWS_REDUCE; csrc/hgs_preprocess.hip row_reduce_kernel: runs of 512 rows per wavefront, whatever Gaussians they
 * belong to): what a pass with many instances per Gaussian wants (a Stage-I cloud at 1080p, the merged strand model: 4 - 12 x
 * faster); neither: the launch where R >= 8 P.  R is the caller's argument -- in capacity mode a CAPACITY, not a count --, so
 * a caller that wants the choice to follow the model rather than its capacity sets a bit itself (the Python layer does: from
 * the instance counts of the warm-up passes of a capture, diff_gaussian_rasterization._C.set_row_reduce).  The same terms
 * either way, associated differently (rounding); every form is a fixed sequence of additions for a given pass. */
#define HGS_ROWS_INLINE 64
#define HGS_ROWS_REDUCE 128
int hgs_backward(void* stream, int P, int D, int M, int R, int W, int H, int n_extra, int flags, const float* bg,
                 const float* means3D, const float* shs, const float* colors_precomp,
                 const float* scales, float scale_modifier, const float* rotations,
                 const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                 const float* campos, float tan_fovx, float tan_fovy, const int* radii,
                 const void* geom_buf, const void* binning_buf, const void* image_buf,
                 const float* const* dL_dpix_planes, void* scratch, float* dL_dextra,
                 float* dL_dmeans2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolors,
                 float* dL_dmeans3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscales,
                 float* dL_drotations);

/* present[i] = (view-space z > 0.2)   (cuda_rasterizer/rasterizer_impl.cu:54-66) */
int hgs_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix,
                     const float* projmatrix, uint8_t* present);

/* distCUDA2: out[i] = mean of the 3 smallest squared distances from point i to the other points. */
size_t hgs_dist2_scratch_bytes(int P);
int hgs_dist2(void* stream, int P, const float* points, float* out, void* scratch, size_t scratch_bytes);

/* ---- MI355X-native fusions of PyTorch-side work ON the training-step path.  The reference has
 * no native counterpart: it runs these as chains of small torch kernels.  Every pointer is a device pointer except
 * `window11_host` (the 11 normalised fp32 taps of the Gaussian window, host memory).
 *
 * hgs_ssim_l1_forward/backward <-> loss/losses.py:16-17 (l1_loss) + :43-84 (ssim: five grouped 11x11 conv2d) and
 *   their autograd.  forward writes 3*C*H*W floats of derivative maps + 2 floats per 32x32 block and channel
 *   (hgs_ssim_l1_num_blocks of them)
 *   (partial sums of the SSIM map and of |img1-img2|; the caller sums them and divides by C*H*W).
 *   backward: dL_dimg1 = g_ssim_mean/(CHW) * dSSIM/dimg1 + g_l1_mean/(CHW) * sign(img1-img2), g_* device scalars.
 * hgs_strand_geometry_forward/backward <-> scene/hair_gaussian_model.py:134-201 getters (get_xyz, get_scaling,
 *   get_rotation, get_orientation) + utils/transform.py:69-86, and their autograd (gather / Rodrigues /
 *   matrix_to_quaternion / scatter-add into shared endpoints).  endpoint_pairs is int64 [P,2] as torch stores it.
 *   backward: any of g_xyz/g_scale/g_quat/g_dir may be NULL (output unused); d_endpoints [E,3] is zeroed inside. ---- */
size_t hgs_ssim_l1_scratch_floats(int C, int H, int W);
int hgs_ssim_l1_num_blocks(int C, int H, int W);
int hgs_ssim_l1_forward(void* stream, int C, int H, int W, const float* window11_host, const float* img1,
                        const float* img2, float* dmaps, float* partials);
int hgs_ssim_l1_backward(void* stream, int C, int H, int W, const float* window11_host, const float* img1,
                         const float* img2, const float* dmaps, const float* g_ssim_mean, const float* g_l1_mean,
                         float* dL_dimg1);
/* hgs_orientation_loss_forward/backward <-> loss/losses.py:250-288 (everything after the orientation render):
 *   omap [3,H,W] rendered world-space directions; viewmatrix = world_view_transform [4,4] (device; rows 0-2, cols 0-1 used);
 *   mask uint8 [H,W] or NULL (then mask = any(omap != bg3_host)); partials: 2 floats per 256-pixel block
 *   (sum of diff*confidence over the mask, mask count); loss = sum0 / sum1.  backward: g_loss, mask_count are
 *   device scalars; d_omap [3,H,W] fully written. */
int hgs_orientation_loss_num_blocks(int H, int W);
int hgs_orientation_loss_forward(void* stream, int H, int W, const float* omap, const float* viewmatrix,
                                 const float* bg3_host, float min_val, const float* gt_theta, const float* confidence,
                                 const uint8_t* mask, float* partials);
int hgs_orientation_loss_backward(void* stream, int H, int W, const float* omap, const float* viewmatrix,
                                  const float* bg3_host, float min_val, const float* gt_theta, const float* confidence,
                                  const uint8_t* mask, const float* g_loss, const float* mask_count, float* d_omap);
/* hgs_adam_step <-> torch.optim.Adam(lr=0, eps=1e-15) as built at scene/gaussian_model.py:250 and
 *   scene/hair_gaussian_model.py:246: all parameter tensors (<= 8) updated by ONE launch.  The six arrays are HOST arrays
 *   of n_tensors DEVICE pointers; lr[k] and step[k] point to fp32 device scalars (step is incremented by the call, by
 *   the workgroup that takes the tensor's last ticket).  tickets: 8 uint32 words in device memory owned by the optimizer,
 *   zero before its first step (they return to zero at the end of every completed launch; an optimizer whose launch was
 *   aborted zeroes them again).  NULL: process-wide words -- all such calls must then be stream-ordered.
 * hgs_smoothness_forward/backward <-> loss/losses.py:175-221 angle_smoothness_loss: index_pairs is the int64 [N,2,2]
 *   table of consecutive strand segments (endpoint ids); partials: 2 floats per 256 pairs (sum of squared angles of the
 *   pairs bent more than the threshold, their count); loss = sum0 / max(sum1, 1).  backward zeroes d_endpoints [E,3]
 *   and scatters with fp32 atomics (order-dependent in the last bits). */
int hgs_adam_step(void* stream, int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, const float* const* lr, float* const* step, const long long* numel,
                  float beta1, float beta2, float eps, unsigned int* tickets);
int hgs_smoothness_num_blocks(int N);
int hgs_smoothness_forward(void* stream, int N, const float* endpoints, const long long* index_pairs,
                           float cos_threshold, float eps, float* partials);
int hgs_smoothness_backward(void* stream, int N, int E, const float* endpoints, const long long* index_pairs,
                            float cos_threshold, float eps, const float* g_loss, const float* count, float* d_endpoints);
int hgs_strand_geometry_forward(void* stream, int P, const float* endpoints, const long long* endpoint_pairs,
                                const float* width, float dist_to_scale_factor, float* xyz, float* scale, float* quat,
                                float* dir);
int hgs_strand_geometry_backward(void* stream, int P, int E, const float* endpoints, const long long* endpoint_pairs,
                                 const float* width, float dist_to_scale_factor, const float* g_xyz, const float* g_scale,
                                 const float* g_quat, const float* g_dir, float* d_endpoints, float* d_width);

/* ---- the strand-Gaussian training iteration as a handful of launches -------------------------
 * The reference runs everything between the model parameters and the rasterizer, and between the rendered images and
 * the scalar loss, as ~60 small PyTorch kernels per iteration (train.py:135-168, loss/losses.py:224-355,
 * scene/hair_gaussian_model.py:134-201,1401-1408).  On MI355X those launches, not the math, bound the step; the
 * entry points below do the same arithmetic in one kernel per stage.
 *
 * HgsViewTargets: one training view's targets, resident in HBM for the whole run (288 GB holds every view of a capture
 *   session).  The loss-head kernels read it from DEVICE memory, so a captured HIP graph switches views by rewriting
 *   this one struct (hgs_select_view) instead of copying ~50 MB of images into a staging slot.  viewmatrix /
 *   projmatrix / campos are stored by value in the layout the reference's Camera holds them (world_view_transform,
 *   full_proj_transform: row-major, transposed; scene/cameras.py:59-62), so `&slot->viewmatrix[0]` is a valid
 *   `viewmatrix` argument of the rasterizer entry points. */
typedef struct HgsViewTargets {
  const float* image;           /* [3,H,W] ground-truth RGB (Camera.original_image) */
  const float* float_mask;      /* [H,W] mask as floats, BCE target (Camera.float_mask); NULL: no mask term */
  const float* orientation;     /* [H,W] ground-truth strand angle in [0,pi) (Camera.orientation_field) */
  const float* confidence;      /* [H,W] (Camera.orientation_confidence) */
  const unsigned char* mask;    /* [H,W] bool mask of the orientation term (Camera.mask); NULL: any(omap != bg) */
  float viewmatrix[16];
  float projmatrix[16];
  float campos[3];
  float mask_count;             /* number of set pixels of `mask` (0: unknown / no mask); lets the orientation term's
                                   gradient be formed in the forward pass */
} HgsViewTargets;
size_t hgs_view_targets_bytes(void);   /* sizeof(HgsViewTargets), for bindings that mirror the struct */
size_t hgs_head_params_bytes(void);    /* sizeof(HgsHeadParams) */
size_t hgs_strand_fusion_bytes(void);  /* sizeof(HgsStrandFusion) */
/* ---- Adam in the backward's own lanes (round 5; one rank).  The lane of the backward that has just finished the gradient of a
 * parameter element -- hgs_backward_multi_params' per-Gaussian lanes, hgs_hair_endpoint_gather's endpoint lanes -- applies that
 * element's Adam update at once (HgsAdamSlot: parameter, both moments, the step's two coefficients); an iteration then has no
 * optimizer launch.  The coefficients lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) and the advance of the step counters t are the
 * business of the iteration's PROLOGUE (HgsPrologue.adam_prep: one thread per tensor of a DEVICE-resident HgsAdamPrep), i.e. of
 * a launch in front of every kernel that reads them.  Same arithmetic as hgs_adam_step, bit for bit (csrc/hgs_adam.h): a run
 * may mix iterations of either form.  The gradients are written as without it. ---- */
#define HGS_ADAM_MAX_TENSORS 8
typedef struct HgsAdamSlot { float* p; float* m; float* v; const float* coef; } HgsAdamSlot;   /* p == NULL: not updated here */
typedef struct HgsAdamPrep {                     /* lives in DEVICE memory */
  int n; const float* lr[HGS_ADAM_MAX_TENSORS]; float* step[HGS_ADAM_MAX_TENSORS]; float beta1, beta2;
  float* coef;                                   /* [n][2] out: step_size, inv_sqrt_bc2 of tensor k (HgsAdamSlot.coef = coef + 2 k) */
} HgsAdamPrep;
/* slots by HgsParamBackward.kind -- HGS_PARAMS_HAIR: 0 width, 1 opacity, 2 mask, 3 SH DC ([P,1,3]);  HGS_PARAMS_CLOUD: 0 xyz,
 * 1 scaling, 2 rotation, 3 opacity, 4 mask, 5 SH DC;  hgs_hair_endpoint_gather: 0 endpoints */
typedef struct HgsAdamInline { HgsAdamSlot slot[6]; float beta1, beta2, eps; } HgsAdamInline;
size_t hgs_adam_prep_bytes(void);     /* sizeof(HgsAdamPrep) */
size_t hgs_adam_inline_bytes(void);   /* sizeof(HgsAdamInline) */

/* slot[0] = table[view]; if lr_dst != NULL also *lr_dst = lr (the position learning rate of this iteration, a by-value
 * kernel argument, so the host may run ahead of the device without racing on a staging buffer). */
int hgs_select_view(void* stream, const HgsViewTargets* table, int view, HgsViewTargets* slot, float lr, float* lr_dst);
/* Iteration prologue: hgs_select_view and, in the same launch, the clearing of zero_bytes bytes at zero_ptr -- meant for
 * the counters at the head of the image buffer of the coming hgs_forward_preprocess (range: hgs_image_zero_range; pass
 * HGS_IMAGE_PREZEROED to that call so that it does not clear them again).  One launch instead of three small ones in
 * front of every iteration. */
int hgs_iteration_prologue(void* stream, const HgsViewTargets* table, int view, HgsViewTargets* slot, float lr, float* lr_dst,
                           void* zero_ptr, size_t zero_bytes, const HgsAdamPrep* adam_prep /* NULL: none */);
int hgs_image_zero_range(int W, int H, size_t* offset, size_t* bytes);   /* of an image_buf of hgs_image_bytes(W, H) */
/* The same prologue as a rider of another launch: hgs_params_forward -- the first launch of
 * an iteration, which needs neither the view nor the counters -- run it in spare workgroups when HgsStrandFusion.prologue
 * is filled in (table != NULL): no launch of its own in front of the iteration (4 us of a 290 us iteration).  The graph
 * functions below find and re-point such a rider exactly like a stand-alone prologue launch. */
typedef struct HgsPrologue {
  const HgsViewTargets* table; int view; HgsViewTargets* slot; float lr; float* lr_dst;   /* as hgs_iteration_prologue */
  void* zero_ptr; size_t zero_bytes;
  const HgsAdamPrep* adam_prep;   /* NULL: none (see HgsAdamSlot) */
} HgsPrologue;
/* A captured HIP graph that holds exactly ONE hgs_iteration_prologue / hgs_select_view launch is re-pointed at another
 * view (and learning rate) without any launch between two replays: hgs_graph_find_prologue(hipGraph_t) returns that
 * kernel node once after the capture, hgs_graph_set_prologue(hipGraphExec_t, node, ...) rewrites its arguments (host
 * work only; takes effect at the next launch of the executable graph). */
int hgs_graph_find_prologue(void* graph, void** node_out);
/* several iterations captured in one graph: all its prologue nodes (any order) with the `lr` each was captured with, which
 * the caller uses as a tag to tell them apart */
int hgs_graph_find_prologues(void* graph, int max_nodes, void** nodes_out, float* lr_out, int* n_out);
/* (the node's HgsPrologue.adam_prep stays what it was captured with) */
int hgs_graph_set_prologue(void* graph_exec, void* node, const HgsViewTargets* table, int view, HgsViewTargets* slot, float lr,
                           float* lr_dst, void* zero_ptr, size_t zero_bytes);
/* Several views per optimizer step inside ONE captured graph (strong-scaling protocol, SURVEY.md 8e: a fixed global batch
 * of V views per step, rank r takes views r, r+N, ...).  The graph holds one hgs_select_view_queued launch per local view,
 * which reads the view index from DEVICE memory; before every replay the host writes the step's indices (and the
 * position learning rate) with ONE hgs_set_view_queue launch whose values are by-value kernel arguments (n <=
 * HGS_VIEW_QUEUE_MAX), so the host may run ahead of the device.
 *   hgs_set_view_queue:     queue[i] = views[i] (i < n), *lr_slot = lr
 *   hgs_select_view_queued: slot[0] = table[*view_index]; if lr_dst != NULL also *lr_dst = *lr_slot.  An index outside
 *                           [0, n_views) selects view 0 (a replay with an unwritten queue must not read wild memory). */
#define HGS_VIEW_QUEUE_MAX 16
int hgs_set_view_queue(void* stream, int* queue, int n, const int* views_host, float lr, float* lr_slot);
int hgs_select_view_queued(void* stream, const HgsViewTargets* table, int n_views, const int* view_index,
                           HgsViewTargets* slot, const float* lr_slot, float* lr_dst);

/* The tail of the loss head's reduction (hgs_loss_head_forward, below): the sums over the per-pixel kernel's partials
 *   and what depends on them --
 *   out[HGS_HEAD_MASK], out[HGS_HEAD_ORIENTATION], out[HGS_HEAD_ORI_COUNT] and the last three terms of out[HGS_HEAD_TOTAL]
 *   (every other entry of `out`, and total's first two terms, are written by the forward's own kernels).  The forward runs
 *   it as a one-workgroup launch of its own -- 5.7 us on the iteration's critical path -- unless HgsHeadParams.defer_tail is
 *   set: then `out` is complete only once a later launch has run the tail in a spare workgroup: hgs_hair_params_backward /
 *   hgs_cloud_params_backward do when HgsStrandFusion.head_tail is filled in (hgs_loss_head_tail), and
 *   hgs_loss_head_backward runs it first itself when its per-pixel pass needs out[HGS_HEAD_ORI_COUNT] (no
 *   HGS_HEAD_SKIP_PIXELS).  Same arithmetic either way: the values do not depend on who runs the tail. */
typedef struct HgsHeadTail {
  const float* pix_partials; int nb_pix;   /* [nb_pix][3]: orientation sum, orientation count, mask BCE sum */
  float* out;                              /* NULL: none */
  float inv_hw, l_mask, l_ori, l_smooth;
  int bce, ori, smooth;
} HgsHeadTail;

/* hgs_params_forward (HGS_PARAMS_HAIR) / hgs_hair_params_backward: hgs_strand_geometry_* plus the appearance activations of the same Gaussians
 *   (scene/gaussian_model.py:93-99 get_opacity / get_mask = sigmoid) and the 4 extra blended channels of the
 *   single-pass rasterizer, extra4 = [sigmoid(mask_raw), dir.xyz].  backward: g_extra4 [P,4] carries the gradient of
 *   the mask channel and of the direction (added to g_dir); `opacity`/`extra4` are the forward outputs;
 *   accumulate_endpoints != 0: d_endpoints is NOT zeroed first (it already holds the smoothness gradient). */
/* Optional work folded into the two launches (host struct, NULL = none): extra workgroups evaluate the smoothness term
 * over the same endpoints (forward: partial sums in the layout of hgs_smoothness_forward; backward: its gradient scattered
 * into d_endpoints, scaled by head_out[HGS_HEAD_G_SMOOTH] * *grad_out / max(head_out[HGS_HEAD_SMOOTH_COUNT], 1)), and the
 * backward also updates the densification statistics of hgs_densify_stats for its Gaussians.  Any group whose first
 * pointer is NULL is skipped. */
typedef struct HgsStrandFusion {
  const long long* smooth_pairs; int n_smooth; float cos_threshold, eps;
  float* smooth_partials;                          /* forward out */
  float* smooth_pair_grads;                        /* optional, [n_smooth][2][4]: forward out -- the pairs' unit gradients (g0, ok),
                                                      (g1, ok) -- and hgs_hair_endpoint_gather in: its endpoint lanes then read 16
                                                      bytes per pair role instead of evaluating the pair again (same bits) */
  const float* head_out; const float* grad_out;    /* backward in (device) */
  const int* radii; const float* dmean2D; int dmean2D_stride;   /* backward in: statistics inputs */
  float* max_radii2D; float* grad_accum; float* denom;          /* backward in/out */
  /* backward, gather mode: adjacency of the endpoints.  ep_segments [E][2]: 2 * segment + (0|1 = which end of it), -1 =
   * none; ep_pairs [E][4]: 4 * smoothness pair + role (0..3 = a0, a1, b0, b1), -1 = none.  When ep_segments is given,
   * d_endpoints is written with ONE plain store per endpoint (one extra workgroup range recomputes the adjacent segments'
   * and pairs' contributions): no float atomics, bitwise reproducible, and accumulate_endpoints is ignored. */
  const int* ep_segments; const int* ep_pairs; int n_endpoints;
  HgsHeadTail head_tail;   /* backward: out != NULL -> one spare workgroup of the launch runs the loss head's deferred tail */
  HgsPrologue prologue;    /* forward: table != NULL -> spare workgroups of the launch run the iteration prologue */
} HgsStrandFusion;
/* The model's raw parameters behind the Gaussians of a pass, for the launches that derive them -- the forward counterpart of
 * HgsParamBackward (below), with the same `kind`. */
enum { HGS_PARAMS_HAIR = 1, HGS_PARAMS_CLOUD = 2 };
typedef struct HgsParamForward {
  int kind;                                                                /* HGS_PARAMS_HAIR | HGS_PARAMS_CLOUD */
  const float* endpoints; const long long* endpoint_pairs; const float* width; float dist_to_scale_factor;   /* hair: in */
  const float* scaling_raw; const float* rotation_raw;                     /* cloud: in ([P,4] rotation: 16-byte aligned for the one-launch form) */
  const float* opacity_raw; const float* mask_raw;                         /* in [P] */
  /* the derived Gaussians: means3D [P,3] hair: out, cloud: the model's own parameter, in;  scale [P,3], quat [P,4], opacity [P],
   * extra4 [P,4]: out (quat / extra4: 16-byte aligned for the one-launch form) */
  float* means3D; float* scale; float* quat; float* opacity; float* extra4;
} HgsParamForward;
size_t hgs_param_forward_bytes(void);    /* sizeof(HgsParamForward) */
/* parameters -> Gaussians in one launch (strand_fwd_kernel / cloud_fwd_kernel by `kind`; the cloud form is described at
 *   hgs_cloud_params_backward and uses only the prologue group of `fusion`).  The segments' direction alone: hgs_strand_geometry_forward. */
int hgs_params_forward(void* stream, int P, const HgsParamForward* params, const HgsStrandFusion* fusion);
/* hgs_params_forward_preprocess: hgs_params_forward AND hgs_forward_preprocess of the same model as ONE launch
 *   (the iteration's first: every lane derives its Gaussian -- written to means3D (hair) / scale / quat / opacity / extra4 for
 *   the backward and the render entry points, bit-identical to hgs_params_forward's -- and preprocesses it from
 *   registers; SH colours only, scale_modifier 1).  Capacity mode only (max_rendered as in hgs_forward_preprocess; no
 *   blocking count), at most 8192 tiles.  `flags`: HGS_IMAGE_PREZEROED as in hgs_forward_preprocess.  The riders of
 *   `fusion` (smoothness partial sums, HgsPrologue; a cloud: the prologue group only) run BESIDE the preprocess workgroups, hence
 *   two rules:
 *     - viewmatrix / projmatrix / campos are read from fusion->prologue.table[view] when a prologue rides (the slot is being
 *       written by that very launch; the three pointers are used only without a prologue);
 *     - the prologue's zero range must start BEHIND the per-tile instance counters (hgs_image_layout: from
 *       HGS_IMG_TILE_CURSOR on): those must already be zero when the launch starts, which every pass of
 *       hgs_forward_render in capacity mode leaves behind (its scan clears what it has read); after a pass in blocking mode,
 *       or on a buffer of unknown content, run hgs_iteration_prologue with the full range of hgs_image_zero_range first. */
#define HGS_FUSED_PREPROCESS_MAX_TILES 8192
int hgs_params_forward_preprocess(void* stream, int P, int D, int M, int W, int H, const HgsParamForward* params, const float* shs,
                                  const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                  float tan_fovy, int flags, void* geom_buf, void* image_buf, int* radii,
                                  unsigned int* max_rendered, const HgsStrandFusion* fusion);
int hgs_hair_params_backward(void* stream, int P, int E, const float* endpoints, const long long* endpoint_pairs,
                             const float* width, float dist_to_scale_factor, const float* opacity, const float* extra4,
                             const float* g_xyz, const float* g_scale, const float* g_quat, const float* g_dir,
                             const float* g_opacity, const float* g_extra4, int accumulate_endpoints,
                             float* d_endpoints, float* d_width, float* d_opacity_raw, float* d_mask_raw,
                             const HgsStrandFusion* fusion);

/* ---- hgs_backward_multi_params: the BACKWARD mirror of hgs_params_forward_preprocess (round 5).
 *   hgs_backward (n_extra 4) whose last per-Gaussian launch also applies the backward of the derivation parameters -> Gaussian, in the
 *   lane that has just finished the Gaussian's gradients (they never travel through memory):
 *     HGS_PARAMS_HAIR   what hgs_hair_params_backward's per-segment lanes compute -- d_width, d_opacity_raw, d_mask_raw, the
 *                       densification statistics -- and, in seg_contrib [P][2][4 floats], the gradient of the segment's first and
 *                       second endpoint (xyz, pad).  hgs_hair_endpoint_gather then sums, per endpoint, its (<= 2) segments'
 *                       contributions and (<= 4) smoothness-pair roles with one plain store (HgsStrandFusion.ep_segments /
 *                       ep_pairs are required: gather mode only) and runs the loss head's deferred tail if one is given.
 *     HGS_PARAMS_CLOUD  everything hgs_cloud_params_backward computes (d_means3D = the rasterizer's dL_dmeans3D); a deferred tail
 *                       (head_tail.out != NULL) rides in a spare workgroup of the launch.  No second launch.
 *   Results are those of hgs_backward (n_extra 4) + hgs_hair_params_backward (gather mode) / hgs_cloud_params_backward bit for bit.
 *   SH colours, scale_modifier 1 (as the forward entry points).  dL_dsh [P,M,3] is written as hgs_backward writes it.
 *   flags: HGS_ROWS_* as in hgs_backward.
 *   `extra4` / `opacity`-like inputs are the FORWARD's outputs of the same pass.  Optional (NULL = skipped): dL_dmeans2D_rgb
 *   [P,3], the statistics group (max_radii2D / grad_accum / denom, all three or none). ---- */
typedef struct HgsParamBackward {
  int kind;                                                                /* HGS_PARAMS_HAIR | HGS_PARAMS_CLOUD */
  const float* endpoints; const long long* endpoint_pairs; float dist_to_scale_factor;   /* hair: in */
  float* seg_contrib; float* d_width;                                                    /* hair: out */
  const float* rotation_raw;                                                             /* cloud: in [P,4], 16-byte aligned */
  float* d_means3D; float* d_scaling_raw; float* d_rotation_raw;                         /* cloud: out */
  const float* extra4;                                                     /* in: the forward's [P,4] (mask channel first) */
  float* d_opacity_raw; float* d_mask_raw;                                 /* out [P] */
  float* dL_dmeans2D_rgb;                                                  /* out [P,3], optional */
  float* max_radii2D; float* grad_accum; float* denom;                     /* in/out [P], optional (hgs_densify_stats) */
  HgsHeadTail head_tail;                                                   /* cloud: out != NULL -> a spare workgroup runs the tail */
  HgsAdamInline adam;                                                      /* slots with p != NULL: updated by the lane (see HgsAdamSlot) */
} HgsParamBackward;
size_t hgs_param_backward_bytes(void);   /* sizeof(HgsParamBackward) */
int hgs_backward_multi_params(void* stream, int P, int D, int M, int R, int W, int H, int flags, const float* bg7,
                              const float* means3D, const float* shs, const float* scales, const float* rotations,
                              const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                              float tan_fovy, const int* radii, const void* geom_buf, const void* binning_buf, const void* image_buf,
                              const float* const* dL_dpix_planes7, void* scratch, float* dL_dsh, const HgsParamBackward* params);
/* ---- hgs_backward_multi_params_planned (HGS_PARAMS_HAIR): hgs_backward_multi_params AND hgs_hair_endpoint_gather as ONE launch.
 *   The gather is a launch of its own only because an endpoint's two segments may sit in different workgroups of the per-Gaussian
 *   launch.  A BLOCK PLAN cuts the segments into chunks that own whole strands: workgroup c takes the segments
 *   [s0, s0 + ns) (storage order, 1 <= ns <= 256) and the ne <= 256 endpoints ep_list[e0 .. e0 + ne); every segment and every
 *   endpoint belongs to exactly one chunk, and every segment an endpoint's ep_segments codes name lies in that endpoint's chunk.
 *   The segments' contributions then meet in LDS: behind one workgroup barrier lane t sums endpoint ep_list[e0 + t] exactly as
 *   hgs_hair_endpoint_gather does (segment codes 0, 1, then pair roles 0..3), stores d_endpoints and applies the endpoint's Adam
 *   update (ep_adam.p != NULL).  No workgroup waits for another one; seg_contrib is neither written nor read (it may be NULL).
 *   The barrier also orders the lanes' reads of the endpoints in front of that update, and nothing behind it reads an endpoint:
 *   the pairs' gradients arrive precomputed, i.e. a smoothness term (n_smooth > 0 with ep_pairs) REQUIRES smooth_pair_grads.
 *   A deferred loss-head tail (params->head_tail.out != NULL) rides in one spare workgroup behind the chunks.
 *   Results against the two launches: the endpoint sums, the parameter arithmetic and the Adam updates are the same operations in
 *   the same order, so the results are the two launches' BIT FOR BIT wherever the per-Gaussian row sums are -- with
 *   HGS_ROWS_REDUCE (row_reduce_kernel knows no wavefronts of Gaussians), and with the rows summed in the launch as long as no
 *   wavefront streams its rows (no Gaussian with more than 32 instances: fresh strands).  The plan changes which 64 segments
 *   form a wavefront, and with it which wavefronts stream and where a Gaussian's rows fall in the streamed run: on such a pass
 *   the row sums of those wavefronts hold the same terms associated differently (as HGS_TILE_CULL above), the two forms agree
 *   to that rounding -- every gradient of those Gaussians, their endpoints' and the Adam state behind them --, and each form
 *   remains a fixed sequence of additions for a given pass (bitwise reproducible).  chunks / ep_list are DEVICE tables whose contents the host cannot see:
 *   the kernel clamps what it reads from them to the model's sizes, but a table that breaks the rules above gives wrong
 *   gradients.  plan == NULL: hgs_backward_multi_params.  A plan whose sizes, pointers or alignment are wrong is an error. ---- */
typedef struct HgsBlockPlan {
  int n_chunks;                         /* > 0 */
  const int* chunks;                    /* [n_chunks][4] = s0, ns, e0, ne; 16-byte aligned */
  const int* ep_list;                   /* [n_endpoints]: the chunks' endpoint ids, chunk after chunk */
  int n_segments, n_endpoints;          /* what the chunks cover: n_segments must be the call's P */
  const int* ep_segments;               /* [n_endpoints][2] as HgsStrandFusion.ep_segments; 8-byte aligned */
  const int* ep_pairs;                  /* [n_endpoints][4] as HgsStrandFusion.ep_pairs, or NULL; 16-byte aligned */
  const float* smooth_pair_grads;       /* [n_smooth][2][4] as HgsStrandFusion.smooth_pair_grads; 16-byte aligned */
  int n_smooth;                         /* 0: no smoothness term */
  const float* head_out; const float* grad_out;   /* the smoothness scale's inputs, as HgsStrandFusion (n_smooth > 0) */
  float* d_endpoints;                   /* out [n_endpoints][3] */
  HgsAdamSlot ep_adam;                  /* p != NULL: the endpoint lanes apply the update, with the betas / eps below */
  float beta1, beta2, eps;
} HgsBlockPlan;
size_t hgs_block_plan_bytes(void);   /* sizeof(HgsBlockPlan) */
int hgs_backward_multi_params_planned(void* stream, int P, int D, int M, int R, int W, int H, int flags, const float* bg7,
                                      const float* means3D, const float* shs, const float* scales, const float* rotations,
                                      const float* viewmatrix, const float* projmatrix, const float* campos, float tan_fovx,
                                      float tan_fovy, const int* radii, const void* geom_buf, const void* binning_buf,
                                      const void* image_buf, const float* const* dL_dpix_planes7, void* scratch, float* dL_dsh,
                                      const HgsParamBackward* params, const HgsBlockPlan* plan);
/* d_endpoints [E,3] fully written.  fusion: ep_segments (required), ep_pairs + the smoothness group (smooth_pairs, n_smooth,
 * cos_threshold, eps, head_out, grad_out) and head_tail as for hgs_hair_params_backward; its other groups are ignored. */
/* adam (may be NULL): slot 0 = the endpoints' Adam state; the lane then also applies endpoint i's update (HgsAdamSlot).  With a
 * smoothness term this requires fusion->smooth_pair_grads (no lane may read an endpoint while others update them: refused otherwise). */
int hgs_hair_endpoint_gather(void* stream, int E, const float* seg_contrib, const float* endpoints, float* d_endpoints,
                             const HgsStrandFusion* fusion, const HgsAdamInline* adam);

/* hgs_params_forward (HGS_PARAMS_CLOUD) / hgs_cloud_params_backward: the Stage-I counterpart of the strand forms -- the rasterizer-facing getters of the
 *   Gaussian cloud (scene/gaussian_model.py:118-157) and their autograd in one launch each:
 *   scale = exp(scaling_raw); quat = rotation_raw / max(|rotation_raw|, 1e-12) (F.normalize); opacity / mask = sigmoid;
 *   direction = column argmax(scale) of build_rotation(rotation_raw) (get_orientation: the longest axis in world space);
 *   extra4 = [mask, direction].  backward: g_scale / g_quat / g_opacity / g_extra4 are the rasterizer's gradients;
 *   `fusion` may carry the densification-statistics group of HgsStrandFusion (its smoothness group is ignored). */
int hgs_cloud_params_backward(void* stream, int P, const float* scaling_raw, const float* rotation_raw,
                              const float* opacity, const float* extra4, const float* g_scale, const float* g_quat,
                              const float* g_opacity, const float* g_extra4, float* d_scaling_raw, float* d_rotation_raw,
                              float* d_opacity_raw, float* d_mask_raw, const HgsStrandFusion* fusion);

/* hgs_loss_head_forward/backward <-> loss/losses.py:319-355 loss_function on the three rendered images:
 *   total = (1-l_dssim) L1 + l_dssim (1-SSIM) + l_mask BCEWithLogits(mask_img, float_mask) + l_orientation ORI
 *           + l_smooth SMOOTH(endpoints),  terms with weight 0 (or a NULL target) skipped.
 *   forward: 4 launches (SSIM/L1 map, BCE + orientation per pixel, smoothness per segment pair, one-block reduction);
 *   out[HGS_HEAD_*] device floats.  scratch: hgs_loss_head_scratch_floats() floats, kept for the backward.
 *   d_extra_unit ([4,H,W]: mask plane, then the 3 orientation planes; may be NULL): if given, the per-pixel pass also
 *   writes dL/d(mask_img) and dL/d(omap) FOR grad_out = 1 (requires targets->mask_count > 0 when the orientation term
 *   is on, since that gradient is normalised by the mask count); a caller whose upstream gradient is exactly 1 then
 *   passes HGS_HEAD_SKIP_PIXELS to the backward and uses those planes as they are.  With HgsHeadParams.tile_used given the
 *   planes are UNWRITTEN on the 16 x 16 tiles that are not read (ABI 5).
 *   smooth_partials_ext (may be NULL): smoothness partial sums already computed elsewhere (HgsStrandFusion): the head then
 *   launches no smoothness kernel of its own and reduces these.
 *   backward: d_image [3,H,W] fully written (but see HgsHeadParams.tile_used); d_mask_img [H,W], d_omap [3,H,W] fully written unless HGS_HEAD_SKIP_PIXELS;
 *   d_endpoints [E,3] zeroed, then (unless HGS_HEAD_SKIP_SMOOTH) the smoothness gradient scattered into it;
 *   grad_out = device scalar dL/dtotal. */
enum { HGS_HEAD_SKIP_PIXELS = 1, HGS_HEAD_SKIP_SMOOTH = 2 };
typedef struct HgsHeadParams {
  int H, W;
  float lambda_dssim, lambda_mask, lambda_orientation, lambda_smooth;
  float bg[3];                  /* background of the orientation render (loss/losses.py:249: black) */
  float min_val;                /* HairGaussianModel.min_val */
  float window[11];             /* SSIM window taps */
  int n_smooth;                 /* rows of the smoothness index table */
  float cos_threshold, eps;     /* loss/losses.py:175: threshold 30 deg, eps 1e-6 */
  int n_endpoints;
  int defer_tail;               /* != 0: the forward leaves the sums over the per-pixel partials (see HgsHeadTail) to the caller */
  /* Optional hint (NULL: none): tile_used[ty * tiles_x + tx] != 0 <=> the consumer of d_image reads the 16 x 16 tile
   * (tx, ty).  For the rasterizer backward that is the image buffer's per-tile contributor count (hgs_image_layout,
   * HGS_IMG_TILE_MAXC) of the forward pass that produced `image`: it touches dL/dpixel only where a pixel blended an entry.
   * With the hint, hgs_loss_head_backward leaves d_image UNWRITTEN on 32 x 32 blocks none of whose tiles is read (it
   * neither filters nor zero-fills them), and hgs_loss_head_forward leaves d_extra_unit UNWRITTEN on the tiles that are
   * not read.  The hint must be 16-byte aligned (HGS_IMG_TILE_MAXC is): hgs_loss_head_forward fails otherwise. */
  const unsigned int* tile_used; int tiles_x, tiles_y;
} HgsHeadParams;
enum { HGS_HEAD_TOTAL = 0, HGS_HEAD_L1, HGS_HEAD_DSSIM, HGS_HEAD_MASK, HGS_HEAD_ORIENTATION, HGS_HEAD_SMOOTH,
       HGS_HEAD_ORI_COUNT, HGS_HEAD_SMOOTH_COUNT, HGS_HEAD_G_SSIM, HGS_HEAD_G_L1, HGS_HEAD_G_MASK, HGS_HEAD_G_ORI,
       HGS_HEAD_G_SMOOTH, HGS_HEAD_TOTAL_FWD, HGS_HEAD_NOUT = 16 };
/* (HGS_HEAD_TOTAL_FWD: total's first two terms -- what the tail, HgsHeadTail, starts from) */
size_t hgs_loss_head_scratch_floats(const HgsHeadParams* p);
/* fills `tail` for the forward that used (p, scratch, out) */
int hgs_loss_head_tail(const HgsHeadParams* p, const float* scratch, float* out, HgsHeadTail* tail);
int hgs_loss_head_forward(void* stream, const HgsHeadParams* p, const float* image, const float* mask_img,
                          const float* omap, const HgsViewTargets* targets, const float* endpoints,
                          const long long* smooth_pairs, float* scratch, float* out, float* d_extra_unit,
                          const float* smooth_partials_ext);
int hgs_loss_head_backward(void* stream, const HgsHeadParams* p, const float* image, const float* mask_img,
                           const float* omap, const HgsViewTargets* targets, const float* endpoints,
                           const long long* smooth_pairs, const float* scratch, const float* out,
                           const float* grad_out, int skip, float* d_image, float* d_mask_img,
                           float* d_omap, float* d_endpoints);

/* hgs_densify_stats <-> scene/hair_gaussian_model.py:1401-1408 / gaussian_model.py:675-682 add_densification_stats +
 *   train.py:170-171 max_radii2D update, for the Gaussians with radii > 0:
 *   max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |dL_dmean2D.xy|; denom += 1.
 *   dL_dmean2D has `stride` floats per Gaussian (3 as the rasterizer returns it). */
int hgs_densify_stats(void* stream, int P, const int* radii, const float* dL_dmean2D, int stride, float* max_radii2D,
                      float* xyz_gradient_accum, float* denom);

/* ---- per-kernel device timing (bench.py roofline): when enabled every kernel launch of the library is bracketed
 * by hipEvents recorded on the launch stream.  hgs_prof_collect() synchronises those events, ADDS elapsed
 * milliseconds / launch counts per kernel id into the caller's arrays (length HGS_K_COUNT) and clears the log.
 * Enabling calibrates the fixed cost of an event pair with empty kernels once; every reading has it subtracted.
 * No reference counterpart (the reference only times whole iterations, train.py:81-82,133,156). ---- */
enum { HGS_K_PREPROCESS_FWD = 0, HGS_K_SCAN, HGS_K_SCATTER, HGS_K_SORT_TILES, HGS_K_BLEND_FWD, HGS_K_BLEND_BWD,
       HGS_K_PREPROCESS_BWD, HGS_K_KNN, HGS_K_SSIM_FWD, HGS_K_SSIM_BWD, HGS_K_STRAND_FWD, HGS_K_STRAND_BWD,
       HGS_K_ORI_FWD, HGS_K_ORI_BWD, HGS_K_ADAM, HGS_K_SMOOTH, HGS_K_HEAD, HGS_K_MISC, HGS_K_COUNT };
int hgs_prof_enable(int on);
double hgs_prof_bracket_overhead_ms(void);   /* calibrated cost of one event pair, subtracted from every reading */
int hgs_prof_collect(double* total_ms, long long* launches);
const char* hgs_prof_kernel_name(int kernel_id);

/* hgs_radius_pairs <-> the candidate search of strand merging, scipy cKDTree(pos).query_pairs(r) + the direction test at
 *   scene/hair_gaussian_model.py:1205-1290: all index pairs a < b of the N strand ends with
 *   |pos_a - pos_b| <= radius and -(dir_a . dir_b) >= min_cos (|.| instead if bidirectional).  Brute force, one
 *   256-point tile against all others through LDS: strand ends number in the thousands, where N^2/2 distance tests cost
 *   tens of microseconds and no tree has to be built or kept consistent with the moving endpoints.  sorted_by_x != 0: the
 *   caller passes the points in ascending order of x, and a block stops at the first tile that starts more than `radius`
 *   beyond its own last point (a model late in training has 10^5 strand ends within a few hundred radii of each other:
 *   52 ms -> 1 ms).
 *   Appends (a, b) to pairs[capacity][2] and the distance to dist[capacity] in unspecified order; *count (device, must be
 *   zero on entry) ends as the number of pairs FOUND, which may exceed capacity (the excess is dropped). */
int hgs_radius_pairs(void* stream, int N, const float* pos, const float* dir, float radius, float min_cos,
                     int bidirectional, int capacity, int* pairs, float* dist, int* count, int sorted_by_x);

/* hgs_knn3 <-> pytorch3d.ops.knn_points(p, p, K=3, return_sorted=True) as strand_joints_magnet_loss calls it on the strand
 *   ends (loss/losses.py:139-144; pytorch3d is a from-source dependency of the reference, README.md:25-30, absent from the tree):
 *   for every point the indices and squared distances of its 3 nearest points OF THE SAME SET, ascending, the point itself
 *   included (first, at distance 0); equal distances in ascending index order; fewer than 3 points: index -1, distance
 *   +inf.  Brute force through LDS tiles: the ends move every iteration and number in the thousands. */
int hgs_knn3(void* stream, int N, const float* points, int* idx /* [N,3] */, float* dist2 /* [N,3] */);
/* hgs_magnet_forward / hgs_magnet_backward <-> loss/losses.py strand_joints_magnet_loss (reference loss/losses.py:106-172) and its
 *   autograd, statement for statement, as a device op (csrc/hgs_magnet.hip): no allocation, no host synchronisation, no copy to
 *   the host; every launch on `stream`; launch shapes depend on n and E only, so a captured graph stays valid until the next
 *   topology event.  Host side of a topology event (hgs_runtime.fused.MagnetTable):
 *     ends[n]     int32, the degree-1 endpoint ids, ascending (torch.unique(endpoint_pairs, return_counts=True));
 *     partner[n]  int32, each end's segment partner (get_complementary_endpoint_idx);
 *     mapping[E]  int32, zero except mapping[ends[i]] = partner[i] (losses.py:137-138).
 *   Device side, every call:
 *     (a) ends whose own segment |endpoints[ends[i]] - endpoints[partner[i]]| is not longer than min_val are removed; every
 *         neighbour index below is a POSITION in that compacted list (the rank is an exclusive scan on the device);
 *     (b) the three nearest of every end, itself included, by (distance, position), distance = dx*dx + dy*dy + dz*dz in float32
 *         without contraction: the indices and distances hgs_knn3 gives on the compacted points, bit for bit; fewer than three
 *         comparable ends (or non-finite coordinates): index -1, distance +inf;
 *     (c) the second is selected unless it equals the end's own position or the GLOBAL id of the end's partner, else the third;
 *     (d) the selected position q, read as a global id, must have |endpoints[q] - endpoints[mapping[q]]| > min_val;
 *     (e) rows with a missing neighbour or a non-finite distance are left out;
 *     (f) out[0] = mean over the kept rows of the squared squared distance (the float32 products summed in float64 in a fixed
 *         order); exactly 0 when no row is kept (fewer than three valid ends among the causes);
 *     (g) d_endpoints = grad_out[0] * weight * 4 s (p - q) / m at the end, the opposite at its neighbour (s the squared distance,
 *         m the kept rows), zero everywhere else; every endpoint is written.  No float atomics: the neighbour side is a key sort
 *         of (selected position, own position) and a sum per destination in ascending order of the contributing end, so the bits
 *         are the same from run to run and under either search path.
 *   Outputs of the forward, all caller-owned, read back by the backward: out[4] (value; rows m and valid ends as int32 bits in
 *   [1], [2]), sel[n,2] (position a: the selected position or -1 when the row is not kept; the index into `ends`, -1 behind the
 *   valid ends), sq[n] (the kept rows' squared distance), nn_idx[n,3] / nn_d2[n,3] (statement (b), for tests).
 *   scratch: >= hgs_magnet_scratch_bytes(n, E) bytes (every array is per end today: E is taken for the signature's sake and does
 *   not enter the size), 256-byte aligned, private to one call at a time; the backward uses only what
 *   it writes itself, so a forward on the same scratch may run between a forward and its backward.
 * hgs_set_magnet_search: the search path of (b), process-wide: -1 automatic (by n), 0 tiles through LDS (brute force, candidate
 *   range split over workgroups for small n), 1 grid of Morton cells (the plan of hgs_dist2).  Returns the previous mode.  Both
 *   paths give identical bits in every output. */
size_t hgs_magnet_scratch_bytes(int n_ends, int n_endpoints);
int hgs_magnet_forward(void* stream, int E, int n, const float* endpoints, const int* ends, const int* partner, const int* mapping,
                       float min_val, void* scratch, size_t scratch_bytes, float* out /* [4] */, int* sel /* [n,2] */,
                       float* sq /* [n] */, int* nn_idx /* [n,3] */, float* nn_d2 /* [n,3] */);
int hgs_magnet_backward(void* stream, int E, int n, const float* endpoints, const int* ends, const int* sel, const float* sq,
                        const float* out, const float* grad_out /* device scalar */, float weight, void* scratch,
                        size_t scratch_bytes, float* d_endpoints /* [E,3] */);
int hgs_set_magnet_search(int mode);
/* hgs_nearest_distance_f64 <-> scipy cKDTree(refs).query(points, k=1)[0] as compute_strands_info uses it on the strands' ends
 *   (scene/hair_gaussian_model.py:1466-1470): out[i] = min_m |points[i] - refs[m]| in float64 (points float32 [N,3], refs
 *   float64 [M,3], M >= 1). */
int hgs_nearest_distance_f64(void* stream, int N, int M, const float* points, const double* refs, double* out);
/* hgs_pointcloud_normals <-> pytorch3d.ops.estimate_pointcloud_normals as the reference's hair and head loaders call it
 *   (data/hair_data.py:124-128, data/head_data.py:40-43); the contract is the docstring of utils/normals.py (csrc/hgs_normals.hip).
 *   points float64 [N,3] (finite: the caller checks); for every point its K nearest points of the same set, itself included, by
 *   d2 = (dx*dx + dy*dy) + dz*dz in float64, equal d2 in ascending index order; normals[i] = the unit eigenvector of the smallest
 *   eigenvalue of their covariance, negated when fewer than K / 2 neighbours q have (q - p) . n > 0; neighbors (nullable):
 *   the K indices in rank order.  1 <= K <= 64, K <= N, N <= 2^27 = 134217728 (32-bit keys and positions); N = 0 returns 0
 *   without a launch.  scratch: >= hgs_pointcloud_normals_scratch_bytes(N, K) bytes, 256-byte aligned. */
size_t hgs_pointcloud_normals_scratch_bytes(int N, int K);
int hgs_pointcloud_normals(void* stream, int N, int K, const double* points /* [N,3] */, double* normals /* [N,3] */,
                           int* neighbors /* [N,K] in rank order, or NULL */, void* scratch, size_t scratch_bytes);
/* hgs_strand_walk_ends / hgs_strand_walk_fill <-> the walk over every open polyline of the segment table in compute_strands_info
 *   (scene/hair_gaussian_model.py:1410-1498; its per-strand Python loop :1432-1464).  pairs[n][2]: endpoint ids of the segments
 *   (every id of degree 1 or 2, ids < n_ep).
 *   _ends: builds the node table (nodes: n_ep x 16 bytes of scratch, 16-byte aligned; deg[n_ep]: degrees) and walks from every
 *   chain end: other[e] = the end its chain runs into (-1 for ids that are no chain end -- which makes `other` the reference's
 *   strand_endpoint_id_to_complementary), len[e] = the chain's segment count.  flags[0] != 0 afterwards: the table is not a set of
 *   chains (an id out of range or of degree > 2); the outputs are then undefined.
 *   _fill: for the S strands the caller has numbered (starts[s] = the end the strand is stored FROM, offsets[S+1] = prefix of their
 *   lengths, flip[s] != 0 = store it in the opposite direction), writes rows[total][2] = (current, next) endpoint id of every
 *   segment in strand order, seg_rows[total] = its row of `pairs`, id_to_strand[id] = s for every endpoint on a strand (the caller
 *   pre-fills -1).  Closed loops have no end and appear nowhere, like in the reference's walk. */
int hgs_strand_walk_ends(void* stream, int n, int n_ep, const long long* pairs, int* deg, void* nodes, int* other, int* len, int* flags);
int hgs_strand_walk_fill(void* stream, int S, const long long* starts, const long long* offsets, const unsigned char* flip,
                         const void* nodes, long long* rows, long long* seg_rows, int* id_to_strand);
/* hgs_strand_grow_plan / hgs_strand_grow_fill <-> growing() of the Stage-III model (scene/hair_gaussian_model.py:1098-1200), on the
 *   strands of hgs_strand_walk_fill (offsets[S+1], rows[total][2] root -> tip, seg_rows[total]: row of the whole segment table).
 *   _plan, one lane per strand: status[s] = 1 if strand s grows, 0 if it has >= max_segments segments or every one of its last
 *   k = min(n_seg, k_avg) segments is shorter than min_val, 2 if it would grow but its tip id has deg[tip] != 1 (deg[n_deg]: segments
 *   per endpoint id over the whole table), 3 if an id of its rows is outside [0, n_ep); keep[s] bit j = row offsets[s+1] - k + j is
 *   kept (1 <= k_avg <= 32); mean_len[s] = mean length of the kept segments (numpy's float32 pairwise sum / count).
 *   _fill, one wavefront per strand, for the strands with status 1: rank[s] = exclusive prefix count of the grown strands (the
 *   caller's scan), the new row r = rank[s] is pair (tip, n_ep + r), endpoint tip + mean(d / |d|) * L (L = *length_src if
 *   length_src is not NULL, else growth_length) and the means of the kept rows' f_dc [P][3], f_rest [P][rest_floats], opacity,
 *   mask, width [P]; every value has the bits of the reference's numpy float32 arithmetic.  No atomics: deterministic. */
int hgs_strand_grow_plan(void* stream, int S, const long long* offsets, const long long* rows, const float* endpoints, int n_ep,
                         const long long* deg, int n_deg, int max_segments, int k_avg, float min_val, int* status, unsigned* keep,
                         float* mean_len);
int hgs_strand_grow_fill(void* stream, int S, const long long* offsets, const long long* rows, const long long* seg_rows, int P,
                         const int* status, const int* rank, const unsigned* keep, int k_avg, const float* endpoints, int n_ep,
                         float growth_length, const float* length_src, const float* f_dc, const float* f_rest, int rest_floats,
                         const float* opacity, const float* mask, const float* width, long long* new_pairs, float* new_endpoints,
                         float* new_f_dc, float* new_f_rest, float* new_opacity, float* new_mask, float* new_width);

/* hgs_strand_arclen / hgs_strand_resample (csrc/hgs_export.hip) <-> the strand-file export (scene/strand_export.py; the reference has
 *   only scripts/convert_output.py's MeshLab PLYs of the joints): arc-length resampling of the strands of hgs_strand_walk_fill
 *   (offsets[S+1], rows[total][2] root -> tip, seg_rows[total]: row of attr) to M points per strand with a per-segment attribute
 *   table attr[P][C] (float32, 1 <= C <= 16).  Strand s, n segments on the vertices v_0..v_n: len_i = sqrt((dx*dx + dy*dy) + dz*dz),
 *   cum_0 = 0, cum_{i+1} = cum_i + len_i, L = cum_n; joint attributes a_0 = attr[seg_0], a_n = attr[seg_{n-1}], a_i = 0.5 (attr[seg_{i-1}]
 *   + attr[seg_i]); sample j: t = (j / (M - 1)) L, i = the largest index with cum_i <= t (at most n - 1), w = (t - cum_i) / len_i (0 if
 *   len_i is 0), v_i + w (v_{i+1} - v_i) and a_i + w (a_{i+1} - a_i); samples 0 and M - 1 are (v_0, a_0) and (v_n, a_n) themselves.  All of
 *   it float64 on the float32 inputs, operation by operation, rounded once to float32.
 *   _arclen, one wavefront per strand: cum[offsets[s] + s + i] = cum_i (i = 0..n; the table has total + S entries and is the one place
 *   _resample looks, so a strand may be any length) and length[s] = L, summed in segment order (the definition's bits); status[0]
 *   (zeroed by the caller) becomes 1 if a row names an endpoint id outside [0, n_ep) -- that segment counts as length 0 -- and 2
 *   if offsets does not describe `rows`.
 *   _resample, one lane per output point, for the K strands kept[K] (int32, ascending): M >= 2 writes sample j of kept[k] to row
 *   k M + j (n_out = K M); M == 0 writes the n + 1 joints with their joint attributes to rows out_offsets[k].. (out_offsets[K+1]: the
 *   caller's prefix sums of n + 1, n_out = out_offsets[K]).  out_points [n_out][3], out_attrs [n_out][C], float32.  Rows of strands
 *   or ids out of range are written as zeros.  No atomics: bitwise reproducible. */
int hgs_strand_arclen(void* stream, int S, const long long* offsets, const long long* rows, long long total, const float* endpoints,
                      int n_ep, double* cum, double* length, int* status);
int hgs_strand_resample(void* stream, int S, const long long* offsets, const long long* rows, const long long* seg_rows, long long total,
                        const float* endpoints, int n_ep, const float* attr, int P, int C, const double* cum, int K, const int* kept,
                        int M, const long long* out_offsets, long long n_out, float* out_points, float* out_attrs);

/* hgs_groom_neighbours / hgs_groom_blend (csrc/hgs_groom.hip) <-> the groom interpolation (scene/groom.py, export_strands.py --interpolate;
 *   the reference has nothing of the kind): a strand for every root, blended from its nearest guides.  Guides: guide_points [K][M][3] and
 *   guide_attrs [K][M][C], float32, M >= 2, 1 <= C <= 16; roots [N][3], float64.  All arithmetic float64 on these inputs, operation by
 *   operation, results rounded once to float32 (scene/groom.py states the contract in full).
 *   _neighbours, one lane per root: among the guides g (ascending) whose d2 = (dx*dx + dy*dy) + dz*dz from the root to guide_points[g][0]
 *   is finite and <= max_d2 (+inf: no limit), the k (1..8) smallest by (d2, g).  Rank 0 is kept; rank i >= 1 is kept iff the chords
 *   c = guide_points[g][M-1] - guide_points[g][0] of both have a length sqrt((cx*cx + cy*cy) + cz*cz) > 0 and (cix*c0x + ciy*c0y) + ciz*c0z
 *   >= cos_max * (len_i * len_0); if d2 of rank 0 is 0 only rank 0 is kept.  w_i = d2_0 / d2_i (w_0 = 1), W = their sum in rank order
 *   from 0.0.  Written, compacted in rank order: idx [N][k] int32, d2 [N][k] and w [N][k] = w_i / W float64, count [N] int32; slots at or
 *   past count hold -1, +inf and 0.  K == 0 is legal: every count is 0.
 *   _blend, one lane per output point, for the n_kept roots kept[n_kept] (int32, ascending, every one in [0, N): the caller's duty,
 *   N is not passed): point j of root n = kept[n'] goes to row n' M + j: coordinate c = (float)(roots[n][c] + acc), acc = 0.0 then
 *   acc = acc + w[n][i] * ((double)guide_points[g_i][j][c] - (double)guide_points[g_i][0][c]) over the row's slots i in order up to the
 *   first idx outside [0, K); attribute a = (float)acc of acc = acc + w[n][i] * (double)guide_attrs[g_i][j][a].  out_points
 *   [n_kept M][3], out_attrs [n_kept M][C], float32; n_kept M is at most 2^31 - 1.  No atomics: bitwise reproducible.
 *   Bad sizes (k, M, C out of range, negative counts, a NaN max_d2 or cos_max, kept roots without a guide) and null arguments return 1
 *   before anything is launched; N == 0 and n_kept == 0 return 0. */
int hgs_groom_neighbours(void* stream, int N, const double* roots, int K, int M, const float* guide_points, int k, double max_d2,
                         double cos_max, int* idx, double* d2, double* w, int* count);
int hgs_groom_blend(void* stream, int K, int M, int C, const float* guide_points, const float* guide_attrs, const double* roots, int k,
                    const int* idx, const double* w, int n_kept, const int* kept, float* out_points, float* out_attrs);

/* hgs_undistort_images (csrc/hgs_undistort.hip) <-> the undistortion of a COLMAP capture (utils/undistort.py, undistort.py; the reference
 *   leaves it to COLMAP's image_undistorter): N images [N][Hs][Ws][C] uint8 (C = 1, 3 or 4, PIL's layout) seen through the camera
 *   `model` (COLMAP's model id: SIMPLE_PINHOLE 0, PINHOLE 1, SIMPLE_RADIAL 2, RADIAL 3, OPENCV 4, FULL_OPENCV 6; any other is an error)
 *   with COLMAP's parameter list src_params_host[12] (host; the model's leading entries are read) are resampled into the pinhole camera
 *   dst_pinhole_host[4] = (fx, fy, cx, cy) (host) of Wd x Hd pixels: dst [N][Hd][Wd][C].  Output pixel (x, y): u = ((x + 0.5) - cx') / fx',
 *   v = ((y + 0.5) - cy') / fy', (sx, sy) = img_from_cam(u, v) - 0.5 in float64, every operation rounded once in the order utils/undistort.py
 *   states; the sample is valid iff 0 <= sx <= Ws - 1 and 0 <= sy <= Hs - 1; x0 = floor(sx), x1 = min(x0 + 1, Ws - 1), wx = sx - x0 (likewise
 *   y), value = (1 - wy)*((1 - wx)*p00 + wx*p01) + wy*((1 - wx)*p10 + wx*p11).  mode 0 (bilinear): floor(value + 0.5); mode 1 (threshold,
 *   for masks): 255 where value >= 127.5, else 0; an invalid sample gives 0.  valid (nullable): [Hd][Wd], 1 where the sample is valid.
 *   Bad arguments (N <= 0, sizes <= 0, another C, model or mode, a null buffer, an image above 2^31 - 1 bytes) return non-zero
 *   before anything is launched. */
int hgs_undistort_images(void* stream, int N, int C, int Hs, int Ws, int Hd, int Wd, int model, const double* src_params_host,
                         const double* dst_pinhole_host, const unsigned char* src, unsigned char* dst, unsigned char* valid, int mode);

/* hgs_rescale_images / hgs_rescale_orientation (csrc/hgs_rescale.hip) <-> the downscaling of a capture (utils/rescale.py states the
 *   contract, rescale.py is the driver; the reference's parsers write the size they want, and the loader here subsamples the hair
 *   planes).  Area averaging of [Hs][Ws] planes into [Hd][Wd], 1 <= Wd <= Ws and 1 <= Hd <= Hs, float64, one rounding per operation:
 *     output column x covers lo = (x*Ws)/Wd to hi = ((x + 1)*Ws)/Wd; i0 = floor(lo); tap k = 0..(Ws + Wd - 1)/Wd reads column
 *     min(i0 + k, Ws - 1) with wx = min(i0 + k + 1, hi) - max(i0 + k, lo), 0 unless > 0; rows likewise; terms ky outer, kx inner, w = wy*wx.
 *   hgs_rescale_images: src [N][Hs][Ws][C] uint8 (C = 1, 3 or 4, PIL's layout) -> dst [N][Hd][Wd][C]; per channel acc += w*p, A += w;
 *     mode 0 (average): min(255, floor(acc/A + 0.5)); mode 1 (threshold, for masks): 255 where acc/A >= 127.5, else 0.
 *   hgs_rescale_orientation: angle, conf [N][Hs][Ws] uint8 (theta = angle*pi/255, so an orientation is averaged as its double-angle
 *     vector), mask [N][Hs][Ws] uint8 or NULL (every pixel counts); tables: DEVICE float64 [4][256] built by the host --
 *     C[t] = cos(2 pi t/255), S[t] = sin(2 pi t/255) (entry 255 = entry 0) and the half-step boundaries HC[j], HS[j] =
 *     cos, sin(2 pi (j - 0.5)/255), j = 1..255 (entry 0 unused); no trigonometric function is evaluated on the device.  Per term with
 *     mask != 0: g = w*conf, X += g*C[angle], Y += g*S[angle], Am += w.  conf_out [N][Hd][Wd]: 0 if Am == 0, else
 *     min(255, floor(sqrt(X*X + Y*Y)/Am + 0.5)).  angle_out: 0 if X == 0 and Y == 0, else (the number of boundaries j that (X, Y) is at
 *     or past) mod 255, where upper(x, y) = y > 0 or (y == 0 and x > 0) and V is at or past H iff upper(V) != upper(H) and H is the upper
 *     one, or the halves are equal and HC*Y - HS*X >= 0.
 *   Bad arguments (N <= 0, sizes <= 0, an output larger than the source, another C or mode, a null buffer other than mask, a plane above
 *   2^31 - 1 bytes, more than 65535 planes or output rows) return non-zero before anything is launched. */
int hgs_rescale_images(void* stream, int N, int C, int Hs, int Ws, int Hd, int Wd, const unsigned char* src, unsigned char* dst, int mode);
int hgs_rescale_orientation(void* stream, int N, int Hs, int Ws, int Hd, int Wd, const unsigned char* angle, const unsigned char* conf,
                            const unsigned char* mask, const double* tables, unsigned char* angle_out, unsigned char* conf_out);

/* hgs_carve_votes / hgs_carve_grid / hgs_carve_shell (csrc/hgs_carve.hip) <-> the Stage-I point cloud carved from a capture's hair masks
 *   (utils/carve.py states the contract, init_cloud.py is the driver; the reference starts from COLMAP's points or the FLAME vertices).
 *   A view is a PINHOLE camera with its image's pose: R[9] row-major world -> camera, t[3], fx, fy, cx, cy (COLMAP's principal point),
 *   W, H, and the byte offsets of its uint8 mask [H][W] and RGB image [H][W][3] in ONE mask buffer and ONE image buffer
 *   (image_offset = -1: none).  Vote of the point (x, y, z) in view k, float64, one rounding per operation in this order:
 *     xc = ((R00*x + R01*y) + R02*z) + tx (yc, zc: rows 1, 2);  u = fx*(xc/zc) + cx, v = fy*(yc/zc) + cy;
 *     seen iff zc > 0 and 0 <= u < W and 0 <= v < H (a NaN: not seen);  px = floor(u), py = floor(v);  hit iff seen and mask[py][px] != 0.
 *   _votes: seen[N], hits[N] = the counts over the V views, rgb_sum[N][3] (nullable; needs images) = the sum of image[py][px] over the
 *   views that hit and have an image.  No early exit: the counts are the contract.  N == 0 launches nothing.
 *   _grid: occ[nz][ny][nx] = 1 where the voxel centre origin_host[k] + (i_k + 0.5)*h is kept: seen >= min_views and 100*hits >=
 *   min_percent*seen (integers, min_views >= 1, 0 <= min_percent <= 100).  A voxel's view loop stops once the rule is decided; the
 *   result is that of the full counts.  1 <= nx, ny, nz <= 1024 and 1 <= V <= 4096, anything else is an error before any launch.
 *   _shell: out = 1 where occ != 0 and one of the six face neighbours is 0 or outside the grid.
 *   The kernels trust the offsets: the caller (hgs_runtime.carve_check) guarantees mask_offset + W*H and image_offset + 3*W*H lie inside
 *   their buffers; `seen` guarantees 0 <= px < W and 0 <= py < H.  views_dev: V records in device memory. */
typedef struct HgsCarveView {
  double R[9], t[3], fx, fy, cx, cy;
  int32_t W, H;
  int64_t mask_offset, image_offset;
} HgsCarveView;
size_t hgs_carve_view_bytes(void);
int hgs_carve_votes(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev, const unsigned char* masks,
                    const unsigned char* images, int* seen, int* hits, int* rgb_sum);
int hgs_carve_grid(void* stream, const double* origin_host, double h, int nx, int ny, int nz, int V, const HgsCarveView* views_dev,
                   const unsigned char* masks, int min_views, int min_percent, unsigned char* occ);
int hgs_carve_shell(void* stream, int nx, int ny, int nz, const unsigned char* occ, unsigned char* out);

/* hgs_lift_moments / hgs_lift_solve (csrc/hgs_lift.hip) <-> 3-D hair directions lifted from the capture's 2-D orientation maps for the
 *   Stage-I cloud (utils/lift.py states the contract, init_cloud.py --directions is the driver; the reference starts from isotropic
 *   Gaussians).  The views are HgsCarveView records; orients and confs are uint8 planes laid out like masks, at the records' mask_offset
 *   of their own buffers.  tab_dev[256][2] = (sin, cos)(o*pi/255), float64, built on the host.  Term of the point (x, y, z) in view k,
 *   float64, one rounding per operation in this order, with xc, yc, zc, u, v, seen, px, py as in hgs_carve_votes:
 *     used iff seen and mask[py][px] != 0 and conf[py][px] >= min_conf;  o = orient[py][px];  a = tab[o][0]/fx, b = tab[o][1]/fy;
 *     ncx = -(zc*b), ncy = zc*a, ncz = xc*b - yc*a;  n_i = (R0i*ncx + R1i*ncy) + R2i*ncz;  nn = (n0*n0 + n1*n1) + n2*n2;
 *     not used unless nn > 0 and finite;  w = conf[py][px]/255.0;  with prev (nullable [N][3]) and prev[i] != (0, 0, 0):
 *     r2 = ((n0*p0 + n1*p1) + n2*p2)^2 / nn, w = w*(s2/(s2 + r2));  g = w/nn;
 *     M[i] += g*(n0n0, n0n1, n0n2, n1n1, n1n2, n2n2) (product, times g, added), wsum[i] += w, count[i] += 1, views in index order.
 *   One lane per point with the view loop inside it: the sums have that order, bitwise repeatable and equal to the numpy path.
 *   _solve: with the eigenvalues l0 <= l1 <= l2 of M[i] (cyclic Jacobi), d[i] = the unit eigenvector of l0, its component of largest
 *   magnitude positive (lowest index on a tie), coherence[i] = (l1 - l0)/(l1 + l0), 0 where the denominator is not > 0; d = 0 and
 *   coherence = 0 where count[i] < min_views, l1 <= 0 or an entry of M[i] is not finite.
 *   Errors before any launch: a null buffer, V outside 1..4096, min_conf outside 0..255, min_views < 2, s2 not finite and positive
 *   while prev is given.  N == 0 launches nothing.  The kernels trust the offsets: the caller (hgs_runtime.lift_check) guarantees
 *   mask_offset + W*H lies inside masks, orients and confs, and that tab_dev holds 512 doubles. */
int hgs_lift_moments(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev, const unsigned char* masks,
                     const unsigned char* orients, const unsigned char* confs, const double* tab_dev, const double* prev, double s2,
                     int min_conf, double* M, double* wsum, int* count);
int hgs_lift_solve(void* stream, long long N, const double* M, const int* count, int min_views, double* d, double* coherence);
/* hgs_lift_moments_gated: hgs_lift_moments with one more condition of `used`: bit k % 32 of visible[i][k / 32] is set (visible: int32
 *   [N][words], hgs_hull_visibility's words; words must be ceil(V/32), a null visible is an error).  The same kernel body, the same order
 *   of the sums; with every bit below V set the outputs are hgs_lift_moments' bit for bit.  hgs_runtime.lift_check guarantees that visible
 *   holds N*words values. */
int hgs_lift_moments_gated(void* stream, long long N, const double* points, int V, const HgsCarveView* views_dev, const unsigned char* masks,
                           const unsigned char* orients, const unsigned char* confs, const double* tab_dev, const double* prev, double s2,
                           int min_conf, const int* visible, int words, double* M, double* wsum, int* count);

/* hgs_hull_visibility (csrc/hgs_visibility.hip) <-> which views can see a point of the carved hull (utils/visibility.py states the contract,
 *   init_cloud.py --directions --visibility is the driver; the reference has no such step).  occ[nz][ny][nx] is hgs_carve_grid's uint8
 *   buffer: voxel i spans origin_host + i*h .. origin_host + (i + 1)*h per axis.  centres_dev[V][3]: the camera centres -R^T t, float64,
 *   computed on the host.  For the point p and the centre C, float64, one rounding per operation in this order:
 *     t_a = (p_a - origin_a)/h;  inside iff 0 <= t_a < n_a on every axis (a NaN fails; the test precedes the conversion to an integer);
 *     a point that does not start inside has every bit below V set.  Otherwise i0_a = (int)floor(t_a), D = C - p and per axis
 *       D_a > 0:  step = +1, tmax = ((origin_a + (i0_a + 1)*h) - p_a)/D_a, td = h/D_a
 *       D_a < 0:  step = -1, tmax = ((origin_a + i0_a*h) - p_a)/D_a,       td = h/(-D_a)
 *       D_a == 0: step = 0,  tmax = +inf
 *     walk from i = i0, blocked = 0:  a = the axis of the smallest tmax (strict <: the lowest axis wins a tie);  VISIBLE unless tmax_a < 1.0;
 *     i_a += step_a, VISIBLE if i_a has left the grid;  tmax_a = tmax_a + td_a;  if max_a |i_a - i0_a| > skip and occ[i] != 0: blocked += 1,
 *     BLOCKED if blocked > max_blocked;  at most nx + ny + nz steps (unreachable: the indices move monotonically), then VISIBLE.
 *   visible int32 [N][ceil(V/32)]: bit k % 32 of word k / 32 is set iff view k is not blocked; the bits at and above V are 0.
 *   One lane per (point, word); no atomics: bitwise repeatable and equal to the numpy path.  N == 0 launches nothing.
 *   Errors before any launch, the text beginning with the function's name: a null buffer, V outside 1..4096, an axis outside 1..1024, skip
 *   outside 0..1024, max_blocked outside 0..3072, h or 1/h not finite and positive, an origin that is not finite.  The kernel trusts the
 *   shapes: the caller (hgs_runtime.visibility_check) guarantees occ holds nx*ny*nz bytes, points N*3, centres V*3 and visible
 *   N*ceil(V/32) values. */
int hgs_hull_visibility(void* stream, long long N, const double* points, int V, const double* centres_dev, const unsigned char* occ,
                        const double* origin_host, double h, int nx, int ny, int nz, int skip, int max_blocked, int* visible);

/* hgs_scalp_depth / hgs_scalp_votes (csrc/hgs_scalp.hip) <-> the scalp labelled on a capture's head mesh from its hair masks (utils/scalp.py
 *   states the contract, init_scalp.py is the driver; the reference takes FLAME's fixed scalp region).  The views are HgsCarveView records;
 *   `depth` is ONE buffer of doubles that holds view k's map [H][W] at ELEMENT offset mask_offset: the masks' layout with 8-byte elements.
 *   All float64, one rounding per operation in this order, with xc, yc, zc, u, v, seen, px, py as in hgs_carve_votes.
 *   _depth: sets every map to +inf and *dropped to 0 (a launch of its own in front), then for every face (verts[NV][3], faces[F][3], int32
 *   indices in 0..NV-1) and view, with (xc_i, yc_i, zc_i), (u_i, v_i) of the vertices i = 0, 1, 2:
 *     dropped, and counted in *dropped, when a zc_i is not > 0 or a u_i, v_i is not finite (no near-plane clipping);
 *     candidates max(0, ceil(min u - 0.5)) <= px <= min(W - 1, floor(max u - 0.5)), likewise py; centre (cx, cy) = (px + 0.5, py + 0.5);
 *     E0 = (u2 - u1)*(cy - v1) - (v2 - v1)*(cx - u1), E1 = (u0 - u2)*(cy - v2) - (v0 - v2)*(cx - u2),
 *     E2 = (u1 - u0)*(cy - v0) - (v1 - v0)*(cx - u0), S = (E0 + E1) + E2;  covered iff S != 0 and (every E >= 0 or every E <= 0);
 *     iz = (E0*(1/zc0) + E1*(1/zc1)) + E2*(1/zc2), z = S/iz;  Z[py][px] = min(Z[py][px], z) where covered and 0 < z < inf
 *   (an atomic minimum on z's bit pattern: exact and order-free, the maps are bitwise reproducible).  F == 0 only sets the maps.
 *   _votes: for the sample (points[i], normals[i]) over the V views:
 *     nc_r = (R_r0*n0 + R_r1*n1) + R_r2*n2;  d = -((nc0*xc + nc1*yc) + nc2*zc);  nn = (nc0*nc0 + nc1*nc1) + nc2*nc2;
 *     pp = (xc*xc + yc*yc) + zc*zc;  facing iff d > 0 and d*d >= (min_cos*min_cos)*(nn*pp);
 *     visible iff seen and facing and zc <= Z[py][px] + depth_tol;  vis[i] += visible, hits[i] += visible and mask[py][px] != 0.
 *   N == 0 launches nothing.
 *   Errors before any launch, the text beginning with the function's name: a null buffer, V outside 1..4096, NV or F outside 0..2^24
 *   (or faces without a vertex), min_cos outside [0, 1], depth_tol not finite or negative.  The kernels trust the offsets and the
 *   indices: the caller (hgs_runtime.scalp_check) guarantees that mask_offset + W*H lies inside masks and depth, W*H < 2^31 and
 *   0 <= faces < NV. */
int hgs_scalp_depth(void* stream, int NV, const double* verts, int F, const int* faces, int V, const HgsCarveView* views_dev, double* depth,
                    unsigned long long* dropped);
int hgs_scalp_votes(void* stream, long long N, const double* points, const double* normals, int V, const HgsCarveView* views_dev,
                    const unsigned char* masks, const double* depth, double min_cos, double depth_tol, int* vis, int* hits);

/* Strand metrics (csrc/hgs_metrics.hip) <-> pct_matched_points of the reference's loss/metrics.py:12-85: the cKDTree
 *   query_ball_point per (distance, angle) pair, the direction test and the per-point Python loop that counts matches and
 *   strand-consistency votes.  Points and directions are float64 [n][3]; thresholds_host[K][2] = (r_k, cos_k), 1 <= K <= 32;
 *   box_host[6] = lo xyz, hi xyz: a box holding every point of B (its per-axis min and max), which must need at most 2^21
 *   cells of edge max r_k (1 + 1e-6) per axis.
 * hgs_oriented_match: mask[i] bit k = some B point j has d2 = (dx*dx + dy*dy) + dz*dz <= r_k*r_k (float64, in that order)
 *   and dot(a_dir_i, b_dir_j) >= cos_k (|dot| when bidirectional; NaN never matches).  Builds a hashed grid of B in scratch
 *   (>= hgs_oriented_match_scratch_bytes(nB) bytes, 256-byte aligned), which hgs_strand_votes reads afterwards.
 * hgs_strand_votes: A's S strands are runs of its points, offsets[S+1] (int64); b_strand[nB] = a strand number per B point
 *   (only equality matters: any int, -1 and INT_MIN included).  best[k][s] = max over B strands b of the number of points of strand s that some point of b
 *   matches under pair k.  Needs the scratch of an hgs_oriented_match call with the same B, thresholds and box, left
 *   unchanged.  `capacity` (a power of two <= 2048) sizes the workgroup's LDS tables; a strand whose distinct (point,
 *   B strand) matches do not fit is appended to overflow[*n_overflow] (*n_overflow device, zero on entry) and its best[.][s]
 *   is left unwritten: the caller counts it.
 * Empty sides: nA == 0 (S == 0) returns 0 and writes nothing; nB == 0 needs no B arrays and no scratch and zeroes mask
 *   (best; overflow and *n_overflow stay as they are). */
size_t hgs_oriented_match_scratch_bytes(int nB);
int hgs_oriented_match(void* stream, int nA, int nB, int K, const double* a_pts, const double* a_dirs, const double* b_pts,
                       const double* b_dirs, const double* thresholds_host, int bidirectional, const double* box_host,
                       uint32_t* mask, void* scratch, size_t scratch_bytes);
int hgs_strand_votes(void* stream, int S, int nB, int K, const double* a_pts, const double* a_dirs, const long long* offsets,
                     const int* b_strand, const double* thresholds_host, int bidirectional, const double* box_host,
                     const void* scratch, int capacity, int* best, int* overflow, int* n_overflow);

/* Orientation maps (csrc/hgs_vision.hip) <-> estimate_orientation_field of the reference's utils/vision.py (cv2.filter2D of A
 *   Gabor kernels, first argmax, response-weighted angular variance).  N gray uint8 views [N][H][W]; weights[A][side][side]
 *   float64 (device; the float32 kernel values, row ky, column kx, correlated with the anchor at the centre), side odd and
 *   <= 63; thetas[A] float64 (device), 2 <= A <= 256.
 * hgs_orientation_field: r_k = the correlation with BORDER_REFLECT_101, accumulated in float64, rounded half to even and
 *   saturated to uint8; idx_out[N][H][W] = the first k of the largest r_k; var_out[N][H][W] =
 *   sum_k (d_k*d_k)*r_k / (sum_k r_k + 1e-7) in k order, d_k = pi/2 - | |thetas[idx] - thetas[k]| - pi/2 |; maxinv_out[N] =
 *   the largest 1/(var*var) of the view over var != 0 (0: no such pixel).  responses (nullable): [N][H][W][A] uint8 r_k.
 *   scratch: >= hgs_orientation_scratch_bytes(N, H, W, A, side) bytes, 256-byte aligned.
 * hgs_orientation_confidence: conf_out[N][H][W] = float((1/(var*var)) / maxinv[n]) where var != 0, else 1. */
size_t hgs_orientation_scratch_bytes(int N, int H, int W, int A, int side);
int hgs_orientation_field(void* stream, int N, int H, int W, const unsigned char* gray, int A, int side, const double* weights,
                          const double* thetas, unsigned char* idx_out, double* var_out, double* maxinv_out, unsigned char* responses,
                          void* scratch, size_t scratch_bytes);
int hgs_orientation_confidence(void* stream, int N, int H, int W, const double* var, const double* maxinv, float* conf_out);

/* Image metrics of rendered views against their capture (csrc/hgs_view_stats.hip) <-> loss/image_metrics.py view_metrics (this
 *   project; the reference has no counterpart), whose CPU path is the contract.  V views of one size, every plane device memory,
 *   float32 unless stated: pred, gt [V][3][H][W] (pred: the render clamped to [0, 1]); gt_mask [V][H][W] uint8 (nonzero: set), fg
 *   [V][H][W] (the rendered foreground channel, foreground where >= fg_threshold), omap [V][3][H][W] (rendered world-space
 *   directions), viewmats [V][16] (world_view_transform, row-major), gt_theta [V][H][W], confidence [V][H][W].  Every plane but pred
 *   and gt may be NULL and turns its statistics off; the orientation ones need omap, viewmats and gt_theta (its mask: gt_mask,
 *   else omap != 0 in any channel; no confidence: weight 1).  Per-pixel values are float32 in the CPU path's order, the sums
 *   float64 in a fixed order: bitwise reproducible, and a view's row does not depend on the other views of the batch.
 *   partials: V * hgs_view_stats_num_blocks(H, W) * HGS_VIEW_STATS_N doubles of scratch; out [V][HGS_VIEW_STATS_N] doubles:
 *   sse, sse over the GT mask, GT mask count, foreground count, intersection count, orientation |diff| sum, diff * confidence sum,
 *   orientation mask count, count of diff <= 10 degrees, count of diff <= 20 degrees. */
#define HGS_VIEW_STATS_N 10
int hgs_view_stats_num_blocks(int H, int W);
int hgs_view_stats(void* stream, int V, int H, int W, const float* pred, const float* gt, const unsigned char* gt_mask, const float* fg,
                   float fg_threshold, const float* omap, const float* viewmats, const float* gt_theta, const float* confidence,
                   float min_val, double* partials, double* out);

/* Line / triangle rasterizer of the dataset synthesis (csrc/hgs_raster.hip) <-> the reference's OpenGL renderer
 *   (scene/OpenGLRenderer.py); the contract is scene/mesh_renderer.py's (this project), which both backends meet bit for bit.
 *   Vertex arrays are the selected models' concatenated, float64: pw[NV][4] = M [p, 1], nw[NV][3] = inv(M3)^T n, col[NV][3];
 *   idx: uint32 global vertex ids, models[n_models] (device) in list order, draw index = draw_base + primitive.  views / projs:
 *   [V][16] row-major float64 (device).  vout: V * NV records of hgs_raster_vertex_bytes().  Tiles are 32 x 32 window pixels,
 *   hgs_raster_tiles(W, H) per view, row-major from the bottom-left.
 * hgs_raster_vertices: the per-(view, vertex) stage.
 * hgs_raster_count: tile_counts[V][T] (zeroed by the caller) += tiles each primitive reaches; *dropped (zeroed) += dropped ones.
 * hgs_raster_fill: list[tile_offsets[vt] + k] = the draw indices of tile vt (tile_offsets: exclusive scan of tile_counts, int64;
 *   tile_cursor[V][T] zeroed); in no particular order.
 * hgs_raster_resolve: rgb[V][H][W][3] (image rows top-down), gray[V][H][W] (nullable); light_host: position, ambient rgb, diffuse
 *   rgb (9 doubles); background_host: 3 bytes. */
#define HGS_RASTER_MAX_MODELS 64
typedef struct HgsRasterModel {
  long long draw_base;          /* draw index of the model's first primitive */
  long long idx_offset;         /* its first entry in idx */
  int n_prims, kind;            /* kind: 2 = lines, 3 = triangles */
  int width, lit;               /* line width in pixels (>= 1); lit: 1 = the diffuse shader, 0 = colour as it is */
  double ka, kd;
} HgsRasterModel;
size_t hgs_raster_model_bytes(void);
size_t hgs_raster_vertex_bytes(void);
int hgs_raster_tiles(int W, int H);
int hgs_raster_vertices(void* stream, int V, int NV, int W, int H, const double* pw, const double* views, const double* projs,
                        void* vout);
int hgs_raster_count(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, long long n_prims,
                     const unsigned* idx, int NV, const void* vout, int* tile_counts, unsigned long long* dropped);
int hgs_raster_fill(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, long long n_prims,
                    const unsigned* idx, int NV, const void* vout, const int* tile_counts, const long long* tile_offsets,
                    int* tile_cursor, unsigned* list);
int hgs_raster_resolve(void* stream, int V, int W, int H, int n_models, const HgsRasterModel* models, const unsigned* idx,
                       int NV, const void* vout, const double* pw, const double* nw, const double* col, const double* light_host,
                       const unsigned char* background_host, const int* tile_counts, const long long* tile_offsets,
                       const unsigned* list, unsigned char* rgb, unsigned char* gray);

/* The head mesh as a signed distance field and the penetration term that samples it (csrc/hgs_sdf.hip; utils/head_sdf.py states
 *   the contract and has the numpy path).  Every argument is checked before a pointer is touched.
 * hgs_mesh_sdf: tris [F][9] float64 (device): v0, v1, v2 of every face, all finite (the caller drops the others).  Node (ix, iy, iz)
 *   of the grid lies at origin + index * h; phi [nz][ny][nx] float32 receives +-sqrt(min over the faces of the squared point-triangle
 *   distance), negative where the generalized winding number exceeds 0.5, a zero as +0; winding (nullable) [nz][ny][nx] float64
 *   receives that number.  Float64, one rounding per operation; |phi| does not depend on the faces' order.  1 <= F <= 2^24, 1 <= n <=
 *   1024 an axis.
 * hgs_head_penalty_forward: points [E][3] float32, phi as above, origin and 1/h rounded to float32.  Per point, in float32:
 *   t = (p - origin) * inv_h; in range iff 0 <= t < n - 1 on every axis (a NaN is not); d = the trilinear interpolant (x, then y,
 *   then z), r = margin - d; pen = r r and g = (-2 r) grad d where in range and r > 0, else 0.  g [E][3] (scratch the backward reads),
 *   pen [E] and dist [E] (both nullable; dist = d, +inf out of range), partials: hgs_head_penalty_num_blocks(E) doubles of scratch,
 *   out [1] = float(sum of pen in float64 / E), 0 for E = 0.  Two launches, bitwise reproducible, no atomics.
 * hgs_head_penalty_backward: d_points [E][3] = g * (upstream[0] / float(E)), upstream in device memory.  One launch. */
int hgs_mesh_sdf(void* stream, int F, const double* tris, double ox, double oy, double oz, double h, int nx, int ny, int nz, float* phi,
                 double* winding);
int hgs_head_penalty_num_blocks(int E);
int hgs_head_penalty_forward(void* stream, int E, const float* points, const float* phi, int nx, int ny, int nz, float ox, float oy,
                             float oz, float inv_h, float margin, float* g, float* pen, float* dist, double* partials, float* out);
int hgs_head_penalty_backward(void* stream, int E, const float* g, const float* upstream, float* d_points);

/* hgs_direction_loss_* (csrc/hgs_direction.hip) <-> the 3-D direction term of a strand model (utils/direction_term.py states the
 *   contract and has the numpy path; train.py --lambda_direction; the reference has nothing of the kind).  Added under ABI 15.
 * hgs_direction_loss_forward: points [E][3] float32; pairs [S][2] int64, every entry in [0, E): the caller's duty (the Python binding
 *   checks it when it builds the incidence table).  vol [nz][ny][nx][4] float32 = (dir.x, dir.y, dir.z, conf) per node, 16-byte
 *   aligned; origin and 1/h rounded to float32.  Per segment, float32, one rounding per operation: a, b its endpoints, u = b - a,
 *   m = (a + b) * 0.5, t = (m - origin) * inv_h; in range iff 0 <= t < n - 1 on every axis (a NaN is not; the test precedes every
 *   load); the eight corners with z outermost, then y, then x: tw = (gx gy) gz, q = tw conf, w += q, q = -q where dot(dir, u) < 0,
 *   v += q dir; active iff in range, w >= min_conf and dot(v, v), dot(u, u) finite and > 0; fd = v / sqrt(dot(v, v)), cu = dot(u, fd),
 *   k = cu / dot(u, u); term = 1 - cu k, gs = (-2 k)(fd - k u); both 0 where inactive.  gs [S][3] (scratch the backward reads), term
 *   [S] and w [S] (both nullable), partials: 2 * hgs_direction_loss_num_blocks(S) doubles of scratch, out [2]: [0] = float(sum of
 *   term in float64 / S), 0 for S = 0; [1] = the number of active segments, int32 bits.  Two launches, bitwise reproducible, no
 *   atomics.  2 <= n <= 1024 an axis, at most 2^26 nodes, 0 <= S <= 2^28.
 * hgs_direction_loss_backward: the incidence table of the endpoints as CSR: offsets [E + 1] int32, entries [2 S] int32 = 2 s + side
 *   for every pairs[s][side] == e, ascending within an endpoint's run (trusted).  d_points [E][3] = acc * (upstream[0] / float(S)),
 *   acc the float32 sum over the run, in order, of +gs[s] (side 1) or -gs[s] (side 0); upstream in device memory; every endpoint is
 *   written (0 for one that no segment uses, and for S = 0).  One launch, no atomics. */
int hgs_direction_loss_num_blocks(int S);
int hgs_direction_loss_forward(void* stream, int S, const float* points, const long long* pairs, const float* vol, int nx, int ny, int nz,
                               float ox, float oy, float oz, float inv_h, float min_conf, float* gs, float* term, float* w,
                               double* partials, float* out);
int hgs_direction_loss_backward(void* stream, int E, int S, const int* offsets, const int* entries, const float* gs,
                                const float* upstream, float* d_points);

/* hgs_strand_collide (csrc/hgs_collide.hip) <-> the push-out of exported strands (scene/strand_collide.py states the contract and has
 *   the numpy path; export_strands.py --resolve_head; the reference has nothing of the kind): every strand is walked from its root, a
 *   joint inside the head (in range and d < margin) is pushed along the field's gradient to margin + skin, and every joint behind a
 *   pushed one is put back at its segment's original length from its moved predecessor, aiming at its original place.
 *   K strands, strand s owning points offsets[s] .. offsets[s + 1] - 1 of points [P][3] float32; offsets [K + 1] int64 with
 *   offsets[0] == 0, non-decreasing, offsets[K] == P: the caller's duty (a strand whose range does not lie inside the P points is
 *   skipped, its counts 0).  phi [nz][ny][nx] float32 with origin and 1/h rounded to float32, sampled by hgs_head_penalty_forward's
 *   statement at float32(x) (csrc/hgs_sdf_sample.h: one definition for both).  Per strand with joints p_0 .. p_{n-1} (n < 2: copied),
 *   float64, one rounding per operation, dot(u, v) = (u0*v0 + u1*v1) + u2*v2: q_0 = p_0; for j = 1 .. n-1: e = p_j - p_{j-1},
 *   L = sqrt(dot(e, e)); relen(x) = q_{j-1} + (L / lu) * u for u = x - q_{j-1}, lu = sqrt(dot(u, u)), where L and lu are finite and
 *   lu > 0, else q_{j-1} + e; x = p_j, or relen(p_j) once a joint of the strand has been pushed; then at most iters (1..32) times:
 *   sample (d, g) at x, stop unless in range and d < margin, gn = sqrt(dot(g, g)), stop unless gn is finite and > 0,
 *   x = relen(x + (((margin + skin) - d) / gn) * g).  out_points[j] = float32(x); a joint that was pushed at least once adds one to
 *   moved[s]; a joint whose written place is in range with d < margin adds one to unresolved[s].  margin, skin: finite, >= 0.
 *   out_points [P][3] float32 must not alias points; moved, unresolved [K] int32.  One lane per strand, no atomics: bitwise
 *   reproducible.  Bad sizes (negative counts, iters out of range, a margin or skin that is negative or not finite, an axis < 2 or
 *   > 1024, an origin or 1/h that is not finite) and, for K > 0, null or aliased pointers return 1 before anything is launched;
 *   K == 0 returns 0. */
int hgs_strand_collide(void* stream, int K, const long long* offsets, long long P, const float* points, const float* phi, int nx, int ny,
                       int nz, float ox, float oy, float oz, float inv_h, float margin, float skin, int iters, float* out_points,
                       int* moved, int* unresolved);

/* hgs_root_attach, hgs_strand_rejoin (csrc/hgs_attach.hip) <-> exported strands rooted on the head (scene/strand_attach.py states the
 *   contract and has the numpy path; export_strands.py --attach_roots; the reference has nothing of the kind).  Added under ABI 15.
 *   Strands as for hgs_strand_collide: K strands over points [P][3] float32 through offsets [K + 1] int64 (the caller's duty; a range
 *   that does not lie inside the P points counts as a strand without joints).  The head's field phi as for hgs_strand_collide,
 *   sampled by S(x) = csrc/hgs_sdf_sample.h at float32(x): (ok, d, G).  The direction volume (vol_dir [vnz][vny][vnx][3], vol_conf
 *   [vnz][vny][vnx] float64 on the grid origin + index * vh, 2 to 1024 nodes an axis, at most 2^26 in all) may be null (both
 *   pointers): it is sampled by hgs_strand_trace's corner loop at t = (x - origin) * (1 / vh), signs chosen against p.
 * hgs_root_attach: per strand with joints p_0 .. p_{n-1}, float64, one rounding per operation, dot(u, v) = (u0*v0 + u1*v1) + u2*v2;
 *   m = (double)margin, tl = (double)tol:
 *     n < 2: DEGENERATE.  x = p_0; (ok, d, G) = S(x).  not ok: RANGE.  d <= m + tl: NEAR.  d - m > max_distance: FAR.
 *     e = x - p_1, le = sqrt(dot(e, e)); p = e / le where le is finite and > 0, else -G / sqrt(dot(G, G)).
 *     at most max_steps (1 to 1024) times:
 *       gn = sqrt(dot(G, G)); unless finite and > 0: FLAT
 *       if d - m <= step: at most land_iters (1 to 8) times: c = (m - d) / gn; x = x + (c * G) / gn; (ok, d, G) = S(x); not ok: RANGE;
 *         |d - m| <= tl: append x, REACHED; gn = sqrt(dot(G, G)); unless finite and > 0: FLAT.  Then UNLANDED.
 *       nrm = -G / gn; f = the volume's direction v / sqrt(dot(v, v)) where there is a volume, x is in its range, w >= min_conf and
 *       dot(v, v) is finite and > 0, else p; v = f + pull * nrm; dd = v / sqrt(dot(v, v)) where that length is finite and > 0, else
 *       nrm; dot(dd, nrm) < descent: dd = nrm; x = x + step * dd; p = dd; append x; (ok, d, G) = S(x); not ok: RANGE.
 *     then STEPS.
 *   ext [K][max_steps + 1][3] float64 receives the appended points in order (rows from count on are unspecified), count [K] int32
 *   their number, reason [K] int32: 0 reached, 1 near, 2 degenerate, 3 range, 4 flat, 5 steps, 6 unlanded, 7 far; landed [K] float32
 *   the distance d at the landed point (reached) or at the root (near), +inf otherwise.  margin, tol: finite, >= 0; step finite and
 *   > 0; pull finite and >= 0; 0 < descent <= 1; max_distance >= 0, may be +inf; min_conf finite.  One lane per strand, no atomics.
 * hgs_strand_rejoin: attrs [P][C] float32 (0 <= C <= 64), ext / count / reason as above with ext_rows = max_steps + 1 rows a strand,
 *   out_offsets [K + 1] int64 made by the caller: a strand that is not reached (reason != 0) owns n output points and is copied; a
 *   reached one owns count + n points with M == 0 -- float32(ext[count - 1]), .., float32(ext[0]), then p_0 .. p_{n-1}, the new joints
 *   with p_0's attributes -- and M points with M >= 2: that polyline resampled by arc length by hgs_strand_resample's statement
 *   (len_i and cum in float64 in segment order, t = (j / (M - 1)) L, the largest i <= m - 2 with cum_i <= t or 0 where there is none,
 *   w = (t - cum_i) / len_i or 0 unless len_i > 0, v_i + w (v_{i+1} - v_i), the same for the joints' own attributes, rounded once; the
 *   end samples are the end joints' bits).  A strand whose output range is not the size this asks for, or does not lie inside the
 *   n_out points, is not written.  out_points [n_out][3] and out_attrs [n_out][C] must not alias the inputs.
 *   Both: bad sizes and parameters and, for K > 0, null or aliased pointers return 1 before anything is launched; K == 0 returns 0. */
int hgs_root_attach(void* stream, int K, const long long* offsets, long long P, const float* points, const float* phi, int nx, int ny,
                    int nz, float ox, float oy, float oz, float inv_h, const double* vol_dir, const double* vol_conf, int vnx, int vny,
                    int vnz, double vox, double voy, double voz, double vh, double min_conf, float margin, float tol, double step,
                    int max_steps, int land_iters, double pull, double descent, double max_distance, double* ext, int* count,
                    int* reason, float* landed);
int hgs_strand_rejoin(void* stream, int K, const long long* offsets, long long P, const float* points, const float* attrs, int C,
                      const double* ext, int ext_rows, const int* count, const int* reason, int M, const long long* out_offsets,
                      long long n_out, float* out_points, float* out_attrs);

/* hgs_strand_smooth (csrc/hgs_strand_smooth.hip) <-> exported strands smoothed without shrinking them (scene/strand_smooth.py states
 *   the contract and has the numpy path; export_strands.py --smooth_strands; the reference has nothing of the kind).  Added under
 *   ABI 15.  Taubin's lambda|mu low-pass over every strand's polyline, both end joints pinned, weights from the original segment
 *   lengths.  Strands as for hgs_strand_collide: K strands over points [P][3] float32 through offsets [K + 1] int64 (the caller's
 *   duty; a range that does not lie inside the P points counts as a strand without joints).  Per strand with joints p_0 .. p_{n-1},
 *   float64, one rounding per operation, dot(u, v) = (u0*v0 + u1*v1) + u2*v2:
 *     n < 3: status 1 (short).  n > 1024: status 2 (long).  Any coordinate not finite: status 3.  The strand is copied.
 *     Otherwise status 0:  l_i = sqrt(dot(e_i, e_i)) for e_i = p_{i+1} - p_i;  for inner j = 1 .. n-2: s_j = l_{j-1} + l_j, a_j =
 *     l_j / s_j and b_j = l_{j-1} / s_j where s_j > 0, else both 0.5.  A sweep with factor f (Jacobi: sweep t+1 reads sweep t only):
 *     m = a_j*x_{j-1}[c] + b_j*x_{j+1}[c]; x'_j[c] = x_j[c] + f*(m - x_j[c]) for every inner j and coordinate c; x_0 and x_{n-1} stay.
 *     iters (1 to 256) times: a sweep with lam, then, unless mu == 0, a sweep with mu.  With has_max_move != 0, for every inner j:
 *     u = x_j - p_j, du = sqrt(dot(u, u)); if du > max_move: x_j = p_j + (max_move / du)*u and clamped[s] += 1.  out_j = float32(x_j)
 *     for the inner joints; the two end joints get their input bits.
 *   0 < lam <= 1; mu == 0 or -1 <= mu < -lam; |(1 - 2 lam)(1 - 2 mu)| <= 1; max_move finite and > 0 where has_max_move != 0 (it is
 *   not looked at otherwise).  max_joints (0 to 1024): the number of joints of the launch's longest strand with 3 <= n <= 1024, which
 *   the caller reads off the offsets (0 where there is none); it sizes the dynamic LDS -- one wavefront per strand keeps the strand in
 *   five float64 rows of max_joints entries, 4, 2 or 1 wavefronts a workgroup, whichever is the most that fits 64 KB -- and a strand
 *   longer than it is treated as long, never written past its slice.  out_points [P][3] float32 must not alias points; status,
 *   clamped [K] int32.  No atomics, bitwise reproducible.  Bad sizes, iters or parameters and, for K > 0, null or aliased pointers
 *   return 1 before anything is launched; K == 0 returns 0. */
int hgs_strand_smooth(void* stream, int K, const long long* offsets, long long P, const float* points, int max_joints, int iters,
                      double lam, double mu, int has_max_move, double max_move, float* out_points, int* status, int* clamped);

/* hgs_strand_simplify (csrc/hgs_strand_simplify.hip) <-> exported strands simplified to a tolerance (scene/strand_simplify.py states
 *   the contract and has the numpy path; export_strands.py --simplify; the reference has nothing of the kind).  Added under ABI 15.
 *   Douglas-Peucker with the distance to the segment, per strand.  Strands as for hgs_strand_smooth: K strands over points [P][3]
 *   float32 through offsets [K + 1] int64 (the caller's duty; a range that does not lie inside the P points counts as a strand
 *   without joints).  Per strand with joints p_0 .. p_{n-1}, float64, one rounding per operation, dot(u, v) = (u0*v0 + u1*v1) + u2*v2:
 *     n < 3: status 1 (short).  n > max_joints: status 2 (long).  Any coordinate not finite: status 3.  Every joint is kept, rounds 0.
 *     Otherwise status 0.  d2(p; a, b): ab = b - a, ap = p - a, L2 = dot(ab, ab), t = dot(ap, ab) / L2 where L2 > 0, else 0, clamped
 *     to [0, 1]; q_c = ap_c - t*ab_c; d2 = dot(q, q).  Joints 0 and n - 1 are kept; the interval (0, n - 1) has depth 1.  In an interval
 *     (i, k) of consecutive kept joints with k > i + 1 the joint j* of the largest d2(p_j; p_i, p_k), the smallest j among equals, is
 *     kept if d2 > tol*tol (strict; the product is formed once), and (i, j*) and (j*, k), of the next depth, are treated alike.
 *     rounds[s] = the largest depth at which a joint was kept.
 *   tol is finite and >= 0.  max_joints (3 to 1024): the number of joints of the launch's longest strand with 3 <= n <= 1024, which
 *   the caller reads off the offsets; 0 where there is none (every strand of 3 joints or more is then long).  It sizes the dynamic
 *   LDS -- one wavefront per strand keeps the strand in 48 * max_joints + 128 bytes, 4, 2 or 1 wavefronts a workgroup, whichever is
 *   the most that fits 64 KB.  keep [P] uint8 is written for every joint of every strand (1: kept); status, rounds [K] int32.  Integer
 *   LDS atomics on exact keys only: bitwise reproducible.  Bad sizes, tol or max_joints and, for K > 0, null or aliased pointers
 *   return 1 before anything is launched; K == 0 returns 0. */
int hgs_strand_simplify(void* stream, int K, const long long* offsets, long long P, const float* points, int max_joints, double tol,
                        unsigned char* keep, int* status, int* rounds);

/* hgs_guides_assign / hgs_guides_update / hgs_guides_pick (csrc/hgs_guides.hip) <-> guide strands picked from an exported groom by
 *   Lloyd's k-means (scene/strand_guides.py states the contract and has the numpy path; export_strands.py --select_guides).  N strands
 *   of M >= 2 points each, points float32 [n_points][3] with N*M <= n_points; strand i's feature is its S sampled points
 *   j_s = (s*(M-1)) / (S-1), 2 <= S <= min(64, M), as doubles; centroids float64 [K][S][3], 1 <= K <= 65536.  All arithmetic is float64,
 *   one rounding per operation in the order written.  Every argument is checked before anything is launched; N == 0 returns 0.
 * hgs_guides_assign: status int32 [N] (0: the strand takes part; anything else: label -1, dist2 +inf).  d2(i, k) is accumulated from
 *   0.0 over s in order, acc = acc + ((dx*dx + dy*dy) + dz*dz), d = feature - centroid; label [N] int32 = the k smallest by (d2, k),
 *   dist2 [N] float64 its d2.  prev_label (may be NULL): changed [1] int32 is ADDED the number of strands whose label differs from
 *   prev_label's (an integer atomic; the caller zeroes it).  label must not alias prev_label or status.  Bitwise reproducible.
 * hgs_guides_update: order int64 [n_order] lists the strands that have a label, sorted by label and, within one, ascending (a stable
 *   sort), start int64 [K + 1] the clusters' ranges in it.  For every cluster with members each of its 3S coordinates becomes the sum
 *   of the members' coordinates, added from 0.0 in list order, divided by the member count as a double; an empty cluster keeps its
 *   centroid.  count [K] int32 = the members.  Entries of order outside [0, N) and ranges outside [0, n_order] are skipped.
 * hgs_guides_pick: guide [K] int64 = the member of cluster k smallest by (dist2, i); -1 for an empty cluster. */
int hgs_guides_assign(void* stream, int N, int M, int S, long long n_points, const float* points, const int* status, int K,
                      const double* centroids, const int* prev_label, int* label, double* dist2, int* changed);
int hgs_guides_update(void* stream, int N, int M, int S, long long n_points, const float* points, int K, const long long* order,
                      long long n_order, const long long* start, double* centroids, int* count);
int hgs_guides_pick(void* stream, int N, int K, const long long* order, long long n_order, const long long* start, const double* dist2,
                    long long* guide);

/* hgs_dedupe_count / hgs_dedupe_fill / hgs_dedupe_resolve (csrc/hgs_dedupe.hip) <-> near-copy strands dropped from an exported groom
 *   (scene/strand_dedupe.py states the contract and has the numpy path; export_strands.py --dedupe; the reference has nothing of the
 *   kind).  Added under ABI 15.  N strands of M >= 2 points each, points float32 [n_points][3] with N*M <= n_points.  All arithmetic
 *   is float64, one rounding per operation in the order written.  pair(i, j), i != j, holds iff (dx*dx + dy*dy) + dz*dz <= tol*tol
 *   (the product formed once) at EVERY joint s = 0 .. M-1, d = x_i[s] - x_j[s]; a coordinate that is not finite makes the comparison
 *   false.  tol is finite and >= 0.  Every argument is checked before anything is launched; N == 0 returns 0.
 * hgs_dedupe_count: counts [N][HGS_DEDUPE_PARTS] int32; counts[i][c] = the j < i with pair(i, j) among the strands of part c: the
 *   strands below the last strand of i's block of 256 are cut, in tiles of 256, into HGS_DEDUPE_PARTS contiguous parts of ascending j,
 *   a workgroup each.  Row i sums to strand i's lower neighbours.
 * hgs_dedupe_fill: starts [N*HGS_DEDUPE_PARTS] int64 = the exclusive prefix sum of the flattened counts (so starts[i*HGS_DEDUPE_PARTS]
 *   is strand i's lower_offsets), n_pairs their total; lower [n_pairs] int32 gets every strand's lower neighbours, ascending in j.  tol
 *   and the points must be the count pass's; a list that does not match is truncated at its slot's end, never overrun.  n_pairs == 0
 *   returns 0.  No atomics: the same bytes on every run.
 * hgs_dedupe_resolve: one Jacobi round of "a strand is kept unless a kept earlier strand pairs with it".  lower_offsets [N + 1]
 *   int64 and lower [n_pairs] int32 as above (entries outside [0, i) and ranges outside [0, n_pairs] are skipped); state [N] uint8:
 *   0 undecided, 1 kept, 2 dropped.  A strand that is undecided in `state` and whose lower neighbours are all decided there gets, in
 *   state_out, 2 with kept_by [N] int64 = its smallest kept lower neighbour, or 1 with kept_by = itself where none is kept, and
 *   rounds [N] int32 = round (>= 1); every other strand's state is copied and its kept_by and rounds are left alone.  undecided [1]
 *   int32 is ADDED the number of strands undecided in state_out (an integer atomic per wavefront; the caller zeroes it).  state_out
 *   must not be state; no output may alias another buffer. */
#define HGS_DEDUPE_PARTS 8
int hgs_dedupe_count(void* stream, int N, int M, long long n_points, const float* points, double tol, int* counts);
int hgs_dedupe_fill(void* stream, int N, int M, long long n_points, const float* points, double tol, const long long* starts,
                    long long n_pairs, int* lower);
int hgs_dedupe_resolve(void* stream, int N, const long long* lower_offsets, long long n_pairs, const int* lower, const unsigned char* state,
                       unsigned char* state_out, int round, long long* kept_by, int* rounds, int* undecided);

/* Strands traced from the scalp through the lifted hair directions (csrc/hgs_trace.hip; utils/trace.py states the contract and has
 *   the numpy paths).  All float64, one rounding per operation.  Every argument is checked before a pointer is touched.  The grid:
 *   node (ix, iy, iz) lies at origin + index * h, 2 <= n <= 1024 an axis, at most 2^26 nodes in all.
 * hgs_field_splat: points, dirs [N][3] float64 (device), 0 <= N <= 2^24.  A point that is not finite, or whose dot(dir, dir) is not
 *   finite or not > 0, adds one to skipped[0] and nothing else.  The others, with d = dir / sqrt(dot(dir, dir)), add to every node
 *   with d2 = |node - point|^2 < r2, for k = 1 - d2 / r2: rint(k * 2^32) to the node's W and rint((k * (d_a * d_b)) * 2^32) to its
 *   xx, xy, xz, yy, yz, zz.  acc [nz][ny][nx][7] int64 (W, xx, xy, xz, yy, yz, zz) and skipped [1] int32 are ADDED to: the caller
 *   zeroes them, and may splat a cloud in parts.  64-bit integer atomics: the sums are exact, the same bits in any order.
 *   sqrt(r2) <= 8 h.
 * hgs_field_solve: per node, T = Tq * 2^-32; dir [nz][ny][nx][3] = the unit eigenvector of the largest eigenvalue l2, its component
 *   of largest magnitude positive (lowest index on a tie); conf [nz][ny][nx] = l2 - l1; both 0 where W == 0.  Cyclic Jacobi.
 * hgs_strand_trace: roots, p0 [S][3] float64, 0 <= S <= 2^24; dir, conf as above.  One lane per root walks utils/trace.py's loop:
 *   at most max_steps (1 to 4096) steps of length `step` through the field interpolated at t = (x - origin) * (1 / h), the range test
 *   0 <= t < n - 1 in front of every load.  joints [S][max_steps + 1][3] (rows from count on are unspecified), count [S] int32,
 *   reason [S] int32: 0 steps, 1 bounds, 2 turn, 3 gap. */
int hgs_field_splat(void* stream, int N, const double* points, const double* dirs, double ox, double oy, double oz, double h, int nx,
                    int ny, int nz, double r2, long long* acc, int* skipped);
int hgs_field_solve(void* stream, int nx, int ny, int nz, const long long* acc, double* dir, double* conf);
int hgs_strand_trace(void* stream, int S, const double* roots, const double* p0, const double* dir, const double* conf, double ox,
                     double oy, double oz, double h, int nx, int ny, int nz, double step, int max_steps, double cos_max, double min_conf,
                     int max_gap, double* joints, int* count, int* reason);

/* The direction volume filled between the scalp and the visible hair (csrc/hgs_fill.hip; utils/field_fill.py states the contract and
 *   has the numpy path).  All float64, one rounding per operation.  Every argument is checked before a pointer is touched.
 * hgs_field_fill: `sweeps` Jacobi sweeps (0 to 65536) over the F nodes free_index [F] int32 names (ascending node indices of the
 *   nodes whose kind is 1), on the grid of hgs_field_splat.  kind [nz][ny][nx] uint8: 0 out, 1 free, 2 fixed.  a and b, [6][nz][ny][nx]
 *   float64 each (planes xx, xy, xz, yy, yz, zz), both hold the seed on entry; sweep k reads a and writes b for even k, the other way
 *   round for odd k.  A listed node becomes, per plane, the sum of its face neighbours (-x, +x, -y, +y, -z, +z; one that is off the
 *   grid or out adds +0.0) divided by the number that counted, or keeps its value where none did; no other node is written.  The
 *   result is in a for even `sweeps` and in b for odd, the iterate before it in the other buffer.  One plain launch per sweep on
 *   `stream`, no host synchronisation.  F == 0 or sweeps == 0 launches nothing. */
int hgs_field_fill(void* stream, int nx, int ny, int nz, const unsigned char* kind, const int* free_index, int F, double* a, double* b,
                   int sweeps);

/* Tuning knob of the segment-parallel blend (csrc/hgs_blend.hip): tile lists longer than 1.5 segment lengths are walked
 * by one workgroup per segment (the forward walks a list of exactly two segments with one workgroup); the segment length of a pass with R instances is R / target_segments rounded up to a
 * multiple of 64 and clamped to [min_len, max_len] (multiples of 64, min_len >= 128; default 128, 1024, 2048).  Process-wide, takes
 * effect at the next forward pass (a captured graph keeps the policy it was captured with).  Results do not depend
 * on it beyond the association of the per-pixel transmittance product. */
int hgs_set_segment_policy(int min_len, int max_len, int target_segments);
/* Development aid (tools/wg_trace.py): when a buffer of 8 uint64 per workgroup of the blend grid (2 T + 1024 is always
 * enough) is registered, blend_fwd / blend_bwd record per workgroup: start, phase marks 1..5, its work item, end (times
 * from s_memrealtime, 100 MHz); NULL (the default) switches it off. */
int hgs_debug_set_wg_trace(void* device_buf_fwd, void* device_buf_bwd);

/* ---- introspection used by the parity tests (byte offsets of the sub-arrays of each buffer) ---- */
enum { HGS_GEOM_DEPTHS = 0, HGS_GEOM_CLAMPED, HGS_GEOM_MEANS2D, HGS_GEOM_COV3D, HGS_GEOM_CONIC_OPACITY,
       HGS_GEOM_RGB, HGS_GEOM_TILES_TOUCHED, HGS_GEOM_POINT_OFFSETS, HGS_GEOM_RECT, HGS_GEOM_BLOCK_SUMS,
       HGS_GEOM_NFIELDS };
enum { HGS_IMG_FINAL_T = 0, HGS_IMG_N_CONTRIB, HGS_IMG_RANGES, HGS_IMG_TILE_COUNT, HGS_IMG_TILE_CURSOR,
       HGS_IMG_TILE_MAXC, HGS_IMG_STATUS, HGS_IMG_TILE_ORDER, HGS_IMG_NFIELDS };
enum { HGS_BIN_KEYS = 0, HGS_BIN_POINT_LIST, HGS_BIN_PACKED, HGS_BIN_INV, HGS_BIN_KEYS_TMP, HGS_BIN_NFIELDS };
int hgs_geom_layout(int P, size_t* offsets /* [HGS_GEOM_NFIELDS] */);
int hgs_image_layout(int W, int H, size_t* offsets /* [HGS_IMG_NFIELDS] */);
int hgs_binning_layout(int R, size_t* offsets /* [HGS_BIN_NFIELDS] */);

/* status words written by the kernels into image_buf (HGS_IMG_STATUS): [0]=num_rendered, [1]=overflow flag (the pass
 * dropped instances: its image is incomplete and its backward returns exactly zero gradients), [8]=a cooperative wait
 * between workgroups timed out (never expected; results of that pass are invalid); the others are internal */
#define HGS_STATUS_WORDS 16
/* floats per packed instance record in HGS_BIN_PACKED, 3-channel mode: x,y, conic a,b,c, opacity, r,g,b, id, quadrant
 * mask, pad (the 7-channel mode uses 16: ..., 7 features, id, quadrant mask, pad) */
#define HGS_PACKED_FLOATS 12
/* floats per instance in the backward scratch: sums over the tile's pixels of u dx, u dy, u dx dx, u dx dy, u dy dy, u
 * (u = G dL/dalpha, d = mean - pixel; the moments from which dmean2D, dconic and dopacity follow per Gaussian), dcolor.rgb,
 * pad */
#define HGS_INST_GRAD_FLOATS 12

#ifdef __cplusplus
}
#endif
#endif /* HGS_H_INCLUDED */
