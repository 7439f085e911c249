/* se3ds_hip.h -- C ABI of libse3ds_hip.so: the MI355X (gfx950) kernels behind the SE3DS hot
 * path.  The reference (google-research/se3ds) has no FFI of its own: its "native layer" is
 * the set of TensorFlow / tensorflow-addons ops its Python calls.  Each entry point below
 * replaces the TF op sequence at the cited reference lines; INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - raw DEVICE pointers + explicit sizes; `stream` is a hipStream_t passed as void*
 *   - returns 0 on success or a negative SE3DS_E_* code; never throws, never allocates,
 *     never synchronises the stream, owns nothing; re-entrant for distinct streams
 *   - scratch memory comes from the caller (`*_workspace_bytes` query functions)
 *   - tensors are dense, row-major, NHWC for images; fp32 unless a dtype code says otherwise
 */
#ifndef SE3DS_HIP_H_
#define SE3DS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SE3DS_OK 0
#define SE3DS_E_BADSHAPE (-1)
#define SE3DS_E_BADDTYPE (-2)
#define SE3DS_E_WORKSPACE (-3)
#define SE3DS_E_LAUNCH (-4)
#define SE3DS_E_UNSUPPORTED (-5)

/* element type codes */
#define SE3DS_F32 0
#define SE3DS_I32 1
#define SE3DS_U8 2
#define SE3DS_BF16 3
/* OR-ed into the `feat_dtype` of the splat entry points (se3ds_project_equirect*,
 * se3ds_project_to_feat) together with SE3DS_I32: the caller PROMISES that every feature of a
 * valid point -- one whose channels all differ from `input_void` -- is an integer in [0, 255]
 * (RGB memories: int32 in [-1, 255] with void -1, reference models/models.py:127-134,325-331).
 * The splat then moves 8-byte packed records instead of 20-byte ones.  SE3DS_U8 features need no
 * promise.  A broken promise is detected (se3ds_splat_promise_broken) but the outputs of that
 * call are undefined. */
#define SE3DS_FEAT_BYTE_RANGE 0x100
/* OR-ed into the `feat_dtype` of se3ds_unproject_equirect_into / se3ds_warp_views_to_target: the caller
 * guarantees that row 3 of xyz1 (the homogeneous 1, models/models.py:225-226 adds 0 to it) ALREADY holds
 * 1.0 in the window being written -- a point-cloud memory fills that row once when it is allocated -- and
 * the kernel does not write it again: 40 instead of 44 bytes per pixel (round 6; the splat never reads
 * the row, the memory keeps it for callers of the (N,4,M) view). */
#define SE3DS_XYZ1_ONES_PRESET 0x200

/* Library / build identification: returns a static string "se3ds_hip <abi> gfx950". */
const char* se3ds_version(void);
/* HIP error string of the last failed launch on this thread (or ""). */
const char* se3ds_last_error(void);

/* ======================================================================================
 * Geometry (point-cloud warp)
 * ====================================================================================== */

/* equirectangular_to_pointcloud -- reference utils/pano_utils.py:164-242 (core :219-242).
 * feats (N,H,W,C) of `feat_dtype`, depth (N,H,W) fp32 in [0,1].  sin_el/cos_el (H) and
 * sin_hd/cos_hd (W) are the fp32 sin/cos tables of the half-pixel-centre elevation/heading
 * grids (:211-218), built on the host.  `position` (N,3) is optional (may be NULL) and is
 * ADDED to xyz after the unprojection (models/models.py:225-226 `xyz1 += position`, the
 * 4th row gets += 0).  Outputs: xyz1 (N,4,H*W) fp32, feats_out (N,H*W,C) same dtype with
 * `void_class` where depth is not in (0,1). */
int se3ds_unproject_equirect(const void* feats, int feat_dtype, const float* depth,
                             const float* sin_el, const float* cos_el, const float* sin_hd,
                             const float* cos_hd, const float* position, int n, int height,
                             int width, int channels, float void_class, float depth_scale,
                             float* xyz1, void* feats_out, void* stream);

/* The same, written straight into a point-cloud MEMORY (the concat of models/models.py:239-245
 * and utils/eval_metric.py:238-239 without the copy): xyz1 is (N,4,m_total) and feats_out
 * (N,m_total,C); this view fills columns / rows [m_offset, m_offset + H*W). */
int se3ds_unproject_equirect_into(const void* feats, int feat_dtype, const float* depth,
                                  const float* sin_el, const float* cos_el, const float* sin_hd,
                                  const float* cos_hd, const float* position, int n, int height,
                                  int width, int channels, float void_class, float depth_scale,
                                  float* xyz1, void* feats_out, int64_t m_total, int64_t m_offset,
                                  void* stream);

/* Scratch bytes for the two splat entry points below. */
size_t se3ds_splat_workspace_bytes(int n, int64_t m, int height, int width, int channels);

/* project_feats_to_equirectangular -- reference utils/pano_utils.py:117-161 fused with
 * utils/point_cloud_utils.py:90-183 (project_to_feat) and, optionally, the mask of
 * models/models.py:282-287.
 * xyz1 (N,4,M) fp32 world coords; `offset` (N,3) optional, SUBTRACTED first
 * (models.py:273-275 / eval_metric.py:162 `memory - position`).  feats (N,M,C) of
 * `feat_dtype` (cast to fp32 as pano_utils.py:159 does).  Outputs: depth (N,H,W) in [0,1],
 * feat (N,H,W,C) fp32, mask (N,H,W) fp32 {0,1} or NULL
 * (mask = depth in (0,1) and all(feat != mask_void)).
 * Semantics kept from the reference: invalid / culled points scatter into flat index 0
 * (batch 0, pixel (0,0)); 0.1 m tolerance; per-channel max over all survivors. */
int se3ds_project_equirect(const float* xyz1, const float* offset, const void* feats,
                           int feat_dtype, int n, int64_t m, int channels, int height, int width,
                           float depth_scale, float input_void, float output_void, float* depth,
                           float* feat, float* mask, float mask_void, void* workspace,
                           size_t workspace_bytes, void* stream);

/* Number of elements of an int32 / uint8 feature array that are neither `void_class` nor an
 * integer in [0, 255]: 0 means SE3DS_FEAT_BYTE_RANGE may be promised for it.  *bad_out is a
 * device uint32 (written, not accumulated). */
int se3ds_feats_byte_range(const void* feats, int feat_dtype, int64_t count, float void_class,
                           uint32_t* bad_out, void* stream);
/* After a packed / sorted splat call (same workspace, same n / m): *broken_out (device uint32) = 1
 * if a valid point of THAT call violated the SE3DS_FEAT_BYTE_RANGE promise, else 0 (the verdict is
 * an epoch the violating workgroups exchange into the workspace: nothing is zeroed per call). */
int se3ds_splat_promise_broken(const void* workspace, int n, int64_t m, uint32_t* broken_out,
                               void* stream);
/* The same verdict, STICKY over calls: header word 3 of a splat workspace (byte 12) is OR-ed with 1
 * by every packed / sorted splat that meets a feature outside [0, 255] under the promise, and is
 * never cleared by the library.  The caller zeroes the first 256 bytes of a workspace once, and
 * reads the flag whenever convenient (e.g. every n-th call, asynchronously): a broken promise is
 * then detected late, never missed.  clear != 0 resets the word after reading it. */
int se3ds_splat_promise_sticky(void* workspace, uint32_t* broken_out, int clear, void* stream);

/* The same over the first `m` points of a preallocated point-cloud MEMORY of `capacity` points
 * per image -- xyz1 (N,4,capacity), feats (N,capacity,C) -- so that a trajectory appends frames in
 * place (se3ds_unproject_equirect_into) and renders without ever concatenating or copying the
 * memory (utils/eval_metric.py:162-165,236-239; trainers/gan_manager.py:476-485,540-541). */
int se3ds_project_equirect_memory(const float* xyz1, const float* offset, const void* feats,
                                  int feat_dtype, int n, int64_t m, int64_t capacity, int channels,
                                  int height, int width, float depth_scale, float input_void,
                                  float output_void, float* depth, float* feat, float* mask,
                                  float mask_void, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* One trajectory step as ONE host call: `views` source panoramas are unprojected into consecutive
 * windows [m_offset + v*H*W, ...) of a point-cloud memory (se3ds_unproject_equirect_into each, with
 * view_position[v] (N,3) added, or view_position == NULL) and ONE target is rendered from the
 * memory's first m_offset + views*H*W points, relative to `target` (N,3)
 * (se3ds_project_equirect_memory) -- utils/eval_metric.py:153-166,233-240 and the RE10K notebook's
 * cell 15 per step, trainers/gan_manager.py:476-485,540-541.  view_feats / view_depth /
 * view_position are HOST arrays of `views` device pointers.  The launches are queued back to
 * back: from Python the four separate calls of a 2-view step cost 154 us of host time for 124 us
 * of kernels.  feat_dtype may carry SE3DS_FEAT_BYTE_RANGE (a promise about every view's features
 * AND what the memory already holds).  views == 0 renders the memory as it is. */
int se3ds_warp_views_to_target(const void* const* view_feats, int feat_dtype,
                               const float* const* view_depth, const float* const* view_position,
                               int views, int n, int height, int width, int channels,
                               float void_class, float depth_scale, const float* sin_el,
                               const float* cos_el, const float* sin_hd, const float* cos_hd,
                               float* mem_xyz1, void* mem_feats, int64_t capacity, int64_t m_offset,
                               const float* target, int out_height, int out_width,
                               float output_void, float* depth, float* feat, float* mask,
                               float mask_void, void* workspace, size_t workspace_bytes,
                               void* stream);

/* project_to_feat -- reference utils/point_cloud_utils.py:90-183 on already transformed
 * coordinates (N,4,M) = (x, y, z, 1).  Same outputs/semantics as above. */
int se3ds_project_to_feat(const float* coords, const void* feats, int feat_dtype, int n, int64_t m,
                          int channels, int height, int width, float depth_scale,
                          float input_void, float output_void, float* depth, float* feat,
                          float* mask, float mask_void, void* workspace, size_t workspace_bytes,
                          void* stream);

/* Debug/parity tap: first-stage flat indices of the last se3ds_project_* call that used
 * `workspace` (int32 per point: index inside the image v*W+u, or -1 = sink) and z. */
int se3ds_splat_debug_indices(const void* workspace, int n, int64_t m, int32_t* idx_out,
                              float* z_out, void* stream);

/* Debug/parity tap: the DEVICE evaluation of the fast index screen (se3ds_geom_math.h) on
 * camera-relative xyz (3,M): fx, fy as the screen computes them and its verdict per point
 * (>= -1: decided index v*W+u or -1 = not a valid splat; -2: left to the exact chain). */
int se3ds_debug_fast_fxy(const float* xyz, int64_t m, int width, int height, float* fx, float* fy,
                         int32_t* verdict, void* stream);

/* get_filtered_coords_and_feats -- reference utils/point_cloud_utils.py:32-87 (perspective,
 * 90 deg HFOV).  feats (N,H,W,C) int32, depth (N,H,W) fp32; xs (W), ys (H) are the fp32
 * linspace(-1,1) grids and kinv (4x4 row-major) the inverse intrinsics, built on the host.
 * Outputs xyz (N,4,H*W) fp32, feats_out (N,H*W,C) fp32. */
int se3ds_unproject_perspective(const int32_t* feats, const float* depth, const float* xs,
                                const float* ys, const float* kinv, int n, int height, int width,
                                int channels, float depth_scale, float* xyz, float* feats_out,
                                void* stream);

/* tfa.image.interpolate_bilinear -- called at utils/pano_utils.py:339,412,472.
 * grid (B,H,W,C) fp32, query (B,Q,2) fp32, out (B,Q,C) fp32.  indexing_xy: 0 = 'ij'
 * (query = (row, col)), 1 = 'xy' (query = (x, y)). */
int se3ds_interp_bilinear(const float* grid, const float* query, int b, int height, int width,
                          int channels, int64_t q, int indexing_xy, float* out, void* stream);

/* Coordinate generation of rotate_pano -- utils/pano_utils.py:326-338.  rays (3,Q) fp32
 * (equirectangular_pixel_rays), matrix (N,3,3); out (N,Q,2) = (pitch_px, heading_px) for a
 * source pano of src_h x src_w. */
int se3ds_rotate_coords(const float* rays, const float* matrix, int n, int64_t q, int src_h,
                        int src_w, float* out, void* stream);

/* Coordinate generation of project_perspective_image -- utils/pano_utils.py:387-402.
 * rays (3,Q), world_to_image (3,3); out (Q,2) = xy/z where z > 0 else -1, optional
 * round-half-even, plus `add` (1.0 when the image was padded by one pixel, :409). */
int se3ds_perspective_coords(const float* rays, const float* w2i, int64_t q, int round_nearest,
                             float add, float* out, void* stream);

/* Coordinate generation of get_perspective_from_equirectangular_image --
 * utils/pano_utils.py:459-469.  m (3,3) = K^-T . R applied as xyz_row . kinv_t then . rot
 * (two fp32 3x3 products per pixel, in that order); out (height*width, 2) = (u, v). */
int se3ds_persp_from_equirect_coords(const float* kinv_t, const float* rot, int height, int width,
                                     int eq_h, int eq_w, float* out, void* stream);

/* Fused perspective paths (notebooks/SE3DS_RE10K_Colab.ipynb cells 15, 17).
 * se3ds_perspective_to_pointcloud = project_perspective_image(image) and (depth)
 * (utils/pano_utils.py:344-417, constant padding `pad_value`), int32(image * 255), and
 * equirectangular_to_pointcloud (:164-242, + optional position (3)) without the two equirect
 * intermediates: image (ih,iw,C<=4) fp32, depth (ih,iw) fp32, rays (3,H*W) = equirectangular
 * pixel rays, w2i (3,3) = get_world_to_image_transform; outputs xyz1 (1,4,H*W), feats (1,H*W,C)
 * int32.  se3ds_perspective_guidance = the three get_perspective_from_equirectangular_image
 * calls (:443-476) of cell 17 on the splat outputs pred_rgb (H,W,3) / pred_depth (H,W) -- RGB,
 * depth, and the mask (depth != 0, != 1, all(rgb != 0)) -- with the glue: rgb / 255 clipped,
 * mask == 1, products with the mask: proj_image (h,w,3), proj_depth (h,w), proj_mask (h,w). */
int se3ds_perspective_to_pointcloud(const float* image, const float* depth, int ih, int iw,
                                    int channels, const float* rays, const float* w2i,
                                    int round_nearest, float pad_value, const float* sin_el,
                                    const float* cos_el, const float* sin_hd, const float* cos_hd,
                                    const float* position, int height, int width, float void_class,
                                    float depth_scale, float* xyz1, int32_t* feats_out, void* stream);
int se3ds_perspective_guidance(const float* pred_rgb, const float* pred_depth, int eq_h, int eq_w,
                               const float* kinv_t, const float* rot, int height, int width,
                               float* proj_image, float* proj_depth, float* proj_mask,
                               void* stream);

/* tf.image.resize with half-pixel centres on an NHWC tensor (F32 / I32 / U8): method 0 = nearest
 * (output of the input dtype), 1 = bilinear (fp32 output, antialias off).  Callers:
 * utils/pano_utils.py:203-208 (equirectangular_to_pointcloud with size_mult != 1) and :299-301
 * (crop_pano(resize_to_original=True): an up-scaling, where TF's antialias=True changes nothing). */
int se3ds_resize(const void* x, int dtype, int n, int h, int w, int c, int oh, int ow, int method,
                 void* y, void* stream);
/* *out = mean(x[0..n)) accumulated in binary64: the padding value of
 * project_perspective_image(pad_mode='mean'), utils/pano_utils.py:403-407. */
int se3ds_mean_f32(const float* x, int64_t n, float* out, void* stream);

/* mask_pano -- utils/pano_utils.py:245-265: rows [mh, H-mh] kept, others := value. */
int se3ds_mask_pano(const void* pano, int dtype, int n, int height, int width, int channels,
                    int masked_height, float value, void* out, void* stream);

/* Stream compaction of valid points -- models/models.py:229-236.  Keeps point j iff
 * any(feats[:, j, :] != void) over batch and channel.  xyz1 (N,4,M), feats (N,M,C) of dtype.
 * Outputs xyz1_out (N,4,M) / feats_out (N,M,C) hold `*count` points per row with the
 * compacted stride `out_stride` (== M); count_out is a DEVICE int64.  workspace:
 * se3ds_compact_workspace_bytes(m). */
size_t se3ds_compact_workspace_bytes(int64_t m);
int se3ds_compact_valid(const float* xyz1, const void* feats, int feat_dtype, int n, int64_t m,
                        int channels, float void_class, float* xyz1_out, void* feats_out,
                        int64_t* count_out, void* workspace, size_t workspace_bytes, void* stream);

/* ======================================================================================
 * Convolutions (implicit GEMM on MFMA; NHWC; dtype = SE3DS_F32 or SE3DS_BF16, fp32 accumulate)
 * Geometry arguments always describe the ASSOCIATED FORWARD CONV: input (n,h,w,cin), output
 * (n,ho,wo,cout), kernel kh x kw, stride (1|2), explicit top/left zero padding (the bottom /
 * right padding follows from ho/wo), wrap_w = circular padding along W (PadLayer at
 * inference, models/layers.py:67-72; stride 1 and wo == w only).
 * ====================================================================================== */

/* fp32 master kernel HWIO viewed [K = kh*kw*cin][cout] -> compute-dtype operand copies:
 * wt [cout][K] (forward operand) and, if non-NULL, wn [K][cout] (input-gradient operand). */
int se3ds_weight_prep(const float* w, int64_t k, int cout, int dtype, void* wt, void* wn,
                      void* stream);
/* The same for MANY layers in one launch (bf16 only; every layer needs k % 8 == 0, cout % 4 == 0,
 * 16-byte aligned w / wt, 8-byte aligned wn): `table` is a device int64 [nlayers][6] =
 * {w, k, cout, wt, wn, first 64 x 64 tile}, total_tiles the sum of ceil(k/64) * ceil(cout/64).
 * The trainer refreshes a whole module's operand copies behind its Adam update with it. */
#define SE3DS_WEIGHT_PREP_FIELDS 6
int se3ds_weight_prep_multi(const int64_t* table, int nlayers, int64_t total_tiles, void* stream);

/* y = epilogue(conv(x * in_mask, W)).  Replaces tf.nn.conv2d at models/layers.py:193-198
 * (PartialConv), :334-339 (SpectralConv), Keras Conv2D (image_models.py:513-517,542-543),
 * and is the input-gradient of Conv2DTranspose.  in_mask (n,h,w) fp32 or NULL;
 * in_mask_binary != 0 promises that it only holds 0.0 / 1.0 (the reference's masks are binary),
 * which lets masked pixels be fetched from a zero page by the LDS-DMA kernel.  Epilogue:
 *   t = acc * (*scale)                                  scale: device scalar or NULL
 *   row_a != NULL, bias != NULL: t = ((t - b)*row_a + b) * row_b   (layers.py:199-202)
 *   row_a != NULL, bias == NULL: t = t * row_a                     (layers.py:203-204)
 *   row_a == NULL, bias != NULL: t = t + b
 *   act: 0 none, 1 ReLU, 2 LeakyReLU(act_alpha)
 * row_a / row_b are (n*ho*wo) fp32 vectors (mask_ratio / update_mask). */
int se3ds_conv2d_fwd(const void* x, const void* wt, void* y, int dtype, int n, int h, int w,
                     int cin, int ho, int wo, int cout, int kh, int kw, int stride, int pad_t,
                     int pad_l, int wrap_w, const float* in_mask, int in_mask_binary,
                     const float* scale, const float* bias, const float* row_a,
                     const float* row_b, int act, float act_alpha, void* stream);

/* Keras Conv2DTranspose, 2x2 kernel, stride 2 (layers.py:475-480 residual upsampling;
 * image_models.py:440-441 final_deconv): y (n, 2 hi, 2 wi, cout) from x (n, hi, wi, cin).  `wn` is
 * the compute-dtype copy of the kernel in its own layout (ky, kx, cout, cin) -- se3ds_weight_prep's
 * second output for the layer.  Each output pixel sees exactly one tap, so the layer is two 1x1
 * forward convolutions (one per output row parity) with 2 * cout "channels" (kx, co) whose results
 * are contiguous in y: round 5 replaces the four parity-class passes of se3ds_conv2d_dgrad (K = cin:
 * two K steps per 128 x 128 tile, 256-byte output pieces) by 256-wide tiles writing 512-byte runs.
 * bias (cout floats) or NULL. */
int se3ds_conv_transpose2x2_fwd(const void* x, const void* wn, void* y, int dtype, int n, int hi, int wi,
                                int cin, int cout, const float* bias, void* stream);

/* Forward conv that also emits the batch-norm statistics of its (rounded) output, so that
 * SyncBatchNormalization (models/layers.py BN after conv) needs no separate pass over y:
 * stats[row][2][cout] = per-row-block (sum, sum of squares) over the stored outputs, with
 * rows = se3ds_conv2d_fwd_stats_rows(...) (0: this shape has no fused path, use
 * se3ds_conv2d_fwd + se3ds_norm_stats).  Reduce with se3ds_norm_reduce_rows. */
int64_t se3ds_conv2d_fwd_stats_rows(int dtype, int n, int cin, int ho, int wo, int cout, int kh,
                                    int kw, int stride, int has_in_mask, int in_mask_binary);
int se3ds_conv2d_fwd_stats(const void* x, const void* wt, void* y, int dtype, int n, int h, int w,
                           int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                           int pad_t, int pad_l, int wrap_w, const float* in_mask,
                           int in_mask_binary, const float* scale, const float* bias,
                           const float* row_a, const float* row_b, int act, float act_alpha,
                           float* stats, void* stream);

/* dx = epilogue(conv_transpose(dy, W)): the input-gradient of the conv above AND the forward
 * of Keras Conv2DTranspose (models/layers.py:417-423,475-480; image_models.py:440-441), whose
 * kernel (kh,kw,Cout_T,Cin_T) is the HWIO kernel of the associated forward conv.  wn is the
 * [K][cout] operand copy.  dy_row_scale (n*ho*wo) optionally multiplies dy rows (partial
 * conv: ratio*update_mask).  Epilogue: t = acc*(*scale); row_a (n*h*w): t *= row_a (the
 * partial conv's input mask); bias (cin) added when given (ConvT bias); act as above. */
int se3ds_conv2d_dgrad(const void* dy, const void* wn, void* dx, int dtype, int n, int h, int w,
                       int cin, int ho, int wo, int cout, int kh, int kw, int stride, int pad_t,
                       int pad_l, int wrap_w, const float* dy_row_scale, const float* scale,
                       const float* bias, const float* row_a, int act, float act_alpha,
                       void* stream);
/* The same with dx = result + addend (addend: same layout / dtype as dx, may be dx itself): the
 * gradient of a tensor with two consumers (a ResNet block's input) without an extra pass. */
int se3ds_conv2d_dgrad_acc(const void* dy, const void* wn, void* dx, int dtype, int n, int h, int w,
                       int cin, int ho, int wo, int cout, int kh, int kw, int stride, int pad_t,
                       int pad_l, int wrap_w, const float* dy_row_scale, const float* scale,
                       const float* bias, const float* row_a, int act, float act_alpha,
                       const void* addend, void* stream);

/* Data gradient with FUSED batch-norm backward statistics (round 3).  dx (+ addend when given)
 * is the gradient of y = act(norm(bn_x) [+ res]), the output of a SyncBatchNormalization
 * (tf.keras.layers.experimental.SyncBatchNormalization behind models/layers.py:241-251,
 * 424-444); besides dx the epilogue emits stats[rows][2][cin] = per 64-pixel tile
 * (sum dz, sum dz * xhat) with dz = dx_stored * act'(y) (bn_mask: one "y > 0" bit per element,
 * or NULL without activation; bn_act 0 / 1 relu / 2 leaky relu with slope bn_alpha) and
 * xhat = (bn_x - bn_mean) * bn_rstd -- the sums se3ds_norm_bwd_stats takes from a second pass over
 * dx and bn_x.  se3ds_norm_reduce_rows_dst reduces the rows (and writes the beta / gamma
 * gradients).  _rows returns 0 when this shape cannot (strided, fp32, thin / ragged channels,
 * a dy row scale): call se3ds_conv2d_dgrad[_acc] and se3ds_norm_bwd_stats then. */
int64_t se3ds_conv2d_dgrad_bnstats_rows(int dtype, int n, int h, int w, int cin, int cout, int kh,
                                        int kw, int stride, int has_row_scale);
int se3ds_conv2d_dgrad_bnstats(const void* dy, const void* wn, void* dx, int dtype, int n, int h,
                               int w, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                               int pad_t, int pad_l, int wrap_w, const float* scale,
                               const float* row_a, const void* addend, const void* bn_x,
                               const uint8_t* bn_mask, const float* bn_mean, const float* bn_rstd,
                               int bn_act, float bn_alpha, float* stats, void* stream);

/* dW[kh,kw,cin,cout] (fp32) (+)= (*out_scale) * sum_pixels (x*in_mask)^T (dy*row_scale).
 * The reduction over n*ho*wo is split across workgroups and reduced deterministically. */
size_t se3ds_conv2d_wgrad_workspace_bytes(int n, int ho, int wo, int cin, int cout, int kh,
                                          int kw);
int se3ds_conv2d_wgrad(const void* x, const void* dy, float* dw, int dtype, int n, int h, int w,
                       int cin, int ho, int wo, int cout, int kh, int kw, int stride, int pad_t,
                       int pad_l, int wrap_w, const float* in_mask, int in_mask_binary,
                       const float* row_scale, const float* out_scale, int accumulate,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The same without its final split reduction (round 4): the partial slabs stay in `workspace`
 * (which the caller therefore keeps per layer until the reduction has run) and reduce_row (HOST
 * memory, 5 x int64) receives [slabs, splits, n / 4, dw, 1]; rows of many layers go to ONE
 * se3ds_wgrad_reduce_multi launch (device table of such rows with the 5th field replaced by the
 * row's first workgroup: running sum of ceil(n4 / se3ds_wgrad_reduce_tile())).  When the 16-byte
 * reduction does not apply (ragged sizes), the reduction is launched as usual and reduce_row[4]
 * stays 0.  Bit-identical to se3ds_conv2d_wgrad.  Same reference semantics: the kernel gradient of
 * tf.nn.conv2d (models/layers.py:153,193,334). */
int se3ds_conv2d_wgrad_partial(const void* x, const void* dy, float* dw, int dtype, int n, int h,
                               int w, int cin, int ho, int wo, int cout, int kh, int kw, int stride,
                               int pad_t, int pad_l, int wrap_w, const float* in_mask,
                               int in_mask_binary, const float* row_scale, void* workspace,
                               size_t workspace_bytes, int64_t* reduce_row, void* stream);
int se3ds_wgrad_reduce_multi(const int64_t* table, int rows, int64_t workgroups, void* stream);
int se3ds_wgrad_reduce_tile(void);
/* n / d as the convolution kernels compute it for tile row -> (image, row, column): the host-made
 * multiplier and shifts, evaluated on the host (test hook: no device work).  d >= 1. */
uint32_t se3ds_fastdiv_host(uint32_t n, uint32_t d);
/* Which kernel the convolution dispatchers chose (test hooks: host only, no device work, per host
 * thread).  Every launch of the family -- forward / data gradient / weight gradient and its split
 * reduction, the swapped weight gradient and its helpers, weight prep -- records one small integer
 * that names the template instantiation (tile shape, MFMA shape, dtype, mode, fused-BN flag).
 * _last_conv_route: the calling thread's most recent launch, -1 before the first.
 * _conv_route_history(back): the launch `back` launches earlier (0 = the last; the ring keeps 8).
 * _conv_route_name(route): its name, or NULL for route < 0 or past the last route -- iterate from 0
 * to enumerate all routes (tests/test_conv_lattice_gpu.py keeps one bit-exact case per name). */
int se3ds_debug_last_conv_route(void);
int se3ds_debug_conv_route_history(int back);
const char* se3ds_debug_conv_route_name(int route);

/* Weight gradient of a THIN-Cout (cout <= 16), stride-1, same-size conv (the generator's
 * 128->3 / 128->1 output convs, image_models.py:93-104) computed with the operand roles
 * swapped: sum_l dy[l - tap, co] * x[l, ci] is the weight gradient of a conv whose INPUT is dy and
 * whose output gradient is x, with the taps mirrored.  The thin operand then packs into one
 * linear-K tile and x is streamed once instead of kh*kw times. */
size_t se3ds_conv2d_wgrad_swapped_workspace_bytes(int n, int h, int w, int cin, int cout, int k);
int se3ds_conv2d_wgrad_swapped(const void* x, const void* dy, float* dw, int dtype, int n, int h,
                               int w, int cin, int cout, int k, int pad, int accumulate,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Partial-conv mask statistics -- models/layers.py:153-163: cnt = window sum of the mask
 * (n,h,w); ratio = kh*kw/(cnt+1e-6)*clip(cnt,0,1); um = clip(cnt,0,1); optionally
 * ru = ratio*um and bu = (1-ratio)*um (backward helpers).  All (n,ho,wo) fp32. */
int se3ds_mask_window(const float* mask, int n, int h, int w, int ho, int wo, int kh, int kw,
                      int stride, int pad_t, int pad_l, int wrap_w, float* ratio, float* um,
                      float* ru, float* bu, void* stream);

/* se3ds_norm_reduce_rows + se3ds_norm_finalize in one launch for the single-replica batch norm
 * whose column statistics came out of the producing convolution's epilogue (rows <= 2048 partial
 * rows of [2][c]); bit-identical to the pair.  Replaces the statistics half of
 * tf.keras.layers.experimental.SyncBatchNormalization (image_models.py:170-176). */
int se3ds_norm_reduce_rows_finalize(const float* partial, int64_t rows, int c, float count,
                                    const float* gamma, const float* beta, float eps, float momentum,
                                    float* moving_mean, float* moving_var, float* scale, float* shift,
                                    float* mean, float* rstd, void* stream);

/* One pass over dy [r][c] (bf16, c % 8 == 0) for the backward of a partial convolution with bias:
 * scaled_out = dy * out_row_scale[row]  (what se3ds_row_scale would write: the renormalised output
 * gradient the LDS-DMA data / weight gradient kernels take) and colsum_out[c] = sum_rows dy *
 * sum_row_scale[row] (the bias gradient, models/layers.py:199-203).  sums: [1][2][c] scratch like
 * se3ds_norm_stats.  SE3DS_E_UNSUPPORTED for other layouts (callers use the two separate calls). */
int se3ds_colsum_row_scale(const void* x, int dtype, int64_t r, int c, const float* sum_row_scale,
                           const float* out_row_scale, void* scaled_out, float* sums,
                           float* colsum_out, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ======================================================================================
 * Normalisation: tensors viewed as [g][r][c]; g = 1 for SyncBatchNormalization (279 sites in
 * the generator, e.g. models/layers.py:235-251), g = batch for tfa InstanceNormalization
 * (image_models.py:534).  sums are [g][2][c] fp32.
 * ====================================================================================== */
size_t se3ds_norm_workspace_bytes(int g, int c);
/* sums[g][0][c] = sum_r x*row_scale, sums[g][1][c] = sum_r (x*row_scale)^2 (row_scale may be NULL);
 * also the column-sum primitive behind bias gradients: colsum_out (c floats, may be NULL)
 * additionally receives sums[0][0][:] (written straight into a gradient arena). */
int se3ds_norm_stats(const void* x, int dtype, int g, int64_t r, int c, const float* row_scale,
                     float* sums, float* colsum_out, void* workspace, size_t workspace_bytes,
                     void* stream);
/* sums[2][c] = sum over rows of partial[rows][2][c] (deterministic; workspace of
 * se3ds_norm_workspace_bytes(ceil(rows/512), c) bytes for rows > 2048). */
int se3ds_norm_reduce_rows(const float* partial, int64_t rows, int c, float* sums, void* workspace,
                           size_t workspace_bytes, void* stream);
/* The same; dst0 / dst1 (c floats each, may be NULL) additionally receive sums[0][:] / sums[1][:]
 * (the beta / gamma gradients when the rows are fused batch-norm backward statistics). */
int se3ds_norm_reduce_rows_dst(const float* partial, int64_t rows, int c, float* sums, float* dst0,
                               float* dst1, void* workspace, size_t workspace_bytes, void* stream);
/* mean = S0/count, var = S1/count - mean^2 (biased); scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale; moving stats (c) updated in place unless NULL;
 * use_moving != 0: inference (statistics from moving_mean / moving_var). */
int se3ds_norm_finalize(const float* sums, float count, int g, int c, const float* gamma,
                        const float* beta, float eps, float momentum, float* moving_mean,
                        float* moving_var, int use_moving, float* scale, float* shift, float* mean,
                        float* rstd, void* stream);
/* y = act(x*scale + shift [+ res]) [+ post]  (scale/shift are [g][c]).
 * act_mask (bf16, c % 8 == 0; may be NULL): g*r*c/8 bytes, bit e of byte i = (y[8*i + e] > 0).
 * The backward entry points below take the same buffer and then do not read y (16x less
 * traffic for the activation derivative); with act_mask == NULL they read y. */
int se3ds_norm_apply(const void* x, int dtype, int g, int64_t r, int c, const float* scale,
                     const float* shift, const void* res, const void* post, int act, float alpha,
                     void* y, void* act_mask, void* stream);
/* sums[g][0][c] = sum dpre, sums[g][1][c] = sum dpre*xhat with dpre = dy*act'(y).  For g == 1
 * dbeta_out / dgamma_out (c floats, may be NULL) receive the two rows directly. */
int se3ds_norm_bwd_stats(const void* dy, const void* y, const void* x, int dtype, int g, int64_t r,
                         int c, const float* mean, const float* rstd, int act, float alpha,
                         float* sums, float* dbeta_out, float* dgamma_out, const void* act_mask,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dx = gamma*rstd*(dpre - S0/count - xhat*S1/count); dres = dpre when non-NULL.
 * in_act != 0: x is itself the output of activation in_act (alpha in_alpha) whose producer
 * skips its own derivative pass: dx is additionally multiplied by act'(x). */
int se3ds_norm_bwd_apply(const void* dy, const void* y, const void* x, int dtype, int g, int64_t r,
                         int c, const float* mean, const float* rstd, const float* gamma,
                         const float* sums, float count, int act, float alpha, void* dx,
                         void* dres, const void* act_mask, int in_act, float in_alpha,
                         void* stream);
/* se3ds_norm_bwd_apply for a SyncBatchNormalization (one group, bf16, c % 8 == 0) whose input x
 * is the output of a PartialConv with a bias (models/layers.py:100-209) and this norm its only
 * consumer: dx is stored pre-scaled by out_row[row] (mask_ratio * update_mask, the multiplier of
 * layers.py:199-204 the conv's weight / data gradients need) and colsum_dst[c] = sum over rows of
 * the rounded dx * sum_row[row] (update_mask: the bias gradient) -- what se3ds_colsum_row_scale
 * takes from a pass of its own over dx.  workspace: se3ds_norm_workspace_bytes(3, c).
 * SE3DS_E_UNSUPPORTED where the fast kernel does not apply. */
int se3ds_norm_bwd_apply_rows(const void* dy, const void* x, int dtype, int64_t r, int c,
                              const float* mean, const float* rstd, const float* gamma,
                              const float* sums, float count, int act, float alpha, void* dx,
                              void* dres, const void* act_mask, const float* sum_row,
                              const float* out_row, float* colsum_dst, void* workspace,
                              size_t workspace_bytes, void* stream);
/* Batch-norm backward (one group, bf16) in TWO launches instead of three (round 5): statistics
 * partials + apply in the channel-group layout (64 channels = one 128-byte line per row and
 * workgroup); every apply workgroup folds the <= 64 partial rows of its own channels in a prologue,
 * the stand-alone column reduction between se3ds_norm_bwd_stats and se3ds_norm_bwd_apply is gone
 * (layers.py:235-251: the backward of every BatchNormalization of the generator).  dbeta_out /
 * dgamma_out (c floats, or NULL) receive sum dz / sum dz * xhat, sums_out ([2][c] or NULL) both.
 * With sum_row / out_row (the rows variant, se3ds_norm_bwd_apply_rows): dx is stored pre-scaled and
 * colpart[se3ds_norm_bwd_cg_col_rows(r, c)][c] receives the bias-gradient partials as compact slabs
 * -- reduce them with se3ds_wgrad_reduce_multi (row: colpart, rows, c / 4, destination).
 * workspace: se3ds_norm_bwd_cg_workspace_bytes(c).  SE3DS_E_UNSUPPORTED where
 * se3ds_norm_bwd_cg_supported() is 0 (c % 64, c < 512, other dtypes; SE3DS_NORM_CG=0). */
int se3ds_norm_bwd_cg_supported(int dtype, int64_t r, int c, int act, int has_mask, int in_act);
size_t se3ds_norm_bwd_cg_workspace_bytes(int c);
int se3ds_norm_bwd_cg_col_rows(int64_t r, int c);
int se3ds_norm_bwd_cg(const void* dy, const void* x, int dtype, int64_t r, int c, const float* mean,
                      const float* rstd, const float* gamma, float count, int act, float alpha,
                      void* dx, void* dres, const void* act_mask, int in_act, float in_alpha,
                      float* dbeta_out, float* dgamma_out, float* sums_out, const float* sum_row,
                      const float* out_row, float* colpart, void* workspace, size_t workspace_bytes,
                      void* stream);
/* inference-mode backward: dx = dpre*scale; dres = dpre. */
int se3ds_affine_bwd(const void* dy, const void* y, int dtype, int g, int64_t r, int c,
                     const float* scale, int act, float alpha, void* dx, void* dres,
                     const void* act_mask, void* stream);

/* ======================================================================================
 * Pointwise / pooling
 * ====================================================================================== */
int se3ds_act_bwd(const void* dy, const void* y, int dtype, int64_t n, int act, float alpha,
                  void* dx, void* stream);
int se3ds_add(const void* a, const void* b, int dtype, int64_t n, void* out, void* stream);
/* out[r,:] = x[r,:] * scale[r] (partial-conv backward: dy * ratio * update_mask). */
int se3ds_row_scale(const void* x, int dtype, int64_t rows, int c, const float* scale, void* out,
                    void* stream);
/* Keras MaxPool2D(2, padding='SAME') -- image_models.py:267,289 */
int se3ds_maxpool2x2_fwd(const void* x, int dtype, int n, int h, int w, int c, void* y,
                         void* stream);
int se3ds_maxpool2x2_bwd(const void* dy, const void* x, const void* y, int dtype, int n, int h,
                         int w, int c, void* dx, void* stream);
/* tf.nn.avg_pool(ksize=3, strides=2, 'SAME') -- image_models.py:617 */
int se3ds_avgpool3s2_fwd(const void* x, int dtype, int n, int h, int w, int c, void* y,
                         void* stream);
int se3ds_avgpool3s2_bwd(const void* dy, int dtype, int n, int h, int w, int c, void* dx,
                         void* stream);
/* Keras UpSampling2D() nearest x2 -- image_models.py:371,378 */
int se3ds_upsample2x_fwd(const void* x, int dtype, int n, int h, int w, int c, void* y,
                         void* stream);
int se3ds_upsample2x_bwd(const void* dy, int dtype, int n, int h, int w, int c, void* dx,
                         void* stream);
/* dst[r, dst_c0 + i] = convert(src[r, src_c0 + i]), i < ncopy: tf.concat / tf.split along
 * channels with dtype conversion (image_models.py:157-162, se3ds_trainer.py:181-192). */
int se3ds_copy_channels(const void* src, int src_dtype, int src_c, int src_c0, void* dst,
                        int dst_dtype, int dst_c, int dst_c0, int ncopy, int64_t rows,
                        void* stream);
int se3ds_fill(void* p, int dtype, int64_t n, float value, void* stream);
/* SE3DSModel quantisation glue -- models/models.py:198 (int / 255 -> fp32), :289-291
 * (proj_rgb / 255 clipped to [0,1]), :325-331 (int32(g * 255) clipped to [-1,255];
 * int32(clip(g,0,1) * 255)), :353,:359 (casts to uint8): out = Q(clamp?(in) * mul / div) with one
 * rounding per op; float outputs are clamped to [lo,hi] as tf.clip_by_value does (NaN
 * propagates), integer outputs truncate toward zero (tf.cast) and are then clamped to [lo,hi];
 * lo > hi selects the pure cast (no clamp; int32 -> uint8 wraps modulo 256 like tf.cast).
 * dtypes: SE3DS_F32 / SE3DS_I32 / SE3DS_U8. */
int se3ds_quantize(const void* in, int in_dtype, int64_t n, int pre_clamp, float pre_lo,
                   float pre_hi, float mul, float div, float lo, float hi, void* out, int out_dtype,
                   void* stream);
/* PadLayer as a standalone op -- models/layers.py:22-97: pad H and W by `pad`; mode 0
 * CONSTANT(value) / 1 REFLECT / 2 SYMMETRIC; wrap_w != 0: W is padded circularly. */
int se3ds_pad2d(const void* x, int dtype, int n, int h, int w, int c, int pad, int mode, int wrap_w,
                float value, void* y, void* stream);
/* heads -- image_models.py:187-190. kind 0: (tanh(x)+1)/2, kind 1: clip(x,0,1); y is fp32. */
int se3ds_head_fwd(const void* x, int dtype, int64_t n, int kind, float* y, void* stream);
int se3ds_head_bwd(const float* dy, const float* y, const void* x, int dtype, int64_t n, int kind,
                   void* dx, void* stream);

/* ======================================================================================
 * Losses -- trainers/se3ds_trainer.py:39-71,148-234 (fp32)
 * ====================================================================================== */
/* out[n] = per-sample sum; mode 0: sum(a); 1: sum(|a-b|*m[p]); 2: count(0<a<1);
 * 3: sum(a*(1-b)); 4: sum((a-b)^2 * 1[0<b<1]) (depth RMSE numerator, utils/eval_metric.py:225-231).
 * a,b: (n,p,c); m: (n,p). */
int se3ds_sample_sum(const float* a, const float* b, const float* m, int n, int64_t p, int c,
                     int mode, float* out, float* workspace /* n*256 floats */, void* stream);
/* grad = coef[n]*sign(a-b)*w; mode 0: w = 1[0<b<1] (depth L1); mode 1: w = m*(1-m2) (wc). */
int se3ds_l1_grad(const float* a, const float* b, const float* m, const float* m2,
                  const float* coef, int n, int64_t p, int c, int mode, float* grad, void* stream);
/* out[i] = scale / max(sums[i], 1): per-sample loss normalisers (se3ds_trainer.py:151-152). */
int se3ds_recip_clamp(const float* sums, int n, float scale, float* out, void* stream);
/* logits (2*half) [fake | real]: sums[0] = sum(-fake), sums[1] = sum(relu(1-real)+relu(1+fake));
 * dlog_d = cd * d(sums[1])/dlogits, dlog_g = cg * d(sums[0])/dlogits (either may be NULL). */
int se3ds_hinge(const void* logits, int dtype, int64_t half, float cd, float cg, float* sums,
                void* dlog_d, void* dlog_g, void* stream);

/* ======================================================================================
 * Optimiser step over flat fp32 arenas -- se3ds_trainer.py:27-32,238-257;
 * gan_manager.py:175-183; utils/ema.py:54-64
 * ====================================================================================== */
/* chunks: int64 triples (tensor id, start, length<=65536) covering the arena;
 * tensor_chunk_start: (ntensors+1) prefix into chunks.  sqnorm[t] = sum g^2 of tensor t. */
int se3ds_multi_sqnorm(const float* grads, const int64_t* chunks, int64_t nchunks,
                       const int64_t* tensor_chunk_start, int ntensors, float* partial,
                       float* sqnorm, void* stream);
/* tf.clip_by_norm per tensor, in place: g = (g*clip)/max(||g||, clip); mean_norm_out (device
 * scalar, may be NULL) = mean over tensors of the clipped norms (NaN -> 0). */
int se3ds_multi_clip_by_norm(float* grads, const int64_t* chunks, int64_t nchunks,
                             const float* sqnorm, int ntensors, float clip_norm,
                             float* mean_norm_out, void* stream);
/* out[0] = mean over tensors of min-clipped norms (the grad_norm metrics, se3ds_trainer.py:239). */
int se3ds_mean_clipped_norm(const float* sqnorm, int ntensors, float clip_norm, float* out,
                            void* stream);
/* Keras Adam (ResourceApplyAdam), `step` = iteration count t >= 1. */
int se3ds_multi_adam_keras(float* params, const float* grads, float* m, float* v, int64_t n,
                           float lr, float beta1, float beta2, float eps, int64_t step,
                           void* stream);
/* The same, and the EMA copy of the parameters advanced in the same pass (ema may be NULL):
 * ema -= (ema - params_new) * one_minus_decay  (utils/ema.py:54-88 applied to the trainable
 * variables right where they are produced). */
int se3ds_multi_adam_keras_ema(float* params, const float* grads, float* m, float* v, int64_t n,
                               float lr, float beta1, float beta2, float eps, int64_t step,
                               float* ema, float one_minus_decay, void* stream);
/* One replica: se3ds_multi_clip_by_norm_sn + se3ds_multi_adam_keras_ema in ONE pass over the chunk
 * rows [tensor id, first element, length] -- the clipped (and, for spectral kernels, fixed-up)
 * gradient is formed in registers and consumed by the Adam (+ EMA) update; the gradient arena is
 * read once and NOT rewritten (trainers/se3ds_trainer.py:27-32,238-257 with a single replica:
 * clip_by_norm feeds apply_gradients directly).  Bit-identical to the two separate passes.
 * sqnorm from se3ds_multi_sqnorm_sn; chunk rows carry absolute tensor ids and arena offsets; all
 * arenas 16-byte aligned (SE3DS_E_UNSUPPORTED otherwise).  ema may be NULL. */
int se3ds_multi_clip_adam_keras_ema(float* params, const float* grads, float* m, float* v,
                                    const int64_t* chunks, int64_t nchunks, const float* sqnorm,
                                    float clip_norm, const int64_t* tensor_sn, float lr, float beta1,
                                    float beta2, float eps, int64_t step, float* ema,
                                    float one_minus_decay, void* stream);
/* ema -= (ema - vars) * one_minus_decay */
int se3ds_multi_ema(float* ema, const float* vars, int64_t n, float one_minus_decay, void* stream);

/* Spectral normalisation, batched over layers -- models/layers.py:312-331.  `table` is a
 * device array of se3ds_spectral_table_fields() int64 per layer:
 *   W, u, v (K), uhat (cout), sig (2: sigma, 1/(sigma+1e-10)), part (part_rows*cout),
 *   vpart (vpart_len), K, cout, grad
 * power_iter: v_hat, u_hat, sigma from (W,u); u := u_hat when training != 0.
 * bwd_fixup: grad := grad/(sigma+eps) - <grad,W>/(sigma+eps)^2 * v_hat^T u_hat. */
int se3ds_spectral_table_fields(void);
int se3ds_spectral_part_rows(void);
int se3ds_spectral_vpart_len(void);
int se3ds_spectral_power_iter(const int64_t* table, int nlayers, int training, void* stream);
int se3ds_spectral_bwd_fixup(const int64_t* table, int nlayers, void* stream);
/* The fix-up folded into the clip pass (one read-modify-write of the gradient arena instead of
 * two, no separate norm pass over the spectral kernels):
 *   se3ds_spectral_bwd_dots       pass 1 only: <grad,W>, <grad,grad>, <grad, v_hat^T u_hat> into vpart
 *   se3ds_multi_sqnorm_sn         as se3ds_multi_sqnorm; tensors t with tensor_sn[t] != 0 (address of
 *                                 their table row) get |fixed grad|^2 in closed form from vpart
 *   se3ds_multi_clip_by_norm_sn   as se3ds_multi_clip_by_norm; those tensors are fixed up and
 *                                 clipped in the same pass
 * tensor_sn: int64[number of tensors], absolute tensor ids as in the chunk rows; tensor_base: id of
 * the first tensor of tensor_chunk_start / sqnorm (per-segment calls).  Reference semantics:
 * models/layers.py:299-347 (gradient through sigma), trainers/se3ds_trainer.py:27-32 (clip). */
int se3ds_spectral_bwd_dots(const int64_t* table, int nlayers, void* stream);
int se3ds_multi_sqnorm_sn(const float* grads, const int64_t* chunks, int64_t nchunks,
                          const int64_t* tensor_chunk_start, int ntensors, float* partial,
                          float* sqnorm, const int64_t* tensor_sn, int tensor_base, void* stream);
int se3ds_multi_clip_by_norm_sn(float* grads, const int64_t* chunks, int64_t nchunks,
                                const float* sqnorm, int ntensors, float clip_norm,
                                float* mean_norm_out, const int64_t* tensor_sn, void* stream);

/* ======================================================================================
 * Input pipeline, device-side half
 * ====================================================================================== */

/* datasets/indoor_datasets.py:263-375 (_transform_fn) + :553-597 (_train_batch_transform_fn) on
 * decoded frames resident in HBM: convert_image_dtype (:185-228), band masking of proj_mask
 * (:281-304), bilinear (image) / nearest (everything else) resize to (rh, rw) (:312-314), roll by
 * `roll` and optional flip along W (:34-61), crop at (crop_y, crop_x) to (h, w) (:326-330),
 * proj_image *= proj_mask and proj_depth *= proj_mask (:577-585).  Raw frames are (N,H0,W0[,3]);
 * iparams [N][8] = rh, rw, roll, flip, crop_y, crop_x, hmode (0 none / 1 start<x<end / 2 x>start
 * or x<end), vmode (0 / 1); fparams [N][4] = hstart, hend, vstart, vend (raw-grid pixels).
 * Outputs are the step's batch dict entries, fp32 (N,h,w,C) and int32 segmentation. */
int se3ds_input_transform(const uint8_t* image, const uint8_t* proj_image, const uint16_t* depth,
                          const uint16_t* proj_depth, const uint8_t* proj_mask,
                          const uint8_t* blurred_mask, const uint8_t* segmentation,
                          const int32_t* iparams, const float* fparams, int n, int h0, int w0, int h,
                          int w, float* o_image, float* o_proj_image, float* o_proj_mask,
                          float* o_proj_depth, float* o_depth, float* o_blurred, int32_t* o_seg,
                          void* stream);

/* datasets/indoor_datasets.py:734-792 (R2RVideoDataset._transform_fn) over the N*T frames of a
 * batch resident in HBM, one gather: image fp32 (N,T,H0,W0,3) -> o_original fp32 (N,T,h,w,3) by
 * tf.image.resize bilinear (half-pixel centres, no antialias, NO clip; identity size copies);
 * o_image = o_original * band mask on the OUTPUT grid (:753-765), hmode [N] = 0 none / 1
 * start < x < end / 2 x > start or x < end, hband [N][2] = start, end, one row per example shared
 * by its T frames; o_image NULL: no masked copy is written (hmode / hband may then be NULL).
 * segmentation / pd_segmentation uint8 (N,T,H0,W0) and depth / pd_depth fp32 (N,T,H0,W0) ->
 * (N,T,h,w,1) by nearest.  pd_segmentation with o_pd_seg, and pd_depth with o_pd_depth, may be
 * NULL together.  se3ds_resize's arithmetic: bit-identical to that chain run op by op. */
int se3ds_video_transform(const float* image, const uint8_t* segmentation,
                          const uint8_t* pd_segmentation, const float* depth, const float* pd_depth,
                          const int32_t* hmode, const float* hband, int n, int t, int h0, int w0,
                          int h, int w, float* o_original, float* o_image, uint8_t* o_seg,
                          uint8_t* o_pd_seg, float* o_depth, float* o_pd_depth, void* stream);

/* datasets/indoor_datasets.py:420-450, the reduction in front of the RE10K crop: per example the
 * first and last row and the first and last column of visible_mask uint8 (N,H0,W0) that hold a
 * nonzero pixel, into extents int32 [N][4] = r0, r1, c0, c1 by integer atomic min / max
 * (deterministic).  The CALLER initialises extents to H0, -1, W0, -1 (any r0 > r1 reads as "no
 * visible pixel"); it does so in the upload that carries the draw rows, so there is no memset.
 * 16 bytes a lane when W0 and the plane's address are multiples of 16, a byte a lane otherwise;
 * se3ds_re10k_extent_vector_bytes (host only) tells which. */
int se3ds_re10k_extent(const uint8_t* visible_mask, int n, int h0, int w0, int32_t* extents,
                       void* stream);
int se3ds_re10k_extent_vector_bytes(const uint8_t* visible_mask, int w0);

/* datasets/indoor_datasets.py:377-535 (_transform_fn_re10k) + :553-597 on decoded frames resident
 * in HBM, one gather: convert_image_dtype (:185-228), blurred = 1 - (visible_mask > 0) (:238), band
 * masking of proj_mask on the raw grid (:389-412), the crop box from `extents` and the draws
 * (:445-472, csrc/re10k_box_core.h), crop, bilinear + clip (image) / nearest (everything else,
 * proj_image included) resize of the CROP to (h, w) (:486-491), proj_image *= proj_mask and
 * proj_depth *= proj_mask (:577-585).  iparams [N][3] = hmode (0 none / 1 start<x<end / 2 x>start
 * or x<end), vmode (0 / 1), crop flag; fparams [N][7] = hstart, hend, vstart, vend (raw-grid
 * pixels), pad, x_shift, y_shift.  An example whose crop flag is 0 takes the whole frame as its
 * box: with (h, w) = (h0, w0) that is conversion, band masks and batch transform only (:474).
 * o_bbox int32 [N][4] = x_min, y_min, x_max, y_max (:520); o_status int32 [N] = 0 ok / 1 no
 * visible pixel / 2 the box does not lie inside the frame; such an example's outputs are zeros.
 * No status and no draw makes the kernel read outside a plane.  extents and o_bbox may be NULL
 * together: no example is cropped, the flags are ignored.  Any other NULL is BADSHAPE. */
int se3ds_re10k_transform(const uint8_t* image, const uint8_t* proj_image, const uint16_t* depth,
                          const uint16_t* proj_depth, const uint8_t* proj_mask,
                          const uint8_t* visible_mask, const uint8_t* segmentation,
                          const int32_t* extents, const int32_t* iparams, const float* fparams,
                          int n, int h0, int w0, int h, int w, float* o_image, float* o_proj_image,
                          float* o_proj_mask, float* o_proj_depth, float* o_depth, float* o_blurred,
                          int32_t* o_seg, int32_t* o_bbox, int32_t* o_status, void* stream);

/* PNG reconstruction (un-filtering) of a whole batch in one launch -- the second half of
 * tf.image.decode_png (datasets/indoor_datasets.py:185-228); the host or se3ds_png_inflate
 * inflates.  csrc/png.hip.
 * src: the inflated streams of all images, one device buffer of src_bytes bytes; a stream is
 * height x (1 filter-type byte + row_bytes filtered bytes).  table: device int64
 * [n][se3ds_png_unfilter_fields() = 6] = source byte offset into src, destination device pointer
 * (height x row_bytes bytes, dense), height, row_bytes, bytes per pixel (1, 2 or 3), 16-bit flag
 * (0 / 1; with 2 bytes per pixel only: the two bytes of a sample are stored swapped, big-endian ->
 * little-endian).  Images of different geometry and bytes per pixel share the launch, one wavefront
 * each.  host_table: the HOST copy the device table was made from; it is validated here before
 * anything runs (BADSHAPE: n < 1 or > 65535, a null destination, height < 1, row_bytes not a
 * multiple of the bytes per pixel, a stream that leaves src; UNSUPPORTED: row_bytes above
 * se3ds_png_unfilter_max_row_bytes()), the kernel reads only the device copy.  Filter types above 4
 * are the caller's to reject (utils/png.py does); the kernel treats them as None.  Exact integer
 * arithmetic, deterministic. */
int se3ds_png_unfilter(const uint8_t* src, int64_t src_bytes, const int64_t* table,
                       const int64_t* host_table, int n, void* stream);
int se3ds_png_unfilter_fields(void);
int se3ds_png_unfilter_max_row_bytes(void);

/* zlib inflate (RFC 1950 / 1951) of the IDAT streams of a whole batch in one launch, in front of
 * se3ds_png_unfilter on the same stream -- the first half of tf.image.decode_png, for callers that
 * do not inflate on the host.  csrc/inflate.hip, decoder in csrc/inflate_core.h.
 * buf: one device buffer of buf_bytes bytes, 8-byte aligned, that BEGINS with the device copy of
 * the table and holds the compressed streams behind it.  table: int64
 * [n][se3ds_png_inflate_fields() = 5] = byte offset of the compressed stream in buf (not inside the
 * table), its length, byte offset of the stream's region in workspace, expected inflated length
 * (height x pitch), scan-line pitch (1 filter-type byte + row_bytes).  workspace: device buffer of
 * workspace_bytes bytes; a stream's region receives the inflated, still filtered scan lines, laid
 * out as se3ds_png_unfilter reads them (regions 16-byte aligned are written 16 bytes per lane, others
 * bytewise; regions must not overlap).  One wavefront per stream; the 32 KiB window is an LDS ring
 * of se3ds_png_inflate_ring_bytes() bytes.
 * status_dev: device int32 [n], written by the launch: 0 = the stream inflated to exactly the
 * expected length, its Adler-32 matched and every scan line starts with a filter type <= 4;
 * otherwise the code of `enum class Status` (csrc/inflate_core.h) in the low 8 bits -- for
 * BAD_FILTER with the filter-type byte in bits 8-15 and its row (saturating at 32767) in bits
 * 16-30 -- and the region is zero from the end of the last 16 KiB granule written before the
 * failure (for a failure in the trailer: from the last inflated byte) on.  The kernel reads the compressed bytes only inside [offset, offset + length) and writes only inside
 * the region, whatever the stream says.
 * host_table: the HOST copy of the table, validated here before anything runs (BADSHAPE: n < 1 or
 * > 65535, a null or misaligned pointer, a range that leaves its buffer or enters the table, a
 * length above 2^31 - 1, a pitch < 2, an expected length that is no multiple of the pitch).
 * Deterministic. */
int se3ds_png_inflate(const uint8_t* buf, int64_t buf_bytes, uint8_t* workspace,
                      int64_t workspace_bytes, const int64_t* host_table, int n,
                      int32_t* status_dev, void* stream);
int se3ds_png_inflate_fields(void);
int se3ds_png_inflate_ring_bytes(void);

/* Baseline JPEG decode (ITU-T T.81: SOF0 / SOF1, 8 bit, Huffman, one interleaved scan) of a whole
 * batch -- tf.image.decode_jpeg with its defaults (accurate integer DCT, fancy upscaling).
 * csrc/jpeg.hip, decoder in csrc/jpeg_core.h.  The container is parsed by the caller
 * (utils/jpeg.py); this call gets tables.
 * buf: one device buffer of buf_bytes bytes, 8-byte aligned, that BEGINS with the device copy of the
 * image table, then the segment table, and holds the entropy-coded bytes behind them.
 * image table: int64 [n_images][se3ds_jpeg_decode_fields() = 200], `struct Image` of jpeg_core.h:
 * width, height, components (1 or 3), horizontal and vertical sampling of component 0 (1 x 1, 2 x 1
 * or 2 x 2; the others are 1 x 1; grey is 1 x 1), destination device pointer (height x width x
 * channels uint8, dense), output channels (1 = the Y plane, 3 = RGB, a grey file replicated), byte
 * offsets of the image's coefficients and of its component planes in workspace (16-byte aligned),
 * first segment and segment count, MCUs per row and MCU rows, table selectors (bit c: DC table of
 * component c, bit 4 + c: its AC table), two reserved words; then per component the 64
 * quantisation values as uint16 in row-major order; then four Huffman tables (DC 0, DC 1, AC 0,
 * AC 1) of 16 counts + 256 values each.
 * segment table: int64 [n_segments][se3ds_jpeg_decode_segment_fields() = 5] = image, byte offset of
 * the segment's entropy bytes in buf (not inside the tables; the RSTn marker is not part of it),
 * their count, first MCU, MCU count.  A segment is a restart interval or the whole scan; the
 * segments of an image are consecutive rows and cover its MCUs in order.
 * workspace: device buffer, 16-byte aligned; se3ds_jpeg_decode_workspace_bytes(host_images, n) is
 * the sum over the images of 128 bytes per block and of the planes padded to whole MCUs, each
 * rounded up to 16.  Layout: the coefficients of all images, ascending and disjoint, then the planes
 * of all images, likewise.
 * phases: bit mask, 1 = entropy decode (the coefficients are zeroed first, then one workgroup of
 * se3ds_jpeg_decode_lanes() threads per segment decodes it speculatively in windows of lanes x
 * se3ds_jpeg_decode_chunk_bytes() bytes), 2 = dequantise + inverse DCT into the planes, 4 =
 * upsample + colour + crop into the destinations.  Callers pass 7; a tool may time the parts.
 * status_dev: device int32 [n_segments], written by phase 1: `enum class Status` of jpeg_core.h in
 * the low 8 bits (0 = the segment held exactly its blocks), the rounds of all its windows in bits
 * 8-30 (saturating).  Whatever the bytes say, the kernels read only inside the ranges given and
 * write only inside the image's regions and destination.
 * host_images, host_segments: the HOST copies, validated here before anything runs (BADSHAPE: a
 * count < 1, n_images > 65535, a null or misaligned pointer, a range that leaves its buffer or
 * enters the tables, regions out of order, sizes outside 1..65535, sampling or channels not listed
 * above, MCU or segment counts that do not add up, Huffman counts that no prefix code has;
 * WORKSPACE: workspace_bytes below the size above).  Integer arithmetic, no atomics, no host
 * synchronisation: deterministic. */
int se3ds_jpeg_decode(const uint8_t* buf, int64_t buf_bytes, uint8_t* workspace,
                      int64_t workspace_bytes, const int64_t* host_images, int n_images,
                      const int64_t* host_segments, int n_segments, int32_t* status_dev, int phases,
                      void* stream);
size_t se3ds_jpeg_decode_workspace_bytes(const int64_t* host_images, int n_images);
int se3ds_jpeg_decode_fields(void);
int se3ds_jpeg_decode_segment_fields(void);
int se3ds_jpeg_decode_lanes(void);
int se3ds_jpeg_decode_chunk_bytes(void);

/* One uint8 image sheet from a batch of float images -- utils/image_grid.py:24-51 (get_grid_image:
 * tf.cast(x * 255.0, tf.uint8), then images_to_grid).  csrc/png_encode.hip.
 * src: (n, h, w, c) F32 / BF16, c 1 or 3.  out: uint8 (ny * h, nx * w, out_c), out_c 1 or 3; tile i
 * = image i goes to sheet row i / nx, column i % nx, ny * nx <= n; a 1-channel source is replicated
 * into 3 output channels (the reference tiles depth and masks, trainers/gan_manager.py:560-567).
 * Value: x * 255.0f in fp32 (a bf16 source is widened first), truncated toward zero, saturated to
 * [0, 255], NaN -> 0.  This is NOT convert_image_dtype's x * 255.5 (se3ds_quantize expresses that).
 * BADSHAPE: sizes < 1, c or out_c outside {1, 3}, c 3 with out_c 1, ny * nx > n. */
int se3ds_grid_quantize(const void* src, int dtype, int n, int h, int w, int c, int ny, int nx,
                        int out_c, uint8_t* out, void* stream);

/* PNG filtering + zlib deflate of many uint8 images in two launches -- what a TensorBoard image
 * summary (utils/logger.py:66-71) and the roll-out PNGs (trainers/gan_manager.py:274-296) need
 * between the pixels and the file.  csrc/png_encode.hip, encoder in csrc/deflate_core.h.
 * table: device int64 [n][se3ds_png_encode_fields() = 8] = device pointer of the image (height x
 * row_bytes bytes, dense), height, row_bytes, bytes per pixel (1 or 3), filter (0..4: that PNG
 * filter type on every row; 5: adaptive, per row the type with the smallest sum of
 * |int8(residual)|, ties to the lowest type), index of the image's first strip, byte offset of the
 * image's stream in out, byte offset of the image's first slot behind the workspace's strip records.
 * An image is cut into strips of max(1, 65535 / (1 + row_bytes)) rows, one wavefront each; with S
 * strips it takes S slots of (10 + min(rows per strip, height) x (1 + row_bytes)) bytes rounded up to 8, and
 * 10 S + height x (1 + row_bytes) bytes of out.  The last three fields are running sums of these
 * over the rows in front, starting at 0.  Mixed geometries share the launch.
 * A strip becomes one dynamic-Huffman block over literals and distance-1 runs (length 3..258,
 * greedy; code lengths limited to 15 bits; the code-length code is fixed: 0..15 at 4 bits; one
 * distance code) or, when that would not be smaller, one stored block; an empty stored block ends
 * it on a byte boundary, with BFINAL on the image's last strip.  No strip exceeds 10 bytes + its
 * filtered bytes.  The second launch packs the strips of every image densely at its offset in out
 * and writes sizes_dev: uint32 [n][2] = bytes of the image's deflate stream, Adler-32 of its
 * filtered bytes.  The caller frames it: 78 01 + stream + Adler-32 big-endian.  Bytes of out past
 * an image's size are not written.
 * workspace: device, 16-byte aligned, at least se3ds_png_encode_workspace_bytes(host_table, n)
 * bytes (0: the table is not valid); out: at least se3ds_png_encode_out_bytes(host_table, n).
 * host_table: the HOST copy of the table, validated here before anything runs (BADSHAPE: n < 1 or
 * > 65535, a null pointer, height < 1, row_bytes not a multiple of the bytes per pixel, a filter
 * above 5, running sums that are not the ones above, an out buffer that is too small; UNSUPPORTED:
 * row_bytes above se3ds_png_encode_max_row_bytes(); WORKSPACE: a workspace that is too small).
 * phases: 3 = both launches, what callers pass; 1 = the strips only, 2 = the packing only, on a
 * workspace that phase 1 filled for the same table (tools/png_encode_bench.py times them apart).
 * Both launches on `stream`, no host synchronisation, no atomics, integer arithmetic: the output
 * is the same bytes on every run. */
int se3ds_png_encode(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                     int64_t workspace_bytes, uint8_t* out, int64_t out_bytes, uint32_t* sizes_dev,
                     int phases, void* stream);
size_t se3ds_png_encode_workspace_bytes(const int64_t* host_table, int n);
int64_t se3ds_png_encode_out_bytes(const int64_t* host_table, int n);
int se3ds_png_encode_fields(void);
int se3ds_png_encode_max_row_bytes(void);
/* HOST arithmetic, no device work: the Adler-32 of a concatenation from the Adler-32 `a` of its
 * first part and `b` of its len_b further bytes -- how the second launch folds the strips' sums
 * (csrc/deflate_core.h adler_combine). */
uint32_t se3ds_adler32_combine(uint32_t a, uint32_t b, int64_t len_b);
/* se3ds_png_encode for the planes of a training record (datasets/record_writer.py), two of which --
 * image/depth and proj/depth, datasets/indoor_datasets.py:193-204 -- are 16-bit grey.  Signature,
 * table, strips, slots, the packing launch, sizes and Adler-32 are those of se3ds_png_encode, with
 * one more value of field 3: 2 = one 16-bit sample per pixel, lying in host (little-endian) order in
 * memory, row_bytes = 2 x width.  What is filtered and deflated is the big-endian byte sequence PNG
 * stores (ISO/IEC 15948 7.1): file byte x of a row is memory byte x ^ 1, 2 bytes per pixel.  8-bit and
 * 16-bit planes share the launch.  BADSHAPE etc. as se3ds_png_encode (a field 3 outside {1, 2, 3});
 * the two size functions take this entry's tables. */
int se3ds_png_encode_planes(const int64_t* table, const int64_t* host_table, int n,
                            uint8_t* workspace, int64_t workspace_bytes, uint8_t* out,
                            int64_t out_bytes, uint32_t* sizes_dev, int phases, void* stream);
size_t se3ds_png_encode_planes_workspace_bytes(const int64_t* host_table, int n);
int64_t se3ds_png_encode_planes_out_bytes(const int64_t* host_table, int n);

/* Baseline JPEG encoding of many uint8 images: the entropy-coded data of the files libjpeg's default
 * encoder writes (Pillow's Image.save(f, 'JPEG', quality=q, subsampling=s)), byte for byte:
 * 16-bit colour conversion, box downsampling, slow-integer forward DCT, rounded-division
 * quantisation, the Annex K Huffman tables, restart intervals.  csrc/jpeg_encode.hip, arithmetic
 * in csrc/jpeg_encode_core.h.  The caller adds the container (utils/jpeg.py jpeg_container).
 * table: device int64 [n][se3ds_jpeg_encode_fields() = 48], `struct Image` of jpeg_encode_core.h:
 * device pointer of the pixels (height x width x components uint8, dense), width, height,
 * components (1: a grey file; 3: RGB -> YCbCr), luma sampling h, v (1x1, 2x1 or 2x2; grey 1x1;
 * chroma is 1x1), restart interval in MCUs (0: none), blocks of the images in front (a running
 * sum from 0; an image has mcus_x * mcus_y * (1 or h * v + 2) blocks), transform tiles of the
 * images in front (a running sum from 0; a tile is up to se3ds_jpeg_encode_tile_blocks() / blocks
 * per MCU consecutive MCUs of one MCU row, so an image has mcus_y * ceil(mcus_x / that) tiles), 7
 * reserved, then the luma
 * and the chroma quantisation table, uint16 [2][64] in row-major order, every entry 1..255.
 * out: the images' entropy-coded bytes (stuffed, RSTn markers between the segments, every
 * segment's last byte padded with 1 bits), one image behind the other without gaps; sizes_dev:
 * int64 [n + 1], image i's bytes are out[sizes_dev[i] .. sizes_dev[i + 1]).
 * workspace: device, 16-byte aligned, at least se3ds_jpeg_encode_workspace_bytes(host_table, n)
 * bytes (0: the table is not valid); out: at least se3ds_jpeg_encode_out_bytes(host_table, n), a
 * worst-case bound (every block 1660 bits, every byte stuffed).
 * host_table: the HOST copy of the table, validated before anything runs (BADSHAPE: n < 1 or >
 * 65535, a null pointer, a size < 1, components outside {1, 3}, a restart interval outside
 * 0..65535, a quantiser outside 1..255, a running sum that is not the one above, an out buffer
 * that is too small; UNSUPPORTED: a size above 65535, any other sampling; WORKSPACE: a workspace
 * that is too small).
 * phases: 15 = everything, what callers pass; 1 = the transform (pixels -> quantised coefficients),
 * 2 = measure (every block's Huffman bits, kept, and the scan that places them; groups of
 * se3ds_jpeg_encode_scan_group_blocks() blocks), 4 = pack, count (units of
 * se3ds_jpeg_encode_pack_unit_blocks() blocks: assemble, count the stuffing, scan), 8 = pack, write
 * (assemble again, stuff, store); a later phase needs the workspace the earlier ones filled for the
 * same table (tools/jpeg_encode_bench.py times
 * them apart).  Six launches on `stream`, no host synchronisation, no global atomics, integer
 * arithmetic: the output is the same bytes on every run. */
int se3ds_jpeg_encode(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                      int64_t workspace_bytes, uint8_t* out, int64_t out_bytes, int64_t* sizes_dev,
                      int phases, void* stream);
size_t se3ds_jpeg_encode_workspace_bytes(const int64_t* host_table, int n);
int64_t se3ds_jpeg_encode_out_bytes(const int64_t* host_table, int n);
int se3ds_jpeg_encode_fields(void);
int se3ds_jpeg_encode_scan_group_blocks(void);
int se3ds_jpeg_encode_pack_unit_blocks(void);
int se3ds_jpeg_encode_block_words(void);
int se3ds_jpeg_encode_tile_blocks(void);

/* Animated GIF encoding of many uint8 videos (frames x height x width x 1|3, dense): one global
 * palette of 256 entries per video, ordered dither, LZW in independent strips packed at bit
 * granularity.  The format is DESIGN.md 3.18; csrc/gif.hip, the LZW walk in csrc/gif_lzw_core.h.
 * The caller runs the median cut between histogram and lut, and adds the container (utils/gif.py).
 * table: device int64 [n][se3ds_gif_fields() = 12]: device pointer of the pixels, frames, height,
 * width, channels (1: the pixel is the index; 3: RGB), dither amplitude 0..255, and six fields that
 * se3ds_gif_plan(host_table, n) fills in the HOST copy before it is uploaded: frames and strips of
 * the videos in front, the byte offsets of the video's index plane, strip slots and output area,
 * and the bytes of one frame's output area (its sub-blocks at their longest, rounded up to 16).
 * host_table: the HOST copy, validated before anything runs (BADSHAPE: n < 1 or > 65535, a null
 * pointer, frames < 1, a size outside 1..65535, channels outside {1, 3}, dither outside 0..255, a
 * derived field that is not what se3ds_gif_plan writes, an out buffer that is too small or
 * misaligned; UNSUPPORTED: more than 2^31 - 1 frames or strips; WORKSPACE: a workspace that is too
 * small).  workspace: device, 16-byte aligned, se3ds_gif_workspace_bytes(host_table, n) bytes (0:
 * the table is not valid); its regions begin at se3ds_gif_workspace_offset(host_table, n, region):
 * 0 = histograms uint32 [n][32768], 1 = look-up tables uint8 [n][32768], 2 = index planes, 3 =
 * strip slots, 4 = strip bit counts uint32, 5 = strip bit positions uint64, 6 = the end.
 * A strip is ceil(se3ds_gif_strip_pixels() / width) whole rows of a frame; its slot has
 * se3ds_gif_strip_slot_bytes(pixels of a full strip) bytes.
 * Stages, each one call on `stream` without a host synchronisation, each reading what the one before
 * left in the workspace:
 *   histogram  colour videos: bin = (r>>3)<<10 | (g>>3)<<5 | (b>>3) over every pixel, exact in 32 bits.
 *   lut        palettes: device uint8 [n][256][3]; used: device int32 [n], the entries in use, 0 = a
 *              grey video.  The used entry nearest every bin centre, lowest index on a tie.
 *   index      dither, clamp, look-up: one byte per pixel of every colour video.
 *   lzw        one wave per strip -> the strip's code stream in its slot, and its bit count.
 *   pack       out: device, 8-byte aligned, se3ds_gif_out_bytes(host_table, n) bytes: int64 [frames]
 *              (rounded up to 16 bytes) with every frame's byte count, then per frame, at the video's
 *              output offset + frame * its frame bytes, the sub-blocks and the terminator.
 * Integer arithmetic throughout: the same bytes on every run. */
int se3ds_gif_plan(int64_t* host_table, int n);
size_t se3ds_gif_workspace_bytes(const int64_t* host_table, int n);
int64_t se3ds_gif_out_bytes(const int64_t* host_table, int n);
int64_t se3ds_gif_workspace_offset(const int64_t* host_table, int n, int region);
int se3ds_gif_fields(void);
int se3ds_gif_strip_pixels(void);
int64_t se3ds_gif_strip_slot_bytes(int64_t pixels);
int se3ds_gif_histogram(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                        int64_t workspace_bytes, void* stream);
int se3ds_gif_lut(const int64_t* table, const int64_t* host_table, int n, const uint8_t* palettes,
                  const int32_t* used, uint8_t* workspace, int64_t workspace_bytes, void* stream);
int se3ds_gif_index(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                    int64_t workspace_bytes, void* stream);
int se3ds_gif_lzw(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                  int64_t workspace_bytes, void* stream);
int se3ds_gif_pack(const int64_t* table, const int64_t* host_table, int n, uint8_t* workspace,
                   int64_t workspace_bytes, uint8_t* out, int64_t out_bytes, void* stream);

/* ======================================================================================
 * Writing training records -- the inverse of datasets/indoor_datasets.py:125-247.
 * csrc/records.hip, datasets/record_writer.py.
 * ====================================================================================== */

/* The warp's fp32 results (models/models.py:273-293) -> the planes a record stores, one elementwise
 * pass over `pixels` pixels.  Three independent pairs; a pair is skipped when both its pointers
 * are null, and at least one must be given.
 * proj_rgb: (pixels, 3) F32, void class -1 -> rgb_out uint8: truncated toward zero, saturated to
 * [0, 255]; the void class, negatives and NaN are 0.
 * proj_depth: (pixels) F32 in [0, 1] -> depth_out uint16 = floor((double)d * 65535 + 0.5) saturated
 * to [0, 65535], NaN -> 0: the inverse of the decoder's u16 / 65535 for all 65 536 codes.  Also for
 * a float target depth (image/depth).
 * proj_mask: (pixels) F32 -> mask_out uint8: 255 where the mask is 1, otherwise 0.
 * Where all pointers are 16-byte aligned a thread takes four pixels per load; otherwise one.
 * BADSHAPE: pixels < 1, half a pair, no pair, a float pointer off 4 bytes, depth_out off 2. */
int se3ds_record_planes(const float* proj_rgb, const float* proj_depth, const float* proj_mask,
                        int64_t pixels, uint8_t* rgb_out, uint16_t* depth_out, uint8_t* mask_out,
                        void* stream);

/* Copies n byte ranges from m source buffers to their offsets in `out` in one launch -- how a
 * record file is put together from the literals the host made (PNG signature, IHDR, IEND, the IDAT
 * framing, protobuf keys and varints, record lengths) and the encoder's compact streams.
 * sources_host: HOST int64 [m][2] = device pointer, bytes; m <= 8.  table_dev / host_table: int64
 * [n][se3ds_assemble_fields() = 4] = source index, source offset, destination offset, length.
 * Offsets and lengths need no alignment.  One workgroup per segment: the caller splits a longer
 * range into segments of at most se3ds_assemble_max_segment_bytes().  The kernel stores 16 bytes at
 * a time only at 16-byte-aligned destinations and single bytes at a segment's edges; it reads the
 * source as aligned words (shifted together) or single bytes, and never outside a segment's range.
 * Bytes of out outside the destinations are not written.
 * host_table is validated before anything runs (BADSHAPE: n < 1 or > 2^24, m outside 1..8, a null pointer, a
 * source index outside [0, m), a length outside [0, max segment], a range that leaves its source,
 * a destination that leaves [0, out_bytes) or starts before the end of the one in front:
 * destinations ascend and are disjoint).  One launch on `stream`, no atomics. */
int se3ds_assemble_segments(const int64_t* sources_host, int m, const int64_t* table_dev,
                            const int64_t* host_table, int n, uint8_t* out, int64_t out_bytes,
                            void* stream);
int se3ds_assemble_fields(void);
int64_t se3ds_assemble_max_segment_bytes(void);

/* Writes device-resident CRC words (the results of se3ds_crc32z_multi / se3ds_crc32c_multi) into
 * `out` without a round trip through the host.  table_dev / host_table: int64
 * [n][se3ds_patch_crc_fields() = 3] = index into crc_dev, byte offset in out, form.  Form 0: the raw
 * value big-endian (a PNG chunk's CRC); form 1: TFRecord's masked CRC-32C,
 * ((c >> 15 | c << 17) + 0xa282ead8) little-endian.  Offsets need no alignment.
 * BADSHAPE: n < 1 or > 2^24, a null pointer, an index outside [0, crc_count), a form outside {0, 1}, an
 * offset outside [0, out_bytes - 4] or before the end of the patch in front. */
int se3ds_patch_crc(const uint32_t* crc_dev, int crc_count, const int64_t* table_dev,
                    const int64_t* host_table, int n, uint8_t* out, int64_t out_bytes, void* stream);
int se3ds_patch_crc_fields(void);

/* CRC-32C (Castagnoli: reflected polynomial 0x82F63B78, init and final xor 0xffffffff; RFC 3720
 * B.4, utils/tf_bundle.crc32c) of n byte ranges of one device buffer in one call -- the checksum of
 * TFRecord frames and of the tensors of a checkpoint bundle.  csrc/crc32c.hip, arithmetic in
 * csrc/crc32c_core.h.
 * buf: device buffer of buf_bytes bytes, read only.  table_dev: device int64
 * [n][se3ds_crc32c_fields() = 2] = byte offset into buf, length; offsets and lengths need no
 * alignment and ranges may overlap.  crc_dev: device uint32 [n], receives the raw (unmasked) CRC of
 * every range; length 0 gives 0.  workspace: device buffer of at least
 * se3ds_crc32c_workspace_bytes(sum of the lengths, n) bytes, 8-byte aligned.
 * The work of all ranges is cut into blocks of se3ds_crc32c_block_bytes() bytes, counted from the
 * end of each range, and shared evenly among the wavefronts.  The kernels read buf only inside the
 * ranges (also where they load 4 or 16 bytes at once) and write only crc_dev and the workspace.
 * host_table: the HOST copy of the table, validated here before anything runs (BADSHAPE: n < 1, a
 * null or misaligned pointer, a negative offset or length, a range that leaves [0, buf_bytes), a
 * workspace that is too small); the kernels read only the device copy and skip a row of it that
 * leaves the buffer.  Two launches on `stream`, no host synchronisation, integer arithmetic,
 * deterministic. */
int se3ds_crc32c_multi(const uint8_t* buf, int64_t buf_bytes, const int64_t* table_dev,
                       const int64_t* host_table, int n, uint32_t* crc_dev, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t se3ds_crc32c_workspace_bytes(int64_t total_bytes, int n);
int se3ds_crc32c_fields(void);
int se3ds_crc32c_block_bytes(void);

/* The zip / zlib CRC-32 (ISO 3309: reflected polynomial 0xEDB88320, init and final xor 0xffffffff;
 * zlib.crc32) of n byte ranges of one device buffer in one call, each continued from a seed -- the
 * checksum of the members of a checkpoint archive, whose .npy headers the host has already hashed
 * (trainers/gan_manager.py save_checkpoint_async, utils/npz_writer.py).  The kernels, the schedule,
 * the bounds and the BADSHAPE conditions are those of se3ds_crc32c_multi with the other polynomial.
 * table_dev / host_table: int64 [n][se3ds_crc32z_fields() = 3] = byte offset into buf, length,
 * seed (0 .. 2^32 - 1, anything else is BADSHAPE).  crc_dev[i] = zlib.crc32(range i, seed i): seed
 * 0 is the plain CRC-32, an empty range gives its seed. */
int se3ds_crc32z_multi(const uint8_t* buf, int64_t buf_bytes, const int64_t* table_dev,
                       const int64_t* host_table, int n, uint32_t* crc_dev, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t se3ds_crc32z_workspace_bytes(int64_t total_bytes, int n);
int se3ds_crc32z_fields(void);
int se3ds_crc32z_block_bytes(void);

/* ======================================================================================
 * VLN perturbation augmentation -- inference/perturbation_utils.py:63-70.  csrc/perturb.hip.
 * ====================================================================================== */

/* The collision screen for k candidate offsets in one launch: count[c] = number of pixels (r, x)
 * of image image_index[c] (NULL: image 0) of depth fp32 (n, height, width) with
 * row0 <= r < row1, col0 <= x < col1 and depth * depth_scale < threshold[c] -- one fp32 multiply,
 * one strict compare, a NaN never counts.  windows int32 (k, 4) = row0, row1, col0, col1;
 * threshold fp32 (k); all device pointers.  count int32 (k) is zeroed by the call itself (a memset
 * node on `stream`), the caller pre-fills nothing.  An empty window is legal and counts 0.
 * Deterministic (integer sums).  BADSHAPE for n, height, width or k < 1, k > 65535 or
 * height * width > INT32_MAX.  The window table is validated on the host, by
 * se3ds_collision_check_windows on the copy the caller made it from; the kernel clamps what it
 * gets to the image, so a bad table cannot make it read outside `depth`. */
int se3ds_collision_count(const float* depth, int n, int height, int width, const int32_t* windows,
                          const int32_t* image_index, const float* threshold, float depth_scale,
                          int k, int32_t* count, void* stream);
/* HOST pointers, no device work: BADSHAPE if a window leaves [0, height] x [0, width], has
 * row0 > row1 or col0 > col1, or an image index (NULL: none) lies outside [0, n). */
int se3ds_collision_check_windows(const int32_t* windows, const int32_t* image_index, int n,
                                  int height, int width, int k);

/* ======================================================================================
 * Inception-v3 evaluator -- utils/inception_utils.py, utils/eval_metric.py EvalMetric
 * (reference utils/inception_utils.py, utils/eval_metric.py:66-343).  csrc/inception.hip.
 * ====================================================================================== */
/* (N,H,W,3) fp32 frames in [0,1] -> network input (N,oh,ow,3) F32 / BF16, one gather:
 * indoor_datasets.augment (roll_flip: device int32 [N][2] = (roll, flip) per image, or NULL for
 * none), crop_pano(resize_to_original=False) (crop_rows = floor(H/8) rows off top and bottom),
 * tf.image.resize bilinear (half-pixel centres, no antialias; se3ds_resize's arithmetic), then
 * clip(x*2-1, -1, 1).  Bit-identical to that chain run op by op. */
int se3ds_inception_preprocess(const float* frames, int n, int h, int w, const int32_t* roll_flip,
                               int crop_rows, int oh, int ow, void* out, int out_dtype,
                               void* stream);
/* Keras MaxPooling2D(3, strides=2, 'valid') / AveragePooling2D(3, strides=1, 'same') (padded taps
 * excluded from the divisor), NHWC F32 / BF16.  x is dense (n,h,w,c); y's pixels have y_c
 * channels of which [y_c0, y_c0 + c) are written (a slice of a concatenated block output). */
int se3ds_inception_maxpool3s2(const void* x, int dtype, int n, int h, int w, int c, void* y,
                               int y_c, int y_c0, void* stream);
int se3ds_inception_avgpool3s1(const void* x, int dtype, int n, int h, int w, int c, void* y,
                               int y_c, int y_c0, void* stream);
/* GlobalAveragePooling2D: y (n,c) fp32 = mean over the hw pixels of x (n,hw,c) F32 / BF16. */
int se3ds_global_avg_pool(const void* x, int dtype, int n, int hw, int c, float* y, void* stream);
/* tf.nn.softmax over each row of x (rows,c) F32 / BF16 -> y fp32. */
int se3ds_softmax_rows(const void* x, int dtype, int64_t rows, int c, float* y, void* stream);
/* Running binary64 moments of fp32 rows x (rows,c): *count += rows, sum[j] += sum_b x[b,j],
 * gram[i][j] += sum_b x[b,i] x[b,j] for the 64 x 64 tiles with i-tile <= j-tile (the strictly
 * lower tiles are not written; the matrix is symmetric).  No atomics, fixed order:
 * bit-reproducible. */
int se3ds_feature_moments_accumulate(const float* x, int64_t rows, int c, int64_t* count,
                                     double* sum, double* gram, void* stream);

/* ---- The Frechet distance on the device, binary64 throughout.  csrc/frechet.hip. ---- */
/* C = alpha * A B + diag * I, all row-major n x n binary64, on v_mfma_f64_16x16x4_f64: one
 * 128 x 128 tile of C per 256-thread workgroup, K staged through LDS 16 at a time, the sum over k
 * in ascending order inside one accumulator per element; the epilogue rounds alpha * acc, then adds
 * diag where row == column.  n is arbitrary (1..16384); C must not alias A or B. */
int se3ds_f64_gemm(const double* a, const double* b, double* c, int n, double alpha, double diag,
                   void* stream);
/* The device moments of se3ds_feature_moments_accumulate -> mean[j] = sum[j] / n and the full
 * symmetric cov[i][j] = (gram[min(i,j)][max(i,j)] - sum[i] sum[j] / n) / (n - 1), n = *count as
 * binary64, each operation rounded as written (FeatureMoments.mean_cov()).  Only the upper tiles of
 * gram are read.  *count < 2 gives non-finite values: the caller checks the count. */
int se3ds_moments_mean_cov(const int64_t* count, const double* sum, const double* gram, int dim,
                           double* mean, double* cov, void* stream);
/* tr sqrt(A) (and sqrt(A)) of a symmetric positive semi-definite A (n x n) by the coupled
 * Newton-Schulz iteration: c = ||A||_F, Y0 = A / c, Z0 = I; T = 1.5 I - 0.5 Z Y, Y <- Y T,
 * Z <- T Z (three se3ds_f64_gemm products); after iteration k the trace of Y_k is taken and the
 * iteration stops when |tr Y_k - tr Y_{k-1}| <= tol |tr Y_k|, when the trace is not finite, or after
 * max_iters (0..1024) iterations.  sqrt(A) = sqrt(c) Y, tr sqrt(A) = sqrt(c) tr Y.  The stop rule
 * is part of the algorithm: for a singular A, Z grows without bound if the iteration runs on.
 * Everything is queued on `stream` with no host synchronisation: the trace kernel sets a device flag
 * and the kernels of the later iterations return at once.  Reductions have a fixed order and no
 * atomics.  root: n x n, or NULL.  result: device binary64 [4] = tr sqrt(A), iterations taken,
 * status (SE3DS_SQRT_*), ||A||_F.  A = 0 gives trace 0, a zero root, CONVERGED.  workspace: device,
 * 8-byte aligned, se3ds_sqrt_trace_workspace_bytes(n) bytes (0: n outside 1..16384). */
#define SE3DS_SQRT_CONVERGED 0
#define SE3DS_SQRT_CAP_REACHED 1
#define SE3DS_SQRT_NONFINITE 2
size_t se3ds_sqrt_trace_workspace_bytes(int n);
int se3ds_sqrt_trace(const double* a, int n, int max_iters, double tol, double* root,
                     void* workspace, size_t workspace_bytes, double* result, void* stream);
/* out[3] = |mu1 - mu2|^2, tr sigma1, tr sigma2 (device binary64, one workgroup, fixed order). */
int se3ds_frechet_terms(const double* mu1, const double* mu2, const double* sigma1,
                        const double* sigma2, int n, double* out, void* stream);

/* ======================================================================================
 * Semantic utilities -- utils/utils.py (reference utils/utils.py:23-198).  csrc/semantic.hip,
 * index arithmetic in csrc/nn_inpaint_core.h.
 * ====================================================================================== */

/* nearest_neighbor_inpaint (utils/utils.py:179-198): every pixel of image (n, h, w) U8 / I32 / F32
 * that equals the void class takes the value of the nearest pixel of the same image that does not,
 * nearest by squared Euclidean distance in pixel units; among equidistant sources the smallest row
 * wins, within it the smallest column (the reference's argmin over tf.where's row-major list).
 * Every other pixel is copied.  Values move bit for bit.  void_bits: the void class as the dtype's
 * bits, zero-extended; equality is == of the dtype (F32: -0.0 equals 0.0, a NaN never matches).
 * out: (n, h, w) of the same dtype, must not alias image.  indices: NULL, or int32 (n, h, w) that
 * receives the flat index y * w + x of every pixel's source: its own for a non-void pixel, -1 where
 * the image has no non-void pixel (such an image is copied unchanged).
 * workspace: device, 16-byte aligned, at least se3ds_nn_inpaint_workspace_bytes(n, h, w) bytes (0:
 * the shape is not valid): the row pass's table, an int16 column per pixel.
 * Two launches on `stream`: the row pass (one workgroup per image row, se3ds_nn_inpaint_row_segment()
 * columns at a time) and the column pass (se3ds_nn_inpaint_col_tile_rows() rows x 64 lanes per
 * workgroup; a lane owns one I32 / F32 pixel or four U8 pixels).  phases: 3 = both, what callers
 * pass; 1 = the row pass only, 2 = the column pass only, on a workspace that phase 1 filled for the
 * same image (tools/semantic_utils_bench.py times them apart).  Integers only, no atomics, no host
 * synchronisation: deterministic.
 * All checks run before the first HIP call.  BADSHAPE: n, h or w < 1, h or w > 16384, n > 65535,
 * a null or misaligned pointer, phases outside 1..3; BADDTYPE; WORKSPACE: too small. */
int se3ds_nn_inpaint(const void* image, int dtype, uint32_t void_bits, int n, int h, int w,
                     void* out, int32_t* indices, void* workspace, size_t workspace_bytes,
                     int phases, void* stream);
size_t se3ds_nn_inpaint_workspace_bytes(int n, int h, int w);
int se3ds_nn_inpaint_row_segment(void);
int se3ds_nn_inpaint_col_tile_rows(void);

/* Per-frame sums of compute_sequence_iou (utils/utils.py:98-133) over frames x (pixels, channels)
 * fp32, each frame dense: sums[f][0] = I = sum p * t * s, sums[f][1] = S = sum (p + t) * s, s the
 * spatial mask fp32 (frames, pixels) of the element's PIXEL (NULL: 1).  Every term is formed in
 * binary64 as (double)p * (double)t * (double)s and ((double)p + (double)t) * (double)s and added in
 * binary64.  Two stages: a workgroup per chunk of se3ds_seq_sums_chunk() elements of a frame writes
 * its pair to the workspace, a second launch adds a frame's pairs in a fixed order.  No atomics: the
 * same input at the same addresses gives the same bits on every run.  sums: device binary64
 * (frames, 2).  workspace: device, 8-byte aligned, se3ds_seq_sums_workspace_bytes(frames, pixels *
 * channels) bytes (0: not a valid shape).  BADSHAPE: a size < 1, pixels * channels > INT32_MAX,
 * frames * chunks per frame > INT32_MAX, a null or misaligned pointer; WORKSPACE. */
int se3ds_seq_iou_sums(const float* pred, const float* truth, const float* spatial, int64_t frames,
                       int64_t pixels, int channels, double* sums, void* workspace,
                       size_t workspace_bytes, void* stream);
/* Per-frame sums of compute_sequence_accuracy (utils/utils.py:136-176) over label maps (frames,
 * pixels) U8 / I32 (both of label_dtype): sums[f][0] = sum [pred == gt] * s, sums[f][1] = sum s.
 * spatial: NULL (s = 1) or (frames, pixels) of spatial_dtype U8 (also bool) / I32 / F32.  Integer
 * masks are added as integers (exact below 2^53), an fp32 mask in binary64; stages, workspace
 * (se3ds_seq_sums_workspace_bytes(frames, pixels)) and reproducibility as above. */
int se3ds_seq_label_match(const void* pred, const void* gt, int label_dtype, const void* spatial,
                          int spatial_dtype, int64_t frames, int64_t pixels, double* sums,
                          void* workspace, size_t workspace_bytes, void* stream);
size_t se3ds_seq_sums_workspace_bytes(int64_t frames, int64_t elems_per_frame);
int se3ds_seq_sums_chunk(void);
/* The (n, t)-sized tail of both metrics, one small launch, all in fp32 after I32 = (float)I and
 * S32 = (float)S (for IOU_LABELS: (float)(2 S), the S of the one-hot encodings):
 *   IOU, IOU_LABELS: seq = divide_no_nan(I32 * mask, (S32 - I32) * mask)
 *   ACCURACY:        seq = divide_no_nan(I32, S32)
 *   mean = (sum_n divide_no_nan(sum_t seq, sum_t mask)) / n, t = 0..t-1 and n = 0..n-1 in that order.
 * divide_no_nan(x, y) is 0 where y == 0.  mask fp32 (n, t); seq fp32 (n, t); mean fp32 (1). */
#define SE3DS_SEQ_IOU 0
#define SE3DS_SEQ_ACCURACY 1
#define SE3DS_SEQ_IOU_LABELS 2
int se3ds_seq_finalize(const double* sums, const float* mask, int n, int t, int mode, float* seq,
                       float* mean, void* stream);

/* cmap_to_label (utils/utils.py:43-57): labels[p] = the first k with cmap[k] == image[p] in all
 * three channels, 0 when there is none.  image (pixels, 3) U8 / I32; cmap device int32 (k, 3),
 * k <= 256; an entry or a pixel with a channel outside 0..255 matches nothing.  labels int32. */
int se3ds_cmap_to_label(const void* image, int dtype, int64_t pixels, const int32_t* cmap, int k,
                        int32_t* labels, void* stream);
/* The gather the other way: out uint8 (pixels, 3) = cmap[labels[p]] (low 8 bits of each channel),
 * (0, 0, 0) for a label outside [0, k).  labels U8 / I32. */
int se3ds_label_to_color(const void* labels, int dtype, int64_t pixels, const int32_t* cmap, int k,
                         uint8_t* out, void* stream);

/* ======================================================================================
 * Point-cloud .ply bodies -- utils/ply.py, SE3DSModel.write_memory_as_pointcloud (reference
 * models/models.py:154-178).  csrc/ply.hip, the characters in csrc/ply_format_core.h.
 * ====================================================================================== */

/* The ASCII body: per point the line `x y z r g b \n` (one space after every value), each float as
 * Python's repr of the value widened to binary64 (shortest round-trip digits; positional when the
 * decimal exponent of the first digit is in [-4, 16), else d[.ddd]e+XX; `nan`, `inf`, `-inf`, `-0.0`),
 * each colour as a decimal integer.  coords: three fp32 rows of m values, row k at coords + k *
 * row_stride (row_stride >= m: rows 0-2 of a (4, M) memory).  rgb: (m, 3) I32 or U8, dense.
 * out: device bytes, any alignment, out_capacity >= m * se3ds_ply_max_line_bytes(); the lines are
 * written back to back in input order from out[0], and nothing beyond that capacity is touched.
 * out_bytes: device int64, receives the byte count.  workspace: device, 16-byte aligned,
 * se3ds_ply_ascii_workspace_bytes(m) bytes (0: m is not valid).  0 <= m <= se3ds_ply_max_points() =
 * 2^24; m = 0 launches nothing and writes nothing, out_bytes included.
 * Three launches on `stream`, workgroups of se3ds_ply_chunk_points() points: records and chunk byte
 * totals (phase bit 1), one workgroup scanning the totals into 64-bit offsets and out_bytes (2),
 * characters through LDS with 16-byte stores (4).  phases: 7 is what callers pass; other non-empty
 * subsets run those launches alone on a workspace the earlier ones filled (tools/ply_bench.py).
 * Integers only, no atomics, no host synchronisation: the same input gives the same bytes.
 * All checks run before the first HIP call.  BADDTYPE: rgb_dtype; BADSHAPE: m, row_stride, a null or
 * misaligned pointer, out_capacity, phases outside 1..7; WORKSPACE: too small. */
int se3ds_ply_ascii(const float* coords, int64_t row_stride, const void* rgb, int rgb_dtype,
                    int64_t m, uint8_t* out, int64_t out_capacity, int64_t* out_bytes,
                    void* workspace, size_t workspace_bytes, int phases, void* stream);
size_t se3ds_ply_ascii_workspace_bytes(int64_t m);
int se3ds_ply_chunk_points(void);
int se3ds_ply_max_line_bytes(void);
int64_t se3ds_ply_max_points(void);
/* The binary_little_endian body: per point 15 bytes, float x, y, z then uchar red, green, blue, from
 * the same inputs.  out: device, 16-byte aligned, out_capacity >= 15 * m.  flag: device int32 that the
 * CALLER has zeroed; set to 1 when a colour lies outside [0, 255] (its low byte is written).  One
 * launch; m = 0 launches nothing.  Checks and error codes as above. */
int se3ds_ply_binary(const float* coords, int64_t row_stride, const void* rgb, int rgb_dtype,
                     int64_t m, uint8_t* out, int64_t out_capacity, int32_t* flag, void* stream);

/* ======================================================================================
 * Paired image metrics -- utils/image_metrics.py: PSNR, SSIM and MS-SSIM as tf.image.psnr /
 * ssim / ssim_multiscale define them (not in the reference tree).  csrc/image_metrics.hip.
 * ====================================================================================== */

/* SSIM of a against b, both (n, h, w, c) NHWC dense, both SE3DS_F32 or both SE3DS_U8, c in 1..4.
 * weights: HOST pointer to filter_size fp32 taps (1..15), copied into the launch.  G is the
 * separable window sum over a VALID window: the horizontal pass, then the vertical pass over its
 * results, taps in ascending order, the first tap one product and every later tap one product and
 * one add, all in binary64 with the taps and the pixels widened exactly; a b and a a + b b are formed
 * in binary64 before the window.  With c1 = (k1 max_val)^2, c2 = (k2 max_val)^2, m0 = G(a), m1 = G(b):
 *   n0 = 2 m0 m1, d0 = m0 m0 + m1 m1, lum = (n0 + c1) / (d0 + c1)
 *   n1 = 2 G(a b), d1 = G(a a + b b),  cs = (n1 - n0 + c2) / (d1 - d0 + c2)
 * per pixel of the (h - filter_size + 1) x (w - filter_size + 1) map and per channel.
 * ssim_mean, cs_mean: device binary64 (n, c), the means of lum cs and of cs over the map.  map: NULL,
 * or device binary64 (n, h', w', c) that receives lum cs.  workspace: device, 8-byte aligned,
 * se3ds_ssim_workspace_bytes(n, h, w, c, filter_size) bytes (0: the shape is not valid).
 * Two launches on `stream`: a workgroup per se3ds_ssim_tile_rows() x se3ds_ssim_tile_cols() tile of
 * the map stages its pixels (with a halo of filter_size - 1) in LDS once, forms all window sums there
 * and writes its sums to the workspace; the second launch adds an image's records in a fixed order.
 * No filtered plane is written, no atomics, no host synchronisation: deterministic bits.
 * All checks run before the first HIP call.  BADSHAPE: n outside 1..65535, c outside 1..4,
 * filter_size outside 1..15, h or w < filter_size or > 32768, max_val not > 0, a null or misaligned
 * pointer (map may be null); BADDTYPE; WORKSPACE: too small. */
int se3ds_ssim(const void* a, const void* b, int dtype, int n, int h, int w, int c,
               const float* weights, int filter_size, double max_val, double k1, double k2,
               double* ssim_mean, double* cs_mean, double* map, void* workspace,
               size_t workspace_bytes, void* stream);
size_t se3ds_ssim_workspace_bytes(int n, int h, int w, int c, int filter_size);
int se3ds_ssim_tile_rows(void);
int se3ds_ssim_tile_cols(void);
/* out[i] = sum over image i of (a - b)^2, device binary64 (n): a, b (n, elems_per_image) dense, both
 * F32 or both U8.  F32: ((double)a - (double)b)^2 added in binary64; U8: integers, the sum is exact.
 * Two stages as above: a workgroup per se3ds_sqdiff_chunk() elements, then a fixed-order sum; no
 * atomics.  workspace: device, 8-byte aligned, se3ds_sqdiff_workspace_bytes(n, elems_per_image) bytes
 * (0: not valid).  BADSHAPE: n outside 1..65535, elems_per_image outside 1..2^40, n * chunks >
 * INT32_MAX, a null or misaligned pointer; BADDTYPE; WORKSPACE. */
int se3ds_sqdiff_sum(const void* a, const void* b, int dtype, int n, int64_t elems_per_image,
                     double* out, void* workspace, size_t workspace_bytes, void* stream);
size_t se3ds_sqdiff_workspace_bytes(int n, int64_t elems_per_image);
int se3ds_sqdiff_chunk(void);
/* The step between MS-SSIM scales: x (n, h, w, c) F32 or U8 -> out fp32 (n, ceil(h / 2), ceil(w / 2),
 * c), the 2 x 2 mean at stride 2 after an odd side is extended by repeating its last row or column
 * (TensorFlow's SYMMETRIC pad of one): ((x00 + x01) + x10) + x11 in binary64, times 0.25, rounded
 * once to fp32.  One launch.  BADSHAPE: n outside 1..65535, h or w outside 1..32768, c outside 1..4,
 * a null or misaligned pointer; BADDTYPE. */
int se3ds_downsample2_sym(const void* x, int dtype, int n, int h, int w, int c, float* out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SE3DS_HIP_H_ */
