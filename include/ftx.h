/* libftx — C ABI of the MI355X (gfx950) hot path of FusionTransformer.
 *
 * The reference (aliabdelkader/FusionTransformer) has no FFI layer of its own:
 * its native work is reached through torchsparse v1.1.0 (`spf.*`, `spnn.*`),
 * timm 0.4.9 and torch.  Each entry point below replaces one of those native
 * ops at the call site cited next to it (paths relative to the reference
 * root).  The host side (fusiontransformer_amd/) binds these with ctypes; the
 * binding a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *     row-major, contiguous; the caller owns every buffer (inputs, outputs and
 *     workspaces) and the library keeps nothing beyond the call;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it,
 *     nothing synchronises the host (safe for hipGraph capture) unless stated;
 *   - return 0 on success, a negative FTX_E* code otherwise; the message is in
 *     the thread-local ftx_last_error(); nothing throws, nothing aborts;
 *   - index dtype on the device is int32 (-1 = absent); hashes are int64.
 */
#ifndef FTX_H
#define FTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FTX_OK 0
#define FTX_EINVAL -1  /* bad argument (null pointer, negative size, unsupported shape) */
#define FTX_ELAUNCH -2 /* HIP runtime reported an error at launch */
#define FTX_EWORKSPACE -3 /* workspace too small */

/* library version (major*10000 + minor*100 + patch) and last error text */
int ftx_version(void);
const char *ftx_last_error(void);

/* ---- per-(device, stream) ticket buffer of the statistics kernels (ftx_spconv_reduce_stats, ftx_bn_train_fwd / _bwd) ----
 * Those kernels hand their column totals to "the last block to finish", which needs a few ticket counters and group rows that persist
 * across the blocks of a launch (csrc/ftx_lastblock.h).  The caller owns them: allocate ftx_stream_scratch_bytes() bytes of device
 * memory (256-byte aligned), attach them to the stream (the library zeroes the tickets on that stream) and keep them alive until
 * ftx_stream_scratch_release(stream) or the end of the process.  A stream nobody attached a buffer to gets a library allocation at its
 * first use (outside stream capture), freed by ftx_stream_scratch_release.  ftx_stream_scratch_reset zeroes the tickets on the stream:
 * call it after a kernel of the library died mid-flight (a dirty ticket otherwise trips a device-side assert in the next launch).
 * Keyed by (current device, stream).  No other state of the library outlives a call. */
size_t ftx_stream_scratch_bytes(void);
int ftx_stream_scratch_attach(void *stream, void *buffer, size_t bytes);
int ftx_stream_scratch_reset(void *stream);
int ftx_stream_scratch_release(void *stream);

/* ---- coordinate hashing ------------------------------------------------ */

/* spf.sphash(C): models/utils.py:19,49,79.  coords (n,4) int32 [x,y,z,b] -> out (n) int64. */
int ftx_hash(const int32_t *coords, int64_t n, int64_t *out, void *stream);

/* spf.sphash(C, off): models/utils.py:74-78.  offsets (k,3) int32 -> out (k,n) int64. */
int ftx_hash_kernel(const int32_t *coords, int64_t n, const int32_t *offsets, int32_t k, int64_t *out, void *stream);

/* torch.floor(z.C[:, :3] / s).int() * s ++ z.C[:, -1].int(): models/utils.py:44-48,75-78.
 * pc (n,4) float32 -> out (n,4) int32. */
int ftx_floor_coords(const float *pc, int64_t n, int32_t stride, int32_t *out, void *stream);

/* ---- hash table (spf.sphashquery): models/utils.py:21,50,80 -------------- */

/* Smallest legal capacity (a power of two >= 2n) for n keys. */
int64_t ftx_hashtable_capacity(int64_t n);
/* Build: table_keys (capacity) int64 and table_vals (capacity) int32 are fully
 * (re)initialised here.  Duplicate keys keep the smallest row index. */
int ftx_hashtable_build(const int64_t *keys, int64_t n, int64_t *table_keys, int32_t *table_vals, int64_t capacity, void *stream);
/* Query: out[i] = row of queries[i] in the keys the table was built from, or -1. */
int ftx_hashtable_query(const int64_t *queries, int64_t nq, const int64_t *table_keys, const int32_t *table_vals, int64_t capacity, int32_t *out, void *stream);

/* spf.spcount(idx, m): models/utils.py:22,51.  counts (m) int32 is zeroed here. */
int ftx_count(const int32_t *idx, int64_t n, int32_t *counts, int64_t m, void *stream);

/* torch.unique(hash) (sorted): models/utils.py:20 and torchsparse spdownsample.
 * uniq (n) int64 receives the sorted unique keys, first_index (n) int32 the row of
 * the first occurrence of each, n_unique (1) int32 (device) their number.
 * Rows past n_unique are unspecified. */
size_t ftx_unique_workspace_bytes(int64_t n);
int ftx_unique_sorted(const int64_t *keys, int64_t n, int64_t *uniq, int32_t *first_index, int32_t *n_unique, void *workspace, size_t workspace_bytes, void *stream);
/* rank[i] = position of queries[i] in sorted[0 .. min(*n_sorted, capacity)) (ascending, unique; the count is read ON THE DEVICE), -1 when
 * absent.  On the output of ftx_unique_sorted this is numpy.unique's return_inverse, i.e. the inverse map of torchsparse
 * sparse_quantize(..., return_invs=True) (data/semantic_kitti/semantic_kitti_dataloader.py:231). */
/* out[i,:] = points[i,:] . R (R: 9 floats, row-major, on the HOST) with the rounding of numpy's float32 `points.dot(rot_matrix)` --
 * one fused multiply-add per step of K = 3 --: the rotation / flip of data/utils/augmentation_3d.py:22-41 on the device */
int ftx_rotate_points(const float *points, int64_t n, const float *rot_host, float *out, void *stream);
int ftx_sorted_rank(const int64_t *sorted, const int32_t *n_sorted, int64_t capacity, const int64_t *queries, int64_t nq, int32_t *rank, void *stream);

/* torchsparse spdownsample coordinate rule: floor(c / ratio) * ratio on x,y,z, b kept.
 * coords (n,4) int32 -> out (n,4) int32.  (inside spnn.Conv3d(stride=2): models/spvcnn.py:105,111,117,123) */
int ftx_downsample_coords(const int32_t *coords, int64_t n, int32_t ratio, int32_t *out, void *stream);

/* out[i,:] = src[index[i],:] for int32 rows of width 4 (coordinate gather). */
int ftx_gather_coords(const int32_t *src, const int32_t *index, int64_t n, int32_t *out, void *stream);

/* Every level of the U-Net in ONE pass (models/spvcnn.py:104-126 visits strides 1, 2, 4, 8, 16; torchsparse's spdownsample derives
 * level l+1 from level l, one hash + torch.unique + size read per level): points (n,4) int32 = the floored point coordinates;
 * for each of the n_levels strides (HOST array, each >= 1, at most 8) the set unique(floor_div(p, s) * s) in ascending hash order.
 * uniq (n_levels*n) int64: the levels' sorted unique hashes back to back; first_index (n_levels*n): the point row of the first
 * occurrence of each; level_off (n_levels+1) int32 DEVICE: where each level's run starts (level_off[n_levels] = total).  The caller
 * reads level_off once (the only host read of the whole coordinate build besides the pair counts) and takes the level's coordinates
 * with ftx_level_coords(points, first_index + level_off[l], n_l, stride, out).  Same sets, order and coordinates as the chained form. */
size_t ftx_levels_workspace_bytes(int64_t n, int32_t n_levels);
int ftx_levels_unique(const int32_t *points, int64_t n, const int32_t *strides, int32_t n_levels, int64_t *uniq, int32_t *first_index, int32_t *level_off, int64_t *sorted_keys, int32_t *order, void *workspace, size_t workspace_bytes, void *stream);
/* sorted_keys / order (n_levels*n each, may be NULL): the (level tag << 60 | hash) keys in sorted order and the point row of each; level l
 * owns [l*n, (l+1)*n): its points sorted by voxel, stable.  ftx_level_segments turns that slice into the sorted segments of spvoxelize at
 * the level's stride (what ftx_segment_build(idx_query, n, m) would return) without another sort: seg_off (m+1) from the level's unique
 * hashes (`uniq + level_off[l]`, m = n_l of them). */
int ftx_level_segments(const int64_t *sorted_keys, int64_t n, const int64_t *uniq, int64_t m, int32_t level, int32_t *seg_off, void *stream);
int ftx_level_coords(const int32_t *points, const int32_t *first_index, int64_t n, int32_t stride, int32_t *out, void *stream);

/* ---- kernel maps (inside spnn.Conv3d): models/spvcnn.py:26-30,42-46,57-72,99-101 */

/* nbr[k, o] = row in the table's key set of (out_coords[o] + offsets[k]), or -1.
 * Fuses sphash(out_coords, offsets) + sphashquery.  nbr is (k, n_out) int32. */
int ftx_kernel_map_build(const int32_t *out_coords, int64_t n_out, const int32_t *offsets, int32_t k, const int64_t *table_keys, const int32_t *table_vals, int64_t capacity, int32_t *nbr, void *stream);
/* Pair list of a kernel map (what torchsparse's convert_neighbor_map builds): the valid
 * (k, o) entries of nbr compacted in (k, o) order.
 *   step 1  ftx_kernel_map_count: pos (k, n_out) receives the exclusive scan of the validity
 *           flags, koff (k+1, device) the first pair of every offset; koff[k] = number of pairs
 *           (the caller reads it back to size the pair arrays).
 *   step 2  ftx_kernel_map_pairs: pair_in[p] / pair_out[p] = input / output row of pair p;
 *           pos[k,o] = p or -1; pos_t (k, n_in): pos_t[k, i] = p of the pair (k, i) or -1. */
size_t ftx_kernel_map_count_workspace_bytes(int64_t n_out, int32_t k);
int ftx_kernel_map_count(const int32_t *nbr, int64_t n_out, int32_t k, int32_t *pos, int32_t *koff, void *workspace, size_t workspace_bytes, void *stream);
int ftx_kernel_map_pairs(const int32_t *nbr, int64_t n_out, int64_t n_in, int32_t k, int32_t *pos, int32_t *pos_t, int32_t *pair_in, int32_t *pair_out, int64_t n_pairs, void *stream);

/* spf.calc_ti_weights: models/utils.py:81-82.  pc (n,4) float32 (integer-valued or not),
 * idx (n,8) int32 (point-major, as after the transpose at utils.py:83), weights (n,8) float32. */
int ftx_trilinear_weights(const float *pc, const int32_t *idx, int64_t n, int32_t scale, float *weights, void *stream);

/* ---- point <-> voxel feature movement ----------------------------------- */

/* spf.spvoxelize fwd: models/utils.py:24-27,58.  out (m,c) is zeroed here;
 * out[idx[i]] += feats[i] / counts[idx[i]]. */
int ftx_voxelize_fwd(const float *feats, const int32_t *idx, const int32_t *counts, int64_t n, int32_t c, int64_t m, float *out, void *stream);
/* bwd: grad_feats[i] = grad_out[idx[i]] / counts[idx[i]] (0 where idx<0). */
int ftx_voxelize_bwd(const float *grad_out, const int32_t *idx, const int32_t *counts, int64_t n, int32_t c, int64_t m, float *grad_feats, void *stream);

/* spf.spdevoxelize fwd: models/utils.py:87,99.  out[i] = sum_k w[i,k] * feats[idx[i,k]]. */
int ftx_devoxelize_fwd(const float *feats, const int32_t *idx, const float *weights, int64_t n, int32_t c, int64_t m, float *out, void *stream);
/* bwd: grad_feats (m,c) zeroed here; grad_feats[idx[i,k]] += w[i,k] * grad_out[i]. */
int ftx_devoxelize_bwd(const float *grad_out, const int32_t *idx, const float *weights, int64_t n, int32_t c, int64_t m, float *grad_feats, void *stream);

/* Sorted-segment forms of the two scatter sides (no float atomics, bit-reproducible).
 * ftx_segment_build: keys (n) int32 = destination row of each entry (<0 or >=m: dropped);
 *   order (n) int32 receives the entry ids sorted by destination (ties in ascending entry id),
 *   seg_off (m+1) int32 the first position of every destination's run.
 * voxelize:   keys = idx (point -> voxel), entries = points.
 * devoxelize: keys = idx (n,8) flattened with zero-weight corners set to -1, entries = (point, corner). */
size_t ftx_segment_workspace_bytes(int64_t n, int64_t m);
int ftx_segment_build(const int32_t *keys, int64_t n, int64_t m, int32_t *order, int32_t *seg_off, void *workspace, size_t workspace_bytes, void *stream);
/* out[v] = mean of feats[p] over the points p of voxel v (0 for empty voxels); out (m,c) fully written. */
int ftx_voxelize_fwd_sorted(const float *feats, const int32_t *order, const int32_t *seg_off, int64_t n, int32_t c, int64_t m, float *out, void *stream);
/* grad_feats[v] = sum over entries e=(p,k) of voxel v of weights[e] * grad_out[p]; weights (n,8) flattened, n = points. */
int ftx_devoxelize_bwd_sorted(const float *grad_out, const float *weights, const int32_t *order, const int32_t *seg_off, int64_t n, int32_t c, int64_t m, float *grad_feats, void *stream);

/* out[v] = sum of src[e] over the entries of segment v, in entry order (generic atomic-free scatter-add); out (m,c) fully written. */
int ftx_segment_sum(const float *src, const int32_t *order, const int32_t *seg_off, int64_t n, int32_t c, int64_t m, float *out, void *stream);

/* ---- 2D -> 3D lift ------------------------------------------------------- */

/* Fused `nn.Upsample((H,W))` (nearest) + per-point gather of
 * Net2DBillinear.get_img_feats: models/image_models_billinear.py:113,117-124.
 * grid (b, gh, gw, c) float32 channels-last (= the (B,576,96) token layout);
 * img_idx (n,2) int64 (row,col) in the (H,W) lift image; point_batch (n) int32;
 * out (n,c).  The (H,W,c) map is never materialised. */
int ftx_lift_gather_fwd(const float *grid, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t b, int32_t gh, int32_t gw, int32_t c, int32_t H, int32_t W, float *out, void *stream);
/* bwd: grad_grid (b,gh,gw,c) zeroed here, scatter-add of grad_out rows. */
int ftx_lift_gather_bwd(const float *grad_out, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t b, int32_t gh, int32_t gw, int32_t c, int32_t H, int32_t W, float *grad_grid, void *stream);

/* cells[i] = flat index (frame, source row, source col) of point i's cell in the (b, gh, gw) grid (-1 if out of range):
 * keys for ftx_segment_build so that the lift backward is ftx_segment_sum over the grid cells (no float atomics). */
int ftx_lift_cells(const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t b, int32_t gh, int32_t gw, int32_t H, int32_t W, int32_t *cells, void *stream);

/* `nn.Upsample((oh,ow))` nearest on NCHW: models/image_models_billinear.py:17,41.
 * in (b,c,ih,iw) -> out (b,c,oh,ow). bwd zeroes grad_in and scatter-adds. */
int ftx_resample_nearest_fwd(const float *in, int32_t b, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow, float *out, void *stream);
int ftx_resample_nearest_bwd(const float *grad_out, int32_t b, int32_t c, int32_t ih, int32_t iw, int32_t oh, int32_t ow, float *grad_in, void *stream);

/* Fused Net2DBillinear.sample_down: Conv1x1(3->3) + ReLU + BatchNorm2d(3) on the full-resolution
 * image + nearest pick to (oh, ow) (models/image_models_billinear.py:8-24,41,131).
 * img (b,3,h,w); conv_w (3,3) row-major [out][in]; out (b,3,oh,ow); saved (33) float64 device scratch
 * kept for the backward (training statistics of the full-resolution map).  training != 0: batch
 * statistics (running_* updated when non-NULL); training == 0: running statistics.
 * bwd (training mode) writes the four parameter gradients; the image gets none (it is an input). */
size_t ftx_sample_down_workspace_bytes(void);
int ftx_sample_down_fwd(const float *img, int32_t b, int32_t h, int32_t w, int32_t oh, int32_t ow, const float *conv_w, const float *conv_b, const float *gamma, const float *beta, float *running_mean, float *running_var, float momentum, float eps, int32_t training, float *out, double *saved, void *workspace, size_t workspace_bytes, void *stream);
int ftx_sample_down_bwd(const float *img, const float *grad_out, int32_t b, int32_t h, int32_t w, int32_t oh, int32_t ow, const float *conv_w, const float *conv_b, const float *gamma, const double *saved, float *grad_conv_w, float *grad_conv_b, float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- affine grid sampling (the spatial transformers of ImageSeg) ---------
 * F.grid_sample(src, F.affine_grid(theta, (b, ., H, W), align_corners=False), mode="bilinear", padding_mode="zeros",
 * align_corners=False) of models/transformers.py:133-134 without the grid: output pixel (r, c) of an (H, W) target reads the source at
 *   ix = ((t00 xn + t01 yn + t02 + 1) iw - 1) / 2,  iy likewise from row 1 of theta,  xn = (2c+1)/W - 1, yn = (2r+1)/H - 1,
 * as the four-corner bilinear sum; corners outside the source count as 0.  src is (b, c, ih, iw) float32 addressed through
 * src_strides = the four element strides (frame, channel, row, column) in HOST memory, all >= 0: NCHW and channels-last are the same
 * code.  theta (b, 2, 3) float32.  b <= 128.  The dense and the point form share one device function and agree bit for bit.
 *
 * Dense form (SpatialTransformer.forward): out (b, c, oh, ow) NCHW, fully written. */
int ftx_affine_sample_fwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *theta, int32_t oh, int32_t ow, float *out, void *stream);
/* Workspace of the two theta gradients below (per-block float64 partial rows; the last block to finish adds them in block order). */
size_t ftx_affine_theta_workspace_bytes(int32_t b);
/* grad_theta (b, 2, 3) from grad_out (b, c, oh, ow); no float atomics, bit-reproducible.  The dense form has no gradient for src. */
int ftx_affine_sample_bwd_theta(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *theta, const float *grad_out, int32_t oh, int32_t ow, float *grad_theta, void *workspace, size_t workspace_bytes, void *stream);
/* Point form (ScaleUpModule + get_img_feats, models/image_models_stn.py:88-98): img_idx (n, 2) int64 (row, col) in the (H, W) target,
 * point_batch (n) int32; out (n, c) = the rows the dense result would hold at (point_batch, :, row, col).  A point whose frame or
 * pixel is out of range gives a zero row and takes no gradient.  The (H, W) map is never materialised. */
int ftx_affine_lift_fwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *theta, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t H, int32_t W, float *out, void *stream);
/* cells[i] = flat key ((frame, y0 + 1, x0 + 1) in (b, ih + 1, iw + 1)) of the top-left source cell (y0, x0) of point i's sample, so a
 * sample that is half outside still has a key; -1 for a point that contributes nothing.  Keys for ftx_segment_build. */
int ftx_affine_lift_cells(const float *theta, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t b, int32_t ih, int32_t iw, int32_t H, int32_t W, int32_t *cells, void *stream);
/* Backward of the point form from grad_out (n, c).  grad_src (NULL: skipped): same shape and strides as src, every element written
 * once -- each gathers from the four segments (order, seg_off: ftx_segment_build over ftx_affine_lift_cells' keys, m = b (ih+1) (iw+1))
 * that can touch it, in a fixed order.  grad_theta (NULL: skipped): (b, 2, 3), needs the workspace.  No float atomics. */
int ftx_affine_lift_bwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *theta, const int64_t *img_idx, const int32_t *point_batch, const float *grad_out, int64_t n, int32_t H, int32_t W, const int32_t *order, const int32_t *seg_off, float *grad_src, float *grad_theta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the spatial transformers' localisation net (models/transformers.py:106-114) ---------
 * One fused layer  y = relu(max_pool2d(conv2d(x, w, bias), 2, 2))  of a stride-1, unpadded k x k convolution; served (k, co) = (7, 8)
 * and (5, 90), any c >= 1.  x (b, c, ih, iw) float32 by x_strides = four element strides (frame, channel, row, column) in HOST
 * memory, all >= 0 (NCHW and channels-last are the same code); w (co, c, k, k) and bias (co, NULL: none) contiguous.  Pooled size
 * ph = (ih - k + 1) / 2, pw likewise; a size with ph or pw = 0 is refused (FTX_EINVAL).  b <= 128.  The un-pooled map never exists.
 * Exact float32 products, fixed orders of summation, no float atomics: every output repeats bit for bit.
 *
 * fwd: sel (b, co, ph, pw) int8 = position 0..3 (row-major, the first on a tie) of the window's maximum, -1 where the maximum is <= 0
 * or NaN (dead ReLU, no gradient).  Exactly one of out (b, co, ph, pw) and mean (b, co) is non-NULL: mean receives the spatial mean of
 * the pooled map instead of the map and needs the workspace (per-tile float64 sums, added in tile order). */
size_t ftx_loc_conv_pool_relu_fwd_workspace_bytes(int32_t b, int32_t co, int32_t ph, int32_t pw);
int ftx_loc_conv_pool_relu_fwd(const float *x, const int64_t *x_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *w, const float *bias, int32_t k, int32_t co, float *out, int8_t *sel, float *mean, void *workspace, size_t workspace_bytes, void *stream);
/* grad_w (co, c, k, k) and grad_bias (co) from x, sel and the pooled gradient, which is addressed by grad_strides = four element
 * strides (frame, channel, row, column) in HOST memory, 0 allowed: the mean's backward is g[b, co] / (ph pw) with strides (co, 1, 0, 0).
 * Only the routed position of a window contributes.  Per-block float64 partials in the workspace, added in block order. */
size_t ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes(int32_t b, int32_t c, int32_t ih, int32_t iw, int32_t k, int32_t co);
int ftx_loc_conv_pool_relu_bwd_weight(const float *x, const int64_t *x_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const int8_t *sel, const float *grad, const int64_t *grad_strides, int32_t k, int32_t co, float *grad_w, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream);
/* grad_x (b, c, ih, iw) by grad_x_strides (as x_strides), every element written exactly once (a gather over the routed gradients). */
int ftx_loc_conv_pool_relu_bwd_data(const float *w, const int8_t *sel, const float *grad, const int64_t *grad_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, int32_t k, int32_t co, float *grad_x, const int64_t *grad_x_strides, void *stream);

/* ---- sparse convolution (spnn.Conv3d fwd/bwd) ----------------------------
 * Pair-list gather-GEMM + ordered reduce (exact-fp32 MFMA, no float atomics, bit-reproducible):
 *   forward       tmp = pairs_gemm(A=in,   gather=pair_in,  W, 0);  out = reduce(tmp, pos,   n_out)
 *   data grad     tmp = pairs_gemm(A=gout, gather=pair_out, W, 1);  gin = reduce(tmp, pos_t, n_in)
 *   weight grad   dW  = pairs_wgrad(A=in, pair_in, G=gout, pair_out)
 *   transposed conv (models/spvcnn.py:42-46): the same three calls with in/out roles swapped. */

/* tmp[p,:] = A[gather[p],:] @ Wk(p), k(p) from koff.  A (rows_a, ca); gather (n_pairs) int32;
 * W (kvol, ca, co) row-major when w_transposed == 0, (kvol, co, ca) used as W[k]^T when 1;
 * koff (kvol+1) int32 DEVICE; tmp (n_pairs, co) fully written. */
int ftx_spconv_pairs_gemm(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream);

/* One-launch convolution when every destination row receives exactly one pair (the strided 2^3 map seen from its
 * fine side: data gradient of the strided conv, forward of the transposed conv, models/spvcnn.py:38-50):
 * out[scatter[p],:] = A[gather[p],:] @ Wk(p).  scatter (n_pairs) int32 must be injective; out (rows_out, co); rows not
 * named by scatter are left untouched.  Replaces pairs_gemm + reduce (no tmp round trip). */
int ftx_spconv_pairs_gemm_scatter(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *out, int64_t rows_out, void *stream);

/* Output-stationary convolution for thin layers, ONE launch (csrc/ftx_spconv_ostat.hip): out[o,:] = sum over k (ascending) of
 * A[nbr[k,o],:] @ W[k], with nbr (kvol, n_out) int32 the neighbour table of the map (-1 = absent; what ftx_kernel_map_build returns).
 * No pair-row scratch and no reduce pass; bit-identical to ftx_spconv_pairs_gemm + ftx_spconv_reduce on the pair list of the same
 * table.  Replaces the Conv3d of models/spvcnn.py:22-35,98-126 where ftx_spconv_ostat_supported(ca, co, kvol, w_transposed) != 0
 * (ca in {4, 32, 64}, co in {32, 64}).  W (kvol, ca, co), or (kvol, co, ca) when w_transposed.
 * flip != 0: the data gradient of a submanifold convolution on the SAME table (symmetric map, odd kvol): out[i,:] = sum over k of
 * A[nbr[kvol-1-k, i],:] @ W[k] -- pass the output gradient as A, w_transposed = 1 and the forward kernel as W.
 * part != NULL: also the BatchNorm statistics of `out` as ftx_spconv_reduce_stats leaves them -- nb = ftx_spconv_ostat_blocks(n_out)
 * partial rows [nb][2][co] float64 followed by the totals row [2][co] (read by ftx_bn_train_fwd_totals); uses the stream's ticket buffer. */
int32_t ftx_spconv_ostat_supported(int32_t ca, int32_t co, int32_t kvol, int32_t w_transposed);
int32_t ftx_spconv_ostat_blocks(int64_t n_out);
int ftx_spconv_ostat(const float *A, int64_t rows_a, const int32_t *nbr, int64_t n_out, const float *W, int32_t w_transposed, int32_t flip, int32_t ca, int32_t co, int32_t kvol, float *out, double *part, int32_t nb, void *stream);

/* Dense rows on the same tile code: out[r,:] = A[r,:] @ W (+ bias), r < n.  W as above with kvol = 1;
 * bias (co) may be NULL.  Replaces the point-branch nn.Linear layers (models/spvcnn.py:164-180,
 * models/middle_fusion.py:18-29) and the kernel_size=1 spnn.Conv3d (spvcnn.py:71-75). */
int ftx_rows_gemm(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co, float *out, void *stream);
/* Host-only: the output columns per block (32, 64, 96 or 128) that ftx_spconv_pairs_gemm / _scatter (kvol >= 1, n_pairs pairs) or
 * ftx_rows_gemm (kvol = 0, n_pairs rows) pick for co output channels; -1 for invalid arguments.  Launches nothing. */
int32_t ftx_spconv_gemm_block_cols(int32_t co, int64_t n_pairs, int32_t kvol);

/* out[r,:] = sum over k (ascending) of tmp[pos[k,r],:] for pos >= 0; out (n, co) fully written. */
int ftx_spconv_reduce(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, float *out, void *stream);

/* The reduce with the eval-mode BatchNorm (+ residual) (+ ReLU) in its epilogue, one launch:
 *   out[r,:] = relu?( (sum_k tmp[pos[k,r],:] - running_mean) * 1/sqrt(running_var + eps) * gamma + beta (+ residual[r,:]) )
 * BIT-IDENTICAL to ftx_spconv_reduce followed by ftx_bn_eval_fwd on its output (same summation order, the same per-element expression:
 * csrc/ftx_bn_eval_op.h), without the write and the read of the (n, co) convolution output in between.  What the eval forward of a
 * Conv3d -> BatchNorm layer on the pair-list route runs (models/spvcnn.py:22-35,53-79 under model.eval()).
 * co a multiple of 4; kvol must be 8 or 27; residual (n, co) may be NULL; relu != 0 applies max(., 0) as !(t > 0) ? 0 : t.
 * tmp may be NULL when no entry of pos is >= 0.  No atomics, no host synchronisation, capturable. */
int ftx_spconv_reduce_bn_eval(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, const float *residual, const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps, int32_t relu, float *out, void *stream);

/* The reduce pass that also produces the BatchNorm statistics of its output: part (nb + 1, 2, co) float64 -- nb per-block
 * partial (sum, sum of squares) rows, nb = ftx_spconv_reduce_stats_blocks(n, co), then ONE row of column totals, summed in block
 * order by whichever block finishes last (no second launch; bit-reproducible).  Feed `part + nb*2*co` to
 * ftx_bn_train_fwd_totals: the Conv3d -> BatchNorm pair of every SPVCNN block (models/spvcnn.py:22-35,53-79) then reads the
 * convolution output once.  Uses the stream's ticket buffer (ftx_stream_scratch_* below). */
int32_t ftx_spconv_reduce_stats_blocks(int64_t n, int32_t co);
int ftx_spconv_reduce_stats(const float *tmp, const int32_t *pos, int64_t n, int32_t co, int32_t kvol, float *out, double *part, int32_t nb, void *stream);

/* dW[k] = sum_{p in offset k} A[idx_a[p],:]^T @ G[idx_g[p],:]  -> dW (kvol, ca, cg), fully written.
 * idx_a = idx_g = koff = NULL with kvol = 1: dense rows, dW = A[:n_pairs]^T @ G[:n_pairs]. */
size_t ftx_spconv_pairs_wgrad_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol);
int ftx_spconv_pairs_wgrad(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace, size_t workspace_bytes, void *stream);
/* Resident blocks per CU the weight-gradient tiling assumes for a (ca, cg) layer / for a kernel instantiation (mi, wmg, ni, wng): a
 * constant table (csrc/ftx_spconv.hip), never a device query, so workspace size, tile length and summation order are functions of the
 * arguments alone.  Exposed so that the build can check the table against the code object (tests/test_cabi.py). */
int32_t ftx_spconv_wgrad_resident_blocks(int32_t ca, int32_t cg);
int32_t ftx_spconv_wgrad_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng);

/* bf16-operand sparse convolution (csrc/ftx_spconv_bf16.hip): the same calls, with the same arguments, on v_mfma_f32_32x32x16_bf16.
 * Precision contract: the MFMA operands -- A and W of the pair GEMM and of the dense rows, A and G of the weight gradient -- are rounded
 * to bf16 (round-to-nearest-even) from their stored fp32 values as they are staged; nothing else is rounded.  Accumulation is fp32, and
 * all storage stays fp32: A, W, G, bias, out, dW and the pair rows `tmp`, which keep the layout of ftx_spconv_pairs_gemm, so
 * ftx_spconv_reduce / ftx_spconv_reduce_stats consume them unchanged (fixed summation order over offsets).  The bias is added in
 * fp32.  Gather rules as above: an out-of-range source index gives a zero row.  No atomics: results are deterministic, the weight
 * gradient's partial tiles are added in a fixed order, and tile shapes and workspace sizes are functions of the arguments alone. */
int ftx_spconv_pairs_gemm_bf16(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream);
int ftx_spconv_pairs_gemm_scatter_bf16(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *out, int64_t rows_out, void *stream);
int ftx_rows_gemm_bf16(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co, float *out, void *stream);
size_t ftx_spconv_pairs_wgrad_bf16_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol);
int ftx_spconv_pairs_wgrad_bf16(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only queries, as ftx_spconv_gemm_block_cols / ftx_spconv_wgrad_table_blocks, for the bf16 kernels' own tilings. */
int32_t ftx_spconv_gemm_bf16_block_cols(int32_t co, int64_t n_pairs, int32_t kvol);
int32_t ftx_spconv_wgrad_bf16_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng);

/* fp32-accurate sparse convolution on the bf16 MFMA (csrc/ftx_spconv_split.hip): the same calls, with the same arguments, argument
 * rules and error texts, from a three-piece split of every operand; opt-in (cfg.MODEL.lidar_split), the default stays the exact fp32
 * entries above.  No operand bit is discarded below the stated range and the result is fp32-class (measured: DESIGN section 5).
 * Precision contract, the one of the dense split entries (ftx_dense_gemm_split below; csrc/ftx_split.h is the one definition of the
 * split for both):
 *   split     every fp32 operand element x -- A and W of the pair GEMM and of the dense rows, A and G of the weight gradient -- is split
 *             as it is staged, round-to-nearest-even, both subtractions in fp32 (they are exact):
 *             h = bf16(x),  m = bf16(x - h),  l = bf16((x - h) - m).  If h is not finite, m = l = 0.
 *   products  six of the nine piece products are summed, fp32 accumulation on v_mfma_f32_32x32x16_bf16: hh, hm, mh, hl, lh, mm (first
 *             letter: the piece of A).  Each bf16 x bf16 product is exact in fp32.  The dropped ml, lm, ll are each below
 *             2.01 * 2^-24 * |a b|.
 *   order     fixed: two fp32 accumulators per output element.  One takes the hh products alone, reduction index ascending.  The other
 *             takes, per 16-wide reduction step, mm, hl, lh, hm, mh in that order (smallest first).  They are added once, after the
 *             last step: sum = hh + corrections; the bias is added to that in fp32.  In the weight gradient the waves that share an
 *             output element each take a subset of the steps (on the smallest tiles: of a step's products, in the order above), add
 *             their two accumulators once, and their sums are added in wave order; partial tiles are added by wgrad_reduce_kernel in
 *             tile order.  No atomics: results are deterministic and a function of the arguments alone.  They are not bit-identical to
 *             the fp32 entries (another summation tree).
 *   storage   A, W, G, bias, out, dW and the pair rows `tmp` stay fp32; `tmp` keeps the layout of ftx_spconv_pairs_gemm, so
 *             ftx_spconv_reduce, ftx_spconv_reduce_stats and ftx_spconv_reduce_bn_eval consume it unchanged.
 * Gather rules as above: an out-of-range source index gives a zero row.  Tile shapes and workspace sizes are functions of the arguments
 * alone; the column rule is the fp32 entries' (ftx_spconv_gemm_split_block_cols == ftx_spconv_gemm_block_cols). */
int ftx_spconv_pairs_gemm_split(const float *A, int64_t rows_a, const int32_t *gather, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *tmp, void *stream);
int ftx_spconv_pairs_gemm_scatter_split(const float *A, int64_t rows_a, const int32_t *gather, const int32_t *scatter, const float *W, int32_t w_transposed, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t co, int32_t kvol, float *out, int64_t rows_out, void *stream);
int ftx_rows_gemm_split(const float *A, int64_t n, const float *W, int32_t w_transposed, const float *bias, int32_t ca, int32_t co, float *out, void *stream);
size_t ftx_spconv_pairs_wgrad_split_workspace_bytes(int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol);
int ftx_spconv_pairs_wgrad_split(const float *A, int64_t rows_a, const int32_t *idx_a, const float *G, int64_t rows_g, const int32_t *idx_g, const int32_t *koff, int64_t n_pairs, int32_t ca, int32_t cg, int32_t kvol, float *dW, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only queries, as ftx_spconv_gemm_block_cols / ftx_spconv_wgrad_table_blocks, for the split kernels' own tilings. */
int32_t ftx_spconv_gemm_split_block_cols(int32_t co, int64_t n_pairs, int32_t kvol);
int32_t ftx_spconv_wgrad_split_table_blocks(int32_t mi, int32_t wmg, int32_t ni, int32_t wng);

/* ---- BatchNorm1d over rows (+residual, +ReLU): spnn.BatchNorm / nn.BatchNorm1d
 *      models/spvcnn.py:30-31,71-79,100-102,164-180; models/middle_fusion.py:18-22 */

/* Training forward: batch statistics over the n rows (biased var for
 * normalisation, unbiased for running_var, momentum as torch), then
 * y = relu?( (x-mean)*invstd*gamma + beta (+ residual) ).
 * save_mean / save_invstd (c) are outputs for the backward.
 * running_mean / running_var may be NULL (no update).  residual may be NULL. */
size_t ftx_bn_workspace_bytes(int64_t n, int32_t c);
int ftx_bn_train_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean, float *running_var, float momentum, float eps, int64_t n, int32_t c, int32_t relu, float *y, float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes, void *stream);
/* Training-mode BatchNorm forward from the column totals (2, c) float64 that ftx_spconv_reduce_stats left: one launch that
 * derives mean / invstd, updates the running statistics, stores save_mean / save_invstd and applies. */
int ftx_bn_train_fwd_totals(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean, float *running_var, float momentum, float eps, int64_t n, int32_t c, int32_t relu, float *y, float *save_mean, float *save_invstd, const double *totals, void *stream);

/* Eval forward with running statistics. */
int ftx_bn_eval_fwd(const float *x, const float *residual, const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps, int64_t n, int32_t c, int32_t relu, float *y, void *stream);
/* Training backward.  ReLU mask (relu != 0): when the forward had NO residual (grad_residual == NULL) and `beta` is given, the forward
 * output is RECOMPUTED from x -- bit for bit the value the forward wrote -- and y is not read (it may be NULL): a third of this pass's
 * traffic; otherwise y, the forward output, supplies the mask.
 * grad_x (n,c), grad_residual (n,c, may be NULL), grad_gamma (c), grad_beta (c). */
int ftx_bn_train_bwd(const float *grad_y, const float *x, const float *y, const float *gamma, const float *beta, const float *save_mean, const float *save_invstd, int64_t n, int32_t c, int32_t relu, float *grad_x, float *grad_residual, float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes, void *stream);

/* ---- optimizer step: torch.optim.Adam (L2 weight decay, no amsgrad) over every parameter tensor in one launch ----
 * (common/solver/build.py:7-20 builds the optimizer, modules/SemanticTrainer.py:141-209 steps it once per batch.)
 * table: n_tensors records of ftx_adam_tensor_bytes() bytes in DEVICE memory, little-endian, in this order:
 *   float *param; float *exp_avg; float *exp_avg_sq; const float *grad (NULL: tensor skipped this step); int64 numel;
 *   float step_size = lr / (1 - beta1^t); float inv_bc2_sqrt = 1 / sqrt(1 - beta2^t).
 * chunk_tensor / chunk_offset (n_chunks, device): chunk c covers elements [offset, offset + ftx_adam_chunk_elements()) of tensor
 * chunk_tensor[c].  Update per element: g += wd*p; m += (1-beta1)*(g-m); v = beta2*v + (1-beta2)*g*g;
 * p -= step_size * m / (sqrt(v) * inv_bc2_sqrt + eps).  beta1 / beta2 are doubles: 1 - beta is formed in double and then rounded, as torch does. */
int32_t ftx_adam_chunk_elements(void);
int32_t ftx_adam_tensor_bytes(void);
int ftx_adam_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double beta1, double beta2, float eps, float weight_decay, void *stream);

/* ---- the rest of the solver: AdamW, SGD and max-norm gradient clipping, over the same table and chunk map ----
 * Every entry below reads records of ftx_adam_tensor_bytes() bytes and the chunk_tensor / chunk_offset map of ftx_adam_step; a record
 * whose grad is NULL is skipped by the update rules and counts as zeros in the norm.
 *
 * grad_scale (device, one float, may be NULL): every gradient element is replaced by g * *grad_scale (one rounding) before anything
 * else.  NULL, or a device 1.0f, leaves the bits of the unscaled entry.  It is read on the device by the launch itself: pass
 * out + 1 of ftx_grad_norm_finalize and no value crosses to the host between the norm and the update.  The gradients in memory
 * are NOT rewritten.
 *
 * ftx_adam_step_scaled: ftx_adam_step with grad_scale.
 * ftx_adamw_step: torch.optim.AdamW.  Same record as Adam; per element p *= (float)(1 - lr * weight_decay) (formed in double), then
 *   Adam's update without the L2 term.  step_size in the record already holds lr / (1 - beta1^t); lr is passed for the decay alone.
 * ftx_sgd_step: torch.optim.SGD.  The record's fields are read as
 *   float *param; float *momentum_buffer (NULL when momentum == 0); void *unused; const float *grad; int64 numel; int32 first; int32 pad.
 *   g += wd*p; buf = first ? g : momentum*buf + (1 - dampening)*g; g = nesterov ? g + momentum*buf : buf; p -= lr*g.
 *   first != 0 marks a tensor's first step WITH a gradient: the buffer is written and not read (it may be uninitialised).  The caller
 *   keeps `first` set for a tensor until a step in which it had a gradient.  momentum == 0 reads and writes no buffer.  With
 *   momentum != 0 a record whose buffer is NULL is skipped.  nesterov needs momentum > 0 and dampening == 0, as in torch.
 *
 * ftx_grad_sumsq: partial[c] (n_chunks float64, every element written by every launch) = the sum of the squares of chunk c's gradient
 *   elements, each squared and accumulated in float64 in an order that depends on (chunk offset, position in the chunk) only -- not
 *   on the gradient's alignment; 0.0 for a chunk of a tensor without a gradient.  Several tables (parameter groups) write consecutive
 *   ranges of one partial buffer.  No atomics: two launches on the same input give the same bits.
 * ftx_grad_norm_finalize: one block sums the partials in float64 in an order fixed by n_partials and writes two floats:
 *   out[0] = (float)sqrt(total), out[1] = min(1, max_norm / (out[0] + 1e-6f)) in float32 -- torch.nn.utils.clip_grad_norm_ with
 *   error_if_nonfinite=False: a NaN norm gives a NaN coefficient, an infinite norm 0.  n_partials == 0: (0, 1).  max_norm > 0. */
int ftx_adam_step_scaled(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double beta1, double beta2, float eps, float weight_decay, const float *grad_scale, void *stream);
int ftx_adamw_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double beta1, double beta2, float eps, double lr, double weight_decay, const float *grad_scale, void *stream);
int ftx_sgd_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double lr, double momentum, double dampening, double weight_decay, int32_t nesterov, const float *grad_scale, void *stream);
int ftx_grad_sumsq(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double *partial, void *stream);
int ftx_grad_norm_finalize(const double *partial, int64_t n_partials, float max_norm, float *out, void *stream);

/* ---- LayerNorm of the ViT blocks, fused with the residual add in front of it (timm Block.forward: models/transformers.py:16-45) ----
 * forward: s = x + y (y may be NULL: then s_out is not written and s = x), h = (s - mean) * rstd * gamma + beta over rows of c floats,
 * c in {256, 512, 768, 1024}; mean / rstd (rows) are outputs for the backward.  y_bias (c, may be NULL): y is the output of a Linear
 * computed WITHOUT its bias, s = x + (y + y_bias) -- the rounding order of the GEMM's own bias epilogue. */
int ftx_add_layernorm_fwd(const float *x, const float *y, const float *y_bias, const float *gamma, const float *beta, float eps, int64_t rows, int32_t c, float *s_out, float *h_out, float *mean, float *rstd, void *stream);
/* backward: grad_x (rows, c) = grad_s (may be NULL) + d h / d s applied to grad_h -- the gradient of BOTH x and y;
 * grad_params (2 or 3, c) = d gamma, d beta and, with_y_bias != 0, d y_bias = the column sums of grad_x (float64 accumulation, fixed order). */
size_t ftx_layernorm_bwd_workspace_bytes(int64_t rows, int32_t c);
int ftx_add_layernorm_bwd(const float *grad_h, const float *grad_s, const float *s, const float *gamma, const float *mean, const float *rstd, int64_t rows, int32_t c, int32_t with_y_bias, float *grad_x, float *grad_params, void *workspace, size_t workspace_bytes, void *stream);

/* Column sums of a row-major (rows, cols) float32 matrix, float64 accumulation in a fixed order: out (cols).  The bias gradient of
 * the Linear layers (the reference leaves it to autograd's sum_to: models/transformers.py:16-45, spvcnn.py:164-180).  cols % 4 == 0. */
size_t ftx_colsum_workspace_bytes(int64_t rows, int32_t cols);
int ftx_colsum(const float *x, int64_t rows, int32_t cols, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- ViT self-attention (timm Attention.forward): models/transformers.py:36-37 ----
 * Fused softmax(Q K^T * scale) V on exact-fp32 MFMA; the (t, t) score matrix is never stored. */

/* qkv (b, t, 3, h, d) float32 exactly as the fused qkv Linear produces it; out (b, t, h*d);
 * lse (b, h, t) float32 = ln sum_k exp(scale * q.k), saved for the backward.  d must be 64. */
int ftx_attn_fwd(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, void *stream);
/* grad_qkv (b, t, 3, h, d) fully written.  workspace: ftx_attn_bwd_workspace_bytes(b, t, h).
 * Precision: the backward does not keep P; it recomputes P = exp2(S' - lse * log2(e)) from the saved lse, with S' a differently rounded
 * product than the forward's (scale * log2(e) is folded into K for dK / dV, into Q for the forward and dQ).  The exponent is a difference of
 * two numbers of size |lse| * log2(e), each rounded in fp32, so the relative error of P, and through it of dV, dK and dQ, grows as about
 * u * |lse| (u = 2^-24; at most 4 u |lse| by count of the roundings: tests/attn_ref.py).  Measured on an MI355X with scores around +-7000
 * (max |lse| 4100, 100 tokens): dV within 3.5e-4 of float64, relative to max |dV|, where the unfused fp32 formula is within 2.3e-5; out, lse,
 * dQ and dK stay within about 2x of the unfused formula there.  At the ViT's |lse| < 50 the term is below 1.2e-5 and dV is within 2.8e-6. */
size_t ftx_attn_bwd_workspace_bytes(int32_t b, int32_t t, int32_t h);
int ftx_attn_bwd(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, void *stream);
/* The same two calls with an explicit tiling of the three attention kernels: qw waves of 32 queries (keys) per block x split key (query)
 * groups.  (0, 0) = chosen per launch from b*h*ceil(t/32) (what ftx_attn_fwd / ftx_attn_bwd do); built: (4,2) (2,2) (2,4) (1,2) (1,4) (1,8);
 * anything else is refused.  A per-call argument, not a process-wide switch.  A measurement / test aid: results of different tilings
 * differ in the last bits (the key range is summed in a different grouping), never with timing. */
int ftx_attn_fwd_tiled(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw, int32_t split, void *stream);
int ftx_attn_bwd_tiled(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split, void *stream);
/* bf16-operand attention: the same calls on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (models/transformers.py attn_impl "ftx_bf16").
 * Storage stays fp32: qkv, out, lse, grad_out, grad_qkv as above.  Q, K, V and dO are rounded to bf16 (round-to-nearest-even) from
 * their stored values; scale is applied in fp32 to the fp32 score; the softmax max, row sum and lse use the unrounded fp32 exponentials,
 * so lse is the fp32-accurate log-sum-exp of the bf16-operand scores; P is rounded to bf16 only as the P.V operand.  Backward: P
 * recomputed from lse, dP = dO V^T on bf16 operands, delta = rowsum(bf16(dO) * O) in fp32, dS rounded to bf16 only as the dK / dQ operand,
 * every gradient accumulated and written in fp32.  No atomics: deterministic for a given tiling.  Tilings as ftx_attn_fwd_tiled
 * ((0, 0) = chosen per launch; built (4,2) (2,2) (2,4) (1,2) (1,4) (1,8); anything else refused).  workspace: ftx_attn_bwd_workspace_bytes. */
int ftx_attn_fwd_bf16(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw, int32_t split, void *stream);
int ftx_attn_bwd_bf16(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split, void *stream);
/* fp32-accurate attention on the bf16 MFMA: the same calls once more (models/transformers.py attn_impl "ftx_split").
 * Precision contract.  Storage stays fp32: qkv, out, lse, grad_out, grad_qkv as above.  Every MFMA operand is split into three bf16
 * pieces, x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m) (round-to-nearest-even, the subtractions in fp32): Q, K,
 * V and dO from their stored values, and the accumulator tiles that are operands -- P in the forward and the dK / dV pass, dS in the dK /
 * dV and dQ passes -- from their fp32 registers; nothing is rounded to a single bf16.  Every product is the six piece products mm, hl, lh,
 * hm, mh, hh (first letter: the staged tile's piece) on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, in that order per 16-wide step of
 * the reduction.  Grouping: per product of one staged 32-token tile (32 x 32 x 64 for the scores and dP, 32 x 32 x 32 for P.V, dV, dK and dQ)
 * the five corrections run in an accumulator of their own that starts at zero, hh runs in the product's accumulator, and the corrections
 * are added to it once when that tile's product ends.  scale * log2(e) multiplies the fp32 score; it is not folded into an operand.  dO is
 * exact everywhere: delta = rowsum(dO * O) in fp32, the fp32 kernels' delta.  Softmax max, row sum, lse, rescale and the P rebuilt from lse
 * are fp32, as in the other two families.  No atomics: deterministic for a given tiling.  Meets the bars of the fp32 kernels
 * (tests/attn_ref.py); the terms it leaves out (ll, ml, lm) are below 2^-24 of a product.
 * Tilings: (0, 0) = chosen per launch by the family's own rule; ftx_attn_split_tiling_built(qw, split, backward) != 0 says whether an
 * explicit (qw, split) is built for the forward (backward == 0) or the backward (the set is a subset of the six of ftx_attn_fwd_tiled and
 * holds (4,2)); anything else is refused.  workspace: ftx_attn_bwd_workspace_bytes. */
int32_t ftx_attn_split_tiling_built(int32_t qw, int32_t split, int32_t backward);
int ftx_attn_fwd_split(const float *qkv, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *out, float *lse, int32_t qw, int32_t split, void *stream);
int ftx_attn_bwd_split(const float *qkv, const float *out, const float *grad_out, const float *lse, int32_t b, int32_t t, int32_t h, int32_t d, float scale, float *grad_qkv, void *workspace, size_t workspace_bytes, int32_t qw, int32_t split, void *stream);

/* ---- bf16-operand ViT Linears (timm Mlp / Attention qkv, proj, fc1, fc2: models/transformers.py:36-55) (csrc/ftx_dense_bf16.hip: the
 *      family's description and entries; the kernels, shared with the split entries below: csrc/ftx_dense_common.h) ----
 * Precision contract: the MFMA operands -- A and W of the GEMM, dY and X of the weight gradient -- are rounded to bf16
 * (round-to-nearest-even) from their stored fp32 values as they are staged; nothing else is rounded.  Accumulation is fp32
 * (v_mfma_f32_32x32x16_bf16), and all storage stays fp32: A, W, bias, out, pre_in / pre_out and dW.  Bias, GELU and the GELU
 * derivative are applied in fp32 to the fp32 sum.  No atomics: results are deterministic, the split weight gradient's partials are
 * added in a fixed order, and tiles, splits and workspace sizes are functions of the arguments alone.
 *
 * GEMM: out (m, n) = epilogue(A (m, k) . B), B = W^T with W (n, k) as nn.Linear stores it (w_kn = 0, the forward) or B = W with W
 * stored (k, n) (w_kn = 1, the data gradient dX = dY W).  k % 64 == 0, n % 4 == 0, every pointer 16-byte aligned.  Epilogues:
 *   FTX_EPI_NONE       out = sum
 *   FTX_EPI_BIAS       out = sum + bias (n)
 *   FTX_EPI_BIAS_GELU  pre_out = sum + bias, out = gelu(pre_out) (exact erf GELU, nn.GELU())
 *   FTX_EPI_DGELU      out = sum * gelu'(pre_in), pre_in (m, n) the saved pre-activation: fc1's output gradient straight from fc2's dX
 * Pointers an epilogue does not use are ignored.  m == 0 returns FTX_OK without launching. */
#define FTX_EPI_NONE 0
#define FTX_EPI_BIAS 1
#define FTX_EPI_BIAS_GELU 2
#define FTX_EPI_DGELU 3
int ftx_dense_gemm_bf16(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n, int32_t k, int32_t epilogue, float *out, float *pre_out, void *stream);
/* Weight gradient: dW (n, k) = dY^T X over the m rows of dY (m, n) and X (m, k); n % 4 == 0, k % 4 == 0.  m == 0 zeroes dW.  The
 * rows are split for small tile counts (ftx_dense_bf16_tile); workspace: ftx_dense_wgrad_bf16_workspace_bytes(m, n, k). */
size_t ftx_dense_wgrad_bf16_workspace_bytes(int64_t m, int32_t n, int32_t k);
int ftx_dense_wgrad_bf16(const float *dY, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: the tile (rows x columns of the output) and the row split a launch of `form` (0: GEMM, out (m, n); 1: weight gradient,
 * dW (n, k) over m rows) picks.  Launches nothing. */
int ftx_dense_bf16_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host);

/* ---- fp32-accurate ViT Linears on the bf16 MFMA: three-piece operand split (csrc/ftx_dense_split.hip: the family's
 *      description and entries; the kernels: csrc/ftx_dense_common.h) ----
 * The same GEMM, epilogues, weight gradient, argument rules, error texts and m == 0 behaviour as the bf16-operand entries above, for
 * the fp32 model: no operand bit is discarded below the stated range, and the result is fp32-class (measured: DESIGN section 5).
 * Precision contract:
 *   split     every fp32 operand element x (A, W; dY, X) is split as it is staged, round-to-nearest-even, both subtractions in fp32
 *             (they are exact):  h = bf16(x),  m = bf16(x - h),  l = bf16((x - h) - m).
 *             For finite x with |x| < 2^127 (above it h rounds to inf) x == h + m + l exactly (24 significand bits into 3 x 8), except
 *             that pieces below 2^-126 may be lost.  If h is not finite, m = l = 0: inf and NaN propagate as through an fp32 GEMM,
 *             i.e. to the same output elements, NaN as NaN; an inf may arrive as NaN instead (inf times a zero piece of the
 *             other operand).
 *   products  six of the nine piece products are summed, fp32 accumulation on v_mfma_f32_32x32x16_bf16: hh, hm, mh, hl, lh, mm (first
 *             letter: the piece of A / dY).  Each bf16 x bf16 product is exact in fp32.  The dropped ml, lm, ll are each below
 *             2.01 * 2^-24 * |a b|.
 *   order     fixed: two fp32 accumulators per output element.  One takes the hh products, reduction index ascending.  The other
 *             takes, per 16-wide reduction step, mm, hl, lh, hm, mh in that order (smallest first).  They are added once, in the
 *             epilogue: sum = hh + corrections.  No atomics; a split weight gradient's partials are added in split order.  Results
 *             are bit-reproducible and a function of the arguments alone.
 *   storage   A, W, bias, out, pre_in / pre_out, dW: fp32.  Bias, GELU and the GELU derivative are applied in fp32 to the fp32 sum by
 *             the bf16 entries' epilogue code.
 * ftx_dense_split_tile: as ftx_dense_bf16_tile for these entries (form 0: GEMM, 1: weight gradient).  Host only. */
int ftx_dense_gemm_split(const float *A, const float *W, int32_t w_kn, const float *bias, const float *pre_in, int64_t m, int32_t n, int32_t k, int32_t epilogue, float *out, float *pre_out, void *stream);
size_t ftx_dense_wgrad_split_workspace_bytes(int64_t m, int32_t n, int32_t k);
int ftx_dense_wgrad_split(const float *dY, const float *X, int64_t m, int32_t n, int32_t k, float *dW, void *workspace, size_t workspace_bytes, void *stream);
int ftx_dense_split_tile(int32_t form, int64_t m, int32_t n, int32_t k, int32_t *tile_m_host, int32_t *tile_n_host, int32_t *split_host);

/* ---- fused train-step losses + metric: modules/SemanticTrainer.py:158-194, models/metric.py:37-58 ----
 * losses[0] = loss_2d = CE_w(img_logit) + lambda * KL(softmax(lidar_logit) || softmax(img_logit2))
 * losses[1] = loss_3d = CE_w(lidar_logit) + lambda * KL(softmax(img_logit) || softmax(lidar_logit2))
 * (weighted-mean CE with class_weights (c) or NULL = ones; KL summed over classes, mean over points;
 * second heads NULL = single head, the KL terms then use the main heads, SemanticTrainer.py:164-165).
 * grad_* (n,c) receive d(loss_2d + loss_3d)/d(logits), fully written.  conf3d / conf2d (c,c) int64 are
 * ACCUMULATED: conf[label, argmax] += 1 for label != ignore_index (NULL = no metric).  c % 4 == 0, c <= 32. */
size_t ftx_fusion_loss_workspace_bytes(void);
/* The same with an explicit mix: loss = ce_scale * CE_w + lambda * KL.  ce_scale = 1 is the additive form of SemanticTrainer.py:158-178
 * (ftx_fusion_loss); ce_scale = 1 - lambda is the torchpack / DDP trainer's mix (modules/SemanticTorchpackTrainer.py:70-106). */
int ftx_fusion_loss_mix(const float *lidar_logit, const float *img_logit, const float *lidar_logit2, const float *img_logit2, const int64_t *label, const float *class_weights, float ce_scale, float lambda_xm, int64_t n, int32_t c, int32_t ignore_index, float *losses, float *grad_lidar, float *grad_img, float *grad_lidar2, float *grad_img2, int64_t *conf3d, int64_t *conf2d, void *workspace, size_t workspace_bytes, void *stream);
int ftx_fusion_loss(const float *lidar_logit, const float *img_logit, const float *lidar_logit2, const float *img_logit2, const int64_t *label, const float *class_weights, float lambda_xm, int64_t n, int32_t c, int32_t ignore_index, float *losses, float *grad_lidar, float *grad_img, float *grad_lidar2, float *grad_img2, int64_t *conf3d, int64_t *conf2d, void *workspace, size_t workspace_bytes, void *stream);

/* ---- one-head segmentation loss + metric: the LiDAR-only / image-only branches of modules/SemanticTrainer.py:180-186 and the
 * per-batch validation loss of data/utils/validate.py:122-128 ----
 * loss[0] = CE_w(logit, label): the weighted-mean cross-entropy term of ftx_fusion_loss, same conventions: class_weights (c) or
 * NULL = ones; a label outside [0, c) has weight 0 and is not counted; NaN when the total weight is 0.
 * grad (n,c) receives d loss / d logit = w/W * (softmax - onehot), fully written; grad = NULL selects a forward-only kernel that
 * contains no gradient stores.  conf (c,c) int64 is ACCUMULATED: conf[label, argmax] += 1 for valid labels other than
 * ignore_index, first maximum wins (NULL = no metric).  c % 4 == 0, 4 <= c <= 32, n >= 1.  Three launches, no host
 * synchronisation, no floating-point atomics: two calls on the same inputs give the same bits, and the same bits as
 * ftx_fusion_loss_mix gives for that head at lambda_xm = 0. */
size_t ftx_seg_loss_workspace_bytes(void);
int ftx_seg_loss(const float *logit, const int64_t *label, const float *class_weights, int64_t n, int32_t c, int32_t ignore_index, float *loss, float *grad, int64_t *conf, void *workspace, size_t workspace_bytes, void *stream);

/* ---- evaluation scatter-back: data/utils/validate.py:62-120 + data/utils/evaluate.py:12-26 ----
 * For every ORIGINAL point i (m of them, all frames of the batch concatenated): r = inverse[i] is the row of the
 * model point (voxel) it was quantised into (inverse_map of its frame + the frame's row offset, map_sparse_to_org);
 * pred_3d = argmax(logits3d[r]), pred_2d = argmax(logits2d[r]), pred_ens = argmax(softmax(logits2d[r]) +
 * softmax(logits3d[r])) (first maximum wins); predictions are written as ORIGINAL label ids class_labels[pred]
 * (map_inverse_label).  gt (m) holds learning ids; as in Evaluator.update an original id 0 is replaced by
 * num_classes, and a point only counts if that id occurs in class_labels.  conf_* (c,c) int64 are ACCUMULATED:
 * conf[index of gt id][index of pred id] += 1.  Either logits pointer, any pred_* / conf_* pointer may be NULL.
 * *bad_flag is set to 1 if an inverse index or a gt id is out of range (those points are skipped). c <= 32. */
int ftx_eval_scatter_back(const float *logits3d, const float *logits2d, int64_t n_rows, int32_t num_classes, const int64_t *inverse, const int32_t *gt, int64_t m, const int32_t *class_labels, int32_t *pred3d, int32_t *pred2d, int32_t *pred_ens, int64_t *conf3d, int64_t *conf2d, int64_t *conf_ens, int32_t *bad_flag, void *stream);

/* ---- offline LiDAR -> image projection: data/semantic_kitti/preprocess.py:108-116 ----
 * points (n,3) float32 in the LiDAR frame, proj_matrix (3,4) float32 = P2 * Tr (preprocess.py:32-33).
 * keep[i] = 1 iff x > 0 and 0 < u < width and 0 < v < height (select_points_in_frustum, preprocess.py:75-91);
 * rowcol (n,2) = (v, u) for EVERY point (the caller compacts with keep), i.e. the reference's fliplr(img_points). */
int ftx_project_points(const float *points, int64_t n, const float *proj_matrix, int32_t width, int32_t height, uint8_t *keep, float *rowcol, void *stream);

/* ---- colour jitter of the image-side augmentation: data/semantic_kitti/semantic_kitti_dataloader.py:117,146,196-212 ----
 * T.ColorJitter on the cropped PIL image, then np.array(image, float32) / 255, the optional left-right flip, (x - mean) / std and
 * HWC -> CHW.  src: one uint8 RGB frame, `height` rows of `width` pixels, row r at src + r * pitch (pitch >= 3 * width bytes, any
 * byte offset: a crop view needs no copy); channels must be 3.  ops_host / factors_host (n_ops <= 4, each op at most once) are the
 * draws in application order (torchvision's fn_idx order), host arrays:
 *   FTX_JITTER_BRIGHTNESS f >= 0  ImageEnhance.Brightness(img).enhance(f)
 *   FTX_JITTER_CONTRAST   f >= 0  ImageEnhance.Contrast(img).enhance(f): grey = int(mean luma of the image at that point + 0.5)
 *   FTX_JITTER_SATURATION f >= 0  ImageEnhance.Color(img).enhance(f)
 *   FTX_JITTER_HUE  -0.5 <= f <= 0.5  torchvision adjust_hue: HSV round trip, uint8 hue + (int(f * 255) mod 256)
 * PRECISION: bit-exact with Pillow's uint8 arithmetic (blend in float32 without fused multiply-adds, convert("L"), the HSV
 * conversions of libImaging/Convert.c); the float output is float32(u8) / 255 correctly rounded, then (x - mean) / std rounded twice.
 * workspace: caller-owned, 16-byte aligned, ftx_color_jitter_workspace_bytes(height, width) bytes; only read when a contrast op is
 * present (NULL allowed otherwise).  One launch, or two with a contrast op; no host synchronisation. */
#define FTX_JITTER_BRIGHTNESS 0
#define FTX_JITTER_CONTRAST 1
#define FTX_JITTER_SATURATION 2
#define FTX_JITTER_HUE 3
size_t ftx_color_jitter_workspace_bytes(int32_t height, int32_t width);
/* dst (height, width, 3) uint8, contiguous: the jittered frame. */
int ftx_color_jitter_u8(const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops_host, const double *factors_host, int32_t n_ops, uint8_t *dst, void *workspace, size_t workspace_bytes, void *stream);
/* dst (3, height, width) float32, contiguous: the jittered frame as the model's input; flip != 0 mirrors the columns;
 * mean_host / std_host (3 floats each) both NULL = no normalisation. */
int ftx_color_jitter_chw(const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops_host, const double *factors_host, int32_t n_ops, int32_t flip, const float *mean_host, const float *std_host, float *dst, void *workspace, size_t workspace_bytes, void *stream);

/* ---- image resize of the NuScenes loader: data/nuscenes/nuscenes_dataloader.py:185, image.resize(size, Image.BILINEAR) ----
 * PRECISION: bit-exact with Pillow's 8bpc bilinear resample (libImaging/Resample.c), which is integer arithmetic on a table that is
 * built in double.  For one axis of input length `in` and output length `out`, over the whole axis, all in C double:
 *   scale = filterscale = in / out;  if (filterscale < 1.0) filterscale = 1.0;  support = 1.0 * filterscale;
 *   ksize = (int)ceil(support) * 2 + 1
 *   for xx in 0..out-1:
 *     center = (xx + 0.5) * scale
 *     xmin = (int)(center - support + 0.5), at least 0;  xmax = (int)(center + support + 0.5), at most in;  taps = xmax - xmin
 *     k[x] = tri((x + xmin - center + 0.5) * (1.0 / filterscale)) for x < taps, each divided by their sum if that is not 0; 0 up to ksize
 *     kk[x] = (int)(k[x] < 0 ? -0.5 + k[x] * (1 << 22) : 0.5 + k[x] * (1 << 22))
 *   tri(a) = |a| < 1.0 ? 1.0 - |a| : 0.0;  the (int) casts truncate toward zero; 1.0 / filterscale is formed once and multiplied.
 * A pass over one axis: acc = (1 << 21) + sum_x src[xmin + x] * kk[x] in 32-bit integers per channel, result clip8(acc >> 22)
 * (arithmetic shift, clamped to 0..255).  The horizontal pass runs first and rounds and clamps to uint8; the vertical pass works
 * on those bytes.  A pass whose axis keeps its length is not run.
 * ftx_resize_ksize / ftx_resize_coeffs_host are host code and need no GPU: bounds_host (out, 2) int32 = (xmin, taps) per output
 * index, kk_host (out, ksize) int32.  They answer -1 for in <= 0, out <= 0 or a null pointer.
 * ftx_resize_bilinear_u8: n_frames equal-sized RGB frames, frame f at src + f * frame_stride, row r at + r * pitch (pitch >= 3 * in_w
 * bytes, any byte offset: a crop view needs no copy); channels must be 3.  bounds_x / kk_x / ksize_x are the table of (in_w, out_w),
 * bounds_y / kk_y / ksize_y that of (in_h, out_h), DEVICE pointers; the table of an axis that keeps its length is not read (NULL
 * allowed).  Equal sizes on both axes are refused: there is nothing to resample.  dst (n_frames, out_h, out_w, 3) uint8, contiguous.
 * Both directions (shrinking and enlarging) are supported.  workspace: caller-owned, 16-byte aligned,
 * ftx_resize_workspace_bytes(...) bytes (the uint8 intermediate; 0 when only one axis changes, NULL allowed then).  One launch per
 * axis that changes, for all frames; no atomics, no host synchronisation, capturable. */
int32_t ftx_resize_ksize(int32_t in, int32_t out);
int ftx_resize_coeffs_host(int32_t in, int32_t out, int32_t *bounds_host, int32_t *kk_host);
size_t ftx_resize_workspace_bytes(int32_t n_frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w);
int ftx_resize_bilinear_u8(const uint8_t *src, int64_t frame_stride, int64_t pitch, int32_t n_frames, int32_t in_h, int32_t in_w, int32_t channels, const int32_t *bounds_x, const int32_t *kk_x, int32_t ksize_x, const int32_t *bounds_y, const int32_t *kk_y, int32_t ksize_y, int32_t out_h, int32_t out_w, uint8_t *dst, void *workspace, size_t workspace_bytes, void *stream);

/* ---- native eval-mode executor of the SPVCNN LiDAR branch (models/spvcnn.py:191-233 under model.eval(), no gradients) ----
 * ftx_spvcnn_eval issues the forward of one SPVCNN from the first convolution of the stem to the final point features (z3.F) on
 * `stream`: the same per-op entry points, in the same order, as the Python path issues them one by one (ftx_spconv_pairs_gemm /
 * _scatter / ftx_spconv_ostat, ftx_rows_gemm, ftx_bn_eval_fwd, ftx_spconv_reduce_bn_eval, ftx_voxelize_fwd_sorted, ftx_devoxelize_fwd)
 * plus ftx_rows_concat / ftx_rows_add below where that path uses torch.cat and `+`.  The results are bit-identical to that path.
 * Dropout is the identity in eval mode.  Building the coordinate structures of the batch and the segmentation heads stay with the caller.
 *
 * ftx_rows_concat: out (n, ca + cb) = a (n, ca) ++ b (n, cb) per row.  ftx_rows_add: out = a + b over (n, c), one fp32 add per element;
 * out may alias a or b.  Channels multiples of 4, 16-byte accesses, n = 0 is a no-op.
 *
 * Tables.  All four are arrays of packed little-endian records in HOST memory (the pointers inside them are device pointers); the
 * library reports each record size (ftx_spvcnn_*_bytes) so a binding can assert its layout.
 *   layer (model table; built once per model, rebuilt when a parameter moves):
 *     const float *weight  Conv3d kernel (kvol, ca, co), (ca, co) for kvol = 1; nn.Linear weight (co, ca)
 *     const float *bias    nn.Linear bias (co) or NULL; NULL for a convolution
 *     const float *gamma, *beta, *running_mean, *running_var   the BatchNorm behind the layer, (co) each
 *     int32 ca, co, kvol (1, 8 or 27; 0 for a Linear), stride, transposed, bf16;  float eps;  int32 kind (FTX_SPVCNN_LAYER_*)
 *     bf16 is the layer's operand mode, 0, 1 or 2 (anything else is FTX_EINVAL with the layer named).  1: the layer's GEMM runs on the
 *     bf16-operand entry points (ftx_spconv_pairs_gemm_bf16 / _scatter_bf16, ftx_rows_gemm_bf16), as SPVCNN.set_bf16 makes the Python
 *     path do.  2: on the three-piece split entry points (ftx_spconv_pairs_gemm_split / _scatter_split, ftx_rows_gemm_split, in
 *     training ftx_spconv_pairs_wgrad_split), as SPVCNN.set_split does; the output-stationary route is exact fp32, which meets the
 *     split mode's fp32-class contract, so a mode-2 layer may take it wherever a mode-0 layer may (a mode-1 layer never).  The mode is
 *     honoured here, nothing falls back.
 *   op (the static program of the network, emitted once per model by the host; fusiontransformer_amd/native_eval.py emits SPVCNN's):
 *     int32 kind (FTX_SPVCNN_OP_*), segment (0 stem, 1 encoder, 2 decoder; ascending), layer (index into the model table; for ADD_EXT
 *     0 = the early-fusion addend, 1 = the middle-fusion addend), map (index into the kernel maps for CONV_BN with kvol > 1, into the
 *     point-voxel indices for VOXELIZE / DEVOXELIZE, else -1), src, src2 (second operand of CONCAT / ADD, residual of CONV_BN or -1),
 *     dst, relu, level (whose rows dst has: 0..4 the voxel levels of stride 1, 2, 4, 8, 16; 5 the points), channels (of dst), 2 x reserved.
 *     src / src2 / dst number buffers ("slots"): FTX_SPVCNN_SLOT_INPUT is x0 (the voxelised input features, rows[0] rows),
 *     FTX_SPVCNN_SLOT_OUTPUT is `out` (rows[5] rows), slots from FTX_SPVCNN_SLOT_FIRST up to 255 live in the arena.  Every slot is written
 *     by exactly one op before it is read (ADD_EXT alone works in place).
 *   map (batch table, one per kernel map): const int32 *nbr, *pos, *pos_t, *pair_in, *pair_out, *koff; int64 n_pairs, n_in, n_out;
 *     int32 kvol, fine_bijective -- the arrays ftx_kernel_map_build / _count / _pairs produce.
 *   pv (batch table, one per stride at which points and voxels exchange features): const int32 *vox_idx (n), *vox_counts (n_vox),
 *     *vox_order (n), *vox_seg_off (n_vox + 1) [ftx_segment_build / ftx_level_segments]; const int32 *devox_idx (n, 8);
 *     const float *devox_weights (n, 8) [ftx_kernel_map_build transposed, ftx_trilinear_weights]; int64 n_vox; int32 level, reserved.
 *   rows_host: int64[6], the rows of the five levels and of the point set.
 *   routes_host: int32[n_ops], for every CONV_BN / LINEAR_BN op how its GEMM runs (FTX_SPVCNN_ROUTE_*): chosen by the CALLER (the host's
 *     one routing rule, functional._conv_route).  The library obeys and has no rule of its own; a route an op cannot take (the direct
 *     route on a map that is not a bijection, the output-stationary route on a layer ftx_spconv_ostat_supported refuses, the empty
 *     route on a map with pairs, anything but ROWS on a dense layer) is FTX_EINVAL.
 * Segments.  A call runs the ops of segments [first_segment, last_segment]: 0 = the stem up to z0, 1 = stage1..stage4, point
 * transform 0, z1, 2 = up1..up4, point transforms 1 and 2, z3.  Slots keep their place in the arena between the calls of one forward,
 * so a fusion model runs one call per segment and produces the image-side addend in between: add_early (rows[5], channels of z0) is
 * added to z0 by the ADD_EXT op that opens segment 1, add_middle to z1 by the one that opens segment 2; NULL skips the add.
 * Arena.  Every intermediate lives in `arena` (device memory, 256-byte aligned, caller-owned): ftx_spvcnn_eval_arena_bytes is a host
 * function of the tables alone (needs no GPU; 0 and an error text for tables it refuses), a multiple of 256, and never decreases when a
 * row or pair count grows.  Buffers whose last reader has run are reused.  An arena that is too small is FTX_EWORKSPACE.
 * Every table is validated before the first launch; a failing launch is reported with the op and layer index in ftx_last_error().
 * No host synchronisation, no allocation, no state kept beyond the call. */
#define FTX_SPVCNN_LAYER_CONV_BN 1
#define FTX_SPVCNN_LAYER_LINEAR_BN 2
#define FTX_SPVCNN_OP_CONV_BN 1
#define FTX_SPVCNN_OP_LINEAR_BN 2
#define FTX_SPVCNN_OP_VOXELIZE 3
#define FTX_SPVCNN_OP_DEVOXELIZE 4
#define FTX_SPVCNN_OP_CONCAT 5
#define FTX_SPVCNN_OP_ADD 6
#define FTX_SPVCNN_OP_ADD_EXT 7
#define FTX_SPVCNN_OP_DROPOUT 8 /* the training program's alone, see ftx_spvcnn_train_fwd_rng */
#define FTX_SPVCNN_ROUTE_EMPTY 0
#define FTX_SPVCNN_ROUTE_DIRECT 1
#define FTX_SPVCNN_ROUTE_OSTAT 2
#define FTX_SPVCNN_ROUTE_PAIRS 3
#define FTX_SPVCNN_ROUTE_ROWS 4
#define FTX_SPVCNN_SLOT_INPUT 0
#define FTX_SPVCNN_SLOT_OUTPUT 1
#define FTX_SPVCNN_SLOT_FIRST 2
int ftx_rows_concat(const float *a, int32_t ca, const float *b, int32_t cb, int64_t n, float *out, void *stream);
int ftx_rows_add(const float *a, const float *b, int64_t n, int32_t c, float *out, void *stream);
int32_t ftx_spvcnn_layer_bytes(void);
int32_t ftx_spvcnn_op_bytes(void);
int32_t ftx_spvcnn_map_bytes(void);
int32_t ftx_spvcnn_pv_bytes(void);
size_t ftx_spvcnn_eval_arena_bytes(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host);
int ftx_spvcnn_eval(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const float *x0, int32_t first_segment, int32_t last_segment, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out, void *stream);

/* ---- native training executor of the SPVCNN LiDAR branch (models/spvcnn.py:191-233 under model.train(), gradients enabled) ----
 * ftx_spvcnn_train_fwd issues the train-mode forward of the segments [first_segment, last_segment] of the program ftx_spvcnn_eval
 * takes, ftx_spvcnn_train_bwd their backward: the program in reverse, for every op what its autograd node issues on the per-op path and
 * in that node's order (CONV_BN: ftx_bn_train_bwd, the data gradient, ftx_spconv_pairs_wgrad; dense layers: ftx_bn_train_bwd,
 * ftx_rows_gemm, the dense ftx_spconv_pairs_wgrad, ftx_colsum; ftx_voxelize_bwd, ftx_devoxelize_bwd(_sorted); ftx_rows_split for CONCAT).
 * The forward runs the statistics-producing forms (ftx_spconv_reduce_stats / ftx_spconv_ostat with partials + ftx_bn_train_fwd_totals,
 * else ftx_bn_train_fwd) and updates the running statistics through them.  Results are bit-identical to the per-op path.
 *
 * ftx_rows_split: a (n, ca), b (n, cb) = the two column blocks of in (n, ca + cb), the backward of ftx_rows_concat; channels multiples
 * of 4, 16-byte accesses, n = 0 is a no-op.
 *
 * Tables: layer, op, map, pv, rows_host and routes_host as ftx_spvcnn_eval reads them (records unchanged), except that segments are
 * numbered 0 .. 7 without a gap and every level needs at least one row.  Dropout is either the caller's (a segment ends where one
 * follows, and the caller hands the next segment what its Dropout returned) or an op of the program (FTX_SPVCNN_OP_DROPOUT, below).
 *   grad_routes_host: int32[n_ops], for every CONV_BN op with kvol > 1 whose input needs a gradient how the data gradient runs:
 *     FTX_SPVCNN_ROUTE_EMPTY (zero fill), _DIRECT or _PAIRS, the caller's choice as in routes_host (functional._conv_route(grad=True)).
 *     An op that reads FTX_SPVCNN_SLOT_INPUT computes no data gradient.
 *   train layer (parallel to the model table; ftx_spvcnn_train_layer_bytes): float *dweight, *dbias (NULL without a bias), *dgamma,
 *     *dbeta -- where the backward writes the layer's parameter gradients, in the parameters' shapes; float momentum; int32 reserved.
 *   train pv (parallel to the pv table; ftx_spvcnn_train_pv_bytes): const int32 *devox_order (8 n), *devox_seg_off (n_vox + 1), the sorted
 *     segments of the devoxelise backward [ftx_segment_build]; NULL: ftx_devoxelize_bwd.  A pv record with NULL vox_order runs
 *     ftx_voxelize_fwd.
 * Buffers.  seg_in stands for the input of first_segment: the voxelised features x0 for segment 0, else the buffer the previous
 * segment returned in *seg_out or -- where only first_segment reads it -- a replacement of it (what Dropout returned); the backward
 * of a segment takes the same seg_in as its forward.  *seg_out receives the address of last_segment's result: inside the arena, or
 * `out` (rows[5] x channels, the caller's) for the last segment of the program.  grad_out is the gradient of that result;
 * *grad_in receives the address, inside the arena, of the gradient of seg_in (NULL for segment 0), which is also the gradient of the
 * fusion addend a segment opened with.  A slot read by two ops has its two gradients added by one ftx_rows_add; a program in which a
 * slot would receive more than two, or in which an operand of ADD has another reader, is FTX_EINVAL.
 * Arena.  ftx_spvcnn_train_arena_bytes is a host function of the tables alone with the properties of ftx_spvcnn_eval_arena_bytes.  One
 * region per slot, per slot gradient, per layer output and per layer statistics, none shared, plus one shared region for per-op
 * temporaries: nothing the backward reads is written again while the caller keeps the arena.  The caller keeps it, unchanged, from the
 * first forward call of a step to its last backward call and runs the backward of the segments in descending order.
 * Every table is validated before the first launch.  No host synchronisation, no allocation, no state kept beyond the call; the
 * stream's ticket buffer (ftx_stream_scratch_attach) is the caller's as for the per-op entry points.
 *
 * Dropout as an op.  FTX_SPVCNN_OP_DROPOUT (training program only; ftx_spvcnn_eval refuses it: Dropout is the identity there) works in
 * place on an arena slot that no op has read yet, like ADD_EXT: dst == src, level / channels those of the slot, layer = the site
 * number s >= 0, reserved0 = the IEEE bits of p (0 <= p < 1).  The forward issues ftx_dropout (below) over the slot's rows x channels
 * elements with call = call_base + s and elem0 = 0; the backward issues the same call on the slot's gradient buffer in place, so the op
 * sends no gradient anywhere and adds no region to the arena.  A slot whose gradient is another buffer's (an operand of ADD, the result
 * of a segment) is FTX_EINVAL.  (seed, call_base) are arguments of ftx_spvcnn_train_fwd_rng / ftx_spvcnn_train_bwd_rng, which are
 * otherwise ftx_spvcnn_train_fwd / _bwd; nothing is kept between calls, so the backward is given the pair its forward was given.  The
 * plain entries refuse a program that holds the op before their first launch.  With the op after the two voxelisations that feed
 * SPVCNN's Dropouts the training program runs in the eval program's three segments. */
int ftx_rows_split(const float *in, int64_t n, int32_t ca, int32_t cb, float *a, float *b, void *stream);
int32_t ftx_spvcnn_train_layer_bytes(void);
int32_t ftx_spvcnn_train_pv_bytes(void);
size_t ftx_spvcnn_train_arena_bytes(const void *layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host);
int ftx_spvcnn_train_fwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment, const float *seg_in, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out, float **seg_out, void *stream);
int ftx_spvcnn_train_bwd(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, const void *train_pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in, void *stream);
int ftx_spvcnn_train_fwd_rng(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment, const float *seg_in, const float *add_early, const float *add_middle, void *arena, size_t arena_bytes, float *out, float **seg_out, void *stream, uint64_t seed, uint64_t call_base);
int ftx_spvcnn_train_bwd_rng(const void *layers_host, const void *train_layers_host, int32_t n_layers, const void *ops_host, int32_t n_ops, const int64_t *rows_host, const void *maps_host, int32_t n_maps, const void *pvs_host, const void *train_pvs_host, int32_t n_pvs, const int32_t *routes_host, const int32_t *grad_routes_host, int32_t first_segment, int32_t last_segment, const float *seg_in, const float *grad_out, void *arena, size_t arena_bytes, float **grad_in, void *stream, uint64_t seed, uint64_t call_base);

/* ---- counter-based Dropout ----
 * y[i] = x[i] * (keep(i) ? scale : 0.0f), one fp32 multiply per element: a product, not a select, so NaN or Inf in a dropped element
 * gives NaN, as torch's input * mask * scale does.  The mask is a pure function of (seed, call, logical element index); it does not
 * depend on the launch geometry, on the device or on any library version, and it is never stored: the backward is the same call on
 * the gradient (dx = dy * mask * scale).
 *
 * The random stream (the contract; tests/dropout_ref.py restates it in numpy):
 *   generator  Philox4x32-10: multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), key increments 0x9E3779B9 and
 *              0xBB67AE85, ten rounds, the key bumped between rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3")
 *   key        (seed & 0xffffffff, seed >> 32)
 *   element    g = elem0 + i (uint64, wrapping), i the index into the buffer of this call; block q = g >> 2, lane j = g & 3
 *   counter    (q & 0xffffffff, q >> 32, call & 0xffffffff, call >> 32)
 *   u          word j of the ten-round output
 *   threshold  thr = (uint32) floor((double) p * 2^32), scale = (float) (1.0 / (1.0 - (double) p)), both computed on the host
 *   rule       keep iff u >= thr; p = 0 keeps everything with scale 1 and returns x bit for bit
 * elem0 lets a tensor that is processed in pieces take the mask of the whole.  `call` numbers the draws of one seed: two calls with
 * the same (seed, call) draw the same mask.  seed and call are by value, so a launch captured into a HIP graph repeats its mask on
 * every replay.
 *
 * ftx_dropout: x, y (n) float32, 4-byte aligned; y == x (in place) is allowed, any other overlap is FTX_EINVAL.  0 <= p < 1, anything
 * else (NaN included) is FTX_EINVAL before a launch.  n = 0 launches nothing.  Exactly n elements are written; no allocation, no
 * synchronisation.  Where the logical index is a multiple of four at a 16-byte boundary of both buffers (elem0 % 4 == 0 and aligned
 * pointers is the common case) four consecutive elements share one Philox block and one 16-byte load and store; the elements in
 * front of and behind that range, and every element of a buffer aligned otherwise, take a scalar path with the same bits.
 * ftx_dropout_mask: keep (n) uint8, 1 = kept, 0 = dropped, of the same stream.
 * ftx_dropout_sweep_elements: the elements one sweep of the capped grid covers on the 16-byte path (a larger n grid-strides). */
int64_t ftx_dropout_sweep_elements(void);
int ftx_dropout(const float *x, int64_t n, float p, uint64_t seed, uint64_t call, uint64_t elem0, float *y, void *stream);
int ftx_dropout_mask(int64_t n, float p, uint64_t seed, uint64_t call, uint64_t elem0, uint8_t *keep, void *stream);

/* ---- native index build of the SPVCNN LiDAR branch: from raw points to the batch tables ftx_spvcnn_eval reads ----
 * Everything of a batch that depends on its coordinates only (SPVCNN._index_steps(ahead=True) in the Python package): the voxel sets of
 * the five levels (strides 1, 2, 4, 8, 16), their coordinates and hash tables, the nine kernel maps (the 3^3 map of every level, then the
 * strided 2^3 map between consecutive levels), the point <-> voxel structures at strides 1, 16 and 4 and the voxelised input features.
 * Two sizes are data dependent, so the build is three calls with a host read between them; no call allocates, synchronises or blocks,
 * and every argument is checked before the first launch (FTX_EINVAL / FTX_EWORKSPACE with a text in ftx_last_error()).
 *   A  ftx_spvcnn_index_levels: coords (n, 4) float32 [x, y, z, batch].  Rescales x, y, z by init_res / after_res when the two differ
 *      (float32: (x * init_res) * (1 / after_res)), floors, and finds every level's voxel set in one sort (ftx_levels_unique).  Queues
 *      the copy of the 6 level offsets (int32; level l has offsets[l + 1] - offsets[l] voxels) into level_off_pinned and returns.
 *   B  ftx_spvcnn_index_maps: level_off_host = those 6 values once the copy has arrived; feats (n, c_in) float32, c_in a multiple of 4.
 *      Builds everything that does not depend on a pair count: per-level coordinates and hash tables; the stride-1 point -> voxel rows,
 *      counts, sorted segments and the voxelised features x0; nbr, pos and koff of the five 3^3 maps; the four 2^3 maps complete (their
 *      pair count is n_in); idx / counts / segments / corner rows / trilinear weights at strides 1, 16, 4; with
 *      with_backward_segments != 0 also the (point, corner) entries sorted by voxel that the devoxelise backward reduces over.  Queues
 *      the copy of the five 3^3 pair counts (int32) into pair_counts_pinned and returns.  coords, n, init_res, after_res as in phase A.
 *   C  ftx_spvcnn_index_pairs: pair_counts_host = those 5 values.  Builds pos_t, pair_in and pair_out of the five 3^3 maps and writes
 *      the host tables rows_host (int64[6]), maps_host (9 map records: the 3^3 maps of strides 1..16, then the 2^3 maps 1->2 .. 8->16)
 *      and pvs_host (3 pv records: strides 1, 16, 4) in the layouts ftx_spvcnn_eval reads (ftx_spvcnn_map_bytes / ftx_spvcnn_pv_bytes
 *      per record); *x0 (optional) receives the device pointer of the voxelised features (rows[0], c_in).  level_off_host, c_in and
 *      with_backward_segments must be the values phase B was given.
 * Each repeated step (level coordinates + hash-table insert, the neighbour tables of the nine maps and the corner queries, the
 * validity scan, the pair compaction, the per-stride point queries / segments / weights) is one launch over all its instances.  The
 * results equal those of the per-level entry points bit for bit.
 * Memory.  One caller-owned device arena per phase, 256-byte aligned, every region inside 256-byte aligned; each is sized from the values
 * known when its phase is issued by a host function that needs no GPU (0 and an error text for arguments it refuses), is a multiple of
 * 256 and never decreases when n, a level size or a pair count grows.  Arena A is read by phases B and C, arena B by phase C; the batch's
 * structures live in all three, so all three stay allocated while the batch is in use.  The tails of arenas A and B hold the sort and
 * scan temporaries; the part of them that the sorting library sizes is reserved by a bound and checked against the library's own
 * figure when the phase is issued (FTX_EWORKSPACE if the bound falls short: nothing is launched).
 * ftx_spvcnn_index_layout: the byte offsets of every array inside its arena, ftx_spvcnn_index_layout_words() int64 words, for a binding
 * that wants views of the arrays: a_total, b_total, c_total; arena A: coords (rescaled, n x 4 float), points (floored, n x 4 int32),
 * uniq (5n int64), first (5n int32), sorted_keys (5 x n int64), order (5 x n int32); arena B: per level {coords, table keys, table
 * values, table capacity (a count, not an offset)}; x0; per map (9) {nbr, pos, koff}; per 2^3 map (4) {pos_t, pair_in, pair_out}; per
 * pv (3) {vox_idx, vox_counts, vox_seg_off, devox_idx, devox_weights, devox_bwd_order, devox_bwd_seg_off}; arena C: per 3^3 map (5)
 * {pos_t, pair_in, pair_out}.  level_off_host / pair_counts_host may be NULL: the arenas that depend on them are reported as 0. */
int32_t ftx_spvcnn_index_layout_words(void);
int ftx_spvcnn_index_layout(int64_t n, int32_t c_in, const int32_t *level_off_host, const int32_t *pair_counts_host, int32_t with_backward_segments, int64_t *words_host);
size_t ftx_spvcnn_index_levels_arena_bytes(int64_t n);
size_t ftx_spvcnn_index_maps_arena_bytes(int64_t n, int32_t c_in, const int32_t *level_off_host, int32_t with_backward_segments);
size_t ftx_spvcnn_index_pairs_arena_bytes(int64_t n, const int32_t *level_off_host, const int32_t *pair_counts_host);
int ftx_spvcnn_index_levels(const float *coords, int64_t n, float init_res, float after_res, void *arena_a, size_t arena_a_bytes, int32_t *level_off_pinned, void *stream);
int ftx_spvcnn_index_maps(const float *coords, int64_t n, float init_res, float after_res, const float *feats, int32_t c_in, const int32_t *level_off_host, int32_t with_backward_segments, void *arena_a, size_t arena_a_bytes, void *arena_b, size_t arena_b_bytes, int32_t *pair_counts_pinned, void *stream);
int ftx_spvcnn_index_pairs(int64_t n, int32_t c_in, const int32_t *level_off_host, int32_t with_backward_segments, const int32_t *pair_counts_host, void *arena_a, void *arena_b, size_t arena_b_bytes, void *arena_c, size_t arena_c_bytes, int64_t *rows_host, void *maps_host, void *pvs_host, const float **x0, void *stream);

/* ---- the ViT image branch in eval mode: patch embedding, tap stems and the trunk executor (models/transformers.py:16-45,90-100,
 *      models/image_models_billinear.py:8-24,88-126) (csrc/ftx_dense_common.h, csrc/ftx_dense_common.hip, csrc/ftx_exec_vit.hip) ----
 * Two A-addressing forms of the dense GEMM families above.  The tile rule, the piece split, the accumulator order and the reduction
 * order are those of ftx_dense_gemm_split / ftx_dense_gemm_bf16 (the precision contracts above hold unchanged), so each form returns
 * the bits of that entry run with FTX_EPI_BIAS on a materialised copy of its A, followed by its own epilogue.
 *
 * ftx_vit_patch_embed_<split|bf16>: tokens (b, t0 + gh gw, dim) from img (b, c, h, w) float32 (what ftx_sample_down_fwd wrote), gh = h /
 * patch, gw = w / patch.  A is never materialised: row (frame, gy, gx), reduction index k = (ci, py, px) reads img[frame][ci][gy patch +
 * py][gx patch + px].  W: the Conv2d weight (dim, c, patch, patch) viewed (dim, c patch patch); bias (dim).  Epilogue, in this rounding
 * order: tokens[frame][t0 + patch] = (sum + bias) + pos[t0 + patch], pos (t0 + gh gw, dim).  One more small launch writes the leading
 * rows: tokens[frame][0] = cls + pos[0] and, with t0 = 2, tokens[frame][1] = dist + pos[1] (cls, dist (dim); dist may be NULL only with
 * t0 = 1).  Refused before anything is launched: c patch patch % 64 != 0, dim % 4 != 0, patch % 4 != 0, h or w not whole patches, t0
 * outside {1, 2}, null or not 16-byte aligned pointers.  b == 0 returns FTX_OK without launching.
 *
 * ftx_vit_tap_stem_<split|bf16>: BilinearModule's stem on the token grid in eval mode, one launch: out (b, g, co) = BatchNorm(ReLU(
 * tokens[:, t0:] W^T + bias)), tokens (b, t0 + g, dim), W (co, dim).  Row r of A is token row (r / g) (t0 + g) + t0 + r % g.  Epilogue
 * order: bias, ReLU, then the eval-mode BatchNorm with the rounding sequence of ftx_bn_eval_fwd.  out is (b, gh, gw, co) channels-last:
 * what ftx_lift_gather_fwd reads.  dim % 64 == 0, co % 4 == 0, t0 in {0, 1, 2}.
 *
 * ftx_rows_add_bias: out (n, c) = r + (p + pb), pb (c) broadcast over the rows, in that rounding order (the residual stream of the
 * trunk as one tensor).  p and pb NULL together: out = r.  c % 4 == 0, 16-byte aligned pointers. */
int ftx_vit_patch_embed_split(const float *img, const float *W, const float *bias, const float *cls, const float *dist, const float *pos, int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *tokens, void *stream);
int ftx_vit_patch_embed_bf16(const float *img, const float *W, const float *bias, const float *cls, const float *dist, const float *pos, int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *tokens, void *stream);
int ftx_vit_tap_stem_split(const float *tokens, const float *W, const float *bias, const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *out, void *stream);
int ftx_vit_tap_stem_bf16(const float *tokens, const float *W, const float *bias, const float *gamma, const float *beta, const float *running_mean, const float *running_var, float eps, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *out, void *stream);
int ftx_rows_add_bias(const float *r, const float *p, const float *pb, int64_t n, int32_t c, float *out, void *stream);

/* ---- the patch embedding and the tap stems in training (models/transformers.py:90-100, models/image_models_billinear.py:8-24)
 *      (csrc/ftx_dense_common.h, csrc/ftx_dense_common.hip) ----
 * Operand forms of the dense families' weight-gradient kernel and output forms of their GEMM kernel, as the eval forms above are forms
 * of the GEMM's A: the tile and split rules, the piece split, the accumulator order and the reduction order are those of
 * ftx_dense_wgrad_<split|bf16> / ftx_dense_gemm_<split|bf16>, so every product below returns the bits of that plain entry run on
 * materialised operands, followed by the stated store.  Every entry validates all of its arguments, the workspace size included, before
 * its first launch; none allocates, synchronises the host or uses atomics; all are capturable.  Every pointer 16-byte aligned.
 * The forward of the patch embedding in training is ftx_vit_patch_embed_<split|bf16> above.
 *
 * ftx_vit_patch_embed_bwd_<split|bf16>: from dtokens (b, t0 + g, dim), the gradient of the tokens, and img (b, c, h, w), g = (h / patch)
 * (w / patch), dY = the rows t0.. of every frame of dtokens (b g rows, never copied):
 *   dW (dim, c patch patch) = dY^T unfold(img)   the weight gradient with G = the strip rows of dtokens and X = the unfold addressing of
 *                                                ftx_vit_patch_embed; workspace partials as ftx_dense_wgrad_* for (b g, dim, c patch patch)
 *   dpos (t0 + g, dim)      = dtokens[0] + dtokens[1] + ... + dtokens[b - 1], fp32, frames ascending
 *   dcls (dim) = dpos[0];  ddist (dim) = dpos[1] (t0 = 2; ddist may be NULL with t0 = 1)
 *   dbias (dim)             = ftx_colsum of the g rows dpos[t0 ..]: the frames are summed first (fp32, ascending), the patches second
 *                             (float64, ftx_colsum's fixed order).  This order is the definition of the bias gradient: it is
 *                             reproducible and is NOT the column sum of the b g rows of dY.
 *   dimg (b, c, h, w)       only with dimg != NULL (W (dim, c patch patch) is then required, and dim % 64 == 0): fold(dY W), the data
 *                             gradient of ftx_dense_gemm_* (w_kn = 1) with A = the strip rows and the output written through the
 *                             fold: element (row (frame, gy, gx), column (ci, py, px)) to dimg[frame][ci][gy patch + py][gx patch + px].
 *                             The patches do not overlap: every pixel is written exactly once, nothing is accumulated.
 * Refused: c patch patch % 64 != 0, patch % 4 != 0, dim % 4 != 0, h or w not whole patches, t0 outside {1, 2}, b < 1, null or
 * misaligned pointers, workspace_bytes < ftx_vit_patch_embed_bwd_<split|bf16>_workspace_bytes(b, c, h, w, patch, dim).
 *
 * ftx_vit_tap_stem_train_fwd_<split|bf16>: rows (b g, co) = ReLU(tokens[:, t0:] W^T + bias), tokens (b, t0 + g, dim), W (co, dim): the
 * A addressing of ftx_vit_tap_stem_*, the epilogue stops behind the ReLU (x < 0 ? 0 : x, NaN stays NaN).  The sequence of a stem in
 * training is   ftx_vit_tap_stem_train_fwd -> ftx_bn_train_fwd on rows (b g, co) -> the lift;   backward:   ftx_bn_train_bwd -> its
 * input gradient is drows of ftx_vit_tap_stem_bwd.  dim % 64 == 0, co % 4 == 0, t0 in {0, 1, 2}; b == 0 returns FTX_OK.
 *
 * ftx_vit_tap_stem_bwd_<split|bf16>: from drows (b g, co), the saved rows (b g, co) and tokens; gm = drows where rows > 0, else 0 (a
 * select: also 0 where rows is NaN):
 *   dW (co, dim)             = gm^T tokens[:, t0:]   the weight gradient with the mask in G's load and the strip addressing as X
 *   dbias (co)               = ftx_colsum of gm (b g rows), gm written once to the workspace
 *   dtokens (b, t0 + g, dim) = rows t0.. of every frame: gm . W; the t0 leading rows: zero.  Fully written.  The product's reduction
 *                              is co (96), no multiple of the dense GEMM's 64: it runs on the rows GEMM of the mode,
 *                              ftx_rows_gemm_<split|bf16>(gm, b g, W, w_transposed = 0, bias = NULL, ca = co, co = dim), into the
 *                              workspace, and one store pass moves its rows behind the leading rows.  W is not padded.
 * workspace: ftx_vit_tap_stem_bwd_<split|bf16>_workspace_bytes(b, g, dim, co).  Refusals as the forward, and b < 1. */
size_t ftx_vit_patch_embed_bwd_split_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim);
size_t ftx_vit_patch_embed_bwd_bf16_workspace_bytes(int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim);
int ftx_vit_patch_embed_bwd_split(const float *dtokens, const float *img, const float *W, int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *dW, float *dbias, float *dcls, float *ddist, float *dpos, float *dimg, void *workspace, size_t workspace_bytes, void *stream);
int ftx_vit_patch_embed_bwd_bf16(const float *dtokens, const float *img, const float *W, int32_t b, int32_t c, int32_t h, int32_t w, int32_t patch, int32_t dim, int32_t t0, float *dW, float *dbias, float *dcls, float *ddist, float *dpos, float *dimg, void *workspace, size_t workspace_bytes, void *stream);
int ftx_vit_tap_stem_train_fwd_split(const float *tokens, const float *W, const float *bias, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *rows, void *stream);
int ftx_vit_tap_stem_train_fwd_bf16(const float *tokens, const float *W, const float *bias, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *rows, void *stream);
size_t ftx_vit_tap_stem_bwd_split_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co);
size_t ftx_vit_tap_stem_bwd_bf16_workspace_bytes(int32_t b, int32_t g, int32_t dim, int32_t co);
int ftx_vit_tap_stem_bwd_split(const float *drows, const float *rows, const float *tokens, const float *W, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *dW, float *dbias, float *dtokens, void *workspace, size_t workspace_bytes, void *stream);
int ftx_vit_tap_stem_bwd_bf16(const float *drows, const float *rows, const float *tokens, const float *W, int32_t b, int32_t g, int32_t t0, int32_t dim, int32_t co, float *dW, float *dbias, float *dtokens, void *workspace, size_t workspace_bytes, void *stream);

/* ftx_vit_eval: the eval-mode, no-gradient forward of blocks [block_first, block_last] of the trunk, with the tap stems behind the
 * tapped blocks.  Tables: packed little-endian records in HOST memory holding device pointers (float32, contiguous); the library
 * reports each record size (ftx_vit_*_bytes).
 *   model (one record): const float *patch_w (dim, in_chans patch patch), *patch_b (dim), *cls (dim), *dist (dim, NULL with t0 = 1),
 *     *pos (t0 + grid grid, dim); int32 dim, heads, hidden (the MLP width), patch, grid (patches per side: the image is (in_chans,
 *     grid patch, grid patch)), t0 (1, or 2 for a distilled trunk), in_chans; float eps (of every LayerNorm).
 *   block (n_blocks records): const float *norm1_w, *norm1_b, *qkv_w (3 dim, dim), *qkv_b, *proj_w (dim, dim), *proj_b, *norm2_w,
 *     *norm2_b, *fc1_w (hidden, dim), *fc1_b, *fc2_w (dim, hidden), *fc2_b.
 *   tap (n_taps records, ascending by block): const float *stem_w (co, dim), *stem_b, *gamma, *beta, *running_mean, *running_var (co);
 *     int32 block, co; float eps; int32 reserved.  tap_out_host[i]: where tap i goes, (b, grid, grid, co) float32 on the device.
 * A call with block_first = 0 starts from tokens_in (b, t0 + grid grid, dim) if it is given, else from img (b, in_chans, grid patch, grid
 * patch) through ftx_vit_patch_embed_*; a call with block_first > 0 continues from the residual state the previous call left in the
 * arena (which must have ended at block_first - 1, for the same b), so a fusion caller runs to the middle tap, hands the lifted features
 * to the LiDAR stream and continues.  Per block the call issues what transformers.Block.chain issues: ftx_add_layernorm_fwd (y NULL on
 * the first block, else the previous block's MLP output with fc2's bias as y_bias), the qkv GEMM with FTX_EPI_BIAS, attention (scale
 * 1/8), the proj GEMM with FTX_EPI_NONE, ftx_add_layernorm_fwd with y_bias = proj's bias, fc1 with FTX_EPI_BIAS_GELU, fc2 with
 * FTX_EPI_NONE.  linear_mode: 0 = ftx_dense_gemm_split, 1 = ftx_dense_gemm_bf16 (and the matching patch embedding and tap stem);
 * attn_mode: 0 = ftx_attn_fwd_tiled(..., 0, 0) (the automatic tiling, what ftx_attn_fwd runs), 1 = ftx_attn_fwd_bf16(..., 0, 0),
 * 2 = ftx_attn_fwd_split(..., 0, 0); any other value is refused.  At a tap the stream r + (p + pb) becomes one tensor (ftx_rows_add_bias) and
 * ftx_vit_tap_stem_* writes tap_out_host[i]; both residual forms round in that order, so the results do not depend on where a caller
 * materialises.  Taps in front of block_first are skipped (an earlier call wrote them).
 * Refused before the first launch (FTX_EINVAL): heads * 64 != dim, dim outside {256, 512, 768, 1024}, hidden % 64 != 0, taps not
 * ascending or past block_last, a null or not 16-byte aligned parameter of a block or tap the call runs (the tap's BatchNorm vectors
 * need no alignment), a misaligned tap output, block_first > 0 on an arena that holds no state for this b; an arena that is too small
 * is FTX_EWORKSPACE.  b == 0 returns FTX_OK.
 * Arena: device memory, 256-byte aligned, caller-owned; ftx_vit_eval_arena_bytes(model, n_blocks, b) is a host function (needs no GPU;
 * 0 and an error text for a record it refuses), a multiple of 256, and grows with b.  No host synchronisation and no allocation: a call
 * can be captured into a HIP graph.  The one thing the library keeps beyond a call is a host-side note, per arena address, of the b and
 * the block its residual state stands in front of: the signature above has no other place for it, and the state itself is device
 * memory the host must not read.  The note is written when a call is ISSUED.  It vouches for the order of the calls a host makes, not
 * for the arena's contents: a captured continuation (block_first > 0) is checked once, at capture, and a replay runs on whatever the
 * arena then holds, so a caller that replays it must replay (or issue) the calls in front of it on that arena first, with nothing else
 * using the arena in between.  ftx_vit_eval_release(arena) drops the note (host only, always FTX_OK): call it before freeing an arena
 * or giving its memory another use, otherwise a later buffer at the same address with the same b would pass for a continuation. */
int32_t ftx_vit_model_bytes(void);
int32_t ftx_vit_block_bytes(void);
int32_t ftx_vit_tap_bytes(void);
size_t ftx_vit_eval_arena_bytes(const void *model_host, int32_t n_blocks, int32_t b);
int ftx_vit_eval_release(const void *arena);
int ftx_vit_eval(const void *model_host, const void *blocks_host, int32_t n_blocks, const void *taps_host, int32_t n_taps, int32_t b, const float *img, const float *tokens_in, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode, float *const *tap_out_host, void *arena, size_t arena_bytes, void *stream);

/* ---- the ViT trunk in training: one forward and one backward call per trunk segment (models/transformers.py:16-45)
 *      (csrc/ftx_exec_vit_train.hip; the tables and their checker, shared with ftx_vit_eval: csrc/ftx_vit_tables.h) ----
 * A segment is blocks [block_first, block_last] from one materialised token tensor x_in (b, t0 + grid grid, dim) to one materialised
 * token tensor x_out of that shape, x_out = r + (m + fc2_b): the patch embedding, the tap stems, the lift and the heads stay with the
 * caller.  The model and block records, linear_mode and attn_mode are ftx_vit_eval's, refused with the same texts (the model record's
 * patch-embedding pointers are not read).
 *
 * ftx_vit_train_fwd issues per block what ftx_vit_eval issues -- ftx_add_layernorm_fwd (y NULL on the first block of the segment), the
 * qkv GEMM with FTX_EPI_BIAS, attention with the automatic tiling and scale 1/8, the proj GEMM with FTX_EPI_NONE, ftx_add_layernorm_fwd
 * with y_bias = proj's bias, fc1 with FTX_EPI_BIAS_GELU, fc2 with FTX_EPI_NONE -- into per-block regions of the arena, then
 * ftx_rows_add_bias into x_out.  ftx_vit_train_bwd walks the blocks in reverse and issues per block: for the last block ftx_colsum of
 * grad_out (the last fc2 bias); fc2's data gradient (w_kn = 1) with FTX_EPI_DGELU, fc2's weight gradient, fc1's data gradient, fc1's
 * weight gradient, ftx_colsum of fc1's output gradient; ftx_add_layernorm_bwd at norm2 with with_y_bias (d gamma, d beta, d proj bias);
 * proj's data and weight gradient; the attention backward of the mode; qkv's data gradient, weight gradient and ftx_colsum;
 * ftx_add_layernorm_bwd at norm1 with with_y_bias (d gamma, d beta and the previous block's d fc2 bias), or without grad_s and y_bias on
 * the first block of the segment.  x_in feeds that first norm1 and the residual: its two gradients are added by one ftx_rows_add into
 * grad_in (b, t0 + grid grid, dim), which is fully written.  These are the calls, arguments and workspace sizes of the autograd nodes
 * of the Python package (transformers.Block.chain), so x_out, grad_in and every parameter gradient have that path's bits.
 *
 * Gradient table (grads_host): n_blocks records of the block record's layout (ftx_vit_train_block_bytes() bytes each, twelve device
 * pointers in the same order) that say where each parameter gradient is written: float32, the parameter's shape, 16-byte aligned,
 * caller-owned, every element written (not accumulated into).  Records outside [block_first, block_last] are not read.  The LayerNorm
 * backward writes (d gamma, d beta, d y_bias) as one (3, dim) array: where norm2_w, norm2_b, proj_b of a record are consecutive in
 * memory (and norm1_w, norm1_b and the previous record's fc2_b, for a block behind the first of the segment) it writes them in place;
 * otherwise they pass through the arena and three more small launches copy them.
 *
 * Arena: device memory, 256-byte aligned, caller-owned, the same buffer for the forward and its backward, not to be written in between.
 * ftx_vit_train_arena_bytes(model, n_blocks, block_first, block_last, b) is a host function of its arguments alone (0 and an error
 * text for a record or a range it refuses), a multiple of 256, growing with b and with the number of blocks.  With rows = b (t0 + grid
 * grid), row = 4 rows dim, wide = 4 rows hidden, stat = 8 rows and lse = 4 b heads (t0 + grid grid) bytes, each rounded up to 256:
 *   per block      what the backward reads: s, h, att, s2, h2 (row each; no s for the first block of the segment, whose s is x_in),
 *                  qkv (3 row), pre, act (wide each), the two LayerNorm statistics (stat each), lse:
 *                  8 row + 2 wide + 2 stat + lse, less one row for the first block;
 *   once           3 row (the flowing gradients and the second contribution to grad_in; the forward keeps fc2's and proj's output
 *                  there) + wide (fc1's output gradient) + 3 row (the attention's input gradient) + the largest of
 *                  ftx_attn_bwd_workspace_bytes(b, t0 + grid grid, heads), ftx_layernorm_bwd_workspace_bytes(rows, dim),
 *                  ftx_colsum_workspace_bytes(rows, dim | hidden | 3 dim) and ftx_dense_wgrad_<split|bf16>_workspace_bytes(rows, n, k)
 *                  over the four Linears + 12 dim (the LayerNorm's parameter gradients on their way to buffers that are apart).
 * Refused before the first launch (FTX_EINVAL): what ftx_vit_eval refuses of the model record, the block range and the modes; a null or
 * not 16-byte aligned parameter or gradient pointer of a block in the range; null or misaligned x_in, x_out, grad_out, grad_in; an
 * arena that is too small is FTX_EWORKSPACE.  b == 0 returns FTX_OK without touching the arena.  A failing launch names the block and
 * the op.  No host synchronisation and no allocation.  The library keeps a host-side note per arena address of the forward it holds:
 * ftx_vit_train_bwd is refused when no forward with the same (b, block_first, block_last, linear_mode, attn_mode) was issued on that
 * arena, and when it is issued a second time (the first backward overwrites the temporaries).  ftx_vit_train_release(arena) drops the
 * note (host only, always FTX_OK): call it before freeing an arena or giving its memory another use. */
int32_t ftx_vit_train_block_bytes(void);
size_t ftx_vit_train_arena_bytes(const void *model_host, int32_t n_blocks, int32_t block_first, int32_t block_last, int32_t b);
int ftx_vit_train_release(const void *arena);
int ftx_vit_train_fwd(const void *model_host, const void *blocks_host, int32_t n_blocks, int32_t b, const float *x_in, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode, float *x_out, void *arena, size_t arena_bytes, void *stream);
int ftx_vit_train_bwd(const void *model_host, const void *blocks_host, const void *grads_host, int32_t n_blocks, int32_t b, const float *x_in, const float *grad_out, int32_t block_first, int32_t block_last, int32_t linear_mode, int32_t attn_mode, float *grad_in, void *arena, size_t arena_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FTX_H */
