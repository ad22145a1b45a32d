// Differentiable affine grid sampling of the spatial transformers (models/transformers.py:102-156 of the reference):
//   F.grid_sample(src, F.affine_grid(theta, (b, ., H, W), align_corners=False), mode="bilinear", padding_mode="zeros", align_corners=False)
// without the grid.  Output pixel (r, c) of an (H, W) target:
//   xn = (2c+1)/W - 1, yn = (2r+1)/H - 1;  gx = t00 xn + t01 yn + t02, gy = t10 xn + t11 yn + t12;
//   ix = ((gx+1) iw - 1)/2, iy = ((gy+1) ih - 1)/2;  value = the four-corner bilinear sum, corners outside the source count as 0.
// aff_tap() is the ONE place that computes coordinates, corners and weights; the dense form (stn_down: every pixel of the target) and the
// point form (ScaleUpModule + get_img_feats: only the ~20 k pixels the points pick, the 96 x 370 x 1226 map never exists) both call it,
// so they agree bit for bit (floating-point contraction is off in this file: no kernel may fuse what another one rounds twice).
//
// The source is described by element strides (frame, channel, row, column): NCHW and channels-last are the same code.
//
// Backward, no float atomics anywhere:
//   d/d theta   every block reduces the six sums of ONE frame over its slice of pixels / points in float64 and leaves a row of partials;
//               the last block to finish adds the rows in block order (ftx_lastblock.h) -> bit-reproducible, one launch.
//   d/d src     (point form only; the dense form's source is the input image) the points are sorted by their top-left source cell
//               (ftx_affine_lift_cells -> ftx_segment_build, key space (b, ih+1, iw+1) so that a sample half outside still has a key);
//               every source element then gathers from the four segments whose samples can touch it, in a fixed order, and is
//               written exactly once.
#include "ftx_common.h"
#include "ftx_lastblock.h"
#include "ftx_reduce.h"

#pragma clang fp contract(off)

using namespace ftx;

namespace {

constexpr int AFF_MAX_B = 128;          // frames: a partial row holds 6 b doubles (<= LB_MAX_COLS * 2)
constexpr int AFF_MAX_BLOCKS = 1024;    // blocks of a d/d theta launch (<= LB_GROUP * LB_MAX_GROUPS)

struct AffSrc {
  const float *p;
  int64_t sb, sc, sy, sx;   // element strides of (frame, channel, row, column)
  int b, c, ih, iw;
};

struct AffTap {
  int x0, y0;                  // top-left source cell: -1 .. iw-1, -1 .. ih-1
  float ex, fx, ey, fy;        // ex = x0 + 1 - ix, fx = ix - x0 (likewise y): the weights are their products
  float xn, yn;                // normalised target coordinates (the d/d theta factors)
  bool live;                   // at least one corner can lie inside the source
  bool nan;                    // a coordinate is NaN (a NaN theta): the forward value is NaN, as grid_sample's arithmetic would give
};

__device__ inline AffTap aff_tap(const float *__restrict__ th, int r, int col, int H, int W, int ih, int iw) {
  AffTap t;
  t.xn = (float)(2 * col + 1) / (float)W - 1.f;
  t.yn = (float)(2 * r + 1) / (float)H - 1.f;
  const float gx = (th[0] * t.xn + th[1] * t.yn) + th[2];
  const float gy = (th[3] * t.xn + th[4] * t.yn) + th[5];
  const float ix = ((gx + 1.f) * (float)iw - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)ih - 1.f) / 2.f;
  t.nan = ix != ix || iy != iy;
  t.live = ix > -1.f && ix < (float)iw && iy > -1.f && iy < (float)ih;   // false for NaN / Inf: the floor below always fits an int
  t.x0 = t.y0 = 0;
  t.ex = t.fx = t.ey = t.fy = 0.f;
  if (t.live) {
    const float xf = floorf(ix), yf = floorf(iy);
    t.x0 = (int)xf;
    t.y0 = (int)yf;
    t.ex = (xf + 1.f) - ix;
    t.fx = ix - xf;
    t.ey = (yf + 1.f) - iy;
    t.fy = iy - yf;
  }
  return t;
}

// The four corner values of one (frame, channel) plane; a corner outside the source is 0.  Only call with t.live.
__device__ inline void aff_corners(const AffSrc &S, int f, int ch, const AffTap &t, float &v00, float &v01, float &v10, float &v11) {
  const float *pl = S.p + (int64_t)f * S.sb + (int64_t)ch * S.sc;
  const bool xa = t.x0 >= 0, xb = t.x0 + 1 < S.iw, ya = t.y0 >= 0, yb = t.y0 + 1 < S.ih;
  const int64_t o = (int64_t)t.y0 * S.sy + (int64_t)t.x0 * S.sx;
  v00 = (xa && ya) ? pl[o] : 0.f;
  v01 = (xb && ya) ? pl[o + S.sx] : 0.f;
  v10 = (xa && yb) ? pl[o + S.sy] : 0.f;
  v11 = (xb && yb) ? pl[o + S.sy + S.sx] : 0.f;
}

__device__ inline float aff_value(const AffSrc &S, int f, int ch, const AffTap &t) {
  if (!t.live) return t.nan ? __builtin_nanf("") : 0.f;
  float v00, v01, v10, v11;
  aff_corners(S, f, ch, t, v00, v01, v10, v11);
  return ((v00 * (t.ex * t.ey) + v01 * (t.fx * t.ey)) + v10 * (t.ex * t.fy)) + v11 * (t.fx * t.fy);
}

// Frame, row and column of point i; false (a zero row, no gradient) when the frame or the pixel is outside its range.
__device__ inline bool aff_point(const int64_t *__restrict__ img_idx, const int32_t *__restrict__ pb, int64_t i, int b, int H, int W, int &f,
                                 int &r, int &col) {
  const int64_t rr = img_idx[i * 2], cc = img_idx[i * 2 + 1];
  f = pb[i];
  r = (int)rr;
  col = (int)cc;
  return f >= 0 && f < b && rr >= 0 && rr < H && cc >= 0 && cc < W;
}

__global__ __launch_bounds__(256) void aff_sample_fwd_kernel(AffSrc S, const float *__restrict__ theta, int oh, int ow, float *__restrict__ out) {
  const int64_t P = (int64_t)oh * ow, total = (int64_t)S.b * P;
  for (int64_t p = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const int f = (int)(p / P);
    const int64_t q = p - (int64_t)f * P;
    const int r = (int)(q / ow), col = (int)(q - (int64_t)r * ow);
    const AffTap t = aff_tap(theta + f * 6, r, col, oh, ow, S.ih, S.iw);
    for (int ch = 0; ch < S.c; ++ch) out[((int64_t)f * S.c + ch) * P + q] = aff_value(S, f, ch, t);
  }
}

// out (n, c): channel innermost over the threads -- the row stores are coalesced, and so are the corner loads of a channels-last source.
__global__ __launch_bounds__(256) void aff_lift_fwd_kernel(AffSrc S, const float *__restrict__ theta, const int64_t *__restrict__ img_idx,
                                                           const int32_t *__restrict__ pb, int64_t n, int H, int W, float *__restrict__ out) {
  const int64_t total = n * S.c;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / S.c;
    const int ch = (int)(e - i * S.c);
    int f, r, col;
    float v = 0.f;
    if (aff_point(img_idx, pb, i, S.b, H, W, f, r, col)) v = aff_value(S, f, ch, aff_tap(theta + f * 6, r, col, H, W, S.ih, S.iw));
    out[e] = v;
  }
}

__global__ __launch_bounds__(256) void aff_lift_cells_kernel(const float *__restrict__ theta, const int64_t *__restrict__ img_idx,
                                                             const int32_t *__restrict__ pb, int64_t n, int b, int ih, int iw, int H, int W,
                                                             int32_t *__restrict__ cells) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int f, r, col;
    int32_t key = -1;
    if (aff_point(img_idx, pb, i, b, H, W, f, r, col)) {
      const AffTap t = aff_tap(theta + f * 6, r, col, H, W, ih, iw);
      if (t.live) key = (int32_t)(((int64_t)f * (ih + 1) + (t.y0 + 1)) * (iw + 1) + (t.x0 + 1));
    }
    cells[i] = key;
  }
}

struct StoreTheta {
  float *grad_theta;
  int c3;   // 3 b: the first half of a row of totals holds grad_theta[0 .. 3b), the second half the rest
  __device__ void operator()(int col, double lo, double hi) const {
    grad_theta[col] = (float)lo;
    grad_theta[c3 + col] = (float)hi;
  }
};

// d loss / d theta.  Block (f, k) = blockIdx.x / bpf, % bpf takes slice k of the items of frame f: POINTS false -- the oh x ow pixels of
// the frame, one thread each, grad_out (b, c, oh, ow); POINTS true -- the points whose frame is f, G lanes (a power of two <= 64) per
// point over the channels, grad_out (n, c).  Per item gix = sum_ch g * d value / d ix in float32 as grid_sample's backward has it; the six
// sums gx' xn, gx' yn, gx', gy' xn, gy' yn, gy' (gx' = gix iw / 2) are float64.  Every order of summation depends on the sizes only.
template <bool POINTS>
__global__ __launch_bounds__(256) void aff_theta_kernel(AffSrc S, const float *__restrict__ theta, const float *__restrict__ go,
                                                        const int64_t *__restrict__ img_idx, const int32_t *__restrict__ pb, int64_t n, int H, int W,
                                                        int G, int bpf, double *__restrict__ part, StreamScratch sc, float *__restrict__ grad_theta) {
  __shared__ double lds[256 + 6 * AFF_MAX_B];
  const int tid = threadIdx.x;
  const int f = blockIdx.x / bpf, k = blockIdx.x - f * bpf;
  const int per = 256 / G, sub = tid & (G - 1);
  const int64_t P = (int64_t)H * W;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t base = (int64_t)k * per; base < n; base += (int64_t)bpf * per) {
    const int64_t item = base + tid / G;
    bool ok = item < n;
    int r = 0, col = 0;
    if (POINTS) {
      int pf = -1;
      ok = ok && aff_point(img_idx, pb, item, S.b, H, W, pf, r, col) && pf == f;
    } else if (ok) {
      r = (int)(item / W);
      col = (int)(item - (int64_t)r * W);
    }
    AffTap t;
    t.live = false;
    if (ok) t = aff_tap(theta + f * 6, r, col, H, W, S.ih, S.iw);
    float gix = 0.f, giy = 0.f;
    if (ok && t.live) {
      for (int ch = sub; ch < S.c; ch += G) {
        float v00, v01, v10, v11;
        aff_corners(S, f, ch, t, v00, v01, v10, v11);
        const float g = POINTS ? go[item * S.c + ch] : go[((int64_t)f * S.c + ch) * P + item];
        gix += ((v01 - v00) * t.ey + (v11 - v10) * t.fy) * g;
        giy += ((v10 - v00) * t.ex + (v11 - v01) * t.fx) * g;
      }
    }
    for (int off = 1; off < G; off <<= 1) {   // lanes of a group hold consecutive lane ids: a fixed tree, every lane ends with the sum
      gix += __shfl_xor(gix, off, 64);
      giy += __shfl_xor(giy, off, 64);
    }
    if (sub == 0 && ok && t.live) {
      const double gx = (double)(gix * ((float)S.iw / 2.f)), gy = (double)(giy * ((float)S.ih / 2.f));
      acc[0] += gx * t.xn; acc[1] += gx * t.yn; acc[2] += gx;
      acc[3] += gy * t.xn; acc[4] += gy * t.yn; acc[5] += gy;
    }
  }
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double v = wave_sum_down(acc[q]);
    if (lane == 0) lds[wave * 6 + q] = v;
  }
  __syncthreads();
  const int c2 = 6 * S.b;
  double *row = part + (int64_t)blockIdx.x * c2;
  for (int j = tid; j < c2; j += 256) {   // this block's row: its frame's six sums, zero for every other frame
    const int jf = j / 6, q = j - jf * 6;
    lb_store(&row[j], jf == f ? ((lds[q] + lds[6 + q]) + lds[12 + q]) + lds[18 + q] : 0.0);
  }
  __syncthreads();   // lds is free again
  last_block_totals(part, (int)gridDim.x, 3 * S.b, sc, lds, StoreTheta{grad_theta, 3 * S.b});
}

// d loss / d src of the point form.  One thread per source element; it walks the four segments of points whose top-left cell is
// (y, x), (y, x-1), (y-1, x), (y-1, x-1) -- this element is their corner 00, 01, 10, 11 -- in that order, each in ascending point id
// (ftx_segment_build's order), and recomputes the weight with aff_tap.  chan_inner: channel fastest over the threads (channels-last).
__global__ __launch_bounds__(256) void aff_lift_bwd_src_kernel(AffSrc S, float *__restrict__ gs, const float *__restrict__ theta,
                                                               const int64_t *__restrict__ img_idx, const float *__restrict__ go,
                                                               const int32_t *__restrict__ order, const int32_t *__restrict__ seg_off, int H,
                                                               int W, int chan_inner) {
  const int64_t total = (int64_t)S.b * S.c * S.ih * S.iw;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int f, ch, y, x;
    int64_t q = e;
    if (chan_inner) {
      ch = (int)(q % S.c); q /= S.c;
      x = (int)(q % S.iw); q /= S.iw;
      y = (int)(q % S.ih);
      f = (int)(q / S.ih);
    } else {
      x = (int)(q % S.iw); q /= S.iw;
      y = (int)(q % S.ih); q /= S.ih;
      ch = (int)(q % S.c);
      f = (int)(q / S.c);
    }
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int ky = y + 1 - (s >> 1), kx = x + 1 - (s & 1);   // key coordinates are cell + 1
      const int64_t key = ((int64_t)f * (S.ih + 1) + ky) * (S.iw + 1) + kx;
      const int lo = seg_off[key], hi = seg_off[key + 1];
      for (int j = lo; j < hi; ++j) {
        const int64_t i = order[j];
        const AffTap t = aff_tap(theta + f * 6, (int)img_idx[i * 2], (int)img_idx[i * 2 + 1], H, W, S.ih, S.iw);
        const float w = (s & 1 ? t.fx : t.ex) * (s >> 1 ? t.fy : t.ey);
        acc += w * go[i * S.c + ch];
      }
    }
    gs[(int64_t)f * S.sb + (int64_t)ch * S.sc + (int64_t)y * S.sy + (int64_t)x * S.sx] = acc;
  }
}

int aff_src(const char *who, AffSrc *S, const float *src, const int64_t *strides, int b, int c, int ih, int iw) {
  FTX_REQUIRE(b >= 1 && c >= 1 && ih >= 1 && iw >= 1, "%s: bad source size", who);
  FTX_REQUIRE(b <= AFF_MAX_B, "%s: more than %d frames", who, AFF_MAX_B);
  FTX_REQUIRE(ih < 32768 && iw < 32768 && (int64_t)b * (ih + 1) * (iw + 1) < 0x7ffffffe, "%s: source too large for int32 cell keys", who);
  FTX_REQUIRE(strides, "%s: null strides", who);
  for (int d = 0; d < 4; ++d) FTX_REQUIRE(strides[d] >= 0, "%s: negative stride", who);
  S->p = src;
  S->sb = strides[0]; S->sc = strides[1]; S->sy = strides[2]; S->sx = strides[3];
  S->b = b; S->c = c; S->ih = ih; S->iw = iw;
  return FTX_OK;
}

int aff_target(const char *who, int H, int W) {
  FTX_REQUIRE(H >= 1 && W >= 1 && H < (1 << 24) && W < (1 << 24) && (int64_t)H * W < 0x7fffffff, "%s: bad target size", who);
  return FTX_OK;
}

int aff_blocks_per_frame(int b, int64_t items, int per_block) {
  int64_t g = ceil_div(items, per_block);
  const int cap = AFF_MAX_BLOCKS / b;
  if (g > cap) g = cap;
  return g < 1 ? 1 : (int)g;
}

int aff_workspace(const char *who, int b, void *workspace, size_t workspace_bytes) {
  FTX_REQUIRE(workspace, "%s: null workspace", who);
  if (workspace_bytes < ftx_affine_theta_workspace_bytes(b)) return workspace_short(who, workspace_bytes, ftx_affine_theta_workspace_bytes(b));
  return FTX_OK;
}

}  // namespace

extern "C" size_t ftx_affine_theta_workspace_bytes(int32_t b) {
  if (b < 1 || b > AFF_MAX_B) return 0;
  return sizeof(double) * (size_t)AFF_MAX_BLOCKS * 6 * (size_t)b;   // one row of 6 b partial sums per block
}

extern "C" int ftx_affine_sample_fwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw,
                                     const float *theta, int32_t oh, int32_t ow, float *out, void *stream) {
  AffSrc S;
  int rc = aff_src("ftx_affine_sample_fwd", &S, src, src_strides, b, c, ih, iw);
  if (rc == FTX_OK) rc = aff_target("ftx_affine_sample_fwd", oh, ow);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(src && theta && out, "ftx_affine_sample_fwd: null pointer");
  aff_sample_fwd_kernel<<<grid_for((int64_t)b * oh * ow, 256), 256, 0, (hipStream_t)stream>>>(S, theta, oh, ow, out);
  return check_launch("ftx_affine_sample_fwd");
}

extern "C" int ftx_affine_sample_bwd_theta(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw,
                                           const float *theta, const float *grad_out, int32_t oh, int32_t ow, float *grad_theta,
                                           void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "ftx_affine_sample_bwd_theta";
  AffSrc S;
  int rc = aff_src(who, &S, src, src_strides, b, c, ih, iw);
  if (rc == FTX_OK) rc = aff_target(who, oh, ow);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(src && theta && grad_out && grad_theta, "%s: null pointer", who);
  rc = aff_workspace(who, b, workspace, workspace_bytes);
  if (rc != FTX_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const StreamScratch sc = stream_scratch(st);
  if (!sc.counters) return FTX_ELAUNCH;
  const int64_t P = (int64_t)oh * ow;
  const int bpf = aff_blocks_per_frame(b, P, 256);
  aff_theta_kernel<false><<<b * bpf, 256, 0, st>>>(S, theta, grad_out, nullptr, nullptr, P, oh, ow, 1, bpf, (double *)workspace, sc, grad_theta);
  return check_launch(who);
}

extern "C" int ftx_affine_lift_fwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw,
                                   const float *theta, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t H, int32_t W,
                                   float *out, void *stream) {
  AffSrc S;
  int rc = aff_src("ftx_affine_lift_fwd", &S, src, src_strides, b, c, ih, iw);
  if (rc == FTX_OK) rc = aff_target("ftx_affine_lift_fwd", H, W);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 0 && n < 0x7fffffff, "ftx_affine_lift_fwd: bad point count");
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(src && theta && img_idx && point_batch && out, "ftx_affine_lift_fwd: null pointer");
  aff_lift_fwd_kernel<<<grid_for(n * c, 256), 256, 0, (hipStream_t)stream>>>(S, theta, img_idx, point_batch, n, H, W, out);
  return check_launch("ftx_affine_lift_fwd");
}

extern "C" int ftx_affine_lift_cells(const float *theta, const int64_t *img_idx, const int32_t *point_batch, int64_t n, int32_t b, int32_t ih,
                                     int32_t iw, int32_t H, int32_t W, int32_t *cells, void *stream) {
  AffSrc S;
  const int64_t none[4] = {0, 0, 0, 0};
  int rc = aff_src("ftx_affine_lift_cells", &S, nullptr, none, b, 1, ih, iw);
  if (rc == FTX_OK) rc = aff_target("ftx_affine_lift_cells", H, W);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 0 && n < 0x7fffffff, "ftx_affine_lift_cells: bad point count");
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(theta && img_idx && point_batch && cells, "ftx_affine_lift_cells: null pointer");
  aff_lift_cells_kernel<<<grid_for(n, 256), 256, 0, (hipStream_t)stream>>>(theta, img_idx, point_batch, n, b, ih, iw, H, W, cells);
  return check_launch("ftx_affine_lift_cells");
}

extern "C" int ftx_affine_lift_bwd(const float *src, const int64_t *src_strides, int32_t b, int32_t c, int32_t ih, int32_t iw,
                                   const float *theta, const int64_t *img_idx, const int32_t *point_batch, const float *grad_out, int64_t n,
                                   int32_t H, int32_t W, const int32_t *order, const int32_t *seg_off, float *grad_src, float *grad_theta,
                                   void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "ftx_affine_lift_bwd";
  AffSrc S;
  int rc = aff_src(who, &S, src, src_strides, b, c, ih, iw);
  if (rc == FTX_OK) rc = aff_target(who, H, W);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 0 && n < 0x7fffffff, "%s: bad point count", who);
  FTX_REQUIRE(theta && (n == 0 || (img_idx && point_batch && grad_out)), "%s: null pointer", who);
  hipStream_t st = (hipStream_t)stream;
  if (grad_src) {
    FTX_REQUIRE(seg_off && (n == 0 || order), "%s: grad_src needs the segments of ftx_affine_lift_cells", who);
    const int chan_inner = S.sc == 1 && c > 1;
    aff_lift_bwd_src_kernel<<<grid_for((int64_t)b * c * ih * iw, 256), 256, 0, st>>>(S, grad_src, theta, img_idx, grad_out, order, seg_off, H, W,
                                                                                    chan_inner);
    rc = check_launch(who);
    if (rc != FTX_OK) return rc;
  }
  if (grad_theta) {
    FTX_REQUIRE(src, "%s: grad_theta needs the source", who);
    rc = aff_workspace(who, b, workspace, workspace_bytes);
    if (rc != FTX_OK) return rc;
    const StreamScratch sc = stream_scratch(st);
    if (!sc.counters) return FTX_ELAUNCH;
    int G = 1;
    while (G < 64 && G < c) G <<= 1;
    const int bpf = aff_blocks_per_frame(b, n, 256 / G);
    aff_theta_kernel<true><<<b * bpf, 256, 0, st>>>(S, theta, grad_out, img_idx, point_batch, n, H, W, G, bpf, (double *)workspace, sc, grad_theta);
    rc = check_launch(who);
  }
  return rc;
}
