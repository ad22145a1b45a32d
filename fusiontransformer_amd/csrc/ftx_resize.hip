// Image resize of the NuScenes loader on the device: data/nuscenes/nuscenes_dataloader.py:185, image.resize(size, Image.BILINEAR) on
// an 8-bit RGB frame.  The arithmetic is Pillow's libImaging/Resample.c at 8 bits per channel, restated in include/ftx.h: a table of
// integer coefficients per axis (built on the host in double, ftx_resize_coeffs_host), a horizontal pass that rounds and clamps to
// uint8, then a vertical pass on those bytes.  Bit-exact: every sum is a 32-bit integer sum, in any order.
//
// TWO LAUNCHES (horizontal, vertical), not one fused kernel with the intermediate rows in LDS.  A fused block has to hold every
// horizontally resampled source row under its output rows; that count is set by the table (9 rows per output row at 900 -> 225, in_h
// of them at out_h = 1), so a fused kernel needs a size limit or a second path for the ratios that do not fit.  The intermediate of
// the NuScenes case is 1 MB per frame and stays in L2 between the two launches; the pair is latency-sized either way.  A pass whose
// axis keeps its length is not launched; all frames of a batch go through the same launch (blockIdx.z).
//
// Memory: every frame is read as packed RGB with a row pitch at any byte alignment (a crop view): a lane reads the aligned dwords that
// cover 12 bytes (4 pixels) and realigns them with v_alignbyte, as ftx_image.hip does; never a dword without one of its bytes.  The
// intermediate rows are padded to 12 ceil(out_w / 4) bytes, so the vertical pass finds them dword aligned.
//   horizontal  lane = output column, 4 input rows per wave at a time (4 independent load chains, each coefficient used 12 times);
//               the block's 64 columns x ksize coefficients are staged in LDS once (read from the table directly when they exceed 32 KB);
//   vertical    lane = 4 adjacent output pixels, one output row per wave: the row's coefficients are wave-uniform scalar loads.
#include "ftx_common.h"
#include <math.h>
using namespace ftx;

namespace {

constexpr int RS_BLOCK = 256;         // 4 waves
constexpr int RS_COLS = 64;           // horizontal: output columns per block, one per lane
constexpr int RS_ROWS = 4;            // horizontal: input rows a wave works on at a time
constexpr int RS_ROWS_PER_BLOCK = 16;  // horizontal: 4 waves x RS_ROWS
constexpr int RS_LDS_INTS = 8192;     // horizontal: coefficients staged in LDS up to 32 KB
constexpr int RS_PRECISION_BITS = 32 - 8 - 2;

// Pillow's precompute_coeffs for the bilinear filter over the whole axis, in double, in its order of operations.
int resize_ksize(int in, int out) {
  double filterscale = (double)in / out;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;
  return (int)ceil(support) * 2 + 1;
}

inline double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// The 12 bytes at p (any alignment), of which the first nbytes >= 1 are needed, as three little-endian dwords.
__device__ inline void load12(const uint8_t *p, int nbytes, uint32_t w[3]) {
  const uintptr_t addr = (uintptr_t)p;
  const uint32_t sh = (uint32_t)(addr & 3);
  const uint32_t *wp = (const uint32_t *)(p - sh);  // derived from the argument, not from an integer: global (not flat) loads
  const int last = (int)(((addr + nbytes - 1) >> 2) - (addr >> 2));
  const uint32_t d0 = wp[0];
  const uint32_t d1 = last >= 1 ? wp[1] : 0u;
  const uint32_t d2 = last >= 2 ? wp[2] : 0u;
  const uint32_t d3 = last >= 3 ? wp[3] : 0u;
  w[0] = __builtin_amdgcn_alignbyte(d1, d0, sh);
  w[1] = __builtin_amdgcn_alignbyte(d2, d1, sh);
  w[2] = __builtin_amdgcn_alignbyte(d3, d2, sh);
}

// Products are formed with __mul24: a byte times a coefficient of at most 1 << 22 (a normalised weight) is exact in 24-bit operands.
__device__ inline int byte_of(const uint32_t w[3], int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }

__device__ inline int clip8(int acc) { return min(255, max(0, acc >> RS_PRECISION_BITS)); }

// For packing four results into a dword.  hipcc folds clip8(a) | clip8(b) << 8 into v_ashr_pk_u8_i32 and takes the upper 16 bits of
// its result for zero; on the MI355X they held the destination register's earlier contents, which the following OR then merged into
// bytes 2 and 3 (seen as wrong bytes 2, 3, 6 and 10 of every 12).  The empty asm keeps each clipped byte out of that pattern.
__device__ inline uint32_t clip8_for_pack(int acc) {
  uint32_t v = (uint32_t)clip8(acc);
  asm volatile("" : "+v"(v));
  return v;
}

// The table is the caller's: an entry that points outside the axis must not become an address.
__device__ inline void clamp_bounds(int &lo, int &taps, int in, int ksize) {
  lo = min(max(lo, 0), in);
  taps = min(min(max(taps, 0), ksize), in - lo);
}

// grid (ceil(out_w / 64), ceil(in_h / 16), n_frames); dst rows of out_w pixels, dst_pitch bytes apart.
__global__ __launch_bounds__(RS_BLOCK) void resize_horizontal_kernel(const uint8_t *__restrict__ src, int64_t frame_stride, int64_t pitch, int in_h,
                                                                     int in_w, int out_w, const int32_t *__restrict__ bounds,
                                                                     const int32_t *__restrict__ kk, int ksize, int staged,
                                                                     uint8_t *__restrict__ dst, int64_t dst_frame_stride, int64_t dst_pitch) {
  extern __shared__ int32_t s_kk[];  // [tap][column of the block]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = blockIdx.x * RS_COLS;
  if (staged) {
    for (int i = threadIdx.x; i < ksize * RS_COLS; i += RS_BLOCK) {
      const int c = i & (RS_COLS - 1), t = i / RS_COLS;
      s_kk[i] = x0 + c < out_w ? kk[(int64_t)(x0 + c) * ksize + t] : 0;
    }
    __syncthreads();
  }
  const int xx = x0 + lane;
  int xmin = 0, taps = 0;
  if (xx < out_w) {
    xmin = bounds[2 * xx];
    taps = bounds[2 * xx + 1];
    clamp_bounds(xmin, taps, in_w, ksize);
  }
  const int32_t *krow = kk + (int64_t)min(xx, out_w - 1) * ksize;
  const int y0 = blockIdx.y * RS_ROWS_PER_BLOCK + wave * RS_ROWS;
  const uint8_t *frame = src + blockIdx.z * frame_stride;
  const uint8_t *row[RS_ROWS];
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) row[r] = frame + min(y0 + r, in_h - 1) * pitch + 3 * (int64_t)xmin;  // rows past the end: loaded, not stored
  int acc[RS_ROWS][3];
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (RS_PRECISION_BITS - 1);
  for (int t0 = 0; t0 < taps; t0 += 4) {  // 4 taps = 12 source bytes per row
    int k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) k[j] = t0 + j < taps ? (staged ? s_kk[(t0 + j) * RS_COLS + lane] : krow[t0 + j]) : 0;
    const int nbytes = 3 * min(4, taps - t0);
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
      uint32_t w[3];
      load12(row[r] + 3 * t0, nbytes, w);
#pragma unroll
      for (int j = 0; j < 4; ++j)  // bytes past nbytes meet k == 0
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) acc[r][ch] += __mul24(byte_of(w, 3 * j + ch), k[j]);
    }
  }
  if (xx >= out_w) return;
  uint8_t *out = dst + blockIdx.z * dst_frame_stride + 3 * (int64_t)xx;
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) {
    if (y0 + r >= in_h) break;
    uint8_t *o = out + (y0 + r) * dst_pitch;
    o[0] = (uint8_t)clip8(acc[r][0]);
    o[1] = (uint8_t)clip8(acc[r][1]);
    o[2] = (uint8_t)clip8(acc[r][2]);
  }
}

// block (64, 4): grid (ceil(ceil(w / 4) / 64), ceil(out_h / 4), n_frames); src rows of w pixels (the horizontal pass's output or the
// caller's frame), dst (n_frames, out_h, w, 3) contiguous.
__global__ __launch_bounds__(RS_BLOCK) void resize_vertical_kernel(const uint8_t *__restrict__ src, int64_t frame_stride, int64_t pitch, int in_h,
                                                                   int w, int out_h, const int32_t *__restrict__ bounds,
                                                                   const int32_t *__restrict__ kk, int ksize, uint8_t *__restrict__ dst) {
  const int yy = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y);  // one output row per wave: scalar table loads
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (yy >= out_h || x0 >= w) return;
  int ymin = bounds[2 * yy], taps = bounds[2 * yy + 1];
  clamp_bounds(ymin, taps, in_h, ksize);
  const int32_t *krow = kk + (int64_t)yy * ksize;
  const int n = min(4, w - x0);
  const uint8_t *p = src + blockIdx.z * frame_stride + ymin * pitch + 3 * (int64_t)x0;
  int acc[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) acc[j] = 1 << (RS_PRECISION_BITS - 1);
#pragma unroll 2
  for (int t = 0; t < taps; ++t) {
    const int k = krow[t];
    uint32_t wd[3];
    load12(p + t * pitch, 3 * n, wd);
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] += __mul24(byte_of(wd, j), k);
  }
  uint8_t *o = dst + 3 * (((int64_t)blockIdx.z * out_h + yy) * w + x0);
  if (n == 4 && ((uintptr_t)o & 3) == 0) {
    uint32_t *o32 = (uint32_t *)o;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      o32[q] = clip8_for_pack(acc[4 * q]) | (clip8_for_pack(acc[4 * q + 1]) << 8) | (clip8_for_pack(acc[4 * q + 2]) << 16) |
               (clip8_for_pack(acc[4 * q + 3]) << 24);
  } else {
    for (int j = 0; j < 3 * n; ++j) o[j] = (uint8_t)clip8(acc[j]);
  }
}

int64_t padded_pitch(int width) { return 12 * (int64_t)ceil_div(width, 4); }

}  // namespace

extern "C" int32_t ftx_resize_ksize(int32_t in, int32_t out) {
  FTX_REQUIRE(in > 0 && out > 0, "ftx_resize_ksize: sizes must be positive, got in %d out %d", in, out);
  return resize_ksize(in, out);
}

extern "C" int ftx_resize_coeffs_host(int32_t in, int32_t out, int32_t *bounds_host, int32_t *kk_host) {
  FTX_REQUIRE(in > 0 && out > 0, "ftx_resize_coeffs_host: sizes must be positive, got in %d out %d", in, out);
  FTX_REQUIRE(bounds_host && kk_host, "ftx_resize_coeffs_host: null pointer");
  const double in0 = 0.0, in1 = (double)in;
  double filterscale, scale;
  filterscale = scale = (in1 - in0) / out;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;
  const int ksize = (int)ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  double *k = new double[ksize];
  for (int xx = 0; xx < out; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    int x;
    for (x = 0; x < xmax; ++x) {
      const double w = bilinear_filter((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    for (x = 0; x < xmax; ++x)
      if (ww != 0.0) k[x] /= ww;
    for (; x < ksize; ++x) k[x] = 0.0;
    bounds_host[2 * xx] = xmin;
    bounds_host[2 * xx + 1] = xmax;
    for (x = 0; x < ksize; ++x)
      kk_host[(int64_t)xx * ksize + x] =
          k[x] < 0 ? (int)(-0.5 + k[x] * (1 << RS_PRECISION_BITS)) : (int)(0.5 + k[x] * (1 << RS_PRECISION_BITS));
  }
  delete[] k;
  return FTX_OK;
}

extern "C" size_t ftx_resize_workspace_bytes(int32_t n_frames, int32_t in_h, int32_t in_w, int32_t out_h, int32_t out_w) {
  if (n_frames <= 0 || in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0) return 0;
  if (in_h == out_h || in_w == out_w) return 0;  // one pass at most: no intermediate
  return (size_t)n_frames * (size_t)in_h * (size_t)padded_pitch(out_w);
}

extern "C" int ftx_resize_bilinear_u8(const uint8_t *src, int64_t frame_stride, int64_t pitch, int32_t n_frames, int32_t in_h, int32_t in_w,
                                      int32_t channels, const int32_t *bounds_x, const int32_t *kk_x, int32_t ksize_x, const int32_t *bounds_y,
                                      const int32_t *kk_y, int32_t ksize_y, int32_t out_h, int32_t out_w, uint8_t *dst, void *workspace,
                                      size_t workspace_bytes, void *stream) {
  const char *who = "ftx_resize_bilinear_u8";
  FTX_REQUIRE(n_frames >= 0 && n_frames <= 65535, "%s: n_frames %d outside 0..65535", who, n_frames);
  FTX_REQUIRE(in_h > 0 && in_w > 0 && out_h > 0 && out_w > 0, "%s: sizes must be positive, got %d x %d -> %d x %d (w x h)", who, in_w, in_h,
              out_w, out_h);
  FTX_REQUIRE(channels == 3, "%s: channels must be 3 (RGB), got %d", who, channels);
  FTX_REQUIRE(pitch >= 3 * (int64_t)in_w, "%s: row pitch %lld smaller than 3 * width = %lld", who, (long long)pitch, 3 * (long long)in_w);
  FTX_REQUIRE(frame_stride >= 0, "%s: negative frame stride", who);
  const bool do_x = in_w != out_w, do_y = in_h != out_h;
  FTX_REQUIRE(do_x || do_y, "%s: the size does not change (%d x %d): nothing to resample, keep the frame", who, in_w, in_h);
  FTX_REQUIRE(in_h <= 16 * 65535 && out_h <= 4 * 65535, "%s: more than %d rows", who, 4 * 65535);
  if (do_x) {
    FTX_REQUIRE(bounds_x && kk_x, "%s: null pointer (horizontal table)", who);
    FTX_REQUIRE(ksize_x == resize_ksize(in_w, out_w), "%s: ksize_x %d, ftx_resize_ksize(%d, %d) = %d", who, ksize_x, in_w, out_w,
                resize_ksize(in_w, out_w));
  }
  if (do_y) {
    FTX_REQUIRE(bounds_y && kk_y, "%s: null pointer (vertical table)", who);
    FTX_REQUIRE(ksize_y == resize_ksize(in_h, out_h), "%s: ksize_y %d, ftx_resize_ksize(%d, %d) = %d", who, ksize_y, in_h, out_h,
                resize_ksize(in_h, out_h));
  }
  FTX_REQUIRE(src && dst, "%s: null pointer", who);
  const size_t need = ftx_resize_workspace_bytes(n_frames, in_h, in_w, out_h, out_w);
  if (need) {
    FTX_REQUIRE(workspace, "%s: resizing both axes needs the workspace", who);
    FTX_REQUIRE(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    FTX_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
  }
  if (n_frames == 0) return FTX_OK;
  hipStream_t st = (hipStream_t)stream;
  const uint8_t *vsrc = src;  // what the vertical pass reads
  int64_t vstride = frame_stride, vpitch = pitch;
  if (do_x) {
    uint8_t *hdst = dst;
    int64_t hpitch = 3 * (int64_t)out_w;
    if (do_y) {
      hdst = (uint8_t *)workspace;
      hpitch = padded_pitch(out_w);
      vsrc = hdst;
      vpitch = hpitch;
      vstride = in_h * hpitch;
    }
    const int staged = (int64_t)ksize_x * RS_COLS <= RS_LDS_INTS;
    const dim3 grid((unsigned)ceil_div(out_w, RS_COLS), (unsigned)ceil_div(in_h, RS_ROWS_PER_BLOCK), (unsigned)n_frames);
    resize_horizontal_kernel<<<grid, RS_BLOCK, staged ? (size_t)ksize_x * RS_COLS * sizeof(int32_t) : 0, st>>>(
        src, frame_stride, pitch, in_h, in_w, out_w, bounds_x, kk_x, ksize_x, staged, hdst, in_h * hpitch, hpitch);
  }
  if (do_y) {
    const dim3 grid((unsigned)ceil_div(ceil_div(out_w, 4), 64), (unsigned)ceil_div(out_h, 4), (unsigned)n_frames);
    resize_vertical_kernel<<<grid, dim3(64, 4), 0, st>>>(vsrc, vstride, vpitch, in_h, out_w, out_h, bounds_y, kk_y, ksize_y, dst);
  }
  return check_launch(who);
}
