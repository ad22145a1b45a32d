// The convolutional part of the spatial transformers' localisation net (models/transformers.py:106-114 of the reference), one fused
// layer at a time:   y = relu(max_pool2d(conv2d(x, w, bias), 2, 2))   for a stride-1, unpadded k x k convolution.
// Served (k, co): (7, 8) -- Conv2d(C, 8, 7) -- and (5, 90) -- Conv2d(8, 90, 5); any c >= 1, any size with a pooled pixel.
//
// What exists in memory: x, the pooled map (or, for the second layer, only its per-(frame, channel) mean) and one routing byte per
// pooled element: sel = 0..3, the row-major position of the 2 x 2 window's maximum (the first on a tie, as torch's pool chooses), or
// -1 where that maximum is <= 0 or NaN (the ReLU is dead: no gradient).  The un-pooled (b, co, oh, ow) map never exists, neither in the
// forward nor in the backward.  The conv row / column that the pool drops on an odd size is never computed.
//
// x (and dX) are described by element strides (frame, channel, row, column) like AffSrc in ftx_stn.hip: NCHW and channels-last are the
// same code.  The pooled gradient is strided too, so the mean's backward is a stride-0 broadcast with no tensor behind it.
//
// Arithmetic: float32 operands, products accumulated with explicit fmaf() in a fixed order (channel, tap row, tap column) -- packed /
// plain VALU FMA, weights arrive through wave-uniform loads.  Floating-point contraction is OFF in this file: the only fused
// operations are the fmaf() calls that are written out.  Forward: float32 accumulators of LOC_CH channels are flushed to float64
// totals, so the rounding of a 4704-term sum is that of its 196-term pieces.  Weight gradient: float32 over one 16 x 16 pooled tile,
// float64 across tiles and across blocks (per-block partials in the caller's workspace, added in block order by a second kernel).
// Data gradient: float32 over one pass of <= 10 output channels, float64 across the passes.
// No float atomics anywhere; every order of summation depends on the sizes only, so every output repeats bit for bit.
#include "ftx_common.h"
#include "ftx_reduce.h"

#pragma clang fp contract(off)

using namespace ftx;

namespace {

constexpr int LOC_T = 16;        // a block's tile: 16 x 16 pooled pixels (forward, weight gradient) or 16 x 16 input pixels (data gradient)
constexpr int LOC_CH = 4;        // input channels staged in LDS at a time (forward, weight gradient)
constexpr int LOC_MAX_B = 128;
constexpr int LOC_WG_BLOCKS = 512;   // target number of blocks of a weight-gradient launch
constexpr int LOC_MAX_SPLIT = 256;

struct LocX {
  const float *p;
  int64_t sb, sc, sy, sx;   // element strides of (frame, channel, row, column)
  int b, c, ih, iw;
};

struct LocG {               // the pooled gradient (b, co, ph, pw) by element strides; 0 strides broadcast
  const float *p;
  int64_t sb, sc, sy, sx;
};

struct LocGO {              // one pooled gradient routed to its conv position: g (0 when the ReLU is dead), off = dy * pitch + dx
  float g;
  int off;
};

template <int K>
struct LocGeom {
  static constexpr int E = 2 * LOC_T + K - 1;   // input rows / columns under a tile of pooled pixels: 38 (k = 7), 36 (k = 5)
  static constexpr int P = E + (E & 1);         // even pitch: a thread's (2 px, 2 px + 1) pair is one 8-byte LDS read
};

// Stages channels ch0 .. ch0 + LOC_CH of the E x E input window at (y0, x0) of frame f; zero outside the image / past the last channel.
template <int K>
__device__ inline void loc_stage_x(const LocX &X, int f, int ch0, int y0, int x0, float *__restrict__ xt, int tid, int nthreads) {
  constexpr int E = LocGeom<K>::E, P = LocGeom<K>::P;
  const bool chan_inner = X.sc == 1 && X.c > 1;
  for (int e = tid; e < LOC_CH * E * E; e += nthreads) {
    int cc, r, col;
    if (chan_inner) {
      cc = e % LOC_CH;
      const int q = e / LOC_CH;
      col = q % E;
      r = q / E;
    } else {
      col = e % E;
      const int q = e / E;
      r = q % E;
      cc = q / E;
    }
    const int ch = ch0 + cc, y = y0 + r, x = x0 + col;
    float v = 0.f;
    if (ch < X.c && y < X.ih && x < X.iw) v = X.p[(int64_t)f * X.sb + (int64_t)ch * X.sc + (int64_t)y * X.sy + (int64_t)x * X.sx];
    xt[(cc * E + r) * P + col] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------------- forward
// Block (tile, co group, frame): 256 threads = 16 x 16 pooled pixels, each with the 2 x 2 conv window of COT output channels.
template <int K, int COT>
__global__ __launch_bounds__(256) void loc_fwd_kernel(LocX X, const float *__restrict__ w, const float *__restrict__ bias, int co, int ph, int pw,
                                                      int tiles_x, float *__restrict__ out, int8_t *__restrict__ sel,
                                                      double *__restrict__ part) {
  constexpr int E = LocGeom<K>::E, P = LocGeom<K>::P, KK = K * K;
  __shared__ __align__(16) float xt[LOC_CH * E * P];
  __shared__ double red[256];
  const int tid = threadIdx.x, lx = tid & (LOC_T - 1), ly = tid >> 4;
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int co0 = blockIdx.y * COT, f = blockIdx.z;
  const int py = ty * LOC_T + ly, px = tx * LOC_T + lx;
  const int64_t wco = (int64_t)X.c * KK;   // weight stride of an output channel

  double tot[2][2][COT];
#pragma unroll
  for (int j = 0; j < COT; ++j) tot[0][0][j] = tot[0][1][j] = tot[1][0][j] = tot[1][1][j] = 0.0;

  for (int ch0 = 0; ch0 < X.c; ch0 += LOC_CH) {
    __syncthreads();
    loc_stage_x<K>(X, f, ch0, ty * 2 * LOC_T, tx * 2 * LOC_T, xt, tid, 256);
    __syncthreads();
    float acc[2][2][COT];
#pragma unroll
    for (int j = 0; j < COT; ++j) acc[0][0][j] = acc[0][1][j] = acc[1][0][j] = acc[1][1][j] = 0.f;
    const int nch = X.c - ch0 < LOC_CH ? X.c - ch0 : LOC_CH;
    for (int cc = 0; cc < nch; ++cc) {
      const float *__restrict__ wp = w + (int64_t)co0 * wco + (int64_t)(ch0 + cc) * KK;
      const float *__restrict__ xr = xt + (cc * E + 2 * ly) * P + 2 * lx;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        float in0[K + 1], in1[K + 1];   // input rows 2 py + ky and 2 py + ky + 1, columns 2 px .. 2 px + K
#pragma unroll
        for (int q = 0; q < (K + 1) / 2; ++q) {
          const float2 a = *reinterpret_cast<const float2 *>(xr + ky * P + 2 * q);
          const float2 c2 = *reinterpret_cast<const float2 *>(xr + (ky + 1) * P + 2 * q);
          in0[2 * q] = a.x; in0[2 * q + 1] = a.y;
          in1[2 * q] = c2.x; in1[2 * q + 1] = c2.y;
        }
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
#pragma unroll
          for (int j = 0; j < COT; ++j) {
            const float wv = wp[j * wco + ky * K + kx];
            acc[0][0][j] = fmaf(in0[kx], wv, acc[0][0][j]);
            acc[0][1][j] = fmaf(in0[kx + 1], wv, acc[0][1][j]);
            acc[1][0][j] = fmaf(in1[kx], wv, acc[1][0][j]);
            acc[1][1][j] = fmaf(in1[kx + 1], wv, acc[1][1][j]);
          }
        }
      }
    }
#pragma unroll
    for (int j = 0; j < COT; ++j) {
      tot[0][0][j] += (double)acc[0][0][j];
      tot[0][1][j] += (double)acc[0][1][j];
      tot[1][0][j] += (double)acc[1][0][j];
      tot[1][1][j] += (double)acc[1][1][j];
    }
  }

  const bool live = py < ph && px < pw;
#pragma unroll
  for (int j = 0; j < COT; ++j) {
    const double bj = bias ? (double)bias[co0 + j] : 0.0;
    const float v[4] = {(float)(tot[0][0][j] + bj), (float)(tot[0][1][j] + bj), (float)(tot[1][0][j] + bj), (float)(tot[1][1][j] + bj)};
    float m = v[0];
    int idx = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (v[q] > m || v[q] != v[q]) {   // torch's pool: a later value wins only when greater; a NaN always wins
        m = v[q];
        idx = q;
      }
    const float y = m > 0.f ? m : (m != m ? m : 0.f);
    if (live) {
      const int64_t o = (((int64_t)f * co + co0 + j) * ph + py) * pw + px;
      sel[o] = (int8_t)(m > 0.f ? idx : -1);
      if (out) out[o] = y;
    }
    if (part) {   // the mean form: this block's sum of channel co0 + j, a fixed tree over the 256 threads
      __syncthreads();
      red[tid] = live ? (double)y : 0.0;
      __syncthreads();
      for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
      }
      if (tid == 0) part[((int64_t)f * co + co0 + j) * gridDim.x + tile] = red[0];
    }
  }
}

// mean[f, co] = (sum of the tiles' partial sums, in tile order per lane, then a fixed tree) / (ph pw).  One wave per (frame, channel).
__global__ __launch_bounds__(64) void loc_mean_kernel(const double *__restrict__ part, int tiles, double inv, float *__restrict__ mean) {
  const double *row = part + (int64_t)blockIdx.x * tiles;
  double v = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) v += row[t];
  v = wave_sum_down(v);
  if (threadIdx.x == 0) mean[blockIdx.x] = (float)(v * inv);
}

// ---------------------------------------------------------------------------------------------------------------- weight gradient
// dW[co, c, ky, kx] = sum over (frame, pooled pixel) of g routed to its conv position (2 py + dy, 2 px + dx) times
// x[c, 2 py + dy + ky, 2 px + dx + kx].  Block (channel chunk, split s, co group): thread (j, ky, kx) owns that tap of LOC_CH input
// channels and walks the tiles s, s + S, s + 2 S, ... of all frames; per tile float32 over the 256 pooled pixels, float64 across tiles.
// Its sums go to row s of the partials; loc_wgrad_sum_kernel adds the rows in order.  Chunk 0 also sums g itself (db).
template <int K, int COT, int NT>
__global__ __launch_bounds__(NT) void loc_wgrad_kernel(LocX X, const int8_t *__restrict__ sel, LocG G, int co, int ph, int pw, int tiles_x,
                                                       int tiles, double *__restrict__ part_w, double *__restrict__ part_b) {
  constexpr int E = LocGeom<K>::E, P = LocGeom<K>::P, KK = K * K;
  __shared__ __align__(16) float xt[LOC_CH * E * P];
  __shared__ __align__(16) LocGO gl[LOC_T * LOC_T * COT];
  const int tid = threadIdx.x;
  const int ch0 = blockIdx.x * LOC_CH, s = blockIdx.y, S = gridDim.y, co0 = blockIdx.z * COT;
  const bool owner = tid < COT * KK;
  const int j = owner ? tid / KK : 0, t = owner ? tid - j * KK : 0, ky = t / K, kx = t - ky * K;
  const int tap = ky * P + kx;
  const bool with_db = blockIdx.x == 0 && owner && t == 0;
  double d[LOC_CH] = {0.0, 0.0, 0.0, 0.0}, dbias = 0.0;

  for (int item = s; item < X.b * tiles; item += S) {
    const int f = item / tiles, tile = item - f * tiles, ty = tile / tiles_x, tx = tile - ty * tiles_x;
    __syncthreads();
    loc_stage_x<K>(X, f, ch0, ty * 2 * LOC_T, tx * 2 * LOC_T, xt, tid, NT);
    for (int e = tid; e < LOC_T * LOC_T * COT; e += NT) {   // e = jj * 256 + p: coalesced over the pooled pixels of a channel
      const int jj = e / (LOC_T * LOC_T), p = e - jj * (LOC_T * LOC_T);
      const int py = ty * LOC_T + (p >> 4), px = tx * LOC_T + (p & 15);
      LocGO v = {0.f, 0};
      if (py < ph && px < pw) {
        const int r = sel[(((int64_t)f * co + co0 + jj) * ph + py) * pw + px];
        if (r >= 0 && r < 4) {
          v.g = G.p[(int64_t)f * G.sb + (int64_t)(co0 + jj) * G.sc + (int64_t)py * G.sy + (int64_t)px * G.sx];
          v.off = (r >> 1) * P + (r & 1);
        }
      }
      gl[p * COT + jj] = v;
    }
    __syncthreads();
    if (owner) {
      float a[LOC_CH] = {0.f, 0.f, 0.f, 0.f};
      for (int p = 0; p < LOC_T * LOC_T; ++p) {
        const LocGO v = gl[p * COT + j];
        const float *xr = xt + (2 * (p >> 4)) * P + 2 * (p & 15) + v.off + tap;
#pragma unroll
        for (int cc = 0; cc < LOC_CH; ++cc) a[cc] = fmaf(v.g, xr[cc * E * P], a[cc]);
      }
#pragma unroll
      for (int cc = 0; cc < LOC_CH; ++cc) d[cc] += (double)a[cc];
      if (with_db) {
        float sb = 0.f;
        for (int p = 0; p < LOC_T * LOC_T; ++p) sb += gl[p * COT + j].g;
        dbias += (double)sb;
      }
    }
  }
  if (owner) {
#pragma unroll
    for (int cc = 0; cc < LOC_CH; ++cc)
      if (ch0 + cc < X.c) part_w[(((int64_t)s * co + co0 + j) * X.c + ch0 + cc) * KK + t] = d[cc];
    if (with_db) part_b[(int64_t)s * co + co0 + j] = dbias;
  }
}

__global__ __launch_bounds__(256) void loc_wgrad_sum_kernel(const double *__restrict__ part_w, const double *__restrict__ part_b, int S, int64_t nw,
                                                            int co, float *__restrict__ dw, float *__restrict__ db) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < nw + co; e += (int64_t)gridDim.x * blockDim.x) {
    double v = 0.0;
    if (e < nw) {
      for (int s = 0; s < S; ++s) v += part_w[(int64_t)s * nw + e];
      dw[e] = (float)v;
    } else {
      for (int s = 0; s < S; ++s) v += part_b[(int64_t)s * co + (e - nw)];
      db[e - nw] = (float)v;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ data gradient
// dX[c, y, x] = sum over (co, pooled pixel) whose routed conv position (2 py + dy, 2 px + dx) lies within k - 1 up / left of (y, x) of
// g * w[co, c, y - 2 py - dy, x - 2 px - dx]: the gather form, one thread per input pixel and CT channels, every element written once.
// Exactly (K + 1) / 2 pooled rows (columns) can reach a given y (x): ceil((y - K) / 2) + 0 .. (K - 1) / 2.
// Block (tile of 16 x 16 input pixels, channel chunk, frame); the output channels pass through LDS COC at a time, in order.
template <int K, int COC, int CT>
__global__ __launch_bounds__(256) void loc_dgrad_kernel(LocX X, const float *__restrict__ w, const int8_t *__restrict__ sel, LocG G, int co, int ph,
                                                        int pw, int tiles_x, float *__restrict__ dx) {
  constexpr int KK = K * K, NPC = (K + 1) / 2, HALF = (K - 1) / 2, PRN = LOC_T / 2 + HALF;
  __shared__ __align__(16) float wl[COC * KK * CT];
  __shared__ __align__(16) LocGO gl[PRN * PRN * COC];   // off = dy * 2 + dx here
  const int tid = threadIdx.x, lx = tid & (LOC_T - 1), ly = tid >> 4;
  const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int c0 = blockIdx.y * CT, f = blockIdx.z;
  const int y = ty * LOC_T + ly, x = tx * LOC_T + lx;
  const int pby = ty * (LOC_T / 2) - HALF, pbx = tx * (LOC_T / 2) - HALF;   // first pooled row / column of the staged region
  const int qy = ((ly - K + 1) >> 1) + HALF, qx = ((lx - K + 1) >> 1) + HALF;   // this thread's first candidate, local
  double tot[CT];   // float32 over the <= NPC^2 COC terms of one pass of output channels, float64 across the passes
#pragma unroll
  for (int cc = 0; cc < CT; ++cc) tot[cc] = 0.0;

  for (int co0 = 0; co0 < co; co0 += COC) {
    float acc[CT];
#pragma unroll
    for (int cc = 0; cc < CT; ++cc) acc[cc] = 0.f;
    __syncthreads();
    for (int e = tid; e < COC * KK * CT; e += 256) {   // wl[(jj, t, cc)] <- w[co0 + jj, c0 + cc, t]
      const int cc = e % CT, q = e / CT, t = q % KK, jj = q / KK;
      float v = 0.f;
      if (co0 + jj < co && c0 + cc < X.c) v = w[((int64_t)(co0 + jj) * X.c + c0 + cc) * KK + t];
      wl[e] = v;
    }
    for (int e = tid; e < PRN * PRN * COC; e += 256) {   // e = jj * PRN^2 + region pixel
      const int jj = e / (PRN * PRN), q = e - jj * (PRN * PRN), ry = q / PRN, rx = q - ry * PRN;
      const int py = pby + ry, px = pbx + rx;
      LocGO v = {0.f, -1};
      if (co0 + jj < co && py >= 0 && py < ph && px >= 0 && px < pw) {
        const int r = sel[(((int64_t)f * co + co0 + jj) * ph + py) * pw + px];
        if (r >= 0 && r < 4) {
          v.g = G.p[(int64_t)f * G.sb + (int64_t)(co0 + jj) * G.sc + (int64_t)py * G.sy + (int64_t)px * G.sx];
          v.off = r;
        }
      }
      gl[q * COC + jj] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int iy = 0; iy < NPC; ++iy) {
      const int ry = qy + iy, ky0 = y - 2 * (pby + ry);   // tap row when dy = 0
#pragma unroll 1
      for (int ix = 0; ix < NPC; ++ix) {
        const int rx = qx + ix, kx0 = x - 2 * (pbx + rx);
        const LocGO *__restrict__ gp = gl + (ry * PRN + rx) * COC;
        for (int jj = 0; jj < COC; ++jj) {
          const LocGO v = gp[jj];
          const int ky = ky0 - (v.off >> 1), kx = kx0 - (v.off & 1);
          if (v.off >= 0 && ky >= 0 && ky < K && kx >= 0 && kx < K) {
            const float *__restrict__ wr = wl + (jj * KK + ky * K + kx) * CT;
#pragma unroll
            for (int cc = 0; cc < CT; ++cc) acc[cc] = fmaf(v.g, wr[cc], acc[cc]);
          }
        }
      }
    }
#pragma unroll
    for (int cc = 0; cc < CT; ++cc) tot[cc] += (double)acc[cc];
  }
  if (y < X.ih && x < X.iw) {
#pragma unroll
    for (int cc = 0; cc < CT; ++cc)
      if (c0 + cc < X.c) dx[(int64_t)f * X.sb + (int64_t)(c0 + cc) * X.sc + (int64_t)y * X.sy + (int64_t)x * X.sx] = (float)tot[cc];
  }
}

// ------------------------------------------------------------------------------------------------------------------------- host
int loc_shape(const char *who, LocX *X, const float *x, const int64_t *strides, int b, int c, int ih, int iw, int k, int co, int *ph, int *pw) {
  FTX_REQUIRE((k == 7 && co == 8) || (k == 5 && co == 90), "%s: (k, co) = (%d, %d) is not served: (7, 8) and (5, 90) are", who, k, co);
  FTX_REQUIRE(b >= 1 && c >= 1 && ih >= 1 && iw >= 1, "%s: bad input size", who);
  FTX_REQUIRE(b <= LOC_MAX_B, "%s: more than %d frames", who, LOC_MAX_B);
  FTX_REQUIRE(ih < 32768 && iw < 32768 && c < 65536, "%s: input too large", who);
  *ph = (ih - k + 1) / 2;
  *pw = (iw - k + 1) / 2;
  FTX_REQUIRE(ih >= k && iw >= k && *ph >= 1 && *pw >= 1, "%s: a %d x %d input has no pooled pixel under a %d x %d kernel", who, ih, iw, k, k);
  FTX_REQUIRE(strides, "%s: null strides", who);
  for (int d = 0; d < 4; ++d) FTX_REQUIRE(strides[d] >= 0, "%s: negative stride", who);
  X->p = x;
  X->sb = strides[0]; X->sc = strides[1]; X->sy = strides[2]; X->sx = strides[3];
  X->b = b; X->c = c; X->ih = ih; X->iw = iw;
  return FTX_OK;
}

int loc_grad(const char *who, LocG *G, const float *g, const int64_t *strides) {
  FTX_REQUIRE(g && strides, "%s: null gradient or gradient strides", who);
  for (int d = 0; d < 4; ++d) FTX_REQUIRE(strides[d] >= 0, "%s: negative gradient stride", who);
  G->p = g;
  G->sb = strides[0]; G->sc = strides[1]; G->sy = strides[2]; G->sx = strides[3];
  return FTX_OK;
}

int loc_tiles(int n) { return (int)ceil_div(n, LOC_T); }

// The split of a weight-gradient launch: a function of the sizes only (the size query and the launch must agree).
int loc_wgrad_split(int b, int c, int ph, int pw, int k, int co) {
  const int64_t items = (int64_t)b * loc_tiles(ph) * loc_tiles(pw);
  const int64_t fixed = ceil_div(c, LOC_CH) * (k == 7 ? 1 : 9);
  int64_t s = LOC_WG_BLOCKS / fixed;
  if (s > LOC_MAX_SPLIT) s = LOC_MAX_SPLIT;
  if (s > items) s = items;
  return s < 1 ? 1 : (int)s;
}

int loc_workspace(const char *who, void *workspace, size_t have, size_t need) {
  FTX_REQUIRE(workspace, "%s: null workspace", who);
  if (have < need) return workspace_short(who, have, need);
  return FTX_OK;
}

}  // namespace

extern "C" size_t ftx_loc_conv_pool_relu_fwd_workspace_bytes(int32_t b, int32_t co, int32_t ph, int32_t pw) {
  if (b < 1 || b > LOC_MAX_B || co < 1 || ph < 1 || pw < 1) return 0;
  return sizeof(double) * (size_t)b * co * loc_tiles(ph) * loc_tiles(pw);   // the mean form's per-tile sums
}

extern "C" int ftx_loc_conv_pool_relu_fwd(const float *x, const int64_t *x_strides, int32_t b, int32_t c, int32_t ih, int32_t iw, const float *w,
                                          const float *bias, int32_t k, int32_t co, float *out, int8_t *sel, float *mean, void *workspace,
                                          size_t workspace_bytes, void *stream) {
  const char *who = "ftx_loc_conv_pool_relu_fwd";
  LocX X;
  int ph, pw;
  int rc = loc_shape(who, &X, x, x_strides, b, c, ih, iw, k, co, &ph, &pw);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(x && w && sel, "%s: null pointer", who);
  FTX_REQUIRE((out != nullptr) != (mean != nullptr), "%s: exactly one of out (the pooled map) and mean must be given", who);
  double *part = nullptr;
  if (mean) {
    rc = loc_workspace(who, workspace, workspace_bytes, ftx_loc_conv_pool_relu_fwd_workspace_bytes(b, co, ph, pw));
    if (rc != FTX_OK) return rc;
    part = (double *)workspace;
  }
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = loc_tiles(pw), tiles = tiles_x * loc_tiles(ph);
  if (k == 7)
    loc_fwd_kernel<7, 8><<<dim3(tiles, 1, b), 256, 0, st>>>(X, w, bias, co, ph, pw, tiles_x, out, sel, part);
  else
    loc_fwd_kernel<5, 10><<<dim3(tiles, 9, b), 256, 0, st>>>(X, w, bias, co, ph, pw, tiles_x, out, sel, part);
  rc = check_launch(who);
  if (rc != FTX_OK || !mean) return rc;
  loc_mean_kernel<<<b * co, 64, 0, st>>>(part, tiles, 1.0 / ((double)ph * (double)pw), mean);
  return check_launch(who);
}

extern "C" size_t ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes(int32_t b, int32_t c, int32_t ih, int32_t iw, int32_t k, int32_t co) {
  if (!((k == 7 && co == 8) || (k == 5 && co == 90)) || b < 1 || b > LOC_MAX_B || c < 1 || ih < k + 1 || iw < k + 1) return 0;
  const int ph = (ih - k + 1) / 2, pw = (iw - k + 1) / 2;
  return sizeof(double) * (size_t)loc_wgrad_split(b, c, ph, pw, k, co) * ((size_t)co * c * k * k + co);   // rows of dW partials, then of db
}

extern "C" int ftx_loc_conv_pool_relu_bwd_weight(const float *x, const int64_t *x_strides, int32_t b, int32_t c, int32_t ih, int32_t iw,
                                                 const int8_t *sel, const float *grad, const int64_t *grad_strides, int32_t k, int32_t co,
                                                 float *grad_w, float *grad_bias, void *workspace, size_t workspace_bytes, void *stream) {
  const char *who = "ftx_loc_conv_pool_relu_bwd_weight";
  LocX X;
  LocG G;
  int ph, pw;
  int rc = loc_shape(who, &X, x, x_strides, b, c, ih, iw, k, co, &ph, &pw);
  if (rc == FTX_OK) rc = loc_grad(who, &G, grad, grad_strides);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(x && sel && grad_w && grad_bias, "%s: null pointer", who);
  rc = loc_workspace(who, workspace, workspace_bytes, ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes(b, c, ih, iw, k, co));
  if (rc != FTX_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int S = loc_wgrad_split(b, c, ph, pw, k, co);
  const int64_t nw = (int64_t)co * c * k * k;
  double *part_w = (double *)workspace, *part_b = part_w + (int64_t)S * nw;
  const int tiles_x = loc_tiles(pw), tiles = tiles_x * loc_tiles(ph), chunks = (int)ceil_div(c, LOC_CH);
  if (k == 7)
    loc_wgrad_kernel<7, 8, 448><<<dim3(chunks, S, 1), 448, 0, st>>>(X, sel, G, co, ph, pw, tiles_x, tiles, part_w, part_b);
  else
    loc_wgrad_kernel<5, 10, 256><<<dim3(chunks, S, 9), 256, 0, st>>>(X, sel, G, co, ph, pw, tiles_x, tiles, part_w, part_b);
  rc = check_launch(who);
  if (rc != FTX_OK) return rc;
  loc_wgrad_sum_kernel<<<grid_for(nw + co, 256), 256, 0, st>>>(part_w, part_b, S, nw, co, grad_w, grad_bias);
  return check_launch(who);
}

extern "C" int ftx_loc_conv_pool_relu_bwd_data(const float *w, const int8_t *sel, const float *grad, const int64_t *grad_strides, int32_t b,
                                               int32_t c, int32_t ih, int32_t iw, int32_t k, int32_t co, float *grad_x,
                                               const int64_t *grad_x_strides, void *stream) {
  const char *who = "ftx_loc_conv_pool_relu_bwd_data";
  LocX X;
  LocG G;
  int ph, pw;
  int rc = loc_shape(who, &X, nullptr, grad_x_strides, b, c, ih, iw, k, co, &ph, &pw);
  if (rc == FTX_OK) rc = loc_grad(who, &G, grad, grad_strides);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(w && sel && grad_x, "%s: null pointer", who);
  hipStream_t st = (hipStream_t)stream;
  const int tiles_x = loc_tiles(iw), tiles = tiles_x * loc_tiles(ih);
  if (k == 7)
    loc_dgrad_kernel<7, 8, 16><<<dim3(tiles, (unsigned)ceil_div(c, 16), b), 256, 0, st>>>(X, w, sel, G, co, ph, pw, tiles_x, grad_x);
  else
    loc_dgrad_kernel<5, 10, 8><<<dim3(tiles, (unsigned)ceil_div(c, 8), b), 256, 0, st>>>(X, w, sel, G, co, ph, pw, tiles_x, grad_x);
  return check_launch(who);
}
