// Column sums of a row-major (rows, cols) float32 matrix: the bias gradient of every Linear of the ViT trunk and of the point
// branch (the reference reaches it through autograd's sum_to reduction: models/transformers.py:16-45, timm Mlp / Attention).
// Pass 1: block = up to 256 columns (<= 64 lanes x float4 of a row) x (256 / lanes) row lanes over one chunk of rows -> one float64 partial row;
// pass 2: 16 lanes per column sum the chunk rows (every 16th each, combined in lane order: chunk_rows_sum_kernel, ftx_chunk_rows.h).  Float64
// throughout: the rounding to float32 happens once.
// A (1, M) x (M, N) library GEMM took 14 us for the 2312 x 768..3072 gradients, 48 times per step; these two take 3-6 us together.
#include "ftx_common.h"
#include "ftx_chunk_rows.h"

using namespace ftx;

// geometry of pass 1: c4w float4 column groups per row (<= 64: 1 KB of a row per wave), RL = 256 / c4w row lanes, `chunks` row ranges
struct ColsumGeom {
  int c4w, rl, slab, chunks;
};
static ColsumGeom colsum_geom(int64_t rows, int cols) {
  ColsumGeom g;
  const int c4 = (cols + 3) / 4;
  g.c4w = c4 < 64 ? c4 : 64;
  g.rl = 256 / g.c4w;
  g.slab = g.c4w * 4;
  int64_t ch = ceil_div(rows, (int64_t)g.rl * 8);   // ~8 rows per thread
  if (ch > 256) ch = 256;
  g.chunks = (int)(ch < 1 ? 1 : ch);
  return g;
}
extern "C" size_t ftx_colsum_workspace_bytes(int64_t rows, int32_t cols) {
  if (rows <= 0 || cols <= 0) return 256;
  return sizeof(double) * (size_t)colsum_geom(rows, cols).chunks * (size_t)cols + 256;
}

__global__ __launch_bounds__(256) void colsum_partial_kernel(const float *__restrict__ x, int64_t rows, int cols, int c4w, int RL,
                                                             double *__restrict__ part) {
  __shared__ double sh[1024];   // [RL][slab], RL * slab <= 256 * 4
  const int slab = c4w * 4;
  const int cq = threadIdx.x % c4w, rl = threadIdx.x / c4w;
  const int col = blockIdx.x * slab + cq * 4;
  const int64_t per = ceil_div(rows, (int64_t)gridDim.y);
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = r0 + per < rows ? r0 + per : rows;
  if (rl < RL) {
    double s[4] = {0, 0, 0, 0};
    if (col < cols) {
      int64_t r = r0 + rl;
      for (; r + RL < r1; r += 2 * RL) {   // two rows in flight per thread
        const float4 a = *(const float4 *)&x[r * cols + col], b = *(const float4 *)&x[(r + RL) * cols + col];
        s[0] += (double)a.x; s[1] += (double)a.y; s[2] += (double)a.z; s[3] += (double)a.w;
        s[0] += (double)b.x; s[1] += (double)b.y; s[2] += (double)b.z; s[3] += (double)b.w;
      }
      for (; r < r1; r += RL) {
        const float4 a = *(const float4 *)&x[r * cols + col];
        s[0] += (double)a.x; s[1] += (double)a.y; s[2] += (double)a.z; s[3] += (double)a.w;
      }
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) sh[rl * slab + cq * 4 + v] = s[v];
  }
  __syncthreads();
  for (int j = threadIdx.x; j < slab; j += 256) {
    const int c = blockIdx.x * slab + j;
    if (c < cols) {
      double t = 0;
      for (int q = 0; q < RL; ++q) t += sh[q * slab + j];
      part[(int64_t)blockIdx.y * cols + c] = t;
    }
  }
}

extern "C" int ftx_colsum(const float *x, int64_t rows, int32_t cols, float *out, void *workspace, size_t workspace_bytes, void *stream) {
  FTX_REQUIRE(rows >= 0 && cols >= 4 && cols % 4 == 0, "ftx_colsum: cols must be a positive multiple of 4 (got %d)", cols);
  FTX_REQUIRE(out && workspace && (x || rows == 0), "ftx_colsum: null pointer");
  if (workspace_bytes < ftx_colsum_workspace_bytes(rows, cols)) return workspace_short("ftx_colsum", workspace_bytes, ftx_colsum_workspace_bytes(rows, cols));
  hipStream_t st = (hipStream_t)stream;
  const ColsumGeom g = colsum_geom(rows, cols);
  double *part = (double *)workspace;
  dim3 grid((unsigned)ceil_div(cols, g.slab), (unsigned)g.chunks);
  colsum_partial_kernel<<<grid, 256, 0, st>>>(x, rows, cols, g.c4w, g.rl, part);
  chunk_rows_sum_kernel<<<(unsigned)ceil_div(cols, 16), 256, 0, st>>>(part, g.chunks, cols, out);
  return check_launch("ftx_colsum");
}
