// BatchNorm1d over the rows of a voxel/point feature matrix, fused with the optional
// residual add and ReLU that follow it in every SPVCNN block
// (models/spvcnn.py:30-31,71-79,100-102,164-180).  HBM-bound: x is read twice in the
// forward (statistics, apply) and the output written once; statistics accumulate in
// float64 so mean/var do not depend on how rows are split over workgroups.
#include "ftx_common.h"
#include "ftx_bn_eval_op.h"
#include "ftx_lastblock.h"

using namespace ftx;

// Grid of the statistics passes.  They stream 1-3 row matrices once and are bound by loads in flight, not by bytes: at 128 rows per
// block the 81k-row level ran 635 blocks (2.5 per CU) and reached 1.7 TB/s.  48 rows per block, at most 2048 blocks: constants, because
// the grid fixes the summation tree and with it the bits of the statistics (sweeps: DESIGN.md section 5, rounds 2 and 3).
static int bn_blocks(int64_t n) {
  constexpr int rows = 48, maxb = 2048;
  int64_t b = ceil_div(n, rows);
  if (b > maxb) b = maxb;
  if (b > LB_GROUP * LB_MAX_GROUPS) b = LB_GROUP * LB_MAX_GROUPS;
  if (b < 1) b = 1;
  return (int)b;
}

extern "C" size_t ftx_bn_workspace_bytes(int64_t n, int32_t c) {
  if (c <= 0) return 256;
  return sizeof(double) * (size_t)bn_blocks(n) * 2 * c + sizeof(double) * 2 * c;
}

// Per-block partial column sums of two quantities (q0, q1) produced by `Op` for each element.
//   forward:  q0 = x,        q1 = x*x
//   backward: q0 = dy,       q1 = dy * xhat      (dy masked by y>0 when relu)
// y = (x - mean) * invstd * gamma + beta with the rounding of every step pinned (no contraction left to the compiler): the forward apply
// pass and the ReLU mask the backward RECOMPUTES from x (instead of reading y back: a third of the backward's traffic for the
// BatchNorm + ReLU layers that have no residual) must agree to the last bit.
__device__ inline float bn_affine(float x, float mean, float invstd, float gamma, float beta) {
  return __fmaf_rn(__fmul_rn(__fsub_rn(x, mean), invstd), gamma, beta);
}

struct FwdOp {
  __device__ static void eval(float x, float, float, float, float, float, float, int, double &q0, double &q1) {
    q0 = (double)x;
    q1 = (double)x * (double)x;
  }
};
// relu: 0 none, 1 mask from the stored forward output y, 2 mask recomputed from x (no residual went into y)
struct BwdOp {
  __device__ static void eval(float x, float gy, float y, float mean, float invstd, float gamma, float beta, int relu, double &q0, double &q1) {
    if (relu == 2) y = bn_affine(x, mean, invstd, gamma, beta);
    float dy = (relu && !(y > 0.f)) ? 0.f : gy;
    q0 = (double)dy;
    q1 = (double)dy * (double)((x - mean) * invstd);
  }
};

template <class Op>
__global__ __launch_bounds__(256) void bn_partial_kernel(const float *__restrict__ x, const float *__restrict__ gy,
                                                         const float *__restrict__ y, const float *__restrict__ mean,
                                                         const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                         const float *__restrict__ beta, int relu, int64_t n, int c,
                                                         double *part, StreamScratch sc) {
  // part: gridDim.x rows [2][c], then the totals row [2][c] written by the last block to finish (ftx_lastblock.h)
  extern __shared__ double sh[];  // [2][RL][c]
  const auto [c4, RL] = row_lanes(c);
  const int tid = threadIdx.x;
  const int cg = tid % c4, rl = tid / c4;
  const int64_t rows_per_block = ceil_div(n, (int64_t)gridDim.x);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = (r0 + rows_per_block < n) ? r0 + rows_per_block : n;
  double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  if (rl < RL) {
    float4 mu = make_float4(0, 0, 0, 0), is = mu, gm = mu, bt = mu;
    if (mean) {
      mu = *(const float4 *)&mean[cg * 4];
      is = *(const float4 *)&invstd[cg * 4];
    }
    if (relu == 2) {
      gm = *(const float4 *)&gamma[cg * 4];
      bt = *(const float4 *)&beta[cg * 4];
    }
    auto accumulate = [&](const float4 &xv, const float4 &gv, const float4 &yv) {
      double a, b;
      Op::eval(xv.x, gv.x, yv.x, mu.x, is.x, gm.x, bt.x, relu, a, b); s0[0] += a; s1[0] += b;
      Op::eval(xv.y, gv.y, yv.y, mu.y, is.y, gm.y, bt.y, relu, a, b); s0[1] += a; s1[1] += b;
      Op::eval(xv.z, gv.z, yv.z, mu.z, is.z, gm.z, bt.z, relu, a, b); s0[2] += a; s1[2] += b;
      Op::eval(xv.w, gv.w, yv.w, mu.w, is.w, gm.w, bt.w, relu, a, b); s0[3] += a; s1[3] += b;
    };
    const float4 zero4 = make_float4(0, 0, 0, 0);
    int64_t r = r0 + rl;
    for (; r + RL < r1; r += 2 * RL) {   // two rows per trip: six independent 16-byte loads in flight per thread, summed in row order
      const int64_t o0 = r * c + cg * 4, o1 = (r + RL) * c + cg * 4;
      const float4 xa = *(const float4 *)&x[o0], xb = *(const float4 *)&x[o1];
      const float4 ga = gy ? *(const float4 *)&gy[o0] : zero4, gb = gy ? *(const float4 *)&gy[o1] : zero4;
      const float4 ya = y ? *(const float4 *)&y[o0] : zero4, yb = y ? *(const float4 *)&y[o1] : zero4;
      accumulate(xa, ga, ya);
      accumulate(xb, gb, yb);
    }
    for (; r < r1; r += RL) {
      const int64_t o0 = r * c + cg * 4;
      accumulate(*(const float4 *)&x[o0], gy ? *(const float4 *)&gy[o0] : zero4, y ? *(const float4 *)&y[o0] : zero4);
    }
  }
  colstats_block_tail(s0, s1, rl, cg, RL, c, sh, part, sc);
}

// mean / invstd of a column from its two totals, in float64 (every apply block computes the same values; block 0 also stores them
// and updates the running statistics -- the work of the former finalize launch).
__device__ inline void bn_column_stats(double s, double ss, int64_t n, float eps, float &mean, float &invstd, double &var_out) {
  const double m = s / (double)n;
  double var = ss / (double)n - m * m;
  if (var < 0) var = 0;
  mean = (float)m;
  invstd = (float)(1.0 / sqrt(var + (double)eps));
  var_out = var;
}

// Apply passes: thread (column group cg, row lane rl) keeps its four channels' constants in registers and walks rows rl, rl + RL*grid, ...
// two at a time (independent 16-byte loads in flight); RL = 256 / (c/4) rows per block and trip.
__global__ __launch_bounds__(256) void bn_apply_fwd_kernel(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const double *__restrict__ totals, float eps,
                                                           float momentum, float *__restrict__ running_mean, float *__restrict__ running_var,
                                                           float *__restrict__ save_mean, float *__restrict__ save_invstd, int64_t n, int c,
                                                           int relu, float *__restrict__ y) {
  const auto [c4, RL] = row_lanes(c);
  const int cg = threadIdx.x % c4, rl = threadIdx.x / c4;
  if (rl >= RL) return;
  const int col = cg * 4;
  float mu_[4], is_[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    double var;
    bn_column_stats(totals[col + v], totals[c + col + v], n, eps, mu_[v], is_[v], var);
    if (blockIdx.x == 0 && rl == 0) {
      save_mean[col + v] = mu_[v];
      save_invstd[col + v] = is_[v];
      if (running_mean) running_mean[col + v] = (1.f - momentum) * running_mean[col + v] + momentum * mu_[v];
      if (running_var) {
        const double unbiased = n > 1 ? var * (double)n / (double)(n - 1) : var;
        running_var[col + v] = (1.f - momentum) * running_var[col + v] + momentum * (float)unbiased;
      }
    }
  }
  const float4 mu = make_float4(mu_[0], mu_[1], mu_[2], mu_[3]), is = make_float4(is_[0], is_[1], is_[2], is_[3]);
  const float4 g = *(const float4 *)&gamma[col], b = *(const float4 *)&beta[col];
  auto one = [&](int64_t r) {
    const int64_t o = r * c + col;
    const float4 xv = *(const float4 *)&x[o];
    float4 ov;
    ov.x = bn_affine(xv.x, mu.x, is.x, g.x, b.x);
    ov.y = bn_affine(xv.y, mu.y, is.y, g.y, b.y);
    ov.z = bn_affine(xv.z, mu.z, is.z, g.z, b.z);
    ov.w = bn_affine(xv.w, mu.w, is.w, g.w, b.w);
    if (res) {
      const float4 rv = *(const float4 *)&res[o];
      ov.x += rv.x; ov.y += rv.y; ov.z += rv.z; ov.w += rv.w;
    }
    if (relu) {
      ov.x = ov.x > 0.f ? ov.x : 0.f; ov.y = ov.y > 0.f ? ov.y : 0.f;
      ov.z = ov.z > 0.f ? ov.z : 0.f; ov.w = ov.w > 0.f ? ov.w : 0.f;
    }
    *(float4 *)&y[o] = ov;
  };
  const int64_t stride = (int64_t)gridDim.x * RL;
  int64_t r = (int64_t)blockIdx.x * RL + rl;
  for (; r + stride < n; r += 2 * stride) {
    one(r);
    one(r + stride);
  }
  if (r < n) one(r);
}

static unsigned bn_apply_grid(int64_t n, int c) {
  int64_t g = ceil_div(n, 2 * (int64_t)row_lanes(c).RL);   // two rows per thread
  if (g > 4096) g = 4096;
  return (unsigned)(g < 1 ? 1 : g);
}

static int bn_check(const char *who, int64_t n, int c) {
  FTX_REQUIRE(n >= 0, "%s: n < 0", who);
  FTX_REQUIRE(c >= 4 && c % 4 == 0 && c <= 1024, "%s: c must be a multiple of 4 in [4,1024] (got %d)", who, c);
  return FTX_OK;
}

extern "C" int ftx_bn_train_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                                float *running_var, float momentum, float eps, int64_t n, int32_t c, int32_t relu, float *y,
                                float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes, void *stream) {
  int rc = bn_check("ftx_bn_train_fwd", n, c);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 1, "ftx_bn_train_fwd: needs at least one row");
  FTX_REQUIRE(x && gamma && beta && y && save_mean && save_invstd && workspace, "ftx_bn_train_fwd: null pointer");
  FTX_REQUIRE(c <= 512, "ftx_bn_train_fwd: c > 512 unsupported");
  if (workspace_bytes < ftx_bn_workspace_bytes(n, c)) return workspace_short("ftx_bn_train_fwd", workspace_bytes, ftx_bn_workspace_bytes(n, c));
  hipStream_t st = (hipStream_t)stream;
  const StreamScratch sc = stream_scratch(st);
  if (!sc.counters) return FTX_ELAUNCH;
  const int nb = bn_blocks(n);
  double *part = (double *)workspace;
  bn_partial_kernel<FwdOp><<<nb, 256, colstats_lds_bytes(c), st>>>(x, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, n, c, part, sc);
  bn_apply_fwd_kernel<<<bn_apply_grid(n, c), 256, 0, st>>>(x, residual, gamma, beta, part + (size_t)nb * 2 * c, eps, momentum, running_mean,
                                                           running_var, save_mean, save_invstd, n, c, relu, y);
  return check_launch("ftx_bn_train_fwd");
}

// BatchNorm forward whose statistics were produced by the pass that wrote x (ftx_spconv_reduce_stats): `totals` is the row
// [2][c] of float64 column sums / sums of squares that pass leaves behind its partial rows.  One launch: x is read once.
extern "C" int ftx_bn_train_fwd_totals(const float *x, const float *residual, const float *gamma, const float *beta, float *running_mean,
                                       float *running_var, float momentum, float eps, int64_t n, int32_t c, int32_t relu, float *y,
                                       float *save_mean, float *save_invstd, const double *totals, void *stream) {
  int rc = bn_check("ftx_bn_train_fwd_totals", n, c);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 1, "ftx_bn_train_fwd_totals: needs at least one row");
  FTX_REQUIRE(x && gamma && beta && y && save_mean && save_invstd && totals, "ftx_bn_train_fwd_totals: null pointer");
  bn_apply_fwd_kernel<<<bn_apply_grid(n, c), 256, 0, (hipStream_t)stream>>>(x, residual, gamma, beta, totals, eps, momentum, running_mean,
                                                                            running_var, save_mean, save_invstd, n, c, relu, y);
  return check_launch("ftx_bn_train_fwd_totals");
}

__global__ void bn_apply_eval_kernel(const float *__restrict__ x, const float *__restrict__ res, const float *__restrict__ gamma,
                                     const float *__restrict__ beta, const float *__restrict__ rm, const float *__restrict__ rv, float eps,
                                     int64_t n, int c, int relu, float *__restrict__ y) {
  const int c4 = c >> 2;
  const int64_t total = n * c4;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int col = (int)(e % c4) * 4;
    float4 xv = *(const float4 *)&x[e * 4];
    *(float4 *)&y[e * 4] = bn_eval_apply4(xv, res, e * 4, rm, rv, eps, gamma, beta, col, relu);
  }
}

extern "C" int ftx_bn_eval_fwd(const float *x, const float *residual, const float *gamma, const float *beta, const float *running_mean,
                               const float *running_var, float eps, int64_t n, int32_t c, int32_t relu, float *y, void *stream) {
  int rc = bn_check("ftx_bn_eval_fwd", n, c);
  if (rc != FTX_OK) return rc;
  if (n == 0) return FTX_OK;
  FTX_REQUIRE(x && gamma && beta && running_mean && running_var && y, "ftx_bn_eval_fwd: null pointer");
  bn_apply_eval_kernel<<<grid_for(n * (c / 4), 256), 256, 0, (hipStream_t)stream>>>(x, residual, gamma, beta, running_mean, running_var, eps,
                                                                                     n, c, relu, y);
  return check_launch("ftx_bn_eval_fwd");
}

__global__ __launch_bounds__(256) void bn_apply_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ mean,
                                                           const float *__restrict__ invstd, const double *__restrict__ sums, int64_t n, int c,
                                                           int relu, float *__restrict__ gx, float *__restrict__ gres,
                                                           float *__restrict__ grad_gamma, float *__restrict__ grad_beta) {
  const auto [c4, RL] = row_lanes(c);
  const int cg = threadIdx.x % c4, rl = threadIdx.x / c4;
  if (rl >= RL) return;
  const int col = cg * 4;
  const float inv_n = 1.f / (float)n;
  float mu[4], is[4], gm[4], bt[4], sdy[4], sdyx[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    mu[v] = mean[col + v];
    is[v] = invstd[col + v];
    gm[v] = gamma[col + v];
    bt[v] = relu == 2 ? beta[col + v] : 0.f;
    sdy[v] = (float)sums[col + v] * inv_n;
    sdyx[v] = (float)sums[c + col + v] * inv_n;
    if (blockIdx.x == 0 && rl == 0) {   // the parameter gradients are the two totals themselves
      if (grad_beta) grad_beta[col + v] = (float)sums[col + v];
      if (grad_gamma) grad_gamma[col + v] = (float)sums[c + col + v];
    }
  }
  auto one = [&](int64_t r) {
    const int64_t o = r * c + col;
    const float4 g4 = *(const float4 *)&gy[o];
    const float4 x4 = *(const float4 *)&x[o];
    float dy[4] = {g4.x, g4.y, g4.z, g4.w};
    const float xv[4] = {x4.x, x4.y, x4.z, x4.w};
    if (relu == 2) {          // the forward output recomputed from x (bit for bit: bn_affine), not read back
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (!(bn_affine(xv[v], mu[v], is[v], gm[v], bt[v]) > 0.f)) dy[v] = 0.f;
    } else if (relu) {
      const float4 y4 = *(const float4 *)&y[o];
      const float yv[4] = {y4.x, y4.y, y4.z, y4.w};
#pragma unroll
      for (int v = 0; v < 4; ++v)
        if (!(yv[v] > 0.f)) dy[v] = 0.f;
    }
    float ov[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float xhat = (xv[v] - mu[v]) * is[v];
      ov[v] = gm[v] * is[v] * (dy[v] - sdy[v] - xhat * sdyx[v]);
    }
    *(float4 *)&gx[o] = make_float4(ov[0], ov[1], ov[2], ov[3]);
    if (gres) *(float4 *)&gres[o] = make_float4(dy[0], dy[1], dy[2], dy[3]);
  };
  const int64_t stride = (int64_t)gridDim.x * RL;
  int64_t r = (int64_t)blockIdx.x * RL + rl;
  for (; r + stride < n; r += 2 * stride) {
    one(r);
    one(r + stride);
  }
  if (r < n) one(r);
}

extern "C" int ftx_bn_train_bwd(const float *grad_y, const float *x, const float *y, const float *gamma, const float *beta, const float *save_mean,
                                const float *save_invstd, int64_t n, int32_t c, int32_t relu, float *grad_x, float *grad_residual,
                                float *grad_gamma, float *grad_beta, void *workspace, size_t workspace_bytes, void *stream) {
  int rc = bn_check("ftx_bn_train_bwd", n, c);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(n >= 1, "ftx_bn_train_bwd: needs at least one row");
  FTX_REQUIRE(grad_y && x && gamma && save_mean && save_invstd && grad_x && workspace, "ftx_bn_train_bwd: null pointer");
  // ReLU mask: recomputed from x when the forward had no residual and beta is given (y is then not read and may be NULL), else from y
  const bool remask = relu && beta != nullptr && grad_residual == nullptr;
  FTX_REQUIRE(!relu || remask || y, "ftx_bn_train_bwd: relu needs the forward output y (or beta, when no residual went into it)");
  const int rmode = !relu ? 0 : (remask ? 2 : 1);
  FTX_REQUIRE(c <= 512, "ftx_bn_train_bwd: c > 512 unsupported");
  if (workspace_bytes < ftx_bn_workspace_bytes(n, c)) return workspace_short("ftx_bn_train_bwd", workspace_bytes, ftx_bn_workspace_bytes(n, c));
  hipStream_t st = (hipStream_t)stream;
  const StreamScratch sc = stream_scratch(st);
  if (!sc.counters) return FTX_ELAUNCH;
  const int nb = bn_blocks(n);
  double *part = (double *)workspace;
  double *sums = part + (size_t)nb * 2 * c;   // written by the last block of the statistics pass
  bn_partial_kernel<BwdOp><<<nb, 256, colstats_lds_bytes(c), st>>>(x, grad_y, rmode == 1 ? y : nullptr, save_mean, save_invstd, gamma, beta, rmode, n, c, part, sc);
  bn_apply_bwd_kernel<<<bn_apply_grid(n, c), 256, 0, st>>>(grad_y, x, y, gamma, beta, save_mean, save_invstd, sums, n, c, rmode, grad_x, grad_residual,
                                                           grad_gamma, grad_beta);
  return check_launch("ftx_bn_train_bwd");
}
