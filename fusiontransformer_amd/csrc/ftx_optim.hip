// The solver over all parameters of the model, one launch per rule (torch.optim.Adam / AdamW / SGD's update rules; the optimizer
// common/solver/build.py:7-20 builds for the reference's trainers and SemanticTrainer.train_step steps once per batch), and max-norm
// gradient clipping (torch.nn.utils.clip_grad_norm_) as one extra read of the gradients: a per-chunk sum of squares, a one-block
// finalize that leaves (norm, coefficient) in device memory, and the coefficient applied to g inside the update.
//
// The model has ~300 parameter tensors (108 M floats).  A table in device memory describes them: parameter / first moment / second
// moment pointers and the element count (static), and per step the gradient pointer and the two bias-correction factors (the
// gradients are freshly allocated by autograd every step, so their addresses are not).  The work is cut into chunks of 16 K elements
// ahead of time (chunk -> tensor, offset: static), one block per chunk, 16-byte loads and stores.  Streams of 4 B per element:
// Adam / AdamW 7 (read p, g, m, v; write p, m, v) = 3.0 GB per step at HBM rate instead of 14 multi-tensor launches; SGD with
// momentum 5 (read p, g, buf; write p, buf), without 3; the sum of squares 1.
#include "ftx_common.h"
#include "ftx_reduce.h"

using namespace ftx;

struct FtxAdamTensor {      // 48 bytes; mirrored by fusiontransformer_amd/optim.py
  float *p;
  float *m;
  float *v;
  const float *g;           // per step; NULL: no gradient this step, the tensor is skipped
  int64_t n;
  float step_size;          // lr / (1 - beta1^t)
  float inv_bc2_sqrt;       // 1 / sqrt(1 - beta2^t)
};

struct FtxSgdTensor {       // the same 48 bytes read by ftx_sgd_step: p, g and n sit where FtxAdamTensor has them
  float *p;
  float *buf;               // momentum buffer; NULL with momentum == 0
  float *unused;
  const float *g;
  int64_t n;
  int32_t first;            // != 0: the tensor's first step with a gradient, buf = g (buf is written, not read)
  int32_t pad;
};
static_assert(sizeof(FtxSgdTensor) == sizeof(FtxAdamTensor), "one record size for every rule");

constexpr int ADAM_CHUNK = 16384;   // elements per block

// One chunk, 256 threads: vec4(i) for the whole groups of four when every pointer allows 16-byte accesses, one(i, true) for the same
// elements when not, one(i, false) for the 1..3 elements behind the last whole group.
template <class V, class S>
__device__ inline void walk_chunk(int64_t off, int64_t end, bool vec, V &&vec4, S &&one) {
  const int64_t end4 = off + ((end - off) & ~(int64_t)3);
  if (vec) {
    for (int64_t i = off + (int64_t)threadIdx.x * 4; i < end4; i += 256 * 4) vec4(i);
  } else {
    for (int64_t i = off + threadIdx.x; i < end4; i += 256) one(i, true);
  }
  for (int64_t i = end4 + threadIdx.x; i < end; i += 256) one(i, false);
}

// DECOUPLED: AdamW (p *= 1 - lr wd, no L2 term; `decay` holds 1 - lr wd), else Adam (g += wd p; `decay` holds wd).
// SCALED: g is multiplied by *grad_scale first (the clip coefficient ftx_grad_norm_finalize left).
template <bool DECOUPLED, bool SCALED>
__global__ __launch_bounds__(256) void adam_kernel(const FtxAdamTensor *__restrict__ table, const int32_t *__restrict__ chunk_tensor,
                                                   const int64_t *__restrict__ chunk_offset, float omb1, float beta2, float omb2, float eps,
                                                   float decay, const float *__restrict__ grad_scale) {
  const FtxAdamTensor t = table[chunk_tensor[blockIdx.x]];
  if (t.g == nullptr) return;
  const float scale = SCALED ? *grad_scale : 1.f;
  const int64_t off = chunk_offset[blockIdx.x];
  const int64_t end = off + ADAM_CHUNK < t.n ? off + ADAM_CHUNK : t.n;
  // omb1 = 1 - beta1, omb2 = 1 - beta2 come from the host, formed in double like torch does (1.f - 0.999f is off by 1.3e-5 relative)
  // Every rounding is spelled out.  Left to the compiler's contraction, the float4 body fused beta2 * v + (omb2 * g) * g and the scalar
  // loops did not, so the last bit of v depended on the pointers' alignment.  Which form an element gets is now a function of its place
  // alone: FUSED for the whole groups of four counted from the chunk's offset, unfused for the 1..3 elements behind them -- what the
  // float4 body and its scalar tail have always computed on 16-byte aligned tensors (a training run keeps its bits), and now also what a
  // tensor at any other alignment gets.  The other four operations were contracted alike on both paths and are written as they were.
  auto update = [&](float &p, float g, float &m, float &v, bool fused) {
    if (SCALED) g = __fmul_rn(g, scale);
    if (DECOUPLED)
      p = __fmul_rn(p, decay);                                           // param.mul_(1 - lr * weight_decay)
    else
      g = __fmaf_rn(decay, p, g);                                        // L2 form: grad.add(param, alpha=weight_decay)
    m = __fmaf_rn(omb1, __fsub_rn(g, m), m);                             // exp_avg.lerp_(grad, 1 - beta1)
    const float gg = __fmul_rn(__fmul_rn(omb2, g), g);                   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    v = fused ? __fmaf_rn(beta2, v, gg) : __fadd_rn(__fmul_rn(beta2, v), gg);
    const float denom = __fmaf_rn(sqrtf(v), t.inv_bc2_sqrt, eps);
    p = __fmaf_rn(-t.step_size, m / denom, p);
  };
  const bool vec = ((((uintptr_t)t.p | (uintptr_t)t.m | (uintptr_t)t.v | (uintptr_t)t.g) & 15) == 0) && ((off & 3) == 0);
  walk_chunk(
      off, end, vec,
      [&](int64_t i) {
        float4 p = *(const float4 *)&t.p[i], m = *(const float4 *)&t.m[i], v = *(const float4 *)&t.v[i];
        const float4 g = *(const float4 *)&t.g[i];
        update(p.x, g.x, m.x, v.x, true);
        update(p.y, g.y, m.y, v.y, true);
        update(p.z, g.z, m.z, v.z, true);
        update(p.w, g.w, m.w, v.w, true);
        *(float4 *)&t.p[i] = p;
        *(float4 *)&t.m[i] = m;
        *(float4 *)&t.v[i] = v;
      },
      [&](int64_t i, bool fused) { update(t.p[i], t.g[i], t.m[i], t.v[i], fused); });
}

// torch.optim.SGD: g += wd p; buf = first ? g : momentum buf + (1 - dampening) g; g = nesterov ? g + momentum buf : buf; p -= lr g.
// Every rounding is spelled out, and none depends on the element's place.  They sit where torch's own sequence of operations puts
// them: momentum buf is rounded on its own (buf.mul_), every add with an alpha is one multiply-add.
template <bool MOMENTUM, bool SCALED>
__global__ __launch_bounds__(256) void sgd_kernel(const FtxSgdTensor *__restrict__ table, const int32_t *__restrict__ chunk_tensor,
                                                  const int64_t *__restrict__ chunk_offset, float neg_lr, float momentum, float omd,
                                                  float weight_decay, int nesterov, const float *__restrict__ grad_scale) {
  const FtxSgdTensor t = table[chunk_tensor[blockIdx.x]];
  if (t.g == nullptr || (MOMENTUM && t.buf == nullptr)) return;
  const float scale = SCALED ? *grad_scale : 1.f;
  const int64_t off = chunk_offset[blockIdx.x];
  const int64_t end = off + ADAM_CHUNK < t.n ? off + ADAM_CHUNK : t.n;
  const bool first = t.first != 0;
  auto update = [&](float &p, float g, float &buf) {
    if (SCALED) g = __fmul_rn(g, scale);
    g = __fmaf_rn(weight_decay, p, g);                                   // grad.add(param, alpha=weight_decay)
    if (MOMENTUM) {
      buf = first ? g : __fmaf_rn(omd, g, __fmul_rn(momentum, buf));     // buf.mul_(momentum).add_(grad, alpha=1 - dampening)
      g = nesterov ? __fmaf_rn(momentum, buf, g) : buf;                  // grad.add(buf, alpha=momentum)
    }
    p = __fmaf_rn(neg_lr, g, p);                                         // param.add_(grad, alpha=-lr)
  };
  const uintptr_t bits = (uintptr_t)t.p | (uintptr_t)t.g | (MOMENTUM ? (uintptr_t)t.buf : 0);
  const bool vec = ((bits & 15) == 0) && ((off & 3) == 0);
  walk_chunk(
      off, end, vec,
      [&](int64_t i) {
        float4 p = *(const float4 *)&t.p[i], b = make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 g = *(const float4 *)&t.g[i];
        if (MOMENTUM && !first) b = *(const float4 *)&t.buf[i];
        update(p.x, g.x, b.x);
        update(p.y, g.y, b.y);
        update(p.z, g.z, b.z);
        update(p.w, g.w, b.w);
        *(float4 *)&t.p[i] = p;
        if (MOMENTUM) *(float4 *)&t.buf[i] = b;
      },
      [&](int64_t i, bool) {
        float b = (MOMENTUM && !first) ? t.buf[i] : 0.f;
        update(t.p[i], t.g[i], b);
        if (MOMENTUM) t.buf[i] = b;
      });
}

// Sum of the squares of one chunk of one gradient, in float64 (the square of a float32 is exact there): partial[chunk].
// Thread x takes the groups of four x, x + 256, ... counted from the chunk's offset, the last group possibly short, and adds their
// elements in ascending order; the 16-byte load is only another way to fetch a whole group, so the bits of the sum do not depend on
// the gradient's alignment.  Then the wave tree and the four waves in ascending order (block_sum).
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const FtxAdamTensor *__restrict__ table, const int32_t *__restrict__ chunk_tensor,
                                                         const int64_t *__restrict__ chunk_offset, double *__restrict__ partial) {
  __shared__ double sh[4];
  const FtxAdamTensor t = table[chunk_tensor[blockIdx.x]];
  double acc = 0.0;
  if (t.g != nullptr) {
    const int64_t off = chunk_offset[blockIdx.x];
    const int64_t end = off + ADAM_CHUNK < t.n ? off + ADAM_CHUNK : t.n;
    const bool vec = (((uintptr_t)t.g & 15) == 0) && ((off & 3) == 0);
    for (int64_t i = off + (int64_t)threadIdx.x * 4; i < end; i += 256 * 4) {
      if (vec && i + 4 <= end) {
        const float4 g = *(const float4 *)&t.g[i];
        acc += (double)g.x * (double)g.x;
        acc += (double)g.y * (double)g.y;
        acc += (double)g.z * (double)g.z;
        acc += (double)g.w * (double)g.w;
      } else {
        const int64_t stop = i + 4 < end ? i + 4 : end;
        for (int64_t j = i; j < stop; ++j) acc += (double)t.g[j] * (double)t.g[j];
      }
    }
  }
  const double r = block_sum(acc, sh);      // the table is uniform over the block: every thread reaches the barriers
  if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// One block: thread x adds partials x, x + 256, ... in ascending order, then block_sum.  out[0] = norm, out[1] = clip coefficient
// (clip_grad_norm_ with error_if_nonfinite=False: max_norm / (norm + 1e-6) clamped to 1; NaN stays NaN, an infinite norm gives 0).
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const double *__restrict__ partial, int64_t n_partials, float max_norm,
                                                                 float *__restrict__ out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_partials; i += 256) acc += partial[i];
  const double total = block_sum(acc, sh);
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(total);
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    out[0] = norm;
    out[1] = c > 1.f ? 1.f : c;
  }
}

extern "C" int32_t ftx_adam_chunk_elements(void) { return ADAM_CHUNK; }
extern "C" int32_t ftx_adam_tensor_bytes(void) { return (int32_t)sizeof(FtxAdamTensor); }

static int adam_checks(const char *who, const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks,
                       double beta1, double beta2, float eps) {
  FTX_REQUIRE(n_chunks >= 0, "%s: n_chunks < 0", who);
  if (n_chunks == 0) return FTX_OK;
  FTX_REQUIRE(table && chunk_tensor && chunk_offset, "%s: null pointer", who);
  FTX_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps >= 0.f, "%s: bad hyper-parameter", who);
  return FTX_OK;
}

template <bool DECOUPLED>
static int adam_launch(const char *who, const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks,
                       double beta1, double beta2, float eps, float decay, const float *grad_scale, void *stream) {
  const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
  if (grad_scale)
    adam_kernel<DECOUPLED, true><<<(unsigned)n_chunks, 256, 0, (hipStream_t)stream>>>((const FtxAdamTensor *)table, chunk_tensor, chunk_offset,
                                                                                     omb1, (float)beta2, omb2, eps, decay, grad_scale);
  else
    adam_kernel<DECOUPLED, false><<<(unsigned)n_chunks, 256, 0, (hipStream_t)stream>>>((const FtxAdamTensor *)table, chunk_tensor, chunk_offset,
                                                                                      omb1, (float)beta2, omb2, eps, decay, nullptr);
  return check_launch(who);
}

extern "C" int ftx_adam_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double beta1,
                             double beta2, float eps, float weight_decay, void *stream) {
  const int rc = adam_checks("ftx_adam_step", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps);
  if (rc != FTX_OK || n_chunks == 0) return rc;
  return adam_launch<false>("ftx_adam_step", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps, weight_decay, nullptr, stream);
}

extern "C" int ftx_adam_step_scaled(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks,
                                    double beta1, double beta2, float eps, float weight_decay, const float *grad_scale, void *stream) {
  const int rc = adam_checks("ftx_adam_step_scaled", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps);
  if (rc != FTX_OK || n_chunks == 0) return rc;
  return adam_launch<false>("ftx_adam_step_scaled", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps, weight_decay, grad_scale,
                            stream);
}

extern "C" int ftx_adamw_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double beta1,
                              double beta2, float eps, double lr, double weight_decay, const float *grad_scale, void *stream) {
  const int rc = adam_checks("ftx_adamw_step", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps);
  if (rc != FTX_OK) return rc;
  FTX_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "ftx_adamw_step: bad hyper-parameter");
  if (n_chunks == 0) return FTX_OK;
  // 1 - lr * weight_decay is formed in double and then rounded, as torch forms the scalar of param.mul_
  return adam_launch<true>("ftx_adamw_step", table, chunk_tensor, chunk_offset, n_chunks, beta1, beta2, eps, (float)(1.0 - lr * weight_decay),
                           grad_scale, stream);
}

extern "C" int ftx_sgd_step(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double lr,
                            double momentum, double dampening, double weight_decay, int32_t nesterov, const float *grad_scale, void *stream) {
  FTX_REQUIRE(n_chunks >= 0, "ftx_sgd_step: n_chunks < 0");
  FTX_REQUIRE(lr >= 0.0 && momentum >= 0.0 && weight_decay >= 0.0 && dampening == dampening, "ftx_sgd_step: bad hyper-parameter");
  FTX_REQUIRE(!nesterov || (momentum > 0.0 && dampening == 0.0), "ftx_sgd_step: nesterov needs momentum > 0 and dampening == 0");
  if (n_chunks == 0) return FTX_OK;
  FTX_REQUIRE(table && chunk_tensor && chunk_offset, "ftx_sgd_step: null pointer");
  const FtxSgdTensor *tab = (const FtxSgdTensor *)table;
  const float neg_lr = (float)-lr, mom = (float)momentum, omd = (float)(1.0 - dampening), wd = (float)weight_decay;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)n_chunks;
  if (momentum != 0.0) {
    if (grad_scale)
      sgd_kernel<true, true><<<grid, 256, 0, s>>>(tab, chunk_tensor, chunk_offset, neg_lr, mom, omd, wd, nesterov, grad_scale);
    else
      sgd_kernel<true, false><<<grid, 256, 0, s>>>(tab, chunk_tensor, chunk_offset, neg_lr, mom, omd, wd, nesterov, nullptr);
  } else {
    if (grad_scale)
      sgd_kernel<false, true><<<grid, 256, 0, s>>>(tab, chunk_tensor, chunk_offset, neg_lr, mom, omd, wd, 0, grad_scale);
    else
      sgd_kernel<false, false><<<grid, 256, 0, s>>>(tab, chunk_tensor, chunk_offset, neg_lr, mom, omd, wd, 0, nullptr);
  }
  return check_launch("ftx_sgd_step");
}

extern "C" int ftx_grad_sumsq(const void *table, const int32_t *chunk_tensor, const int64_t *chunk_offset, int32_t n_chunks, double *partial,
                              void *stream) {
  FTX_REQUIRE(n_chunks >= 0, "ftx_grad_sumsq: n_chunks < 0");
  if (n_chunks == 0) return FTX_OK;
  FTX_REQUIRE(table && chunk_tensor && chunk_offset && partial, "ftx_grad_sumsq: null pointer");
  grad_sumsq_kernel<<<(unsigned)n_chunks, 256, 0, (hipStream_t)stream>>>((const FtxAdamTensor *)table, chunk_tensor, chunk_offset, partial);
  return check_launch("ftx_grad_sumsq");
}

extern "C" int ftx_grad_norm_finalize(const double *partial, int64_t n_partials, float max_norm, float *out, void *stream) {
  FTX_REQUIRE(n_partials >= 0, "ftx_grad_norm_finalize: n_partials < 0");
  FTX_REQUIRE(max_norm > 0.f, "ftx_grad_norm_finalize: max_norm must be positive");
  FTX_REQUIRE(out && (partial || n_partials == 0), "ftx_grad_norm_finalize: null pointer");
  grad_norm_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partial, n_partials, max_norm, out);
  return check_launch("ftx_grad_norm_finalize");
}
