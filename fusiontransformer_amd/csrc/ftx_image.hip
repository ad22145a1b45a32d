// Colour jitter of the image-side augmentation and the conversion to the model's input, on one uint8 HWC RGB frame.
// Reference: data/semantic_kitti/semantic_kitti_dataloader.py:196-212 -- T.ColorJitter on the cropped PIL image, then
// np.array(image, float32) / 255, the left-right flip, (x - mean) / std and HWC -> CHW.  The per-pixel arithmetic is Pillow's
// (ftx_image_ops.h); this file schedules it.
//
// The only frame-wide quantity is the contrast op's mean luma of the image it receives.  The ops are split at the contrast op:
//   pass A  ops before contrast, writes the intermediate frame and one exact integer luma sum per block
//           (contrast first: a luma-only pre-pass instead);
//   pass B  every block adds the per-block sums in block order (integers: any order gives the same total), forms
//           int(sum / (h w) + 0.5) like ImageStat, applies contrast and the ops after it, and writes the output: uint8 HWC,
//           or float32 CHW with the flip folded into the store index.
// Without a contrast op pass B alone runs.  So a call is one or two launches; no host synchronisation, no atomics.
//
// Work item: 4 consecutive pixels of one row (12 bytes).  The source may be a crop view (row pitch > 3 w, any byte offset):
// a lane reads the aligned dwords that cover its 12 bytes (never a dword without one of its bytes, so never outside the
// allocation's pages) and realigns them with v_alignbyte.  The intermediate frame rows are padded to 12 ceil(w / 4) bytes.
#include "ftx_common.h"
#include "ftx_image_ops.h"
using namespace ftx;

namespace {

constexpr int IMG_BLOCK = 128;
constexpr int IMG_MAX_BLOCKS = 2048;  // per-block luma partials held in the workspace
constexpr size_t IMG_PARTIAL_BYTES = IMG_MAX_BLOCKS * sizeof(uint64_t);

enum OutKind { OUT_NONE = 0, OUT_PADDED = 1, OUT_U8 = 2, OUT_CHW = 3 };

struct PassArgs {
  const uint8_t *src;
  int64_t src_pitch;
  int height, width, chunks_per_row;
  int n_ops;
  int op[4];
  float alpha[4];
  int shift;              // hue shift (uint8) when a hue op is in this pass
  int use_mean;           // op[0] is contrast: read the partials of the previous pass
  int n_partials_in;      // blocks of the previous pass
  const unsigned long long *partials_in;
  unsigned long long *partials_out;  // non-null: write this block's luma sum of the pass's result
  uint8_t *dst_u8;
  int64_t dst_pitch;
  float *dst_f32;
  int flip;
  float mean[3], stdv[3];
};

__device__ inline unsigned long long block_sum_u64(unsigned long long v, unsigned long long *red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = v;
  __syncthreads();
  unsigned long long t = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < IMG_BLOCK / 64; ++w) t += red[w];
  __syncthreads();
  return t;  // valid in thread 0
}

template <int OUT>
__global__ __launch_bounds__(IMG_BLOCK) void jitter_pass_kernel(PassArgs a) {
  __shared__ unsigned long long red[IMG_BLOCK / 64];
  __shared__ int s_grey;
  int grey = 0;
  if (a.use_mean) {
    unsigned long long part = 0;
    for (int i = threadIdx.x; i < a.n_partials_in; i += IMG_BLOCK) part += a.partials_in[i];
    const unsigned long long total = block_sum_u64(part, red);
    if (threadIdx.x == 0) {
      // ImageStat.mean: the histogram's exact sum over the pixel count, a correctly rounded double division (total < 2^53)
      const double mean = (double)total / ((double)a.height * (double)a.width);
      s_grey = (int)(mean + 0.5);
    }
    __syncthreads();
    grey = s_grey;
  }
  unsigned long long luma_acc = 0;
  const int64_t work = (int64_t)a.height * a.chunks_per_row;
  for (int64_t c = blockIdx.x * (int64_t)IMG_BLOCK + threadIdx.x; c < work; c += (int64_t)gridDim.x * IMG_BLOCK) {
    const int y = (int)(c / a.chunks_per_row);
    const int x0 = (int)(c - (int64_t)y * a.chunks_per_row) * 4;
    const int n = min(4, a.width - x0);
    // aligned dword loads of the 3n source bytes, realigned to the first one
    const uint8_t *sp = a.src + y * a.src_pitch + 3 * x0;
    const uintptr_t addr = (uintptr_t)sp;
    const uint32_t sh = (uint32_t)(addr & 3);
    const uint32_t *wp = (const uint32_t *)(sp - sh);  // derived from a.src, not from an integer: global (not flat) loads
    const int last = (int)(((addr + 3 * n - 1) >> 2) - (addr >> 2));
    const uint32_t d0 = wp[0];
    const uint32_t d1 = last >= 1 ? wp[1] : 0u;
    const uint32_t d2 = last >= 2 ? wp[2] : 0u;
    const uint32_t d3 = last >= 3 ? wp[3] : 0u;
    uint32_t w[3] = {__builtin_amdgcn_alignbyte(d1, d0, sh), __builtin_amdgcn_alignbyte(d2, d1, sh), __builtin_amdgcn_alignbyte(d3, d2, sh)};
    int px[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) px[j] = (w[j >> 2] >> (8 * (j & 3))) & 255;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      for (int o = 0; o < a.n_ops; ++o)
        jitter_pixel(a.op[o], a.alpha[o], grey, a.shift, px[3 * k], px[3 * k + 1], px[3 * k + 2]);
      if (a.partials_out && k < n) luma_acc += pil_luma(px[3 * k], px[3 * k + 1], px[3 * k + 2]);
    }
    if (OUT == OUT_PADDED || OUT == OUT_U8) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
        w[q] = (uint32_t)px[4 * q] | ((uint32_t)px[4 * q + 1] << 8) | ((uint32_t)px[4 * q + 2] << 16) | ((uint32_t)px[4 * q + 3] << 24);
      uint8_t *o = a.dst_u8 + y * a.dst_pitch + 3 * x0;
      if (OUT == OUT_PADDED || (n == 4 && ((uintptr_t)o & 3) == 0)) {  // padded rows: always 12 aligned bytes
        uint32_t *o32 = (uint32_t *)o;
        o32[0] = w[0]; o32[1] = w[1]; o32[2] = w[2];
      } else {
        for (int j = 0; j < 3 * n; ++j) o[j] = (uint8_t)px[j];
      }
    } else if (OUT == OUT_CHW) {
      const int64_t plane = (int64_t)a.height * a.width;
      float *row = a.dst_f32 + (int64_t)y * a.width;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // np.array(image, float32) / 255: a correctly rounded float32 division; then (x - mean) / std, two roundings
          const float x = (float)px[3 * k + ch] / 255.0f;
          v[k] = (x - a.mean[ch]) / a.stdv[ch];
        }
        float *p = row + ch * plane;
        if (n == 4 && (a.width & 3) == 0) {  // 16-byte aligned: the output is a fresh allocation and w % 4 == 0
          if (a.flip)
            *(float4 *)(p + a.width - 4 - x0) = make_float4(v[3], v[2], v[1], v[0]);
          else
            *(float4 *)(p + x0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
          for (int k = 0; k < n; ++k) p[a.flip ? a.width - 1 - (x0 + k) : x0 + k] = v[k];
        }
      }
    }
  }
  if (a.partials_out) {
    const unsigned long long t = block_sum_u64(luma_acc, red);
    if (threadIdx.x == 0) a.partials_out[blockIdx.x] = t;
  }
}

int64_t padded_pitch(int width) { return 12 * (int64_t)ceil_div(width, 4); }

unsigned pass_grid(int height, int width) {
  int64_t g = ceil_div((int64_t)height * ceil_div(width, 4), IMG_BLOCK);
  if (g > IMG_MAX_BLOCKS) g = IMG_MAX_BLOCKS;
  if (g < 1) g = 1;
  return (unsigned)g;
}

template <int OUT>
void launch_pass(const PassArgs &a, unsigned grid, hipStream_t st) {
  jitter_pass_kernel<OUT><<<grid, IMG_BLOCK, 0, st>>>(a);
}

int validate(const char *who, const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops,
             const double *factors, int32_t n_ops, const void *dst) {
  FTX_REQUIRE(height >= 0 && width >= 0, "%s: negative size", who);
  FTX_REQUIRE(channels == 3, "%s: channels must be 3 (RGB), got %d", who, channels);
  FTX_REQUIRE(pitch >= 3 * (int64_t)width, "%s: row pitch %lld smaller than 3 * width = %lld", who, (long long)pitch, 3 * (long long)width);
  FTX_REQUIRE(n_ops >= 0 && n_ops <= 4, "%s: n_ops %d outside 0..4", who, n_ops);
  FTX_REQUIRE(n_ops == 0 || (ops && factors), "%s: null ops or factors with n_ops %d", who, n_ops);
  int seen = 0;
  for (int i = 0; i < n_ops; ++i) {
    FTX_REQUIRE(ops[i] >= FTX_JITTER_BRIGHTNESS && ops[i] <= FTX_JITTER_HUE, "%s: unknown op code %d", who, ops[i]);
    FTX_REQUIRE(!(seen & (1 << ops[i])), "%s: op %d repeated", who, ops[i]);
    seen |= 1 << ops[i];
    const double f = factors[i];
    if (ops[i] == FTX_JITTER_HUE)
      FTX_REQUIRE(f >= -0.5 && f <= 0.5, "%s: hue factor %g not in [-0.5, 0.5]", who, f);
    else
      FTX_REQUIRE(f >= 0.0 && f < 1e30, "%s: negative or non-finite factor %g for op %d", who, f, ops[i]);
  }
  FTX_REQUIRE((int64_t)height * width == 0 || (src && dst), "%s: null pointer", who);
  return FTX_OK;
}

// Shared body of the two entry points: validates, plans the passes, launches them.
int jitter_chain(const char *who, const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops,
                 const double *factors, int32_t n_ops, int out_kind, uint8_t *dst_u8, float *dst_f32, int32_t flip, const float *mean_host,
                 const float *std_host, void *workspace, size_t workspace_bytes, void *stream) {
  int rc = validate(who, src, pitch, height, width, channels, ops, factors, n_ops, out_kind == OUT_U8 ? (const void *)dst_u8 : dst_f32);
  if (rc != FTX_OK) return rc;
  int contrast_at = -1;
  for (int i = 0; i < n_ops; ++i)
    if (ops[i] == FTX_JITTER_CONTRAST) contrast_at = i;
  if (contrast_at >= 0) {
    FTX_REQUIRE(workspace || (int64_t)height * width == 0, "%s: a contrast op needs the workspace", who);
    FTX_REQUIRE(workspace_bytes >= ftx_color_jitter_workspace_bytes(height, width), "%s: workspace of %zu bytes, %zu needed", who,
                workspace_bytes, ftx_color_jitter_workspace_bytes(height, width));
    FTX_REQUIRE(((uintptr_t)workspace & 15) == 0, "%s: workspace must be 16-byte aligned", who);
  }
  if ((int64_t)height * width == 0) return FTX_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = pass_grid(height, width);
  unsigned long long *partials = (unsigned long long *)workspace;
  uint8_t *inter = (uint8_t *)workspace + IMG_PARTIAL_BYTES;

  PassArgs base = {};
  base.height = height;
  base.width = width;
  base.chunks_per_row = (int)ceil_div(width, 4);
  auto set_ops = [&](PassArgs &p, int from, int to) {
    p.n_ops = to - from;
    for (int i = from; i < to; ++i) {
      p.op[i - from] = ops[i];
      p.alpha[i - from] = (float)factors[i];  // Pillow's blend takes the factor as a C float
      if (ops[i] == FTX_JITTER_HUE) {
        // torchvision 0.8 adds np.uint8(hue_factor * 255) to the uint8 hue; numpy of that era wrapped a negative value modulo 256
        // through the C cast (numpy 2 raises instead).  Same as Python's int(hue_factor * 255) % 256: truncation toward zero.
        const int q = (int)(factors[i] * 255.0);
        p.shift = ((q % 256) + 256) % 256;
      }
    }
  };

  PassArgs b = base;
  b.src = src;
  b.src_pitch = pitch;
  if (contrast_at >= 0) {
    PassArgs a = base;
    a.src = src;
    a.src_pitch = pitch;
    a.partials_out = partials;
    set_ops(a, 0, contrast_at);
    if (contrast_at == 0) {
      launch_pass<OUT_NONE>(a, grid, st);  // luma-only pre-pass
    } else {
      a.dst_u8 = inter;
      a.dst_pitch = padded_pitch(width);
      launch_pass<OUT_PADDED>(a, grid, st);
      b.src = inter;
      b.src_pitch = padded_pitch(width);
    }
    b.use_mean = 1;
    b.partials_in = partials;
    b.n_partials_in = (int)grid;
    set_ops(b, contrast_at, n_ops);
  } else {
    set_ops(b, 0, n_ops);
  }
  if (out_kind == OUT_U8) {
    b.dst_u8 = dst_u8;
    b.dst_pitch = 3 * (int64_t)width;
    launch_pass<OUT_U8>(b, grid, st);
  } else {
    b.dst_f32 = dst_f32;
    b.flip = flip ? 1 : 0;
    for (int c = 0; c < 3; ++c) {
      b.mean[c] = mean_host ? mean_host[c] : 0.0f;  // (x - 0) / 1 == x exactly
      b.stdv[c] = std_host ? std_host[c] : 1.0f;
    }
    launch_pass<OUT_CHW>(b, grid, st);
  }
  return check_launch(who);
}

}  // namespace

extern "C" size_t ftx_color_jitter_workspace_bytes(int32_t height, int32_t width) {
  if (height < 0 || width < 0) return 0;
  return IMG_PARTIAL_BYTES + (size_t)height * (size_t)padded_pitch(width);
}

extern "C" int ftx_color_jitter_u8(const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops_host,
                                   const double *factors_host, int32_t n_ops, uint8_t *dst, void *workspace, size_t workspace_bytes,
                                   void *stream) {
  return jitter_chain("ftx_color_jitter_u8", src, pitch, height, width, channels, ops_host, factors_host, n_ops, OUT_U8, dst, nullptr, 0,
                      nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int ftx_color_jitter_chw(const uint8_t *src, int64_t pitch, int32_t height, int32_t width, int32_t channels, const int32_t *ops_host,
                                    const double *factors_host, int32_t n_ops, int32_t flip, const float *mean_host, const float *std_host,
                                    float *dst, void *workspace, size_t workspace_bytes, void *stream) {
  FTX_REQUIRE(!mean_host == !std_host, "ftx_color_jitter_chw: mean and std must both be given or both be null");
  if (std_host)
    for (int c = 0; c < 3; ++c) FTX_REQUIRE(std_host[c] != 0.0f, "ftx_color_jitter_chw: std[%d] is zero", c);
  return jitter_chain("ftx_color_jitter_chw", src, pitch, height, width, channels, ops_host, factors_host, n_ops, OUT_CHW, nullptr, dst, flip,
                      mean_host, std_host, workspace, workspace_bytes, stream);
}
