// Per-pixel colour operations of Pillow on uint8 RGB, reproduced to the bit (ftx_image.hip).
//
// Every function mirrors one C statement sequence of Pillow (libImaging Blend.c, Convert.c) with its types: where Pillow
// computes in float the code here computes in float, where a double literal promotes an expression to double it does so here.
// Contraction into fused multiply-adds is switched off for this header: Pillow's x86-64 build rounds the product and the sum
// separately, and one fused rounding changes pixels (the blend at alpha 1.37 is the documented case).
// __host__ __device__ so that the same text can be compiled for the CPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ftx {

enum JitterOp { JIT_BRIGHTNESS = 0, JIT_CONTRAST = 1, JIT_SATURATION = 2, JIT_HUE = 3 };

// Image.blend(im1, im2, alpha) for one channel (Blend.c): float32 multiply, float32 add, truncation; clipped to [0, 255] (the
// extrapolating branch, alpha outside [0, 1]; inside it the value is already in range and the clip is a no-op).
__host__ __device__ inline int pil_blend(int in1, int in2, float alpha) {
  const float t = (float)in1 + alpha * (float)(in2 - in1);
  if (t <= 0.0f) return 0;
  if (t >= 255.0f) return 255;
  return (int)t;
}

// convert("L") of an RGB pixel (Convert.c rgb2l, ITU-R 601-2 with 16-bit fixed-point weights and rounding).
__host__ __device__ inline int pil_luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

__host__ __device__ inline int pil_clip8(int v) { return v <= 0 ? 0 : (v >= 255 ? 255 : v); }

// convert("HSV") (Convert.c rgb2hsv_row, after colorsys.py).
__host__ __device__ inline void pil_rgb2hsv(int r, int g, int b, int &uh, int &us, int &uv) {
  const int maxc = r > g ? (r > b ? r : b) : (g > b ? g : b);
  const int minc = r < g ? (r < b ? r : b) : (g < b ? g : b);
  uv = maxc;
  if (minc == maxc) {
    uh = 0;
    us = 0;
    return;
  }
  const float cr = (float)(maxc - minc);
  const float s = cr / (float)maxc;
  const float rc = ((float)(maxc - r)) / cr;
  const float gc = ((float)(maxc - g)) / cr;
  const float bc = ((float)(maxc - b)) / cr;
  float h;
  if (r == maxc) {
    h = bc - gc;
  } else if (g == maxc) {
    h = 2.0 + rc - bc;  // double
  } else {
    h = 4.0 + gc - rc;  // double
  }
  h = fmod((h / 6.0 + 1.0), 1.0);  // double, stored to float
  uh = pil_clip8((int)(h * 255.0));
  us = pil_clip8((int)(s * 255.0));
}

// convert("RGB") of an HSV pixel (Convert.c hsv2rgb).
__host__ __device__ inline void pil_hsv2rgb(int h, int s, int v, int &r, int &g, int &b) {
  if (s == 0) {
    r = g = b = v;
    return;
  }
  const int i = (int)floor((float)h * 6.0 / 255.0);
  const float f = (float)h * 6.0 / 255.0 - (float)i;
  const float fs = ((float)s) / 255.0;
  const int up = pil_clip8((int)round((float)v * (1.0 - fs)));
  const int uq = pil_clip8((int)round((float)v * (1.0 - fs * f)));  // fs * f: a float product
  const int ut = pil_clip8((int)round((float)v * (1.0 - fs * (1.0 - f))));
  switch (i % 6) {
    case 0: r = v; g = ut; b = up; break;
    case 1: r = uq; g = v; b = up; break;
    case 2: r = up; g = v; b = ut; break;
    case 3: r = up; g = uq; b = v; break;
    case 4: r = ut; g = up; b = v; break;
    default: r = v; g = up; b = uq; break;
  }
}

// One jitter operation on one pixel.  `alpha` = (float)factor (Pillow passes the blend factor as a C float); `grey` = the contrast
// op's degenerate value int(mean luma + 0.5); `shift` = the hue op's uint8 shift.
__host__ __device__ inline void jitter_pixel(int op, float alpha, int grey, int shift, int &r, int &g, int &b) {
  switch (op) {
    case JIT_BRIGHTNESS:  // ImageEnhance.Brightness: blend(black, img)
      r = pil_blend(0, r, alpha); g = pil_blend(0, g, alpha); b = pil_blend(0, b, alpha);
      break;
    case JIT_CONTRAST:  // ImageEnhance.Contrast: blend(grey image of the mean luma, img)
      r = pil_blend(grey, r, alpha); g = pil_blend(grey, g, alpha); b = pil_blend(grey, b, alpha);
      break;
    case JIT_SATURATION: {  // ImageEnhance.Color: blend(img.convert("L").convert("RGB"), img)
      const int l = pil_luma(r, g, b);
      r = pil_blend(l, r, alpha); g = pil_blend(l, g, alpha); b = pil_blend(l, b, alpha);
      break;
    }
    default: {  // torchvision adjust_hue: HSV round trip with the uint8 hue shifted modulo 256
      int h, s, v;
      pil_rgb2hsv(r, g, b, h, s, v);
      pil_hsv2rgb((h + shift) & 255, s, v, r, g, b);
      break;
    }
  }
}

}  // namespace ftx
