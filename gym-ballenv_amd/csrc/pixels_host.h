// pixels_host.h -- be_observe_pixels' host side that needs no HIP (host_logic.h's sibling): the
// coefficients of PIL's bicubic resize 100 -> 40 as PIL's C code computes them, their packing into
// the six distinct rows the kernel takes by value, and the entry's argument checks.  Only ballenv.h
// and standard headers, so the host C++ compiler alone builds and tests it
// (tests/pixels_host_main.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "ballenv.h"

namespace behost {

// extract_patch of examples/ball_cnn_reinforce.py:120-163: span = 50 (a 100 x 100 patch), resized to
// 40 x 40.  The reference's only values: constants, not parameters.
constexpr int PIX_PATCH = 100, PIX_OUT = 40;
constexpr int PIX_TAPS = 10;          // most input pixels under one output's filter (support 2 * 2.5 = 5 a side)
constexpr int PIX_ROWS = 6;           // distinct coefficient rows: outputs 0, 1, the two interior phases, 38, 39
constexpr int PIX_BITS = 22;          // PIL's PRECISION_BITS = 32 - 8 - 2
// The kernel's row spans take isqrt(4 r^2 - dy^2) through f32, exact below 2^24: r <= 2047, which is
// be_config_check's own bound on radius_obstacle + radius_agent.
constexpr int PIX_MAX_RADIUS = 2047;

// PIL's bicubic_filter (a = -0.5), in its operand order
inline double pix_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

// PIL's precompute_coeffs(inSize 100, in0 0, in1 100, outSize 40, bicubic) and normalize_coeffs_8bpc:
// kk[xx] holds output xx's fixed-point taps (zero behind the last), bounds[xx] = {first input, taps}.
// false: a row has more than PIX_TAPS taps, a coefficient does not fit 24 signed bits, or
// 2^21 + 255 sum |k| would not fit PIL's (and the kernel's) int accumulator.
inline bool pix_coeffs(int32_t (&kk)[PIX_OUT][PIX_TAPS], int32_t (&bounds)[PIX_OUT][2]) {
  const double scale = (double)PIX_PATCH / PIX_OUT;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  bool ok = true;
  for (int xx = 0; xx < PIX_OUT; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > PIX_PATCH) xmax = PIX_PATCH;
    xmax -= xmin;
    if (xmax > PIX_TAPS) { ok = false; xmax = PIX_TAPS; }
    double k[PIX_TAPS], ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      const double w = pix_bicubic((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    int64_t mag = 0;
    for (int x = 0; x < PIX_TAPS; ++x) {
      double v = 0.0;
      if (x < xmax) v = ww != 0.0 ? k[x] / ww : k[x];
      const int32_t q = v < 0 ? (int32_t)(-0.5 + v * (1 << PIX_BITS)) : (int32_t)(0.5 + v * (1 << PIX_BITS));
      kk[xx][x] = q;
      mag += q < 0 ? -(int64_t)q : q;
      if (q >= (1 << 23) || q < -(1 << 23)) ok = false;   // the kernel multiplies in 24 bits
    }
    if (((int64_t)1 << (PIX_BITS - 1)) + 255 * mag >= ((int64_t)1 << 31)) ok = false;
    bounds[xx][0] = xmin;
    bounds[xx][1] = xmax;
  }
  return ok;
}

// Which of the six rows output xx uses, and its first input index, as the kernel computes them:
// centre (xx + 0.5) * 2.5 has the fraction .25 (xx even) or .75 (odd), and only the first and last
// two outputs are cut by the patch's edge.
constexpr int pix_row_of(int xx) { return xx < 2 ? xx : xx >= PIX_OUT - 2 ? xx - (PIX_OUT - 2) + 4 : 2 + (xx & 1); }
constexpr int pix_first_of(int xx) { return xx < 2 ? 0 : (10 * xx - 13) >> 2; }

// The kernel's coefficients (by value in its parameter struct): the six rows.  false: pix_coeffs
// failed, or its 40 rows are not these six under pix_row_of / pix_first_of.
struct PixCoeffs { int32_t k[PIX_ROWS][PIX_TAPS]; };
inline bool pix_coeffs_pack(PixCoeffs* out) {
  int32_t kk[PIX_OUT][PIX_TAPS], bounds[PIX_OUT][2];
  if (!pix_coeffs(kk, bounds)) return false;
  bool seen[PIX_ROWS] = {};
  for (int xx = 0; xx < PIX_OUT; ++xx) {
    const int r = pix_row_of(xx);
    if (bounds[xx][0] != pix_first_of(xx)) return false;
    if (!seen[r]) { memcpy(out->k[r], kk[xx], sizeof kk[xx]); seen[r] = true; }
    else if (memcmp(out->k[r], kk[xx], sizeof kk[xx]) != 0) return false;
  }
  return true;
}

// be_observe_pixels' argument checks that need no device, in this order; NULL: fine, else the message.
inline const char* pixels_args_error(const void* patch, const void* out, const void* out_f32, int32_t radius_agent,
                                     int32_t radius_obstacle) {
  if (!patch && !out && !out_f32) return "be_observe_pixels needs patch, out or out_f32";
  if (((uintptr_t)patch & 15) || ((uintptr_t)out & 15) || ((uintptr_t)out_f32 & 15))
    return "be_observe_pixels: patch, out and out_f32 must be 16-byte aligned";
  if (radius_agent < 0 || radius_agent > PIX_MAX_RADIUS || radius_obstacle < 0 || radius_obstacle > PIX_MAX_RADIUS)
    return "be_observe_pixels: radius_agent and radius_obstacle must be in [0, 2047] (the row spans' exact range)";
  return nullptr;
}

}  // namespace behost
