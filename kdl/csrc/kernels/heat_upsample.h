// The heatmap upsample that kernels/overlay.hip and kernels/palette.hip share: steps 1 and 2 of
// kdl/serving/overlay.py (quantise the h x w fp32 map, then Pillow's two "L" resample passes onto
// S x S) for one band of output rows, a workgroup of 256 threads at a time, and the host checks of
// the tables it follows. The caller owns the LDS arrays:
//   q    uint8 [kClassMapMaxHW]                         the quantised map (the band's rows of it)
//   tmp  uint8 [(kOverlayMaxRows + kOverlayMaxTaps) * kOverlayMaxS]   the horizontal pass of those rows
//   ykk  int32 [rows * kOverlayMaxTaps]                 [row of the band][tap], 0 behind the row's taps
//   ymn  int32 [rows]                                   first staged map row of each row of the band
// with rows >= r1e - r0 and rows * kOverlayMaxTaps <= 256.
// Accumulators: uint32 from 1 << 21, += k * value, (int32) >> 22 clamped to 0..255 (Pillow's clip8).
#pragma once
#include "common.h"
#include "launch.h"
#include "runtime/resample.h"

namespace kdl {

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
  const int32_t v = (int32_t)acc >> kResampleBits;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Stage what the output rows [r0, r1e) need: the quantised map rows (q = rint(clamp(heat, 0, 1) * 255):
// one fp32 multiply, then v_rndne; nothing to contract) and the rows' bounds and coefficients. The
// tables live in device memory: the host checked its copies, every value read here is clamped to
// what is staged all the same. The caller synchronises behind it.
__device__ __forceinline__ void upsample_stage(const float* heat, const int32_t* yb, const int32_t* yk, int yks,
                                               int h, int w, int r0, int r1e, int tid, uint8_t* q, int32_t* ykk,
                                               int32_t* ymn, int& row0, int& nrow) {
  row0 = clampi(yb[2 * r0], 0, h);
  nrow = clampi(yb[2 * (r1e - 1)] + yb[2 * (r1e - 1) + 1], row0, h) - row0;
  nrow = nrow < kOverlayMaxRows ? nrow : kOverlayMaxRows;
  for (int p = row0 * w + tid; p < (row0 + nrow) * w; p += 256) {
    float f = heat[p];
    f = f > 0.f ? f : 0.f;                                       // NaN -> 0
    f = f < 1.f ? f : 1.f;
    q[p] = (uint8_t)__builtin_rintf(f * 255.0f);
  }
  if (tid < (r1e - r0) * kOverlayMaxTaps) {
    const int i = tid / kOverlayMaxTaps, t = tid - i * kOverlayMaxTaps, yy = r0 + i;
    const int mn = clampi(yb[2 * yy], row0, row0 + nrow) - row0;
    int n = clampi(yb[2 * yy + 1], 0, yks);
    n = n < nrow - mn ? n : nrow - mn;
    ykk[tid] = t < n ? yk[(size_t)yy * yks + t] : 0;
    if (t == 0) ymn[i] = mn;
  }
}

// Pillow's horizontal pass of the staged map rows into tmp [nrow][S], a thread per column with the
// column's taps in registers (a column's coefficients are used by one thread only, so they do not
// go through LDS). The caller synchronises behind it.
__device__ __forceinline__ void upsample_hpass(const int32_t* xb, const int32_t* xk, int xks, int S, int w, int row0,
                                               int nrow, int tid, const uint8_t* q, uint8_t* tmp) {
  for (int xx = tid; xx < S; xx += 256) {
    const int mn = clampi(xb[2 * xx], 0, w);
    int n = clampi(xb[2 * xx + 1], 0, xks);
    n = n < w - mn ? n : w - mn;
    uint32_t k[kOverlayMaxTaps];
#pragma unroll
    for (int t = 0; t < kOverlayMaxTaps; ++t) k[t] = t < n ? (uint32_t)xk[(size_t)xx * xks + t] : 0u;
    for (int r = 0; r < nrow; ++r) {
      const uint8_t* qr = q + (row0 + r) * w + mn;
      uint32_t acc = 1u << (kResampleBits - 1);
#pragma unroll
      for (int t = 0; t < kOverlayMaxTaps; ++t)
        if (t < n) acc += k[t] * qr[t];
      tmp[r * S + xx] = (uint8_t)clip8(acc);
    }
  }
}

// The vertical pass of pixel (r0 + yi, xx) of the band: the upsampled value u, 0..255.
// mn + t < kOverlayMaxRows + kOverlayMaxTaps, and a tap behind the row's own has weight 0.
__device__ __forceinline__ uint32_t upsample_pixel(const uint8_t* tmp, const int32_t* ykk, const int32_t* ymn,
                                                   int yi, int xx, int S, int yks) {
  const uint8_t* t0 = tmp + ymn[yi] * S + xx;
  const int32_t* kk = ykk + yi * kOverlayMaxTaps;
  uint32_t acc = 1u << (kResampleBits - 1);
#pragma unroll
  for (int t = 0; t < kOverlayMaxTaps; ++t)
    if (t < yks) acc += (uint32_t)kk[t] * t0[t * S];             // yks is uniform: no divergence
  return clip8(acc);
}

// bounds [S][2] of one axis against a map of `in` samples: every tap inside the map, at most
// `ks` of them, and neither end stepping back (Pillow's rule: a run of outputs then needs the
// samples [bounds[first].min, bounds[last].min + n))
inline bool valid_bounds(const int32_t* bd, int S, int in, int ks) {
  int32_t pmn = 0, pend = 0;
  for (int i = 0; i < S; ++i) {
    const int32_t mn = bd[2 * i], n = bd[2 * i + 1];
    if (mn < 0 || n < 0 || n > ks || mn > in || n > in - mn) return false;
    if (mn < pmn || mn + n < pend) return false;
    pmn = mn;
    pend = mn + n;
  }
  return true;
}

// no run of `band` output rows (plus `reach` rows below it) needs more than kOverlayMaxRows map rows
inline bool valid_band_rows(const int32_t* yb, int S, int band, int reach) {
  for (int r0 = 0; r0 < S; r0 += band) {
    int r1 = r0 + band + reach;
    r1 = r1 < S ? r1 : S;
    if (yb[2 * (r1 - 1)] + yb[2 * (r1 - 1) + 1] - yb[2 * r0] > kOverlayMaxRows) return false;
  }
  return true;
}

inline bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace kdl
