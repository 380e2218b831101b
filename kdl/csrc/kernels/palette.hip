// Dominant colours: the K colours of the S x S x 3 uint8 picture the model saw, weighted by the
// h x w map of its explain / rollout row (launch.h PaletteArgs; kdl/serving/palette.py is the
// definition). Integers throughout: every sum is a uint32 or uint64 add, so no order of the atomics
// changes a bit. Two launches:
//
// palette_hist over (band of kPaletteBand rows, image). A workgroup zeroes a private histogram of
// kPaletteBins x {n, sr, sg, sb} uint32 in dynamic LDS (64 KiB), then walks its band kOverlayBand
// rows at a time: with weight 1 it stages the map rows and tables and runs the two resample passes
// of heat_upsample.h (the code heat_overlay runs), w = u >> 4; with weight 0, w = 15. A pixel of
// weight 0 adds nothing. A wave whose live lanes all hit one bin (a flat region: the worst case for
// LDS atomics) sums its four values across the wave first and adds them once. At the end the
// workgroup adds its non-empty bins into the image's global histogram.
//
// palette_cluster, one workgroup of 1024 threads per image. Thread t owns bins 4t .. 4t + 3 in
// registers: it reads them, zeroes the ones that were not zero (the next launch finds the
// workspace as the first one did), and runs steps 3 to 7 of the rule. The argmax of the start
// centres reduces a 64-bit key, value << 12 | (4095 - bin), so ties go to the lowest bin; a round
// sums each cluster's {N, Sr, Sg, Sb} per wave, then through 32 LDS words. Thread 0 sorts the K
// answers and writes the 1 + 2K words.
#include "common.h"
#include "heat_upsample.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kPaletteBand = 64;                               // output rows per workgroup of palette_hist
constexpr int kClusterThreads = 1024;
constexpr int kBinsPerThread = kPaletteBins / kClusterThreads; // 4
constexpr uint32_t kHistBytes = kPaletteBins * 4 * sizeof(uint32_t);
static_assert(kPaletteBand % kOverlayBand == 0, "a band is walked in whole overlay bands");
static_assert(kOverlayBand * kOverlayMaxTaps <= 256, "one thread per (row, tap) of a staged band");

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void palette_hist_kernel(PaletteArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];   // [kPaletteBins][4]: n, sr, sg, sb
  __shared__ uint8_t q[kClassMapMaxHW];
  __shared__ uint8_t tmp[(kOverlayMaxRows + kOverlayMaxTaps) * kOverlayMaxS];
  __shared__ int32_t ykk[kOverlayBand * kOverlayMaxTaps];
  __shared__ int32_t ymn[kOverlayBand];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63;
  const int S = a.S;
  const int band0 = blockIdx.x * kPaletteBand;                   // < S by the grid
  const int band1 = band0 + kPaletteBand < S ? band0 + kPaletteBand : S;
  const float* heat = a.out + (size_t)b * a.ldo + 2;
  const uint8_t* img = a.inp + (size_t)b * S * S * 3;

  for (int i = tid; i < kPaletteBins * 4; i += 256) hist[i] = 0u;

  for (int r0 = band0; r0 < band1; r0 += kOverlayBand) {
    const int r1 = r0 + kOverlayBand < band1 ? r0 + kOverlayBand : band1;
    __syncthreads();                                             // the zeroes / the last band's readers of tmp
    if (a.weight) {
      int row0, nrow;
      upsample_stage(heat, a.yb, a.yk, a.yks, a.h, a.w, r0, r1, tid, q, ykk, ymn, row0, nrow);
      __syncthreads();
      upsample_hpass(a.xb, a.xk, a.xks, S, a.w, row0, nrow, tid, q, tmp);
      __syncthreads();
    }
    const int npix = (r1 - r0) * S;
    for (int p0 = 0; p0 < npix; p0 += 256) {                     // every lane makes every trip
      const int p = p0 + tid;
      uint32_t wgt = 0, r = 0, g = 0, bl = 0;
      if (p < npix) {
        const int yi = p / S, x = p - yi * S;
        wgt = a.weight ? upsample_pixel(tmp, ykk, ymn, yi, x, S, a.yks) >> 4 : 15u;
        if (wgt) {
          const uint8_t* px = img + ((size_t)(r0 + yi) * S + x) * 3;   // pixel (r0 + yi, x) < (S, S): inside image b
          r = px[0];
          g = px[1];
          bl = px[2];
        }
      }
      const uint32_t bin = ((r >> 4) << 8) | ((g >> 4) << 4) | (bl >> 4);
      const unsigned long long live = __ballot(wgt != 0);
      if (!live) continue;
      const uint32_t lead = (uint32_t)__shfl((int)bin, __ffsll(live) - 1, 64);
      if (__ballot(wgt != 0 && bin != lead) == 0) {
        // one bin for the whole wave: lanes of weight 0 add 0
        const uint32_t n = wave_sum(wgt), sr = wave_sum(wgt * r), sg = wave_sum(wgt * g), sb = wave_sum(wgt * bl);
        if (lane == 0) {
          atomicAdd(&hist[4 * lead + 0], n);
          atomicAdd(&hist[4 * lead + 1], sr);
          atomicAdd(&hist[4 * lead + 2], sg);
          atomicAdd(&hist[4 * lead + 3], sb);
        }
      } else if (wgt) {
        atomicAdd(&hist[4 * bin + 0], wgt);
        atomicAdd(&hist[4 * bin + 1], wgt * r);
        atomicAdd(&hist[4 * bin + 2], wgt * g);
        atomicAdd(&hist[4 * bin + 3], wgt * bl);
      }
    }
  }
  __syncthreads();

  uint32_t* gh = a.work + (size_t)b * kPaletteBins * 4;
  for (int i = tid; i < kPaletteBins; i += 256) {
    const uint32_t n = hist[4 * i];
    if (n) {
      atomicAdd(&gh[4 * i + 0], n);
      atomicAdd(&gh[4 * i + 1], hist[4 * i + 1]);
      atomicAdd(&gh[4 * i + 2], hist[4 * i + 2]);
      atomicAdd(&gh[4 * i + 3], hist[4 * i + 3]);
    }
  }
}

__device__ __forceinline__ uint32_t dist2(uint32_t m, uint32_t c) {
  const int dr = (int)(m & 255u) - (int)(c & 255u);
  const int dg = (int)((m >> 8) & 255u) - (int)((c >> 8) & 255u);
  const int db = (int)((m >> 16) & 255u) - (int)((c >> 16) & 255u);
  return (uint32_t)(dr * dr + dg * dg + db * db);
}

// the rounded mean (s + n / 2) / n of the three channel sums, r | g << 8 | b << 16 (n > 0)
__device__ __forceinline__ uint32_t mean3(uint32_t n, uint32_t sr, uint32_t sg, uint32_t sb) {
  const uint32_t hf = n >> 1;
  return ((sr + hf) / n) | (((sg + hf) / n) << 8) | (((sb + hf) / n) << 16);
}

// the largest key of the workgroup, in every thread (sh: one word per wave)
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  __syncthreads();                                               // the last call's readers of sh
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = 0;
#pragma unroll
  for (int i = 0; i < kClusterThreads / 64; ++i) m = sh[i] > m ? sh[i] : m;
  return m;
}

__global__ __launch_bounds__(kClusterThreads) void palette_cluster_kernel(PaletteArgs a) {
  __shared__ unsigned long long red[kClusterThreads / 64];
  __shared__ uint32_t cen[kPaletteMaxK];                         // centres, r | g << 8 | b << 16
  __shared__ uint32_t acc[kPaletteMaxK * 4];                     // a round's N, Sr, Sg, Sb per cluster
  __shared__ uint32_t total;
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63;
  const int K = a.K;
  uint32_t* res = reinterpret_cast<uint32_t*>(a.out + (size_t)b * a.ldo + 2 + a.h * a.w);   // W, K x (colour, N)

  uint4* gh = reinterpret_cast<uint4*>(a.work) + (size_t)b * kPaletteBins + tid * kBinsPerThread;
  uint32_t n[kBinsPerThread], sr[kBinsPerThread], sg[kBinsPerThread], sb[kBinsPerThread], m[kBinsPerThread];
  if (tid == 0) total = 0u;
  if (tid < kPaletteMaxK * 4) acc[tid] = 0u;
  if (tid < kPaletteMaxK) cen[tid] = 0u;
  __syncthreads();
  uint32_t mine = 0;
#pragma unroll
  for (int i = 0; i < kBinsPerThread; ++i) {
    const uint4 v = gh[i];
    if (v.x | v.y | v.z | v.w) gh[i] = make_uint4(0u, 0u, 0u, 0u);   // the workspace is zero again behind this launch
    n[i] = v.x;
    sr[i] = v.y;
    sg[i] = v.z;
    sb[i] = v.w;
    m[i] = v.x ? mean3(v.x, v.y, v.z, v.w) : 0u;
    mine += v.x;
  }
  mine = wave_sum(mine);
  if (lane == 0 && mine) atomicAdd(&total, mine);
  __syncthreads();
  const uint32_t W = total;
  if (W == 0) {                                                  // an all-zero map: uniform across the workgroup
    if (tid < 1 + 2 * K) res[tid] = 0u;
    return;
  }

  // start centres: the heaviest bin, then the bin with the largest n * (distance to its nearest centre)
  uint32_t D[kBinsPerThread];
  int k = 0;
  for (int j = 0; j < K; ++j) {
    unsigned long long key = 0;
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      if (j == 0) {
        D[i] = 0xffffffffu;
      } else {
        const uint32_t d = dist2(m[i], cen[j - 1]);
        D[i] = d < D[i] ? d : D[i];
      }
      const unsigned long long val = j == 0 ? (unsigned long long)n[i] : (unsigned long long)n[i] * D[i];
      const unsigned long long ky = (val << 12) | (unsigned long long)(kPaletteBins - 1 - (tid * kBinsPerThread + i));
      key = n[i] && ky > key ? ky : key;
    }
    const unsigned long long best = block_max(key, red);
    if ((best >> 12) == 0) break;                                // fewer distinct bin means than K
    const int bin = kPaletteBins - 1 - (int)(best & (kPaletteBins - 1));
    if (tid == bin / kBinsPerThread) {
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i)
        if (i == bin % kBinsPerThread) cen[j] = m[i];
    }
    __syncthreads();
    k = j + 1;
  }

  // T rounds: assign every live bin to its nearest centre, then move the centres to the clusters' means
  for (int t = 0; t < a.T; ++t) {
    int asg[kBinsPerThread];
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      uint32_t bd = 0xffffffffu;
      asg[i] = -1;
      if (n[i])
        for (int j = 0; j < k; ++j) {
          const uint32_t d = dist2(m[i], cen[j]);
          if (d < bd) {                                          // ties stay with the lower centre
            bd = d;
            asg[i] = j;
          }
        }
    }
    __syncthreads();                                             // everyone has read cen
    if (tid < kPaletteMaxK * 4) acc[tid] = 0u;
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
      for (int i = 0; i < kBinsPerThread; ++i)
        if (asg[i] == j) {
          v0 += n[i];
          v1 += sr[i];
          v2 += sg[i];
          v3 += sb[i];
        }
      if (__ballot(v0 != 0) == 0) continue;
      v0 = wave_sum(v0);
      v1 = wave_sum(v1);
      v2 = wave_sum(v2);
      v3 = wave_sum(v3);
      if (lane == 0) {
        atomicAdd(&acc[4 * j + 0], v0);
        atomicAdd(&acc[4 * j + 1], v1);
        atomicAdd(&acc[4 * j + 2], v2);
        atomicAdd(&acc[4 * j + 3], v3);
      }
    }
    __syncthreads();
    if (tid < k && acc[4 * tid]) cen[tid] = mean3(acc[4 * tid], acc[4 * tid + 1], acc[4 * tid + 2], acc[4 * tid + 3]);
    __syncthreads();
  }

  // by N descending, ties to the lower centre; the K - k centres that do not exist are 0, 0
  if (tid == 0) {
    uint32_t col[kPaletteMaxK], cnt[kPaletteMaxK];
    for (int j = 0; j < kPaletteMaxK; ++j) {
      col[j] = j < k ? cen[j] : 0u;
      cnt[j] = j < k ? acc[4 * j] : 0u;
    }
    res[0] = W;
    for (int o = 0; o < K; ++o) {
      int bj = 0;
      bool have = false;
      for (int j = 0; j < kPaletteMaxK; ++j)
        if (j < K && cnt[j] != 0xffffffffu && (!have || cnt[j] > cnt[bj])) {
          bj = j;
          have = true;
        }
      res[1 + 2 * o] = col[bj];
      res[2 + 2 * o] = cnt[bj];
      cnt[bj] = 0xffffffffu;                                     // taken (no N reaches 2^32 - 1: the bound above)
    }
  }
}

bool valid(const PaletteArgs& a) {
  if (!a.inp || !a.out || !a.work || !a.xb || !a.xk || !a.yb || !a.yk || !a.h_xb || !a.h_yb) return false;
  if (!aligned16(a.out) || !aligned16(a.work) || !aligned16(a.xb) || !aligned16(a.xk) || !aligned16(a.yb) ||
      !aligned16(a.yk))
    return false;
  if (a.B < 1 || a.B > 65535 || a.h < 1 || a.w < 1 || (int64_t)a.h * a.w > kClassMapMaxHW) return false;
  if (a.S < a.h || a.S < a.w || a.S > kOverlayMaxS) return false;
  if (a.K < 1 || a.K > kPaletteMaxK || a.T < 1 || a.T > kPaletteMaxT || (a.weight != 0 && a.weight != 1)) return false;
  if ((int64_t)a.ldo < 2 + (int64_t)a.h * a.w + 1 + 2 * a.K) return false;
  if (a.xks < 1 || a.xks > kOverlayMaxTaps || a.yks < 1 || a.yks > kOverlayMaxTaps) return false;
  if (!valid_bounds(a.h_xb, a.S, a.w, a.xks) || !valid_bounds(a.h_yb, a.S, a.h, a.yks)) return false;
  return valid_band_rows(a.h_yb, a.S, kOverlayBand, 0);          // the map rows one staged band needs
}

}  // namespace

size_t palette_workspace(int B) { return B > 0 ? (size_t)B * kPaletteBins * 4 * sizeof(uint32_t) : 0; }

hipError_t palette(const PaletteArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.S + kPaletteBand - 1) / kPaletteBand), (unsigned)a.B);
  hipLaunchKernelGGL(palette_hist_kernel, grid, dim3(256), kHistBytes, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(palette_cluster_kernel, dim3((unsigned)a.B), dim3(kClusterThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
