// Garment cutouts: the S x S x 3 uint8 picture the model saw with an alpha channel, the backdrop made
// transparent by a colour model that the h x w map of its explain / rollout row seeds (launch.h
// CutoutArgs; kdl/serving/cutout.py is the definition). Integers throughout: every sum is a uint32 add
// and every decision one 64-bit compare, so no order of the atomics changes a bit. Three launches:
//
// cutout_hist over (band of kCutHistBand rows, image). A workgroup zeroes private tables N, G and F
// of kPaletteBins uint32 each in dynamic LDS (48 KiB), then walks its band kOverlayBand rows at a
// time through the two resample passes of heat_upsample.h (the code heat_overlay and palette_hist
// run). A wave takes one (row, 64 columns) item at a time: N[bin] += 1, G[bin] += u >= gate,
// F[bin] += u, and lane 0 stores the wave's ballot of u >= gate as one 64-bit word of the image's
// gate mask: S rows of ceil(S / 64) words, so a word never straddles rows and the bits at and behind
// column S are 0. A wave whose live lanes all hit one bin (a flat region: the worst case for LDS
// atomics) adds its three sums once. At the end the workgroup adds its non-empty bins into the
// image's global tables.
//
// cutout_bins, one workgroup of 1024 threads per image. Thread t owns bins 4t .. 4t + 3 in registers:
// it reads them, zeroes the ones that were not zero (the next launch finds the tables as the first
// one did) and runs the R + 1 rounds of step 4, which need no pixels: a workgroup sum gives TF, then
// one 64-bit compare per bin. The 4096 colour bits go to the workspace, and thread 0 zeroes the
// row's count word.
//
// cutout_render over (band of kCutBand rows, image). The workgroup builds the raw mask fg[bin] & ok
// of its rows and M + 1 rows above and below as bit rows in LDS (the halo is recomputed, never
// exchanged), runs the M majority rounds bit-parallel (a thread per 64 columns: two full adders per
// row, then a carry-save sum of the three rows), and writes r | g << 8 | b << 16 | a << 24 per pixel,
// four words per 16-byte store wherever the four lie inside the band. The band's garment pixels go
// into the row's count word by one atomic per workgroup.
#include "common.h"
#include "heat_upsample.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kCutHistBand = 64;                               // output rows per workgroup of cutout_hist
constexpr int kCutBand = 32;                                   // output rows per workgroup of cutout_render
constexpr int kBinThreads = 1024;
constexpr int kBinsPerThread = kPaletteBins / kBinThreads;     // 4
constexpr int kFgWords = kPaletteBins / 32;                    // 128
constexpr uint32_t kTableBytes = 3 * kPaletteBins * sizeof(uint32_t);
constexpr int kMaskWords = kOverlayMaxS / 64;                  // 16
constexpr int kRowStride = kMaskWords + 2;                     // one zero word before and behind a bit row
constexpr int kMaxRows = kCutBand + 2 * (kCutoutMaxSmooth + 1);
static_assert(kCutHistBand % kOverlayBand == 0, "a band is walked in whole overlay bands");
static_assert(kOverlayBand * kOverlayMaxTaps <= 256, "one thread per (row, tap) of a staged band");
static_assert(kBinsPerThread == 4, "a thread's bins are one uint4 of each table");
static_assert(kOverlayMaxS % 64 == 0, "whole mask words");

// one image's part of the workspace: N, G, F, the colour bits, the gate mask
struct Layout {
  int wpr;                // 64-bit words per mask row
  size_t fg, mask, image; // byte offsets of the colour bits and of the mask; bytes of the image
};
__host__ __device__ inline Layout layout(int S) {
  Layout l;
  l.wpr = (S + 63) / 64;
  l.fg = kTableBytes;
  l.mask = l.fg + kFgWords * sizeof(uint32_t);
  l.image = l.mask + ((size_t)S * l.wpr * 8 + 15) / 16 * 16;
  return l;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ uint32_t bin_of(const uint8_t* px) {
  return ((uint32_t)(px[0] >> 4) << 8) | ((uint32_t)(px[1] >> 4) << 4) | (uint32_t)(px[2] >> 4);
}

__global__ __launch_bounds__(256) void cutout_hist_kernel(CutoutArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t tab[];    // N, G, F: [kPaletteBins] each
  __shared__ uint8_t q[kClassMapMaxHW];
  __shared__ uint8_t tmp[(kOverlayMaxRows + kOverlayMaxTaps) * kOverlayMaxS];
  __shared__ int32_t ykk[kOverlayBand * kOverlayMaxTaps];
  __shared__ int32_t ymn[kOverlayBand];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int S = a.S;
  const uint32_t gate = (uint32_t)a.gate;
  const Layout L = layout(S);
  const int band0 = blockIdx.x * kCutHistBand;                   // < S by the grid
  const int band1 = band0 + kCutHistBand < S ? band0 + kCutHistBand : S;
  const float* heat = a.out + (size_t)b * a.ldo + 2;
  const uint8_t* img = a.inp + (size_t)b * S * S * 3;
  uint8_t* base = a.work + (size_t)b * L.image;
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(base + L.mask);
  uint32_t* tN = tab;
  uint32_t* tG = tab + kPaletteBins;
  uint32_t* tF = tab + 2 * kPaletteBins;

  for (int i = tid; i < 3 * kPaletteBins; i += 256) tab[i] = 0u;

  for (int r0 = band0; r0 < band1; r0 += kOverlayBand) {
    const int r1 = r0 + kOverlayBand < band1 ? r0 + kOverlayBand : band1;
    __syncthreads();                                             // the zeroes / the last band's readers of tmp
    int row0, nrow;
    upsample_stage(heat, a.yb, a.yk, a.yks, a.h, a.w, r0, r1, tid, q, ykk, ymn, row0, nrow);
    __syncthreads();
    upsample_hpass(a.xb, a.xk, a.xks, S, a.w, row0, nrow, tid, q, tmp);
    __syncthreads();
    const int items = (r1 - r0) * L.wpr;                         // (row of the band, word of the row)
    for (int it = wave; it < items; it += 4) {                   // uniform per wave
      const int yi = it / L.wpr, wd = it - yi * L.wpr, x = wd * 64 + lane;
      const bool live = x < S;                                   // lane 0 always is: wd < ceil(S / 64)
      uint32_t u = 0, bin = 0;
      if (live) {
        u = upsample_pixel(tmp, ykk, ymn, yi, x, S, a.yks);
        bin = bin_of(img + ((size_t)(r0 + yi) * S + x) * 3);     // pixel (r0 + yi, x) < (S, S): inside image b
      }
      const bool ok = live && u >= gate;
      const unsigned long long okm = __ballot(ok), lv = __ballot(live);
      if (lane == 0) mask[(size_t)(r0 + yi) * L.wpr + wd] = okm; // row r0 + yi < S, word wd < wpr: inside the mask
      const uint32_t lead = (uint32_t)__shfl((int)bin, 0, 64);
      if (__ballot(live && bin != lead) == 0) {
        // one bin for the whole wave: dead lanes add 0
        const uint32_t f = wave_sum(u);
        if (lane == 0) {
          atomicAdd(&tN[lead], (uint32_t)__popcll(lv));
          if (okm) atomicAdd(&tG[lead], (uint32_t)__popcll(okm));
          if (f) atomicAdd(&tF[lead], f);
        }
      } else if (live) {
        atomicAdd(&tN[bin], 1u);
        if (ok) atomicAdd(&tG[bin], 1u);
        if (u) atomicAdd(&tF[bin], u);
      }
    }
  }
  __syncthreads();

  uint32_t* gN = reinterpret_cast<uint32_t*>(base);
  for (int i = tid; i < kPaletteBins; i += 256) {
    const uint32_t n = tN[i];
    if (n) {                                                     // G and F of an empty bin are 0
      atomicAdd(&gN[i], n);
      const uint32_t g = tG[i], f = tF[i];
      if (g) atomicAdd(&gN[kPaletteBins + i], g);
      if (f) atomicAdd(&gN[2 * kPaletteBins + i], f);
    }
  }
}

// the sum of the workgroup, in every thread (sh: one word per wave)
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* sh) {
  v = wave_sum(v);
  __syncthreads();                                               // the last call's readers of sh
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < kBinThreads / 64; ++i) s += sh[i];
  return s;
}

__global__ __launch_bounds__(kBinThreads) void cutout_bins_kernel(CutoutArgs a) {
  __shared__ uint32_t red[kBinThreads / 64];
  __shared__ uint32_t fgw[kFgWords];
  const int tid = threadIdx.x, b = blockIdx.x;
  const Layout L = layout(a.S);
  uint8_t* base = a.work + (size_t)b * L.image;
  uint4* gt = reinterpret_cast<uint4*>(base);
  constexpr int kQuads = kPaletteBins / 4;                       // uint4s per table
  const uint4 vn = gt[tid], vg = gt[kQuads + tid], vf = gt[2 * kQuads + tid];
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  if (vn.x | vn.y | vn.z | vn.w) gt[tid] = zero;                 // the tables are zero again behind this launch
  if (vg.x | vg.y | vg.z | vg.w) gt[kQuads + tid] = zero;
  if (vf.x | vf.y | vf.z | vf.w) gt[2 * kQuads + tid] = zero;
  const uint32_t n[kBinsPerThread] = {vn.x, vn.y, vn.z, vn.w}, g[kBinsPerThread] = {vg.x, vg.y, vg.z, vg.w};
  uint32_t f[kBinsPerThread] = {vf.x, vf.y, vf.z, vf.w};
  if (tid < kFgWords) fgw[tid] = 0u;

  const unsigned long long full = 255ull * (unsigned long long)a.S * (unsigned long long)a.S;   // < 2^28
  uint32_t bits = 0;
  for (int t = 0; t <= a.rounds; ++t) {
    const unsigned long long TF = block_sum(f[0] + f[1] + f[2] + f[3], red);   // <= full: no uint32 wraps
    const unsigned long long TB = full - TF;
    bits = 0;
#pragma unroll
    for (int i = 0; i < kBinsPerThread; ++i) {
      const unsigned long long F = f[i], Bk = 255ull * n[i] - F; // F <= 255 N: u <= 255, G <= N
      const bool on = n[i] != 0u && F * TB >= Bk * TF;           // both products < 2^54
      bits |= on ? 1u << i : 0u;
      f[i] = on ? 255u * g[i] : 0u;
    }
  }
  // block_sum's last barrier is behind the zeroes of fgw
  if (bits) atomicOr(&fgw[tid >> 3], bits << ((tid & 7) * 4));   // bin 4 tid + i: word (4 tid + i) / 32, bit (4 tid + i) % 32
  __syncthreads();
  if (tid < kFgWords) reinterpret_cast<uint32_t*>(base + L.fg)[tid] = fgw[tid];
  if (tid == 0) reinterpret_cast<uint32_t*>(a.out + (size_t)b * a.ldo + 2 + a.h * a.w)[0] = 0u;   // count
}

// the three mask bits of columns x - 1, x, x + 1 of a padded bit row (bit 64 + x of the row is column x)
__device__ __forceinline__ uint32_t win3(const unsigned long long* row, int x) {
  const int pos = 63 + x, k = pos >> 6, off = pos & 63;          // k <= wpr; off > 61 needs word k + 1 <= wpr + 1
  unsigned long long v = row[k] >> off;
  if (off > 61) v |= row[k + 1] << (64 - off);
  return (uint32_t)v & 7u;
}

// per column of 64: the low and high bit of (left + centre + right) of one padded bit row at word p
__device__ __forceinline__ void hsum(const unsigned long long* p, unsigned long long& s, unsigned long long& c) {
  const unsigned long long m = p[0], l = (m << 1) | (p[-1] >> 63), r = (m >> 1) | (p[1] << 63);
  s = l ^ m ^ r;
  c = (l & m) | (l & r) | (m & r);
}

__global__ __launch_bounds__(256) void cutout_render_kernel(CutoutArgs a) {
  __shared__ unsigned long long rows[2][kMaxRows * kRowStride];
  __shared__ uint32_t fg[kFgWords];
  __shared__ uint32_t band_count;
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int S = a.S, M = a.smooth;
  const Layout L = layout(S);
  const int wpr = L.wpr;
  const int band0 = blockIdx.x * kCutBand;                       // < S by the grid
  const int band1 = band0 + kCutBand < S ? band0 + kCutBand : S;
  const int e0 = band0 - (M + 1), nrows = band1 - band0 + 2 * (M + 1);   // <= kMaxRows; rows outside the picture are unset
  const uint8_t* img = a.inp + (size_t)b * S * S * 3;
  const uint8_t* base = a.work + (size_t)b * L.image;
  const unsigned long long* mask = reinterpret_cast<const unsigned long long*>(base + L.mask);
  uint32_t* res = reinterpret_cast<uint32_t*>(a.out + (size_t)b * a.ldo + 2 + a.h * a.w);   // count, S*S pixels

  if (tid < kFgWords) fg[tid] = reinterpret_cast<const uint32_t*>(base + L.fg)[tid];
  if (tid == 0) band_count = 0u;
  for (int i = tid; i < 2 * nrows; i += 256) {                   // the zero words around every row of both buffers
    unsigned long long* r = rows[i & 1] + (i >> 1) * kRowStride;
    r[0] = 0ull;
    r[wpr + 1] = 0ull;
  }
  __syncthreads();

  // the raw mask: fg[bin] & ok
  for (int it = wave; it < nrows * wpr; it += 4) {               // uniform per wave
    const int i = it / wpr, wd = it - i * wpr, y = e0 + i, x = wd * 64 + lane;
    unsigned long long m = 0ull;
    if (y >= 0 && y < S) {                                       // uniform per wave
      bool on = false;
      if (x < S && ((mask[(size_t)y * wpr + wd] >> lane) & 1ull)) {   // row y < S, word wd < wpr: inside the mask
        const uint32_t bin = bin_of(img + ((size_t)y * S + x) * 3);    // pixel (y, x) < (S, S): inside image b
        on = (fg[bin >> 5] >> (bin & 31u)) & 1u;
      }
      m = __ballot(on);
    }
    if (lane == 0) rows[0][i * kRowStride + wd + 1] = m;
  }
  __syncthreads();

  // M majority rounds. After round r the rows r .. nrows - 1 - r are the rule's; the others are never
  // read by a row that is kept. The last word's bits at and behind column S stay 0.
  const unsigned long long last = (S & 63) ? (1ull << (S & 63)) - 1ull : ~0ull;
  int cur = 0;
  for (int r = 0; r < M; ++r) {
    const unsigned long long* src = rows[cur];
    unsigned long long* dst = rows[cur ^ 1];
    for (int it = tid; it < nrows * wpr; it += 256) {
      const int i = it / wpr, wd = it - i * wpr, y = e0 + i;
      unsigned long long v = 0ull;
      if (i > 0 && i < nrows - 1 && y >= 0 && y < S) {
        const unsigned long long* mid = src + i * kRowStride + wd + 1;
        unsigned long long a0, a1, b0, b1, c0, c1;
        hsum(mid - kRowStride, a0, a1);
        hsum(mid, b0, b1);
        hsum(mid + kRowStride, c0, c1);
        const unsigned long long s0 = a0 ^ b0 ^ c0, k0 = (a0 & b0) | (a0 & c0) | (b0 & c0);   // weights 1, 2
        const unsigned long long s1 = a1 ^ b1 ^ c1, k1 = (a1 & b1) | (a1 & c1) | (b1 & c1);   // weights 2, 4
        const unsigned long long t1 = s1 ^ k0, k2 = s1 & k0;                                   // weights 2, 4
        const unsigned long long t2 = k1 ^ k2, t3 = k1 & k2;                                   // weights 4, 8
        v = t3 | (t2 & (t1 | s0));                               // the count s0 + 2 t1 + 4 t2 + 8 t3 >= 5
        if (wd == wpr - 1) v &= last;
      }
      dst[i * kRowStride + wd + 1] = v;
    }
    __syncthreads();
    cur ^= 1;
  }

  // the pixels of the band, in quads of words that are 16-byte aligned in memory
  const unsigned long long* fin = rows[cur];
  uint32_t* pix = res + 1;
  const long long wa = (long long)(reinterpret_cast<uintptr_t>(pix) >> 2);   // the word address of pixel 0
  const long long P0 = (long long)band0 * S, P1 = (long long)band1 * S;      // this band's pixels of the image
  const long long q0 = (wa + P0) >> 2, q1 = (wa + P1 - 1) >> 2;
  uint32_t mine = 0;
  for (long long qd = q0 + tid; qd <= q1; qd += 256) {
    uint32_t wv[4];
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long p = 4 * qd + j - wa;
      in[j] = p >= P0 && p < P1;
      wv[j] = 0u;
      if (in[j]) {
        const int y = (int)(p / S), x = (int)(p - (long long)y * S), i = y - e0;   // M + 1 <= i <= nrows - 2 - M
        const unsigned long long* mid = fin + i * kRowStride;
        const uint32_t wm = win3(mid, x);
        const uint32_t c = (uint32_t)(__popc(win3(mid - kRowStride, x)) + __popc(wm) + __popc(win3(mid + kRowStride, x)));
        const uint32_t m = (wm >> 1) & 1u;
        const uint32_t al = a.feather ? (255u * c + 4u) / 9u : 255u * m;
        const uint8_t* px = img + (size_t)p * 3;                 // pixel p < S*S: inside image b
        wv[j] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16) | (al << 24);
        mine += m;
      }
    }
    if (in[0] && in[3]) {                                        // all four inside the band: one 16-byte store
      *reinterpret_cast<uint4*>(pix + (4 * qd - wa)) = make_uint4(wv[0], wv[1], wv[2], wv[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (in[j]) pix[4 * qd + j - wa] = wv[j];
    }
  }
  mine = wave_sum(mine);
  if (lane == 0 && mine) atomicAdd(&band_count, mine);
  __syncthreads();
  if (tid == 0 && band_count) atomicAdd(res, band_count);        // cutout_bins zeroed the word
}

bool valid(const CutoutArgs& a) {
  if (!a.inp || !a.out || !a.work || !a.xb || !a.xk || !a.yb || !a.yk || !a.h_xb || !a.h_yb) return false;
  if (!aligned16(a.out) || !aligned16(a.work) || !aligned16(a.xb) || !aligned16(a.xk) || !aligned16(a.yb) ||
      !aligned16(a.yk))
    return false;
  if (a.B < 1 || a.B > 65535 || a.h < 1 || a.w < 1 || (int64_t)a.h * a.w > kClassMapMaxHW) return false;
  if (a.S < a.h || a.S < a.w || a.S > kOverlayMaxS) return false;
  if (a.gate < 1 || a.gate > 255 || a.rounds < 0 || a.rounds > kCutoutMaxRounds || a.smooth < 0 ||
      a.smooth > kCutoutMaxSmooth || (a.feather != 0 && a.feather != 1))
    return false;
  if ((int64_t)a.ldo < 2 + (int64_t)a.h * a.w + 1 + (int64_t)a.S * a.S) return false;
  if (a.xks < 1 || a.xks > kOverlayMaxTaps || a.yks < 1 || a.yks > kOverlayMaxTaps) return false;
  if (!valid_bounds(a.h_xb, a.S, a.w, a.xks) || !valid_bounds(a.h_yb, a.S, a.h, a.yks)) return false;
  return valid_band_rows(a.h_yb, a.S, kOverlayBand, 0);          // the map rows one staged band needs
}

}  // namespace

size_t cutout_workspace(int B, int S) {
  return B > 0 && S > 0 && S <= kOverlayMaxS ? (size_t)B * layout(S).image : 0;
}

hipError_t cutout(const CutoutArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const dim3 hgrid((unsigned)((a.S + kCutHistBand - 1) / kCutHistBand), (unsigned)a.B);
  hipLaunchKernelGGL(cutout_hist_kernel, hgrid, dim3(256), kTableBytes, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cutout_bins_kernel, dim3((unsigned)a.B), dim3(kBinThreads), 0, s, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 rgrid((unsigned)((a.S + kCutBand - 1) / kCutBand), (unsigned)a.B);
  hipLaunchKernelGGL(cutout_render_kernel, rgrid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
