// Rendered heatmap overlays: the h x w map of an explain / rollout row painted over the S x S x 3
// uint8 picture the model saw (launch.h HeatOverlayArgs; kdl/serving/overlay.py is the definition).
//
// One launch over (band of kOverlayBand output rows, image). A workgroup
//   1. quantises the map rows its band needs from the image's own output row into LDS
//      (q = rint(clamp(heat, 0, 1) * 255): one fp32 multiply, then v_rndne; nothing to contract),
//      packs the 768-byte colour table into 256 LDS dwords and copies its rows' bounds and
//      coefficients to LDS (kOverlayMaxTaps per row, zeros behind a row's taps);
//   2. runs Pillow's horizontal pass for those map rows into an LDS intermediate of at most
//      kOverlayMaxRows x S bytes, a thread per column with the column's taps in registers (a column's
//      coefficients are used by one thread only, so they do not go through LDS);
//   3. per thread and step, produces the 16 bytes of one 16-byte-aligned chunk of the output row:
//      the vertical pass once per pixel (the three channels share it), the table lookup, the blend,
//      then one 16-byte store.
// Alignment follows the STORE side. The picture starts at word 2 + h*w of a row of ldo words, so its
// first byte is 4-byte but not 16-byte aligned; chunks are cut at absolute multiples of 16, a band
// owns the chunks whose first picture byte lies in its rows (they reach at most 15 bytes into the
// rows below, whose tables the band stages too). A chunk wholly inside the picture starts inside
// some pixel, at channel ch0: the six pixels it touches are worked out as a pixel-aligned stream of
// 18 bytes (the photograph is read from the pixel's first byte on, as the 5 or 6 aligned dwords that
// hold those bytes, merged with v_alignbyte: the images sit at b * S*S*3 bytes, any residue mod 4),
// every byte position is then static, and the 16 output bytes are that stream shifted by ch0 with
// v_alignbyte again. Only the first and last chunk of an image can be partial: those go byte by
// byte, so the pad bytes of the last word and everything past them stay untouched. A dword of the
// photograph that is not wholly inside [inp, inp + B*S*S*3) is read by bytes.
// Steps 1 and 2 are the device code of heat_upsample.h, which kernels/palette.hip runs as well.
// Accumulators: uint32 from 1 << 21, += k * value, (int32) >> 22 clamped to 0..255 (Pillow's clip8).
#include "common.h"
#include "heat_upsample.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kYRows = kOverlayBand + 6;          // rows whose tables a band stages: a chunk reaches 15 bytes
                                                  // = at most 5 rows + 1 (S = 1) past the band's last row
constexpr int kTmpRows = kOverlayMaxRows + kOverlayMaxTaps;   // the taps behind a row's own (weight 0) stay in LDS

// one aligned dword at address q of an input whose bytes are [beg, end): whole where it lies
// inside, by bytes (the rest 0) at the two ends
__device__ __forceinline__ uint32_t load_dword(uintptr_t q, uintptr_t beg, uintptr_t end) {
  if (q >= beg && q + 4 <= end) return *reinterpret_cast<const uint32_t*>(q);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (q + b >= beg && q + b < end) v |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + b) << (8 * b);
  return v;
}

// the 20 bytes of the photograph from address pa on (any alignment), as 5 dwords
__device__ __forceinline__ void load_stream(uintptr_t pa, uintptr_t beg, uintptr_t end, uint32_t v[5]) {
  const uint32_t sh = (uint32_t)(pa & 3);
  const uintptr_t qa = pa - sh;                                  // aligned down
  uint32_t wd[6];
#pragma unroll
  for (int j = 0; j < 5; ++j) wd[j] = load_dword(qa + 4 * j, beg, end);
  wd[5] = sh ? load_dword(qa + 20, beg, end) : 0u;
#pragma unroll
  for (int j = 0; j < 5; ++j) v[j] = __builtin_amdgcn_alignbyte(wd[j + 1], wd[j], sh);
}

__global__ __launch_bounds__(256) void heat_overlay_kernel(HeatOverlayArgs a) {
  __shared__ uint8_t q[kClassMapMaxHW];                          // the quantised map (the band's rows of it)
  __shared__ uint8_t tmp[kTmpRows * kOverlayMaxS];               // horizontal pass of the band's map rows
  __shared__ uint32_t tab[256];                                  // r | g << 8 | b << 16
  __shared__ int32_t ykk[kYRows * kOverlayMaxTaps];              // [row of the band][tap], 0 behind the row's taps
  __shared__ int32_t ymn[kYRows];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int S = a.S, rowb = S * 3, N = S * rowb, w = a.w, yks = a.yks;
  const int r0 = blockIdx.x * kOverlayBand;                      // < S by the grid
  const int r1 = r0 + kOverlayBand < S ? r0 + kOverlayBand : S;
  const int reach = 15 / rowb + 1;                               // rows below the band a chunk can touch
  const int r1e = r1 + reach < S ? r1 + reach : S;               // r1e - r0 <= kYRows

  float* orow = a.out + (size_t)b * a.ldo;
  const uintptr_t in_beg = reinterpret_cast<uintptr_t>(a.inp), in_end = in_beg + (size_t)a.B * N;
  const uintptr_t img = in_beg + (size_t)b * N;
  uint8_t* pic = reinterpret_cast<uint8_t*>(orow + 2 + a.h * w);
  const int head = (int)(reinterpret_cast<uintptr_t>(pic) & 15);  // 0, 4, 8 or 12: the picture is word-aligned
  const int b0 = r0 * rowb, b1 = r1 * rowb;
  const int cs0 = b0 ? (b0 + head + 15) >> 4 : 0;
  const int cs1 = (b1 + head + 15) >> 4;

  // the photograph of this thread's first chunk does not wait for the tables: its loads are in
  // flight while the workgroup stages them
  int c = cs0 + tid;
  uint32_t v[5] = {0u, 0u, 0u, 0u, 0u};
  int i0 = 16 * c - head;                                        // picture byte of the chunk's byte 0: >= -12
  bool full = c < cs1 && i0 >= 0 && i0 + 16 <= N;
  int y = 0, x = 0, ch0 = 0;
  if (full) {
    y = i0 / rowb;
    const int rem = i0 - y * rowb;
    x = rem / 3;
    ch0 = rem - 3 * x;
    load_stream(img + (size_t)(i0 - ch0), in_beg, in_end, v);
  }

  // steps 1 and 2 of the rule for the band's rows: heat_upsample.h
  int row0, nrow;
  upsample_stage(orow + 2, a.yb, a.yk, yks, a.h, w, r0, r1e, tid, q, ykk, ymn, row0, nrow);
  tab[tid] = (uint32_t)a.tab[3 * tid] | ((uint32_t)a.tab[3 * tid + 1] << 8) | ((uint32_t)a.tab[3 * tid + 2] << 16);
  __syncthreads();
  upsample_hpass(a.xb, a.xk, a.xks, S, w, row0, nrow, tid, q, tmp);
  __syncthreads();

  const uint32_t A = (uint32_t)a.a;
  // the vertical pass of pixel (yy, xx) of the band
  auto pixel = [&](int yy, int xx, uint32_t& col, uint32_t& ap) {
    const uint32_t u = upsample_pixel(tmp, ykk, ymn, yy - r0, xx, S, yks);   // yy - r0 < r1e - r0: see `reach`
    col = tab[u];
    ap = a.blend ? (A * u + 127u) / 255u : A;
  };

  for (; c < cs1; c += 256) {
    if (full) {
      // six pixels from (y, x) on, a pixel-aligned stream of 18 bytes in v; every position is static
      uint32_t e[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        uint32_t col, ap;
        pixel(y, x, col, ap);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const int k = 3 * p + ch;
          const uint32_t im = (v[k >> 2] >> (8 * (k & 3))) & 255u;
          const uint32_t cc = (col >> (8 * ch)) & 255u;
          e[k >> 2] |= ((im * (256u - ap) + cc * ap + 128u) >> 8) << (8 * (k & 3));
        }
        if (p < 5 && ++x == S) {                                 // the chunk's 16 bytes end inside pixel 5
          x = 0;
          ++y;
        }
      }
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], (uint32_t)ch0);
      *reinterpret_cast<uint4*>(pic + i0) = make_uint4(o[0], o[1], o[2], o[3]);   // pic + i0: a multiple of 16
    } else {
      // the first or the last chunk of an image: byte by byte, inside the picture only
      const int lo = i0 > 0 ? i0 : 0, hi = i0 + 16 < N ? i0 + 16 : N;
      int yy = lo / rowb;
      const int rem = lo - yy * rowb;
      int xx = rem / 3;
      int ch = rem - 3 * xx;
      uint32_t col = 0, ap = 0;
      pixel(yy, xx, col, ap);
#pragma unroll 1
      for (int i = lo; i < hi; ++i) {
        const uint32_t im = *reinterpret_cast<const uint8_t*>(img + (size_t)i);   // 0 <= i < N: inside image b
        const uint32_t cc = (col >> (8 * ch)) & 255u;
        pic[i] = (uint8_t)((im * (256u - ap) + cc * ap + 128u) >> 8);
        if (++ch == 3 && i + 1 < hi) {
          ch = 0;
          if (++xx == S) {
            xx = 0;
            ++yy;
          }
          pixel(yy, xx, col, ap);
        }
      }
    }
    // the next chunk of this thread
    const int cn = c + 256;
    i0 = 16 * cn - head;
    full = cn < cs1 && i0 + 16 <= N;                             // i0 > 0 from the second step on
    if (full) {
      y = i0 / rowb;
      const int rem = i0 - y * rowb;
      x = rem / 3;
      ch0 = rem - 3 * x;
      load_stream(img + (size_t)(i0 - ch0), in_beg, in_end, v);
    }
  }
}

bool valid(const HeatOverlayArgs& a) {
  if (!a.inp || !a.out || !a.tab || !a.xb || !a.xk || !a.yb || !a.yk || !a.h_xb || !a.h_yb) return false;
  if (!aligned16(a.out) || !aligned16(a.tab) || !aligned16(a.xb) || !aligned16(a.xk) || !aligned16(a.yb) ||
      !aligned16(a.yk))
    return false;
  if (a.B < 1 || a.B > 65535 || a.h < 1 || a.w < 1 || (int64_t)a.h * a.w > kClassMapMaxHW) return false;
  if (a.S < a.h || a.S < a.w || a.S > kOverlayMaxS) return false;
  const int64_t words = ((int64_t)a.S * a.S * 3 + 3) / 4;
  if ((int64_t)a.ldo < 2 + (int64_t)a.h * a.w + words) return false;
  if (a.a < 0 || a.a > 256 || (a.blend != 0 && a.blend != 1)) return false;
  if (a.xks < 1 || a.xks > kOverlayMaxTaps || a.yks < 1 || a.yks > kOverlayMaxTaps) return false;
  if (!valid_bounds(a.h_xb, a.S, a.w, a.xks) || !valid_bounds(a.h_yb, a.S, a.h, a.yks)) return false;
  return valid_band_rows(a.h_yb, a.S, kOverlayBand, 15 / (a.S * 3) + 1);   // the map rows one workgroup stages
}

}  // namespace

hipError_t heat_overlay(const HeatOverlayArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.S + kOverlayBand - 1) / kOverlayBand), (unsigned)a.B);
  hipLaunchKernelGGL(heat_overlay_kernel, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
