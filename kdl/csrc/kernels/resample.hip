// Pillow's filtered resize (+ center crop) of uint8 RGB on the GPU, bit for bit.
//
// Image.resize with BOX / BILINEAR / HAMMING / BICUBIC / LANCZOS is integer arithmetic: two
// separable passes, 22-bit fixed-point coefficients, a uint8 intermediate. The host builds the
// tables (runtime/resample.cpp, a port of precompute_coeffs); a crop window is a slice of them.
// Two launches cover all images of a request, each with its own source size:
//   resample_h_u8  horizontal pass over the source rows the vertical pass will read and the OW
//                  output columns only. A workgroup owns CW columns x a band of rows: the
//                  coefficients of its columns go to LDS once, the source span of the columns
//                  is staged in LDS per group of rows, one dword per pixel (a tap is then one
//                  LDS read for the pixel and one for its coefficient), each thread accumulates
//                  output pixels. Raw kind: packed [H][W][3] pixels, loaded as aligned dwords
//                  (aligned down, the edges of the image by bytes) and unpacked. JPEG kind: the
//                  sample planes of jpeg_idct_u8; every source pixel is converted once by
//                  jpeg_pixel() on its way into LDS, so the full-size RGB image never exists.
//   resample_v_u8  vertical pass down the intermediate ([rows][align4(OW*3)] per image), four
//                  bytes of an output row per thread, into the image's row of the batch.
// Accumulator: uint32 from 1 << 21, += kk * pixel, (int32) >> 22 clamped to 0..255 (Pillow's clip8).
#include "common.h"
#include "launch.h"
#include "runtime/jpeg.h"
#include "runtime/resample.h"

namespace kdl {

namespace {

constexpr int kSpanMax = 2048;                    // source pixels of one staged row
constexpr int kCoefMax = 4096;                    // coefficients of a workgroup's columns
constexpr int kPixWords = kSpanMax;               // staged rows share this many LDS dwords, one per pixel
constexpr int kBand = 16;                         // source rows per workgroup
constexpr int kColsMax = 64;

__device__ __forceinline__ uint8_t clip8(uint32_t acc) {
  const int32_t v = (int32_t)acc >> kResampleBits;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// one aligned dword of a raw image whose bytes are [img, end): whole where it lies inside, by
// bytes (the rest 0) at the first / last bytes of the image
__device__ __forceinline__ uint32_t load_dword(const uint8_t* q, const uint8_t* img, const uint8_t* end) {
  if (q >= img && q + 4 <= end) return *reinterpret_cast<const uint32_t*>(q);
  uint32_t v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (q + b >= img && q + b < end) v |= (uint32_t)q[b] << (8 * b);
  return v;
}

// KIND 0: raw packed pixels, 1: JPEG sample planes. cw: columns per workgroup (a power of two).
template <int KIND>
__global__ __launch_bounds__(256) void resample_h_kernel(ResampleArgs a, int cw) {
  __shared__ uint32_t pixw[kPixWords];                          // staged rows: one dword (R | G << 8 | B << 16) per pixel
  __shared__ int32_t kks[kCoefMax];
  const ResampleDesc& d = a.desc[blockIdx.z];
  const int band0 = blockIdx.y * kBand;
  if (band0 >= d.rows) return;                                  // uniform per workgroup
  const int band1 = band0 + kBand < d.rows ? band0 + kBand : d.rows;
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * cw;                               // < OW by the grid
  const int nc = cw < a.OW - c0 ? cw : a.OW - c0;
  const int* xb = reinterpret_cast<const int*>(d.xb);
  const int* xk = reinterpret_cast<const int*>(d.xk);
  const int ks = d.xksize;

  // the tables live in device memory: the host cannot vouch for their contents, so every value
  // read from them is clamped to what was staged
  const int x0 = clampi(xb[2 * c0], 0, d.W);
  int span = clampi(xb[2 * (c0 + nc - 1)] + xb[2 * (c0 + nc - 1) + 1], x0, d.W) - x0;
  span = span < kSpanMax ? span : kSpanMax;
  const int rs = span > 0 ? span : 1;                           // LDS dwords of a staged row
  // rows staged together: as many as fit, so their loads are in flight at once and the band
  // costs few barriers
  int rows_it = kPixWords / rs;                                 // >= 1: rs <= kSpanMax
  rows_it = rows_it < kBand ? rows_it : kBand;
  const int rstep = 256 / cw;                                   // rows the threads cover per step

  for (int i = tid; i < nc * ks; i += 256) {                    // cw * ks <= kCoefMax (launcher)
    const int c = i / ks, t = i - c * ks;
    kks[t * cw + c] = xk[(size_t)(c0 + c) * ks + t];
  }
  const int tx = tid & (cw - 1), ty = tid / cw;
  int mn = 0, n = 0;
  if (tx < nc) {
    mn = clampi(xb[2 * (c0 + tx)], x0, x0 + span);
    n = clampi(xb[2 * (c0 + tx) + 1], 0, ks);
    n = n < x0 + span - mn ? n : x0 + span - mn;
  }
  const int tstride = (a.OW * 3 + 3) & ~3;
  uint8_t* tmp = a.tmp + d.tmp_off;

  for (int r0 = band0; r0 < band1; r0 += rows_it) {
    const int nr = rows_it < band1 - r0 ? rows_it : band1 - r0;
    if (KIND == 0) {
      // wide loads: a thread takes 4 pixels = 12 bytes, as the 4 aligned dwords that hold them
      // (rows start at y * W * 3 bytes, any alignment), shifted into place and unpacked
      const uint8_t* img = reinterpret_cast<const uint8_t*>(d.src);
      const uint8_t* end = img + (size_t)d.H * d.W * 3;
      const int ng = (span + 3) >> 2;
      for (int i = tid; i < nr * ng; i += 256) {
        const int j = i / ng, g = i - j * ng;
        const uint8_t* p = img + ((size_t)(d.row0 + r0 + j) * d.W + x0 + 4 * g) * 3;
        const int head = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        const uint8_t* q = p - head;                            // aligned down
        uint32_t w0 = load_dword(q, img, end), w1 = load_dword(q + 4, img, end), w2 = load_dword(q + 8, img, end);
        if (head) {
          const uint32_t w3 = load_dword(q + 12, img, end);
          const int sh = 8 * head;
          w0 = (w0 >> sh) | (w1 << (32 - sh));
          w1 = (w1 >> sh) | (w2 << (32 - sh));
          w2 = (w2 >> sh) | (w3 << (32 - sh));
        }
        const uint32_t px[4] = {w0 & 0xffffffu, (w0 >> 24) | ((w1 & 0xffffu) << 8), (w1 >> 16) | ((w2 & 0xffu) << 16),
                                w2 >> 8};
        uint32_t* o = pixw + j * rs + 4 * g;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (4 * g + e < span) o[e] = px[e];
      }
    } else {
      const JpegDesc& jd = a.jdesc[d.src];
      for (int i = tid; i < nr * span; i += 256) {
        const int j = i / span, x = i - j * span;
        uint8_t rgb[3];
        jpeg_pixel(jd, a.planes, d.row0 + r0 + j, x0 + x, rgb);
        pixw[j * rs + x] = (uint32_t)rgb[0] | ((uint32_t)rgb[1] << 8) | ((uint32_t)rgb[2] << 16);
      }
    }
    __syncthreads();
    for (int r = ty; tx < nc && r < nr; r += rstep) {
      const uint32_t* p = pixw + r * rs + (mn - x0);
      uint32_t s0 = 1u << (kResampleBits - 1), s1 = s0, s2 = s0;
      for (int t = 0; t < n; ++t) {
        const uint32_t k = (uint32_t)kks[t * cw + tx], v = p[t];
        s0 += k * (v & 255u);
        s1 += k * ((v >> 8) & 255u);
        s2 += k * (v >> 16);
      }
      uint8_t* o = tmp + (size_t)(r0 + r) * tstride + (c0 + tx) * 3;
      o[0] = clip8(s0);
      o[1] = clip8(s1);
      o[2] = clip8(s2);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void resample_v_kernel(ResampleArgs a) {
  const int rowb = a.OW * 3, tstride = (rowb + 3) & ~3;
  const int b = (blockIdx.x * 256 + threadIdx.x) * 4;           // first of this thread's 4 bytes of the row
  if (b >= rowb) return;
  const ResampleDesc& d = a.desc[blockIdx.z];
  const int oy = blockIdx.y;
  const int* yb = reinterpret_cast<const int*>(d.yb);
  const int mn = clampi(yb[2 * oy], d.row0, d.row0 + d.rows);   // device tables: clamped (see above)
  int n = clampi(yb[2 * oy + 1], 0, d.yksize);
  n = n < d.row0 + d.rows - mn ? n : d.row0 + d.rows - mn;
  const int* k = reinterpret_cast<const int*>(d.yk) + (size_t)oy * d.yksize;
  // tmp, tmp_off and tstride are multiples of 4 (launcher): aligned dword loads
  const uint8_t* p = a.tmp + d.tmp_off + (size_t)(mn - d.row0) * tstride + b;
  uint32_t s[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) s[c] = 1u << (kResampleBits - 1);
  for (int t = 0; t < n; ++t) {
    const uint32_t w = (uint32_t)k[t];
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p + (size_t)t * tstride);
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] += w * ((v >> (8 * c)) & 255u);
  }
  // the batch row of image i starts at i * OH * OW * 3 bytes (odd for 299): byte stores
  uint8_t* o = a.out + ((size_t)d.out_row * a.OH + oy) * rowb + b;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (b + c < rowb) o[c] = clip8(s[c]);
}

bool valid_jpeg_desc(const JpegDesc& d, uint64_t plane_cap) {
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
  if (d.ncomp == 1 && (d.hs != 1 || d.vs != 1)) return false;
  if (d.W < 1 || d.H < 1 || d.W > 65535 || d.H > 65535) return false;
  for (int c = 0; c < d.ncomp; ++c) {
    const int32_t bw = d.bw[c], bh = d.bh[c];
    if (bw < 1 || bh < 1 || bw > 8192 || bh > 8192) return false;
    const int32_t dw = c ? (d.W + d.hs - 1) / d.hs : d.W, dh = c ? (d.H + d.vs - 1) / d.vs : d.H;
    if (d.dw[c] != dw || d.dh[c] != dh || dw > bw * 8 || dh > bh * 8) return false;
    const uint64_t nb = (uint64_t)bw * bh * 64;
    if (d.plane_off[c] > plane_cap || nb > plane_cap - d.plane_off[c]) return false;
  }
  return true;
}

// Every offset the kernels will follow, checked against the capacities of the call: the host
// copies of the descriptors and of the bounds tables. kind: 0 raw, 1 JPEG, -1 the vertical pass
// (sources unused). *cw: the columns per workgroup of the horizontal pass, the most whose source
// span and coefficients fit the LDS budget for every image of the call.
bool valid(const ResampleArgs& a, int kind, int* cw) {
  if (!a.desc || !a.h_desc || !a.tmp || !a.out) return false;
  if (a.n < 1 || a.n > 65535 || a.OH < 1 || a.OW < 1 || a.OH > 65535 || a.OW > 65535 || a.out_rows < 1) return false;
  if (reinterpret_cast<uintptr_t>(a.tmp) % 4) return false;
  if (kind == 1 && (!a.jdesc || !a.h_jdesc || !a.planes || a.n_jdesc < 1)) return false;
  const uint64_t tstride = ((uint64_t)a.OW * 3 + 3) & ~3ull;
  int w = kColsMax;
  for (int i = 0; i < a.n; ++i) {
    const ResampleDesc& d = a.h_desc[i];
    if (d.W < 1 || d.H < 1 || d.W > 65535 || d.H > 65535 || d.xksize < 1 || d.yksize < 1) return false;
    if (!d.xb || !d.xk || !d.yb || !d.yk || !d.h_xb || !d.h_yb) return false;
    if (d.out_row < 0 || d.out_row >= a.out_rows) return false;
    if (d.row0 < 0 || d.rows < 1 || d.rows > d.H - d.row0) return false;
    if (d.tmp_off % 4 || d.tmp_off > a.tmp_cap || (uint64_t)d.rows * tstride > a.tmp_cap - d.tmp_off) return false;
    if (kind == 0 && !d.src) return false;
    if (kind == 1) {
      if (d.src >= (uint64_t)a.n_jdesc) return false;
      const JpegDesc& jd = a.h_jdesc[d.src];
      if (!valid_jpeg_desc(jd, a.plane_cap) || jd.W != d.W || jd.H != d.H) return false;
    }
    const int32_t* yb = reinterpret_cast<const int32_t*>(d.h_yb);
    for (int y = 0; y < a.OH; ++y) {
      const int32_t mn = yb[2 * y], n = yb[2 * y + 1];
      if (mn < d.row0 || n < 0 || n > d.yksize || n > d.row0 + d.rows - mn) return false;
    }
    const int32_t* xb = reinterpret_cast<const int32_t*>(d.h_xb);
    int32_t pmn = 0, pend = 0;
    for (int x = 0; x < a.OW; ++x) {
      const int32_t mn = xb[2 * x], n = xb[2 * x + 1];
      if (mn < 0 || n < 0 || n > d.xksize || mn > d.W || n > d.W - mn) return false;
      // both ends never step back (Pillow's rule): a column group's span is then
      // [bounds[first].min, bounds[last].min + n), which is what the kernel stages
      if (mn < pmn || mn + n < pend) return false;
      pmn = mn;
      pend = mn + n;
    }
    for (;;) {                                                  // shrink until every column group fits
      bool fits = (int64_t)w * d.xksize <= kCoefMax;
      for (int c0 = 0; fits && c0 < a.OW; c0 += w) {
        const int c1 = c0 + w < a.OW ? c0 + w : a.OW;
        fits = xb[2 * (c1 - 1)] + xb[2 * (c1 - 1) + 1] - xb[2 * c0] <= kSpanMax;
      }
      if (fits) break;
      if (w == 1) return false;                                 // one column must fit
      w >>= 1;
    }
  }
  *cw = w;
  return true;
}

}  // namespace

hipError_t resample_h_u8(const ResampleArgs& a, int kind, hipStream_t s) {
  int cw = 0;
  if ((kind != 0 && kind != 1) || !valid(a, kind, &cw)) return hipErrorInvalidValue;
  int rows = 0;
  for (int i = 0; i < a.n; ++i) rows = a.h_desc[i].rows > rows ? a.h_desc[i].rows : rows;
  const dim3 grid((unsigned)((a.OW + cw - 1) / cw), (unsigned)((rows + kBand - 1) / kBand), (unsigned)a.n);
  if (kind == 0)
    hipLaunchKernelGGL(resample_h_kernel<0>, grid, dim3(256), 0, s, a, cw);
  else
    hipLaunchKernelGGL(resample_h_kernel<1>, grid, dim3(256), 0, s, a, cw);
  return hipGetLastError();
}

hipError_t resample_v_u8(const ResampleArgs& a, hipStream_t s) {
  int cw = 0;
  if (!valid(a, -1, &cw)) return hipErrorInvalidValue;
  const int quads = (a.OW * 3 + 3) / 4;
  hipLaunchKernelGGL(resample_v_kernel, dim3((unsigned)((quads + 255) / 256), (unsigned)a.OH, (unsigned)a.n),
                     dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
