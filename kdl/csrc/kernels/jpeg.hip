// Baseline JPEG pixel work on the GPU (the serving_bytes signature, kdl/serving/jpeg.py).
//
// The host has Huffman-decoded each image into quantised coefficient planes (runtime/jpeg.cpp);
// two launches turn a whole request into model inputs:
//   jpeg_idct_u8        coefficients -> uint8 sample planes in device scratch (dequantise + the
//                       libjpeg ISLOW IDCT), every block of every image of the call in one grid
//   jpeg_sample_rgb_u8  one output pixel per thread: the PIL-NEAREST source position from the
//                       resize tables, Y, the 2- or 4-tap fancy chroma upsample evaluated at
//                       that position only, YCbCr -> RGB, store into the request's row of the
//                       [n][OH][OW][3] batch. The full-size RGB image never exists.
// The arithmetic (jpeg_idct_1d, jpeg_descale, jpeg_pixel) is shared with the CPU path through
// runtime/jpeg.h, so the two are identical by construction and both equal Pillow.
#include "common.h"
#include "launch.h"
#include "runtime/jpeg.h"

namespace kdl {

namespace {

// per 8x8 block a 8 x 9 dword tile (row stride 9, block stride 72): with 8 lanes per block, both
// the row-wise and the column-wise dword accesses of a 32-lane group fall on 32 distinct banks
constexpr int kRow = 9, kTile = 72;

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegArgs a) {
  __shared__ uint32_t t[kJpegBlocksPerWg * kTile];
  __shared__ uint16_t q[64];
  const int wg = blockIdx.x;
  int lo = 0, hi = a.n - 1;                 // the image whose workgroup range holds wg
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.desc[mid].wg_start[0] <= wg) lo = mid; else hi = mid - 1;
  }
  const JpegDesc& d = a.desc[lo];
  if (wg < d.wg_start[0] || wg >= d.wg_start[3]) return;     // uniform per workgroup
  int c = 0;
  while (c < 2 && wg >= d.wg_start[c + 1]) ++c;

  const int tid = threadIdx.x, lb = tid >> 3, r = tid & 7;   // block of the workgroup, row / column
  if (tid < 64) q[tid] = a.qt[d.qoff[c] + tid];
  const int bw = d.bw[c];
  const long nblk = (long)bw * d.bh[c];
  const long blk = (long)(wg - d.wg_start[c]) * kJpegBlocksPerWg + lb;
  const bool live = blk < nblk;
  uint4 w = make_uint4(0, 0, 0, 0);                           // one 16-byte coefficient row
  if (live) w = *reinterpret_cast<const uint4*>(a.coef + d.coef_off[c] + blk * 64 + r * 8);
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
  __syncthreads();

  uint32_t* tb = t + lb * kTile;
  uint32_t in[8], o[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int32_t cf = (int16_t)(uint16_t)(ww[k >> 1] >> (16 * (k & 1)));
    tb[r * kRow + k] = (uint32_t)cf * (uint32_t)q[r * 8 + k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) in[k] = tb[k * kRow + r];      // column r
  jpeg_idct_1d(in, o);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) tb[k * kRow + r] = (uint32_t)jpeg_descale(o[k], 11);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 8; ++k) in[k] = tb[r * kRow + k];      // row r
  jpeg_idct_1d(in, o);
  uint32_t px[2] = {0, 0};
#pragma unroll
  for (int k = 0; k < 8; ++k) px[k >> 2] |= (uint32_t)jpeg_clamp(jpeg_descale(o[k], 18) + 128) << (8 * (k & 3));
  if (live) {
    const long by = blk / bw, bx = blk % bw;
    uint8_t* dst = a.planes + d.plane_off[c] + (by * 8 + r) * ((long)bw * 8) + bx * 8;
    *reinterpret_cast<uint2*>(dst) = make_uint2(px[0], px[1]);
  }
}

__global__ __launch_bounds__(256) void jpeg_sample_kernel(JpegArgs a) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;         // OH * OW < 2^31 (checked by the launcher)
  const unsigned plane = (unsigned)a.OH * (unsigned)a.OW;
  if (i >= plane) return;
  const JpegDesc& d = a.desc[blockIdx.y];
  const int oy = (int)(i / (unsigned)a.OW), ox = (int)(i % (unsigned)a.OW);
  int sy = reinterpret_cast<const int*>(d.ytab)[oy], sx = reinterpret_cast<const int*>(d.xtab)[ox];
  sy = sy < 0 ? 0 : sy >= d.H ? d.H - 1 : sy;                 // the tables live in device memory: the host
  sx = sx < 0 ? 0 : sx >= d.W ? d.W - 1 : sx;                 // cannot vouch for their contents
  uint8_t rgb[3];
  jpeg_pixel(d, a.planes, sy, sx, rgb);
  uint8_t* dst = a.out + ((long)d.out_row * plane + i) * 3;   // 64-bit: rows x plane may pass 2^31
  dst[0] = rgb[0];
  dst[1] = rgb[1];
  dst[2] = rgb[2];
}

// every offset the kernels will follow, checked against the capacities of the call
bool valid(const JpegArgs& a) {
  if (!a.desc || !a.h_desc || !a.coef || !a.qt || !a.planes || !a.out) return false;
  if (a.n < 1 || a.n > 65535 || a.OH < 1 || a.OW < 1 || a.out_rows < 1) return false;
  if ((uint64_t)a.OH * (uint64_t)a.OW >= (1ull << 31)) return false;
  if (reinterpret_cast<uintptr_t>(a.coef) % 16 || reinterpret_cast<uintptr_t>(a.planes) % 8) return false;
  int32_t wg = 0;
  for (int i = 0; i < a.n; ++i) {
    const JpegDesc& d = a.h_desc[i];
    if (d.ncomp != 1 && d.ncomp != 3) return false;
    if (!((d.hs == 1 && d.vs == 1) || (d.hs == 2 && d.vs == 1) || (d.hs == 2 && d.vs == 2))) return false;
    if (d.ncomp == 1 && (d.hs != 1 || d.vs != 1)) return false;
    if (d.W < 1 || d.H < 1 || d.W > 65535 || d.H > 65535 || !d.ytab || !d.xtab) return false;
    if (d.out_row < 0 || d.out_row >= a.out_rows) return false;
    for (int c = 0; c < 3; ++c) {
      if (d.wg_start[c] != wg) return false;
      if (c >= d.ncomp) continue;
      const int32_t bw = d.bw[c], bh = d.bh[c];
      if (bw < 1 || bh < 1 || bw > 8192 || bh > 8192) return false;
      const int32_t dw = c ? (d.W + d.hs - 1) / d.hs : d.W, dh = c ? (d.H + d.vs - 1) / d.vs : d.H;
      if (d.dw[c] != dw || d.dh[c] != dh || dw > bw * 8 || dh > bh * 8) return false;
      const uint64_t nc = (uint64_t)bw * bh * 64;
      if (d.coef_off[c] % 8 || d.coef_off[c] > a.coef_cap || nc > a.coef_cap - d.coef_off[c]) return false;
      if (d.plane_off[c] % 8 || d.plane_off[c] > a.plane_cap || nc > a.plane_cap - d.plane_off[c]) return false;
      if (d.qoff[c] < 0 || d.qoff[c] > a.qt_cap - 64) return false;
      wg += (int32_t)((nc / 64 + kJpegBlocksPerWg - 1) / kJpegBlocksPerWg);
    }
    if (d.wg_start[3] != wg) return false;
  }
  return wg == a.n_wg;
}

}  // namespace

hipError_t jpeg_idct_u8(const JpegArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)a.n_wg), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t jpeg_sample_rgb_u8(const JpegArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const long plane = (long)a.OH * a.OW;
  hipLaunchKernelGGL(jpeg_sample_kernel, dim3((unsigned)((plane + 255) / 256), a.n), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
