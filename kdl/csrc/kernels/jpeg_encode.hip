// Baseline JPEG encode of uint8 RGB pictures, byte for byte the file Pillow (libjpeg-turbo) writes
// (launch.h JpegEncodeArgs; kdl/serving/jpeg_encode.py encode_rule is the definition).
//
// Four launches, all integer arithmetic:
//   1. coef   one workgroup per (MCU row, picture). It converts the band's pixels to Y / Cb / Cr byte
//             planes in LDS (coalesced byte reads of the picture, edge replication by clamping the
//             source coordinates, the h2v2 average with its alternating bias), then a thread per 8 x 8
//             block runs libjpeg's islow DCT from LDS, quantises, stores the 64 int16 coefficients in
//             zig-zag order at the block's place in the scan, and the bits its AC part will take.
//   2. scan   one workgroup per picture: adds every block's DC bits (the difference to the component's
//             previous block, dummies resolved), prefix-sums the lengths in scan order into bit offsets,
//             decides the early overflow and clears the words of the picture's bit stream.
//   3. bits   a thread per block Huffman-codes its coefficients and ORs whole words into the stream
//             (atomicOr: two blocks share a word only at their ends; OR commutes, so every launch gives
//             the same words).
//   4. file   one workgroup per picture counts the 0xFF bytes per chunk, prefix-sums them, and writes the
//             front words, the length, the header, the stuffed scan, EOI and the zero bytes up to the cap.
// A dummy block (a Y block of a 4:2:0 MCU outside the component's block grid) has zero coefficients
// in step 1; its DC is resolved where differences are formed (dc_value).
// Bounds: the picture is read at clamped coordinates only; coef / len are indexed by scan positions
// < nblk; the stream is written below ceil(nbytes / 4) + 1 words, which the early overflow test keeps
// under the ceil(cap / 4) + 2 words each picture owns; the row is written below nfront + 1 + ceil(cap / 4).
#include <cstring>

#include "common.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kMaxMcuX = kJpegEncMaxSide / 8;                    // MCUs (4:4:4) per row at most
constexpr int kScanThreads = 1024;

constexpr uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
constexpr uint8_t kQuantBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61,  12, 12, 14, 19, 26, 58, 60, 55,  14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62,  18, 22, 37, 56, 68, 109, 103, 77,  24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101,  72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99,  18, 21, 26, 66, 99, 99, 99, 99,  24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99,  99, 99, 99, 99, 99, 99, 99, 99}};
// Annex K Huffman tables: code counts per length 1..16, then the symbols
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                    {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
     0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
     0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
     0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
     0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
     0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
     0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
     0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
     0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
     0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
     0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
     0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
     0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

// code << 8 | length per symbol (0: the symbol has no code), [0 luminance / 1 chrominance]
struct EncTabs {
  uint32_t ac[2][256];
  uint32_t dc[2][16];
};
constexpr EncTabs make_tabs() {
  EncTabs t{};
  for (int c = 0; c < 2; ++c) {
    uint32_t code = 0;
    int k = 0;
    for (int n = 1; n <= 16; ++n) {
      for (int i = 0; i < kDcBits[c][n - 1]; ++i) t.dc[c][k++] = (code++ << 8) | (uint32_t)n;   // symbols 0..11 in order
      code <<= 1;
    }
    code = 0;
    k = 0;
    for (int n = 1; n <= 16; ++n) {
      for (int i = 0; i < kAcBits[c][n - 1]; ++i) t.ac[c][kAcVals[c][k++]] = (code++ << 8) | (uint32_t)n;
      code <<= 1;
    }
  }
  return t;
}
__constant__ EncTabs c_tabs = make_tabs();

// the scan's geometry, from H, W and the sampling alone
struct Geo {
  int hs;          // Y blocks per MCU side: 1 (4:4:4) or 2 (4:2:0)
  int mcux, mcuy;  // MCUs per row / column
  int bpm;         // blocks per MCU: hs * hs + 2
  int nblk;        // blocks in the scan
  int gx, gy;      // the Y component's own block grid, ceil(W / 8) x ceil(H / 8)
};
__host__ __device__ inline Geo geo_of(int H, int W, int sampling) {
  Geo g;
  g.hs = sampling ? 2 : 1;
  g.mcux = (W + 8 * g.hs - 1) / (8 * g.hs);
  g.mcuy = (H + 8 * g.hs - 1) / (8 * g.hs);
  g.bpm = g.hs * g.hs + 2;
  g.nblk = g.mcux * g.mcuy * g.bpm;
  g.gx = (W + 7) / 8;
  g.gy = (H + 7) / 8;
  return g;
}

// the workspace of a call: [coef int16 B x nblk x 64][len uint32 B x nblk][meta uint32 B x 4][stream B x sw words]
struct Work {
  size_t len, meta, stream, bytes;
  int sw;          // stream words a picture owns
};
__host__ __device__ inline Work work_of(int B, int nblk, int cap) {
  Work w;
  w.sw = (((cap + 3) / 4 + 2) + 3) & ~3;
  w.len = (size_t)B * nblk * 128;
  w.meta = w.len + (((size_t)B * nblk * 4 + 15) & ~(size_t)15);
  w.stream = w.meta + (size_t)B * 16;
  w.bytes = w.stream + (size_t)B * w.sw * 4;
  return w;
}

__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }

// ------------------------------------------------------------------------------------------ 1. coef
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg jfdctint.c, one pass over d[0], d[ST], .. d[7 * ST]
template <int ST, bool FIRST>
__device__ __forceinline__ void dct_pass(int* d) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7 * ST], t7 = d[0] - d[7 * ST], t1 = d[ST] + d[6 * ST], t6 = d[ST] - d[6 * ST];
  const int t2 = d[2 * ST] + d[5 * ST], t5 = d[2 * ST] - d[5 * ST], t3 = d[3 * ST] + d[4 * ST], t4 = d[3 * ST] - d[4 * ST];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4 * ST] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * ST] = descale(z1 + t13 * 6270, N);
  d[6 * ST] = descale(z1 - t12 * 15137, N);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  d[7 * ST] = descale(u4 + z1 + z3, N);
  d[5 * ST] = descale(u5 + z2 + z4, N);
  d[3 * ST] = descale(u6 + z2 + z3, N);
  d[ST] = descale(u7 + z1 + z4, N);
}

__device__ __forceinline__ void ycc(const uint8_t* p, int& y, int& cb, int& cr) {
  const int r = p[0], g = p[1], b = p[2];
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

__global__ __launch_bounds__(256) void jpeg_enc_coef_kernel(JpegEncodeArgs a) {
  __shared__ __align__(16) uint8_t ypl[16 * kMaxMcuX * 8];       // 4:2:0: 16 rows of mcux * 16; 4:4:4: 8 rows of mcux * 8
  __shared__ __align__(16) uint8_t cpl[2][8 * kMaxMcuX * 8];     // Cb, Cr: 8 rows of mcux * 8
  __shared__ uint16_t q8[2][64];                                 // 8 * the table entry, zig-zag order
  __shared__ uint8_t aclen[2][256];
  const int tid = threadIdx.x, my = blockIdx.x, b = blockIdx.y;
  const Geo g = geo_of(a.H, a.W, a.sampling);
  const int H = a.H, W = a.W, hs = g.hs;
  const int ys = g.mcux * 8 * hs, cs = g.mcux * 8, yrows = 8 * hs;
  const uint8_t* pic = a.inp + (size_t)b * a.ldi;

  if (tid < 128) q8[tid >> 6][tid & 63] = (uint16_t)(8 * a.hdr[(tid < 64 ? 25 : 94 - 64) + tid]);
  aclen[0][tid] = (uint8_t)(c_tabs.ac[0][tid] & 255u);
  aclen[1][tid] = (uint8_t)(c_tabs.ac[1][tid] & 255u);

  for (int i = tid; i < yrows * ys; i += 256) {                  // the Y plane (4:4:4: the chroma planes too)
    const int ry = i / ys, x = i - ry * ys;
    const int sy = mini(my * yrows + ry, H - 1), sx = mini(x, W - 1);
    int y, cb, cr;
    ycc(pic + ((size_t)sy * W + sx) * 3, y, cb, cr);
    ypl[i] = (uint8_t)y;
    if (hs == 1) {
      cpl[0][i] = (uint8_t)cb;
      cpl[1][i] = (uint8_t)cr;
    }
  }
  if (hs == 2) {
    // h2v2: the last row replicated only to an even height, the last column as far as needed, the
    // average, and below the last downsampled row that row again
    const int h2 = (H + 1) / 2;
    for (int i = tid; i < 8 * cs; i += 256) {
      const int cy = i / cs, cx = i - cy * cs;
      const int cyg = mini(my * 8 + cy, h2 - 1);
      const int r0 = mini(2 * cyg, H - 1), r1 = mini(2 * cyg + 1, H - 1);
      const int c0 = mini(2 * cx, W - 1), c1 = mini(2 * cx + 1, W - 1);
      int y, cb, cr, sb = 1 + (cx & 1), sr = sb;
      ycc(pic + ((size_t)r0 * W + c0) * 3, y, cb, cr); sb += cb; sr += cr;
      ycc(pic + ((size_t)r0 * W + c1) * 3, y, cb, cr); sb += cb; sr += cr;
      ycc(pic + ((size_t)r1 * W + c0) * 3, y, cb, cr); sb += cb; sr += cr;
      ycc(pic + ((size_t)r1 * W + c1) * 3, y, cb, cr); sb += cb; sr += cr;
      cpl[0][i] = (uint8_t)(sb >> 2);
      cpl[1][i] = (uint8_t)(sr >> 2);
    }
  }
  __syncthreads();

  const Work wk = work_of(a.B, g.nblk, a.cap);
  int16_t* coef = reinterpret_cast<int16_t*>(a.work) + (size_t)b * g.nblk * 64;
  uint32_t* len = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(a.work) + wk.len) + (size_t)b * g.nblk;
  const int ny = hs * hs;
  for (int t = tid; t < g.mcux * g.bpm; t += 256) {              // block i of MCU mx: neighbours in a wave share a plane
    const int i = t / g.mcux, mx = t - i * g.mcux;
    const int tab = i >= ny;
    const uint8_t* src;
    int stride;
    bool dummy = false;
    if (!tab) {
      const int by = i / hs, bx = mx * hs + (i - by * hs);
      src = ypl + by * 8 * ys + bx * 8;
      stride = ys;
      dummy = my * hs + by >= g.gy || bx >= g.gx;
    } else {
      src = cpl[i - ny] + mx * 8;
      stride = cs;
    }
    int d[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const uint2 v = *reinterpret_cast<const uint2*>(src + r * stride);   // 8-byte aligned: strides and offsets are multiples of 8
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int s = (int)(((c < 4 ? v.x : v.y) >> (8 * (c & 3))) & 255u) - 128;
        d[r * 8 + c] = dummy ? 0 : s;
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) dct_pass<1, true>(d + 8 * r);
#pragma unroll
    for (int c = 0; c < 8; ++c) dct_pass<8, false>(d + c);

    uint32_t packed[32];
    uint32_t bits = 0;
    int run = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const int c = d[kZigzag[k]];
      const uint32_t q = q8[tab][k];
      const uint32_t m = ((uint32_t)(c < 0 ? -c : c) + (q >> 1)) / q;
      const int v = c < 0 ? -(int)m : (int)m;
      if (k & 1) packed[k >> 1] |= (uint32_t)(uint16_t)v << 16;
      else packed[k >> 1] = (uint32_t)(uint16_t)v;
      if (k > 0) {
        if (m == 0) {
          ++run;
        } else {
          const int nb = 32 - __builtin_clz(m);
          bits += (uint32_t)(run >> 4) * aclen[tab][0xF0] + aclen[tab][(((run & 15) << 4) | nb) & 255] + (uint32_t)nb;
          run = 0;
        }
      }
    }
    if (run) bits += aclen[tab][0];
    const int j = (my * g.mcux + mx) * g.bpm + i;                // < nblk
    uint4* dst = reinterpret_cast<uint4*>(coef + (size_t)j * 64);
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = make_uint4(packed[4 * k], packed[4 * k + 1], packed[4 * k + 2], packed[4 * k + 3]);
    len[j] = bits;
  }
}

// ------------------------------------------------------------------------------------------ DC differences
// the DC of block i of MCU m as the scan sends it: a dummy has the DC of the block before it (block 0 of
// an MCU is never a dummy)
__device__ __forceinline__ int dc_value(const int16_t* coef, const Geo& g, int m, int i) {
  if (i < g.hs * g.hs) {
    const int my = m / g.mcux, mx = m - my * g.mcux;
    while (i > 0 && (my * g.hs + i / g.hs >= g.gy || mx * g.hs + i % g.hs >= g.gx)) --i;
  }
  return coef[((size_t)m * g.bpm + i) * 64];
}

// DC of scan block j minus its component's previous DC (0 at the start of the scan)
__device__ __forceinline__ int dc_diff(const int16_t* coef, const Geo& g, int j) {
  const int m = j / g.bpm, i = j - m * g.bpm, ny = g.hs * g.hs;
  int prev = 0;
  if (i < ny && i > 0) prev = dc_value(coef, g, m, i - 1);
  else if (m > 0) prev = dc_value(coef, g, m - 1, i < ny ? ny - 1 : i);
  return dc_value(coef, g, m, i) - prev;
}

__device__ __forceinline__ int magnitude_bits(int v) {
  const uint32_t m = (uint32_t)(v < 0 ? -v : v);
  return m ? mini(32 - __builtin_clz(m), 15) : 0;              // an encoder's values have at most 11: 15 keeps every table index inside
}

// ------------------------------------------------------------------------------------------ 2. scan
__global__ __launch_bounds__(kScanThreads) void jpeg_enc_scan_kernel(JpegEncodeArgs a) {
  __shared__ uint32_t part[kScanThreads];
  const int tid = threadIdx.x, b = blockIdx.x;
  const Geo g = geo_of(a.H, a.W, a.sampling);
  const Work wk = work_of(a.B, g.nblk, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  const int16_t* coef = reinterpret_cast<const int16_t*>(base) + (size_t)b * g.nblk * 64;
  uint32_t* len = reinterpret_cast<uint32_t*>(base + wk.len) + (size_t)b * g.nblk;
  uint32_t* meta = reinterpret_cast<uint32_t*>(base + wk.meta) + (size_t)b * 4;
  uint32_t* stream = reinterpret_cast<uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;

  const int per = (g.nblk + kScanThreads - 1) / kScanThreads;
  const int j0 = mini(tid * per, g.nblk), j1 = mini(j0 + per, g.nblk);
  uint32_t sum = 0;
  for (int j = j0; j < j1; ++j) {
    const int nb = magnitude_bits(dc_diff(coef, g, j));          // <= 11: a table entry exists
    const uint32_t l = len[j] + (c_tabs.dc[(j % g.bpm) >= g.hs * g.hs][nb] & 255u) + (uint32_t)nb;
    len[j] = l;
    sum += l;
  }
  part[tid] = sum;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {             // inclusive scan
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  uint32_t at = part[tid] - sum;
  for (int j = j0; j < j1; ++j) {
    const uint32_t l = len[j];
    len[j] = at;                                                 // the block's first bit
    at += l;
  }
  const uint32_t total = part[kScanThreads - 1];                 // < 2^32: at most 49152 blocks of 64 * 27 bits
  const uint32_t nbytes = (total + 7) / 8;
  const bool over = (uint64_t)kJpegHeaderBytes + nbytes + 2 > (uint64_t)a.cap;
  if (tid == 0) {
    meta[0] = total;
    meta[1] = over;
  }
  if (!over)                                                     // nbytes <= cap - 625: (nbytes + 3) / 4 + 1 <= sw
    for (uint32_t i = tid; i < (nbytes + 3) / 4 + 1; i += kScanThreads) stream[i] = 0u;
}

// ------------------------------------------------------------------------------------------ 3. bits
struct BitWriter {
  uint32_t* w;       // the next word of the stream
  uint32_t* end;     // behind the words the picture owns: nothing is written there, whatever the lengths said
  uint64_t acc;      // the low `n` bits are pending
  int n;             // < 32 between calls
  __device__ __forceinline__ void put(uint32_t code, int len) {  // len <= 27
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      if (w < end) atomicOr(w, (uint32_t)(acc >> n));
      ++w;
      acc &= (1ull << n) - 1;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n && w < end) atomicOr(w, (uint32_t)(acc << (32 - n)));
  }
};

__global__ __launch_bounds__(256) void jpeg_enc_bits_kernel(JpegEncodeArgs a) {
  __shared__ uint32_t ac[2][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const Geo g = geo_of(a.H, a.W, a.sampling);
  const Work wk = work_of(a.B, g.nblk, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  const int16_t* coef = reinterpret_cast<const int16_t*>(base) + (size_t)b * g.nblk * 64;
  const uint32_t* len = reinterpret_cast<const uint32_t*>(base + wk.len) + (size_t)b * g.nblk;
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(base + wk.meta) + (size_t)b * 4;
  uint32_t* stream = reinterpret_cast<uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;
  if (meta[1]) return;                                           // the whole workgroup: the picture overflowed
  ac[0][tid] = c_tabs.ac[0][tid];
  ac[1][tid] = c_tabs.ac[1][tid];
  __syncthreads();
  const int j = blockIdx.x * 256 + tid;
  if (j >= g.nblk) return;
  const int tab = (j % g.bpm) >= g.hs * g.hs;
  const uint32_t at = len[j];
  BitWriter bw{stream + (at >> 5), stream + wk.sw, 0ull, (int)(at & 31u)};       // the bits in front of `at` are another block's: 0 here

  const int diff = dc_diff(coef, g, j);
  int nb = magnitude_bits(diff);
  uint32_t e = c_tabs.dc[tab][nb];
  bw.put(((e >> 8) << nb) | ((uint32_t)(diff - (diff < 0)) & ((1u << nb) - 1u)), (int)(e & 255u) + nb);
  const uint4* src = reinterpret_cast<const uint4*>(coef + (size_t)j * 64);
  int run = 0;
  for (int c = 0; c < 8; ++c) {
    const uint4 q = src[c];
    const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (c == 0 && k == 0) continue;
      const int v = (int)(int16_t)(wd[k >> 1] >> (16 * (k & 1)));
      if (v == 0) {
        ++run;
        continue;
      }
      for (; run >= 16; run -= 16) bw.put(ac[tab][0xF0] >> 8, (int)(ac[tab][0xF0] & 255u));
      nb = magnitude_bits(v);
      e = ac[tab][(run << 4) | nb];
      bw.put(((e >> 8) << nb) | ((uint32_t)(v - (v < 0)) & ((1u << nb) - 1u)), (int)(e & 255u) + nb);
      run = 0;
    }
  }
  if (run) bw.put(ac[tab][0] >> 8, (int)(ac[tab][0] & 255u));
  bw.flush();
}

// ------------------------------------------------------------------------------------------ 4. file
__global__ __launch_bounds__(kScanThreads) void jpeg_enc_file_kernel(JpegEncodeArgs a) {
  __shared__ uint32_t part[kScanThreads];
  const int tid = threadIdx.x, b = blockIdx.x;
  const Geo g = geo_of(a.H, a.W, a.sampling);
  const Work wk = work_of(a.B, g.nblk, a.cap);
  const uint8_t* base = reinterpret_cast<const uint8_t*>(a.work);
  const uint32_t* meta = reinterpret_cast<const uint32_t*>(base + wk.meta) + (size_t)b * 4;
  const uint32_t* stream = reinterpret_cast<const uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;
  uint32_t* row = a.out + (size_t)b * a.ldo;
  for (int i = tid; i < a.nfront; i += kScanThreads) row[i] = a.front[(size_t)b * a.ldf + i];
  if (meta[1]) {
    if (tid == 0) row[a.nfront] = 0u;
    return;
  }
  const uint32_t total = meta[0], nbytes = (total + 7) / 8;
  const uint32_t fill = (total & 7u) ? (1u << (8 - (total & 7u))) - 1u : 0u;   // 1 bits behind the last code
  const uint32_t chunk = 4 * (((nbytes + 3) / 4 + kScanThreads - 1) / kScanThreads);
  const uint32_t k0 = tid * chunk < nbytes ? tid * chunk : nbytes;
  const uint32_t k1 = k0 + chunk < nbytes ? k0 + chunk : nbytes;
  auto byte_at = [&](uint32_t k) {                               // k < nbytes: word k / 4 <= (nbytes - 1) / 4 was cleared
    const uint32_t v = (stream[k >> 2] >> (24 - 8 * (k & 3u))) & 255u;
    return k + 1 == nbytes ? v | fill : v;
  };
  uint32_t nff = 0;
  for (uint32_t k = k0; k < k1; ++k) nff += byte_at(k) == 255u;
  part[tid] = nff;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const uint64_t flen = (uint64_t)kJpegHeaderBytes + nbytes + part[kScanThreads - 1] + 2;
  if (flen > (uint64_t)a.cap) {                                  // the whole workgroup: nothing of the file was written yet
    if (tid == 0) row[a.nfront] = 0u;
    return;
  }
  uint8_t* file = reinterpret_cast<uint8_t*>(row + a.nfront + 1);
  uint32_t pos = kJpegHeaderBytes + k0 + (part[tid] - nff);      // every byte below goes in front of flen - 2 <= cap - 2
  for (uint32_t k = k0; k < k1; ++k) {
    const uint32_t v = byte_at(k);
    file[pos++] = (uint8_t)v;
    if (v == 255u) file[pos++] = 0;
  }
  for (int i = tid; i < kJpegHeaderBytes; i += kScanThreads) file[i] = a.hdr[i];
  const uint32_t n = (uint32_t)flen, capw = ((uint32_t)a.cap + 3) / 4;
  if (tid == 0) {
    file[n - 2] = 0xFF;
    file[n - 1] = 0xD9;
    row[a.nfront] = n;
  }
  const uint32_t w0 = (n + 3) / 4;                               // zero bytes up to the end of word capw - 1
  if (tid < (int)(4 * w0 - n)) file[n + tid] = 0;
  for (uint32_t i = w0 + tid; i < capw; i += kScanThreads) row[a.nfront + 1 + i] = 0u;
}

// ------------------------------------------------------------------------------------------ host
// the header of these arguments (kdl/serving/jpeg_encode.py header)
void build_header(const JpegEncodeArgs& a, uint8_t* h) {
  static const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  memcpy(h, app0, 20);
  int n = 20;
  const int s = a.quality < 50 ? 5000 / a.quality : 200 - 2 * a.quality;
  for (int t = 0; t < 2; ++t) {
    const uint8_t m[5] = {0xFF, 0xDB, 0, 67, (uint8_t)t};
    memcpy(h + n, m, 5);
    n += 5;
    for (int k = 0; k < 64; ++k) {
      const int v = (kQuantBase[t][kZigzag[k]] * s + 50) / 100;
      h[n++] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
  }
  const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, (uint8_t)(a.H >> 8), (uint8_t)a.H, (uint8_t)(a.W >> 8), (uint8_t)a.W, 3,
                           1, (uint8_t)(a.sampling ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
  memcpy(h + n, sof, 19);
  n += 19;
  for (int t = 0; t < 4; ++t) {                                  // DC0, AC0, DC1, AC1
    const int ac = t & 1, c = t >> 1, nv = ac ? 162 : 12;
    const uint8_t m[5] = {0xFF, 0xC4, 0, (uint8_t)(19 + nv), (uint8_t)(ac << 4 | c)};
    memcpy(h + n, m, 5);
    n += 5;
    memcpy(h + n, ac ? kAcBits[c] : kDcBits[c], 16);
    n += 16;
    for (int k = 0; k < nv; ++k) h[n++] = ac ? kAcVals[c][k] : (uint8_t)k;
  }
  static const uint8_t sos[14] = {0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  memcpy(h + n, sos, 14);
  static_assert(20 + 2 * 69 + 19 + 2 * (21 + 12) + 2 * (21 + 162) + 14 == kJpegHeaderBytes, "header size");
}

bool valid(const JpegEncodeArgs& a) {
  if (!a.inp || !a.hdr || !a.h_hdr || !a.out || !a.work) return false;
  if (reinterpret_cast<uintptr_t>(a.out) % 4 || reinterpret_cast<uintptr_t>(a.work) % 16) return false;
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.H > kJpegEncMaxSide || a.W < 1 || a.W > kJpegEncMaxSide) return false;
  if (a.quality < 1 || a.quality > 100 || (a.sampling != 0 && a.sampling != 1)) return false;
  if (a.cap < 1 || a.cap > kJpegEncMaxCap || a.ldi < (int64_t)a.H * a.W * 3) return false;
  if (a.nfront < 0 || a.ldf < a.nfront) return false;
  if (a.nfront > 0 && (!a.front || reinterpret_cast<uintptr_t>(a.front) % 4)) return false;
  if ((int64_t)a.ldo < (int64_t)a.nfront + 1 + (a.cap + 3) / 4) return false;
  uint8_t h[kJpegHeaderBytes];
  build_header(a, h);
  return memcmp(h, a.h_hdr, kJpegHeaderBytes) == 0;
}

}  // namespace

size_t jpeg_encode_workspace(int B, int H, int W, int sampling, int cap) {
  if (B < 1 || B > 65535 || H < 1 || H > kJpegEncMaxSide || W < 1 || W > kJpegEncMaxSide || cap < 1 ||
      cap > kJpegEncMaxCap || (sampling != 0 && sampling != 1))
    return 0;
  return work_of(B, geo_of(H, W, sampling).nblk, cap).bytes;
}

hipError_t jpeg_encode(const JpegEncodeArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const Geo g = geo_of(a.H, a.W, a.sampling);
  hipLaunchKernelGGL(jpeg_enc_coef_kernel, dim3((unsigned)g.mcuy, (unsigned)a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_enc_scan_kernel, dim3((unsigned)a.B), dim3(kScanThreads), 0, s, a);
  hipLaunchKernelGGL(jpeg_enc_bits_kernel, dim3((unsigned)((g.nblk + 255) / 256), (unsigned)a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(jpeg_enc_file_kernel, dim3((unsigned)a.B), dim3(kScanThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
