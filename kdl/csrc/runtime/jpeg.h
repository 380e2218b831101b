// Baseline JPEG for the ``serving_bytes`` signature (kdl/serving/jpeg.py).
//
// The HOST does the serial part: jpeg_parse() walks the markers and Huffman-decodes the scan
// into quantised coefficients (int16, 64 per block, natural order, one plane per component
// over its padded block grid -- no MCU interleave). The PIXEL work -- dequantise, IDCT, chroma
// upsample, YCbCr -> RGB, the PIL-NEAREST resize gather -- is a pair of HIP kernels
// (kernels/jpeg.hip); jpeg_pixels_cpu() is the same arithmetic for servers without a GPU and
// for the tests. The arithmetic is libjpeg-turbo's default decode (JDCT_ISLOW, fancy
// upsampling), which is what Pillow produces, and lives in this header ONCE (jpeg_idct_1d,
// jpeg_descale, jpeg_pixel) so that the CPU and the GPU path cannot drift apart.
// The entropy decode has an opt-in device path as well: runtime/jpeg_huff.h, kernels/jpeg_huff.hip.
//
// Self-contained on purpose: plain C++17, no HIP, no libjpeg, referenced only by
// bindings_rt.cpp (host) and kernels/jpeg.hip + bindings_gpu.cpp (descriptor + arithmetic).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define KDL_JPEG_HD __host__ __device__ inline
#else
#define KDL_JPEG_HD inline
#endif

namespace kdl {

enum JpegStatus : int {
  JPEG_OK = 0,
  JPEG_UNSUPPORTED = 1,   // well formed, not covered here (progressive, CMYK, a PNG, ...): use PIL
  JPEG_MALFORMED = 2,     // a baseline file that breaks a rule: reject the request
};

struct JpegComp {
  int id, h, v, tq;       // component id, sampling factors, quantisation table
  int bw, bh;             // padded block grid (whole MCUs)
  int dw, dh;             // real samples: ceil(W*h/hmax) x ceil(H*v/vmax)
  uint64_t coef_off;      // first coefficient of the plane, in int16 units
};

struct JpegHeader {
  int W = 0, H = 0, ncomp = 0, hmax = 1, vmax = 1;
  JpegComp comp[3] = {};
  uint16_t qt[4][64] = {};       // natural order
  uint64_t ncoef = 0;            // coefficients of all planes == bytes of all sample planes
  int restart = 0;
  const char* why = "";          // what made the status not ok
};

// Marker walk up to the frame header: geometry only (W, H, sampling, grids, ncoef). The caller
// sizes its buffers from it -- after checking W*H against its pixel limit.
JpegStatus jpeg_probe(const uint8_t* data, size_t n, uint64_t max_pixels, JpegHeader* h);
// Full parse + entropy decode into ``coef`` (capacity ``cap`` int16; needs h->ncoef).
JpegStatus jpeg_parse(const uint8_t* data, size_t n, uint64_t max_pixels, int16_t* coef, uint64_t cap,
                      JpegHeader* h);
// coefficients -> RGB [H][W][3]
void jpeg_pixels_cpu(const JpegHeader& h, const int16_t* coef, uint8_t* rgb);

// ---------------------------------------------------------------------------------------------
// One image of a GPU decode call (device memory; built and validated on the host).
struct JpegDesc {
  uint64_t coef_off[3];    // int16 units from the call's coefficient base
  uint64_t plane_off[3];   // bytes from the call's sample-plane scratch
  uint64_t ytab, xtab;     // device addresses of the PIL-NEAREST tables: int32 [OH], [OW]
  int32_t bw[3], bh[3], dw[3], dh[3];
  int32_t qoff[3];         // uint16 units from the call's quantisation-table base
  int32_t wg_start[4];     // first IDCT workgroup of each component; [ncomp..3] = one past the last
  int32_t ncomp, hs, vs;   // hs x vs: luma sampling (1x1, 2x1, 2x2); chroma is 1x1
  int32_t W, H, out_row;   // out_row: the image's row of the [n][OH][OW][3] output
};
static_assert(sizeof(JpegDesc) % 8 == 0, "JpegDesc is copied as raw bytes");

constexpr int kJpegBlocksPerWg = 32;   // 256 threads, 8 lanes per 8x8 block

void jpeg_fill_desc(const JpegHeader& h, uint64_t coef_base, uint64_t plane_base, int32_t qt_base, int32_t* wg,
                    int32_t out_row, uint64_t ytab, uint64_t xtab, JpegDesc* d);

// ---------------------------------------------------------------------------------------------
// Shared arithmetic: 32-bit two's-complement wraparound (unsigned ops), >> arithmetic.

KDL_JPEG_HD int32_t jpeg_descale(uint32_t x, int s) { return (int32_t)(x + (1u << (s - 1))) >> s; }

// libjpeg's jidctint 1-D pass (13-bit constants), no descale
KDL_JPEG_HD void jpeg_idct_1d(const uint32_t* in, uint32_t* out) {
  uint32_t z1 = (in[2] + in[6]) * 4433u;
  const uint32_t t2 = z1 - in[6] * 15137u;
  const uint32_t t3 = z1 + in[2] * 6270u;
  const uint32_t t0 = (in[0] + in[4]) << 13;
  const uint32_t t1 = (in[0] - in[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  uint32_t a0 = in[7], a1 = in[5], a2 = in[3], a3 = in[1];
  z1 = a0 + a3;
  uint32_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  a0 *= 2446u; a1 *= 16819u; a2 *= 25172u; a3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
  out[0] = t10 + a3; out[7] = t10 - a3;
  out[1] = t11 + a2; out[6] = t11 - a2;
  out[2] = t12 + a1; out[5] = t12 - a1;
  out[3] = t13 + a0; out[4] = t13 - a0;
}

KDL_JPEG_HD uint8_t jpeg_clamp(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

// one chroma sample at full-resolution (y, x): libjpeg's fancy (triangle) upsampling evaluated
// at a single position; neighbours are clamped to the component's real samples. libjpeg takes
// the fancy upsamplers only for planes more than 2 samples wide (downsampled_width > 2) and
// replicates otherwise, vertically too: images up to 4 pixels wide
KDL_JPEG_HD int32_t jpeg_chroma(const uint8_t* p, int stride, int dw, int dh, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(size_t)y * stride + x];
  const int i = x >> 1;
  if (dw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + i];
  const int i2 = (x & 1) ? (i + 1 < dw ? i + 1 : dw - 1) : (i > 0 ? i - 1 : 0);
  if (vs == 1) {
    const uint8_t* r = p + (size_t)y * stride;
    return (3 * r[i] + r[i2] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int j = y >> 1;
  const int j2 = (y & 1) ? (j + 1 < dh ? j + 1 : dh - 1) : (j > 0 ? j - 1 : 0);
  const uint8_t* r = p + (size_t)j * stride;
  const uint8_t* r2 = p + (size_t)j2 * stride;
  const int32_t v = 3 * r[i] + r2[i], v2 = 3 * r[i2] + r2[i2];
  return (3 * v + v2 + ((x & 1) ? 7 : 8)) >> 4;
}

// RGB of source pixel (y, x) from the sample planes of image ``d``
KDL_JPEG_HD void jpeg_pixel(const JpegDesc& d, const uint8_t* planes, int y, int x, uint8_t* rgb) {
  const int32_t Y = planes[d.plane_off[0] + (size_t)y * (d.bw[0] * 8) + x];
  if (d.ncomp == 1) {
    rgb[0] = rgb[1] = rgb[2] = (uint8_t)Y;
    return;
  }
  const int32_t cb = jpeg_chroma(planes + d.plane_off[1], d.bw[1] * 8, d.dw[1], d.dh[1], d.hs, d.vs, y, x) - 128;
  const int32_t cr = jpeg_chroma(planes + d.plane_off[2], d.bw[2] * 8, d.dw[2], d.dh[2], d.hs, d.vs, y, x) - 128;
  rgb[0] = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16));
  rgb[1] = jpeg_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  rgb[2] = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
}

}  // namespace kdl
