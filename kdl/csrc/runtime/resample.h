// Pillow's filtered resize (Image.resize with BOX / BILINEAR / HAMMING / BICUBIC / LANCZOS) as
// tables: two separable passes over uint8 with 22-bit fixed-point coefficients and a uint8
// intermediate, so the result can be reproduced bit for bit.
//
// The HOST builds, per axis, the table pair of Pillow's precompute_coeffs + normalize_coeffs_8bpc
// (resample_coeffs); the PIXEL work is a pair of HIP kernels (kernels/resample.hip) that only
// follow the tables. Plain C++17, no HIP: referenced by bindings_rt.cpp (tables, descriptors)
// and by kernels/resample.hip (descriptor + the accumulator arithmetic).
#pragma once
#include <cstdint>
#include <vector>

namespace kdl {

enum ResampleFilter : int { RS_BOX = 0, RS_BILINEAR = 1, RS_HAMMING = 2, RS_BICUBIC = 3, RS_LANCZOS = 4 };

constexpr int kResampleBits = 32 - 8 - 2;   // Pillow's PRECISION_BITS

// taps per output sample: ceil(support * max(in / out, 1)) * 2 + 1; 0 for an unknown filter
int resample_ksize(int in_size, int out_size, int filter);
// bounds [out][2] = {first source sample, taps}, kk [out][ksize] fixed-point weights (0 behind
// the taps). Returns ksize, 0 on bad arguments.
int resample_coeffs(int in_size, int out_size, int filter, std::vector<int32_t>* bounds, std::vector<int32_t>* kk);

// ---------------------------------------------------------------------------------------------
// One image of a GPU resample call (device memory; built and validated on the host). The tables
// are those of the S output columns / rows only: a crop window is a slice of the full tables.
struct ResampleDesc {
  uint64_t src;            // raw kind: device address of the packed [H][W][3] image;
                           // JPEG kind: index of the image's JpegDesc in the call's array
  uint64_t xb, xk;         // device tables of the OW columns: bounds int32 [OW][2], kk int32 [OW][xksize]
  uint64_t yb, yk;         // the same of the OH rows
  uint64_t h_xb, h_yb;     // HOST copies of the bounds (the launchers check them; never followed on the device)
  uint64_t tmp_off;        // bytes from the call's intermediate scratch: [rows][align4(OW * 3)]
  int32_t W, H;            // source size
  int32_t xksize, yksize;
  int32_t row0, rows;      // the source rows the vertical pass reads: yb[0].min .. yb[OH-1].min + n
  int32_t out_row;         // the image's row of the [out_rows][OH][OW][3] output
  int32_t pad_;
};
static_assert(sizeof(ResampleDesc) == 96, "ResampleDesc is copied as raw bytes");

}  // namespace kdl
