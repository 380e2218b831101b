// Coefficient tables of Pillow's filtered resize: a port of precompute_coeffs and
// normalize_coeffs_8bpc (libImaging/Resample.c). Every operation is the double-precision one
// Pillow performs, in its order: compile this file without floating-point contraction
// (-ffp-contract=off, see build.py) -- a fused multiply-add can move a coefficient by one unit.
#include "runtime/resample.h"

#include <cmath>

namespace kdl {

namespace {

constexpr double kPi = 3.14159265358979323846;

double box_filter(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

double hamming_filter(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * kPi;
  return std::sin(x) / x * (0.54 + 0.46 * std::cos(x));
}

double bicubic_filter(double x) {
  constexpr double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

double sinc_filter(double x) {
  if (x == 0.0) return 1.0;
  x = x * kPi;
  return std::sin(x) / x;
}

double lanczos_filter(double x) {
  if (-3.0 <= x && x < 3.0) return sinc_filter(x) * sinc_filter(x / 3);
  return 0.0;
}

struct Filter {
  double (*fn)(double);
  double support;
};

const Filter* filter_of(int f) {
  static const Filter k[5] = {{box_filter, 0.5}, {bilinear_filter, 1.0}, {hamming_filter, 1.0},
                              {bicubic_filter, 2.0}, {lanczos_filter, 3.0}};
  return f >= 0 && f < 5 ? &k[f] : nullptr;
}

}  // namespace

int resample_ksize(int in_size, int out_size, int filter) {
  const Filter* fp = filter_of(filter);
  if (!fp || in_size < 1 || out_size < 1) return 0;
  double filterscale = (double)in_size / out_size;
  if (filterscale < 1.0) filterscale = 1.0;
  return (int)std::ceil(fp->support * filterscale) * 2 + 1;
}

int resample_coeffs(int in_size, int out_size, int filter, std::vector<int32_t>* bounds, std::vector<int32_t>* kk) {
  const Filter* fp = filter_of(filter);
  const int ksize = resample_ksize(in_size, out_size, filter);
  if (!fp || ksize < 1) return 0;
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = fp->support * filterscale;
  const double ss = 1.0 / filterscale;
  bounds->assign((size_t)out_size * 2, 0);
  kk->assign((size_t)out_size * ksize, 0);
  std::vector<double> k(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale;
    double ww = 0.0;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    for (int x = 0; x < xmax; ++x) {
      const double w = fp->fn((x + xmin - center + 0.5) * ss);
      k[x] = w;
      ww += w;
    }
    int32_t* o = kk->data() + (size_t)xx * ksize;
    for (int x = 0; x < xmax; ++x) {
      if (ww != 0.0) k[x] /= ww;
      // normalize_coeffs_8bpc: round half away from zero
      o[x] = k[x] < 0 ? (int32_t)(-0.5 + k[x] * (1 << kResampleBits)) : (int32_t)(0.5 + k[x] * (1 << kResampleBits));
    }
    (*bounds)[(size_t)xx * 2] = xmin;
    (*bounds)[(size_t)xx * 2 + 1] = xmax;
  }
  return ksize;
}

}  // namespace kdl
