// ConvNeXt's block head and downsample input (Liu et al. 2022), NHWC bf16, fp32 arithmetic:
//
//   dwconv7_ln  depthwise 7x7 ('same', stride 1) + bias, then LayerNorm over the channels of every
//               pixel, in one launch: the conv output d never reaches memory.
//   ln_s2d      LayerNorm over the channels of every pixel, written space-to-depth so that the
//               2x2 / stride-2 conv behind it is one pointwise GEMM with K = 4 C.
//
// dwconv7_ln. The statistics need every channel of a pixel, so a workgroup owns one image x a band
// of R output rows x a strip of TW output columns x ALL channels:
//
//   * input rows live in an LDS ring of up to 8 row slots (7 live + the one in flight), each
//     LW = TW' + 6 pixels of C channels (pixel stride 2 C + 16 bytes), TW' = TW rounded up to whole
//     pixel groups. A row is fetched once per band with 16-byte loads: while output row oy is
//     computed, input row oy + 4 is in flight in registers and lands in the slot of row oy - 4.
//     Columns outside the map are stored as zeros when the row lands, rows outside the map are
//     skipped by a workgroup-uniform predicate: no tap is bounds-checked.
//   * conv: an item is (a group of PW = 7 or 4 consecutive pixels, an 8-channel chunk); chunks run
//     fastest over the lanes, so a wave reads consecutive 16-byte pieces of the ring. Per kernel
//     row the item loads the row's 7 x 8 weights and walks PW + 6 ring pixels once, each feeding up
//     to 7 of its PW x 8 fp32 accumulators (fmaf chains the compiler pairs into packed FMAs): 13
//     LDS reads per 392 FMAs at PW = 7. W * C is 5376 at every ConvNeXt-Tiny stage (56 x 96 ..
//     7 x 768), and 7 divides every one of its widths: 96 items per full row.
//   * the row's d goes to an fp32 LDS tile [TW'][C]; behind one barrier, groups of 4 .. 32 lanes
//     (C / 32 rounded up to a power of two) each normalise one pixel: chunks to registers, sum and
//     butterfly, mean by division, deviations in registers, their squares and a second butterfly,
//     then gamma / beta and 16-byte bf16 stores. A second barrier frees the tile for the next row.
//
// Every sum has a fixed order and nothing is atomic: replays are bit-identical.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int DL_T = 256;               // threads per workgroup
constexpr int DL_PF = 6;                // 16-byte chunks of the next input row a thread holds in flight
constexpr int DL_LDS_MAX = 160 * 1024;

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // the fp32 vectors are 4-byte aligned

__device__ __forceinline__ void dl_load8(const float* p, float* o) {
  const f32x4u a = *(const f32x4u*)p, b = *(const f32x4u*)(p + 4);
  o[0] = a[0]; o[1] = a[1]; o[2] = a[2]; o[3] = a[3];
  o[4] = b[0]; o[5] = b[1]; o[6] = b[2]; o[7] = b[3];
}

// lanes that share a pixel in the LayerNorm pass: each owns up to 4 chunks of 8 channels
static int dl_lpp(int C) {
  int l = 4;
  while (l * 32 < C) l *= 2;
  return l;
}

// LayerNorm of one pixel whose channels sit in the registers of `lpp` neighbouring lanes: lane
// `sub` holds chunks sub + lpp * j (zeros where that is past C / 8) and their sum s. Two passes:
// the mean, then the squared deviations from it; v keeps the deviations for the output.
__device__ __forceinline__ void dl_norm_store(float (&v)[4][8], float s, int sub, int lpp, int C, float eps,
                                              const float* gamma, const float* beta, uint16_t* yp, bool live) {
  const int C8 = C >> 3;
  for (int off = lpp >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  const float mu = s / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float mj = sub + lpp * j < C8 ? mu : 0.f;      // an absent chunk is zeros about 0
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      v[j][d] -= mj;
      sq = fmaf(v[j][d], v[j][d], sq);
    }
  }
  for (int off = lpp >> 1; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);
  const float rstd = rsqrtf(sq / (float)C + eps);
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c8 = sub + lpp * j;
    if (c8 < C8) {
      float g[8], bb[8];
      dl_load8(gamma + c8 * 8, g);
      dl_load8(beta + c8 * 8, bb);
      u32x4 o;
#pragma unroll
      for (int d = 0; d < 4; ++d)
        o[d] = pack_bf16(fmaf(v[j][2 * d] * rstd, g[2 * d], bb[2 * d]),
                         fmaf(v[j][2 * d + 1] * rstd, g[2 * d + 1], bb[2 * d + 1]));
      *(u32x4*)(yp + c8 * 8) = o;
    }
  }
}

template <int PW>
__global__ __launch_bounds__(DL_T) void dwconv7_ln_kernel(DwLnArgs a, int R, int TW, int nring, int lpp) {
  extern __shared__ __attribute__((aligned(16))) uint8_t dsm[];
  const int tid = threadIdx.x;
  const int C = a.C, C8 = C >> 3;
  const int x0 = blockIdx.x * TW, tw = min(TW, a.W - x0);
  const int oy0 = blockIdx.y * R, oy1 = min(a.H, oy0 + R);
  const int b = blockIdx.z;
  const int NPG = (TW + PW - 1) / PW, LW = NPG * PW + 6;
  const int PSTR = 2 * C + 16, ROWB = LW * PSTR;
  const int NCH = LW * C8;                                  // 16-byte chunks of one ring row
  float* dbuf = (float*)(dsm + (size_t)nring * ROWB);       // the row's d: [NPG * PW][C] fp32
  const uint16_t* xb = a.x + (long)b * a.H * a.W * a.ldx;

  // chunk i of input row r: ring column i / C8 is map column x0 - 3 + i / C8; zeros outside the map
  auto fetch = [&](int r, int i) {
    const int col = i / C8, c8 = i - col * C8, gx = x0 - 3 + col;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (gx >= 0 && gx < a.W) v = *(const u32x4*)(xb + ((long)r * a.W + gx) * a.ldx + c8 * 8);
    return v;
  };
  auto slot = [&](int r, int i) {
    const int col = i / C8, c8 = i - col * C8;
    return (u32x4*)(dsm + (size_t)(r % nring) * ROWB + col * PSTR + c8 * 16);
  };

  // prologue: the input rows of the band's first output row
  for (int r = max(0, oy0 - 3); r <= min(a.H - 1, oy0 + 3); ++r)
    for (int i = tid; i < NCH; i += DL_T) *slot(r, i) = fetch(r, i);
  __syncthreads();

  const int lsh = __ffs(lpp) - 1, sub = tid & (lpp - 1), grp = tid >> lsh, ngrp = DL_T >> lsh;
  for (int oy = oy0; oy < oy1; ++oy) {
    // the one row output row oy + 1 adds, in flight across this row's FMAs
    const int rn = oy + 4;
    const bool more = oy + 1 < oy1 && rn < a.H;
    u32x4 pf[DL_PF];
    if (more) {
#pragma unroll
      for (int k = 0; k < DL_PF; ++k)
        if (tid + k * DL_T < NCH) pf[k] = fetch(rn, tid + k * DL_T);
    }

    for (int it = tid; it < NPG * C8; it += DL_T) {
      const int pg = it / C8, c8 = it - pg * C8;
      float acc[PW][8];
      dl_load8(a.bias + c8 * 8, acc[0]);
#pragma unroll
      for (int p = 1; p < PW; ++p)
#pragma unroll
        for (int d = 0; d < 8; ++d) acc[p][d] = acc[0][d];
#pragma unroll 1
      for (int ky = 0; ky < 7; ++ky) {
        const int iy = oy + ky - 3;
        if (iy < 0 || iy >= a.H) continue;                  // workgroup-uniform
        float wk[7][8];
#pragma unroll
        for (int kx = 0; kx < 7; ++kx) dl_load8(a.w + (long)(ky * 7 + kx) * C + c8 * 8, wk[kx]);
        const uint8_t* rp = dsm + (size_t)(iy % nring) * ROWB + pg * PW * PSTR + c8 * 16;
#pragma unroll
        for (int j = 0; j < PW + 6; ++j) {
          const u32x4 u = *(const u32x4*)(rp + j * PSTR);
          float xv[8];
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            xv[2 * d] = bf_lo(u[d]);
            xv[2 * d + 1] = bf_hi(u[d]);
          }
#pragma unroll
          for (int p = 0; p < PW; ++p) {
            const int kx = j - p;                           // compile-time after unrolling
            if (kx >= 0 && kx < 7) {
#pragma unroll
              for (int d = 0; d < 8; ++d) acc[p][d] = fmaf(xv[d], wk[kx][d], acc[p][d]);
            }
          }
        }
      }
#pragma unroll
      for (int p = 0; p < PW; ++p) {
        float* dp = dbuf + (pg * PW + p) * C + c8 * 8;
        *(f32x4*)dp = (f32x4){acc[p][0], acc[p][1], acc[p][2], acc[p][3]};
        *(f32x4*)(dp + 4) = (f32x4){acc[p][4], acc[p][5], acc[p][6], acc[p][7]};
      }
    }

    if (more) {
#pragma unroll
      for (int k = 0; k < DL_PF; ++k)
        if (tid + k * DL_T < NCH) *slot(rn, tid + k * DL_T) = pf[k];
    }
    __syncthreads();

    uint16_t* yrow = a.y + (((long)b * a.H + oy) * a.W + x0) * a.ldy;
    for (int p0 = 0; p0 < tw; p0 += ngrp) {                 // same trip count in every lane
      const int p = p0 + grp;
      const bool live = p < tw;
      const float* dp = dbuf + (live ? p : 0) * C;
      float v[4][8];
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c8 = sub + lpp * j;
        if (c8 < C8) {
          const f32x4 lo = *(const f32x4*)(dp + c8 * 8), hi = *(const f32x4*)(dp + c8 * 8 + 4);
#pragma unroll
          for (int d = 0; d < 4; ++d) { v[j][d] = lo[d]; v[j][d + 4] = hi[d]; }
        } else {
#pragma unroll
          for (int d = 0; d < 8; ++d) v[j][d] = 0.f;
        }
#pragma unroll
        for (int d = 0; d < 8; ++d) s += v[j][d];
      }
      dl_norm_store(v, s, sub, lpp, C, a.eps, a.gamma, a.beta, yrow + (long)(live ? p : 0) * a.ldy, live);
    }
    __syncthreads();
  }
}

// one pixel per group of lpp lanes, DL_T / lpp pixels per workgroup
__global__ __launch_bounds__(DL_T) void ln_s2d_kernel(LnS2dArgs a, int lpp, long npix) {
  const int tid = threadIdx.x;
  const int lsh = __ffs(lpp) - 1, sub = tid & (lpp - 1), grp = tid >> lsh, ngrp = DL_T >> lsh;
  const long pix = (long)blockIdx.x * ngrp + grp;
  const bool live = pix < npix;
  const long q = live ? pix : 0;
  const int ox = (int)(q % a.W), oy = (int)(q / a.W % a.H), b = (int)(q / ((long)a.W * a.H));
  const uint16_t* xp = a.x + q * a.ldx;
  const int C8 = a.C >> 3;
  float v[4][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c8 = sub + lpp * j;
    u32x4 u = {0u, 0u, 0u, 0u};
    if (c8 < C8) u = *(const u32x4*)(xp + c8 * 8);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      v[j][2 * d] = bf_lo(u[d]);
      v[j][2 * d + 1] = bf_hi(u[d]);
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) s += v[j][d];
  }
  const long row = ((long)b * (a.H / 2) + oy / 2) * (a.W / 2) + ox / 2;
  uint16_t* yp = a.y + row * a.ldy + ((oy & 1) * 2 + (ox & 1)) * a.C;
  dl_norm_store(v, s, sub, lpp, a.C, a.eps, a.gamma, a.beta, yp, live);
}

static bool dl_al(const void* p, uintptr_t m) { return p && ((uintptr_t)p & (m - 1)) == 0; }

// pixels per conv item: the one of 7 / 4 that pads a strip of TW columns less (7 on a tie)
static int dl_pw(int TW) { return (TW + 6) / 7 * 7 <= (TW + 3) / 4 * 4 ? 7 : 4; }

static int dl_nring(const DwLnArgs& a, int R) { return min(8, min(a.H, R + 6)); }

static size_t dl_smem(const DwLnArgs& a, int R, int TW) {
  const int PW = dl_pw(TW), NP = (TW + PW - 1) / PW * PW;
  return (size_t)dl_nring(a, R) * (NP + 6) * (2 * a.C + 16) + (size_t)NP * a.C * 4;
}

static bool dl_fits(const DwLnArgs& a, int R, int TW) {
  const int PW = dl_pw(TW), NP = (TW + PW - 1) / PW * PW;
  return dl_smem(a, R, TW) <= (size_t)DL_LDS_MAX && (long)(NP + 6) * (a.C / 8) <= DL_PF * DL_T;
}

hipError_t dwconv7_ln_plan(const DwLnArgs& a, int* rows, int* tw) {
  if (a.C % 8 != 0 || a.C < 32 || a.C > 1024) return hipErrorInvalidValue;
  if (a.ldx < a.C || a.ldy < a.C || a.ldx % 8 != 0 || a.ldy % 8 != 0) return hipErrorInvalidValue;
  if (!dl_al(a.x, 16) || !dl_al(a.y, 16) || !dl_al(a.w, 4) || !dl_al(a.bias, 4) || !dl_al(a.gamma, 4) ||
      !dl_al(a.beta, 4))
    return hipErrorInvalidValue;
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.W < 1 || !(a.eps > 0.f)) return hipErrorInvalidValue;
  if (a.rows < 0 || a.tw < 0) return hipErrorInvalidValue;
  // strip width: the whole row where the ring fits, else halved until it does (with the ring of
  // the tallest band where the band height is still open)
  const int Rfit = a.rows ? min(a.rows, a.H) : a.H;
  int TW = a.tw ? min(a.tw, a.W) : a.W;
  while (!a.tw && TW > 1 && !dl_fits(a, Rfit, TW)) TW = (TW + 1) / 2;
  if (!dl_fits(a, Rfit, TW)) return hipErrorInvalidValue;
  // band height: a band of R rows costs R + 6 row steps (six halo rows to fetch) and the grid runs in
  // ceil(workgroups / 256 CUs) rounds; the R with the least rounds x steps, the taller on a tie. At
  // batch 32 that is 7 / 4 / 2 / 1 rows for the 56 / 28 / 14 / 7 maps (224 or 256 workgroups each),
  // the fastest of the heights measured for each of them (profiles/convnext.txt)
  const long ns = (a.W + TW - 1) / TW;
  int R = Rfit;
  long best = -1;
  for (int r = Rfit; !a.rows && r >= 1; --r) {
    const long wgs = (long)a.B * ((a.H + r - 1) / r) * ns, cost = (wgs + 255) / 256 * (r + 6);
    if (best < 0 || cost < best) { best = cost; R = r; }
  }
  *rows = R;
  *tw = TW;
  return hipSuccess;
}

hipError_t dwconv7_ln(const DwLnArgs& a, hipStream_t s) {
  int R = 0, TW = 0;
  const hipError_t e = dwconv7_ln_plan(a, &R, &TW);
  if (e != hipSuccess) return e;
  const long ns = (a.W + TW - 1) / TW, nb = (a.H + R - 1) / R;
  if (ns > 0x7fffffffL || nb > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)ns, (unsigned)nb, (unsigned)a.B);
  const size_t smem = dl_smem(a, R, TW);
  const int nring = dl_nring(a, R), lpp = dl_lpp(a.C);
  if (dl_pw(TW) == 7)
    hipLaunchKernelGGL((dwconv7_ln_kernel<7>), grid, dim3(DL_T), smem, s, a, R, TW, nring, lpp);
  else
    hipLaunchKernelGGL((dwconv7_ln_kernel<4>), grid, dim3(DL_T), smem, s, a, R, TW, nring, lpp);
  return hipGetLastError();
}

hipError_t ln_s2d(const LnS2dArgs& a, hipStream_t s) {
  if (a.C % 8 != 0 || a.C < 32 || a.C > 1024) return hipErrorInvalidValue;
  if (a.H < 2 || a.W < 2 || a.H % 2 != 0 || a.W % 2 != 0 || a.B < 1 || !(a.eps > 0.f)) return hipErrorInvalidValue;
  if (a.ldx < a.C || a.ldy < 4 * a.C || a.ldx % 8 != 0 || a.ldy % 8 != 0) return hipErrorInvalidValue;
  if (!dl_al(a.x, 16) || !dl_al(a.y, 16) || !dl_al(a.gamma, 4) || !dl_al(a.beta, 4)) return hipErrorInvalidValue;
  const int lpp = dl_lpp(a.C), ngrp = DL_T / lpp;
  const long npix = (long)a.B * a.H * a.W, nwg = (npix + ngrp - 1) / ngrp;
  if (nwg > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ln_s2d_kernel, dim3((unsigned)nwg), dim3(DL_T), 0, s, a, lpp, npix);
  return hipGetLastError();
}

}  // namespace kdl
