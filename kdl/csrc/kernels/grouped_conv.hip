// Grouped 3x3 convolution (cg = 4 / 8 / 16 / 32 channels per group) + folded-BN bias + ReLU:
// ResNeXt's conv2. NHWC fp16 / bf16, fp32 accumulation, stride 1 or 2, reading the zero-bordered
// (H + 2) x (W + 2) buffer the preceding 1x1 conv writes with opad = 1.
//
// Unit of work: a 16-channel slab. For cg <= 16 a slab is closed under the grouping (outputs of
// slab j read only inputs of slab j), so its weights are a 16 x 16 tile per tap that is block-
// diagonal in cg x cg blocks: 16 / cg times the MACs of the grouped sum, not G times as in the
// dense block-diagonal lowering. cg = 32 is a pair of slabs that read each other.
//
//   * workgroup = one image x a band of R output rows x NS (1 / 2 / 4) consecutive slabs, one wave
//     per slab. The wave's weights (5 or 9 B fragments, 20 / 36 VGPRs) stay in registers for the
//     workgroup's lifetime.
//   * input rows live in an LDS ring of 3 + stride row slots, each (W + 2) pixels x NS * 16
//     channels (pixel stride padded by 16 bytes). A row is fetched from global memory once per
//     band with row-contiguous 16-byte loads: while output row oy is computed, the `stride` new
//     rows of oy + 1 are in flight in registers; they land in the slots row oy does not read, and
//     one barrier per output row closes the step.
//   * MFMA v_mfma_f32_16x16x32_{bf16,f16}: 16 channels of the slab x 16 pixels of the row, K = 32 =
//     two taps x 16 channels (cg <= 16: five k-steps, the tenth tap's weights are zero and its
//     pixel operand re-reads tap 8, so no stray Inf meets a zero) or one tap x the pair's 32
//     channels (cg = 32: nine k-steps). All nine taps are shifted reads of the same LDS rows.
//   * the weights are the first MFMA operand, so a lane ends with four consecutive channels of one
//     pixel; lanes 16 apart swap halves of two pixel tiles and each stores 8 channels = 16 bytes.
//
// Every lane takes the same path through the loads: chunk indices are clamped, not branched on.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int GC_PF = 4;              // 16-byte chunks of the next rows a thread holds in flight
constexpr int GC_LDS_MAX = 64 * 1024;

template <int DT, int ST, bool PAIR>
__global__ __launch_bounds__(256) void grouped_conv_kernel(GroupedConvArgs a, int R, int csh) {
  using E = Elt<DT>;
  constexpr int KS = PAIR ? 9 : 5, RING = 3 + ST;
  extern __shared__ __attribute__((aligned(16))) uint8_t gsm[];
  const int tid = threadIdx.x, T = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int p = lane & 15, q = lane >> 4;
  const int CPP = 1 << csh;                       // 16-byte chunks per pixel = NS * 2
  const int PSTR = CPP * 16 + 16, WP = a.W + 2, ROWB = WP * PSTR;
  const int NCH = WP * CPP;                       // chunks per input row
  const int ch0 = blockIdx.x * CPP * 8;
  const int oy0 = blockIdx.y * R, oy1 = min(a.OH, oy0 + R);
  const int b = blockIdx.z;
  const uint16_t* xb = a.x + (long)b * (a.H + 2) * WP * a.ldx + ch0;

  // chunk c of padded input row r: global element offset and LDS byte offset
  auto gofs = [&](int r, int c) { return ((long)r * WP + (c >> csh)) * a.ldx + (c & (CPP - 1)) * 8; };
  auto lofs = [&](int r, int c) { return (r % RING) * ROWB + (c >> csh) * PSTR + (c & (CPP - 1)) * 16; };

  // the slab's weights and bias, resident for the whole band
  s16x8 wf[KS];
  {
    const uint16_t* wb = a.wp + ((long)(ch0 / 16 + wave) * KS * 64 + lane) * 8;
#pragma unroll
    for (int t = 0; t < KS; ++t) wf[t] = *(const s16x8*)(wb + t * 512);
  }
  const f32x4 bs = *(const f32x4*)(a.bias + ch0 + wave * 16 + 4 * q);

  // prologue: the three input rows of the band's first output row
  for (int i = tid; i < 3 * NCH; i += T) {
    const int k = i / NCH, c = i - k * NCH, r = oy0 * ST + k;
    *(u32x4*)(gsm + lofs(r, c)) = *(const u32x4*)(xb + gofs(r, c));
  }
  __syncthreads();

  const int npf = (ST * NCH + T - 1) / T;          // <= GC_PF (launcher)
  const int MT2 = (a.OW + 31) / 32;                // pairs of 16-pixel tiles per output row
  // byte offset of the lane's 8 channels inside a pixel of the ring
  const int choff = PAIR ? (wave >> 1) * 64 + q * 16 : wave * 32 + (q & 1) * 16;
  for (int oy = oy0; oy < oy1; ++oy) {
    // the `stride` rows output row oy + 1 adds, in flight across this row's MFMAs
    u32x4 pf[GC_PF];
    const bool more = oy + 1 < oy1;
    const int rn = (oy + 1) * ST + 3 - ST;
    if (more) {
#pragma unroll
      for (int i = 0; i < GC_PF; ++i) {
        if (i < npf) {
          const int idx = min(tid + i * T, ST * NCH - 1);
          const int k = (ST == 2 && idx >= NCH) ? 1 : 0;
          pf[i] = *(const u32x4*)(xb + gofs(rn + k, idx - k * NCH));
        }
      }
    }
    int rb[3];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) rb[ky] = ((oy * ST + ky) % RING) * ROWB;
    int koff[KS];
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      if (PAIR) {
        koff[t] = rb[t / 3] + (t % 3) * PSTR + choff;
      } else {
        const int ta = 2 * t, tb = 2 * t + 1 < 9 ? 2 * t + 1 : 8;
        const int oa = rb[ta / 3] + (ta % 3) * PSTR, ob = rb[tb / 3] + (tb % 3) * PSTR;
        koff[t] = ((q >> 1) ? ob : oa) + choff;
      }
    }
    uint16_t* yrow = a.y + ((long)b * a.OH + oy) * a.OW * a.ldy + ch0 + wave * 16 + 4 * (q & 2);
    for (int tp = 0; tp < MT2; ++tp) {
      const int xa = tp * 32, xc = xa + 16;
      const bool two = xc < a.OW;                  // wave-uniform
      const int pa = min(xa + p, a.OW - 1) * ST * PSTR, pc = min(xc + p, a.OW - 1) * ST * PSTR;
      f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const s16x8 fa = *(const s16x8*)(gsm + koff[t] + pa);
        acca = E::mfma(wf[t], fa, acca);
        if (two) {
          const s16x8 fc = *(const s16x8*)(gsm + koff[t] + pc);
          accc = E::mfma(wf[t], fc, accc);
        }
      }
      // bias, ReLU, round; then lanes q and q ^ 1 swap: even q keeps tile a, odd q tile c, 8 channels each
      float va[4], vc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        va[i] = acca[i] + bs[i];
        vc[i] = accc[i] + bs[i];
        if (a.relu) { va[i] = fmaxf(va[i], 0.f); vc[i] = fmaxf(vc[i], 0.f); }
      }
      const uint32_t a0 = E::pack(va[0], va[1]), a1 = E::pack(va[2], va[3]);
      const uint32_t c0 = E::pack(vc[0], vc[1]), c1 = E::pack(vc[2], vc[3]);
      const bool odd = q & 1;
      const uint32_t r0 = __shfl_xor(odd ? a0 : c0, 16, 64), r1 = __shfl_xor(odd ? a1 : c1, 16, 64);
      const u32x4 o = odd ? (u32x4){r0, r1, c0, c1} : (u32x4){a0, a1, r0, r1};
      const int px = (odd ? xc : xa) + p;
      if (px < a.OW) *(u32x4*)(yrow + (long)px * a.ldy) = o;
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < GC_PF; ++i) {
        const int idx = tid + i * T;
        if (i < npf && idx < ST * NCH) {
          const int k = (ST == 2 && idx >= NCH) ? 1 : 0;
          *(u32x4*)(gsm + lofs(rn + k, idx - k * NCH)) = pf[i];
        }
      }
    }
    __syncthreads();
  }
}

// slabs per workgroup (= waves): the widest of 4 / 2 / 1 that divides the slab count, so a pixel's
// run is 128 / 64 / 32 bytes; cg = 32 needs whole pairs (C = 32 G gives at least 2)
static int gc_slabs(int C) { return C % 64 == 0 ? 4 : C % 32 == 0 ? 2 : 1; }

static bool gc_aligned(const void* p) { return p && ((uintptr_t)p & 15) == 0; }

hipError_t grouped_conv(const GroupedConvArgs& a, hipStream_t s) {
  if (a.cg != 4 && a.cg != 8 && a.cg != 16 && a.cg != 32) return hipErrorInvalidValue;
  if (a.G < 1 || a.C != a.G * a.cg || a.C % 16 != 0) return hipErrorInvalidValue;
  if (a.stride != 1 && a.stride != 2) return hipErrorInvalidValue;
  if (a.B < 1 || a.B > 65535 || a.H < 1 || a.W < 1) return hipErrorInvalidValue;
  if (a.OH != (a.H - 1) / a.stride + 1 || a.OW != (a.W - 1) / a.stride + 1) return hipErrorInvalidValue;
  if (a.ldx < a.C || a.ldy < a.C || a.ldx % 8 != 0 || a.ldy % 8 != 0) return hipErrorInvalidValue;
  if (!gc_aligned(a.x) || !gc_aligned(a.wp) || !gc_aligned(a.bias) || !gc_aligned(a.y)) return hipErrorInvalidValue;
  if (a.dt < 0 || a.dt > 1 || a.rows < 0) return hipErrorInvalidValue;
  const int NS = gc_slabs(a.C), T = 64 * NS, CPP = 2 * NS;
  const int csh = NS == 4 ? 3 : NS == 2 ? 2 : 1;
  const int WP = a.W + 2, ring = 3 + a.stride;
  const size_t smem = (size_t)ring * WP * (CPP * 16 + 16);
  if (smem > (size_t)GC_LDS_MAX || a.stride * WP * CPP > GC_PF * T) return hipErrorInvalidValue;   // map too wide
  // band height: whole maps while they fill the chip twice over; halved (each band re-reads two
  // halo rows) until they do, so 14 x 14 and 7 x 7 maps and small batches still spread over the CUs
  const int nsl = a.C / (16 * NS);
  int R = a.rows ? min(a.rows, a.OH) : a.OH;
  while (!a.rows && R > 2 && (long)a.B * ((a.OH + R - 1) / R) * nsl < 512) R = (R + 1) / 2;
  const dim3 grid(nsl, (a.OH + R - 1) / R, a.B);
  const bool pair = a.cg == 32;
#define KDL_GC(DT, ST, PR) \
  hipLaunchKernelGGL((grouped_conv_kernel<DT, ST, PR>), grid, dim3(T), smem, s, a, R, csh)
  if (a.dt) {
    if (a.stride == 1) { if (pair) KDL_GC(1, 1, true); else KDL_GC(1, 1, false); }
    else { if (pair) KDL_GC(1, 2, true); else KDL_GC(1, 2, false); }
  } else {
    if (a.stride == 1) { if (pair) KDL_GC(0, 1, true); else KDL_GC(0, 1, false); }
    else { if (pair) KDL_GC(0, 2, true); else KDL_GC(0, 2, false); }
  }
#undef KDL_GC
  return hipGetLastError();
}

}  // namespace kdl
