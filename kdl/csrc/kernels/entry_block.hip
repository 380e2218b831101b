// Whole Xception entry block in ONE persistent kernel (block2: 147x147x64 -> 74x74x128):
//
//   y1  = ReLU(BN(pw1(dw1(x))))          SeparableConv2D 64 -> 128  (+ReLU)
//   y2  = BN(pw2(dw2(y1)))               SeparableConv2D 128 -> 128
//   out = maxpool3x3/2_same(y2) + BN(conv1x1/2(x))                  (guide.md:222-229 graph)
//
// Unfused, the block moves ~790 MB per batch of 32 through HBM (y1 and y2 are 177 MB each,
// written and read back, plus the pool pass) in four launches (~280 us measured, round 3).
// Here y1 and y2 never leave the CU: the kernel reads x once (88 MB) and writes the pooled
// block output (45 MB).
//
// Tiling: a work item is one POOLED output row k of one image and one strip of PC pooled
// columns. A workgroup walks a run of consecutive rows of a strip (host-built step table,
// `steps`), keeping rolling windows in LDS:
//   x ring   4 rows x (2PC+5) cols x C0   (DMA: two new rows per step)
//   y1 ring  4 rows x (2PC+3) cols x C1   (two new rows per step, written by GEMM1's epilogue)
//   y2       rows 2k, 2k+1 in accumulators; row 2k-1 carried in registers from the previous step
// The 3x3/2 pool needs y2 rows 2k-1..2k+1 (TF 'same', pad 1 for 147 -> 74), so every y1 / y2
// row is computed once per strip; only the 2 halo columns between strips are recomputed
// (~6 %). A run starts with two warm-up steps (y1 only; y1 + y2 without output).
//
// A step is four dependent stages: dw1 -> GEMM1 (+ residual GEMM) -> dw2 -> GEMM2 + pool. Two kernels:
//   entry_block_kernel     block3 (74x74x128 -> 37x37x256, ReLU on the block input): 8 waves, wave w owns
//                          output channels 32w..32w+31 of EVERY GEMM (pw1, pw2, the residual 1x1), so its
//                          pointwise weights live in registers for the whole kernel and the GEMMs read only
//                          activations from LDS. Every wave runs every stage. Two loops: the four-phase loop
//                          (config 1: a stage per barrier interval, five barriers per step with B0; depthwise
//                          on the VALU, v_dot2c_f32_bf16 over tap pairs with fp32 accumulate, each lane the 8
//                          channels of one pixel = its MFMA operand fragment, written fragment-linear to an
//                          LDS A buffer) and the two-phase loop (TWOPH, configs 21 and 23: the same step
//                          skewed by one stage, TWO barriers per step -- a DW phase (dw2 of step i, dw1 +
//                          residual GEMM of step i+1) and a GEMM phase (GEMM2 + pool + output of step i, GEMM1
//                          of step i+1, the x-row DMA of step i+2 in flight); A1 and A2 are separate buffers,
//                          the horizontal pool exchanges lanes (ds_bpermute) instead of LDS rows, no register
//                          is spilled; 23, block3's default: both depthwise convs on the matrix cores, the
//                          block-diagonal operand of sepconv_ws.hip).
//   entry_block_ws_kernel  block2, 16 waves in two roles that work on different steps at the same time (see
//                          its own comment further down).
// The table comment at the end of the file lists the configurations and what they replaced.
//
// LDS activation images are channel-PLANE major (16-byte slot = 8 channels of one pixel, a
// plane = one 8-channel chunk of a row, pitch PLP px, a multiple of 16): a depthwise / MFMA
// fragment read (16 pixels x 4 chunks per wave instruction) then touches all 64 banks once.
#include "common.h"
#include "launch.h"

#include <algorithm>

namespace kdl {

__device__ __attribute__((aligned(16))) uint8_t eb_zeros[256];

constexpr int EB_MAX_STEPS = 128;                  // steps per workgroup (host plan checks it)

// The workgroup's step words in two VGPRs: word i in lane i % 64 of v[i / 64]. A step is decoded with
// v_readlane at its (uniform) index: no LDS round trip at the head of every step's dependency chain
// (address math -> tap reads), which the LDS-resident table put there once per decode.
struct EbStepRegs {
  uint32_t v0 = 0, v1 = 0;
  __device__ __forceinline__ void load(const uint32_t* st, int n, int lane) {
    v0 = lane < n ? st[lane] : 0u;
    v1 = 64 + lane < n ? st[64 + lane] : 0u;
  }
  __device__ __forceinline__ uint32_t get(int i) const {
    i = __builtin_amdgcn_readfirstlane(i);
    return (uint32_t)__builtin_amdgcn_readlane((int)(i < 64 ? v0 : v1), i & 63);
  }
};
static_assert(EB_MAX_STEPS <= 128, "EbStepRegs holds two words per lane");

template <int C0_, int C1_, int PC_, int NFW_, bool DWM, bool TWOPH>
struct EbGeom {
  static constexpr int C0 = C0_, C1 = C1_, PC = PC_, NFW = NFW_;
  static constexpr int Y2C = 2 * PC + 1;            // y2 columns a strip needs
  static constexpr int Y1C = Y2C + 2;               // y1 columns
  static constexpr int XC = Y1C + 2;                // x columns
  static constexpr int PLP = (XC + 15) / 16 * 16;   // plane pitch (pixels)
  static constexpr int PLB = PLP * 16;              // plane bytes
  static constexpr int XROW = (C0 / 8) * PLB;       // one x ring row
  static constexpr int Y1ROW = (C1 / 8) * PLB;      // one y1 ring row
  static constexpr int KT0 = C0 / 32, KT1 = C1 / 32;
  static constexpr int Y1F = (2 * Y1C + 15) / 16;   // y1 pixel fragments per step (2 rows)
  static constexpr int Y2FR = (Y2C + 15) / 16;      // y2 fragments per row
  static constexpr int Y2F = 2 * Y2FR;
  static constexpr int NW = C1 / (16 * NFW);        // waves (NFW 16-channel output slices each)
  static constexpr int XDMA = XROW / 1024;          // 1 KiB DMA instructions per x row
  static constexpr int A1BYTES = KT0 * Y1F * 1024, A2BYTES = KT1 * Y2F * 1024;
  static constexpr int ABYTES = TWOPH ? A1BYTES + A2BYTES : (A1BYTES > A2BYTES ? A1BYTES : A2BYTES);
  static constexpr int PCOLS = 16 * Y2FR;           // pool row columns
  static constexpr int DWQ = DWM ? 1024 : 640;      // LDS depthwise entries per k-step: 4 lane groups x 40 words
                                                    // (VALU), or pack_dw_entries' 1 KiB (MFMA variant)
  // LDS map: the two depthwise A buffers alias (A1 is read before the barrier that precedes
  // A2's writes, A2 before the next step's first barrier). TWOPH: both are live in one barrier
  // interval (A2 at OFF_A, A1 behind it); the room comes from the pool rows, which that schedule
  // exchanges between lanes instead (ds_bpermute)
  static constexpr int OFF_X = 0;
  static constexpr int OFF_Y1 = OFF_X + 4 * XROW;
  static constexpr int OFF_A = OFF_Y1 + 4 * Y1ROW;
  static constexpr int OFF_A1 = OFF_A + A2BYTES;    // TWOPH only
  static constexpr int OFF_P = OFF_A + ABYTES;      // per-wave pool rows [NW][PCOLS][16*NFW] bf16
  static constexpr int OFF_DW = OFF_P + (TWOPH ? 0 : NW * PCOLS * 16 * NFW * 2);
  static constexpr int OFF_B = OFF_DW + (KT0 + KT1) * DWQ;   // biases [3][C1] fp32
  static constexpr int OFF_S = OFF_B + 3 * C1 * 4;  // this workgroup's step table, one packed word per step
  static constexpr int BYTES = OFF_S + 4 * EB_MAX_STEPS;
  static_assert(XROW % 1024 == 0, "whole DMA instructions per x row");
  static_assert(C0 % 32 == 0 && C1 % (16 * NFW) == 0 && NW <= 16, "channel tiling");
  static_assert(BYTES <= 160 * 1024, "LDS");
};

// four bf16 pairs (two 16-B taps a, b of one pixel: channels c..c+7) -> dot2 operands
// (a[c], b[c]) / (a[c+1], b[c+1]) per channel pair
__device__ __forceinline__ uint32_t eb_lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t eb_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
__device__ __forceinline__ float eb_dot(uint32_t x, uint32_t w, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, x), __builtin_bit_cast(bf16x2, w), c, false);
}

// depthwise 3x3 of 8 channels of one pixel, tap pair by tap pair (taps 2j, 2j+1; tap 9 = 0) so
// only one pair of 16-B taps and its 8 weight words are live at a time: tap(i) -> the 16-B input
// of tap i (dy*3+dx), wq -> [tap pair j][channel e] bf16x2 words (LDS, broadcast per lane group).
// fp32 accumulation (v_dot2c_f32_bf16); returns the 8 outputs as bf16 = one MFMA operand.
template <bool RELU, class Tap>
__device__ __forceinline__ s16x8 eb_dw8(Tap tap, const uint32_t* wq) {
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    u32x4 a = tap(2 * j);
    u32x4 b = j < 4 ? tap(2 * j + 1) : (u32x4){0u, 0u, 0u, 0u};
    const u32x4 w0 = *(const u32x4*)(wq + 8 * j), w1 = *(const u32x4*)(wq + 8 * j + 4);
    if constexpr (RELU) {
#pragma unroll
      for (int d = 0; d < 4; ++d) { a[d] = relu_bf16x2(a[d]); b[d] = relu_bf16x2(b[d]); }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t wl = d < 2 ? w0[2 * d] : w1[2 * d - 4], wh = d < 2 ? w0[2 * d + 1] : w1[2 * d - 3];
      acc[2 * d] = eb_dot(eb_lo(a[d], b[d]), wl, acc[2 * d]);
      acc[2 * d + 1] = eb_dot(eb_hi(a[d], b[d]), wh, acc[2 * d + 1]);
    }
  }
  u32x4 o;
#pragma unroll
  for (int d = 0; d < 4; ++d) o[d] = pack_bf16(acc[2 * d], acc[2 * d + 1]);
  return __builtin_bit_cast(s16x8, o);
}

// eb_dw8 for N units of one wave that share their weights (same k-step, same lane group): every
// tap pair's 8 weight words are read once for the N units, not once per unit, and no store sits
// between the units, so taps that two units share (tap(u, ti) with the same address: the two rows
// of a row pair share 6 of their 9) are read once as well. Per unit the operands and the order of
// the fp32 sums are eb_dw8's: bit-identical to it.
template <bool RELU, int N, class Tap>
__device__ __forceinline__ void eb_dw8_n(Tap tap, const uint32_t* wq, s16x8 (&out)[N]) {
  float acc[N][8];
#pragma unroll
  for (int u = 0; u < N; ++u)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[u][e] = 0.f;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const u32x4 w0 = *(const u32x4*)(wq + 8 * j), w1 = *(const u32x4*)(wq + 8 * j + 4);
#pragma unroll
    for (int u = 0; u < N; ++u) {
      u32x4 a = tap(u, 2 * j);
      u32x4 b = j < 4 ? tap(u, 2 * j + 1) : (u32x4){0u, 0u, 0u, 0u};
      if constexpr (RELU) {
#pragma unroll
        for (int d = 0; d < 4; ++d) { a[d] = relu_bf16x2(a[d]); b[d] = relu_bf16x2(b[d]); }
      }
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t wl = d < 2 ? w0[2 * d] : w1[2 * d - 4], wh = d < 2 ? w0[2 * d + 1] : w1[2 * d - 3];
        acc[u][2 * d] = eb_dot(eb_lo(a[d], b[d]), wl, acc[u][2 * d]);
        acc[u][2 * d + 1] = eb_dot(eb_hi(a[d], b[d]), wh, acc[u][2 * d + 1]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < N; ++u) {
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; ++d) o[d] = pack_bf16(acc[u][2 * d], acc[u][2 * d + 1]);
    out[u] = __builtin_bit_cast(s16x8, o);
  }
}

// depthwise 3x3 of a 16-pixel x 32-channel unit on the MATRIX cores (the block-diagonal operand of
// sepconv_ws.hip): per 16-channel group g, 5 MFMAs over tap pairs. Lane (p16, kb) feeds tap
// 2j + (kb >> 1) of chunk 2g + (kb & 1); tap(g, ti) -> that 16-B input; ent(g) -> the 16-B entry
// (pack_dw_entries) of channel 16g + p16, tap parity kb >> 1. The C fragment [16 ch][16 px] is
// written transposed into the unit's lane-linear A fragment at dst.
template <class Tap, class Ent>
__device__ __forceinline__ void eb_dw_mfma_vals(Tap tap, Ent ent, int lane, const uint32_t (&sel)[2][4], u32x2 (&out)[2]) {
  const int kb = lane >> 4, par = kb >> 1;
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    const u32x4 we = ent(g);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const int ti = 2 * j + par;
      const u32x4 v = ti < 9 ? tap(g, ti) : (u32x4){0u, 0u, 0u, 0u};
      const uint32_t wd = we[j >> 1];
      u32x4 wf;
#pragma unroll
      for (int d = 0; d < 4; ++d) wf[d] = __builtin_amdgcn_perm(wd, wd, sel[j & 1][d]);
      acc = mfma16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, v), acc);
    }
    out[g] = (u32x2){pack_bf16(acc[0], acc[1]), pack_bf16(acc[2], acc[3])};
  }
}

// the C fragment [16 ch][16 px] of both channel groups, written transposed into the unit's
// lane-linear A fragment at dst. Kept apart from the MFMAs so a phase can compute all of its
// units before its first store (a later unit's tap reads would otherwise wait behind it)
__device__ __forceinline__ void eb_dw_store(uint8_t* dst, int lane, const u32x2 (&out)[2]) {
  const int p16 = lane & 15, kb = lane >> 4, par = kb >> 1;
#pragma unroll
  for (int g = 0; g < 2; ++g) *(u32x2*)(dst + (p16 + 16 * (2 * g + par)) * 16 + 8 * (kb & 1)) = out[g];
}

// the block-diagonal weight operand of depthwise MFMA j (tap pair j) from a channel's 16-B entry
__device__ __forceinline__ u32x4 eb_dw_wop(const u32x4 we, int j, const uint32_t (&sel)[2][4]) {
  const uint32_t wd = we[j >> 1];
  u32x4 wf;
#pragma unroll
  for (int d = 0; d < 4; ++d) wf[d] = __builtin_amdgcn_perm(wd, wd, sel[j & 1][d]);
  return wf;
}

// Row-pair form of eb_dw_mfma_vals for ONE 16-channel group: output rows r and r+1 of a 16-pixel
// fragment. Both rows take the same five weight operands (MFMA j: tap 2j in the parity-0 lanes, 2j+1 in
// the parity-1 lanes, counted from each row's own first input row), so a wave whose items keep their
// channels builds them once: wop(j) -> the operand (eb_dw_wop of the entry, or its copy in registers).
// addr(ti) -> the input of tap ti counted over the FOUR input rows r-1..r+2 (ti = 3 * row + dx, 0..11)
// of this lane's chunk: row r+1's tap t is tap t+3. Every operand is exactly eb_dw_mfma_vals', so the
// sums are bit-identical to it. The ten 16-B reads stay: the two rows' windows share six taps, but
// always in the other half-wave (profiles/entry_block_rowpair.txt: 7 reads with the k-halves of row
// r+1 exchanged changed the sums, 8 reads with v_permlane32_swap cost more VALU than the reads saved).
// out[0] = row r, out[1] = row r+1.
template <class Addr, class Wop>
__device__ __forceinline__ void eb_dw_mfma_rowpair(Addr addr, Wop wop, int lane, u32x2 (&out)[2]) {
  const bool par = (lane & 32) != 0;
  u32x4 r0[5], r1[5];                                // tap operands of row r / row r+1
#pragma unroll
  for (int j = 0; j < 5; ++j) {                      // tap 9 (j 4, parity 1): any tap, its weight is 0
    r0[j] = *(const u32x4*)(par ? addr(j < 4 ? 2 * j + 1 : 8) : addr(2 * j));
    r1[j] = *(const u32x4*)(par ? addr(j < 4 ? 2 * j + 4 : 11) : addr(2 * j + 3));
  }
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const u32x4 wf = wop(j);
    acc0 = mfma16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, r0[j]), acc0);
    acc1 = mfma16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, r1[j]), acc1);
  }
  out[0] = (u32x2){pack_bf16(acc0[0], acc0[1]), pack_bf16(acc0[2], acc0[3])};
  out[1] = (u32x2){pack_bf16(acc1[0], acc1[1]), pack_bf16(acc1[2], acc1[3])};
}

// Two output rows of ONE 16-channel group that share their weight operands (eb_dw_mfma_rowpair's
// arithmetic, operand for operand), for the two-phase loop: a0[j] / a1[j] + off -> the input of MFMA j of
// row 0 / row 1 in this lane (the caller folds the tap parity of the half-wave into the addresses once
// per part; off is common to all lanes, an immediate of the read), so the rows need not be neighbours.
// The ten reads are fenced off from the MFMAs (sched_barrier): left alone, the scheduler interleaves
// read, wait and MFMA one by one to save registers, and a wave with a single partner on its SIMD then
// waits out every LDS latency in turn (profiles/entry_block3_dwm.txt, form 1 against form 2).
template <bool RELU, class Wop>
__device__ __forceinline__ void eb_dw_mfma_two(const uint8_t* const (&a0)[5], const uint8_t* const (&a1)[5], int off, Wop wop,
                                               u32x2 (&out)[2]) {
  u32x4 r0[5], r1[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    r0[j] = *(const u32x4*)(a0[j] + off);
    r1[j] = *(const u32x4*)(a1[j] + off);
  }
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    if constexpr (RELU) {
#pragma unroll
      for (int d = 0; d < 4; ++d) { r0[j][d] = relu_bf16x2(r0[j][d]); r1[j][d] = relu_bf16x2(r1[j][d]); }
    }
    const u32x4 wf = wop(j);
    acc0 = mfma16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, r0[j]), acc0);
    acc1 = mfma16(__builtin_bit_cast(s16x8, wf), __builtin_bit_cast(s16x8, r1[j]), acc1);
  }
  out[0] = (u32x2){pack_bf16(acc0[0], acc0[1]), pack_bf16(acc0[2], acc0[3])};
  out[1] = (u32x2){pack_bf16(acc1[0], acc1[1]), pack_bf16(acc1[2], acc1[3])};
}

// one channel group's C fragment [16 ch][16 px], transposed into the A fragment at dst (eb_dw_store's
// mapping for group g)
__device__ __forceinline__ void eb_dw_store_g(uint8_t* dst, int lane, int g, u32x2 val) {
  const int p16 = lane & 15, kb = lane >> 4;
  *(u32x2*)(dst + (p16 + 16 * (2 * g + (kb >> 1))) * 16 + 8 * (kb & 1)) = val;
}

// workgroup barrier for LDS hand-offs only: LDS-scoped release / acquire fences around s_barrier, so
// the compiler orders LDS accesses around it and emits only lgkmcnt(0). __syncthreads() (a fence over
// every address space) lowers to s_waitcnt vmcnt(0) lgkmcnt(0) + s_barrier, which drained the next
// step's x-row LDS-DMA at the first phase barrier after its issue (B2) instead of at B0
__device__ __forceinline__ void eb_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// 16-byte global -> LDS DMA as inline asm (M0 = the wave-uniform LDS address; lane l lands at M0 + 16 l).
// The compiler's waitcnt pass cannot tell an LDS-DMA destination from other LDS regions and drains
// (vmcnt(0)) every in-flight DMA before some later LDS stores; asm is invisible to it. CONTRACT: the
// caller waits for the DMA with its own vmcnt, and no compiler-tracked VMEM load is in flight across it.
__device__ __forceinline__ void glds16_asm(const void* g, void* lds) {
  const uint32_t m0 = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_void*)lds);
  asm volatile("s_mov_b32 m0, %1\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(m0) : "memory", "m0");
}

__device__ __forceinline__ s16x8 eb_frag(const uint16_t* wp, int nf, int kt, int t, int lane) {
  return *(const s16x8*)(wp + ((long)(nf * kt + t) * 64 + lane) * 8);
}

// Block3 (even maps: the leading pad of the TF-'same' 3x3/2 pool is 0; ReLU on the block input). STAMP: the
// diagnostics build; TWOPH: the two-phase loop (false: the four-phase loop of config 1, VALU depthwise only);
// DWM: depthwise on the matrix cores (two-phase only)
template <bool DWM, bool TWOPH>
using Eb3Geom = EbGeom<128, 256, 13, 2, DWM, TWOPH>;
template <bool STAMP, bool DWM, bool TWOPH>
__global__ __launch_bounds__((64 * Eb3Geom<DWM, TWOPH>::NW), (Eb3Geom<DWM, TWOPH>::NW / 4)) void entry_block_kernel(EntryBlockArgs a) {
  using G = Eb3Geom<DWM, TWOPH>;
  static_assert(TWOPH || !DWM, "the four-phase LDS map has no room for the MFMA depthwise entries");
  constexpr int C0 = G::C0, C1 = G::C1, PC = G::PC, NFW = G::NFW;
  constexpr int NW = G::NW, KT0 = G::KT0, KT1 = G::KT1;
  constexpr int PLB = G::PLB, XROW = G::XROW, Y1ROW = G::Y1ROW;
  constexpr int Y1C = G::Y1C, Y2C = G::Y2C, XC = G::XC, PLP = G::PLP;
  constexpr int Y1F = G::Y1F, Y2F = G::Y2F, Y2FR = G::Y2FR, PCOLS = G::PCOLS;
  constexpr int U1 = KT0 * Y1F, U2 = KT1 * Y2F;      // depthwise units (fragment x k-step)
  constexpr int U1W = (U1 + NW - 1) / NW, U2W = (U2 + NW - 1) / NW;
  constexpr int PCH = 16 * NFW;                      // channels per wave
  static_assert(NW % KT0 == 0 && NW % KT1 == 0, "a wave's depthwise units share one k-step");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q16 = lane >> 4, p16 = lane & 15;
  const int H = a.H, W = a.W;
  const int s0 = a.step_off[blockIdx.x], s1 = a.step_off[blockIdx.x + 1];
  if (s0 >= s1 || s1 - s0 > EB_MAX_STEPS) return;   // uniform: no work (or a plan the host must reject)

  uint8_t* const xr = smem + G::OFF_X;
  uint8_t* const y1r = smem + G::OFF_Y1;
  uint8_t* const Ab = smem + G::OFF_A;
  uint16_t* const pool = (uint16_t*)(smem + G::OFF_P) + w * (PCOLS * PCH);
  uint32_t* const dwl = (uint32_t*)(smem + G::OFF_DW);
  float* const bl = (float*)(smem + G::OFF_B);
  uint32_t* const stl = (uint32_t*)(smem + G::OFF_S);
  // the step table goes to LDS once: decoding a step from global memory put an L2 round trip
  // on every step's critical path twice (measured ~3k cycles per step, tools/ebbench.py --stamps).
  // One word per step {image 8 | strip 6 | pooled row + 2 9 | mode 2 bits}
  for (int i = tid; i < s1 - s0; i += 64 * NW) {
    const int4 e = a.steps[s0 + i];
    stl[i] = (uint32_t)e.x | ((uint32_t)e.y << 8) | ((uint32_t)(e.z + 2) << 14) | ((uint32_t)e.w << 23);
  }

  // ---- depthwise weight entries -> LDS. VALU variant: [k-step][lane group q][tap pair j][channel e]
  // bf16x2; MFMA variant (DWM): pack_dw_entries' [k-step][g][n][parity][8] bf16, 1 KiB per k-step
  if constexpr (DWM) {
    for (int i = tid; i < (KT0 + KT1) * 64; i += 64 * NW) {
      const int t = i / 64;
      const u32x4 v = t < KT0 ? *(const u32x4*)((const uint8_t*)a.dwk1 + t * 1024 + (i % 64) * 16)
                              : *(const u32x4*)((const uint8_t*)a.dwk2 + (t - KT0) * 1024 + (i % 64) * 16);
      *(u32x4*)((uint8_t*)dwl + t * G::DWQ + (i % 64) * 16) = v;
    }
  } else
  for (int i = tid; i < (KT0 + KT1) * 4 * 40; i += 64 * NW) {
    const int t = i / 160, q = (i / 40) % 4, j = (i % 40) / 8, e = i % 8;
    const bool second = t >= KT0;
    const float* wsrc = second ? a.dw2 : a.dw1;
    const int C = second ? C1 : C0, c = 32 * (second ? t - KT0 : t) + 8 * q + e;
    const float wa = wsrc[(2 * j) * C + c];
    const float wb = j < 4 ? wsrc[(2 * j + 1) * C + c] : 0.f;
    dwl[i] = pack_bf16(wa, wb);
  }
  // ---- register-resident pointwise weights of this wave's NFW x 16 output channels
  s16x8 w1[NFW][KT0], w2[NFW][KT1];
#pragma unroll
  for (int n = 0; n < NFW; ++n) {
#pragma unroll
    for (int t = 0; t < KT0; ++t) w1[n][t] = eb_frag(a.w1, NFW * w + n, KT0, t, lane);
#pragma unroll
    for (int t = 0; t < KT1; ++t) w2[n][t] = eb_frag(a.w2, NFW * w + n, KT1, t, lane);
  }
  for (int i = tid; i < 3 * C1; i += 64 * NW) bl[i] = (i < C1 ? a.b1 : i < 2 * C1 ? a.b2 : a.br)[i % C1];
  // this lane's 4 accumulator channels of output slice n: bias (LDS) of GEMM g (0 pw1, 1 pw2, 2 residual)
  auto bias = [&](int g, int n) { return *(const float4*)(bl + g * C1 + PCH * w + 16 * n + 4 * q16); };
  const int t1 = w % KT0, t2 = w % KT1;              // every depthwise unit of this wave uses these k-steps
  // ---- x row DMA: row r of image b, strip columns from global col gx0, into ring slot r & 3
  // (preparing the addresses ahead, before B1, measured slower: the wave runs it in order anyway)
  auto dma_rows = [&](int b, int gx0, int r0, int nr) {
    for (int ii = w; ii < nr * G::XDMA; ii += NW) {
      const int r = r0 + ii / G::XDMA, d = ii % G::XDMA;
      const int slot = d * 64 + lane, plane = slot / PLP, px = slot - plane * PLP;
      const int gx = gx0 + px;
      const bool ok = px < XC && (unsigned)r < (unsigned)H && (unsigned)gx < (unsigned)W;
      const uint8_t* src = ok ? (const uint8_t*)(a.x + (((long)b * H + r) * W + gx) * a.ldx + plane * 8) : eb_zeros;
      glds16(src, xr + (r & 3) * XROW + d * 1024);
    }
  };
  auto decode = [&](int q, int& b, int& s, int& k, int& mode) {
    const uint32_t e = stl[q - s0];
    b = e & 255; s = (e >> 8) & 63; k = (int)((e >> 14) & 511) - 2; mode = (e >> 23) & 3;
  };
  // pooled row k pools y2 rows R..R+2, R = 2k; a step computes y1 rows R+2, R+3 from x rows
  // R+1..R+4: the rows its predecessor did not load (a run's first step loads all four)
  auto dma_for = [&](int q) {
    int b, s, k, mode;
    decode(q, b, s, k, mode);
    const int R = 2 * k;
    const int gx0 = 2 * s * PC - 2;
    if (mode == 0) dma_rows(b, gx0, R + 1, 4);
    else dma_rows(b, gx0, R + 3, 2);
  };

  u32x2 carry[NFW][Y2FR];                            // y2 row R+2 of the previous step (= this step's R), bf16
  f32x4 accr[NFW];                                   // residual GEMM of the pooled row it was computed for
  s16x8 wr[NFW][KT0];                                // residual 1x1/2 weights (register-resident)
#pragma unroll
  for (int n = 0; n < NFW; ++n)
#pragma unroll
    for (int t = 0; t < KT0; ++t) wr[n][t] = eb_frag(a.wr, NFW * w + n, KT0, t, lane);
  bool st_pend = false;                              // deferred output store of the previous step
  uint16_t* st_ptr = nullptr;
  u32x2 st_val[NFW];

  // STAMP builds (diagnostics, tools/ebbench.py --stamps): thread 0 of workgroups < 8 records
  // s_memtime after each barrier of its first 64 steps: [wg][step][B0, B1, B2, B3, end]
  auto stamp = [&](int q, int ph) {
    if constexpr (STAMP) {
      if (tid == 0 && blockIdx.x < 8 && q - s0 < 64 && a.stamps)
        a.stamps[((long)blockIdx.x * 64 + (q - s0)) * 5 + ph] = __builtin_amdgcn_s_memtime();
    }
  };
  __syncthreads();                                   // step table, weights, biases in LDS
  dma_for(s0);
  if constexpr (TWOPH) {
    // ---- two-phase schedule (config 21): the step skewed by one stage, two barriers per step.
    // Iteration `it` runs the second half of step it next to the first half of step it + 1:
    //   DW phase    dw2(it): y1 ring -> A2         dw1(it + 1): x ring -> A1, + its residual 1x1/2 GEMM
    //   barrier A   then the x-row DMA of step it + 2 and the deferred output store of step it - 1
    //   GEMM phase  GEMM2(it) + pool + output      GEMM1(it + 1): A1 -> y1 ring
    //   barrier B   (= B0: vmcnt(0) for the landed x rows)
    // The first iteration (it = s0 - 1) has only the (it + 1) half, the last only the (it) half; the
    // halves are predicated, every wave runs both barriers of every iteration. Operands, dot orders
    // and rounding points are the four-phase loop's: the output is bit-identical to it.
    // y1 ring slots are counted by steps: step j writes its rows R+2, R+3 into pair j & 1 and reads
    // R, R+1 from the other pair (its predecessor's), so the rows of two runs walked back to back
    // never meet in a slot whatever their row numbers are.
    static_assert(Y2FR == 2 && U1 % NW == 0 && NW == KT1,
                  "two-phase schedule: block3's two-slice build (a wave's dw2 units: one k-step)");
    uint8_t* const A2 = Ab;
    uint8_t* const A1 = smem + G::OFF_A1;
    auto word = [&](int q) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)stl[q - s0]); };
    auto yslot = [](int j, int o) { return 2 * ((j + (o >> 1) + 1) & 1) + (o & 1); };   // row R + o of step j
    // every part of an iteration derives its per-lane addresses from an opaque copy of the lane index:
    // as loop invariants they are hoisted out of the loop by the dozen and kept in scratch, and a
    // scratch reload in the GEMM phase waits, in vmcnt order, for the x-row DMA issued ahead of it
    auto fresh = [&]() { int l = lane; asm volatile("" : "+v"(l)); return l; };
    // DWM: the v_perm selectors of the block-diagonal operand, rebuilt per iteration like the addresses
    auto mksel = [](int lane, uint32_t (&sl)[2][4]) {
      const int p16 = lane & 15, q16 = lane >> 4, e = p16 & 7;
      const bool wv = (p16 >> 3) == (q16 & 1);
#pragma unroll
      for (int jp = 0; jp < 2; ++jp)
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const uint32_t pair = (2u * jp) | ((2u * jp + 1u) << 8);
          const uint32_t val = (e & 1) ? (0x0c0cu | (pair << 16)) : (0x0c0c0000u | pair);
          sl[jp][d] = (wv && (e >> 1) == d) ? val : 0x0c0c0c0cu;
        }
    };
    // residual carry: dw1 runs a step early, so the residual of pooled row k + 1 (read with x row
    // 2k + 2 in the ring) is two iterations ahead of its output. fp32, never rounded.
    f32x4 res0[NFW], res1[NFW], res2[NFW];           // of the output of step it / it + 1 / it + 2
#pragma unroll
    for (int n = 0; n < NFW; ++n) res0[n] = res1[n] = res2[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                 // the first step's x rows landed
    for (int it = s0 - 1; it < s1; ++it) {
      const bool hn = it + 1 < s1;                   // uniform (SGPR) predicates of the two halves
      const uint32_t ec = it >= s0 ? word(it) : 0u, en = hn ? word(it + 1) : 0u;
      const int mc = (ec >> 23) & 3, mn = (en >> 23) & 3;   // mc 0: nothing to do for step it
      const int b = ec & 255, pc0 = (int)((ec >> 8) & 63) * PC, k = (int)((ec >> 14) & 511) - 2;
      const int pcn = (int)((en >> 8) & 63) * PC, Rn = 2 * ((int)((en >> 14) & 511) - 2);
      const int R = 2 * k;
      if (it >= s0) stamp(it, 0);
      // DWM (config 23): both depthwise convs on the matrix cores. The v_perm selectors of the block-diagonal
      // weight operand are rebuilt once per DW phase, and each part folds the half-wave's tap parity into
      // five addresses per row once (MFMA j reads tap 2j in the parity-0 lanes, 2j + 1 in the parity-1
      // lanes; j 4, parity 1: any tap, its weight is 0): the items of a part differ by an immediate
      uint32_t sel[2][4];
      if constexpr (DWM) mksel(fresh(), sel);
      // ---- DW phase. dw2(it) -> A2 (y2 rows R+1, R+2: fragments [row][col / 16])
      if (mc >= 1) {
        const int lane = fresh(), p16 = lane & 15, q16 = lane >> 4;
        if constexpr (DWM) {
          // per 16-channel group g the five weight operands are rebuilt from the group's LDS entry (no
          // registers to keep them) and serve the row pair of both column fragments: 10 tap reads and 10
          // MFMAs per (g, fragment), all eight results stored after the last read
          const bool par = (lane & 32) != 0;
          const uint8_t* base = y1r + (4 * t2 + (q16 & 1)) * PLB + p16 * 16;
          const uint8_t *a0[5], *a1[5];              // y2 row R+1 reads y1 rows R..R+2, row R+2 rows R+1..R+3
#pragma unroll
          for (int j = 0; j < 5; ++j) {
            const int te = 2 * j, to = j < 4 ? 2 * j + 1 : 8;
            a0[j] = base + (par ? yslot(it, to / 3) * Y1ROW + (to % 3) * 16 : yslot(it, te / 3) * Y1ROW + (te % 3) * 16);
            a1[j] = base + (par ? yslot(it, to / 3 + 1) * Y1ROW + (to % 3) * 16 : yslot(it, te / 3 + 1) * Y1ROW + (te % 3) * 16);
          }
          u32x2 dv[2][Y2FR][2];
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const u32x4 we = *(const u32x4*)((const uint8_t*)dwl + (KT0 + t2) * G::DWQ + ((g * 16 + p16) * 2 + (q16 >> 1)) * 16);
            u32x4 wk[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) wk[j] = eb_dw_wop(we, j, sel);
#pragma unroll
            for (int fc = 0; fc < Y2FR; ++fc)
              eb_dw_mfma_two<false>(a0, a1, 2 * g * PLB + fc * 256, [&](int j) { return wk[j]; }, dv[g][fc]);
          }
#pragma unroll
          for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int fc = 0; fc < Y2FR; ++fc)
#pragma unroll
              for (int rr = 0; rr < 2; ++rr)
                eb_dw_store_g(A2 + (t2 * Y2F + rr * Y2FR + fc) * 1024, lane, g, dv[g][fc][rr]);
        } else {
          // a wave's four units are the two rows of both column fragments at its k-step: per fragment a
          // row pair (eb_dw8_n: 12 distinct tap reads for the two rows), all four stored after the last read
          const uint32_t* wq = dwl + ((KT0 + t2) * 4 + q16) * 40;
          s16x8 o2[Y2FR][2];
#pragma unroll
          for (int fc = 0; fc < Y2FR; ++fc) {
            const uint8_t* base = y1r + (4 * t2 + q16) * PLB + (fc * 16 + p16) * 16;
            auto tap = [&](int rr, int ti) {         // y2 row R+1+rr reads y1 rows R+rr .. R+rr+2
              return *(const u32x4*)(base + yslot(it, rr + ti / 3) * Y1ROW + (ti % 3) * 16);
            };
            eb_dw8_n<false, 2>(tap, wq, o2[fc]);
          }
#pragma unroll
          for (int fc = 0; fc < Y2FR; ++fc)
#pragma unroll
            for (int rr = 0; rr < 2; ++rr) *(s16x8*)(A2 + (t2 * Y2F + rr * Y2FR + fc) * 1024 + lane * 16) = o2[fc][rr];
        }
      }
      // dw1(it + 1) -> A1 (y1 rows Rn+2, Rn+3) and the residual of pooled row kn + 1 (x row Rn+2)
      if (hn) {
        const int lane = fresh(), p16 = lane & 15, q16 = lane >> 4;
        const uint8_t* base[U1W];
        int row[U1W];
#pragma unroll
        for (int i = 0; i < U1W; ++i) {
          int pi = 16 * ((w + NW * i) / KT0) + p16;
          pi = pi < 2 * Y1C ? pi : 2 * Y1C - 1;
          const int rr = pi >= Y1C, col = pi - rr * Y1C;
          row[i] = Rn + 2 + rr;
          base[i] = xr + (4 * t1 + (DWM ? q16 & 1 : q16)) * PLB + col * 16;
        }
        if constexpr (DWM) {
          // the y1 fragments are 16 of the two rows' linearised pixels, not a row each, so no row pairs: the
          // wave's two units (each lane its own pixel and row) share a group's weight operands instead
          static_assert(U1W == 2, "the wave's two dw1 units as one pair");
          const bool par = (lane & 32) != 0;
          const uint8_t* ad[U1W][5];
#pragma unroll
          for (int i = 0; i < U1W; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) {
              const int te = 2 * j, to = j < 4 ? 2 * j + 1 : 8;
              ad[i][j] = base[i] + (par ? ((row[i] - 1 + to / 3) & 3) * XROW + (to % 3) * 16
                                        : ((row[i] - 1 + te / 3) & 3) * XROW + (te % 3) * 16);
            }
          u32x2 dv[U1W][2];
#pragma unroll
          for (int g = 0; g < 2; ++g) {
            const u32x4 we = *(const u32x4*)((const uint8_t*)dwl + t1 * G::DWQ + ((g * 16 + p16) * 2 + (q16 >> 1)) * 16);
            u32x4 wk[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) wk[j] = eb_dw_wop(we, j, sel);
            u32x2 o[2];
            eb_dw_mfma_two<true>(ad[0], ad[1], 2 * g * PLB, [&](int j) { return wk[j]; }, o);
            dv[0][g] = o[0];
            dv[1][g] = o[1];
          }
#pragma unroll
          for (int i = 0; i < U1W; ++i) eb_dw_store(A1 + (t1 * Y1F + (w + NW * i) / KT0) * 1024, lane, dv[i]);
        } else {
          const uint32_t* wq = dwl + (t1 * 4 + q16) * 40;
          auto tap = [&](int i, int ti) {
            return *(const u32x4*)(base[i] + ((row[i] - 1 + ti / 3) & 3) * XROW + (ti % 3) * 16);
          };
          s16x8 o1[U1W];
          eb_dw8_n<true, U1W>(tap, wq, o1);
#pragma unroll
          for (int i = 0; i < U1W; ++i) *(s16x8*)(A1 + (t1 * Y1F + (w + NW * i) / KT0) * 1024 + lane * 16) = o1[i];
        }
        if (mn >= 1) {
          // the residual weights are fetched here, every step (8 KiB per wave, L2-resident; nothing else is
          // in flight: barrier B drained vmcnt), and live only for the eight MFMAs below. As residents (32
          // VGPRs) they pushed the allocation into scratch, and so did fetching them any earlier in the
          // phase (the allocator parked them in scratch across the depthwise; with the MFMA depthwise too:
          // 12 VGPRs spilled); a scratch reload in the GEMM phase waits, in vmcnt order, for the x-row DMA
          // issued ahead of it
          s16x8 wrs[NFW][KT0];
#pragma unroll
          for (int n = 0; n < NFW; ++n)
#pragma unroll
            for (int t = 0; t < KT0; ++t) wrs[n][t] = eb_frag(a.wr, NFW * w + n, KT0, t, lane);
          const int xrow = Rn + 2, xcol = 2 * p16 + 2;
#pragma unroll
          for (int n = 0; n < NFW; ++n) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT0; ++t)
              acc = mfma16(wrs[n][t], *(const s16x8*)(xr + (xrow & 3) * XROW + (4 * t + q16) * PLB + xcol * 16), acc);
            res2[n] = acc;
          }
        }
      }
      eb_lds_barrier();                              // A: A1, A2 complete; y1 pair (it + 1) & 1 and the x ring free
      if (it >= s0) stamp(it, 1);
      if (it + 2 < s1) dma_for(it + 2);
      // ---- GEMM phase. GEMM2(it) + bias -> bf16; vertical max with the carried row; horizontal max
      if (mc >= 1) {
        const int lane = fresh(), p16 = lane & 15, q16 = lane >> 4;
        const bool r0ok = (unsigned)R < (unsigned)H && mc == 2, r1ok = (unsigned)(R + 1) < (unsigned)H;
        const bool r2ok = (unsigned)(R + 2) < (unsigned)H;
        float4 bz1[NFW];
#pragma unroll
        for (int n = 0; n < NFW; ++n) bz1[n] = bias(1, n);
        u32x2 pv[NFW][Y2FR];                         // vertical maxima: lane (p16, q16) = column 16 fc + p16
#pragma unroll
        for (int fc = 0; fc < Y2FR; ++fc) {
          const s16x8* a0 = (const s16x8*)(A2 + fc * 1024 + lane * 16);
          const s16x8* a1 = (const s16x8*)(A2 + (Y2FR + fc) * 1024 + lane * 16);
          const int col = fc * 16 + p16, gcol = 2 * pc0 + col;
          const bool cok = col < Y2C && (unsigned)gcol < (unsigned)W;
#pragma unroll
          for (int n = 0; n < NFW; ++n) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT1; ++t) {
              acc0 = mfma16(w2[n][t], a0[t * Y2F * 64], acc0);
              acc1 = mfma16(w2[n][t], a1[t * Y2F * 64], acc1);
            }
            float vm[4];
            const float4 b4 = bz1[n];
            const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
            // bf16 rounding: the values an unfused separable conv would have stored
            const u32x2 y2a = {pack_bf16(acc0[0] + bb[0], acc0[1] + bb[1]), pack_bf16(acc0[2] + bb[2], acc0[3] + bb[3])};
            const u32x2 y2b = {pack_bf16(acc1[0] + bb[0], acc1[1] + bb[1]), pack_bf16(acc1[2] + bb[2], acc1[3] + bb[3])};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const uint32_t dc = carry[n][fc][e >> 1], da = y2a[e >> 1], db = y2b[e >> 1];
              const float c0 = (e & 1) ? bf_hi(dc) : bf_lo(dc);
              const float v1 = (e & 1) ? bf_hi(da) : bf_lo(da), v2 = (e & 1) ? bf_hi(db) : bf_lo(db);
              float m = r0ok ? c0 : -INFINITY;
              if (r1ok) m = fmaxf(m, v1);
              if (r2ok) m = fmaxf(m, v2);
              vm[e] = cok ? m : -INFINITY;
            }
            carry[n][fc] = y2b;
            pv[n][fc] = (u32x2){pack_bf16(vm[0], vm[1]), pack_bf16(vm[2], vm[3])};   // bf16: lossless here
          }
        }
        if (mc == 2) {
          // horizontal 3/2 max: pooled column j takes y2 local cols 2j .. 2j+2 of this wave's own two
          // fragments from lanes (col & 15, q16), every lane active (uniform branch): no LDS rows
          const int j = p16, gj = pc0 + j;
          u32x2 cc[NFW][3];
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            const int c = 2 * j + d, src = ((lane & 48) | (c & 15)) * 4;
#pragma unroll
            for (int n = 0; n < NFW; ++n)
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)pv[n][0][h]);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)pv[n][1][h]);
                cc[n][d][h] = c >= 16 ? hi : lo;
              }
          }
          if (j < PC && gj < a.OW) {
            // stored at once: GEMM1(it + 1) follows, so the store has the rest of the phase to retire
            // before barrier B's vmcnt(0) (the four-phase loop defers it past its next barrier)
            uint16_t* const yp = a.y + (((long)b * a.OH + k) * a.OW + gj) * a.ldy + PCH * w + 4 * q16;
#pragma unroll
            for (int n = 0; n < NFW; ++n) {
              const float4 brv = bias(2, n);
              const float br4[4] = {brv.x, brv.y, brv.z, brv.w};
              float o[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const uint32_t d0 = cc[n][0][e >> 1], d1 = cc[n][1][e >> 1], d2 = cc[n][2][e >> 1];
                const float m = (e & 1) ? fmaxf(fmaxf(bf_hi(d0), bf_hi(d1)), bf_hi(d2))
                                        : fmaxf(fmaxf(bf_lo(d0), bf_lo(d1)), bf_lo(d2));
                o[e] = m + bf2f(f2bf(res0[n][e] + br4[e]));
              }
              *(u32x2*)(yp + 16 * n) = (u32x2){pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
            }
          }
        }
      }
      // GEMM1(it + 1) (+ bias, ReLU) -> y1 ring rows Rn+2, Rn+3 (pair (it + 1) & 1)
      if (hn) {
        const int lane = fresh(), p16 = lane & 15, q16 = lane >> 4;
        float4 bz0[NFW];
#pragma unroll
        for (int n = 0; n < NFW; ++n) bz0[n] = bias(0, n);
#pragma unroll
        for (int f = 0; f < Y1F; ++f) {
          const s16x8* af = (const s16x8*)(A1 + f * 1024 + lane * 16);
          const int pi = 16 * f + p16;
          const int rr = pi >= Y1C, col = pi - rr * Y1C;
          const int row = Rn + 2 + rr, gcol = 2 * pcn - 1 + col;
          const bool ok = (unsigned)row < (unsigned)H && (unsigned)gcol < (unsigned)W;
#pragma unroll
          for (int n = 0; n < NFW; ++n) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT0; ++t) acc = mfma16(w1[n][t], af[t * Y1F * 64], acc);
            if (pi < 2 * Y1C) {
              const int c = PCH * w + 16 * n + 4 * q16;
              const float4 bv = bz0[n];
              const float v0 = fmaxf(acc[0] + bv.x, 0.f), v1 = fmaxf(acc[1] + bv.y, 0.f);
              const float v2 = fmaxf(acc[2] + bv.z, 0.f), v3 = fmaxf(acc[3] + bv.w, 0.f);
              const u32x2 o = ok ? (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)} : (u32x2){0u, 0u};
              *(u32x2*)(y1r + yslot(it + 1, 2 + rr) * Y1ROW + (c / 8) * PLB + col * 16 + (c & 7) * 2) = o;
            }
          }
        }
      }
#pragma unroll
      for (int n = 0; n < NFW; ++n) { res0[n] = res1[n]; res1[n] = res2[n]; }
      if (it >= s0) stamp(it, 2);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();                               // B: y1 rows written, A1 / A2 free, x rows of step it + 2 landed
    }
    return;
  }
  for (int q = s0; q < s1; ++q) {
    int b, s, k, mode;
    decode(q, b, s, k, mode);
    const int R = 2 * k;
    const int pc0 = s * PC;
    // the residual this step's output adds was computed in the previous step (x row 2k has left the ring
    // by now)
    f32x4 acco[NFW];
#pragma unroll
    for (int n = 0; n < NFW; ++n) acco[n] = accr[n];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                 // B0: x rows landed; previous step done

    stamp(q, 0);

    // ---- P1: depthwise 1 -> A (y1 rows R+2, R+3); residual operands: pooled row k+1 (x row 2k+2 = R+2;
    // x row 2k is no longer in the ring)
    {
      const uint32_t* wq = dwl + (t1 * 4 + q16) * 40;
#pragma unroll
      for (int i = 0; i < U1W; ++i) {
        const int u = w + NW * i;
        if (u < U1) {
          const int f = u / KT0;
          int pi = 16 * f + p16;
          pi = pi < 2 * Y1C ? pi : 2 * Y1C - 1;
          const int rr = pi >= Y1C, col = pi - rr * Y1C;
          const int row = R + 2 + rr;
          const uint8_t* base = xr + (4 * t1 + q16) * PLB + col * 16;
          auto tap = [&](int ti) {
            return *(const u32x4*)(base + ((row - 1 + ti / 3) & 3) * XROW + (ti % 3) * 16);
          };
          // stored at once (the deferred form spilled 67 VGPRs)
          *(s16x8*)(Ab + (t1 * Y1F + f) * 1024 + lane * 16) = eb_dw8<true>(tap, wq);
        }
      }
    }
    if (mode >= 1) {                                 // residual 1x1/2 conv of its pooled row
      const int xrow = R + 2, xcol = 2 * p16 + 2;
#pragma unroll
      for (int n = 0; n < NFW; ++n) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT0; ++t)
          acc = mfma16(wr[n][t], *(const s16x8*)(xr + (xrow & 3) * XROW + (4 * t + q16) * PLB + xcol * 16), acc);
        accr[n] = acc;
      }
    }
    eb_lds_barrier();                                // B1: A (y1) complete; x ring free for the next DMA
    stamp(q, 1);

    if (st_pend) {
#pragma unroll
      for (int n = 0; n < NFW; ++n) *(u32x2*)(st_ptr + 16 * n) = st_val[n];
      st_pend = false;
    }
    if (q + 1 < s1) dma_for(q + 1);

    // ---- P2: GEMM1 (+ bias, ReLU) -> y1 ring rows R+2, R+3; residual GEMM
    float4 bz0[NFW];                                 // read before the y1 stores
#pragma unroll
    for (int n = 0; n < NFW; ++n) bz0[n] = bias(0, n);
#pragma unroll
    for (int f = 0; f < Y1F; ++f) {
      const s16x8* af = (const s16x8*)(Ab + f * 1024 + lane * 16);
      const int pi = 16 * f + p16;
      const int rr = pi >= Y1C, col = pi - rr * Y1C;
      const int row = R + 2 + rr, gcol = 2 * pc0 - 1 + col;
      const bool ok = (unsigned)row < (unsigned)H && (unsigned)gcol < (unsigned)W;
#pragma unroll
      for (int n = 0; n < NFW; ++n) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT0; ++t) acc = mfma16(w1[n][t], af[t * Y1F * 64], acc);
        if (pi < 2 * Y1C) {
          const int c = PCH * w + 16 * n + 4 * q16;
          const float4 bv = bz0[n];
          const float v0 = fmaxf(acc[0] + bv.x, 0.f), v1 = fmaxf(acc[1] + bv.y, 0.f);
          const float v2 = fmaxf(acc[2] + bv.z, 0.f), v3 = fmaxf(acc[3] + bv.w, 0.f);
          const u32x2 o = ok ? (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)} : (u32x2){0u, 0u};
          *(u32x2*)(y1r + (row & 3) * Y1ROW + (c / 8) * PLB + col * 16 + (c & 7) * 2) = o;
        }
      }
    }
    eb_lds_barrier();                                // B2: y1 rows R+2, R+3 written; A free
    stamp(q, 2);

    if (mode == 0) continue;                         // warm-up 1: y1 only
    // ---- P3: depthwise 2 -> A (y2 rows R+1, R+2: fragments [row][col / 16])
    {
      const uint32_t* wq = dwl + ((KT0 + t2) * 4 + q16) * 40;
#pragma unroll
      for (int i = 0; i < U2W; ++i) {
        const int u = w + NW * i;
        if (u < U2) {
          const int f = u / KT1;
          const int rr = f / Y2FR, col = (f % Y2FR) * 16 + p16;
          const int row = R + 1 + rr;
          const uint8_t* base = y1r + (4 * t2 + q16) * PLB + col * 16;
          auto tap = [&](int ti) {
            return *(const u32x4*)(base + ((row - 1 + ti / 3) & 3) * Y1ROW + (ti % 3) * 16);
          };
          *(s16x8*)(Ab + (t2 * Y2F + f) * 1024 + lane * 16) = eb_dw8<false>(tap, wq);
        }
      }
    }
    eb_lds_barrier();                                // B3: A (y2) complete
    stamp(q, 3);

    // ---- P4: GEMM2 + bias -> bf16 values; vertical max with the carried row
    const bool r0ok = (unsigned)R < (unsigned)H && mode == 2, r1ok = (unsigned)(R + 1) < (unsigned)H;
    const bool r2ok = (unsigned)(R + 2) < (unsigned)H;
    float4 bz1[NFW];                                 // read before the pool stores
#pragma unroll
    for (int n = 0; n < NFW; ++n) bz1[n] = bias(1, n);
#pragma unroll
    for (int fc = 0; fc < Y2FR; ++fc) {
      const s16x8* a0 = (const s16x8*)(Ab + fc * 1024 + lane * 16);
      const s16x8* a1 = (const s16x8*)(Ab + (Y2FR + fc) * 1024 + lane * 16);
      const int col = fc * 16 + p16, gcol = 2 * pc0 + col;
      const bool cok = col < Y2C && (unsigned)gcol < (unsigned)W;
#pragma unroll
      for (int n = 0; n < NFW; ++n) {
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < KT1; ++t) {
          acc0 = mfma16(w2[n][t], a0[t * Y2F * 64], acc0);
          acc1 = mfma16(w2[n][t], a1[t * Y2F * 64], acc1);
        }
        float vm[4];
        const float4 b4 = bz1[n];
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
        // bf16 rounding: the values an unfused separable conv would have stored
        const u32x2 y2a = {pack_bf16(acc0[0] + bb[0], acc0[1] + bb[1]), pack_bf16(acc0[2] + bb[2], acc0[3] + bb[3])};
        const u32x2 y2b = {pack_bf16(acc1[0] + bb[0], acc1[1] + bb[1]), pack_bf16(acc1[2] + bb[2], acc1[3] + bb[3])};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t dc = carry[n][fc][e >> 1], da = y2a[e >> 1], db = y2b[e >> 1];
          const float c0 = (e & 1) ? bf_hi(dc) : bf_lo(dc);
          const float v1 = (e & 1) ? bf_hi(da) : bf_lo(da), v2 = (e & 1) ? bf_hi(db) : bf_lo(db);
          float m = r0ok ? c0 : -INFINITY;
          if (r1ok) m = fmaxf(m, v1);
          if (r2ok) m = fmaxf(m, v2);
          vm[e] = cok ? m : -INFINITY;
        }
        carry[n][fc] = y2b;
        if (mode == 2)                               // this wave's pool rows (bf16: lossless here)
          *(u32x2*)(pool + col * PCH + 16 * n + 4 * q16) = (u32x2){pack_bf16(vm[0], vm[1]), pack_bf16(vm[2], vm[3])};
      }
    }
    stamp(q, 4);
    if (mode == 1) continue;                         // warm-up 2: carry and residual only
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own pool rows only: no barrier
    // horizontal 3/2 max: pooled column j reads y2 local cols 2j .. 2j+2
    const int j = p16, gj = pc0 + j;
    if (j < PC && gj < a.OW) {
      st_ptr = a.y + (((long)b * a.OH + k) * a.OW + gj) * a.ldy + PCH * w + 4 * q16;
#pragma unroll
      for (int n = 0; n < NFW; ++n) {
        const uint16_t* pp = pool + (2 * j) * PCH + 16 * n + 4 * q16;
        const float4 brv = bias(2, n);
        const float br4[4] = {brv.x, brv.y, brv.z, brv.w};
        const u32x2 c0 = *(const u32x2*)pp, c1 = *(const u32x2*)(pp + PCH), c2 = *(const u32x2*)(pp + 2 * PCH);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const uint32_t d0 = c0[e >> 1], d1 = c1[e >> 1], d2 = c2[e >> 1];
          const float m = (e & 1) ? fmaxf(fmaxf(bf_hi(d0), bf_hi(d1)), bf_hi(d2))
                                  : fmaxf(fmaxf(bf_lo(d0), bf_lo(d1)), bf_lo(d2));
          o[e] = m + bf2f(f2bf(acco[n][e] + br4[e]));
        }
        st_val[n] = (u32x2){pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
      }
      st_pend = true;
    }
  }
  if (st_pend) {
#pragma unroll
    for (int n = 0; n < NFW; ++n) *(u32x2*)(st_ptr + 16 * n) = st_val[n];
  }
}

// ===================================================================================================
// Warp-specialized entry block (configs 13 / 113: block2, NWAV = 16). The four dependent stages of a
// step (dw1 -> GEMM1 -> dw2 -> GEMM2 + pool) are split between two wave roles that work on DIFFERENT
// steps at the same time, one workgroup barrier per step:
//   producers (waves NWAV/2..)  iteration i:  dw1(i) -> A1[i&1]   dw2(i-2) -> A2[i&1]   (MFMA depthwise)
//                                             + the x-row DMA of step i+1, + step i's residual input row
//   consumers (waves 0..NWAV/2-1) iteration i: GEMM1(i-1) <- A1 -> y1 ring   GEMM2(i-3) <- A2 + pool
//                                             + residual 1x1/2 GEMM + output of step i-3
// Waves w and w+4 share a SIMD (MI355X_MICROARCH.md: cyclic wave placement), so every SIMD pairs
// depthwise streams with GEMM streams instead of running the phases one after another with every wave
// in the same phase (the round-4 kernel: four barriers per step, ~2k cycles per phase, all of them
// LDS-throughput bound -- profiles/entry_block_ab_r4.txt). Rings: x 8 rows (each step's DMA one
// iteration ahead), y1 6 rows (GEMM1(i-1) writes rows R+4, R+5 of step i-2 while dw2(i-2) reads its
// rows R..R+3; slots counted by steps, see yslot), A1 / A2 double-buffered, residual rows in a 4-slot
// buffer (written by producers at step i, read by consumers three iterations later). 13-column strips
// keep the map at 142 KiB
// (pitch 32 px, no padding). A consumer wave owns 32 output channels of every GEMM (register-resident
// weights); a producer wave owns a quarter of each step's depthwise units.
template <int C0_, int C1_, int PC_, int NWAV_, int NCW>
struct EbwGeom {
  static constexpr int C0 = C0_, C1 = C1_, PC = PC_, NWAV = NWAV_;
  static constexpr int Y2C = 2 * PC + 1, Y1C = Y2C + 2, XC = Y1C + 2;
  static constexpr int PLP = (XC + 15) / 16 * 16, PLB = PLP * 16;
  static constexpr int XROW = (C0 / 8) * PLB, Y1ROW = (C1 / 8) * PLB;
  static constexpr int KT0 = C0 / 32, KT1 = C1 / 32;
  static constexpr int Y1F = (2 * Y1C + 15) / 16, Y2FR = (Y2C + 15) / 16, Y2F = 2 * Y2FR;
  static constexpr int Y1FR = (Y1C + 15) / 16;       // row-pair builds: y1 fragments are [row][col / 16] too
  static constexpr int NC = NCW, NP = NWAV - NCW;  // consumer / producer waves (w, w+4, ... share a SIMD)
  static constexpr int CCH = C1 / NC;                // output channels per consumer wave
  static constexpr int NSL = CCH / 16;               // 16-channel slices per consumer wave
  static constexpr int XDMA = XROW / 1024;
  static constexpr int XR = 8, YR = 6, RS = 4;       // x ring, y1 ring, residual slots
  static constexpr int PCOLS = 16 * Y2FR;
  static constexpr int A1B = KT0 * Y1F * 1024, A2B = KT1 * Y2F * 1024;
  static constexpr int RESB = 16 * C0 * 2;           // one residual input row: 16 strided columns x C0
  static constexpr int BYTES = XR * XROW + YR * Y1ROW + 2 * A1B + 2 * A2B + RS * RESB + NC * PCOLS * CCH * 2 +
                               (KT0 + KT1) * 1024 + 4 * EB_MAX_STEPS;
  static_assert(XROW % 1024 == 0 && RESB % 1024 == 0 && C0 % 32 == 0 && C1 % 64 == 0, "channel tiling");
  static_assert(NP % KT0 == 0 && NP % KT1 == 0, "a producer's depthwise units share one k-step");
  static_assert(BYTES <= 160 * 1024, "LDS");
};

// CDW: dw2 units per step that every consumer wave computes too (the consumers idle half of an
// iteration while the producers' depthwise is the critical path); the producers keep the rest
// RP: row-pair depthwise (eb_dw_mfma_rowpair). A step's two y1 rows and its two y2 rows are adjacent,
// so the work is dealt out as (column fragment, channel group, k-step) items that produce both rows
// with one set of weight operands: 2 Y1FR KT0 = 8 items for dw1 (its fragments become [row][col / 16],
// with the same 6 wasted pixels as the 58 linearised ones) and 2 Y2FR KT1 = 16 for dw2. A wave's items
// share k-step and channel group, so the producers build their weight operands once per kernel: the
// operand perms were a third of the producers' VALU instructions, and the SIMDs' VALU issue, not the
// LDS, bounds an iteration (10 VALU per MFMA in config 15; profiles/entry_block_rowpair.txt).
// Block2 (odd maps: the leading pad PT of the TF-'same' 3x3/2 pool is 1, so the residual row 2k is x row R+1 of
// the step; no ReLU on the block input). STAMP: the diagnostics build
using Eb2Geom = EbwGeom<64, 128, 13, 16, 8>;
template <bool STAMP, int CDW, bool RP>
__global__ __launch_bounds__(64 * Eb2Geom::NWAV, Eb2Geom::NWAV / 4) void entry_block_ws_kernel(EntryBlockArgs a) {
  using G = Eb2Geom;
  constexpr int C0 = G::C0, PC = G::PC, NWAV = G::NWAV, PT = 1;
  constexpr int KT0 = G::KT0, KT1 = G::KT1, PLB = G::PLB, XROW = G::XROW, Y1ROW = G::Y1ROW, XDMA = G::XDMA;
  constexpr int Y1C = G::Y1C, Y2C = G::Y2C, XC = G::XC, PLP = G::PLP;
  constexpr int Y1F = G::Y1F, Y2F = G::Y2F, Y2FR = G::Y2FR, PCOLS = G::PCOLS;
  constexpr int XR = G::XR, YR = G::YR, RS = G::RS, NC = G::NC, NP = G::NP, CCH = G::CCH, NSL = G::NSL;
  constexpr int U1 = KT0 * Y1F, U2 = KT1 * Y2F;
  constexpr int CU2 = CDW * NC;                      // dw2 units 0..CU2-1: consumers (units w + NC j); the rest: producers
  static_assert(CU2 % KT1 == 0 && CU2 <= U2, "consumer dw2 units keep the producers' k-step per wave");
  constexpr int U1W = (U1 + NP - 1) / NP, U2W = (U2 - CU2 + NP - 1) / NP;
  constexpr int Y1FR = G::Y1FR;
  static_assert(!RP || (2 * Y1FR == Y1F && NP % (2 * KT0) == 0 && NP % (2 * KT1) == 0 && NC % (2 * KT1) == 0 &&
                        CU2 % (2 * KT1) == 0),
                "row-pair items of a wave share one k-step and one channel group; y1 fragments [row][col / 16]");
  // distinct LDS objects: the compiler may reorder accesses of different regions
  __shared__ __attribute__((aligned(16))) uint8_t s_x[XR * XROW];
  __shared__ __attribute__((aligned(16))) uint8_t s_y1[YR * Y1ROW];
  __shared__ __attribute__((aligned(16))) uint8_t s_a1[2 * G::A1B];
  __shared__ __attribute__((aligned(16))) uint8_t s_a2[2 * G::A2B];
  __shared__ __attribute__((aligned(16))) uint8_t s_res[RS * G::RESB];
  __shared__ __attribute__((aligned(16))) uint16_t s_pool[NC * PCOLS * CCH];
  __shared__ __attribute__((aligned(16))) uint8_t s_dw[(KT0 + KT1) * 1024];
  __shared__ uint32_t s_st[EB_MAX_STEPS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool consumer = w < NC;
  const int q16 = lane >> 4, p16 = lane & 15;
  const int H = a.H, W = a.W;
  const int s0 = a.step_off[blockIdx.x], s1 = a.step_off[blockIdx.x + 1];
  if (s0 >= s1 || s1 - s0 > EB_MAX_STEPS) return;

  for (int i = tid; i < s1 - s0; i += 64 * NWAV) {
    const int4 e = a.steps[s0 + i];
    s_st[i] = (uint32_t)e.x | ((uint32_t)e.y << 8) | ((uint32_t)(e.z + 2) << 14) | ((uint32_t)e.w << 23);
  }
  for (int i = tid; i < (KT0 + KT1) * 64; i += 64 * NWAV) {
    const int t = i / 64;
    const u32x4 v = t < KT0 ? *(const u32x4*)((const uint8_t*)a.dwk1 + t * 1024 + (i % 64) * 16)
                            : *(const u32x4*)((const uint8_t*)a.dwk2 + (t - KT0) * 1024 + (i % 64) * 16);
    *(u32x4*)(s_dw + t * 1024 + (i % 64) * 16) = v;
  }
  uint32_t sel[2][4];
  {
    const bool wv = (p16 >> 3) == (q16 & 1);
    const int e = p16 & 7;
#pragma unroll
    for (int jp = 0; jp < 2; ++jp)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t pair = (2u * jp) | ((2u * jp + 1u) << 8);
        const uint32_t val = (e & 1) ? (0x0c0cu | (pair << 16)) : (0x0c0c0000u | pair);
        sel[jp][d] = (wv && (e >> 1) == d) ? val : 0x0c0c0c0cu;
      }
  }
  __syncthreads();
  if (tid == 0) {                                    // ring slot of each step's first x row (rows R+1..R+4)
    int xp = 0, xs = 0;
    for (int i = 0; i < s1 - s0; ++i) {
      const uint32_t e = s_st[i];
      if (((e >> 23) & 3) == 0) { xs = xp; xp += 4; } else { xs += 2; xp += 2; }
      s_st[i] = e | ((uint32_t)(xs & (XR - 1)) << 25);
    }
  }
  EbStepRegs str;                                    // loaded once the ring-slot bits are in (below)
  auto decode = [&](int q, int& b, int& s, int& k, int& mode, int& xs) {
    const uint32_t e = str.get(q - s0);
    b = e & 255; s = (e >> 8) & 63; k = (int)((e >> 14) & 511) - 2; mode = (e >> 23) & 3; xs = (e >> 25) & 7;
  };
  auto dma_for = [&](int q) {                        // producers only: step q's new x rows
    int b, s, k, mode, xs;
    decode(q, b, s, k, mode, xs);
    const int R = 2 * k - PT, gx0 = 2 * s * PC - PT - 2;
    const int r0 = mode == 0 ? R + 1 : R + 3, nr = mode == 0 ? 4 : 2, sl0 = mode == 0 ? xs : xs + 2;
    for (int ii = w - NC; ii < nr * XDMA; ii += NP) {
      const int r = r0 + ii / XDMA, d = ii % XDMA;
      const int slot = d * 64 + lane, plane = slot / PLP, px = slot - plane * PLP;
      const int gx = gx0 + px;
      const bool ok = px < XC && (unsigned)r < (unsigned)H && (unsigned)gx < (unsigned)W;
      const uint8_t* src = ok ? (const uint8_t*)(a.x + (((long)b * H + r) * W + gx) * a.ldx + plane * 8) : eb_zeros;
      glds16_asm(src, s_x + ((sl0 + ii / XDMA) & (XR - 1)) * XROW + d * 1024);
    }
  };
  // y1 ring slot of row R + d (d = 0..5) of step q, R = the step's first y2 input row. Counted by STEPS, not
  // by rows: inside a run both advance by two per step, but where a run follows another in the same
  // workgroup, GEMM1 of the new run's first step runs in the iteration in which dw2 still reads the old
  // run's last rows, and row numbers of different runs can share a slot (they do not for a 147-row map,
  // where the shared slots hold rows past the bottom edge: zeros, overwritten by zeros)
  auto yslot = [&](int q, int d) { return (2 * (q - s0) + d) % YR; };
  auto stamp = [&](int it, int ph) {
    if constexpr (STAMP) {
      if (lane == 0 && (w == 0 || w == NC) && blockIdx.x < 8 && it - s0 < 64 && a.stamps)
        a.stamps[((long)blockIdx.x * 64 + (it - s0)) * 5 + ph] = __builtin_amdgcn_s_memtime();
    }
  };

  __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (15 << 8));   // prologue loads landed (the waitcnt pass sees it)
  eb_lds_barrier();                                  // ring-slot bits of the step words visible
  str.load(s_st, s1 - s0, lane);

  // The two roles run separate loops with the same trip count and one barrier per iteration (s_barrier
  // counts arrivals, not program counters): each role's registers are live in its own loop only, so
  // the consumers' register-resident weights do not sit in the producers' allocation (and the reverse)
  // RP: the 16-B weight entry of item (k-step tq, group g) for this lane's channel and tap parity
  auto rp_ent = [&](int tq, int g) {
    return *(const u32x4*)(s_dw + tq * 1024 + ((g * 16 + p16) * 2 + (q16 >> 1)) * 16);
  };
  if (!consumer) {
    // RP: a producer's items keep (k-step, group), so the weight operands of its dw1 and dw2 items stay
    // in registers for the whole kernel: 2 x 5 x 4 VGPRs (the producers have them to spare) instead of
    // 20 perms per single-row unit in every iteration
    u32x4 wk1[RP ? 5 : 1], wk2[RP ? 5 : 1];
    if constexpr (RP) {
      const u32x4 e1 = rp_ent((w - NC) % KT0, ((w - NC) / KT0) & 1);
      const u32x4 e2 = rp_ent(KT0 + (w - NC) % KT1, ((w - NC) / KT1) & 1);
#pragma unroll
      for (int j = 0; j < 5; ++j) { wk1[j] = eb_dw_wop(e1, j, sel); wk2[j] = eb_dw_wop(e2, j, sel); }
    }
    dma_for(s0);
    for (int it = s0; it < s1 + 3; ++it) {
      // step `it`'s x rows (their DMA, issued last iteration) must have landed
      __builtin_amdgcn_s_waitcnt(0 | (7 << 4) | (0 << 8));
      eb_lds_barrier();
      stamp(it, 2);
      // =================================================================== producers
      const int pw = w - NC;
      if (it + 1 < s1) dma_for(it + 1);
      u32x2 dv1[U1W][2], dv2[U2W > 0 ? U2W : 1][2];
      uint8_t* d1[U1W];
      uint8_t* d2[U2W > 0 ? U2W : 1];
#pragma unroll
      for (int i = 0; i < U1W; ++i) d1[i] = nullptr;
#pragma unroll
      for (int i = 0; i < U2W; ++i) d2[i] = nullptr;
      if (it < s1) {                                 // dw1(it) -> A1[it & 1]; residual input row of step it
        int b, s, k, mode, xs;
        decode(it, b, s, k, mode, xs);
        const int t1 = pw % KT0;
        uint8_t* const A1 = s_a1 + (it & 1) * G::A1B;
#pragma unroll
        for (int i = 0; i < U1W; ++i) {
          const int u = pw + NP * i;
          if constexpr (RP) {
            if (u < U1) {                            // item (column fragment cf, group g1, k-step t1): rows R+2, R+3
              const int g1 = (pw / KT0) & 1, cf = u / (2 * KT0);
              const int col = min(cf * 16 + p16, Y1C - 1);
              const uint8_t* base = s_x + (4 * t1 + 2 * g1 + (q16 & 1)) * PLB + col * 16;
              auto addr = [&](int ti) { return base + ((xs + ti / 3) & (XR - 1)) * XROW + (ti % 3) * 16; };
              eb_dw_mfma_rowpair(addr, [&](int j) { return wk1[j]; }, lane, dv1[i]);
              d1[i] = A1 + (t1 * Y1F + cf) * 1024;
            }
          } else
          if (u < U1) {
            const int f = u / KT0;
            int pi = 16 * f + p16;
            pi = pi < 2 * Y1C ? pi : 2 * Y1C - 1;
            const int rr = pi >= Y1C, col = pi - rr * Y1C;
            const uint8_t* base = s_x + (4 * t1 + (q16 & 1)) * PLB + col * 16;
            auto tap = [&](int g, int ti) {
              return *(const u32x4*)(base + 2 * g * PLB + ((xs + rr + ti / 3) & (XR - 1)) * XROW + (ti % 3) * 16);
            };
            auto ent = [&](int g) {
              return *(const u32x4*)(s_dw + t1 * 1024 + (((g * 16 + p16) * 2) + (q16 >> 1)) * 16);
            };
            eb_dw_mfma_vals(tap, ent, lane, sel, dv1[i]);
            d1[i] = A1 + (t1 * Y1F + f) * 1024;
          }
        }
        if (mode == 2) {                             // x row 2k = R + 1 (slot xs), 16 strided columns, C0 channels
          uint8_t* const rs = s_res + (it & (RS - 1)) * G::RESB;
          const int xcol = min(2 * p16 + PT + 2, XC - 1);   // lanes p16 >= PC: unused columns (clamped)
          for (int c = q16 + 4 * pw; c < C0 / 8; c += 4 * NP)   // 16-B chunk c of every column
            *(u32x4*)(rs + (c * 16 + p16) * 16) = *(const u32x4*)(s_x + xs * XROW + c * PLB + xcol * 16);
        }
      }
      if (it - 2 >= s0 && it - 2 < s1) {            // dw2(it - 2) -> A2[it & 1]
        int b, s, k, mode, xs;
        decode(it - 2, b, s, k, mode, xs);
        if (mode >= 1) {
          const int t2 = pw % KT1;
          uint8_t* const A2 = s_a2 + (it & 1) * G::A2B;
#pragma unroll
          for (int i = 0; i < U2W; ++i) {
            const int u = CU2 + pw + NP * i;
            if constexpr (RP) {
              if (u < U2) {                          // item (cf, g2, t2): y2 rows R+1, R+2 from y1 rows R..R+3
                const int g2 = (pw / KT1) & 1, cf = u / (2 * KT1);
                const uint8_t* base = s_y1 + (4 * t2 + 2 * g2 + (q16 & 1)) * PLB + (cf * 16 + p16) * 16;
                auto addr = [&](int ti) { return base + yslot(it - 2, ti / 3) * Y1ROW + (ti % 3) * 16; };
                eb_dw_mfma_rowpair(addr, [&](int j) { return wk2[j]; }, lane, dv2[i]);
                d2[i] = A2 + (t2 * Y2F + cf) * 1024;
              }
            } else
            if (u < U2) {
              const int f = u / KT1;
              const int rr = f / Y2FR, col = (f % Y2FR) * 16 + p16;
              const uint8_t* base = s_y1 + (4 * t2 + (q16 & 1)) * PLB + col * 16;
              auto tap = [&](int g, int ti) {
                return *(const u32x4*)(base + 2 * g * PLB + yslot(it - 2, rr + ti / 3) * Y1ROW + (ti % 3) * 16);
              };
              auto ent = [&](int g) {
                return *(const u32x4*)(s_dw + (KT0 + t2) * 1024 + (((g * 16 + p16) * 2) + (q16 >> 1)) * 16);
              };
              eb_dw_mfma_vals(tap, ent, lane, sel, dv2[i]);
              d2[i] = A2 + (t2 * Y2F + f) * 1024;
            }
          }
        }
      }
      if constexpr (RP) {                            // dv[row]: the row r+1 fragment lies a fragment row further
#pragma unroll
        for (int i = 0; i < U1W; ++i)
          if (d1[i]) {
            eb_dw_store_g(d1[i], lane, (pw / KT0) & 1, dv1[i][0]);
            eb_dw_store_g(d1[i] + Y1FR * 1024, lane, (pw / KT0) & 1, dv1[i][1]);
          }
#pragma unroll
        for (int i = 0; i < U2W; ++i)
          if (d2[i]) {
            eb_dw_store_g(d2[i], lane, (pw / KT1) & 1, dv2[i][0]);
            eb_dw_store_g(d2[i] + Y2FR * 1024, lane, (pw / KT1) & 1, dv2[i][1]);
          }
      } else {
#pragma unroll
        for (int i = 0; i < U1W; ++i)
          if (d1[i]) eb_dw_store(d1[i], lane, dv1[i]);
#pragma unroll
        for (int i = 0; i < U2W; ++i)
          if (d2[i]) eb_dw_store(d2[i], lane, dv2[i]);
      }
      stamp(it, 3);
    }
  } else {
    // consumers: this wave's CCH output channels of every GEMM, register-resident
    s16x8 w1[NSL][KT0], w2[NSL][KT1], wr[NSL][KT0];
    float4 bz[3][NSL];
#pragma unroll
    for (int n = 0; n < NSL; ++n) {
#pragma unroll
      for (int t = 0; t < KT0; ++t) {
        w1[n][t] = eb_frag(a.w1, NSL * w + n, KT0, t, lane);
        wr[n][t] = eb_frag(a.wr, NSL * w + n, KT0, t, lane);
      }
#pragma unroll
      for (int t = 0; t < KT1; ++t) w2[n][t] = eb_frag(a.w2, NSL * w + n, KT1, t, lane);
#pragma unroll
      for (int g = 0; g < 3; ++g)
        bz[g][n] = *(const float4*)((g == 0 ? a.b1 : g == 1 ? a.b2 : a.br) + CCH * w + 16 * n + 4 * q16);
    }
    u32x2 carry[NSL][Y2FR];                          // y2 row R+2 of the previous step
    for (int it = s0; it < s1 + 3; ++it) {
      eb_lds_barrier();                              // (no VMEM to wait for: the weights' waits are the compiler's)
      stamp(it, 0);
      if constexpr (CDW > 0) {                       // dw2(it - 2), units w + NC j -> A2[it & 1] (read after the next barrier)
        if (it - 2 >= s0 && it - 2 < s1) {
          int b, s, k, mode, xs;
          decode(it - 2, b, s, k, mode, xs);
          if (mode >= 1) {
            const int t2 = w % KT1;
            auto unit = [&](int u) {
              const int f = u / KT1;
              const int rr = f / Y2FR, col = (f % Y2FR) * 16 + p16;
              const uint8_t* base = s_y1 + (4 * t2 + (q16 & 1)) * PLB + col * 16;
              auto tap = [&](int g, int ti) {
                return *(const u32x4*)(base + 2 * g * PLB + yslot(it - 2, rr + ti / 3) * Y1ROW + (ti % 3) * 16);
              };
              auto ent = [&](int g) {
                return *(const u32x4*)(s_dw + (KT0 + t2) * 1024 + (((g * 16 + p16) * 2) + (q16 >> 1)) * 16);
              };
              u32x2 dv[2];
              eb_dw_mfma_vals(tap, ent, lane, sel, dv);
              eb_dw_store(s_a2 + (it & 1) * G::A2B + (t2 * Y2F + f) * 1024, lane, dv);
            };
            auto item = [&](int u) {                 // RP: item (cf, g2, t2), both rows
              const int g2 = (w / KT1) & 1, cf = u / (2 * KT1);
              const uint8_t* base = s_y1 + (4 * t2 + 2 * g2 + (q16 & 1)) * PLB + (cf * 16 + p16) * 16;
              auto addr = [&](int ti) { return base + yslot(it - 2, ti / 3) * Y1ROW + (ti % 3) * 16; };
              const u32x4 e = rp_ent(KT0 + t2, g2);
              u32x2 dv[2];
              eb_dw_mfma_rowpair(addr, [&](int j) { return eb_dw_wop(e, j, sel); }, lane, dv);
              uint8_t* const dst = s_a2 + (it & 1) * G::A2B + (t2 * Y2F + cf) * 1024;
              eb_dw_store_g(dst, lane, g2, dv[0]);
              eb_dw_store_g(dst + Y2FR * 1024, lane, g2, dv[1]);
            };
            if constexpr (RP) {
              item(w);
              if constexpr (CDW > 1) item(w + NC);
            } else {
              unit(w);
              if constexpr (CDW > 1) unit(w + NC);
            }
          }
        }
      }
      // =================================================================== consumers
      if (it - 1 >= s0 && it - 1 < s1) {             // GEMM1(it - 1) <- A1[(it - 1) & 1] -> y1 ring
        int b, s, k, mode, xs;
        decode(it - 1, b, s, k, mode, xs);
        const int R = 2 * k - PT, pc0 = s * PC;
        const uint8_t* const A1 = s_a1 + ((it - 1) & 1) * G::A1B;
#pragma unroll
        for (int f = 0; f < Y1F; ++f) {
          // fragment f: 16 of the two rows' 2 Y1C linearised pixels, or (RP) columns 16 (f % Y1FR).. of row f / Y1FR
          const int pi = RP ? (f % Y1FR) * 16 + p16 : 16 * f + p16;
          const int rr = RP ? f / Y1FR : pi >= Y1C, col = RP ? pi : pi - rr * Y1C;
          const bool live = pi < (RP ? Y1C : 2 * Y1C);
          const int row = R + 2 + rr, gcol = 2 * pc0 - PT - 1 + col;
          const bool ok = (unsigned)row < (unsigned)H && (unsigned)gcol < (unsigned)W;
          s16x8 af[KT0];
#pragma unroll
          for (int t = 0; t < KT0; ++t) af[t] = *(const s16x8*)(A1 + (t * Y1F + f) * 1024 + lane * 16);
#pragma unroll
          for (int n = 0; n < NSL; ++n) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < KT0; ++t) acc = mfma16(w1[n][t], af[t], acc);
            if (live) {
              const int c = CCH * w + 16 * n + 4 * q16;
              const float4 bv = bz[0][n];
              const float v0 = fmaxf(acc[0] + bv.x, 0.f), v1 = fmaxf(acc[1] + bv.y, 0.f);
              const float v2 = fmaxf(acc[2] + bv.z, 0.f), v3 = fmaxf(acc[3] + bv.w, 0.f);
              const u32x2 o = ok ? (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)} : (u32x2){0u, 0u};
              *(u32x2*)(s_y1 + yslot(it - 1, 2 + rr) * Y1ROW + (c / 8) * PLB + col * 16 + (c & 7) * 2) = o;
            }
          }
        }
      }
      if (it - 3 >= s0 && it - 3 < s1) {             // GEMM2(it - 3) <- A2[(it - 1) & 1] + pool + residual
        int b, s, k, mode, xs;
        decode(it - 3, b, s, k, mode, xs);
        if (mode >= 1) {
          const int R = 2 * k - PT, pc0 = s * PC;
          const uint8_t* const A2 = s_a2 + ((it - 1) & 1) * G::A2B;
          uint16_t* const pool = s_pool + w * (PCOLS * CCH);
          const bool r0ok = (unsigned)R < (unsigned)H && mode == 2, r1ok = (unsigned)(R + 1) < (unsigned)H;
          const bool r2ok = (unsigned)(R + 2) < (unsigned)H;
#pragma unroll
          for (int fc = 0; fc < Y2FR; ++fc) {
            const int col = fc * 16 + p16, gcol = 2 * pc0 - PT + col;
            const bool cok = col < Y2C && (unsigned)gcol < (unsigned)W;
            s16x8 a0[KT1], a1f[KT1];
#pragma unroll
            for (int t = 0; t < KT1; ++t) {
              a0[t] = *(const s16x8*)(A2 + (t * Y2F + fc) * 1024 + lane * 16);
              a1f[t] = *(const s16x8*)(A2 + (t * Y2F + Y2FR + fc) * 1024 + lane * 16);
            }
#pragma unroll
            for (int n = 0; n < NSL; ++n) {
              f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int t = 0; t < KT1; ++t) {
                acc0 = mfma16(w2[n][t], a0[t], acc0);
                acc1 = mfma16(w2[n][t], a1f[t], acc1);
              }
              const float4 b4 = bz[1][n];
              const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
              const u32x2 y2a = {pack_bf16(acc0[0] + bb[0], acc0[1] + bb[1]), pack_bf16(acc0[2] + bb[2], acc0[3] + bb[3])};
              const u32x2 y2b = {pack_bf16(acc1[0] + bb[0], acc1[1] + bb[1]), pack_bf16(acc1[2] + bb[2], acc1[3] + bb[3])};
              float vm[4];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const uint32_t dc = carry[n][fc][e >> 1], da = y2a[e >> 1], db = y2b[e >> 1];
                const float c0 = (e & 1) ? bf_hi(dc) : bf_lo(dc);
                const float v1 = (e & 1) ? bf_hi(da) : bf_lo(da), v2 = (e & 1) ? bf_hi(db) : bf_lo(db);
                float m = r0ok ? c0 : -INFINITY;
                if (r1ok) m = fmaxf(m, v1);
                if (r2ok) m = fmaxf(m, v2);
                vm[e] = cok ? m : -INFINITY;
              }
              carry[n][fc] = y2b;
              if (mode == 2)
                *(u32x2*)(pool + col * CCH + 16 * n + 4 * q16) = (u32x2){pack_bf16(vm[0], vm[1]), pack_bf16(vm[2], vm[3])};
            }
          }
          if (mode == 2) {
            // residual 1x1/2 conv of pooled row k from the staged input row (written three iterations ago)
            const uint8_t* const rs = s_res + ((it - 3) & (RS - 1)) * G::RESB;
            f32x4 racc[NSL];
#pragma unroll
            for (int n = 0; n < NSL; ++n) {
              racc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int t = 0; t < KT0; ++t)
                racc[n] = mfma16(wr[n][t], *(const s16x8*)(rs + ((4 * t + q16) * 16 + p16) * 16), racc[n]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // own pool rows only
            const int j = p16, gj = pc0 + j;
            if (j < PC && gj < a.OW) {
#pragma unroll
              for (int n = 0; n < NSL; ++n) {
                const uint16_t* pp = pool + (2 * j) * CCH + 16 * n + 4 * q16;
                const float4 brv = bz[2][n];
                const float br4[4] = {brv.x, brv.y, brv.z, brv.w};
                const u32x2 c0 = *(const u32x2*)pp, c1 = *(const u32x2*)(pp + CCH), c2 = *(const u32x2*)(pp + 2 * CCH);
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                  const uint32_t d0 = c0[e >> 1], d1v = c1[e >> 1], d2v = c2[e >> 1];
                  const float m = (e & 1) ? fmaxf(fmaxf(bf_hi(d0), bf_hi(d1v)), bf_hi(d2v))
                                          : fmaxf(fmaxf(bf_lo(d0), bf_lo(d1v)), bf_lo(d2v));
                  o[e] = m + bf2f(f2bf(racc[n][e] + br4[e]));
                }
                *(u32x2*)(a.y + (((long)b * a.OH + k) * a.OW + gj) * a.ldy + CCH * w + 16 * n + 4 * q16) =
                    (u32x2){pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3])};
              }
            }
          }
        }
      }
      stamp(it, 1);
    }
  }
}

// Kernel configurations (the ids of EntryBlock(cfg=...) and KDL_ENTRY_BLOCK=block:id); 100 + id: the same
// build with s_memtime stamps (EntryBlockArgs.stamps; diagnostics only, tools/ebbench.py --stamps). Block2
// (147x147x64 -> 74x74x128, leading pool pad 1) runs on entry_block_ws_kernel: 15, 17, 19; block3
// (74x74x128 -> 37x37x256, the asymmetric 74 -> 37 pool: leading pad 0) on entry_block_kernel: 1, 21, 23.
// The engine launches 17 and 23; 15, 19, 1 and 21 are the predecessors their bit-equality tests compare
// against (tests/test_entry_block_rowpair_gpu.py, tests/test_entry_block3_twophase_gpu.py,
// tests/test_entry_block3_dwm_gpu.py). Any other id is refused.
// 1 / 101: block3 on the four-phase loop, two slices per wave, VALU depthwise (the four-phase LDS map has no
// room for the MFMA entries; the two-phase map has: config 23). Measured and removed (round 5,
// profiles/entry_block3_r5.txt): block3 as 16 waves of one slice (VALU / MFMA depthwise: 328 / 246 us)
// and block3 with the MFMA depthwise (378 us) against config 1's 188 us -- all spill (78 / 56 / 91 VGPRs)
// 15 / 115: the warp-specialized kernel with single-row depthwise units, every consumer wave also
// computing one of the step's 16 dw2 units (CDW = 1; against the retired 13 without them): 191.8 vs
// 199.2 us, iteration 7,212 -> 6,636 cycles (consumers busy 4,700,
// producers 5,572), bench +1.0 % in 3 of 3 pairs. Measured and removed (profiles/entry_block_ab_r4.txt):
// 4 consumer + 12 producer waves (227.0 us: the 32-channel consumers spill 32 VGPRs), two dw2 units per
// consumer (215.8 us: consumers 6,168 busy with 14 VGPRs spilled), and the residual-row copy moved to the
// consumers as well (iteration 6,732 vs 6,676, bench -0.2 %).
// 17 / 117 (block2's default), 19 / 119: CDW 0 / 1 with the row-pair depthwise (RP): a step's two
// rows per item, the producers' weight operands built once per kernel. Bit-identical to config 15
// (tests/test_entry_block_rowpair_gpu.py; the bench logits equal the parent build's). One lease
// (profiles/entry_block_rowpair.txt): config 15 iteration 6,440 cycles (producers 5,364, consumers 4,522),
// 17: 5,324 (4,770 / 3,544), 19: 5,652 (4,220 / 4,456); in the step 191.2 -> 163.4 us, VALU per MFMA
// 9.9 -> 7.1; bench +2.4 % in 12 of 12 interleaved pairs (A spread 0.64 %). The consumers' dw2 item of
// config 19 no longer pays: it rebuilds its operands every iteration (no registers to keep them) on
// SIMDs whose VALU issue is the limit. Measured and removed: sharing the tap READS between the two rows
// (7 reads with row r+1's k-halves exchanged: iteration 6,176, but the MFMA sum depends on the half a
// product sits in -- block outputs equal on small maps, bench logits off by 7.6e-3; 8 reads with
// v_permlane32_swap: bit-identical, iteration 6,472: 24 swaps / selects + 16 copies per item cost more
// than two reads), and block3 (VALU depthwise) was not changed: see the same file.
// 21 / 121: config 1 on the two-phase schedule (TWOPH, see the loop's comment). Bit-identical
// to config 1 (tests/test_entry_block3_twophase_gpu.py; the bench logits equal the parent build's). One lease
// (profiles/entry_block3_twophase.txt): 185 -> 145 us per launch, step 23.4k -> 18.4k cycles (DW phase 8.0k,
// GEMM phase 7.8k, barrier B 2.6k), 254 VGPRs and no spill against 256 with 26 spilled; bench +2.6 % in 8 of 8
// interleaved pairs (A spread 1.4 %). The barriers were the smaller part: the same schedule with config 1's
// resident residual weights and hoisted lane addresses spilled 37 VGPRs and ran 174 us, with the depthwise
// reads shared on top 54 spilled and 221 us -- a scratch reload in the GEMM phase waits behind the x-row DMA.
// 23 / 123 (block3's default): config 21 with both depthwise convs on the matrix cores (DWM in the two-phase
// loop: eb_dw_mfma_two; dw2 as row pairs per column fragment and 16-channel group, dw1 as the wave's two
// units per group; weight operands rebuilt from the LDS entries every iteration). NOT bit-identical to 21
// (the MFMA sums a tap pair's products its own way; tests/test_entry_block3_dwm_gpu.py: same bound against
// the fp32 oracle, bit-equal across plans and launches). One lease (profiles/entry_block3_dwm.txt): 240
// VGPRs, no spill; DW phase 715 -> 342 VALU, 8 -> 68 MFMA, 68 -> 70 ds_read per wave; 148 -> 128 us per
// launch, DW phase 8.0k -> 6.0k cycles of an 18.4k -> 16.5k iteration; bench +1.25 % in 8 of 8 interleaved
// pairs (A spread 0.62 %), bench logits within 7.7e-3 of the parent build's. Forms measured and dropped, same
// file: the reads left to the scheduler (eb_dw_mfma_rowpair / single rows: it interleaves read, wait and
// MFMA one by one, 137 us), the reads fenced off but every address rebuilt per item (384 VALU, 133 us),
// the residual weights fetched ahead of dw1 (12 VGPRs spilled, 140 us) or half of them (254 VGPRs, 126 us:
// inside the noise of the simpler form).
//
// Retired configurations (their ids are refused). Each lost a measured comparison to a build above:
// 0, 2, 4, 5: block2 on the four-phase loop of entry_block_kernel; every wave ran dw1 ->
// GEMM1 (+ residual) -> dw2 -> GEMM2 + pool one after another, one slice per wave; VALU / MFMA depthwise
// (0 / 2, 15-column strips) and 13-column strips, small enough (LDS, <= 128 VGPRs) for two workgroups per CU
// (4 / 5). ~2k cycles per phase, all of them LDS-throughput bound: 216.2 us (config 2) and 208.4 us
// (config 5) against the warp-specialized kernel's 210.5 -> 191.8 -> 163.4 us (profiles/entry_block_ab_r4.txt,
// profiles/entry_block_rowpair.txt). With them went the forms only one-slice waves had registers for: the
// biases and step words in registers, the A fragments hoisted above a phase's stores, the deferred depthwise
// stores.
// 13 / 113: block2 warp-specialized (16 waves: 8 producers run the depthwise of later steps while 8
// consumers run the GEMMs of earlier ones; 13-column strips) with no consumer dw2 unit. 210.5 us against
// config 2's 216.2 / config 5's 208.4 (profiles/entry_block_ab_r4.txt, round 5): the producers'
// LDS-latency-bound depthwise (6,336 cycles per step) stays the critical path, consumers idle 37 %; lost to
// 15 above. The 8-wave build (4 + 4) ran 280.4 us (producers 10,252 cycles per step) and was removed.
#define KDL_EB_CONFIGS(X) /* (id, DWM, TWOPH) */ \
  X(1, false, false)      \
  X(21, false, true)      \
  X(23, true, true)       \
  X(101, false, false)    \
  X(121, false, true)     \
  X(123, true, true)

#define KDL_EBW_CONFIGS(X) /* (id, CDW, RP) */ \
  X(15, 1, false)          \
  X(17, 0, true)           \
  X(19, 1, true)           \
  X(115, 1, false)         \
  X(117, 0, true)          \
  X(119, 1, true)

int entry_block_config(int cfg, int* c0, int* c1, int* pc, int* lds) {
  switch (cfg) {
#define KDL_EBINFO(id, dwm, tp) \
  case id: { using G = Eb3Geom<dwm, tp>; *c0 = G::C0; *c1 = G::C1; *pc = G::PC; *lds = G::BYTES; return 0; }
    KDL_EB_CONFIGS(KDL_EBINFO)
#undef KDL_EBINFO
#define KDL_EBWINFO(id, cdw, rp) \
  case id: *c0 = Eb2Geom::C0; *c1 = Eb2Geom::C1; *pc = Eb2Geom::PC; *lds = Eb2Geom::BYTES; return 0;
    KDL_EBW_CONFIGS(KDL_EBWINFO)
#undef KDL_EBWINFO
    default: return -1;
  }
}

hipError_t entry_block(int cfg, const EntryBlockArgs& a, hipStream_t s) {
  int c0, c1, pc, lds;
  if (entry_block_config(cfg, &c0, &c1, &pc, &lds) != 0 || a.ldx != c0 || a.ldy != c1 || a.grid < 1 ||
      a.OH != (a.H - 1) / 2 + 1 || a.OW != (a.W - 1) / 2 + 1 || a.H % 2 != a.W % 2 || !a.steps || !a.step_off ||
      a.B > 256)                                     // the packed LDS step word holds an 8-bit image index
    return hipErrorInvalidValue;
  // TF 'same': leading pool pad 1 iff the size is odd; block2's kernel is built for odd maps, block3's for even ones
  if ((c0 == Eb2Geom::C0) != (a.H % 2 == 1)) return hipErrorInvalidValue;
  switch (cfg) {
#define KDL_EBCASE(id, dwm, tp)                                                                       \
  case id:                                                                                            \
    hipLaunchKernelGGL((entry_block_kernel<(id >= 100), dwm, tp>), dim3(a.grid), dim3(64 * Eb3Geom<dwm, tp>::NW), lds, s, a); \
    break;
    KDL_EB_CONFIGS(KDL_EBCASE)
#undef KDL_EBCASE
#define KDL_EBWCASE(id, cdw, rp)                                                                      \
  case id:                                                                                            \
    hipLaunchKernelGGL((entry_block_ws_kernel<(id >= 100), cdw, rp>), dim3(a.grid), dim3(64 * Eb2Geom::NWAV), 0, s, a); \
    break;   /* static LDS */
    KDL_EBW_CONFIGS(KDL_EBWCASE)
#undef KDL_EBWCASE
  }
  return hipGetLastError();
}

}  // namespace kdl
