// Gallery scan over e4m3 rows (launch.h GalleryTopkArgs::g8 / scale): the scan launch of
// gallery_topk for a gallery stored in one byte per value with one fp32 scale per row,
// score[b][j] = scale[j] * sum_i q[b][i] * val(g8[j][i]). Split, pick and merge are similar.hip's.
//
// What differs from the bf16 scan is how gallery bytes reach the matrix cores. There every wave
// instruction reads 64 bytes from each of 16 rows; here rows go through LDS with row-contiguous
// global loads. A workgroup owns kGalleryChunk = 256 rows and each of its four waves 64 of them.
// A stage is 128 columns of a wave's 64 rows: one 128-byte line per row, fetched with 16-byte
// loads in which the 8 adjacent lanes l, l + 1, ... of a row cover that line (lane l of load i:
// row 8 i + l / 8, bytes 16 (l % 8) .. + 15), eight loads per lane and stage, then written to LDS
// with ds_write_b128. The ring is two stages deep and a third is in registers: iteration s first
// writes stage s + 1 (requested an iteration ago) into the buffer that iteration s - 1 read, then
// requests stage s + 2, then runs the MFMAs of stage s, so a stage's loads are in flight under a
// whole stage of MFMAs and its LDS writes a whole stage ahead of its reads. A wave consumes only
// the rows it staged itself: LDS instructions of one wave complete in order, so the k-loop has
// the wave's own vmcnt / lgkmcnt waits and no workgroup barrier.
//
// LDS row stride F8_ROW = 144 bytes = 36 dwords. A fragment read is ds_read_b64: lane (row
// r = lane % 16, column group c = lane / 16) reads dwords 36 r + 8 ks + 2 c, + 1 of k-step ks.
// The hardware serves a b64 read a half-wave at a time: 16 rows x c in {0, 1} (or {2, 3}).
// 36 r mod 64 = 4 (9 r mod 16) takes 16 distinct multiples of 4 (9 is odd), so the 16 rows start 4
// banks apart and the 2 c, + 1 dwords fill those 4 banks: 64 lanes-dwords on 64 banks, no conflict.
// (The b128 writes, 16 lanes = two rows at a time, overlap in 4 of the 64 banks: 2-way on one
// lane in 16, once per staged byte against once per read byte.)
// Ring: 4 waves x 2 stages x 64 rows x 144 bytes = 73,728 bytes, two workgroups per CU. The
// 32 x 260 fp32 score tile of the epilogue (33,280 bytes) aliases the ring behind a barrier.
//
// Conversion, in registers: v_cvt_pk_f32_fp8 turns two codes into two floats, exactly (every e4m3
// value, subnormal codes and +-0 included, is an fp32 value with at most 4 significant bits), and
// v_perm_b32 keeps their high halves: one bf16 x 2 dword, exact again. Four VALU instructions per
// four codes, issued under the MFMAs, which are the bf16 scan's: v_mfma_f32_16x16x32_bf16 against
// the three pre-split query terms, smallest first, k-steps in ascending order for every row. The
// row scale multiplies the fp32 accumulator once, on the way to the score tile. So equal rows
// with equal scales give bit-equal scores whatever their tile, wave or chunk, two launches are
// bit-equal, and there are no atomics. Rows >= N and 16-byte pieces at columns >= F are never
// loaded (their LDS bytes are zeros), k-steps at or past F are not run, queries >= B are the split
// kernel's zeros.
#include <type_traits>

#include "similar.h"

namespace kdl {

constexpr int F8_STAGE = 128;                        // columns = bytes of a row per stage
constexpr int F8_STEPS = F8_STAGE / 32;              // k-steps per stage
constexpr int F8_ROW = F8_STAGE + 16;                // LDS row stride in bytes
constexpr int F8_RING = 2;
constexpr int F8_LOADS = GAL_WROWS * F8_STAGE / (64 * 16);   // 16-byte loads per lane and stage
constexpr int F8_WSTAGE = GAL_WROWS * F8_ROW;        // bytes of one wave's stage
constexpr int F8_SMEM = GAL_WAVES * F8_RING * F8_WSTAGE;
static_assert(F8_LOADS == 8 && F8_ROW % 16 == 0 && (F8_ROW / 4) % 64 == 36, "staging shape / bank arithmetic");
static_assert(F8_SMEM >= 32 * GAL_LDS * (int)sizeof(float) && F8_SMEM <= 96 * 1024, "the score tile aliases the ring");

// four e4m3 codes -> four bf16 in two dwords, in code order
__device__ __forceinline__ u32x2 f8x4_to_bf16(uint32_t w) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
  return (u32x2){__builtin_amdgcn_perm(__float_as_uint(a[1]), __float_as_uint(a[0]), 0x07060302u),
                 __builtin_amdgcn_perm(__float_as_uint(b[1]), __float_as_uint(b[0]), 0x07060302u)};
}

// LDS traffic of one wave with itself: the hardware keeps a wave's LDS instructions in order, this
// keeps the compiler from moving the reads of a stage above the writes that staged it
__device__ __forceinline__ void f8_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// QT: 16-query tiles per pass
template <int QT>
__global__ __launch_bounds__(64 * GAL_WAVES) void gallery_scan_f8_kernel(GalleryTopkArgs a, int chunks) {
  extern __shared__ __attribute__((aligned(16))) uint8_t f8smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int chunk = blockIdx.x, b0 = blockIdx.y * 32;
  const int row0 = chunk * kGalleryChunk + wave * GAL_WROWS;

  // staging: load i of a stage is row 8 i + lane / 8 of the wave, bytes 16 (lane % 8) .. + 15 of the line.
  // Every lane loads something, so the loop has no divergent branch and the waits stay exact
  // counts: a row >= N loads row N - 1 again (its scores are never picked), a piece at columns
  // >= F loads the row's first piece and is stored as zeros
  const int sr = lane >> 3, sc8 = 16 * (lane & 7);
  const uint8_t* gp[F8_LOADS];
#pragma unroll
  for (int i = 0; i < F8_LOADS; ++i) gp[i] = a.g8 + (long)min(row0 + 8 * i + sr, a.N - 1) * a.ldg;
  uint8_t* const ring = f8smem + wave * (F8_RING * F8_WSTAGE);
  uint8_t* const wp = ring + sr * F8_ROW + sc8;
  // fragments: row lane % 16 of tile t, bytes 32 ks + 8 (lane / 16) .. + 7 of the stage
  const uint8_t* const rp = ring + l15 * F8_ROW + 8 * kg;
  // this pass's split queries: fragment (tile u, k-step ks, term p) at qs[((u * kGalSteps + ks) * 3 + p) * 64]
  const u32x4* qs = (const u32x4*)a.work + (long)blockIdx.y * 2 * kGalSteps * 3 * 64 + lane;
  const int nsteps = (a.F + 31) / 32, nstages = (a.F + F8_STAGE - 1) / F8_STAGE;

  f32x4 acc[GAL_TILES][QT];
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[t][u] = (f32x4){0.f, 0.f, 0.f, 0.f};

  u32x4 st[F8_LOADS], qf[F8_STEPS][QT][3];
  auto fetch = [&](int s) {                          // F % 16 == 0: a lane's 16 columns are in or out
    const int c = s * F8_STAGE + sc8, off = c < a.F ? c : 0;
#pragma unroll
    for (int i = 0; i < F8_LOADS; ++i) st[i] = *(const u32x4*)(gp[i] + off);
  };
  auto stash = [&](int s) {
    const bool cok = s * F8_STAGE + sc8 < a.F;
#pragma unroll
    for (int i = 0; i < F8_LOADS; ++i)
      *(u32x4*)(wp + (s & 1) * F8_WSTAGE + 8 * i * F8_ROW) = cok ? st[i] : (u32x4){0u, 0u, 0u, 0u};
    f8_wave_sync();
  };
  // the query fragments of k-step ks into slot j (a k-step past the last loads the last again: unused)
  auto loadq = [&](int j, int ks) {
    ks = min(ks, nsteps - 1);
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p) qf[j][u][p] = qs[((long)(u * kGalSteps + ks) * 3 + p) * 64];
  };

  // vmcnt counts loads in the order of their issue, so a wait for a load is a wait for every load
  // issued before it. The query fragments of a k-step are therefore requested a whole stage ahead,
  // right after the MFMAs of the same k-step of the stage before, into the registers those just
  // read: when k-step j waits for them, the gallery loads of fetch(s + 2), issued later, stay in
  // flight, and only stash(s + 1) waits for gallery bytes, an iteration after their request.
  // NEXT: a stage s + 1 exists; AHEAD: a stage s + 2 exists; FULL: the stage has all its k-steps.
  // The steady-state body (all three) has no branch, which keeps the compiler's wait counts exact.
  auto stage = [&](int s, auto NEXT, auto AHEAD, auto FULL) {
    if constexpr (NEXT.value) stash(s + 1);
    if constexpr (AHEAD.value) {
      fetch(s + 2);
      __builtin_amdgcn_sched_barrier(0);             // here, not sunk to the last k-step to save registers
    }
    const uint8_t* cur = rp + (s & 1) * F8_WSTAGE;
    const int ks0 = s * F8_STEPS;
#pragma unroll
    for (int j = 0; j < F8_STEPS; ++j) {
      if (FULL.value || ks0 + j < nsteps) {          // uniform
        s16x8 af[GAL_TILES];
#pragma unroll
        for (int t = 0; t < GAL_TILES; ++t) {
          const u32x2 c = *(const u32x2*)(cur + t * 16 * F8_ROW + 32 * j);
          const u32x2 lo = f8x4_to_bf16(c[0]), hi = f8x4_to_bf16(c[1]);
          af[t] = __builtin_bit_cast(s16x8, (u32x4){lo[0], lo[1], hi[0], hi[1]});
        }
        // smallest term first: the same order for every row
#pragma unroll
        for (int p = 2; p >= 0; --p)
#pragma unroll
          for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
            for (int u = 0; u < QT; ++u)
              acc[t][u] = mfma16(af[t], __builtin_bit_cast(s16x8, qf[j][u][p]), acc[t][u]);
      }
      if constexpr (NEXT.value) loadq(j, ks0 + F8_STEPS + j);
    }
    f8_wave_sync();                                  // this stage's reads stay above the next stage's writes
  };
  constexpr std::true_type yes;
  constexpr std::false_type no;
  fetch(0);
  stash(0);
  if (nstages > 1) fetch(1);
#pragma unroll
  for (int j = 0; j < F8_STEPS; ++j) loadq(j, j);
  int s = 0;
  for (; s + 2 < nstages; ++s) stage(s, yes, yes, yes);
  if (s + 1 < nstages) stage(s++, yes, no, yes);
  stage(s, no, no, no);

  // accumulator element: query = lane % 16 of tile u, row = 4 * (lane / 16) + reg of tile t
  float (*sc)[GAL_LDS] = (float (*)[GAL_LDS])f8smem;
  __syncthreads();                                   // every wave has read its last stage: the score tile may overwrite the ring
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t) {
    float rs[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = row0 + t * 16 + 4 * kg + e;
      rs[e] = r < a.N ? a.scale[r] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < QT; ++u)
      *(float4*)&sc[u * 16 + l15][wave * GAL_WROWS + t * 16 + 4 * kg] =
          (float4){acc[t][u][0] * rs[0], acc[t][u][1] * rs[1], acc[t][u][2] * rs[2], acc[t][u][3] * rs[3]};
  }
  __syncthreads();

  gallery_pick<QT>(sc, a, chunks, chunk, b0, lane, wave);
}

void gallery_scan_f8(const GalleryTopkArgs& a, int chunks, hipStream_t s) {
  const dim3 grid(chunks, (a.B + 31) / 32);
  if (a.B <= 16) hipLaunchKernelGGL(gallery_scan_f8_kernel<1>, grid, dim3(64 * GAL_WAVES), F8_SMEM, s, a, chunks);
  else hipLaunchKernelGGL(gallery_scan_f8_kernel<2>, grid, dim3(64 * GAL_WAVES), F8_SMEM, s, a, chunks);
}

}  // namespace kdl
