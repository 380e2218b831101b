// Pooled-feature embeddings (launch.h EmbedRowsArgs): out[b][c] = mean over the HW pixels of
// x[b][p][c] in fp32, then optionally each row divided by max(||row||_2, 1e-12).
//
// embed_mean_kernel has gap_kernel's shape (fc.hip): grid (ceil(F / 8 / EMB_CG), B), a block
// owns EMB_CG 8-channel chunks of one image, its EMB_PARTS thread groups each sum every
// EMB_PARTS-th pixel with four independent 16-byte loads in flight, and the partial sums meet
// in LDS. One workgroup per image would be bound by per-CU bandwidth (pool_head.hip: 35-39 us
// on 32 CUs); this spreads Xception's 32 x 100 x 2048 over 256 workgroups. The last reduction
// is one thread per channel (conflict-free LDS reads, one coalesced 4-byte store each), so
// any row stride ldo >= F works, aligned or not.
// embed_l2_kernel is a second, small launch: one workgroup per row squares and sums the fp32
// means in a fixed order (thread-strided, wave butterfly, waves in order) and divides in place.
// Two launches instead of a last-block-done counter: no state to reset, nothing crosses
// workgroups inside a launch, and the rows (B x F fp32, 256 KB at batch 32) are still in L2.
// Every sum runs in a fixed order: no atomics, two launches are bit-equal.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int EMB_CG = 32, EMB_PARTS = 8, EMB_THREADS = EMB_CG * EMB_PARTS;

template <int DT>
__global__ __launch_bounds__(EMB_THREADS) void embed_mean_kernel(EmbedRowsArgs a) {
  using E = Elt<DT>;
  __shared__ __attribute__((aligned(16))) float red[EMB_PARTS][EMB_CG * 8];
  const int b = blockIdx.y, c = threadIdx.x % EMB_CG, part = threadIdx.x / EMB_CG;
  const int F8 = a.F / 8, c8 = blockIdx.x * EMB_CG + c;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  auto add = [&](const u32x4 v) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      s[2 * d] += E::lo(v[d]);
      s[2 * d + 1] += E::hi(v[d]);
    }
  };
  if (c8 < F8) {
    const uint16_t* xb = a.x + (long)b * a.HW * a.ldx + c8 * 8;
    int p = part;
    for (; p + 3 * EMB_PARTS < a.HW; p += 4 * EMB_PARTS) {
      const u32x4 v0 = *(const u32x4*)(xb + (long)p * a.ldx);
      const u32x4 v1 = *(const u32x4*)(xb + (long)(p + EMB_PARTS) * a.ldx);
      const u32x4 v2 = *(const u32x4*)(xb + (long)(p + 2 * EMB_PARTS) * a.ldx);
      const u32x4 v3 = *(const u32x4*)(xb + (long)(p + 3 * EMB_PARTS) * a.ldx);
      add(v0); add(v1); add(v2); add(v3);
    }
    for (; p < a.HW; p += EMB_PARTS) add(*(const u32x4*)(xb + (long)p * a.ldx));
  }
  float4* r = (float4*)&red[part][c * 8];
  r[0] = (float4){s[0], s[1], s[2], s[3]};
  r[1] = (float4){s[4], s[5], s[6], s[7]};
  __syncthreads();
  const int ch = blockIdx.x * (EMB_CG * 8) + threadIdx.x;     // one channel per thread
  if (ch >= a.F) return;
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < EMB_PARTS; ++q) t += red[q][threadIdx.x];   // fixed order: deterministic
  a.out[(long)b * a.ldo + ch] = t * (1.0f / (float)a.HW);
}

// one workgroup per row; F <= kEmbedMaxF = 16 elements per thread
__global__ __launch_bounds__(256) void embed_l2_kernel(EmbedRowsArgs a) {
  __shared__ float ws[4];
  float* row = a.out + (long)blockIdx.x * a.ldo;
  float v[kEmbedMaxF / 256];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < kEmbedMaxF / 256; ++j) {
    const int i = j * 256 + threadIdx.x;
    v[j] = i < a.F ? row[i] : 0.f;
    ss += v[j] * v[j];
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = ss;
  __syncthreads();
  const float n = fmaxf(sqrtf(((ws[0] + ws[1]) + ws[2]) + ws[3]), 1e-12f);
#pragma unroll
  for (int j = 0; j < kEmbedMaxF / 256; ++j) {
    const int i = j * 256 + threadIdx.x;
    if (i < a.F) row[i] = v[j] / n;
  }
}

hipError_t embed_rows(const EmbedRowsArgs& a, hipStream_t s) {
  if (!a.x || ((uintptr_t)a.x & 15) || !a.out || ((uintptr_t)a.out & 3) || a.B < 1 || a.B > 65535 || a.HW < 1 || a.F < 8 || a.F % 8 != 0 || a.F > kEmbedMaxF ||
      a.ldx % 8 != 0 || a.ldx < a.F || a.ldo < a.F || a.dt < 0 || a.dt > 1 || a.norm < 0 || a.norm > 1)
    return hipErrorInvalidValue;
  const dim3 grid((a.F / 8 + EMB_CG - 1) / EMB_CG, a.B);
  if (a.dt) hipLaunchKernelGGL(embed_mean_kernel<1>, grid, dim3(EMB_THREADS), 0, s, a);
  else hipLaunchKernelGGL(embed_mean_kernel<0>, grid, dim3(EMB_THREADS), 0, s, a);
  if (a.norm) hipLaunchKernelGGL(embed_l2_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
