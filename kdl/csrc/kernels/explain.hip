// Grad-CAM heatmaps (launch.h ClassMapArgs): for the class k that softmax_topk K = 1 left in
// `top`, heat[b][p] = max(raw_p, 0) / max_q max(raw_q, 0) with raw_p = (1/HW) sum_c d_c x[b][p][c]
// and d_c = dlogit_k/dg_c, the gradient of the class's logit by the pooled feature c. For the heads
// served here d has a closed form, so there is no backward pass:
//   linear head  logit = W g + b                  d_c = W[k][c]
//   MLP head     logit = relu(g W1 + b1) W2 + b2  d_c = sum_j [z_j > 0] W2[j][k] W1[j][c]
// Three small launches (two for the linear head), nothing crosses workgroups inside one, no atomics, every sum in a fixed
// order (replays and repeated launches are bit-equal):
//   class_map_alpha_kernel  MLP head only (the linear head's d is a row of W, which the map pass
//       reads itself: one launch less): d into the workspace `alpha` [B][F], one thread per
//       channel, grid (ceil(F / 256), ceil(B / CM_AI)): a workgroup owns 256 channels of CM_AI images, so a value of W1 [H1][F] is loaded once for
//       the four of them (one workgroup per image put 26 MB through L2 at batch 32). It walks j
//       upwards, a wave reads 256 contiguous bytes of W1 per j, 16 such loads are in flight. The
//       pass is bound by its chain of dependent load rounds, about 9 us (profiles/explain.txt). Before that it rebuilds each image's ReLU mask from dense1's
//       K-split partials with dense2_kernel's own code (pool_head.hip: two halves of 128 threads sum
//       the even and the odd slices, then b1 + even + odd), so it is the mask the logits were
//       computed with. A class outside [0, NC) gives d = 0 and reads nothing of W / W2.
//   class_map_raw_kernel    grid (ceil(HW / CM_PG), B): one workgroup per CM_PG pixels of one image
//       (one workgroup per image would be bound by per-CU bandwidth, pool_head.hip: 35-39 us).
//       Thread t owns the 8-channel chunks t, t + 256, ...: its d values stay in registers for
//       all of the workgroup's pixels, every pixel load is 16 bytes (a wave reads 1 KB of one
//       pixel row), all CM_PG loads of a chunk are in flight together. Per pixel: the thread's
//       chunks in order, a wave butterfly, the four waves in order through LDS; then
//       max(sum * (1/HW), 0) goes to out[b][2 + p]. Workgroup 0 of an image copies `top`.
//   class_map_norm_kernel   norm = 1 only, one workgroup per image: the row's maximum (exact in
//       any order) and a real fp32 division of every stored value by it; a row whose maximum is 0
//       stays 0.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int CM_PG = 8;                          // pixels per workgroup of the map pass
constexpr int CM_AI = 4;                          // images per workgroup of the MLP head's gradient pass
static_assert(CM_AI == 4 && kClassMapMaxH1 == 128, "class_map_alpha_kernel: float4 rows of v, two halves of 128 threads");
constexpr int CM_CH = kClassMapMaxF / 8 / 256;    // 8-channel chunks per thread of the map pass

__global__ __launch_bounds__(256) void class_map_alpha_kernel(ClassMapArgs a) {
  __shared__ __attribute__((aligned(16))) float v[kClassMapMaxH1][CM_AI];   // [z_j > 0] * w2[j][k] per image
  __shared__ float red[2][kClassMapMaxH1];
  const int tid = threadIdx.x, c = blockIdx.x * 256 + tid;
  const int b0 = blockIdx.y * CM_AI, nimg = min(CM_AI, a.B - b0);
  const int nkb = a.F / 64, o = tid & (kClassMapMaxH1 - 1), h = tid / kClassMapMaxH1;
#pragma unroll
  for (int i = 0; i < CM_AI; ++i) {
    // dense2_kernel's own sums: half h takes the K-split slices h, h + 2, ... from 0 upwards
    float s = 0.f;
    if (i < nimg && o < a.H1) {
#pragma unroll 16
      for (int kb = h; kb < nkb; kb += 2) s += a.hid[((long)kb * a.B + b0 + i) * a.H1 + o];
    }
    red[h][o] = s;
    __syncthreads();
    if (tid < kClassMapMaxH1) {
      float val = 0.f;                            // units past H1 and images past B: 0, they add nothing below
      if (i < nimg && tid < a.H1) {
        const int k = a.top[2 * (b0 + i)];
        const float z = a.b1[tid] + red[0][tid] + red[1][tid];
        if (k >= 0 && k < a.NC && z > 0.f) val = a.w2[(long)tid * a.NC + k];
      }
      v[tid][i] = val;
    }
    __syncthreads();
  }
  if (c >= a.F) return;
  float d[CM_AI];
#pragma unroll
  for (int i = 0; i < CM_AI; ++i) d[i] = 0.f;
  for (int j0 = 0; j0 < a.H1; j0 += 16) {         // j upwards, 16 independent loads of w1 in flight
    float w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) w[u] = a.w1[(long)min(j0 + u, a.H1 - 1) * a.F + c];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const float4 vv = *(const float4*)v[j0 + u];
      d[0] += vv.x * w[u];
      d[1] += vv.y * w[u];
      d[2] += vv.z * w[u];
      d[3] += vv.w * w[u];
    }
  }
#pragma unroll
  for (int i = 0; i < CM_AI; ++i)
    if (i < nimg) a.alpha[(long)(b0 + i) * a.F + c] = d[i];
}

template <int DT, int HEAD>
__global__ __launch_bounds__(256) void class_map_raw_kernel(ClassMapArgs a) {
  using E = Elt<DT>;
  __shared__ float ws[4][CM_PG];
  const int b = blockIdx.y, p0 = blockIdx.x * CM_PG, tid = threadIdx.x;
  const int F8 = a.F / 8, np = min(CM_PG, a.HW - p0);
  const uint16_t* xb = a.x + ((long)b * a.HW + p0) * a.ldx;
  const float* al = a.alpha + (long)b * a.F;
  const int k = a.top[2 * b];
  const bool kok = k >= 0 && k < a.NC;            // linear head: d is row k of w, read here
  float acc[CM_PG];
#pragma unroll
  for (int i = 0; i < CM_PG; ++i) acc[i] = 0.f;
#pragma unroll
  for (int q = 0; q < CM_CH; ++q) {
    const int c8 = q * 256 + tid;
    if (c8 < F8) {
      float d[8];
      if (HEAD == 0) {
        const u32x4 wv = kok ? *(const u32x4*)(a.w + (long)k * a.F + c8 * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) { d[2 * e] = E::lo(wv[e]); d[2 * e + 1] = E::hi(wv[e]); }
      } else {
        const float4 d0 = *(const float4*)(al + c8 * 8), d1 = *(const float4*)(al + c8 * 8 + 4);
        d[0] = d0.x; d[1] = d0.y; d[2] = d0.z; d[3] = d0.w; d[4] = d1.x; d[5] = d1.y; d[6] = d1.z; d[7] = d1.w;
      }
      u32x4 xv[CM_PG];
#pragma unroll
      for (int i = 0; i < CM_PG; ++i)
        xv[i] = i < np ? *(const u32x4*)(xb + (long)i * a.ldx + c8 * 8) : (u32x4){0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < CM_PG; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[i] += d[2 * e] * E::lo(xv[i][e]);
          acc[i] += d[2 * e + 1] * E::hi(xv[i][e]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CM_PG; ++i) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[i] += __shfl_xor(acc[i], m, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int i = 0; i < CM_PG; ++i) ws[tid >> 6][i] = acc[i];
  }
  __syncthreads();
  float* row = a.out + (long)b * a.ldo;
  if (tid < np) {
    const float s = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
    row[2 + p0 + tid] = fmaxf(s * (1.0f / (float)a.HW), 0.f);
  }
  if (blockIdx.x == 0 && tid >= 64 && tid < 66)   // class and score, as 32-bit words
    ((int32_t*)row)[tid - 64] = a.top[2 * b + tid - 64];
}

// the MLP head's gradient pass: d into the workspace `alpha` [B][F]

// one workgroup per image; HW <= kClassMapMaxHW = 16 values per thread
__global__ __launch_bounds__(256) void class_map_norm_kernel(ClassMapArgs a) {
  __shared__ float ws[4];
  float* row = a.out + (long)blockIdx.x * a.ldo + 2;
  float v[kClassMapMaxHW / 256];
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < kClassMapMaxHW / 256; ++j) {
    const int i = j * 256 + threadIdx.x;
    v[j] = i < a.HW ? row[i] : 0.f;
    m = fmaxf(m, v[j]);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(ws[0], ws[1]), fmaxf(ws[2], ws[3]));
#pragma unroll
  for (int j = 0; j < kClassMapMaxHW / 256; ++j) {
    const int i = j * 256 + threadIdx.x;
    if (i < a.HW) row[i] = m > 0.f ? v[j] / m : 0.f;
  }
}

hipError_t class_map(const ClassMapArgs& a, hipStream_t s) {
  auto bad = [](const void* p, uintptr_t mask) { return !p || ((uintptr_t)p & mask); };
  if (bad(a.x, 15) || bad(a.top, 3) || bad(a.alpha, 15) || bad(a.out, 3)) return hipErrorInvalidValue;
  if (a.head < 0 || a.head > 1 || a.dt < 0 || a.dt > 1 || a.norm < 0 || a.norm > 1) return hipErrorInvalidValue;
  if (a.B < 1 || a.B > 65535 || a.HW < 1 || a.HW > kClassMapMaxHW || a.F < 8 || a.F > kClassMapMaxF ||
      a.NC < 1 || a.NC > kClassMapMaxNC)
    return hipErrorInvalidValue;
  if (a.ldx % 8 != 0 || a.ldx < a.F || a.ldo < 2 + a.HW) return hipErrorInvalidValue;
  if (a.head == 0) {
    if (a.F % 8 != 0 || bad(a.w, 15)) return hipErrorInvalidValue;
  } else {
    if (a.F % 64 != 0 || a.H1 < 1 || a.H1 > kClassMapMaxH1 || bad(a.w1, 3) || bad(a.w2, 3) || bad(a.b1, 3) ||
        bad(a.hid, 3))
      return hipErrorInvalidValue;
  }
  const dim3 gr((a.HW + CM_PG - 1) / CM_PG, a.B);
  if (a.head) {
    hipLaunchKernelGGL(class_map_alpha_kernel, dim3((a.F + 255) / 256, (a.B + CM_AI - 1) / CM_AI), dim3(256), 0, s, a);
    if (a.dt) hipLaunchKernelGGL((class_map_raw_kernel<1, 1>), gr, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((class_map_raw_kernel<0, 1>), gr, dim3(256), 0, s, a);
  } else {
    if (a.dt) hipLaunchKernelGGL((class_map_raw_kernel<1, 0>), gr, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((class_map_raw_kernel<0, 0>), gr, dim3(256), 0, s, a);
  }
  if (a.norm) hipLaunchKernelGGL(class_map_norm_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
