// ViT above 256 tokens (ViT-B/16 at 384 x 384: 577 tokens), launch.h attn_ahat / rollout_chain: the
// rollout heatmap for up to kLongMaxT = 1024 tokens. rollout.hip is built around T <= 256 (a whole
// score row, the head mean and two heads of K in registers, four waves x 64 output columns); these two
// kernels are sized by the T they get. Attention itself stays on attention.hip's query-tiled kernel: a
// 13-wave query-block kernel with double-buffered K / V^T tiles measured 5 % slower at B 32, T 577
// (profiles/vit_384.txt) and is not here.
//
// attn_ahat_kernel<WF>: A^ = (mean_h softmax(Q_h K_h^T scale) + I) / 2 for 16 query rows per workgroup,
// 8 waves. Wave w owns the key fragments (16 keys) w, w + 8, ..: WF of them, WF = 3 / 5 / 8 for
// T <= 384 / 640 / 1024, so 577 tokens run the 5-fragment instance. A K fragment is used once per
// workgroup: it goes from global memory into the MFMA A operand, in two groups per head: the second
// group is requested under the first group's MFMAs, the next head's first group under the second's and
// under the softmax. A head's scores stay in registers, the waves' (max, sum) pairs meet in LDS (one
// barrier per head, two buffers by head parity) and are combined in wave order, the head mean
// accumulates in fp32 registers and the rows go straight to global memory.
//   16 rows, 8 waves: the scores and the mean of ONE B operand keep the 5-fragment instance under 128
//   VGPRs, so two workgroups share a CU and one's barrier and softmax hide behind the other's loads;
//   32 rows would halve the K traffic from L2 but double both register sets. 8 waves, not 4, halve
//   the fragments (and registers) per wave and put twice the loads in flight.
// A row depends on that row's Q alone and every sum runs in a fixed order: launches are bit-identical
// and row 0 of a Tq = 1 launch equals row 0 of a Tq = T launch.
//
// rollout_chain_kernel: the heatmap needs row 0 of R = A^_L .. A^_1 only, so the chain is applied from
// the left: v = row 0 of A^_L, then v = v A^_l for l = L-1 .. 1: T^2 multiply-adds per layer where the
// layer-by-layer product does T^3. One workgroup per image, 16 waves, one launch: the steps depend on
// each other through v, which lives in LDS, so nothing has to cross workgroups. Lanes run along the
// output columns (a wave reads 1 KB of an A^ row at a time, 8 rows in flight); wave w sums the rows
// [w ch, (w + 1) ch), ch = ceil(T / 16), upwards, and the 16 partial rows are added in wave order.
// Then [class, score, v[1..T-1] / max] as rollout_map writes it. No atomics: launches are bit-identical.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int VL_DH = 64;

constexpr int AH_Q = 16;                   // query rows per workgroup
constexpr int AH_NW = 8;                   // waves: wave w owns the key fragments w, w + 8, ..

template <int WF>
__global__ __launch_bounds__(64 * AH_NW) void attn_ahat_kernel(AttnAhatArgs a) {
  constexpr int G0 = (WF + 1) / 2, G1 = WF - G0;   // the two fragment groups of a head
  static_assert(G1 >= 1, "two groups per head");
  __shared__ float redm[2][AH_NW][AH_Q], redl[2][AH_NW][AH_Q];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int nqt = (a.Tq + AH_Q - 1) / AH_Q;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);   // an image's tiles read its K through one L2
  const int qt = bid % nqt, b = bid / nqt;
  const int T = a.T;
  const long ld = 3L * a.H * VL_DH;
  const uint16_t* base = a.qkv + (long)b * T * ld;
  const int qi = qt * AH_Q + c;
  const bool qvalid = qi < a.Tq;
  const int nkf = (T + 15) / 16;
  const float sl2 = a.scale * 1.4426950408889634f;
  const u32x4 z4 = {0u, 0u, 0u, 0u};

  // fragment i of this wave: key rows 16 (8i + wave) + c, dims 32kk + 8q ..
  u32x4 ka[G0][2], kb[G1][2], qc[2], qn[2] = {z4, z4};
  auto frag = [&](int h, int i, u32x4 (&dst)[2]) {
    const int key = 16 * (AH_NW * i + wave) + c;
    const uint16_t* kp = base + (long)key * ld + (a.H + h) * VL_DH + 8 * q;
    dst[0] = key < T ? *(const u32x4*)kp : z4;
    dst[1] = key < T ? *(const u32x4*)(kp + 32) : z4;
  };
  auto load_q = [&](int h, u32x4 (&dst)[2]) {
    const uint16_t* qp = base + (long)qi * ld + h * VL_DH + 8 * q;
    dst[0] = qvalid ? *(const u32x4*)qp : z4;
    dst[1] = qvalid ? *(const u32x4*)(qp + 32) : z4;
  };
  f32x4 acc[WF];
#pragma unroll
  for (int i = 0; i < WF; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  load_q(0, qc);
#pragma unroll
  for (int i = 0; i < G0; ++i) frag(0, i, ka[i]);
  for (int h = 0; h < a.H; ++h) {                  // H is the same for every wave: the barriers match
#pragma unroll
    for (int i = 0; i < G1; ++i) frag(h, G0 + i, kb[i]);
    const s16x8 qf[2] = {__builtin_bit_cast(s16x8, qc[0]), __builtin_bit_cast(s16x8, qc[1])};
    // S^T[key 16 (8i + wave) + 4q + r][query c]
    f32x4 s[WF];
#pragma unroll
    for (int i = 0; i < G0; ++i) {
      s[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[i] = mfma16(__builtin_bit_cast(s16x8, ka[i][kk]), qf[kk], s[i]);
    }
    if (h + 1 < a.H) {
      load_q(h + 1, qn);
#pragma unroll
      for (int i = 0; i < G0; ++i) frag(h + 1, i, ka[i]);
    }
#pragma unroll
    for (int i = 0; i < G1; ++i) {
      s[G0 + i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[G0 + i] = mfma16(__builtin_bit_cast(s16x8, kb[i][kk]), qf[kk], s[G0 + i]);
    }
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < WF; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * (AH_NW * i + wave) + 4 * q + r;
        const float v = key < T ? s[i][r] * sl2 : -INFINITY;
        s[i][r] = v;
        m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    const float mu = m == -INFINITY ? 0.f : m;     // a wave whose keys are all masked: p = 0, l = 0
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < WF; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __builtin_amdgcn_exp2f(s[i][r] - mu);
        s[i][r] = p;
        l += p;
      }
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    const int par = h & 1;
    if (q == 0) { redm[par][wave][c] = m; redl[par][wave][c] = l; }
    __syncthreads();
    // the full row: maximum over the waves, sum in wave order
    float mw[AH_NW], M = -INFINITY;
#pragma unroll
    for (int w = 0; w < AH_NW; ++w) { mw[w] = redm[par][w][c]; M = fmaxf(M, mw[w]); }   // key 0 is real: M is finite
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < AH_NW; ++w) L += redl[par][w][c] * __builtin_amdgcn_exp2f(mw[w] - M);
    const float f = __builtin_amdgcn_exp2f(m - M) / L;
#pragma unroll
    for (int i = 0; i < WF; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][r] += s[i][r] * f;
    qc[0] = qn[0];
    qc[1] = qn[1];
  }

  // A^ rows: (mean over the heads + I) / 2
  if (!qvalid) return;
  const float hs = 0.5f / (float)a.H;
#pragma unroll
  for (int i = 0; i < WF; ++i) {
    const int kf = AH_NW * i + wave;
    if (kf >= nkf) continue;
    const int key0 = 16 * kf + 4 * q;
    float4 v;
    v.x = acc[i][0] * hs + (key0 == qi ? 0.5f : 0.f);
    v.y = acc[i][1] * hs + (key0 + 1 == qi ? 0.5f : 0.f);
    v.z = acc[i][2] * hs + (key0 + 2 == qi ? 0.5f : 0.f);
    v.w = acc[i][3] * hs + (key0 + 3 == qi ? 0.5f : 0.f);
    float* row = a.out + ((long)b * T + qi) * a.ldr + key0;
    if (key0 + 3 < T) {
      *(float4*)row = v;
    } else {
      if (key0 < T) row[0] = v.x;
      if (key0 + 1 < T) row[1] = v.y;
      if (key0 + 2 < T) row[2] = v.z;
    }
  }
}

constexpr int RC_NW = 16;                  // waves: the row partition of a layer's sum
constexpr int RC_U = 8;                    // A^ rows in flight per wave

__global__ __launch_bounds__(64 * RC_NW) void rollout_chain_kernel(RolloutChainArgs a) {
  extern __shared__ __attribute__((aligned(16))) float rc_sm[];   // v [Tp] | part [RC_NW][Tp]
  __shared__ float ws[RC_NW];
  const int T = a.T, Tp = (T + 3) & ~3;
  float* v = rc_sm;
  float* part = rc_sm + Tp;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long img = (long)b * T * a.ldr;
  const float* top_row = a.ahat[a.L - 1] + img;    // row 0 of A^_L
  if (tid < T) v[tid] = top_row[tid];              // T <= 1024 = the block
  __syncthreads();
  const int ch = (T + RC_NW - 1) / RC_NW;
  const int i0 = wave * ch, i1 = min(T, i0 + ch);  // this wave's rows (none when i0 >= T)
  for (int l = a.L - 2; l >= 0; --l) {
    const float* A = a.ahat[l] + img;
    // lane = four columns from j0 on; j0 < T and ldr % 4 == 0: the 16 bytes lie inside the row stride.
    // What a padding column holds only reaches the components that are never read back.
    for (int j0 = 4 * lane; j0 < T; j0 += 256) {
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int i = i0; i < i1; i += RC_U) {
        float4 r[RC_U];
#pragma unroll
        for (int u = 0; u < RC_U; ++u) r[u] = *(const float4*)(A + (long)min(i + u, i1 - 1) * a.ldr + j0);
#pragma unroll
        for (int u = 0; u < RC_U; ++u) {
          if (i + u >= i1) break;
          const float vi = v[i + u];
          acc.x = fmaf(vi, r[u].x, acc.x);
          acc.y = fmaf(vi, r[u].y, acc.y);
          acc.z = fmaf(vi, r[u].z, acc.z);
          acc.w = fmaf(vi, r[u].w, acc.w);
        }
      }
      *(float4*)(part + wave * Tp + j0) = acc;
    }
    __syncthreads();
    if (tid < T) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < RC_NW; ++w) s += part[w * Tp + tid];
      v[tid] = s;
    }
    __syncthreads();
  }
  // the maximum of v[1 .. T-1] (exact in any order), a real division, `top` in front
  const float x = tid + 1 < T ? v[tid + 1] : 0.f;
  float m = x;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
  if (lane == 0) ws[wave] = m;
  __syncthreads();
  m = ws[0];
#pragma unroll
  for (int w = 1; w < RC_NW; ++w) m = fmaxf(m, ws[w]);
  float* row = a.out + (long)b * a.ldo;
  if (tid + 1 < T) row[2 + tid] = m > 0.f ? x / m : 0.f;
  if (tid < 2) ((int32_t*)row)[tid] = a.top[2 * b + tid];   // class and score, as 32-bit words
}

static bool long_bad_ptr(const void* p, uintptr_t mask) { return !p || ((uintptr_t)p & mask); }

hipError_t attn_ahat(const AttnAhatArgs& a, hipStream_t s) {
  if (a.dh != VL_DH || a.T < 1 || a.T > kLongMaxT || a.H < 1 || a.B < 1) return hipErrorInvalidValue;
  if (a.Tq < 1 || a.Tq > a.T || a.ldr < a.T || a.ldr % 4 != 0) return hipErrorInvalidValue;
  if (long_bad_ptr(a.qkv, 15) || long_bad_ptr(a.out, 15)) return hipErrorInvalidValue;
  const long nwg = (long)a.B * ((a.Tq + AH_Q - 1) / AH_Q);
  if (nwg > 0x7fffffffL) return hipErrorInvalidValue;
  const int wf = ((a.T + 15) / 16 + AH_NW - 1) / AH_NW;   // key fragments per wave
  const dim3 grid((unsigned)nwg), block(64 * AH_NW);
  if (wf <= 3) hipLaunchKernelGGL(attn_ahat_kernel<3>, grid, block, 0, s, a);
  else if (wf <= 5) hipLaunchKernelGGL(attn_ahat_kernel<5>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(attn_ahat_kernel<8>, grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t rollout_chain(const RolloutChainArgs& a, hipStream_t s) {
  if (a.T < 2 || a.T > kLongMaxT || a.L < 1 || a.B < 1) return hipErrorInvalidValue;
  if (a.ldr < a.T || a.ldr % 4 != 0 || a.ldo < a.T + 1) return hipErrorInvalidValue;
  if (long_bad_ptr(a.ahat, 7) || long_bad_ptr(a.top, 3) || long_bad_ptr(a.out, 3)) return hipErrorInvalidValue;
  const size_t smem = (size_t)(RC_NW + 1) * ((a.T + 3) & ~3) * sizeof(float);
  hipLaunchKernelGGL(rollout_chain_kernel, dim3((unsigned)a.B), dim3(64 * RC_NW), smem, s, a);
  return hipGetLastError();
}

}  // namespace kdl
