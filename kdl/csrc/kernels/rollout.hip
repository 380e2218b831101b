// Attention rollout for ViT (Abnar & Zuidema 2020), launch.h AttnRolloutArgs / RolloutMapArgs. Per
// layer, with P_h = softmax(Q_h K_h^T * scale) over the keys of head h:
//   A^ = (mean_h P_h + I) / 2,   R_out = A^ R_in   (the first layer: R_out = A^),
// and after the last layer heat = R[0][1..T-1] / its largest value. The flash-style attention
// kernel never materialises P, so this is a kernel of its own beside each layer's attention step.
//
// attn_rollout_kernel: workgroup = (image, RO_Q = 16 query rows), 4 waves. A 16-row tile makes
// ceil(197 / 16) * 32 = 416 workgroups at batch 32 (a 64-row tile: 128 on 256 CUs).
//   1. Scores. Per head every wave forms S^T = K Q^T with v_mfma_f32_16x16x32_bf16 exactly as
//      attn_head_kernel does (A = 16 K rows, B = Q^T in registers), for the key fragments
//      kf = wave, wave + 4, ...: a lane holds 4 x 4 scores of ONE query (lane & 15). A K fragment is
//      used once per workgroup (16 queries are one B operand), so it goes from global memory
//      straight into the A operand (16 bytes per lane), not through LDS; the next head's fragments
//      are loaded while this head's softmax runs. Each wave reduces its keys to a local maximum and
//      sum per query, the four (max, sum) pairs meet in LDS (one barrier per head, two buffers by
//      head parity), and every wave rescales to the full-row maximum and sum in wave order 0..3.
//      The head mean accumulates in fp32 registers. Keys >= T are masked to -inf by a select.
//   2. A^ = acc / (2H) + I / 2 goes to LDS [16][RO_AS] fp32 (r_in == null: straight to r_out).
//   3. Product. Wave w owns the 64 output columns from 64w on and runs v_mfma_f32_16x16x4_f32 (exact
//      fp32: a k-ordered fmaf chain) over k = 0 .. T-1 upwards on four accumulator tiles. Tile i holds
//      the columns 64w + 4c + i (c = lane & 15), so a lane's four B values of a k-step are one 16-byte
//      load of r_in (a wave reads 4 rows x 256 contiguous bytes) and its four results of an output
//      row one 16-byte store; eight k-steps are requested at a time, the next eight behind them. The
//      A operand is one float per lane from LDS (row stride 260 words: the 64 lanes hit 64 banks).
//      Rows >= T of r_in are never read and its columns >= T never used (they may hold anything);
//      rows >= Tq and columns >= T of r_out are never written.
//   Blocks are remapped so that an image's tiles run on one XCD and share its L2 (K is read once per
//   tile: 13 times per image at T = 197).
// No atomics, every sum in a fixed order: launches are bit-identical. A row's values depend on that
// row's Q alone, so row 0 of a Tq = 1 launch equals row 0 of a Tq = T launch bit for bit, and
// r_in == null equals an explicit identity (x * 1 + 0 and + x * 0 are exact).
//
// rollout_map_kernel: one workgroup per image: the maximum of r[b][0][1..T-1] (exact in any order),
// a real fp32 division of each value by it, and `top`'s class and score in front.
#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int RO_Q = 16;                     // query rows per workgroup
constexpr int RO_DH = 64;
constexpr int RO_KF = kRolloutMaxT / 16;     // key fragments of 16 at the largest T
constexpr int RO_WF = RO_KF / 4;             // key fragments (and output column tiles) per wave
constexpr int RO_AS = kRolloutMaxT + 4;      // LDS row stride of A^ in words: 4 (mod 64)
static_assert(RO_KF % 4 == 0, "four waves share the key fragments");

__device__ __forceinline__ f32x4 mfma_f32(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256) void attn_rollout_kernel(AttnRolloutArgs a) {
  __shared__ __attribute__((aligned(16))) float ahat[RO_Q * RO_AS];
  __shared__ float redm[2][4][RO_Q], redl[2][4][RO_Q];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q = lane >> 4, c = lane & 15;
  const int nqt = (a.Tq + RO_Q - 1) / RO_Q;
  // blocks n, n + 8, ... run on one XCD: give each XCD a contiguous run of (image, tile) pairs, so the
  // ceil(Tq / 16) workgroups of an image read its K and R through one L2
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = bid % nqt, b = bid / nqt;
  const int T = a.T;
  const long ld = 3L * a.H * RO_DH;
  const uint16_t* base = a.qkv + (long)b * T * ld;
  const int qi = qt * RO_Q + c;                    // this lane's query row in phase 1
  const bool qvalid = qi < a.Tq;
  const int nkf = (T + 15) / 16;
  const float sl2 = a.scale * 1.4426950408889634f; // fold log2(e): p = exp2(s * sl2 - m)
  const u32x4 z4 = {0u, 0u, 0u, 0u};

  // K fragments of head h for this wave: fragment i = key rows 16 (4i + wave) + c, dims 32kk + 8q ..
  // Two heads' fragments are held: head h + 2 is requested as soon as head h's MFMAs have their operands.
  u32x4 k0[RO_WF][2], q0[2], k1[RO_WF][2], q1[2];
  auto fetch = [&](int h, u32x4 (&kreg)[RO_WF][2], u32x4 (&qreg)[2]) {
    const int koff = (a.H + h) * RO_DH;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
      qreg[kk] = qvalid ? *(const u32x4*)(base + (long)qi * ld + h * RO_DH + 32 * kk + 8 * q) : z4;
#pragma unroll
    for (int i = 0; i < RO_WF; ++i) {
      const int key = 16 * (4 * i + wave) + c;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        kreg[i][kk] = key < T ? *(const u32x4*)(base + (long)key * ld + koff + 32 * kk + 8 * q) : z4;
    }
  };
  f32x4 acc[RO_WF];
#pragma unroll
  for (int i = 0; i < RO_WF; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto head = [&](int h, u32x4 (&kreg)[RO_WF][2], u32x4 (&qreg)[2]) {
    const s16x8 qf[2] = {__builtin_bit_cast(s16x8, qreg[0]), __builtin_bit_cast(s16x8, qreg[1])};
    // S^T[key 16 (4i + wave) + 4q + r][query c]
    f32x4 s[RO_WF];
#pragma unroll
    for (int i = 0; i < RO_WF; ++i) {
      s[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) s[i] = mfma16(__builtin_bit_cast(s16x8, kreg[i][kk]), qf[kk], s[i]);
    }
    if (h + 2 < a.H) fetch(h + 2, kreg, qreg);
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < RO_WF; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = 16 * (4 * i + wave) + 4 * q + r;
        const float v = key < T ? s[i][r] * sl2 : -INFINITY;
        s[i][r] = v;
        m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    const float mu = m == -INFINITY ? 0.f : m;     // a wave whose keys are all masked: p = 0, l = 0
    float l = 0.f;
#pragma unroll
    for (int i = 0; i < RO_WF; ++i)
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
    // the full row: maximum over the four waves, sum in wave order
    float mw[4], lw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) { mw[w] = redm[par][w][c]; lw[w] = redl[par][w][c]; }
    const float M = fmaxf(fmaxf(mw[0], mw[1]), fmaxf(mw[2], mw[3]));   // key 0 is real: M is finite
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) L += lw[w] * __builtin_amdgcn_exp2f(mw[w] - M);
    const float f = __builtin_amdgcn_exp2f(m - M) / L;
#pragma unroll
    for (int i = 0; i < RO_WF; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][r] += s[i][r] * f;
  };
  fetch(0, k0, q0);
  if (a.H > 1) fetch(1, k1, q1);
  for (int h = 0; h < a.H; h += 2) {               // H is the same for every wave: the barriers inside match
    head(h, k0, q0);
    if (h + 1 < a.H) head(h + 1, k1, q1);
  }

  // A^ rows: (mean over the heads + I) / 2
  const float hs = 0.5f / (float)a.H;
#pragma unroll
  for (int i = 0; i < RO_WF; ++i) {
    const int kf = 4 * i + wave;
    if (kf >= nkf) continue;
    const int key0 = 16 * kf + 4 * q;
    float4 v;
    v.x = acc[i][0] * hs + (key0 == qi ? 0.5f : 0.f);
    v.y = acc[i][1] * hs + (key0 + 1 == qi ? 0.5f : 0.f);
    v.z = acc[i][2] * hs + (key0 + 2 == qi ? 0.5f : 0.f);
    v.w = acc[i][3] * hs + (key0 + 3 == qi ? 0.5f : 0.f);
    if (a.r_in) {
      *(float4*)(ahat + c * RO_AS + key0) = v;
    } else if (qvalid) {
      float* row = a.r_out + ((long)b * T + qi) * a.ldr + key0;
      if (key0 + 3 < T) {
        *(float4*)row = v;
      } else {
        if (key0 < T) row[0] = v.x;
        if (key0 + 1 < T) row[1] = v.y;
        if (key0 + 2 < T) row[2] = v.z;
      }
    }
  }
  if (!a.r_in) return;
  __syncthreads();

  // R_out[16 rows][T] = A^ R_in. Wave w owns the 64 columns from 64w on; lane c holds the columns
  // 64w + 4c + i, one per accumulator tile i = 0..3, so its four B values of a k-step are ONE
  // 16-byte load of r_in (a wave reads 4 rows x 256 contiguous bytes) and its four results of an
  // output row one 16-byte store. k runs upwards, k = 4ks + q inside a step.
  if (64 * wave >= T) return;                      // no columns (the last barrier is behind us)
  const int j0 = 64 * wave + 4 * c;                // j0 < T and ldr % 4 == 0: the 16 bytes lie inside the row stride
  const bool cok[4] = {j0 < T, j0 + 1 < T, j0 + 2 < T, j0 + 3 < T};
  const float* rin = a.r_in + (long)b * T * a.ldr + (cok[0] ? j0 : 0);
  f32x4 o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nks = (T + 3) / 4;
  const float* ap = ahat + c * RO_AS + q;          // A^ is 0 at masked keys; no fragment past nkf is read (4 nks <= 16 nkf)
  constexpr int KC = 8;                            // k-steps per group: 8 loads in flight, the next group's behind them
  float4 b0[KC], b1[KC];
  auto load = [&](int ks0, float4 (&buf)[KC]) {
#pragma unroll
    for (int u = 0; u < KC; ++u) {
      const int k = min(4 * min(ks0 + u, nks - 1) + q, T - 1);      // clamped: always a row of the T x T block
      buf[u] = *(const float4*)(rin + (long)k * a.ldr);
    }
  };
  auto run = [&](int ks0, const float4 (&buf)[KC]) {
#pragma unroll
    for (int u = 0; u < KC; ++u) {
      if (ks0 + u >= nks) break;
      const bool kok = 4 * (ks0 + u) + q < T;      // what lies past T (padding, the clamped row) counts as 0
      const float av = ap[4 * (ks0 + u)];
      o[0] = mfma_f32(av, kok && cok[0] ? buf[u].x : 0.f, o[0]);
      o[1] = mfma_f32(av, kok && cok[1] ? buf[u].y : 0.f, o[1]);
      o[2] = mfma_f32(av, kok && cok[2] ? buf[u].z : 0.f, o[2]);
      o[3] = mfma_f32(av, kok && cok[3] ? buf[u].w : 0.f, o[3]);
    }
  };
  load(0, b0);
  for (int ks0 = 0; ks0 < nks; ks0 += 2 * KC) {
    if (ks0 + KC < nks) load(ks0 + KC, b1);
    run(ks0, b0);
    if (ks0 + 2 * KC < nks) load(ks0 + 2 * KC, b0);
    if (ks0 + KC < nks) run(ks0 + KC, b1);
  }
  // D tile i: [row 4q + r][column j0 + i]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = qt * RO_Q + 4 * q + r;
    if (row >= a.Tq || !cok[0]) continue;
    float* dst = a.r_out + ((long)b * T + row) * a.ldr + j0;
    if (cok[3]) {
      *(float4*)dst = make_float4(o[0][r], o[1][r], o[2][r], o[3][r]);
    } else {
      dst[0] = o[0][r];
      if (cok[1]) dst[1] = o[1][r];
      if (cok[2]) dst[2] = o[2][r];
    }
  }
}

__global__ __launch_bounds__(256) void rollout_map_kernel(RolloutMapArgs a) {
  __shared__ float ws[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* r0 = a.r + (long)b * a.T * a.ldr;   // row 0 of the image's R
  float* row = a.out + (long)b * a.ldo;
  const float v = t + 1 < a.T ? r0[t + 1] : 0.f;
  float m = v;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) m = fmaxf(m, __shfl_xor(m, s, 64));
  if ((t & 63) == 0) ws[t >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(ws[0], ws[1]), fmaxf(ws[2], ws[3]));
  if (t + 1 < a.T) row[2 + t] = m > 0.f ? v / m : 0.f;
  if (t < 2) ((int32_t*)row)[t] = a.top[2 * b + t];   // class and score, as 32-bit words
}

static bool rollout_bad_ptr(const void* p, uintptr_t mask) { return !p || ((uintptr_t)p & mask); }

hipError_t attn_rollout(const AttnRolloutArgs& a, hipStream_t s) {
  if (a.dh != RO_DH || a.T < 1 || a.T > kRolloutMaxT || a.H < 1 || a.B < 1) return hipErrorInvalidValue;
  if (a.Tq < 1 || a.Tq > a.T || a.ldr < a.T || a.ldr % 4 != 0) return hipErrorInvalidValue;
  if (rollout_bad_ptr(a.qkv, 15) || rollout_bad_ptr(a.r_out, 15) || ((uintptr_t)a.r_in & 15) || a.r_in == a.r_out)
    return hipErrorInvalidValue;
  const long nwg = (long)a.B * ((a.Tq + RO_Q - 1) / RO_Q);
  if (nwg > 0x7fffffffL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_rollout_kernel, dim3((unsigned)nwg), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t rollout_map(const RolloutMapArgs& a, hipStream_t s) {
  if (a.T < 2 || a.T > kRolloutMaxT || a.B < 1) return hipErrorInvalidValue;
  if (a.ldr < a.T || a.ldr % 4 != 0 || a.ldo < a.T + 1) return hipErrorInvalidValue;
  if (rollout_bad_ptr(a.r, 3) || rollout_bad_ptr(a.top, 3) || rollout_bad_ptr(a.out, 3)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rollout_map_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
