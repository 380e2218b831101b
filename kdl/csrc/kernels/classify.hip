// Classification outputs: softmax + top-k of the head's fp32 logits (launch.h TopkArgs).
// One wave per image, four images per 256-thread workgroup, no LDS and no barrier: the
// image's logits sit in registers (R = ceil(NC / 64) per lane, logit i in lane i % 64,
// register i / 64, so the loads are coalesced), and each of the K rounds is a lane-local scan
// plus a wave-wide (value, index) arg-max butterfly. A picked logit is marked in a per-lane
// taken mask instead of being overwritten, so -inf logits still rank by index. Round 0's value
// is the softmax max; the denominator is summed lane-locally in register order, then by the
// same fixed butterfly: deterministic. At 32 x 1000 logits the kernel is a rounding error of
// the forward (profiles/classify_topk.txt).
#include <climits>

#include "common.h"
#include "launch.h"

namespace kdl {

template <int R>
__global__ __launch_bounds__(256) void softmax_topk_kernel(TopkArgs a) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= a.B) return;                       // whole waves leave; nothing below crosses waves
  const float* xb = a.x + (long)b * a.ldx;
  float v[R];
  unsigned taken = 0;                         // bit r: register r is out of range or already picked
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = r * 64 + lane;
    const bool ok = i < a.NC;
    v[r] = ok ? xb[i] : -INFINITY;
    if (!ok) taken |= 1u << r;
  }
  float mx = 0.f, sum = 0.f, myv = 0.f;
  int myi = 0;
  for (int k = 0; k < a.K; ++k) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int r = 0; r < R; ++r) {              // ascending index: '>' keeps the first of equals
      const bool free_ = !((taken >> r) & 1u);
      if (free_ && (bi == INT_MAX || v[r] > bv)) { bv = v[r]; bi = r * 64 + lane; }
    }
    topk_wave_best(bv, bi);                   // every lane now holds the same winner
    if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
    if (k == 0) {
      mx = bv;
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) s += (r * 64 + lane < a.NC) ? expf(v[r] - mx) : 0.f;
#pragma unroll
      for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
      sum = s;
    }
    if (lane == k) { myv = bv; myi = bi; }
  }
  if (lane < a.K) {
    int32_t* o = a.out + (long)b * 2 * a.K;
    o[lane] = myi;
    reinterpret_cast<float*>(o)[a.K + lane] = expf(myv - mx) / sum;
  }
}

hipError_t softmax_topk(const TopkArgs& a, hipStream_t s) {
  if (!a.x || !a.out || a.B < 1 || a.NC < 1 || a.NC > kTopkMaxNC || a.K < 1 || a.K > a.NC ||
      a.K > kTopkMaxK || a.ldx < a.NC)
    return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.B + 3) / 4));
#define KDL_TOPK(r)                                                             \
  if (a.NC <= 64 * r) {                                                         \
    hipLaunchKernelGGL(softmax_topk_kernel<r>, grid, dim3(256), 0, s, a);       \
    return hipGetLastError();                                                   \
  }
  KDL_TOPK(1) KDL_TOPK(2) KDL_TOPK(4) KDL_TOPK(8) KDL_TOPK(16)
#undef KDL_TOPK
  return hipErrorInvalidValue;
}

}  // namespace kdl
