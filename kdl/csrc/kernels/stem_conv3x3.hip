// Xception block1_conv1 fused into block1_conv2: the 3x3/2 'valid' stem conv (uint8 image,
// 3 -> 32, + bias + ReLU) is computed per tile of the following 3x3 'valid' conv (32 -> N,
// + bias + ReLU) instead of being written to memory by one launch and read back by the next.
//
// Derived from conv3x3_2dw_kernel (conv3x3_2d.hip): the compute waves, their register-resident
// 9 x FN weight fragments, the LDS patch layout (4 planes of 8 channels, slot = pr*PW + pc), the
// ring, the one barrier per tile and the direct epilogue are the same. The single DMA wave is
// replaced by NP PRODUCER waves that build a stage's (TH+2) x (TW+2) patch of stem pixels from
// the image: per 16-pixel fragment the two row-run k-steps of stem_rows_kernel (stem.hip; same
// packed weights, operand roles and k-step order, so the bf16 values are bit-identical to the
// stem1 tensor of the two-launch lowering), bias + ReLU, and one 8-byte LDS store per lane and
// output fragment. A lane's 8 k-slots are 8 consecutive image bytes, fetched as in
// stem_rows_kernel (aligned 12-byte load + v_alignbyte). A producer reduces the loaded bytes of
// the tile it builds to 2 dwords per k-step, requests the next tile's bytes into the same
// registers, and only then converts, multiplies and stores, so that work and the barrier hide
// the load latency (measured: 55 -> 52 us per launch at batch 32; requesting them after the
// build left the whole latency between the barrier and the build). The producers' vmcnt holds
// only those loads and the compute waves' only their output stores. With 2 producer waves the
// producers are the critical path (74 us), with 4 the launch takes 52 us against 47 + 27 us
// for the two launches it replaces (profiles/stem_fused.txt).
//
// LDS stores: the 16 lanes of a ds_write_b64 group hold 16 consecutive slots (16-byte stride,
// 8 bytes each): 2-way on the store's 32-bank view, 24 stores per tile -- nothing is staged
// through LDS besides the patch itself. Patch pixels outside the stem map (ragged tiles) are
// computed from clamped coordinates: finite values that only feed outputs never stored.
#include "common.h"
#include "launch.h"

#include <algorithm>

namespace kdl {

template <int FM, int FN, int WGM, int WGN, int STAGES, int TH, int TW, int NP>
__global__ __launch_bounds__(64 * (WGM * WGN + NP)) void stem_conv3x3_kernel(StemConvArgs a) {
  constexpr int NW = WGM * WGN;
  constexpr int BM = 16 * FM * WGM;
  static_assert(BM == TH * TW && TW % 16 == 0, "the M tile is TH x TW pixels, 16-pixel row segments");
  static_assert(STAGES >= 2 && NP >= 1, "ring depth; producer waves");
  constexpr int PW = TW + 2, PS = (TH + 2) * PW;
  constexpr int IPP = (PS + 63) / 64;
  constexpr int PL = IPP * 1024;                // bytes per plane of 8 channels
  constexpr int STAGE = 4 * PL;
  constexpr int NFRAG = (PS + 15) / 16;         // 16-pixel stem fragments per patch (<= IPP * 4)
  constexpr int FPP = (NFRAG + NP - 1) / NP;    // fragments per producer wave
  constexpr int L = STAGES - 1;                 // tiles the producers run ahead
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* const ring = smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int OH = a.OH, OW = a.OW;
  const int ntw = (OW + TW - 1) / TW, nth = (OH + TH - 1) / TH;
  const int ntiles = a.B * nth * ntw;
  const int G = gridDim.x;
  const int t0 = xcd_remap(blockIdx.x, G);
  const int Q = t0 < ntiles ? (ntiles - t0 + G - 1) / G : 0;   // tiles (= stages) of this workgroup
  if (Q == 0) return;                           // uniform per workgroup; nothing issued yet
  const int p16 = lane & 15, quad = lane >> 4;

  if (wave >= NW) {
    // ---- producer waves: fragment f = pw + i * NP of the patch, lane -> stem pixel slot f*16 + p16
    const int pw = wave - NW;
    const int H = a.H, W = a.W, H1 = a.H1, W1 = a.W1;
    const long total = (long)a.B * H * W * 3, img = (long)H * W * 3;
    s16x8 bw[2][2];                             // stem weights [fragment j][k-step]
    float4 bv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) bw[j][ks] = *(const s16x8*)(a.wp1 + ((j * 2 + ks) * 64 + lane) * 8);
      bv[j] = *(const float4*)(a.b1 + 16 * j + 4 * quad);
    }
    // a use the compiler sees: it waits for the weights and bias HERE. Otherwise its counted waits
    // before their first use inside the tile loop also cover the image bytes just requested there.
#pragma unroll
    for (int j = 0; j < 2; ++j)
      asm volatile("" ::"v"(bw[j][0]), "v"(bw[j][1]), "v"(bv[j].x), "v"(bv[j].y), "v"(bv[j].z), "v"(bv[j].w));
    // row-run K layout (k = ky*16 + kx*3 + c): k-step ks, lane quad -> kernel row 2*ks + quad/2,
    // bytes rq .. rq+7 of its 9-byte run (rq = 8: one byte, the other slots zero; row 3: all zero).
    // Byte offsets are 32-bit within the image (the launcher bounds H*W*3); only the image base is
    // 64-bit, and it is wave-uniform.
    const int rq = 8 * (quad & 1);
    const int W6 = 6 * W;
    const int lane_off = rq + (quad >> 1) * 3 * W;            // row ky = quad/2 of k-step 0; k-step 1: + 2 rows
    const uint32_t m0 = rq ? 0xffu : ~0u, m1 = rq ? 0u : ~0u;  // valid bytes of the lane's 8 (k-step 0)
    const bool row2 = quad < 2;                               // k-step 1: kernel row 2 (quads 0, 1) or none
    int pr[FPP], pc[FPP], lo[FPP];
#pragma unroll
    for (int i = 0; i < FPP; ++i) {
      const int s = (pw + i * NP) * 16 + p16;
      const int sc = min(s, PS - 1);
      pr[i] = sc / PW;
      pc[i] = sc - pr[i] * PW;
      lo[i] = (quad >> 1) * PL + s * 16 + (quad & 1) * 8;   // channels 4*quad .. +3; fragment 1: + 2 planes
    }
    // The image bytes of the next tile to build. build() first reduces them to the lane's 8 masked
    // bytes per k-step, then issues the loads of the tile after it into the same registers, and only
    // then converts, multiplies and stores: that work and the wait at the barrier hide the latency.
    typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
    typedef u32x3 u32x3_a4 __attribute__((aligned(4)));
    u32x3 d[FPP][2];                            // one 12-byte load each: kept whole, so the loop carries the
                                                // load's own register triple (no copies that would wait on it)
    int tt[FPP][2];                             // first byte of the lane's 8 (from xb); bit 31: checked path
    const uint8_t* xb = a.x;                    // 4-byte aligned address, at most 3 bytes before the tile's image
    int rem = 0;                                // bytes from xb to the end of the batch
    auto load = [&](int tq) {
      const int tile = t0 + tq * G;
      const int bimg = tile / (nth * ntw), trem = tile - bimg * (nth * ntw);
      const int h0 = (trem / ntw) * TH, w0 = (trem % ntw) * TW;
      const long sbase = bimg * img;
      const uintptr_t ia = (uintptr_t)a.x + sbase;   // the image's address: aligned base + low bits (a.x may
      const int sb_lo = (int)(ia & 3);               // be any byte of a larger buffer: a lane's share of a batch)
      xb = (const uint8_t*)(ia - sb_lo);
      rem = (int)std::min(total - sbase + sb_lo, (long)0x7fffffff);
      const int last = (rem - 12) & ~3;         // the last aligned 12 bytes that are all inside (rem >= 147)
#pragma unroll
      for (int i = 0; i < FPP; ++i) {
        if (pw + i * NP >= NFRAG) continue;
        const int r = min(h0 + pr[i], H1 - 1), c = min(w0 + pc[i], W1 - 1);
        const int t0b = r * W6 + c * 6 + lane_off + sb_lo;     // first byte of the lane's 8, k-step 0
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          // k-step 1 of quads 2, 3 (no kernel row 3) is masked to zero in build(): re-read k-step 0's bytes
          const int t = t0b + (ks == 1 && row2 ? W6 : 0);
          const int al = t & ~3;
          // the last bytes of the batch: an aligned 12-byte load could end past them. Load the last
          // whole 12 bytes instead (branch-free here) and let build() fetch the lane's bytes one by one
          const bool over = al + 12 > rem;
          d[i][ks] = *(const u32x3_a4*)(xb + (over ? last : al));
          tt[i][ks] = over ? (t | (int)0x80000000) : t;
        }
      }
    };
    auto build = [&](int slotbuf, int next) {
      uint8_t* base = ring + slotbuf * STAGE;
      uint32_t w[FPP][2][2];
#pragma unroll
      for (int i = 0; i < FPP; ++i) {
        if (pw + i * NP >= NFRAG) continue;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          uint32_t d0 = d[i][ks][0], d1 = d[i][ks][1], d2 = d[i][ks][2];
          const int t = tt[i][ks] & 0x7fffffff;
          uint32_t sh = t & 3;
          if (tt[i][ks] < 0) {                  // checked byte loads (only lanes at the end of the batch)
            uint32_t w0b = 0u, w1b = 0u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const uint32_t v = t + j < rem ? xb[t + j] : 0u;
              if (j < 4) w0b |= v << (8 * j); else w1b |= v << (8 * (j - 4));
            }
            d0 = w0b; d1 = w1b; d2 = 0u; sh = 0u;
          }
          // the invalid slots are masked as bytes: 0 -> 0.0f -> bf16 0, as stem_rows_kernel's select
          // gives; a byte value is exact in bf16, so the packed conversion equals the single one
          const uint32_t k0 = ks == 0 || row2 ? m0 : 0u, k1 = ks == 0 || row2 ? m1 : 0u;
          w[i][ks][0] = __builtin_amdgcn_alignbyte(d1, d0, sh) & k0;
          w[i][ks][1] = __builtin_amdgcn_alignbyte(d2, d1, sh) & k1;
        }
      }
      if (next >= 0) load(next);
#pragma unroll
      for (int i = 0; i < FPP; ++i) {
        if (pw + i * NP >= NFRAG) continue;
        f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          u32x4 pk;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t wd = w[i][ks][j >> 1];
            pk[j] = pack_bf16((float)((wd >> (16 * (j & 1))) & 0xffu), (float)((wd >> (16 * (j & 1) + 8)) & 0xffu));
          }
          const s16x8 af = __builtin_bit_cast(s16x8, pk);
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[j] = mfma16(bw[j][ks], af, acc[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const float v0 = fmaxf(acc[j][0] + bv[j].x, 0.f), v1 = fmaxf(acc[j][1] + bv[j].y, 0.f);
          const float v2 = fmaxf(acc[j][2] + bv[j].z, 0.f), v3 = fmaxf(acc[j][3] + bv[j].w, 0.f);
          *(u32x2*)(base + 2 * j * PL + lo[i]) = (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)};
        }
      }
    };
    // tiles 0 .. L-1 before the first barrier; then tile q+L into the slot of stage q-1
    load(0);
    for (int p = 0; p < L; ++p)
      if (p < Q) build(p, p + 1 < Q ? p + 1 : -1);
    for (int q = 0; q < Q; ++q) {
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage q published
      if (q + L < Q) build((q + L) % STAGES, q + L + 1 < Q ? q + L + 1 : -1);
    }
    return;
  }

  // ---- compute waves: the 9 taps x FN weight fragments of this wave's columns, in registers
  const int wm = wave / WGN, wn = wave % WGN;
  s16x8 bw[9][FN];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < FN; ++j)
      bw[t][j] = *(const s16x8*)(a.wp2 + (((long)(wn * FN + j) * 9 + t) * 64 + lane) * 8);
  const int kb = quad, col = p16;
  float4 bvr[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) bvr[j] = *(const float4*)(a.b2 + wn * FN * 16 + j * 16 + 4 * quad);
  int aoff[FM], prow[FM], pcol[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int pix = (wm * FM + i) * 16 + p16;
    const int r = pix / TW, c = pix - r * TW;
    aoff[i] = kb * PL + (r * PW + c) * 16;
    const int op = (wm * FM + i) * 16 + col;    // output pixel of this lane's accumulator rows
    prow[i] = op / TW;
    pcol[i] = op - prow[i] * TW;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // weights + bias in registers

  for (int q = 0; q < Q; ++q) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");   // stage q published by the producers
    const uint8_t* pb = ring + (q % STAGES) * STAGE;
    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int toff = ((t / 3) * PW + t % 3) * 16;
      s16x8 af[FM];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *(const s16x8*)(pb + aoff[i] + toff);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(bw[t][j], af[i], acc[i][j]);
    }
    // ---- epilogue straight from the accumulators: lane holds 4 consecutive channels of
    // one output pixel per fragment (8-byte stores; the XCD L2 merges the row segments)
    const int tile = t0 + q * G;
    const int bimg = tile / (nth * ntw), trem = tile - bimg * (nth * ntw);
    const int h0 = (trem / ntw) * TH, w0 = (trem % ntw) * TW;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int h = h0 + prow[i], w = w0 + pcol[i];
      if (h < OH && w < OW) {
        uint16_t* yrow = a.y + ((long)(bimg * OH + h) * OW + w) * a.ldy;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = wn * FN * 16 + j * 16 + 4 * quad;
          float v0 = acc[i][j][0] + bvr[j].x, v1 = acc[i][j][1] + bvr[j].y;
          float v2 = acc[i][j][2] + bvr[j].z, v3 = acc[i][j][3] + bvr[j].w;
          if (a.relu_out == 1) {
            v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
          }
          if (n < a.nstore) *(u32x2*)(yrow + n) = (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)};
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// (id, FM, FN, WGM, WGN, STAGES, TH, TW, NP): the tile of conv3x3_2dw's config 7 (block1_conv2's
// tuned entry) with 2 or 4 producer waves and a 2- or 3-deep ring.
#define KDL_SC3_CONFIGS(X)            \
  X(0, 2, 4, 4, 1, 2, 8, 16, 4)       \
  X(1, 2, 4, 4, 1, 2, 8, 16, 2)       \
  X(2, 2, 4, 4, 1, 3, 8, 16, 4)       \
  X(3, 2, 4, 4, 1, 3, 8, 16, 2)

static int sc3_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
  }
  return n;
}

template <int FM, int FN, int WGM, int WGN, int ST, int TH, int TW, int NP>
static hipError_t launch_sc3(const StemConvArgs& a, hipStream_t s) {
  constexpr int BN = 16 * FN * WGN, NT = 64 * (WGM * WGN + NP);
  // uint8 image, 3 -> 32 'valid' stride 2, then 32 -> BN 'valid' stride 1: one N tile holding all outputs
  if (!a.x || !a.wp1 || !a.b1 || !a.wp2 || !a.b2 || !a.y || a.B <= 0 || a.H < 7 || a.W < 7 ||
      a.H1 != (a.H - 3) / 2 + 1 || a.W1 != (a.W - 3) / 2 + 1 || a.OH != a.H1 - 2 || a.OW != a.W1 - 2 ||
      a.NF * 16 != BN || a.nstore <= 0 || a.nstore > a.ldy || a.nstore % 4 || a.ldy % 4 || a.relu_out < 0 ||
      a.relu_out > 1 || a.grid < 0 || (long)a.B * a.OH * a.OW > 0x7fffffffL ||
      (long)a.H * a.W * 3 > (1L << 30))   // 32-bit byte offsets within an image
    return hipErrorInvalidValue;
  constexpr int PS = (TH + 2) * (TW + 2), IPP = (PS + 63) / 64;
  const size_t smem = (size_t)ST * 4 * IPP * 1024;
  const int ntiles = a.B * ((a.OH + TH - 1) / TH) * ((a.OW + TW - 1) / TW);
  // resident workgroups per CU of THIS kernel: the tiles are dealt out statically, so a
  // workgroup that is not resident is pure tail
  static int per_cu = 0;
  if (per_cu == 0) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, stem_conv3x3_kernel<FM, FN, WGM, WGN, ST, TH, TW, NP>, NT,
                                                     smem) != hipSuccess || n <= 0)
      n = 1;
    per_cu = n;
  }
  int grid = std::min(ntiles, sc3_num_cus() * per_cu);
  if (a.grid > 0) grid = std::min(grid, a.grid);
  hipLaunchKernelGGL((stem_conv3x3_kernel<FM, FN, WGM, WGN, ST, TH, TW, NP>), dim3(grid), dim3(NT), smem, s, a);
  return hipGetLastError();
}

int stem_conv3x3_config(int cfg, int* bm, int* bn, int* threads) {
  switch (cfg) {
#define KDL_SC3INFO(id, fm, fn, wgm, wgn, st, th, tw, np) \
  case id: *bm = 16 * fm * wgm; *bn = 16 * fn * wgn; *threads = 64 * (wgm * wgn + np); return 0;
    KDL_SC3_CONFIGS(KDL_SC3INFO)
#undef KDL_SC3INFO
    default: return -1;
  }
}

hipError_t stem_conv3x3(int cfg, const StemConvArgs& a, hipStream_t s) {
  switch (cfg) {
#define KDL_SC3CASE(id, fm, fn, wgm, wgn, st, th, tw, np) \
  case id: return launch_sc3<fm, fn, wgm, wgn, st, th, tw, np>(a, s);
    KDL_SC3_CONFIGS(KDL_SC3CASE)
#undef KDL_SC3CASE
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kdl
