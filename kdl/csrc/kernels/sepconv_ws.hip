// Warp-specialized fused SeparableConv2D (+BN)(+ReLU in/out)(+residual) for CDNA4: the
// Xception middle flow (19x19x728 -> 728, 24 layers) and the exit flow's first layers.
//
// Math: the depthwise 3x3 runs on the matrix cores. For a 16-pixel x 16-channel unit, one
// v_mfma_f32_16x16x32_bf16 multiplies a block-diagonal weight operand (two taps x 16
// channels, built from a 16-byte weight entry with v_perm) by the 32 staged input values
// of those taps: 5 MFMAs cover the 9 taps (the 10th tap slot reads a zero slot). Its
// output, bf16, is the A operand of the pointwise GEMM (BN scale folded into the packed
// pointwise weights, BN shift = bias). The x band (every 3x3 neighbour of the tile's
// BM raster pixels: BM + 2W + 2 pixels) is staged by LDS-DMA into a STAGES-deep ring,
// one 32-channel k-step per stage; the depthwise output never leaves the CU.
//
//   waves 0-3  "consumers": the pointwise GEMM. Each owns a BM x BN/4 output slab (FM x FN
//              fragments of 16x16). Its pointwise-weight fragments are used by no other
//              wave, so they skip LDS: global_load_dwordx4 of the packed, lane-linear
//              1 KiB fragments straight into registers, two k-steps ahead (double set,
//              loop unrolled by 2). Consumers also issue the LDS-DMA of the x band.
//   waves 4-7  "producers": LDS-DMA of the depthwise weight entries, and the depthwise of
//              the NEXT k-step on the matrix cores (FM/2 units of 16 px x 16 ch each),
//              written as bf16 into the fragment-linear A double buffer.
//
// Measured on the Xception middle-flow shape with in-kernel s_memtime stamps
// (tools/stamps.py): with every wave doing everything, the phases of the two waves of a
// SIMD serialize; with the roles split but the pointwise weights staged through LDS, LDS
// traffic (DMA writes + 112 KiB of ds_read per k-step) made every LDS read wait ~900
// cycles. Waves go to SIMDs in the cyclic order 0->2->1->3 (MI355X_MICROARCH.md §LDS), so
// waves w and w+4 share a SIMD: every SIMD hosts one consumer and one producer.
//
// Synchronisation: one barrier per k-step. Band stage s lands in ring slot s % STAGES;
// every wave waits for ITS OWN outstanding loads with a counted vmcnt (consumer: band
// DMA + B register loads in issue order; producer: weight DMA), then the barrier
// publishes the stage. Producers write A[(t+1)&1] while consumers read A[t&1].
// The loop runs an even number of steps; a padding step multiplies a zero A, and the
// branch-free loop keeps loading (the last stage again) past the last real one. TAIL
// builds do neither: their loop ends with the last step whose loads are all real, and
// the remaining STAGES - 1 steps follow it peeled, each with the loads that still exist
// and its own wait count (see ws_tile).
#include "common.h"
#include "launch.h"
#include "epilogue.h"

#include <algorithm>
#include <type_traits>

namespace kdl {

// zeros for band slots beyond the staged pixels (K <= 8192); one per translation unit
__device__ __attribute__((aligned(16))) uint8_t sepw_zeros[16384];

// vmcnt(N) + barrier through builtins (not inline asm): the compiler's waitcnt pass then
// knows at most N loads are outstanding after it and does not add its own conservative
// vmcnt(0) before the first use of the register-resident B fragments
template <int N>
__device__ __forceinline__ void ws_wait() {
  static_assert(N < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}
template <int N>
__device__ __forceinline__ void ws_wait_barrier() {
  ws_wait<N>();
  __builtin_amdgcn_s_barrier();
}

template <int V> using ws_int = std::integral_constant<int, V>;

// f(ws_int<I>{}) for I = LO .. HI - 1, unrolled at compile time (TAIL's peeled steps)
template <int LO, int HI, class F>
__device__ __forceinline__ void ws_static_for(F&& f) {
  if constexpr (LO < HI) {
    f(ws_int<LO>{});
    ws_static_for<LO + 1, HI>(f);
  }
}

// LDS bytes of one workgroup of the configuration (the tile body's layout). ZF: every stage
// ends in a 256-byte zero block that out-of-map taps read (see ws_tile)
template <int FM, int FN, int STAGES, int XB, bool ZF = false>
struct WsSmem {
  static constexpr int RING = STAGES * ((XB + 1) * 1024 + (ZF ? 256 : 0));
  static constexpr int PIPE = RING + 2 * FM * 1024;
  static constexpr int CTILE = 16 * FM * (64 * FN * 2 + 16);
  static constexpr int BYTES = PIPE > CTILE ? PIPE : CTILE;
};

// One BM x BN output tile of a fused separable conv: the whole body of sepconv_ws_kernel.
// ABL (timing ablations, never candidates; wrong values):
//   1 = every band glds reads 1 KiB contiguous (8 full lines) instead of 64 pixels x 16 B (64
//       lines) -- the same loads and bytes, so the counted-vmcnt protocol is untouched;
//   2 = producers skip their band LDS reads (taps from registers); 4 = producers skip the
//       depthwise MFMAs; 8 = producers skip the A-buffer writes. Each removes LDS / matrix-pipe
//       work only: every wave still issues and waits for exactly the same global loads.
// ZF: out-of-map taps (image borders, the 10th tap slot) read a per-stage 256-byte zero block
// at the 16-byte slot of the same bank as the in-map address would have, instead of one
// shared zero slot: that slot's bank collided with a live lane of the same ds_read_b128 lane
// group (2-way conflicts on most dx != 0 taps).
// TAIL: no padding step and no load of a stage >= KT. With r = KT - t steps left, step t issues
// band(t + STAGES - 1) only while r >= STAGES and B(t + 2) only while r >= 3, so the loop covers
// r >= STAGES and the steps r = STAGES - 1 .. 1 are peeled behind it (no branch inside the loop
// body: see the producers' issue). The two waves' wait counts, by the same rule as the loop's
// (everything but the previous step's loads has landed):
//   consumer  LCB * [r >= STAGES - 1] + FN * [r >= 2]      producer  clamp(r - 3, 0, STAGES - 4)
// KT < STAGES has no step of the loop's kind: a prologue of KT stages, then one step at a time.
template <int FM, int FN, int STAGES, int XB, bool STAMP, bool KROT, bool RELU, int ABL = 0, bool ZF = false,
          bool TAIL = false>
__device__ __forceinline__ void ws_tile(const ConvGemmArgs& a, int mi, int ni, uint8_t* smem) {
  constexpr int NT = 512;
  constexpr int BM = 16 * FM, BN = 64 * FN;
  constexpr int AF = FM;
  constexpr int NSP = 16 * XB, PL = NSP * 16, ZSLOT = NSP - 1;   // band plane: slots, bytes
  // [band XB KiB][depthwise weight entries 1 KiB][ZF: zero block 256 B]
  constexpr int STAGE = (XB + 1) * 1024 + (ZF ? 256 : 0);
  constexpr int ZOFF = (XB + 1) * 1024;
  constexpr int WOFF = XB * 1024;
  constexpr int RING = STAGES * STAGE;
  constexpr int ABUF = AF * 1024;
  constexpr int CS = BN * 2 + 16;
  constexpr int SMEM_PIPE = RING + 2 * ABUF;
  constexpr int SMEM = SMEM_PIPE > BM * CS ? SMEM_PIPE : BM * CS;
  constexpr int LCB = (XB + 3) / 4;              // band glds per consumer per stage (surplus re-issues)
  constexpr int UPW = FM / 2;                    // depthwise units per producer wave
  // consumer, top of step t: needs B(t) (loaded in step t-2) and band(t+2) (issued in step
  // t+3-STAGES <= t-2; producers read it during step t): everything up to step t-2, so only
  // the LCB + FN loads of step t-1 may still be in flight
  constexpr int WC = LCB + FN;
  static_assert(FM % 2 == 0 && STAGES >= 5, "layout / pipeline depth");
  static_assert(SMEM == WsSmem<FM, FN, STAGES, XB, ZF>::BYTES, "LDS map");
  static_assert(!ZF || (STAGE % 256 == 0 && ZOFF % 256 == 0), "zero block bank alignment");

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool consumer = wave < 4;
  const int W = a.W, H = a.H;
  const long NPIX = (long)a.B * H * W;
  const int m0 = mi * BM, n0 = ni * BN;
  const int KT = a.K >> 5;
  const int KTE = (KT + 1) & ~1;                 // even step count (unroll by 2)
  // band: raster pixels P0 .. P0+NS-1 = every 3x3 neighbour of the tile's pixels, as 4
  // planes (one per 8-channel chunk) of NSP 16-byte slots; slot NSP-1 stays zero
  const long P0 = (long)m0 - W - 1;
  // KROT: every M tile walks K from its own starting chunk (the two N tiles of an M tile
  // share it, so their band reads stay L2-shared): without it all workgroups fetch the
  // same weight fragments at the same time
  int krot = 0;
  if constexpr (KROT) {
    // a.krot > 0: the multiplier (tools probes); 0: 7
    krot = (mi * (a.krot > 0 ? a.krot : 7)) % KT;
  }
  auto kc = [&](int t) {
    // TAIL without KROT: the step index stays a scalar the addresses are computed from, as in the KROT
    // builds (as an induction variable hipcc kept one running pointer per load of the peeled steps too,
    // and spilled seven of them inside the loop)
    if constexpr (TAIL && !KROT) asm("" : "+s"(t));
    t = (TAIL ? t : min(t, KT - 1)) + krot;
    return t >= KT ? t - KT : t;
  };
  const int NS = min(m0 + BM, a.M) - m0 + 2 * W + 2;

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // STAMP variants: lane t keeps s_memtime after step t's barrier (st0) and at the end of
  // its work (st1); written out after the loop (no stores inside: they would count in vmcnt)
  unsigned long long st0 = 0, st1 = 0, tstart = 0;

  auto stamp = [&](unsigned long long& st, int t) {
    if constexpr (STAMP) {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      st = lane == t ? now : st;
    }
  };
  if constexpr (STAMP) tstart = __builtin_amdgcn_s_memtime();

  if (consumer) {
    // ================= consumer: pointwise GEMM on output columns wave*BN/4 ..
    const int wn = wave;
    const uint8_t* bsrc = (const uint8_t*)(a.wp + ((long)(n0 / 16 + wn * FN) * KT) * 512 + lane * 8);
    const long bstride = (long)KT * 1024;        // bytes between consecutive N fragments
    const uint8_t* xsrc[LCB];                    // band chunks: instruction s = wn + 4i covers chunks 64s..
#pragma unroll
    for (int i = 0; i < LCB; ++i) {
      const int c = min(wn + 4 * i, XB - 1) * 64 + lane;
      const int q = c / NSP, slot = c - q * NSP;
      long p = P0 + slot;
      p = p < 0 ? 0 : (p >= NPIX ? NPIX - 1 : p);
      xsrc[i] = slot < NS ? (const uint8_t*)(a.x + p * a.ldx + q * 8) : sepw_zeros;
      if constexpr (ABL & 1)
        xsrc[i] = (const uint8_t*)(a.x + (long)max(P0, 0L) * a.ldx) + (i * 64 + lane) * 16;
    }
    // stages past the end (the branch-free loop keeps issuing) re-load the last one (a scalar
    // clamp; a per-lane select to a zero block cost more VALU than the drain it saves)
    auto issue_band = [&](int t, int slot) {
      t = kc(t);
#pragma unroll
      for (int i = 0; i < LCB; ++i) glds16(xsrc[i] + t * 64, smem + slot * STAGE + min(wn + 4 * i, XB - 1) * 1024);
    };
    // B loads as inline asm: the compiler's waitcnt pass does not track them (it inserted a
    // conservative vmcnt(0) before their first use each iteration); the counted wait above covers them.
    // CONTRACT: every such load must be covered by ws_wait_barrier<WC> before ANY instruction
    // touches its destination registers, and every dword of each destination must stay live
    // until its MFMA (the compiler believes the asm wrote the register at issue: a dword it sees
    // as dead is re-allocated while the load is still in flight -- that was the round-2 GPU
    // fault of the removed "no pointwise MFMA" timing ablation, which read one dword of each
    // fragment). tools/vmcnt_check.py proves it on the built code (tests/test_vmcnt_hazards.py).
    auto gload = [&](s16x8& dst, const uint8_t* p) {
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
    };
    auto load_b = [&](int t, s16x8 (&b)[FN]) {
#pragma unroll
      for (int j = 0; j < FN; ++j) gload(b[j], bsrc + j * bstride + (long)kc(t) * 1024);
    };
    // nwait: loads that may still be in flight at the barrier; band / bload: the step issues
    // band(t + STAGES - 1) / B(t + 2) (always, except in TAIL's peeled steps)
    auto step = [&](int t, s16x8 (&b)[FN], auto nwait, auto band, auto bload) {
      constexpr bool BAND = decltype(band)::value, BLOAD = decltype(bload)::value;
      ws_wait_barrier<decltype(nwait)::value>();
      stamp(st0, t);
      const uint8_t* As = smem + RING + (t & 1) * ABUF + lane * 16;
      s16x8 af[FM];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = *(const s16x8*)(As + i * 1024);
      if constexpr (BAND) issue_band(t + STAGES - 1, (t + STAGES - 1) % STAGES);
      // B(t) is consumed fragment by fragment; each register set is refilled with B(t+2)
      // right behind its last MFMA
#pragma unroll
      for (int j = 0; j < FN; ++j) {
#pragma unroll
        for (int i = 0; i < FM; ++i) acc[i][j] = mfma16(b[j], af[i], acc[i][j]);
        if constexpr (BLOAD) gload(b[j], bsrc + j * bstride + (long)kc(t + 2) * 1024);
      }
      constexpr int NBJ = BAND ? LCB : 0;
      __builtin_amdgcn_sched_group_barrier(0x100, FM, 0);      // A fragment reads
#pragma unroll
      for (int j = 0; j < NBJ; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, FM, 0);    // MFMAs of fragment j
        __builtin_amdgcn_sched_group_barrier(0x010, 1 + BLOAD, 0);   // band DMA + B(t+2)_j
      }
#pragma unroll
      for (int j = NBJ; j < FN; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, FM, 0);
        if constexpr (BLOAD) __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);     // B(t+2)_j
      }
      if constexpr (STAMP) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stamp(st1, t);
      }
    };
    // prologue in need order: band(0..2), B(0), B(1), band(3..STAGES-2); the producers'
    // prologue reads band(0), band(1), step 0 needs band(2) and B(0) (covered by WC)
    s16x8 b0[FN], b1[FN];
    const std::true_type yes;
    auto steady = [&](int t, s16x8 (&b)[FN]) { step(t, b, ws_int<WC>{}, yes, yes); };
    if constexpr (!TAIL) {
      issue_band(0, 0);
      issue_band(1, 1);
      issue_band(2, 2);
      load_b(0, b0);
      load_b(1, b1);
#pragma unroll
      for (int p = 3; p < STAGES - 1; ++p) issue_band(p, p);
      ws_wait_barrier<(STAGES - 3) * LCB + 2 * FN>();   // band(0), band(1) landed
      for (int t = 0; t < KTE; t += 2) {
        steady(t, b0);
        steady(t + 1, b1);
      }
    } else if (KT >= STAGES) {
      // [front step, where nfull is even] [loop of step pairs b0, b1] [step nfull - 1 on b0] [peeled
      // steps r = STAGES - 1 .. 1 on b1, b0, b1, ..., step r being t = KT - r]. Counted back from the
      // peeled steps, step 0 takes b0 where nfull is odd (K = 736) and b1 where it is even: then B(0)
      // is loaded into b1, behind B(1), and the front step waits for both. One path of loads up to the
      // prologue barrier: tools/vmcnt_check.py follows every path, also mixes of two arms
      const int nfull = KT - (STAGES - 1);       // steps whose band(t + STAGES - 1) exists
      const int sw = (nfull & 1) ^ 1;
      issue_band(0, 0);
      issue_band(1, 1);
      issue_band(2, 2);
      load_b(sw, b0);
      load_b(sw ^ 1, b1);
      ws_static_for<3, STAGES - 1>([&](auto p) { issue_band(decltype(p)::value, decltype(p)::value); });
      ws_wait_barrier<(STAGES - 3) * LCB + 2 * FN>();   // band(0), band(1) landed
      int t = 0;
      if (sw) {
        step(0, b1, ws_int<(STAGES - 4) * LCB>{}, yes, yes);
        t = 1;
      }
      for (; t + 1 < nfull; t += 2) {
        steady(t, b0);
        steady(t + 1, b1);
      }
      steady(nfull - 1, b0);
      ws_static_for<0, STAGES - 1>([&](auto ic) {
        constexpr int i = decltype(ic)::value, r = STAGES - 1 - i;
        constexpr int N = (r >= STAGES - 1 ? LCB : 0) + (r >= 2 ? FN : 0);
        if constexpr (i % 2 == 0) step(KT - r, b1, ws_int<N>{}, std::false_type{}, std::bool_constant<(r >= 3)>{});
        else step(KT - r, b0, ws_int<N>{}, std::false_type{}, std::bool_constant<(r >= 3)>{});
      });
    } else {
      // KT < STAGES (no layer of the models): the stages that exist, then one step at a time behind
      // all loads. B comes through plain loads here, which hipcc counts itself: an asm load under a
      // condition has paths on which hipcc sees its destination dead, and re-uses it
      ws_static_for<0, STAGES - 1>([&](auto p) { if (decltype(p)::value < KT) issue_band(decltype(p)::value, decltype(p)::value); });
      ws_wait_barrier<0>();
      for (int t = 0; t < KT; ++t) {
#pragma unroll
        for (int j = 0; j < FN; ++j) b0[j] = *(const s16x8*)(bsrc + j * bstride + (long)kc(t) * 1024);
        step(t, b0, ws_int<0>{}, std::false_type{}, std::false_type{});
      }
    }
  } else {
    // ================= producer: dw weights LDS-DMA, depthwise on MFMA
    // STAMP: prologue milestones (setup done, weight DMAs issued, prologue barrier, A(0) written),
    // producer-side only and stored by the producers: a value held across the consumers' loop
    // took registers of their in-flight B loads (tools/vmcnt_check.py)
    unsigned long long pst[4] = {0, 0, 0, 0};
    auto pstamp = [&](int i) {
      if constexpr (STAMP) pst[i] = __builtin_amdgcn_s_memtime();
    };
    const int pw = wave - 4;
    const uint8_t* wsrc = (const uint8_t*)a.dwk + lane * 16;
    // every producer wave DMAs the same 1 KiB of depthwise weight entries: letting only wave 0
    // load them (round 6) put a branch into the loop body, and hipcc then stopped hoisting the
    // depthwise MFMAs above the barrier (one basic block each side): +2 us per no-ReLU layer
    auto issue = [&](int t, int slot) { glds16(wsrc + (long)kc(t) * 1024, smem + slot * STAGE + WOFF); };
    // the weight DMAs of the first stages go out BEFORE the tap-offset setup below (its runtime
    // divisions by W and H take ~1,400 cycles): the prologue barrier waits for them. Issued after the
    // setup (until round 6), the prologue ran 8,760 instead of 6,892 cycles (stamped ZF build,
    // mid_sep_nr) and the bench read 0.6 % lower in 3 of 3 pairs (profiles/middle_flow_r6.txt)
#pragma unroll
    for (int p = 0; p < STAGES - 1; ++p)
      if (!TAIL || p < KT) issue(p, p);
    pstamp(1);

    const int g = pw & 1;                        // channel group of all this wave's units
    const int p16 = lane & 15, kb = lane >> 4;
    const int par = kb >> 1, qc = 2 * g + (kb & 1);
    int toff[UPW][5];
#pragma unroll
    for (int i = 0; i < UPW; ++i) {
      const int u = pw + 4 * i;                  // unit -> row fragment u >> 1
      int mg = m0 + (u >> 1) * 16 + p16;
      mg = mg < a.M ? mg : a.M - 1;
      const int R = mg / W, w = mg - R * W, h = R % H;
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int tap = 2 * j + par;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const bool ok = tap < 9 && (unsigned)(h + dy) < (unsigned)H && (unsigned)(w + dx) < (unsigned)W;
        if constexpr (ZF) {
          const int raw = (int)(mg + dy * W + dx - P0);   // its bank: 4 * raw mod 64 (PL is bank-aligned)
          toff[i][j] = ok ? qc * PL + raw * 16 : ZOFF + (raw & 15) * 16;
        } else {
          const int slot = ok ? (int)(mg + dy * W + dx - P0) : ZSLOT;
          toff[i][j] = qc * PL + slot * 16;
        }
      }
    }
    const bool wv = (p16 >> 3) == (kb & 1);
    const int e = p16 & 7;
    uint32_t sel[2][4];
#pragma unroll
    for (int jp = 0; jp < 2; ++jp)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const uint32_t pair = (2u * jp) | ((2u * jp + 1u) << 8);
        const uint32_t val = (e & 1) ? (0x0c0cu | (pair << 16)) : (0x0c0c0000u | pair);
        sel[jp][d] = (wv && (e >> 1) == d) ? val : 0x0c0c0c0cu;
      }
    const int went = WOFF + ((g * 16 + p16) * 2 + par) * 16;
    const int aoffw = (p16 + 16 * (2 * g + (kb >> 1))) * 16 + 8 * (kb & 1);

    // depthwise of stage s in two halves: LDS reads (issued a step ahead, so they are spread
    // over the step instead of piling up behind the barrier with everybody else's) ...
    // (the weight entries are read LAST: read first, hipcc re-used a register of their destination
    // as the next tap's address and waited for the read right there -- one LDS round trip inside
    // every step of the no-ReLU instances, +2 us per layer in the pipelined bench)
    auto dw_load = [&](int s, u32x4 (&xv)[UPW][5], u32x4& we) {
      const uint8_t* sb = smem + (s % STAGES) * STAGE;
      if constexpr (ABL & 2) {                   // ablation: taps from registers
        we = *(const u32x4*)(sb + went);
#pragma unroll
        for (int i = 0; i < UPW; ++i)
#pragma unroll
          for (int j = 0; j < 5; ++j) xv[i][j] = we + (uint32_t)(i * 5 + j);
      } else {
#pragma unroll
        for (int i = 0; i < UPW; ++i)
#pragma unroll
          for (int j = 0; j < 5; ++j) xv[i][j] = *(const u32x4*)(sb + toff[i][j]);
        we = *(const u32x4*)(sb + went);
      }
    };
    // ... and the MFMA part (dacc), written into A buffer abuf by write_a; s >= KT (padding
    // step) writes zeros
    auto dw_compute = [&](const u32x4 (&xv)[UPW][5], const u32x4 we, f32x4 (&dacc)[UPW]) {
      s16x8 wf[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const uint32_t wd = we[j >> 1];
        u32x4 f;
#pragma unroll
        for (int d = 0; d < 4; ++d) f[d] = __builtin_amdgcn_perm(wd, wd, sel[j & 1][d]);
        wf[j] = __builtin_bit_cast(s16x8, f);
      }
#pragma unroll
      for (int i = 0; i < UPW; ++i) dacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 5; ++j)
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
          u32x4 v = xv[i][j];
          if constexpr (RELU) {
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] = relu_bf16x2(v[d]);
          }
          if constexpr (ABL & 4) {               // ablation: no matrix-pipe work
            dacc[i] += __builtin_bit_cast(f32x4, v) + __builtin_bit_cast(f32x4, wf[j]);
          } else {
            dacc[i] = mfma16(wf[j], __builtin_bit_cast(s16x8, v), dacc[i]);
          }
        }
    };
    auto write_a = [&](int s, const f32x4 (&dacc)[UPW], int abuf) {
      const bool live = TAIL || s < KT;
      if constexpr (!(ABL & 8)) {
#pragma unroll
        for (int i = 0; i < UPW; ++i) {
          const u32x2 o = {pack_bf16(dacc[i][0], dacc[i][1]), pack_bf16(dacc[i][2], dacc[i][3])};
          *(u32x2*)(smem + RING + abuf * ABUF + ((pw + 4 * i) >> 1) * 1024 + aoffw) =
              live ? o : (u32x2){0u, 0u};
        }
      } else {                                   // ablation: keep the values live, write nothing
#pragma unroll
        for (int i = 0; i < UPW; ++i)
          asm volatile("" ::"v"(dacc[i][0]), "v"(dacc[i][1]), "v"(dacc[i][2]), "v"(dacc[i][3]));
      }
    };
    auto dw_mfma = [&](int s, const u32x4 (&xv)[UPW][5], const u32x4 we, int abuf) {
      f32x4 dacc[UPW];
      dw_compute(xv, we, dacc);
      write_a(s, dacc, abuf);
    };

    pstamp(0);                                   // setup (tap offsets) done
    if constexpr (ZF) {                          // the stages' zero blocks: 16 x 16 B each
      const int z = pw * 64 + lane;
      if (z < STAGES * 16) *(u32x4*)(smem + (z >> 4) * STAGE + ZOFF + (z & 15) * 16) = (u32x4){0u, 0u, 0u, 0u};
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    u32x4 xv[UPW][5], we;
    // nwait: weight DMAs that may still be in flight at the barrier; mf / ld / is: the step runs
    // dw_mfma(t + 1) / dw_load(t + 2) / issue(t + STAGES - 1) (always, except in TAIL's peeled steps)
    auto pstep = [&](int t, auto nwait, auto mf, auto ld, auto is) {
      ws_wait_barrier<decltype(nwait)::value>();     // stage t+2 landed and published
      stamp(st0, t);
      if constexpr (decltype(mf)::value) dw_mfma(t + 1, xv, we, (t + 1) & 1);   // inputs read during the previous step
      if constexpr (decltype(ld)::value) dw_load(t + 2, xv, we);                // consumed next step
      if constexpr (decltype(is)::value) issue(t + STAGES - 1, (t + STAGES - 1) % STAGES);
      if constexpr (STAMP) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stamp(st1, t);
      }
    };
    const std::true_type yes;
    const int nfull = KT - (STAGES - 1);         // steps whose issue(t + STAGES - 1) is a real stage
    if (!TAIL || nfull >= 0) ws_wait<STAGES - 3>();   // weights of stages 0, 1 (consumers: bands)
    else ws_wait<0>();                           // fewer stages than the prologue issues: all of them
    __builtin_amdgcn_s_barrier();
    pstamp(2);
    dw_load(0, xv, we);
    dw_mfma(0, xv, we, 0);
    if (!TAIL || KT >= 2) dw_load(1, xv, we);
    if constexpr (STAMP) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      pstamp(3);                                 // A(0) written, band(1) read
    }
    if constexpr (!TAIL) {
      for (int t = 0; t < KTE; ++t) pstep(t, ws_int<STAGES - 4>{}, yes, yes, yes);
    } else {
      for (int t = 0; t < nfull; ++t) pstep(t, ws_int<STAGES - 4>{}, yes, yes, yes);
      ws_static_for<0, STAGES - 1>([&](auto ic) {   // the peeled steps r = STAGES - 1 .. 1
        constexpr int r = STAGES - 1 - decltype(ic)::value;
        constexpr int N = r < 3 ? 0 : r - 3;
        if (r <= KT)
          pstep(KT - r, ws_int<N>{}, std::bool_constant<(r >= 2)>{}, std::bool_constant<(r >= 3)>{}, std::false_type{});
      });
    }
    if constexpr (STAMP) {
      if (a.stamps && blockIdx.x < 64 && lane == 0) {
        unsigned long long* o = a.stamps + ((long)blockIdx.x * 8 + wave) * 130;
        for (int i = 0; i < 4; ++i) o[120 + i] = pst[i] ? pst[i] - tstart : 0;
      }
    }
  }
  ws_wait_barrier<0>();
  if constexpr (STAMP) {
    const unsigned long long tend = __builtin_amdgcn_s_memtime();
    if (a.stamps && blockIdx.x < 64) {
      unsigned long long* o = a.stamps + ((long)blockIdx.x * 8 + wave) * 130;
      if (lane < KT && lane < 64) { o[2 + 2 * lane] = st0 - tstart; o[3 + 2 * lane] = st1 - tstart; }
      if (lane == 0) { o[0] = tstart; o[1] = tend - tstart; }
    }
  }

  // ---- epilogue (consumers hold the accumulators; all waves store)
  // residual rows (a block's last sepconv): every thread loads its chunks' residuals BEFORE the C-tile
  // barrier -- producers right away, consumers once their accumulators are in LDS -- instead of one
  // load per store-pass iteration, each waiting behind the previous iterations' stores (in-order vmcnt):
  // +1.3 % img/s in 3 of 3 interleaved pairs (profiles/middle_flow_r6.txt section 7)
  constexpr int CPR = BN / 8;
  constexpr int NIT = (BM * CPR + NT - 1) / NT;
  u32x4 rres[NIT];
  auto load_res = [&]() {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c = tid + it * NT, r = c / CPR, cc = c - r * CPR;
      const int m = min(m0 + r, a.M - 1), n = min(n0 + cc * 8, a.nstore - 8);
      rres[it] = c < BM * CPR ? *(const u32x4*)(a.res + (long)m * a.ldr + n) : (u32x4){0u, 0u, 0u, 0u};
    }
  };
  if (a.res && !consumer) load_res();
  if (consumer) {
    const int quad = lane >> 4, col = lane & 15;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int nl = wave * FN * 16 + j * 16 + 4 * quad;
      const float4 bv = *(const float4*)(a.bias + n0 + nl);
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int mll = i * 16 + col;
        float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y;
        float v2 = acc[i][j][2] + bv.z, v3 = acc[i][j][3] + bv.w;
        if (a.relu_out == 1) {
          v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); v2 = fmaxf(v2, 0.f); v3 = fmaxf(v3, 0.f);
        }
        *(u32x2*)(smem + mll * CS + nl * 2) = (u32x2){pack_bf16(v0, v1), pack_bf16(v2, v3)};
      }
    }
    if (a.res) load_res();
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int c = tid + it * NT, r = c / CPR, cc = c - r * CPR;
    const int m = m0 + r, n = n0 + cc * 8;
    if (c < BM * CPR && m < a.M && n < a.nstore)
      epi_store_r(a, m, n, *(const u32x4*)(smem + r * CS + cc * 16), rres[it]);
  }
}

template <int FM, int FN, int STAGES, int XB, bool STAMP, bool KROT, bool RELU, int ABL = 0, bool ZF = false,
          bool TAIL = false>
__global__ __launch_bounds__(512) void sepconv_ws_kernel(ConvGemmArgs a) {
  __shared__ __attribute__((aligned(256))) uint8_t smem[WsSmem<FM, FN, STAGES, XB, ZF>::BYTES];
  constexpr int BM = 16 * FM, BN = 64 * FN;
  const int nN = (a.NF * 16) / BN;
  const int nM = (a.M + BM - 1) / BM;
  const int wg = xcd_remap(blockIdx.x, nM * nN);
  ws_tile<FM, FN, STAGES, XB, STAMP, KROT, RELU, ABL, ZF, TAIL>(a, wg / nN, wg % nN, smem);
}

// (FM, FN, STAGES, XB = band KiB): tile BM = 16*FM, BN = 64*FN; LDS = STAGES*(XB+1) KiB + 2FM KiB
// (+ the BM x BN bf16 C tile, which reuses it); the band needs BM + 2W + 3 <= 16*XB.
// Retired ids (round 3): 8-14, 18, 19, 27 were timing ablations (no depthwise / pointwise MFMA,
// no loop DMA, wrong band placement, no B reloads). Ablations 2-5 and 12 broke the counted-vmcnt
// contract above (tools/vmcnt_check.py flags exactly those five builds and no other kernel):
// the cause of the round-2 fault. Their slots stay reserved so tuning-table ids keep meaning.
#define KDL_SEPW_CONFIGS(X) \
  X(0, 6, 6, 5, 9)          \
  X(1, 6, 6, 6, 9)          \
  X(2, 6, 6, 5, 11)         \
  X(3, 6, 6, 5, 16)         \
  X(4, 6, 3, 5, 9)          \
  X(5, 4, 6, 5, 8)          \
  X(6, 6, 6, 8, 9)          \
  X(7, 6, 6, 6, 9)          \
  X(15, 12, 3, 5, 15)       \
  X(16, 8, 3, 5, 11)        \
  X(17, 12, 3, 6, 15)       \
  X(20, 4, 3, 5, 8)         \
  X(21, 4, 3, 6, 8)         \
  X(22, 2, 6, 5, 8)         \
  X(23, 6, 6, 5, 9)         \
  X(24, 6, 6, 5, 11)        \
  X(25, 6, 6, 5, 16)        \
  X(26, 4, 6, 5, 8)          \
  X(27, 6, 6, 5, 9)          \
  X(8, 6, 6, 5, 9)           \
  X(9, 6, 6, 5, 9)           \
  X(10, 6, 6, 5, 9)          \
  X(11, 6, 6, 5, 9)          \
  X(12, 6, 6, 5, 9)          \
  X(13, 6, 6, 5, 9)          \
  X(28, 6, 6, 5, 9)          \
  X(29, 6, 6, 5, 11)         \
  X(36, 6, 6, 5, 16)         \
  X(37, 4, 6, 5, 8)          \
  X(38, 6, 6, 5, 9)          \
  X(30, 6, 6, 5, 9)          \
  X(31, 6, 6, 5, 11)         \
  X(32, 6, 6, 5, 16)         \
  X(33, 4, 6, 5, 8)          \
  X(34, 6, 6, 5, 9)          \
  X(35, 4, 6, 5, 8)          \
  X(39, 6, 6, 5, 9)

// id 7: s_memtime stamping variant (tools/stamps.py; never tuned); ids 23-26 = 0, 2, 3, 5
// walking K from a per-M-tile rotated start. Round 6: ids 8-11 = stamped producer ablations
// (ABL 2, 4, 8, 14) of the rotated 96x384 tile, 12 = its stamped ZF build, 13 = it stamped as is;
// ids 28, 29, 36, 37 = 23-26 with ZF; 38 = 0 with ZF. (Round 6 also measured a producer read-ahead
// by three k-steps over a 6-stage ring, ids 30-34: slower isolated and in the pipelined bench,
// hipcc hoisting the next step's MFMAs across the barrier; removed.)
// TAIL (peeled tail: no padding step, no load past the last stage): ids 30-34 = 28, 29, 36, 37, 38
// with it, 35 = 5 with it, 39 = 12 with it (stamped).
constexpr bool sepw_tail(int id) { return (id >= 30 && id <= 35) || id == 39; }
constexpr bool sepw_stamp(int id) { return id == 7 || (id >= 8 && id <= 13) || id == 39; }
constexpr bool sepw_krot(int id) {
  return (id >= 8 && id <= 13) || (id >= 23 && id <= 29) || (id >= 30 && id <= 33) || (id >= 36 && id <= 37) || id == 39;
}
constexpr int sepw_abl(int id) {
  return id == 27 ? 1 : id == 8 ? 2 : id == 9 ? 4 : id == 10 ? 8 : id == 11 ? 14 : 0;
}
constexpr bool sepw_zf(int id) {
  return id == 12 || id == 28 || id == 29 || (id >= 30 && id <= 34) || (id >= 36 && id <= 39);
}

static int sepw_fits_xb(int BM, int W, int xb) { return BM + 2 * W + 3 <= 16 * xb; }

int sepconv_ws_config(int cfg, int* bm, int* bn, int* threads) {
  switch (cfg) {
#define KDL_SWINFO(id, fm, fn, st, xb) \
  case id: *bm = 16 * fm; *bn = 64 * fn; *threads = 512; return 0;
    KDL_SEPW_CONFIGS(KDL_SWINFO)
#undef KDL_SWINFO
    default: return -1;
  }
}

int sepconv_ws_fits(int cfg, int W) {
  switch (cfg) {
#define KDL_SWFIT(id, fm, fn, st, xb) \
  case id: return sepw_fits_xb(16 * fm, W, xb);
    KDL_SEPW_CONFIGS(KDL_SWFIT)
#undef KDL_SWFIT
    default: return 0;
  }
}

hipError_t sepconv_ws(int cfg, const ConvGemmArgs& args, hipStream_t s) {
  const ConvGemmArgs& a = args;
  int bm, bn, th;
  if (sepconv_ws_config(cfg, &bm, &bn, &th) != 0 || !sepconv_ws_fits(cfg, a.W) || a.K % 32 != 0 ||
      a.K < 32 || a.K > 8192 || (a.NF * 16) % bn != 0 || a.OH != a.H || a.OW != a.W || a.M <= 0 || a.dwk == nullptr)
    return hipErrorInvalidValue;
  const int grid = ((a.M + bm - 1) / bm) * ((a.NF * 16) / bn);
  switch (cfg) {
#define KDL_SWCASE(id, fm, fn, st, xb)                                                                \
  case id:                                                                                          \
    if (a.relu_in)                                                                                  \
      hipLaunchKernelGGL((sepconv_ws_kernel<fm, fn, st, xb, sepw_stamp(id), sepw_krot(id), true, sepw_abl(id), \
                                            sepw_zf(id), sepw_tail(id)>), dim3(grid), dim3(th), 0, s, a);           \
    else                                                                                            \
      hipLaunchKernelGGL((sepconv_ws_kernel<fm, fn, st, xb, sepw_stamp(id), sepw_krot(id), false, sepw_abl(id), \
                                            sepw_zf(id), sepw_tail(id)>), dim3(grid), dim3(th), 0, s, a);           \
    break;
    KDL_SEPW_CONFIGS(KDL_SWCASE)
#undef KDL_SWCASE
  }
  return hipGetLastError();
}

}  // namespace kdl
