// Gallery search (launch.h GalleryTopkArgs): score[b][j] = sum_i q[b][i] * g[j][i] over a bf16
// gallery of N rows, and per query the K best rows by (score descending, index ascending).
//
// gallery_scan_kernel is a streaming scan on the matrix cores. A workgroup owns GAL_CHUNK = 256
// consecutive gallery rows, each of its four waves 64 of them as four 16-row A tiles that lanes
// load 16 bytes at a time straight from global memory (row lane % 16, columns 8 * (lane / 16)
// of the 32-column k-step), one k-step ahead of the MFMAs that use them. The queries are the B
// operand, 16 per tile and up to two tiles (32 queries) per pass, so the gallery is read once
// for B <= 32; blockIdx.y walks further 32-query groups. A query rounded once to bf16 would be
// 2^-8 off, so every fp32 query value is split into three bf16 terms (hi, the rounded remainder,
// the rounded remainder of that: 24 significant bits, the fp32 value again) and each term is
// one MFMA into the same accumulator. gallery_split_kernel, a small launch in front, does the
// split once and stores the terms in `work` in B-fragment order ([query tile][k-step][term][lane],
// 16 bytes each), so a scanning wave fetches a fragment with one contiguous 1 KB load that stays
// in L2, and the scan has no conversion work. (Splitting the fp32 rows in every scanning wave
// instead took the same time from 100,000 rows on and 20 % longer at 10,000: profiles/similar.txt.)
// Every row's sum runs over the
// k-steps in the same order with the same three terms, whatever its tile, wave or chunk:
// equal rows give bit-equal scores. Rows >= N, queries >= B and columns >= F are never loaded
// (their lanes feed zeros, in the split kernel for the queries), so there are no loads past the
// end and pad columns are never read.
// The 256 x 32 scores then go through LDS, and each wave picks K winners for its queries the way
// softmax_topk does (four scores per lane, a taken mask, a wave-wide arg-max per round) and
// writes them to work[b][k][chunk] as (score, index); missing candidates of a short last
// chunk are (-inf, INT_MAX).
// gallery_merge_kernel, the last launch, is one wave per query. The chunk lists are sorted, so
// a chunk's best remaining candidate is its first entry that ranks strictly after the previous
// winner: no state but the previous winner, and a round reads one entry per chunk (a few more
// for chunks that already won). Separate launches instead of a last-block-done counter, as in
// embed.hip: no state to reset between graph replays. No atomics; two launches are bit-equal.
#include <climits>

#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int GAL_WAVES = 4, GAL_TILES = 4, GAL_WROWS = 16 * GAL_TILES;
constexpr int GAL_LDS = kGalleryChunk + 4;          // fp32 row stride of the score tile
static_assert(GAL_WAVES * GAL_WROWS == kGalleryChunk, "chunk = rows of one workgroup");

struct GalCand { float v; int i; };                 // 8 bytes of work
constexpr int GAL_HEADS = 16;                       // list heads a merging lane loads at once

// work = [split queries: 2 * ceil(B / 32) tiles (whole scan passes; queries >= B are zeros) x
// kGalSteps k-steps x 3 terms x 64 lanes x 16 bytes, sized for kEmbedMaxF because the workspace
// size does not depend on F][candidates]
constexpr int kGalSteps = kEmbedMaxF / 32;
__host__ __device__ static int gallery_tiles(int B) { return 2 * ((B + 31) / 32); }
__host__ __device__ static size_t gallery_split_bytes(int B) {
  return (size_t)gallery_tiles(B) * kGalSteps * 3 * 64 * sizeof(u32x4);
}

// grid (k-steps, query tiles), one wave: lane l splits q[tile * 16 + l % 16][32 * step + 8 * (l / 16) + 0..7]
template <bool QV>
__global__ __launch_bounds__(64) void gallery_split_kernel(GalleryTopkArgs a) {
  const int lane = threadIdx.x, l15 = lane & 15, kg = lane >> 4;
  const int b = blockIdx.y * 16 + l15, k = blockIdx.x * 32 + 8 * kg;
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (b < a.B && k < a.F) {                          // F % 8 == 0: a lane's 8 columns are in or out
    const float* p = a.q + (long)b * a.ldq + k;
    if (QV) {
      const float4 v0 = *(const float4*)p, v1 = *(const float4*)(p + 4);
      x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = p[j];
    }
  }
  u32x4 hi, mid, lo;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const float x0 = x[2 * d], x1 = x[2 * d + 1];
    hi[d] = pack_bf16(x0, x1);
    const float r0 = x0 - bf_lo(hi[d]), r1 = x1 - bf_hi(hi[d]);       // exact
    mid[d] = pack_bf16(r0, r1);
    lo[d] = pack_bf16(r0 - bf_lo(mid[d]), r1 - bf_hi(mid[d]));        // exact, then <= 8 bits left
  }
  u32x4* w = (u32x4*)a.work + ((long)blockIdx.y * kGalSteps + blockIdx.x) * 3 * 64 + lane;
  w[0] = hi; w[64] = mid; w[128] = lo;
}

// QT: 16-query tiles per pass
template <int QT>
__global__ __launch_bounds__(64 * GAL_WAVES) void gallery_scan_kernel(GalleryTopkArgs a, int chunks) {
  __shared__ __attribute__((aligned(16))) float sc[16 * QT][GAL_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;
  const int chunk = blockIdx.x, b0 = blockIdx.y * 32;
  const int row0 = chunk * kGalleryChunk + wave * GAL_WROWS;

  const uint16_t* gp[GAL_TILES];
  bool gok[GAL_TILES];
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t) {
    const int r = row0 + t * 16 + l15;
    gok[t] = r < a.N;
    gp[t] = a.g + (long)(gok[t] ? r : 0) * a.ldg + 8 * kg;
  }
  // this pass's split queries: fragment (tile u, k-step ks, term p) at qs[((u * kGalSteps + ks) * 3 + p) * 64]
  const u32x4* qs = (const u32x4*)a.work + (long)blockIdx.y * 2 * kGalSteps * 3 * 64 + lane;

  f32x4 acc[GAL_TILES][QT];
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
    for (int u = 0; u < QT; ++u) acc[t][u] = (f32x4){0.f, 0.f, 0.f, 0.f};

  u32x4 an[GAL_TILES], qn[QT][3];
  auto load = [&](int k0) {
    const bool kok = k0 + 8 * kg < a.F;              // F % 8 == 0: a lane's 8 columns are in or out
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p) qn[u][p] = qs[((long)(u * kGalSteps + (k0 >> 5)) * 3 + p) * 64];
#pragma unroll
    for (int t = 0; t < GAL_TILES; ++t) {
      an[t] = (u32x4){0u, 0u, 0u, 0u};
      if (kok && gok[t]) an[t] = *(const u32x4*)(gp[t] + k0);
    }
  };

  load(0);
  for (int k0 = 0; k0 < a.F; k0 += 32) {
    s16x8 af[GAL_TILES], bf[QT][3];
#pragma unroll
    for (int t = 0; t < GAL_TILES; ++t) af[t] = __builtin_bit_cast(s16x8, an[t]);
#pragma unroll
    for (int u = 0; u < QT; ++u)
#pragma unroll
      for (int p = 0; p < 3; ++p) bf[u][p] = __builtin_bit_cast(s16x8, qn[u][p]);
    if (k0 + 32 < a.F) load(k0 + 32);
    // smallest term first: the same order for every row
#pragma unroll
    for (int p = 2; p >= 0; --p)
#pragma unroll
      for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
        for (int u = 0; u < QT; ++u) acc[t][u] = mfma16(af[t], bf[u][p], acc[t][u]);
  }

  // accumulator element: query = lane % 16 of tile u, row = 4 * (lane / 16) + reg of tile t
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
    for (int u = 0; u < QT; ++u)
      *(float4*)&sc[u * 16 + l15][wave * GAL_WROWS + t * 16 + 4 * kg] =
          (float4){acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]};
  __syncthreads();

  constexpr int R = kGalleryChunk / 64;
  const int base = chunk * kGalleryChunk;
  for (int ql = wave; ql < 16 * QT && b0 + ql < a.B; ql += GAL_WAVES) {
    float v[R];
    unsigned taken = 0;                       // bit r: row is past N or already picked
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = sc[ql][r * 64 + lane];
      if (base + r * 64 + lane >= a.N) taken |= 1u << r;
    }
    float myv = -INFINITY;
    int myi = INT_MAX;
    for (int k = 0; k < a.K; ++k) {
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int r = 0; r < R; ++r) {            // ascending index: '>' keeps the first of equals
        const bool free_ = !((taken >> r) & 1u);
        if (free_ && (bi == INT_MAX || v[r] > bv)) { bv = v[r]; bi = base + r * 64 + lane; }
      }
      topk_wave_best(bv, bi);                 // every lane now holds the same winner
      if (bi != INT_MAX && ((bi - base) & 63) == lane) taken |= 1u << ((bi - base) >> 6);
      if (lane == k) { myv = bv; myi = bi; }
    }
    if (lane < a.K) {
      GalCand* w = (GalCand*)((char*)a.work + gallery_split_bytes(a.B)) + ((long)(b0 + ql) * a.K + lane) * chunks + chunk;
      *w = GalCand{myv, myi};
    }
  }
}

__global__ __launch_bounds__(64) void gallery_merge_kernel(GalleryTopkArgs a, int chunks) {
  const int lane = threadIdx.x, b = blockIdx.x;
  const GalCand* w = (const GalCand*)((const char*)a.work + gallery_split_bytes(a.B)) + (long)b * a.K * chunks;   // [K][chunks]
  float pv = INFINITY, myv = 0.f;
  int pi = -1, myi = 0;                       // previous winner: everything ranks after (+inf, -1)
  for (int k = 0; k < a.K; ++k) {
    float bv = -INFINITY;
    int bi = INT_MAX;
    for (int c0 = 0; c0 < chunks; c0 += 64 * GAL_HEADS) {
      GalCand e[GAL_HEADS];
#pragma unroll
      for (int j = 0; j < GAL_HEADS; ++j) {    // independent loads of list heads in flight: a round is bound by their latency
        const int c = c0 + j * 64 + lane;
        e[j] = c < chunks ? w[c] : GalCand{-INFINITY, INT_MAX};
      }
#pragma unroll
      for (int j = 0; j < GAL_HEADS; ++j) {
        const int c = c0 + j * 64 + lane;
        if (c >= chunks) continue;
        GalCand h = e[j];
        // sorted list: skip the entries that already won (they do not rank after the last winner)
        for (int p = 1; h.i != INT_MAX && !topk_before(pv, pi, h.v, h.i); ++p)
          h = p < a.K ? w[(long)p * chunks + c] : GalCand{-INFINITY, INT_MAX};
        if (h.i != INT_MAX && topk_before(h.v, h.i, bv, bi)) { bv = h.v; bi = h.i; }
      }
    }
    topk_wave_best(bv, bi);
    pv = bv; pi = bi;
    if (lane == k) { myv = bv; myi = bi; }
  }
  if (lane < a.K) {
    int32_t* o = a.out + (long)b * 2 * a.K;
    o[lane] = myi;
    reinterpret_cast<float*>(o)[a.K + lane] = myv;
  }
}

static int gallery_chunks(int N) { return (N + kGalleryChunk - 1) / kGalleryChunk; }

size_t gallery_topk_workspace(int B, int N, int K) {
  if (B < 1 || N < 1 || K < 1) return 0;
  return gallery_split_bytes(B) + (size_t)B * (size_t)K * (size_t)gallery_chunks(N) * sizeof(GalCand);
}

hipError_t gallery_topk(const GalleryTopkArgs& a, hipStream_t s) {
  if (!a.q || ((uintptr_t)a.q & 3) || !a.g || ((uintptr_t)a.g & 15) || !a.out || ((uintptr_t)a.out & 3) ||
      !a.work || ((uintptr_t)a.work & 15) || a.B < 1 || a.B > 1024 || a.N < 1 || a.N > kGalleryMaxN ||
      a.F < 8 || a.F % 8 != 0 || a.F > kEmbedMaxF || a.ldg % 8 != 0 || a.ldg < a.F || a.ldq < a.F ||
      a.K < 1 || a.K > kTopkMaxK || a.K > a.N)
    return hipErrorInvalidValue;
  const int chunks = gallery_chunks(a.N);
  const dim3 grid(chunks, (a.B + 31) / 32);
  const dim3 sgrid((a.F + 31) / 32, gallery_tiles(a.B));
  if (!((uintptr_t)a.q & 15) && a.ldq % 4 == 0) hipLaunchKernelGGL(gallery_split_kernel<true>, sgrid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(gallery_split_kernel<false>, sgrid, dim3(64), 0, s, a);
  if (a.B <= 16) hipLaunchKernelGGL(gallery_scan_kernel<1>, grid, dim3(64 * GAL_WAVES), 0, s, a, chunks);
  else hipLaunchKernelGGL(gallery_scan_kernel<2>, grid, dim3(64 * GAL_WAVES), 0, s, a, chunks);
  hipLaunchKernelGGL(gallery_merge_kernel, dim3(a.B), dim3(64), 0, s, a, chunks);
  return hipGetLastError();
}

}  // namespace kdl
