// What the gallery scans of similar.hip (bf16 rows) and similar_f8.hip (e4m3 rows) share: the
// shape of a scanning workgroup, the layout of `work`, and the pick of a chunk's K best rows.
#pragma once
#include <climits>

#include "common.h"
#include "launch.h"

namespace kdl {

constexpr int GAL_WAVES = 4, GAL_TILES = 4, GAL_WROWS = 16 * GAL_TILES;
constexpr int GAL_LDS = kGalleryChunk + 4;          // fp32 row stride of the score tile
static_assert(GAL_WAVES * GAL_WROWS == kGalleryChunk, "chunk = rows of one workgroup");

struct GalCand { float v; int i; };                 // 8 bytes of work

// work = [split queries: 2 * ceil(B / 32) tiles (whole scan passes; queries >= B are zeros) x
// kGalSteps k-steps x 3 terms x 64 lanes x 16 bytes, sized for kEmbedMaxF because the workspace
// size does not depend on F][candidates]
constexpr int kGalSteps = kEmbedMaxF / 32;
__host__ __device__ static inline int gallery_tiles(int B) { return 2 * ((B + 31) / 32); }
__host__ __device__ static inline size_t gallery_split_bytes(int B) {
  return (size_t)gallery_tiles(B) * kGalSteps * 3 * 64 * sizeof(u32x4);
}

// The three bf16 terms (hi, the rounded remainder, the rounded remainder of that) of the 8 query
// values q[b][k .. k + 7], zeros for a query >= B or a column >= F (F % 8 == 0: the 8 are in or out)
template <bool QV>
__device__ __forceinline__ void gallery_split_terms(const GalleryTopkArgs& a, int b, int k, u32x4& hi, u32x4& mid,
                                                    u32x4& lo) {
  float x[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (b < a.B && k < a.F) {
    const float* p = a.q + (long)b * a.ldq + k;
    if (QV) {
      const float4 v0 = *(const float4*)p, v1 = *(const float4*)(p + 4);
      x[0] = v0.x; x[1] = v0.y; x[2] = v0.z; x[3] = v0.w; x[4] = v1.x; x[5] = v1.y; x[6] = v1.z; x[7] = v1.w;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = p[j];
    }
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const float x0 = x[2 * d], x1 = x[2 * d + 1];
    hi[d] = pack_bf16(x0, x1);
    const float r0 = x0 - bf_lo(hi[d]), r1 = x1 - bf_hi(hi[d]);       // exact
    mid[d] = pack_bf16(r0, r1);
    lo[d] = pack_bf16(r0 - bf_lo(mid[d]), r1 - bf_hi(mid[d]));        // exact, then <= 8 bits left
  }
}

// The K best of the rows [base, end) of a chunk (at most kGalleryChunk of them) for each of `slots`
// score rows of its tile sc[slot][row - base] in LDS (complete: the caller has passed a barrier);
// slot ql belongs to query query_of(ql). Wave w takes the slots w, w + 4, ...
template <class Q>
__device__ __forceinline__ void gallery_pick_rows(const float (*sc)[GAL_LDS], const GalleryTopkArgs& a, int chunks,
                                                  int chunk, int base, int end, int slots, int lane, int wave,
                                                  Q query_of) {
  constexpr int R = kGalleryChunk / 64;
  for (int ql = wave; ql < slots; ql += GAL_WAVES) {
    float v[R];
    unsigned taken = 0;                       // bit r: row is past the end or already picked
#pragma unroll
    for (int r = 0; r < R; ++r) {
      v[r] = sc[ql][r * 64 + lane];
      if (base + r * 64 + lane >= end) taken |= 1u << r;
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
      GalCand* w = (GalCand*)((char*)a.work + gallery_split_bytes(a.B)) + ((long)query_of(ql) * a.K + lane) * chunks + chunk;
      *w = GalCand{myv, myi};
    }
  }
}

// The dense scans' pick: chunk c holds the rows from c * kGalleryChunk on, slot ql is query b0 + ql
template <int QT>
__device__ __forceinline__ void gallery_pick(const float (*sc)[GAL_LDS], const GalleryTopkArgs& a, int chunks,
                                             int chunk, int b0, int lane, int wave) {
  gallery_pick_rows(sc, a, chunks, chunk, chunk * kGalleryChunk, a.N, min(16 * QT, a.B - b0), lane, wave,
                    [b0](int ql) { return b0 + ql; });
}

// the scan of an fp8 gallery (similar_f8.hip), between gallery_topk's split and merge launches
void gallery_scan_f8(const GalleryTopkArgs& a, int chunks, hipStream_t s);
// gallery_topk's last launch (similar.hip), one wave per query over `chunks` candidate lists;
// `missing`: a place that no candidate fills is written as index -1 (the dense op always has K)
void gallery_merge(const GalleryTopkArgs& a, int chunks, bool missing, hipStream_t s);

}  // namespace kdl
