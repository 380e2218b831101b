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

// The K best of the chunk's rows for each of the pass's queries, from its score tile sc[query][row]
// in LDS (complete: the caller has passed a barrier): wave w takes the queries w, w + 4, ...
template <int QT>
__device__ __forceinline__ void gallery_pick(const float (*sc)[GAL_LDS], const GalleryTopkArgs& a, int chunks,
                                             int chunk, int b0, int lane, int wave) {
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

// the scan of an fp8 gallery (similar_f8.hip), between gallery_topk's split and merge launches
void gallery_scan_f8(const GalleryTopkArgs& a, int chunks, hipStream_t s);

}  // namespace kdl
