// Gallery search over an inverted-file index (launch.h GalleryIvfArgs): the stored rows are grouped
// into L lists, each a run of consecutive rows, and a query is scored only against the rows of the
// P lists that its `probe` row names. The dense scan of similar.hip reads every row on every call;
// this one reads the rows of probed lists, once per 32-query pass however many of the pass's
// queries probe them.
//
// The grid is fixed by the index, not by the probes: the host cuts every list into chunks of at
// most kGalleryChunk rows once (the chunk table, C entries {list, first row, row count}) and the
// scan runs one workgroup per entry, blockIdx.y per 32 queries. Which workgroups have work is
// decided on the device, so a captured graph replays with no host step.
//
//   gallery_ivf_split_kernel  the dense split's three bf16 terms per query value, stored per query
//                             ([query][k-step][term][16-byte piece]) instead of per 16-query tile:
//                             a scanning lane's B fragment is whatever query its tile slot got.
//   gallery_ivf_mask_kernel   one lane per (list, pass): the 32-bit set of the pass's queries with
//                             that list among their P probe words. The B * P words of a pass go
//                             through LDS once per workgroup; each lane compares them all and
//                             stores its word whole, so there are no atomics and nothing to reset.
//   gallery_ivf_scan_kernel   reads its table entry and the mask of its list. Empty mask: every
//                             query of the pass gets the head candidate (-inf, no row) and the
//                             workgroup is done, without a gallery byte; the merge looks past a
//                             chunk's head only after the head has won, so the stale entries behind
//                             it are never read. Otherwise the n = popcount(mask) probing queries
//                             are packed into MFMA B-tile slots 0 .. n - 1 (slot s = the query of
//                             the s-th set bit), one 16-query tile when n <= 16, which is the
//                             expected case and half the MFMAs and query bytes of two, and the rows
//                             stream as in gallery_scan_kernel: four waves of 64 rows, A fragments
//                             in 16-byte pieces straight from global memory one k-step ahead, three
//                             terms per query value, smallest first, into one fp32 accumulator, in
//                             the same k order for every row, slot and chunk, so a row's score is
//                             the dense scan's bit for bit. Scores go through LDS to
//                             gallery_pick_rows (similar.h), which writes each probing query's K
//                             best of the chunk; the pass's other queries get the head sentinel.
//   gallery_merge             similar.hip's, over C chunks, writing index -1 where the probed
//                             lists held fewer than K rows (the dense op never has such a place, so
//                             its merge leaves INT_MAX there; the variant is that one select).
//
// Rows at or past a chunk's count, queries outside the mask and columns >= F are never loaded.
// A table entry that does not lie inside [0, N) or names no list is treated as probed by nobody.
#include "similar.h"

namespace kdl {

// work = [split queries, gallery_split_bytes(B)][candidates [B][K][C]][masks [passes][L]]
__host__ __device__ static inline size_t ivf_mask_offset(int B, int K, int C) {
  return gallery_split_bytes(B) + (size_t)B * (size_t)K * (size_t)C * sizeof(GalCand);
}

// grid (k-steps, ceil(B / 16)), one wave: lane l splits q[16 * y + l % 16][32 * step + 8 * (l / 16) + 0..7]
template <bool QV>
__global__ __launch_bounds__(64) void gallery_ivf_split_kernel(GalleryIvfArgs a) {
  const int lane = threadIdx.x, l15 = lane & 15, kg = lane >> 4;
  const int b = blockIdx.y * 16 + l15, k = blockIdx.x * 32 + 8 * kg;
  if (b >= a.B) return;
  u32x4 hi, mid, lo;
  gallery_split_terms<QV>(a, b, k, hi, mid, lo);
  u32x4* w = (u32x4*)a.work + ((long)b * kGalSteps + blockIdx.x) * 3 * 4 + kg;
  w[0] = hi; w[4] = mid; w[8] = lo;
}

// grid (ceil(L / 256), passes)
__global__ __launch_bounds__(256) void gallery_ivf_mask_kernel(GalleryIvfArgs a) {
  __shared__ int32_t ids[32 * kTopkMaxK];
  const int b0 = blockIdx.y * 32, nq = min(32, a.B - b0), words = nq * a.P;
  for (int i = threadIdx.x; i < words; i += 256) ids[i] = a.probe[(long)(b0 + i / a.P) * a.ldp + i % a.P];
  __syncthreads();
  const int list = blockIdx.x * 256 + threadIdx.x;
  if (list >= a.L) return;
  unsigned m = 0;
  for (int j = 0; j < nq; ++j) {
    bool hit = false;
    for (int p = 0; p < a.P; ++p) hit |= ids[j * a.P + p] == list;   // LDS broadcast reads
    m |= (unsigned)hit << j;
  }
  ((unsigned*)((char*)a.work + ivf_mask_offset(a.B, a.K, a.C)))[(long)blockIdx.y * a.L + list] = m;
}

// position of the s-th set bit of m (s < popcount(m))
__device__ __forceinline__ int ivf_nth_bit(unsigned m, int s) {
  for (int j = 0; j < s; ++j) m &= m - 1;
  return __ffs(m) - 1;
}

// QT 16-query tiles of the n probing queries against the rows [first, first + cnt)
template <int QT>
__device__ __forceinline__ void ivf_scan_rows(const GalleryIvfArgs& a, float (*sc)[GAL_LDS], unsigned mask, int n,
                                              int chunk, int first, int cnt, int b0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l15 = lane & 15, kg = lane >> 4;

  const uint16_t* gp[GAL_TILES];
  bool gok[GAL_TILES];
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t) {
    const int r = wave * GAL_WROWS + t * 16 + l15;
    gok[t] = r < cnt;
    gp[t] = a.g + (long)(gok[t] ? first + r : first) * a.ldg + 8 * kg;
  }
  // tile u, slot l15: the split terms of its query, fragment (k-step ks, term p) at qs[u][(ks * 3 + p) * 4]
  const u32x4* qs[QT];
  bool qok[QT];
#pragma unroll
  for (int u = 0; u < QT; ++u) {
    const int slot = u * 16 + l15;
    qok[u] = slot < n;
    const int b = b0 + (qok[u] ? ivf_nth_bit(mask, slot) : 0);
    qs[u] = (const u32x4*)a.work + (long)b * kGalSteps * 3 * 4 + kg;
  }

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
      for (int p = 0; p < 3; ++p) {
        qn[u][p] = (u32x4){0u, 0u, 0u, 0u};
        if (qok[u]) qn[u][p] = qs[u][((k0 >> 5) * 3 + p) * 4];
      }
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
    // smallest term first: gallery_scan_kernel's order, the same for every row
#pragma unroll
    for (int p = 2; p >= 0; --p)
#pragma unroll
      for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
        for (int u = 0; u < QT; ++u) acc[t][u] = mfma16(af[t], bf[u][p], acc[t][u]);
  }

  // accumulator element: slot = lane % 16 of tile u, row = 4 * (lane / 16) + reg of tile t
#pragma unroll
  for (int t = 0; t < GAL_TILES; ++t)
#pragma unroll
    for (int u = 0; u < QT; ++u)
      *(float4*)&sc[u * 16 + l15][wave * GAL_WROWS + t * 16 + 4 * kg] =
          (float4){acc[t][u][0], acc[t][u][1], acc[t][u][2], acc[t][u][3]};
  __syncthreads();

  gallery_pick_rows(sc, a, a.C, chunk, first, first + cnt, n, lane, wave,
                    [b0, mask](int ql) { return b0 + ivf_nth_bit(mask, ql); });
}

// grid (C, passes)
__global__ __launch_bounds__(64 * GAL_WAVES) void gallery_ivf_scan_kernel(GalleryIvfArgs a) {
  __shared__ __attribute__((aligned(16))) float sc[32][GAL_LDS];
  const int chunk = blockIdx.x, b0 = blockIdx.y * 32, nq = min(32, a.B - b0);
  const int32_t* e = a.table + 3 * (long)chunk;
  const int list = e[0], first = e[1], cnt = e[2];
  const bool ok = list >= 0 && list < a.L && first >= 0 && cnt >= 1 && cnt <= kGalleryChunk && first <= a.N - cnt;
  const unsigned* masks = (const unsigned*)((const char*)a.work + ivf_mask_offset(a.B, a.K, a.C));
  const unsigned mask = ok ? masks[(long)blockIdx.y * a.L + list] : 0u;      // bits >= nq are never set

  // queries of the pass that do not probe this list: the head alone says "nothing here"
  if ((int)threadIdx.x < nq && !((mask >> threadIdx.x) & 1u)) {
    GalCand* w = (GalCand*)((char*)a.work + gallery_split_bytes(a.B)) + (long)(b0 + threadIdx.x) * a.K * a.C + chunk;
    *w = GalCand{-INFINITY, INT_MAX};
  }
  if (mask == 0u) return;                             // uniform: before any barrier
  const int n = __popc(mask);
  if (n <= 16) ivf_scan_rows<1>(a, sc, mask, n, chunk, first, cnt, b0);
  else ivf_scan_rows<2>(a, sc, mask, n, chunk, first, cnt, b0);
}

size_t gallery_ivf_workspace(int B, int K, int L, int C) {
  if (B < 1 || K < 1 || L < 1 || C < 1) return 0;
  return ivf_mask_offset(B, K, C) + (size_t)((B + 31) / 32) * (size_t)L * sizeof(unsigned);
}

hipError_t gallery_ivf_topk(const GalleryIvfArgs& a, hipStream_t s) {
  if (a.g8 || a.scale) return hipErrorInvalidValue;
  if (!a.q || ((uintptr_t)a.q & 3) || !a.g || ((uintptr_t)a.g & 15) || !a.out || ((uintptr_t)a.out & 3) ||
      !a.work || ((uintptr_t)a.work & 15) || a.B < 1 || a.B > 1024 || a.N < 1 || a.N > kGalleryMaxN ||
      a.F < 8 || a.F % 8 != 0 || a.F > kEmbedMaxF || a.ldg % 8 != 0 || a.ldg < a.F || a.ldq < a.F ||
      a.K < 1 || a.K > kTopkMaxK || a.K > a.N)
    return hipErrorInvalidValue;
  if (!a.probe || ((uintptr_t)a.probe & 3) || !a.table || ((uintptr_t)a.table & 3) || a.L < 1 || a.L > kGalleryMaxN ||
      a.P < 1 || a.P > kTopkMaxK || a.P > a.L || a.ldp < a.P || a.C < 1 || a.C > kGalleryMaxN / kGalleryChunk + a.L)
    return hipErrorInvalidValue;
  const int passes = (a.B + 31) / 32;
  const dim3 sgrid((a.F + 31) / 32, (a.B + 15) / 16);
  if (!((uintptr_t)a.q & 15) && a.ldq % 4 == 0) hipLaunchKernelGGL(gallery_ivf_split_kernel<true>, sgrid, dim3(64), 0, s, a);
  else hipLaunchKernelGGL(gallery_ivf_split_kernel<false>, sgrid, dim3(64), 0, s, a);
  hipLaunchKernelGGL(gallery_ivf_mask_kernel, dim3((a.L + 255) / 256, passes), dim3(256), 0, s, a);
  hipLaunchKernelGGL(gallery_ivf_scan_kernel, dim3(a.C, passes), dim3(64 * GAL_WAVES), 0, s, a);
  gallery_merge(a, a.C, true, s);
  return hipGetLastError();
}

}  // namespace kdl
