// Garment boxes: the K largest 8-connected regions of the h x w map of an explain / rollout row,
// upsampled onto S x S and cut at a threshold (launch.h LocateArgs; kdl/serving/locate.py is the
// definition). Integers throughout, and every value that more than one thread writes is written by an
// integer atomic whose result does not depend on the order. The picture is never read. Two launches:
//
// locate_mask over (band of kLocateBand rows, image). A workgroup walks its band kOverlayBand rows at
// a time through the two resample passes of heat_upsample.h (the code heat_overlay and palette_hist
// run). A wave takes one (row, 64 columns) item at a time, compares with the threshold and lane 0
// stores the wave's ballot as one 64-bit word of the image's bitmask: S rows of ceil(S / 64) words,
// so a word never straddles rows and the bits at and behind column S are 0. Every word is written by
// every launch.
//
// locate_boxes, one workgroup of 1024 threads per image, labels RUNS, not pixels; the bitmask crossed
// a launch boundary, the labelling never leaves the workgroup.
//   count    thread y counts the runs of row y (bit operations on its words); a workgroup scan
//            gives row_off[y], the index of the row's first run, and R, the image's run count. Run
//            indices are in raster order, so the smallest index of a component is the run that
//            starts at its first pixel.
//   tables   desc (x0 | x1 << 10 | y << 21), parent and area, one uint32 each per run: in LDS for
//            R <= kLocateLdsRuns, else in the workspace. R is the same in every thread, so the switch
//            is uniform. Thread y writes the entries of row y: parent = the run itself, area = 0.
//   union    a thread per run: a binary search finds the first run of row y - 1 that ends at or behind
//            x0 - 1, and the run joins every one from there that starts at or before x1 (8-connectivity).
//            unite() follows parents to two roots and atomicMin's the smaller into the larger's parent;
//            where another thread was faster it goes on with what it displaced. parent[i] <= i always
//            and only atomicMin writes it, so every find follows strictly decreasing indices and the
//            larger index of the pair unite() holds falls with every trip: no loop waits for
//            another wave.
//   flatten  parent = root for every run, area[root] += the run's length.
//   select   count = the runs that are their own parent; K rounds of a workgroup argmax over the key
//            area << 20 | (2^20 - 1 - root), each below the last one's, so equal areas go to the
//            earlier first pixel (R <= 2^19).
//   boxes    of the K winners only: each thread reduces its runs in registers, then LDS atomics.
// Threads 0..K-1 write the words. Nothing is left behind that the next launch reads before writing it.
#include "common.h"
#include "heat_upsample.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kLocateBand = 32;                                  // output rows per workgroup of locate_mask
constexpr int kBoxThreads = 1024;
constexpr uint32_t kRootBits = 20;
constexpr uint32_t kRootMask = (1u << kRootBits) - 1;
static_assert(kLocateBand % kOverlayBand == 0, "a band is walked in whole overlay bands");
static_assert(kOverlayBand * kOverlayMaxTaps <= 256, "one thread per (row, tap) of a staged band");
static_assert(kOverlayMaxS <= kBoxThreads, "a thread per row");
static_assert(kOverlayMaxS <= 1024, "x0 in 10 bits, x1 in 11, y in 10");
static_assert((kOverlayMaxS / 2) * kOverlayMaxS <= (1 << (kRootBits - 1)), "a run index in the key's low bits");

// one image's part of the workspace: the bitmask, then (where an image can have more runs than LDS
// holds) the three run tables
struct Layout {
  int wpr;                // 64-bit words per bitmask row
  uint32_t cap;           // the most runs an S x S mask can have
  size_t mask, table, image;   // bytes: the bitmask, one table, all of the image
};
__host__ __device__ inline Layout layout(int S) {
  Layout l;
  l.wpr = (S + 63) / 64;
  l.cap = (uint32_t)S * (uint32_t)((S + 1) / 2);
  l.mask = ((size_t)S * l.wpr * 8 + 15) / 16 * 16;
  l.table = l.cap > (uint32_t)kLocateLdsRuns ? ((size_t)l.cap * 4 + 15) / 16 * 16 : 0;
  l.image = l.mask + 3 * l.table;
  return l;
}

__global__ __launch_bounds__(256) void locate_mask_kernel(LocateArgs a) {
  __shared__ uint8_t q[kClassMapMaxHW];
  __shared__ uint8_t tmp[(kOverlayMaxRows + kOverlayMaxTaps) * kOverlayMaxS];
  __shared__ int32_t ykk[kOverlayBand * kOverlayMaxTaps];
  __shared__ int32_t ymn[kOverlayBand];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int S = a.S;
  const uint32_t thr = (uint32_t)a.threshold;
  const Layout L = layout(S);
  const int band0 = blockIdx.x * kLocateBand;                    // < S by the grid
  const int band1 = band0 + kLocateBand < S ? band0 + kLocateBand : S;
  const float* heat = a.out + (size_t)b * a.ldo + 2;
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(a.work + (size_t)b * L.image);

  for (int r0 = band0; r0 < band1; r0 += kOverlayBand) {
    const int r1 = r0 + kOverlayBand < band1 ? r0 + kOverlayBand : band1;
    __syncthreads();                                             // the last band's readers of tmp
    int row0, nrow;
    upsample_stage(heat, a.yb, a.yk, a.yks, a.h, a.w, r0, r1, tid, q, ykk, ymn, row0, nrow);
    __syncthreads();
    upsample_hpass(a.xb, a.xk, a.xks, S, a.w, row0, nrow, tid, q, tmp);
    __syncthreads();
    const int items = (r1 - r0) * L.wpr;                         // (row of the band, word of the row)
    for (int it = wave; it < items; it += 4) {                   // uniform per wave
      const int yi = it / L.wpr, wd = it - yi * L.wpr, x = wd * 64 + lane;
      const bool on = x < S && upsample_pixel(tmp, ykk, ymn, yi, x, S, a.yks) >= thr;
      const unsigned long long m = __ballot(on);
      if (lane == 0) mask[(size_t)(r0 + yi) * L.wpr + wd] = m;   // row r0 + yi < S, word wd < wpr: inside the bitmask
    }
  }
}

// parent and area are written by atomics of other waves while they are read
__device__ __forceinline__ uint32_t ldw(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[x] <= x: the indices fall until a run that is its own parent
__device__ __forceinline__ uint32_t find_root(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ldw(parent + x);
    if (p >= x) return x;
    x = p;
  }
}

__device__ __forceinline__ void unite(uint32_t* parent, uint32_t x, uint32_t y) {
  for (;;) {
    x = find_root(parent, x);
    y = find_root(parent, y);
    if (x == y) return;
    if (x < y) {
      const uint32_t t = x;
      x = y;
      y = t;
    }
    const uint32_t old = atomicMin(parent + x, y);               // x > y
    if (old == x) return;                                        // x was a root and now hangs under y
    x = old;                                                     // old < x: someone hung x under old first; old and y remain to be joined
  }
}

// the largest key of the workgroup, in every thread (sh: one word per wave)
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  __syncthreads();                                               // the last call's readers of sh
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long m = 0;
#pragma unroll
  for (int i = 0; i < kBoxThreads / 64; ++i) m = sh[i] > m ? sh[i] : m;
  return m;
}

struct BoxShared {
  uint32_t row_off[kOverlayMaxS + 1];
  unsigned long long red[kBoxThreads / 64];
  uint32_t wsum[kBoxThreads / 64];
  uint32_t win_root[kLocateMaxK], win_area[kLocateMaxK], bx0[kLocateMaxK], bx1[kLocateMaxK], by1[kLocateMaxK];
  uint32_t roots;
};

// everything behind the run count, on tables of at least R entries each
__device__ __forceinline__ void label_and_select(const LocateArgs& a, const unsigned long long* mask, int wpr,
                                                 uint32_t R, uint32_t* desc, uint32_t* parent, uint32_t* area,
                                                 BoxShared& sh, uint32_t* res) {
  const int tid = threadIdx.x, lane = tid & 63, S = a.S, K = a.K;

  // tables: thread y writes the runs of row y
  if (tid < S) {
    uint32_t cur = sh.row_off[tid];
    const uint32_t end = sh.row_off[tid + 1];                    // <= R
    const unsigned long long* row = mask + (size_t)tid * wpr;
    bool open = false;
    uint32_t xs = 0;
    for (int wd = 0; wd <= wpr; ++wd) {
      unsigned long long m = wd < wpr ? row[wd] : 0ull;          // one empty word behind the row closes a run that reaches S
      const uint32_t base = (uint32_t)wd * 64u;
      for (;;) {
        if (!open) {
          if (!m) break;
          const int s = __ffsll((long long)m) - 1;
          xs = base + (uint32_t)s;
          open = true;
          m |= (1ull << s) - 1ull;                               // ones below the run's start: the next zero is its end
        }
        const unsigned long long z = ~m;
        if (!z) break;                                           // the run goes on in the next word
        const int e = __ffsll((long long)z) - 1;
        if (cur < end) {
          desc[cur] = xs | ((base + (uint32_t)e) << 10) | ((uint32_t)tid << 21);
          parent[cur] = cur;
          area[cur] = 0u;
          ++cur;
        }
        open = false;
        m &= ~((1ull << e) - 1ull);
      }
    }
  }
  if (tid == 0) sh.roots = 0u;
  if (tid < kLocateMaxK) {
    sh.bx0[tid] = 0xffffffffu;
    sh.bx1[tid] = 0u;
    sh.by1[tid] = 0u;
  }
  __syncthreads();

  // union: run r with the runs of the row above that touch it, corners included
  for (uint32_t r = tid; r < R; r += kBoxThreads) {
    const uint32_t d = desc[r], y = d >> 21;
    if (!y) continue;
    const uint32_t x0 = d & 1023u, x1 = (d >> 10) & 2047u;
    uint32_t lo = sh.row_off[y - 1];
    const uint32_t hi = sh.row_off[y];
    uint32_t h = hi;
    while (lo < h) {                                             // the first run above with x1' >= x0
      const uint32_t mid = (lo + h) >> 1;
      if (((desc[mid] >> 10) & 2047u) < x0) lo = mid + 1;
      else h = mid;
    }
    for (uint32_t p = lo; p < hi && (desc[p] & 1023u) <= x1; ++p) unite(parent, r, p);
  }
  __syncthreads();

  // flatten, areas, the number of components
  uint32_t mine = 0;
  for (uint32_t r = tid; r < R; r += kBoxThreads) {
    const uint32_t root = find_root(parent, r);
    if (root != r) __hip_atomic_store(parent + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else ++mine;
    const uint32_t d = desc[r];
    atomicAdd(area + root, ((d >> 10) & 2047u) - (d & 1023u));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0 && mine) atomicAdd(&sh.roots, mine);
  __syncthreads();

  // the K largest, each round's key below the last round's
  unsigned long long last = ~0ull;
  int nw = 0;
  for (int j = 0; j < K; ++j) {
    unsigned long long key = 0;
    for (uint32_t r = tid; r < R; r += kBoxThreads) {
      if (ldw(parent + r) != r) continue;
      const unsigned long long ky = ((unsigned long long)ldw(area + r) << kRootBits) | (kRootMask - r);
      key = ky < last && ky > key ? ky : key;
    }
    const unsigned long long best = block_max(key, sh.red);
    if (!best) break;                                            // fewer components than K
    if (tid == 0) {
      sh.win_root[j] = kRootMask - (uint32_t)(best & kRootMask);
      sh.win_area[j] = (uint32_t)(best >> kRootBits);
    }
    last = best;
    nw = j + 1;
  }
  __syncthreads();

  // their boxes: y0 is the root's row (the first pixel in raster order is in the top row)
  uint32_t wr[kLocateMaxK], mn[kLocateMaxK], mx[kLocateMaxK], my[kLocateMaxK];
#pragma unroll
  for (int j = 0; j < kLocateMaxK; ++j) {
    wr[j] = j < nw ? sh.win_root[j] : 0xffffffffu;
    mn[j] = 0xffffffffu;
    mx[j] = 0u;
    my[j] = 0u;
  }
  for (uint32_t r = tid; r < R; r += kBoxThreads) {
    const uint32_t root = ldw(parent + r), d = desc[r];
    const uint32_t x0 = d & 1023u, x1 = (d >> 10) & 2047u, y1 = (d >> 21) + 1u;
#pragma unroll
    for (int j = 0; j < kLocateMaxK; ++j)
      if (root == wr[j]) {
        mn[j] = x0 < mn[j] ? x0 : mn[j];
        mx[j] = x1 > mx[j] ? x1 : mx[j];
        my[j] = y1 > my[j] ? y1 : my[j];
      }
  }
#pragma unroll
  for (int j = 0; j < kLocateMaxK; ++j)
    if (mx[j]) {                                                 // a run of winner j: x1 >= 1
      atomicMin(&sh.bx0[j], mn[j]);
      atomicMax(&sh.bx1[j], mx[j]);
      atomicMax(&sh.by1[j], my[j]);
    }
  __syncthreads();

  if (tid == 0) res[0] = sh.roots;
  if (tid < K) {
    uint32_t c0 = 0, c1 = 0, ar = 0;
    if (tid < nw) {
      c0 = (desc[sh.win_root[tid]] >> 21) | (sh.bx0[tid] << 16);
      c1 = sh.by1[tid] | (sh.bx1[tid] << 16);
      ar = sh.win_area[tid];
    }
    res[1 + 3 * tid] = c0;
    res[2 + 3 * tid] = c1;
    res[3 + 3 * tid] = ar;
  }
}

__global__ __launch_bounds__(kBoxThreads) void locate_boxes_kernel(LocateArgs a) {
  __shared__ BoxShared sh;
  __shared__ uint32_t tab[3 * kLocateLdsRuns];
  const int tid = threadIdx.x, b = blockIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S;
  const Layout L = layout(S);
  uint8_t* base = a.work + (size_t)b * L.image;
  const unsigned long long* mask = reinterpret_cast<const unsigned long long*>(base);
  uint32_t* res = reinterpret_cast<uint32_t*>(a.out + (size_t)b * a.ldo + 2 + a.h * a.w);   // count, K x (corner, corner, area)

  // the runs of row tid: the set bits whose left neighbour is clear
  uint32_t cnt = 0;
  if (tid < S) {
    const unsigned long long* row = mask + (size_t)tid * L.wpr;
    unsigned long long carry = 0;
    for (int wd = 0; wd < L.wpr; ++wd) {
      const unsigned long long m = row[wd];
      cnt += (uint32_t)__popcll(m & ~((m << 1) | carry));
      carry = m >> 63;
    }
  }
  uint32_t inc = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh.wsum[wave] = inc;
  __syncthreads();
  uint32_t pre = 0, R = 0;
#pragma unroll
  for (int i = 0; i < kBoxThreads / 64; ++i) {
    pre += i < wave ? sh.wsum[i] : 0u;
    R += sh.wsum[i];
  }
  if (tid < S) sh.row_off[tid] = pre + inc - cnt;
  if (tid == 0) sh.row_off[S] = R;
  __syncthreads();

  // R is the same in every thread: the branches below are uniform across the workgroup
  if (R == 0 || R > L.cap) {                                     // an empty mask (no S x S mask has more than cap runs)
    if (tid < 1 + 3 * a.K) res[tid] = 0u;
    return;
  }
  if (R <= (uint32_t)kLocateLdsRuns) {
    label_and_select(a, mask, L.wpr, R, tab, tab + kLocateLdsRuns, tab + 2 * kLocateLdsRuns, sh, res);
  } else {                                                       // cap >= R > kLocateLdsRuns: the layout has the tables
    uint32_t* g = reinterpret_cast<uint32_t*>(base + L.mask);
    const size_t n = L.table / 4;
    label_and_select(a, mask, L.wpr, R, g, g + n, g + 2 * n, sh, res);
  }
}

bool valid(const LocateArgs& a) {
  if (!a.out || !a.work || !a.xb || !a.xk || !a.yb || !a.yk || !a.h_xb || !a.h_yb) return false;
  if (!aligned16(a.out) || !aligned16(a.work) || !aligned16(a.xb) || !aligned16(a.xk) || !aligned16(a.yb) ||
      !aligned16(a.yk))
    return false;
  if (a.B < 1 || a.B > 65535 || a.h < 1 || a.w < 1 || (int64_t)a.h * a.w > kClassMapMaxHW) return false;
  if (a.S < a.h || a.S < a.w || a.S > kOverlayMaxS) return false;
  if (a.K < 1 || a.K > kLocateMaxK || a.threshold < 1 || a.threshold > 255) return false;
  if ((int64_t)a.ldo < 2 + (int64_t)a.h * a.w + 1 + 3 * a.K) return false;
  if (a.xks < 1 || a.xks > kOverlayMaxTaps || a.yks < 1 || a.yks > kOverlayMaxTaps) return false;
  if (!valid_bounds(a.h_xb, a.S, a.w, a.xks) || !valid_bounds(a.h_yb, a.S, a.h, a.yks)) return false;
  return valid_band_rows(a.h_yb, a.S, kOverlayBand, 0);          // the map rows one staged band needs
}

}  // namespace

size_t locate_workspace(int B, int S) {
  return B > 0 && S > 0 && S <= kOverlayMaxS ? (size_t)B * layout(S).image : 0;
}

hipError_t locate(const LocateArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((a.S + kLocateBand - 1) / kLocateBand), (unsigned)a.B);
  hipLaunchKernelGGL(locate_mask_kernel, grid, dim3(256), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(locate_boxes_kernel, dim3((unsigned)a.B), dim3(kBoxThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
