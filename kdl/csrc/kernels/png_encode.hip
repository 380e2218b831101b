// PNG encode of uint8 RGB / RGBA pictures, byte for byte the file of kdl/serving/png_encode.py png_rule
// (launch.h PngEncodeArgs). Integer only, wave size 64, five launches:
//   1. filter  one workgroup per (band of kPngBand rows, picture). The row and the row above it sit in LDS;
//              five residual sums by wave reduction pick the filter; the filtered row stays in LDS. Per
//              candidate distance a thread finds the first mismatch of its chunk, a suffix-min scan over
//              the 256 chunks turns that into match lengths. The greedy parse is next(j) = j + (match ?
//              length : 1); the positions reachable from 0 are found by pointer doubling in LDS
//              (ceil(log2(L + 1)) rounds, one barrier each). Every position gets a 16-bit token (0xFFFF:
//              not reached), the reached ones count into an LDS histogram that is added to the picture's
//              with integer atomics, and the row's Adler sums are stored.
//   2. code    one workgroup per picture: rank-sorts the used symbols, then one thread runs the rule's
//              length-limited code, the canonical codes (bit-reversed), the run-coded header and the
//              fixed / dynamic choice in LDS (build_code, also compiled for the host). The table goes to
//              the workspace and the histogram is left zero for the next launch.
//   3. rowbits a wave per row: the row's bit length under the table. The workgroups of a picture also clear
//              its stream words, a slice each.
//   4. bits    a wave per row: the row's first bit is the header's bits plus the rows in front; a lane takes
//              a run of consecutive positions, a wave scan gives its bit offset, and it ORs whole words
//              into the stream (atomicOr: lanes share a word only at their ends; OR commutes, so every
//              launch gives the same words). Row 0 also ORs the header in, the last row the end-of-block.
//   5. file    one workgroup per picture: the Adler-32 from the rows' sums by a prefix sum modulo 65521, the
//              CRC-32 of the IDAT chunk from per-thread CRCs of equal pieces, each multiplied by
//              x^(8 * bytes behind it) modulo the CRC polynomial, then the row: front words, length, file,
//              zeros up to the cap.
// The workspace must be zero when first used; every launch clears what the next one adds into (the
// histogram) and writes everything else before it reads it.
// Bounds: the picture is read below row_stride * H of each picture; LDS rows are indexed below L = 1 + W*C
// <= kMaxL; tokens below H * lp per picture; the stream below the sw words a picture owns (BitWriter checks
// every word); the row below nfront + 1 + ceil(cap / 4). Every loop is bounded by H, L, cap or a constant.
#include <cstring>

#include "common.h"
#include "launch.h"

namespace kdl {

namespace {

constexpr int kBand = kPngBand;
constexpr int kMaxRow = kPngEncMaxSide * 4;     // picture bytes of a row
constexpr int kMaxL = kMaxRow + 1;              // filtered bytes of a row
constexpr int kMinMatch = 4, kMaxMatch = 258;
constexpr int kLit = 288;                       // literal/length symbols with a fixed code
constexpr int kHist = 320;                      // [0, 288) literal/length, 288 + i: distance index i
constexpr int kHdrWords = 160;                  // 17 + 19 * 3 + 316 * 14 = 4498 bits at most
constexpr int kTabDist = kLit, kTabHdrBits = kLit + 2, kTabMode = kLit + 3, kTabHdr = kLit + 4;
constexpr int kTabWords = kTabHdr + kHdrWords;  // 452
constexpr uint32_t kSkip = 0xFFFFu;             // the token of a position the parse does not reach
constexpr int kFileOverhead = 63;
constexpr int kFileThreads = 1024;

constexpr uint16_t kLenBase[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                   31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
constexpr uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
constexpr uint8_t kClenOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// match length - 3 -> length symbol - 257 | extra bit count << 8 | extra value << 16
struct LenTab {
  uint32_t e[256];
};
constexpr LenTab make_lentab() {
  LenTab t{};
  for (int l = 3; l <= 258; ++l) {
    int s = 0;
    while (s + 1 < 29 && kLenBase[s + 1] <= l) ++s;
    t.e[l - 3] = (uint32_t)s | (uint32_t)kLenExtra[s] << 8 | (uint32_t)(l - kLenBase[s]) << 16;
  }
  return t;
}
__constant__ LenTab c_len = make_lentab();

// the workspace of a call: [tok uint16 B x H x lp][rowinfo uint32 B x H x 4: Adler a, Adler b, bits, -]
// [hist uint32 B x kHist][tab uint32 B x kTabWords][stream uint32 B x sw]
struct Work {
  size_t info, hist, tab, stream, bytes;
  int lp;          // tokens a row owns
  int sw;          // stream words a picture owns
};
__host__ __device__ inline Work work_of(int B, int H, int W, int C, int cap) {
  Work w;
  w.lp = (W * C + 1 + 7) & ~7;
  w.sw = (((cap + 3) / 4 + 2) + 3) & ~3;
  w.info = (size_t)B * H * w.lp * 2;
  w.hist = w.info + (size_t)B * H * 16;
  w.tab = w.hist + (size_t)B * kHist * 4;
  w.stream = w.tab + (((size_t)B * kTabWords * 4 + 15) & ~(size_t)15);
  w.bytes = w.stream + (size_t)B * w.sw * 4;
  return w;
}

__device__ __forceinline__ int mini(int a, int b) { return a < b ? a : b; }

// the sum of v over the 256 threads of the workgroup, in every thread; red: 4 words of LDS
__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------------ 1. filter
__device__ __forceinline__ uint32_t cost_of(int r) {
  const uint32_t v = (uint32_t)r & 255u;
  return v < 128u ? v : 256u - v;
}

// the residual of filter `k` at a byte with neighbours a (left), b (above), c (above left)
__device__ __forceinline__ int residual(int k, int x, int a, int b, int c) {
  if (k == 0) return x;
  if (k == 1) return x - a;
  if (k == 2) return x - b;
  if (k == 3) return x - ((a + b) >> 1);
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  return x - ((pa <= pb && pa <= pc) ? a : pb <= pc ? b : c);
}

__global__ __launch_bounds__(256) void png_filter_kernel(PngEncodeArgs a) {
  __shared__ __align__(16) uint8_t raw[2][kMaxRow];
  __shared__ __align__(16) uint8_t f[kMaxL + 3];
  __shared__ uint16_t mlen[2][kMaxL + 1];
  __shared__ uint16_t jmp[2][kMaxL + 1];
  __shared__ uint8_t reach[kMaxL + 1];
  __shared__ uint32_t hist[kHist];
  __shared__ uint32_t scan[256];
  __shared__ uint32_t red[4];
  const int tid = threadIdx.x, b = blockIdx.y, C = a.C, H = a.H;
  const int n = a.W * C, L = n + 1;
  const int y0 = blockIdx.x * kBand, y1 = mini(y0 + kBand, H);
  const Work wk = work_of(a.B, H, a.W, C, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  uint16_t* tok = reinterpret_cast<uint16_t*>(base) + (size_t)b * H * wk.lp;
  uint32_t* info = reinterpret_cast<uint32_t*>(base + wk.info) + (size_t)b * H * 4;
  uint32_t* ghist = reinterpret_cast<uint32_t*>(base + wk.hist) + (size_t)b * kHist;
  const uint8_t* pic = a.inp + (size_t)b * a.ldi;
  int rounds = 0;
  while ((1 << rounds) < L + 1) ++rounds;                        // <= 13
  const int ch = (L + 255) / 256;                                // consecutive positions a thread scans
  const int s0 = mini(tid * ch, L), s1 = mini(s0 + ch, L);

  for (int i = tid; i < kHist; i += 256) hist[i] = 0u;
  {
    uint8_t* p = raw[(y0 + 1) & 1];                              // the row above the band; zeros above the picture
    for (int i = tid; i < n; i += 256) p[i] = y0 > 0 ? pic[(size_t)(y0 - 1) * a.row_stride + i] : (uint8_t)0;
  }
  for (int y = y0; y < y1; ++y) {
    uint8_t* c = raw[y & 1];
    const uint8_t* p = raw[(y + 1) & 1];
    __syncthreads();                                             // the row before is done with c, f, mlen, jmp, reach
    for (int i = tid; i < n; i += 256) c[i] = pic[(size_t)y * a.row_stride + i];
    __syncthreads();
    uint32_t sum[5] = {0u, 0u, 0u, 0u, 0u};
    for (int i = tid; i < n; i += 256) {
      const int x = c[i], l = i >= C ? c[i - C] : 0, u = p[i], ul = i >= C ? p[i - C] : 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) sum[k] += cost_of(residual(k, x, l, u, ul));
    }
    int kind = 0;
    uint32_t best = 0u;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const uint32_t t = block_sum(sum[k], red);                 // <= 4096 * 128
      if (k == 0 || t < best) {
        best = t;
        kind = k;
      }
    }
    uint32_t as = 0u, bs = 0u;                                   // Adler sums of the row: bytes, bytes * (L - position)
    if (tid == 0) {
      f[0] = (uint8_t)kind;
      as = (uint32_t)kind;
      bs = (uint32_t)kind * (uint32_t)L;
    }
    for (int i = tid; i < n; i += 256) {
      const int x = c[i], l = i >= C ? c[i - C] : 0, u = p[i], ul = i >= C ? p[i - C] : 0;
      const uint32_t v = (uint32_t)residual(kind, x, l, u, ul) & 255u;
      f[1 + i] = (uint8_t)v;
      as += v;
      bs += v * (uint32_t)(n - i);                               // < 2^32: at most 255 * 4097 * 4098 / 2 over the row
    }
    as = block_sum(as, red);
    bs = block_sum(bs, red);                                     // f is complete behind its barriers
    if (tid == 0) {
      uint32_t* ri = info + (size_t)y * 4;
      ri[0] = as;
      ri[1] = bs;
    }
    // match lengths of the distances 1 and C: the first mismatch at or behind every position
    uint32_t z1 = 0xFFFFu, zc = 0xFFFFu;
    for (int j = s1 - 1; j >= s0; --j) {
      if (!(j >= 1 && f[j] == f[j - 1])) z1 = (uint32_t)j;
      if (!(j >= C && f[j] == f[j - C])) zc = (uint32_t)j;
    }
    scan[tid] = z1 | zc << 16;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {                    // inclusive suffix minimum of both halves
      const uint32_t u = tid + off < 256 ? scan[tid + off] : 0xFFFFFFFFu;
      __syncthreads();
      const uint32_t v = scan[tid];
      const uint32_t lo = (v & 0xFFFFu) < (u & 0xFFFFu) ? (v & 0xFFFFu) : (u & 0xFFFFu);
      const uint32_t hi = (v >> 16) < (u >> 16) ? (v >> 16) : (u >> 16);
      scan[tid] = lo | hi << 16;
      __syncthreads();
    }
    {
      const uint32_t behind = tid < 255 ? scan[tid + 1] : 0xFFFFFFFFu;
      int e1 = mini((int)(behind & 0xFFFFu), L), ec = mini((int)(behind >> 16), L);
      for (int j = s1 - 1; j >= s0; --j) {
        if (!(j >= 1 && f[j] == f[j - 1])) e1 = j;
        if (!(j >= C && f[j] == f[j - C])) ec = j;
        mlen[0][j] = (uint16_t)mini(e1 - j, kMaxMatch);
        mlen[1][j] = (uint16_t)mini(ec - j, kMaxMatch);
      }
    }
    __syncthreads();
    for (int j = tid; j <= L; j += 256) {                        // next(j); L is its own successor
      int nx = L;
      if (j < L) {
        const int m1 = mlen[0][j], mc = mlen[1][j], m = mc > m1 ? mc : m1;
        nx = j + (m >= kMinMatch ? m : 1);                       // <= L: a match ends inside the row
      }
      jmp[0][j] = (uint16_t)nx;
      reach[j] = (uint8_t)(j == 0);
    }
    __syncthreads();
    for (int k = 0; k < rounds; ++k) {                           // reach holds next^m(0) for every m < 2^k
      const uint16_t* src = jmp[k & 1];
      uint16_t* dst = jmp[(k + 1) & 1];
      for (int j = tid; j <= L; j += 256) {
        const int jj = mini((int)src[j], L);
        if (reach[j]) reach[jj] = 1;                             // a flag another thread sets in this round is as true
        dst[j] = src[jj];
      }
      __syncthreads();
    }
    for (int j = tid; j < L; j += 256) {
      uint32_t t = kSkip;
      if (reach[j]) {
        const int m1 = mlen[0][j], mc = mlen[1][j];
        const int di = mc > m1, m = di ? mc : m1;                // ties to the distance 1
        if (m >= kMinMatch) {
          t = 0x8000u | (uint32_t)di << 8 | (uint32_t)(m - 3);
          atomicAdd(&hist[257 + (c_len.e[m - 3] & 255u)], 1u);
          atomicAdd(&hist[kLit + di], 1u);
        } else {
          t = f[j];
          atomicAdd(&hist[t], 1u);
        }
      }
      tok[(size_t)y * wk.lp + j] = (uint16_t)t;
    }
  }
  __syncthreads();
  for (int i = tid; i < kHist; i += 256)
    if (hist[i]) atomicAdd(&ghist[i], hist[i]);
}

// ------------------------------------------------------------------------------------------ 2. code
// what one thread needs to build the block's code; LDS on the device
struct CodeWork {
  uint32_t hist[kHist];        // in: the picture's counts, end-of-block included
  uint16_t order[kLit];        // in: the used literal/length symbols by (count, symbol) ascending
  int nused;                   // in
  uint32_t weight[2 * kLit];
  uint16_t parent[2 * kLit];
  uint16_t depth[2 * kLit];
  uint16_t num[16];
  uint8_t lens[kLit + 4];      // literal/length lengths, then the HDIST distance lengths behind HLIT of them
  uint8_t rsym[kLit + 32], rval[kLit + 32];
  uint32_t ccnt[19];
  uint16_t corder[19];
  uint8_t clens[19];
  uint16_t ccode[19];
  uint32_t tab[kTabWords];     // out
};

__host__ __device__ inline uint32_t bit_reverse(uint32_t c, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((c >> i) & 1u) << (len - 1 - i);
  return r;
}

// png_encode.py code_lengths: cnt[order[i]], i < n, ascending by (count, symbol) -> lens[symbol] (zero before)
__host__ __device__ inline void limited_lengths(const uint32_t* cnt, const uint16_t* order, int n, int limit,
                                                CodeWork& w, uint8_t* lens) {
  if (n == 1) lens[order[0]] = 1;
  if (n < 2) return;
  for (int i = 0; i < n; ++i) w.weight[i] = cnt[order[i]];
  int leaf = 0, node = n;
  for (int made = n; made < 2 * n - 1; ++made) {
    uint32_t sum = 0;
    for (int k = 0; k < 2; ++k) {
      int pick;
      if (leaf < n && (node >= made || w.weight[leaf] <= w.weight[node])) pick = leaf++;
      else pick = node++;
      sum += w.weight[pick];
      w.parent[pick] = (uint16_t)made;
    }
    w.weight[made] = sum;
  }
  for (int l = 0; l <= 15; ++l) w.num[l] = 0;
  w.depth[2 * n - 2] = 0;
  for (int i = 2 * n - 3; i >= 0; --i) {
    const int d = w.depth[w.parent[i]] + 1;
    w.depth[i] = (uint16_t)d;
    if (i < n) ++w.num[d < limit ? d : limit];
  }
  uint32_t total = 0;
  for (int l = 1; l <= limit; ++l) total += (uint32_t)w.num[l] << (limit - l);
  for (int it = 0; it < kLit && total > (1u << limit); ++it) {   // every step takes one unit off; a clipped leaf added at most one
    --w.num[limit];
    for (int l = limit - 1; l > 0; --l)
      if (w.num[l]) {
        --w.num[l];
        w.num[l + 1] += 2;
        break;
      }
    --total;
  }
  int i = 0;
  for (int l = limit; l > 0; --l)
    for (int k = 0; k < w.num[l] && i < n; ++k) lens[order[i++]] = (uint8_t)l;
}

struct HeaderBits {
  uint32_t* w;
  int n;
  __host__ __device__ void put(uint32_t v, int len) {            // len <= 15, v below 1 << len
    if (len == 0 || n + len > kHdrWords * 32) return;
    w[n >> 5] |= v << (n & 31);
    if ((n & 31) + len > 32) w[(n >> 5) + 1] |= v >> (32 - (n & 31));
    n += len;
  }
};

__host__ __device__ inline uint32_t fixed_entry(int s) {
  const uint32_t len = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8;
  const uint32_t code = s < 144 ? 0x30 + s : s < 256 ? 0x190 + (s - 144) : s < 280 ? s - 256 : 0xC0 + (s - 280);
  return bit_reverse(code, (int)len) | len << 16;
}

// steps "lengths" to "choice" of the rule, from w.hist / w.order / w.nused into w.tab
__host__ __device__ inline void build_code(CodeWork& w, int C) {
  for (int i = 0; i < kLit + 4; ++i) w.lens[i] = 0;
  for (int i = 0; i < kTabWords; ++i) w.tab[i] = 0u;
  limited_lengths(w.hist, w.order, w.nused, 15, w, w.lens);
  int hlit = 257;
  for (int s = 257; s < 286; ++s)
    if (w.hist[s]) hlit = s + 1;
  // the distance symbols of the indices 0 and 1 are 0 and C - 1; a used one has length 1
  const uint32_t d0 = w.hist[kLit], d1 = w.hist[kLit + 1];
  const int hdist = d1 ? C : 1;
  uint8_t* seq = w.lens;                                         // the HLIT + HDIST lengths as one sequence
  for (int i = 0; i < 4; ++i) seq[hlit + i] = 0;
  if (d0) seq[hlit] = 1;
  if (d1) seq[hlit + C - 1] = 1;
  const int nseq = hlit + hdist;
  // the runs
  int nr = 0, prev = -1;
  for (int i = 0; i < 19; ++i) w.ccnt[i] = 0;
  for (int i = 0; i < nseq && nr < kLit + 32;) {
    const int v = seq[i];
    int r = 1;
    while (i + r < nseq && seq[i + r] == v) ++r;
    int sym, val, step;
    if (v == 0 && r >= 3) {
      step = r < 138 ? r : 138;
      sym = step <= 10 ? 17 : 18;
      val = step <= 10 ? step - 3 : step - 11;
      prev = 0;
    } else if (v == prev && r >= 3) {
      step = r < 6 ? r : 6;
      sym = 16;
      val = step - 3;
    } else {
      step = 1;
      sym = v;
      val = 0;
      prev = v;
    }
    w.rsym[nr] = (uint8_t)sym;
    w.rval[nr] = (uint8_t)val;
    ++nr;
    ++w.ccnt[sym];
    i += step;
  }
  // the code-length code: insertion sort of its used symbols by (count, symbol)
  int nc = 0;
  for (int s = 0; s < 19; ++s) {
    w.clens[s] = 0;
    if (!w.ccnt[s]) continue;
    int k = nc++;
    for (; k > 0 && w.ccnt[w.corder[k - 1]] > w.ccnt[s]; --k) w.corder[k] = w.corder[k - 1];
    w.corder[k] = (uint16_t)s;
  }
  limited_lengths(w.ccnt, w.corder, nc, 7, w, w.clens);
  {
    uint32_t code = 0;
    for (int l = 1; l <= 7; ++l) {
      for (int s = 0; s < 19; ++s)
        if (w.clens[s] == l) w.ccode[s] = (uint16_t)bit_reverse(code++, l);
      code <<= 1;
    }
  }
  int hclen = 4;
  for (int i = 0; i < 19; ++i)
    if (w.clens[kClenOrder[i]] && i + 1 > hclen) hclen = i + 1;
  HeaderBits hb{w.tab + kTabHdr, 0};
  hb.put(1u, 1);
  hb.put(2u, 2);
  hb.put((uint32_t)(hlit - 257), 5);
  hb.put((uint32_t)(hdist - 1), 5);
  hb.put((uint32_t)(hclen - 4), 4);
  for (int i = 0; i < hclen; ++i) hb.put(w.clens[kClenOrder[i]], 3);
  for (int i = 0; i < nr; ++i) {
    const int s = w.rsym[i];
    hb.put(w.ccode[s], w.clens[s]);
    hb.put(w.rval[i], s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
  }
  // the totals under both codes; the extra bits are the same in both
  uint32_t dyn = (uint32_t)hb.n + d0 + d1, fix = 3u + 5u * (d0 + d1);
  for (int s = 0; s < 286; ++s) {
    dyn += w.hist[s] * w.lens[s];
    fix += w.hist[s] * (fixed_entry(s) >> 16);
  }
  if (dyn < fix) {
    uint32_t code = 0;
    for (int l = 1; l <= 15; ++l) {
      for (int s = 0; s < hlit; ++s)
        if (w.lens[s] == l) w.tab[s] = bit_reverse(code++, l) | (uint32_t)l << 16;
      code <<= 1;
    }
    w.tab[kTabDist] = d0 ? 0u | 1u << 16 : 0u;
    w.tab[kTabDist + 1] = d1 ? (d0 ? 1u : 0u) | 1u << 16 : 0u;
    w.tab[kTabHdrBits] = (uint32_t)hb.n;
    w.tab[kTabMode] = 2u;
  } else {
    for (int s = 0; s < kLit; ++s) w.tab[s] = fixed_entry(s);
    w.tab[kTabDist] = bit_reverse(0u, 5) | 5u << 16;
    w.tab[kTabDist + 1] = bit_reverse((uint32_t)(C - 1), 5) | 5u << 16;
    for (int i = 0; i < kHdrWords; ++i) w.tab[kTabHdr + i] = 0u;
    w.tab[kTabHdr] = 3u;                                         // BFINAL 1, BTYPE 01
    w.tab[kTabHdrBits] = 3u;
    w.tab[kTabMode] = 1u;
  }
}

__global__ __launch_bounds__(320) void png_code_kernel(PngEncodeArgs a) {
  __shared__ CodeWork w;
  const int tid = threadIdx.x, b = blockIdx.x;
  const Work wk = work_of(a.B, a.H, a.W, a.C, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  uint32_t* ghist = reinterpret_cast<uint32_t*>(base + wk.hist) + (size_t)b * kHist;
  uint32_t* gtab = reinterpret_cast<uint32_t*>(base + wk.tab) + (size_t)b * kTabWords;
  const uint32_t cnt = ghist[tid] + (tid == 256 ? 1u : 0u);      // kHist threads; one end-of-block
  w.hist[tid] = cnt;
  ghist[tid] = 0u;                                               // zero for the next launch
  const bool used = tid < 286 && cnt > 0u;
  const int nused = __syncthreads_count(used);
  if (used) {
    int rank = 0;
    for (int s = 0; s < 286; ++s) {
      const uint32_t o = w.hist[s];
      rank += o > 0u && (o < cnt || (o == cnt && s < tid));
    }
    w.order[rank] = (uint16_t)tid;                               // ranks are a permutation of 0..nused-1
  }
  if (tid == 0) w.nused = nused;
  __syncthreads();
  if (tid == 0) build_code(w, a.C);
  __syncthreads();
  for (int i = tid; i < kTabWords; i += kHist) gtab[i] = w.tab[i];
}

// ------------------------------------------------------------------------------------------ 3. rowbits
// the bits of a token under the table: lit = the kLit + 2 literal/length and distance entries
__device__ __forceinline__ uint32_t token_bits(uint32_t t, const uint32_t* lit) {
  if (t == kSkip) return 0u;
  if (!(t & 0x8000u)) return lit[t & 255u] >> 16;
  const uint32_t e = c_len.e[t & 255u];
  return (lit[257 + (e & 255u)] >> 16) + ((e >> 8) & 255u) + (lit[kTabDist + ((t >> 8) & 1u)] >> 16);
}

__global__ __launch_bounds__(256) void png_rowbits_kernel(PngEncodeArgs a) {
  __shared__ uint32_t lit[kLit + 2];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63;
  const int L = a.W * a.C + 1;
  const Work wk = work_of(a.B, a.H, a.W, a.C, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  const uint16_t* tok = reinterpret_cast<const uint16_t*>(base) + (size_t)b * a.H * wk.lp;
  uint32_t* info = reinterpret_cast<uint32_t*>(base + wk.info) + (size_t)b * a.H * 4;
  const uint32_t* gtab = reinterpret_cast<const uint32_t*>(base + wk.tab) + (size_t)b * kTabWords;
  uint32_t* stream = reinterpret_cast<uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;
  for (int i = tid; i < kLit + 2; i += 256) lit[i] = gtab[i];
  const int per = (wk.sw + (int)gridDim.x - 1) / (int)gridDim.x;  // this workgroup's slice of the stream
  const int w0 = mini((int)blockIdx.x * per, wk.sw), w1 = mini(w0 + per, wk.sw);
  for (int i = w0 + tid; i < w1; i += 256) stream[i] = 0u;
  __syncthreads();
  const int y = blockIdx.x * 4 + (tid >> 6);
  if (y >= a.H) return;
  uint32_t bits = 0u;
  for (int j = lane; j < L; j += 64) bits += token_bits(tok[(size_t)y * wk.lp + j], lit);
  for (int off = 32; off > 0; off >>= 1) bits += __shfl_down(bits, off);
  if (lane == 0) info[(size_t)y * 4 + 2] = bits;                 // <= 4097 * 21
}

// ------------------------------------------------------------------------------------------ 4. bits
struct BitWriter {
  uint32_t* w;       // the next word of the stream
  uint32_t* end;     // behind the words the picture owns: nothing is written there, whatever the lengths said
  uint64_t acc;      // the low n bits are pending, the lowest goes first
  int n;             // < 32 between calls
  __device__ __forceinline__ void put(uint32_t v, int len) {     // len <= 31
    acc |= (uint64_t)v << n;
    n += len;
    if (n >= 32) {
      if (w < end) atomicOr(w, (uint32_t)acc);
      ++w;
      acc >>= 32;
      n -= 32;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n && w < end) atomicOr(w, (uint32_t)acc);
  }
};

// the bits of the picture's block and whether its file overflows the cap, from the rows' lengths
__device__ __forceinline__ bool overflows(uint32_t total_bits, int cap) {
  return (uint64_t)((total_bits + 7u) / 8u) + kFileOverhead > (uint64_t)cap;
}

__global__ __launch_bounds__(256) void png_bits_kernel(PngEncodeArgs a) {
  __shared__ uint32_t lit[kLit + 4];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63;
  const int L = a.W * a.C + 1, H = a.H;
  const Work wk = work_of(a.B, H, a.W, a.C, a.cap);
  uint8_t* base = reinterpret_cast<uint8_t*>(a.work);
  const uint16_t* tok = reinterpret_cast<const uint16_t*>(base) + (size_t)b * H * wk.lp;
  const uint32_t* info = reinterpret_cast<const uint32_t*>(base + wk.info) + (size_t)b * H * 4;
  const uint32_t* gtab = reinterpret_cast<const uint32_t*>(base + wk.tab) + (size_t)b * kTabWords;
  uint32_t* stream = reinterpret_cast<uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;
  for (int i = tid; i < kLit + 4; i += 256) lit[i] = gtab[i];
  __syncthreads();
  const int y = blockIdx.x * 4 + (tid >> 6);
  if (y >= H) return;
  uint32_t pre = 0u, all = 0u;                                   // the bits of the rows in front, of every row
  for (int r = lane; r < H; r += 64) {
    const uint32_t v = info[(size_t)r * 4 + 2];
    all += v;
    if (r < y) pre += v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    pre += __shfl_xor(pre, off);
    all += __shfl_xor(all, off);
  }
  const uint32_t hdr = lit[kTabHdrBits], eob = lit[256];
  const uint32_t total = hdr + all + (eob >> 16);                // < 2^32: at most 1024 * 4097 * 21 + 4515
  if (overflows(total, a.cap)) return;                           // the same for every wave of the picture
  uint32_t* end = stream + wk.sw;
  const int ch = (L + 63) / 64;
  const int s0 = mini(lane * ch, L), s1 = mini(s0 + ch, L);
  uint32_t mine = 0u;
  for (int j = s0; j < s1; ++j) mine += token_bits(tok[(size_t)y * wk.lp + j], lit);
  uint32_t incl = mine;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off);
    if (lane >= off) incl += v;
  }
  const uint32_t at = hdr + pre + incl - mine;
  BitWriter bw{stream + (at >> 5), end, 0ull, (int)(at & 31u)};  // the bits in front of `at` are another lane's: 0 here
  for (int j = s0; j < s1; ++j) {
    const uint32_t t = tok[(size_t)y * wk.lp + j];
    if (t == kSkip) continue;
    if (!(t & 0x8000u)) {
      const uint32_t e = lit[t & 255u];
      bw.put(e & 0xFFFFu, (int)(e >> 16));
    } else {
      const uint32_t x = c_len.e[t & 255u], e = lit[257 + (x & 255u)], d = lit[kTabDist + ((t >> 8) & 1u)];
      const int len = (int)(e >> 16), xb = (int)((x >> 8) & 255u);
      bw.put((e & 0xFFFFu) | (x >> 16) << len, len + xb);        // <= 15 + 5 bits
      bw.put(d & 0xFFFFu, (int)(d >> 16));
    }
  }
  bw.flush();
  if (y == 0)
    for (int i = lane; i < (int)(hdr + 31u) / 32 && i < kHdrWords && i < wk.sw; i += 64)
      if (gtab[kTabHdr + i]) atomicOr(stream + i, gtab[kTabHdr + i]);
  if (y == H - 1 && lane == 0) {
    const uint32_t p = total - (eob >> 16);
    BitWriter ew{stream + (p >> 5), end, 0ull, (int)(p & 31u)};
    ew.put(eob & 0xFFFFu, (int)(eob >> 16));
    ew.flush();
  }
}

// ------------------------------------------------------------------------------------------ 5. file
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// a * b modulo the CRC polynomial, both in the reflected form (x^0 is bit 31)
__host__ __device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if ((a >> (31 - i)) & 1u) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}

// x^(8 n) modulo the CRC polynomial, n < 2^24
__host__ __device__ inline uint32_t crc_x8n(uint32_t n) {
  uint32_t p = 0x80000000u, sq = 0x00800000u;
  for (int i = 0; i < 24; ++i) {
    if ((n >> i) & 1u) p = crc_mul(sq, p);
    sq = crc_mul(sq, sq);
  }
  return p;
}

__host__ __device__ inline uint32_t crc_entry(uint32_t i) {
  for (int k = 0; k < 8; ++k) i = (i & 1u) ? (i >> 1) ^ kCrcPoly : i >> 1;
  return i;
}

__device__ __forceinline__ uint32_t be_byte(uint32_t v, uint32_t i) { return (v >> (24 - 8 * i)) & 255u; }

__global__ __launch_bounds__(kFileThreads) void png_file_kernel(PngEncodeArgs a) {
  __shared__ uint32_t part[kFileThreads];
  __shared__ uint32_t crctab[256];
  __shared__ uint32_t acc[4];                                    // the rows' bits, Adler b, the CRC
  const int tid = threadIdx.x, b = blockIdx.x, H = a.H;
  const uint32_t L = (uint32_t)(a.W * a.C + 1);
  const Work wk = work_of(a.B, H, a.W, a.C, a.cap);
  const uint8_t* base = reinterpret_cast<const uint8_t*>(a.work);
  const uint32_t* info = reinterpret_cast<const uint32_t*>(base + wk.info) + (size_t)b * H * 4;
  const uint32_t* gtab = reinterpret_cast<const uint32_t*>(base + wk.tab) + (size_t)b * kTabWords;
  const uint32_t* stream = reinterpret_cast<const uint32_t*>(base + wk.stream) + (size_t)b * wk.sw;
  uint32_t* row = a.out + (size_t)b * a.ldo;
  const uint32_t capw = ((uint32_t)a.cap + 3u) / 4u;
  for (int i = tid; i < a.nfront; i += kFileThreads) row[i] = a.front[(size_t)b * a.ldf + i];
  if (tid < 4) acc[tid] = 0u;
  if (tid < 256) crctab[tid] = crc_entry((uint32_t)tid);
  __syncthreads();
  uint32_t as = 0u, bs = 0u;
  if (tid < H) {                                                 // H <= kFileThreads
    atomicAdd(&acc[0], info[(size_t)tid * 4 + 2]);
    as = info[(size_t)tid * 4] % 65521u;
    bs = info[(size_t)tid * 4 + 1] % 65521u;
  }
  part[tid] = as;
  __syncthreads();
  const uint32_t total = gtab[kTabHdrBits] + acc[0] + (gtab[256] >> 16);
  const uint32_t nbytes = (total + 7u) / 8u;
  if (overflows(total, a.cap)) {                                 // the whole workgroup
    if (tid == 0) row[a.nfront] = 0u;
    for (uint32_t i = tid; i < capw; i += kFileThreads) row[a.nfront + 1 + i] = 0u;
    return;
  }
  for (int off = 1; off < kFileThreads; off <<= 1) {             // inclusive prefix sums of the rows' a, modulo 65521
    const uint32_t v = tid >= off ? part[tid - off] : 0u;
    __syncthreads();
    part[tid] = (part[tid] + v) % 65521u;
    __syncthreads();
  }
  if (tid < H) {                                                 // b grows by the row's b and L times the a in front of it
    const uint32_t before = (1u + part[tid] + 65521u - as) % 65521u;
    atomicAdd(&acc[1], (bs + (uint32_t)(((uint64_t)L * before) % 65521u)) % 65521u);   // < 2^26 in all
  }
  __syncthreads();
  const uint32_t adler = (acc[1] % 65521u) << 16 | (1u + part[kFileThreads - 1]) % 65521u;
  // the IDAT chunk behind its length: "IDAT", 78 01, the block, the Adler-32
  const uint32_t n = nbytes + 10u;
  auto chunk_byte = [&](uint32_t k) -> uint32_t {                // k < n; stream words below ceil(nbytes / 4) <= sw
    if (k < 4u) return be_byte(0x49444154u, k);
    if (k < 6u) return k == 4u ? 0x78u : 0x01u;
    if (k < 6u + nbytes) return (stream[(k - 6u) >> 2] >> (8u * ((k - 6u) & 3u))) & 255u;
    return be_byte(adler, k - 6u - nbytes);
  };
  {
    const uint32_t piece = (n + kFileThreads - 1) / kFileThreads;
    const uint32_t k0 = (uint32_t)tid * piece < n ? (uint32_t)tid * piece : n, k1 = k0 + piece < n ? k0 + piece : n;
    uint32_t c = tid == 0 ? 0xFFFFFFFFu : 0u;
    for (uint32_t k = k0; k < k1; ++k) c = crctab[(c ^ chunk_byte(k)) & 255u] ^ (c >> 8);
    if (k1 > k0) atomicXor(&acc[2], crc_mul(crc_x8n(n - k1), c));
  }
  __syncthreads();
  const uint32_t crc = acc[2] ^ 0xFFFFFFFFu, flen = nbytes + kFileOverhead;
  auto file_byte = [&](uint32_t k) -> uint32_t {
    if (k < 33u) return a.head[k];
    if (k < 37u) return be_byte(n - 4u, k - 33u);
    if (k < 37u + n) return chunk_byte(k - 37u);
    if (k < 41u + n) return be_byte(crc, k - 37u - n);
    if (k < flen) {
      const uint32_t i = k - 41u - n;                            // IEND: length 0, the type, its CRC
      return i < 4u ? 0u : i < 8u ? be_byte(0x49454E44u, i - 4u) : be_byte(0xAE426082u, i - 8u);
    }
    return 0u;
  };
  for (uint32_t i = tid; i < capw; i += kFileThreads)            // flen <= cap: the file and the zeros behind it
    row[a.nfront + 1 + i] = file_byte(4 * i) | file_byte(4 * i + 1) << 8 | file_byte(4 * i + 2) << 16 | file_byte(4 * i + 3) << 24;
  if (tid == 0) row[a.nfront] = flen;
}

// ------------------------------------------------------------------------------------------ host
uint32_t host_crc(const uint8_t* p, int n) {
  uint32_t c = 0xFFFFFFFFu;
  for (int i = 0; i < n; ++i) c = crc_entry((c ^ p[i]) & 255u) ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

bool sizes_ok(int B, int H, int W, int C, int cap) {
  return B >= 1 && B <= 65535 && H >= 1 && H <= kPngEncMaxSide && W >= 1 && W <= kPngEncMaxSide && (C == 3 || C == 4) &&
         cap >= 1 && cap <= kPngEncMaxCap;
}

bool valid(const PngEncodeArgs& a) {
  if (!a.inp || !a.out || !a.work) return false;
  if (reinterpret_cast<uintptr_t>(a.out) % 4 || reinterpret_cast<uintptr_t>(a.work) % 16) return false;
  if (!sizes_ok(a.B, a.H, a.W, a.C, a.cap)) return false;
  if (a.row_stride < (int64_t)a.W * a.C || a.ldi < a.row_stride * a.H) return false;
  if (a.nfront < 0 || a.ldf < a.nfront) return false;
  if (a.nfront > 0 && (!a.front || reinterpret_cast<uintptr_t>(a.front) % 4)) return false;
  return (int64_t)a.ldo >= (int64_t)a.nfront + 1 + (a.cap + 3) / 4;
}

}  // namespace

size_t png_encode_workspace(int B, int H, int W, int C, int cap) {
  return sizes_ok(B, H, W, C, cap) ? work_of(B, H, W, C, cap).bytes : 0;
}

hipError_t png_encode(const PngEncodeArgs& args, hipStream_t s) {
  if (!valid(args)) return hipErrorInvalidValue;
  PngEncodeArgs a = args;
  static const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
  memcpy(a.head, sig, 16);
  const uint8_t ihdr[13] = {(uint8_t)(a.W >> 24), (uint8_t)(a.W >> 16), (uint8_t)(a.W >> 8), (uint8_t)a.W,
                            (uint8_t)(a.H >> 24), (uint8_t)(a.H >> 16), (uint8_t)(a.H >> 8), (uint8_t)a.H,
                            8, (uint8_t)(a.C == 3 ? 2 : 6), 0, 0, 0};
  memcpy(a.head + 16, ihdr, 13);
  const uint32_t crc = host_crc(a.head + 12, 17);
  for (int i = 0; i < 4; ++i) a.head[29 + i] = (uint8_t)(crc >> (24 - 8 * i));
  const unsigned bands = (unsigned)((a.H + kBand - 1) / kBand), quads = (unsigned)((a.H + 3) / 4);
  hipLaunchKernelGGL(png_filter_kernel, dim3(bands, (unsigned)a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(png_code_kernel, dim3((unsigned)a.B), dim3(kHist), 0, s, a);
  hipLaunchKernelGGL(png_rowbits_kernel, dim3(quads, (unsigned)a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(png_bits_kernel, dim3(quads, (unsigned)a.B), dim3(256), 0, s, a);
  hipLaunchKernelGGL(png_file_kernel, dim3((unsigned)a.B), dim3(kFileThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
