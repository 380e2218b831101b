// Baseline JPEG entropy (Huffman) decode on the GPU: the opt-in front half of serving_bytes
// (kdl/serving/jpeg.py, entropy="gpu"). The host has walked the markers, built the code tables
// and removed the byte stuffing (jpeg_scan_prepare, runtime/jpeg.cpp); two launches turn the
// scans of a whole request into the coefficient planes that jpeg_idct_u8 reads:
//   jpeg_huff_decode  one workgroup per image. It clears the image's planes, then takes the scan
//                     in chunks of T subsequences of S bits, one thread per subsequence: a cold
//                     decode from (i*S, 0, 0), exit[i] = f_i(exit[i-1]) iterated to its fixed
//                     point (exit[-1] is the chunk's true entry, so the fixed point is the
//                     sequential decode and is reached after at most T rounds), an exclusive scan
//                     of the blocks-completed counts, and a write pass from the true entry states
//                     that stores the AC values and the DC differences.
//   jpeg_dc_scan      DC differences -> DC values: an inclusive prefix sum per component in scan
//                     (MCU) order, wrapping to int16 as the host decoder's predictor does.
// Files with restart intervals (entropy="gpu_rst") take two launches of their own:
//   jpeg_huff_rst_decode  one workgroup per (image, group of intervals). Every interval starts on a
//                     word boundary with the state (its first bit, 0, 0) and owns the blocks of its
//                     MCUs, so nothing has to be guessed: a group is a run of consecutive intervals
//                     that fits one chunk -- a thread owns subsequence s of interval j, the thread
//                     of an interval's first subsequence enters with the true state and never
//                     re-runs, and the rounds end after at most the longest interval's
//                     subsequences -- or one longer interval, walked in chunks like a whole scan.
//                     The workgroup clears the blocks of its own MCUs; the block positions come from
//                     the scan of the counts, taken per interval; the write pass stops behind the
//                     interval's last block and raises the error word when the interval completes
//                     fewer blocks than it owns or its last block used bits past its end.
//   jpeg_dc_rst_scan  the DC sums per (interval, component), one wave each.
// Both decode kernels run the same per-chunk procedure (decode_chunk, decode_walk below).
// The step code (table lookup, symbol step, f_i, block addressing) is runtime/jpeg_huff.h, shared
// with the host emulation jpeg_huff_cpu, which the CPU tests and the sanitizer fuzzers run.
//
// Every loop bound is independent of the data being well formed: the symbol loop consumes at
// least one bit per iteration up to the subsequence's end, the round loop stops at T, the chunk
// loop at ceil(nsub / T). Barriers sit where all threads arrive with the same trip count (the
// round loop leaves through a workgroup-wide OR). No workgroup waits for another: the workgroups
// of one image meet only in its two status words, which the launcher clears on the stream and the
// kernel combines with atomicOr / atomicMax. A per-image error word means "ask jpeg_parse"; only
// the write pass, which sees true states, and the checks on the descriptor raise it.
#include "common.h"
#include "launch.h"
#include "runtime/jpeg_huff.h"

namespace kdl {

namespace {

constexpr int T = kJpegHuffChunk;

__constant__ uint8_t c_zigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                     12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                     58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the accesses of the shared decode code: the staged chunk and the tables in LDS, the
// coefficients in global memory, each checked against its capacity
struct DevMem {
  const uint32_t* lds;
  uint32_t w0;                 // first scan word of the staged chunk
  const uint32_t* tabs;
  const uint8_t* zig;
  int16_t* coef;
  uint64_t coef_cap;
  __device__ uint32_t word(uint32_t w) const {
    const uint32_t r = w - w0;
    return r < (uint32_t)kJpegHuffStaged ? lds[jpeg_huff_lds_index(r)] : 0u;
  }
  __device__ const uint32_t* table(int t) const { return tabs + ((unsigned)t < 6u ? t : 0) * kJpegHuffTabWords; }
  __device__ void store(uint64_t off, int16_t v) const {
    if (off < coef_cap) coef[off] = v;
  }
  __device__ uint32_t zz(uint32_t k) const { return zig[k & 63u]; }
};

// inclusive sum of one value per thread over the workgroup; every thread calls it
__device__ uint32_t block_scan(uint32_t* s, int tid, uint32_t v) {
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < T; off <<= 1) {
    const uint32_t add = tid >= off ? s[tid - off] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  return s[tid];
}

// what a decode workgroup keeps in LDS
struct Lds {
  uint32_t words[kJpegHuffLdsWords];
  uint32_t tab[6 * kJpegHuffTabWords];
  JpegHuffDesc sd;
  uint32_t p[T], bk[T], cnt[T];
  uint32_t own[T];             // jpeg_huff_rst_kernel: the interval (of its group) that a thread works for
  uint8_t zz[64];
  uint32_t err, most;
};

// descriptor, zigzag order and the image's tables; a table outside the staging reads as "no code"
__device__ __forceinline__ void load_image(Lds& L, const JpegHuffArgs& a, int img, int tid) {
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.desc + img);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&L.sd);
    for (int i = tid; i < (int)(sizeof(JpegHuffDesc) / 4); i += T) dst[i] = src[i];
  }
  if (tid < 64) L.zz[tid] = c_zigzag[tid];
  if (tid == 0) L.err = L.most = 0;
  __syncthreads();
  for (int t = 0; t < 6; ++t) {
    const uint64_t at = L.sd.tab_off[t];
    const bool ok = at % 4 == 0 && at <= a.stage_cap && (uint64_t)kJpegHuffTabBytes <= a.stage_cap - at;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.stage + at);
    for (int i = tid; i < kJpegHuffTabWords; i += T) L.tab[t * kJpegHuffTabWords + i] = ok ? src[i] : 0u;
  }
}

__device__ bool scan_ok(const JpegHuffDesc& sd, uint64_t stage_cap) {
  return sd.scan_off % 4 == 0 && sd.scan_off <= stage_cap && sd.scan_bytes <= stage_cap - sd.scan_off &&
         (uint64_t)sd.nbits <= 8ull * sd.scan_bytes && sd.nbits < (1u << 30) && sd.nb >= 1 && sd.nb <= 6 && sd.mx >= 1;
}

// One chunk, staged from scan word w0 of ``words`` (words from w_end on read as zero), thread tid
// being lane ``l`` of it: the cold pass, exit[i] = f_i(exit[i-1]) to the fixed point in at most
// ``bound`` rounds (uniform), the scan of the blocks-completed counts and the write pass. Every
// thread calls it. Leaves the exit states in L.p / L.bk and the inclusive sums in L.cnt; *incl is
// the thread's own. Returns the rounds taken.
__device__ __forceinline__ uint32_t decode_chunk(Lds& L, DevMem& m, const uint32_t* words, uint32_t w0, uint32_t w_end,
                                 const JpegHuffLane& l, uint32_t bound, int tid, uint32_t* err, uint32_t* incl) {
  __syncthreads();                           // the planes are clear / the last chunk's readers are done
  m.w0 = w0;
  for (uint32_t r = tid; r < (uint32_t)kJpegHuffStaged; r += T) {
    const uint64_t w = (uint64_t)w0 + r;
    L.words[jpeg_huff_lds_index(r)] = w < w_end ? words[w] : 0u;
  }
  __syncthreads();
  // subsequences that start behind the data are not live: they decode nothing and stay out of the
  // rounds, where they would hand a change on one thread per round
  JpegHuffState last = l.in0, ex = l.in0;
  uint32_t cnt = 0, unused = 0;
  if (l.live) cnt = jpeg_huff_run<false>(L.sd, m, &ex, l.end, 0, &unused);            // steps 1, 2
  L.p[tid] = ex.p;
  L.bk[tid] = ex.bk;
  __syncthreads();
  const bool chained = tid && !l.head;       // takes the exit of the thread before it
  uint32_t r = 0;
  for (; r < bound; ++r) {                                                             // steps 3, 4
    const JpegHuffState in = chained ? JpegHuffState{L.p[tid - 1], L.bk[tid - 1]} : l.in0;
    __syncthreads();                         // everybody has read its input before anybody writes
    int changed = 0;
    if (chained && l.live && !(in == last)) {
      last = in;
      JpegHuffState e = in;
      cnt = jpeg_huff_run<false>(L.sd, m, &e, l.end, 0, &unused);
      changed = !(e == ex);
      ex = e;
      L.p[tid] = e.p;
      L.bk[tid] = e.bk;
    }
    if (!__syncthreads_or(changed)) break;                                             // uniform
  }
  *incl = block_scan(L.cnt, tid, cnt);                                                 // step 5
  if (l.live) {                                                                        // step 6
    JpegHuffState st = chained ? JpegHuffState{L.p[tid - 1], L.bk[tid - 1]} : l.in0;
    const uint32_t seg = l.seg < (uint32_t)tid ? l.seg : (uint32_t)tid;
    const uint32_t g = l.g0 + (*incl - cnt) - (seg ? L.cnt[seg - 1] : 0u);
    jpeg_huff_run_to<true>(L.sd, m, &st, l.end, g, l.g_end, l.p_end, err);
  }
  return r + 1;
}

// A walk in chunks over ``bits`` bits from scan word ``word`` into the blocks [g0, g_end): a whole
// scan, or one restart interval longer than a chunk. Returns the most rounds of a chunk.
__device__ __forceinline__ uint32_t decode_walk(Lds& L, DevMem& m, const uint32_t* words, uint32_t nwords, uint32_t word, uint32_t bits,
                                uint32_t g0, uint32_t g_end, int tid, uint32_t* err) {
  const uint32_t nchunk = (jpeg_huff_nsub(bits) + T - 1) / T;
  const uint64_t w_lim = (uint64_t)word + jpeg_huff_interval_words(bits);
  const uint32_t w_end = (uint32_t)(w_lim < nwords ? w_lim : nwords);
  JpegHuffState entry{word * 32u, 0};
  uint32_t base = g0, most = 0, incl;
  for (uint32_t ch = 0; ch < nchunk; ++ch) {
    const JpegHuffLane l = jpeg_huff_walk_lane(word * 32u, bits, ch, (uint32_t)tid, entry, base, g_end);
    const uint32_t r = decode_chunk(L, m, words, word + ch * (uint32_t)kJpegHuffChunkWords, w_end, l, (uint32_t)T, tid, err,
                                    &incl);
    most = r > most ? r : most;
    entry = JpegHuffState{L.p[T - 1], L.bk[T - 1]};
    base += L.cnt[T - 1];
  }
  if (base < g_end) *err = 1;                // data that ends before the last MCU
  return most;
}

__global__ __launch_bounds__(T) void jpeg_huff_kernel(JpegHuffArgs a) {
  __shared__ Lds L;
  const int tid = threadIdx.x, img = blockIdx.x;
  load_image(L, a, img, tid);
  const JpegHuffDesc& sd = L.sd;
  const int ncomp = sd.ncomp == 1 ? 1 : 3;
  for (int c = 0; c < ncomp; ++c) {          // step 8: the write pass stores the non-zero coefficients only
    const uint64_t at = sd.coef_off[c], nc = (uint64_t)(uint32_t)sd.bw[c] * (uint32_t)sd.bh[c] * 64;
    if (at % 8 || at > a.coef_cap || nc > a.coef_cap - at) {
      if (tid == 0) L.err = 1;
      continue;
    }
    uint4* dst = reinterpret_cast<uint4*>(a.coef + at);
    for (uint64_t i = tid; i < nc / 8; i += T) dst[i] = make_uint4(0, 0, 0, 0);
  }
  const bool ok = scan_ok(sd, a.stage_cap);
  const uint32_t* words = reinterpret_cast<const uint32_t*>(a.stage + (ok ? sd.scan_off : 0));
  DevMem m{L.words, 0, L.tab, L.zz, a.coef, a.coef_cap};
  uint32_t err = 0;
  const uint32_t most = decode_walk(L, m, words, ok ? sd.scan_bytes / 4 : 0, 0, ok ? sd.nbits : 0, 0, sd.nblocks, tid, &err);
  if (err) L.err = 1;
  __syncthreads();
  if (tid == 0) {
    a.status[2 * img] = (L.err || !ok) ? 1u : 0u;
    a.status[2 * img + 1] = most;
  }
}

// One workgroup per (image, group of restart intervals): blockIdx.y, blockIdx.x. Every interval
// starts at a known word with the state (its first bit, 0, 0) and owns the blocks of its MCUs, so
// the workgroups of an image share nothing but its two status words.
__global__ __launch_bounds__(T) void jpeg_huff_rst_kernel(JpegHuffArgs a) {
  __shared__ Lds L;
  const int tid = threadIdx.x, img = blockIdx.y;
  load_image(L, a, img, tid);
  const JpegHuffDesc& sd = L.sd;
  if (blockIdx.x >= sd.ngroup) return;       // uniform: the grid is as wide as the call's largest image
  const bool ok = scan_ok(sd, a.stage_cap) && sd.ri >= 1 && sd.int_off % 4 == 0 && sd.int_off <= a.stage_cap &&
                  8ull * sd.nint <= a.stage_cap - sd.int_off && sd.grp_off % 4 == 0 && sd.grp_off <= a.stage_cap &&
                  8ull * sd.ngroup <= a.stage_cap - sd.grp_off;
  const JpegHuffInterval* iv = reinterpret_cast<const JpegHuffInterval*>(a.stage + (ok ? sd.int_off : 0));
  JpegHuffGroup gr{0, 0};
  if (ok) gr = reinterpret_cast<const JpegHuffGroup*>(a.stage + sd.grp_off)[blockIdx.x];
  if (!ok || gr.count < 1 || gr.first >= sd.nint || gr.count > sd.nint - gr.first) {     // uniform
    if (tid == 0) atomicOr(&a.status[2 * img], 1u);
    return;
  }
  const uint32_t* words = reinterpret_cast<const uint32_t*>(a.stage + sd.scan_off);
  const uint32_t nwords = sd.scan_bytes / 4;
  const uint32_t g0 = jpeg_huff_interval_block(sd, gr.first);
  const uint32_t g1 = jpeg_huff_interval_block(sd, (uint64_t)gr.first + gr.count);
  // step 8 for the blocks of the group's own MCUs: eight 16-byte stores per block
  for (uint64_t i = tid; i < (uint64_t)(g1 - g0) * 8; i += T) {
    const uint64_t off = jpeg_huff_block_off(sd, g0 + (uint32_t)(i >> 3)) + (i & 7) * 8;
    if (off % 8 == 0 && off < a.coef_cap && a.coef_cap - off >= 8) *reinterpret_cast<uint4*>(a.coef + off) = make_uint4(0, 0, 0, 0);
  }
  DevMem m{L.words, 0, L.tab, L.zz, a.coef, a.coef_cap};
  uint32_t err = 0, most = 0;
  if (gr.count == 1) {                       // an interval of any length: walked in chunks like a whole scan
    const JpegHuffInterval one = iv[gr.first];
    const uint32_t bits = one.bits < (1u << 30) ? one.bits : (1u << 30) - 1;
    most = decode_walk(L, m, words, nwords, one.word, bits, g0, g1, tid, &err);
  } else {
    // thread i < count measures interval i of the group; the scan of the subsequence counts
    // gives every interval its run of threads, and every thread its interval and subsequence
    const uint32_t count = gr.count < (uint32_t)T ? gr.count : (uint32_t)T;
    JpegHuffInterval mine{0, 0};
    if ((uint32_t)tid < count) mine = iv[gr.first + tid];
    if (mine.bits >= (1u << 30)) mine.bits = (1u << 30) - 1;
    const uint32_t nsub = (uint32_t)tid < count ? jpeg_huff_nsub(mine.bits) : 0;
    L.own[tid] = ~0u;
    L.p[tid] = mine.word;
    L.bk[tid] = mine.bits;
    if (nsub) atomicMax(&L.most, nsub);
    const uint32_t start = block_scan(L.cnt, tid, nsub) - nsub;
    for (uint32_t s = 0; s < nsub && start + s < (uint32_t)T; ++s) L.own[start + s] = (uint32_t)tid;
    __syncthreads();
    const uint32_t o = L.own[tid];
    JpegHuffLane l{};
    if (o < count) {
      const JpegHuffInterval v{L.p[o], L.bk[o]};
      l = jpeg_huff_group_lane(sd, v, gr.first + o, (uint32_t)tid - (L.cnt[o] - jpeg_huff_nsub(v.bits)), (uint32_t)tid);
    }
    const bool tail = o < count && (tid + 1 == T || L.own[tid + 1] != o);      // its interval's last subsequence
    const JpegHuffInterval z{L.p[count - 1], L.bk[count - 1]};
    const uint64_t w_lim = (uint64_t)z.word + jpeg_huff_interval_words(z.bits);
    const uint32_t w0 = L.p[0], bound = L.most < (uint32_t)T ? L.most : (uint32_t)T;
    uint32_t incl;
    // decode_chunk starts with a barrier: everybody has read L.p, L.bk and L.cnt by then
    most = decode_chunk(L, m, words, w0, (uint32_t)(w_lim < nwords ? w_lim : nwords), l, bound, tid, &err, &incl);
    const uint32_t seg = l.seg < (uint32_t)tid ? l.seg : (uint32_t)tid;
    if (tail && incl - (seg ? L.cnt[seg - 1] : 0u) < l.g_end - l.g0) err = 1;   // an interval that ends before its last block
  }
  if (err) L.err = 1;
  __syncthreads();
  if (tid == 0) {
    if (L.err) atomicOr(&a.status[2 * img], 1u);
    atomicMax(&a.status[2 * img + 1], most);
  }
}

__global__ __launch_bounds__(T) void jpeg_dc_kernel(JpegHuffArgs a) {               // step 7
  __shared__ uint32_t s_sum[T];
  const JpegHuffDesc& d = a.desc[blockIdx.x];
  const int c = blockIdx.y, tid = threadIdx.x;
  if (c >= d.ncomp || d.h[c] < 1 || d.v[c] < 1 || d.mx < 1) return;                // uniform per workgroup
  const uint32_t n = (uint32_t)d.bw[c] * (uint32_t)d.bh[c], per = (n + T - 1) / T;
  const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
  uint32_t sum = 0;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint64_t off = jpeg_huff_dc_off(d, c, k);
    if (off < a.coef_cap) sum += (uint16_t)a.coef[off];
  }
  uint32_t acc = block_scan(s_sum, tid, sum) - sum;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint64_t off = jpeg_huff_dc_off(d, c, k);
    if (off >= a.coef_cap) continue;
    acc += (uint16_t)a.coef[off];
    a.coef[off] = (int16_t)(uint16_t)acc;
  }
}

// Step 7 with restart intervals: the predictors start again at every interval, so the sums are
// one short run per (interval, component). One wave takes one run, 64 blocks at a time with a
// carry, and the grid grows with the image; no barrier, so the waves need no common trip count.
constexpr int kDcWaves = 4;
__global__ __launch_bounds__(64 * kDcWaves) void jpeg_dc_rst_kernel(JpegHuffArgs a) {
  const JpegHuffDesc& d = a.desc[blockIdx.y];
  const int lane = threadIdx.x & 63;
  if ((d.ncomp != 1 && d.ncomp != 3) || d.ri < 1 || d.mx < 1) return;
  const uint32_t run = blockIdx.x * kDcWaves + (threadIdx.x >> 6);                 // uniform per wave
  const uint32_t j = run / (uint32_t)d.ncomp;
  const int c = (int)(run - j * (uint32_t)d.ncomp);
  if (j >= d.nint || d.h[c] < 1 || d.v[c] < 1) return;
  const uint64_t n = (uint64_t)(uint32_t)d.bw[c] * (uint32_t)d.bh[c], per = (uint64_t)d.ri * (uint32_t)(d.h[c] * d.v[c]);
  const uint64_t lo64 = (uint64_t)j * per < n ? (uint64_t)j * per : n;
  const uint32_t lo = (uint32_t)lo64, hi = (uint32_t)(lo64 + per < n ? lo64 + per : n);
  uint32_t carry = 0;
  for (uint32_t k0 = lo; k0 < hi; k0 += 64) {
    const uint32_t k = k0 + lane;
    const uint64_t off = k < hi ? jpeg_huff_dc_off(d, c, k) : ~0ull;
    const bool in = off < a.coef_cap;
    uint32_t v = in ? (uint16_t)a.coef[off] : 0u;
    for (int s = 1; s < 64; s <<= 1) {                                             // inclusive sum over the wave
      const uint32_t t = __shfl_up(v, s, 64);
      if (lane >= s) v += t;
    }
    v += carry;
    if (in) a.coef[off] = (int16_t)(uint16_t)v;
    carry = __shfl(v, 63, 64);
  }
}

// every offset the kernels will follow, checked against the capacities of the call
bool valid(const JpegHuffArgs& a, bool rst) {
  if (!a.desc || !a.h_desc || !a.stage || !a.coef || !a.status) return false;
  if (a.n < 1 || a.n > 65535 || a.status_cap < 2 * a.n) return false;
  if (reinterpret_cast<uintptr_t>(a.stage) % 4 || reinterpret_cast<uintptr_t>(a.coef) % 16) return false;
  if (rst && !a.h_stage) return false;
  for (int i = 0; i < a.n; ++i) {
    if (jpeg_huff_desc_is_rst(a.h_desc[i]) != rst) return false;     // each launcher takes its own kind of file
    if (!jpeg_huff_desc_valid(a.h_desc[i], a.stage_cap, a.coef_cap, rst ? a.h_stage : nullptr)) return false;
  }
  return true;
}

}  // namespace

hipError_t jpeg_huff_decode(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a, false)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)a.n), dim3(T), 0, s, a);
  return hipGetLastError();
}

hipError_t jpeg_dc_scan(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a, false)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)a.n, 3), dim3(T), 0, s, a);
  return hipGetLastError();
}

hipError_t jpeg_huff_rst_decode(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a, true)) return hipErrorInvalidValue;
  uint32_t groups = 1;
  for (int i = 0; i < a.n; ++i) groups = a.h_desc[i].ngroup > groups ? a.h_desc[i].ngroup : groups;
  const hipError_t e = hipMemsetAsync(a.status, 0, 2 * sizeof(uint32_t) * (size_t)a.n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(jpeg_huff_rst_kernel, dim3(groups, (unsigned)a.n), dim3(T), 0, s, a);
  return hipGetLastError();
}

hipError_t jpeg_dc_rst_scan(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a, true)) return hipErrorInvalidValue;
  uint32_t runs = 1;
  for (int i = 0; i < a.n; ++i) {
    const uint32_t r = a.h_desc[i].nint * (uint32_t)a.h_desc[i].ncomp;
    runs = r > runs ? r : runs;
  }
  hipLaunchKernelGGL(jpeg_dc_rst_kernel, dim3((runs + kDcWaves - 1) / kDcWaves, (unsigned)a.n), dim3(64 * kDcWaves), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
