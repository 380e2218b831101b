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
// The step code (table lookup, symbol step, f_i, block addressing) is runtime/jpeg_huff.h, shared
// with the host emulation jpeg_huff_cpu, which the CPU tests and the sanitizer fuzzer run.
//
// Every loop bound is independent of the data being well formed: the symbol loop consumes at
// least one bit per iteration up to the subsequence's end, the round loop stops at T, the chunk
// loop at ceil(nsub / T). Barriers sit where all threads arrive with the same trip count (the
// round loop leaves through a workgroup-wide OR). No workgroup waits for another. A per-image
// error word means "ask jpeg_parse"; only the write pass, which sees true states, raises it.
#include "common.h"
#include "launch.h"
#include "runtime/jpeg_huff.h"

namespace kdl {

namespace {

constexpr int T = kJpegHuffChunk;
constexpr uint32_t S = kJpegHuffSubBits;

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

__global__ __launch_bounds__(T) void jpeg_huff_kernel(JpegHuffArgs a) {
  __shared__ uint32_t s_words[kJpegHuffLdsWords];
  __shared__ uint32_t s_tab[6 * kJpegHuffTabWords];
  __shared__ JpegHuffDesc sd;
  __shared__ uint32_t s_p[T], s_bk[T], s_cnt[T];
  __shared__ uint8_t s_zz[64];
  __shared__ uint32_t s_err;
  const int tid = threadIdx.x, img = blockIdx.x;
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.desc + img);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&sd);
    for (int i = tid; i < (int)(sizeof(JpegHuffDesc) / 4); i += T) dst[i] = src[i];
  }
  if (tid < 64) s_zz[tid] = c_zigzag[tid];
  if (tid == 0) s_err = 0;
  __syncthreads();

  for (int t = 0; t < 6; ++t) {              // the image's tables; one outside the staging reads as "no code"
    const uint64_t at = sd.tab_off[t];
    const bool ok = at % 4 == 0 && at <= a.stage_cap && (uint64_t)kJpegHuffTabBytes <= a.stage_cap - at;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.stage + at);
    for (int i = tid; i < kJpegHuffTabWords; i += T) s_tab[t * kJpegHuffTabWords + i] = ok ? src[i] : 0u;
  }
  const int ncomp = sd.ncomp == 1 ? 1 : 3;
  for (int c = 0; c < ncomp; ++c) {          // step 8: the write pass stores the non-zero coefficients only
    const uint64_t at = sd.coef_off[c], nc = (uint64_t)(uint32_t)sd.bw[c] * (uint32_t)sd.bh[c] * 64;
    if (at % 8 || at > a.coef_cap || nc > a.coef_cap - at) {
      if (tid == 0) s_err = 1;
      continue;
    }
    uint4* dst = reinterpret_cast<uint4*>(a.coef + at);
    for (uint64_t i = tid; i < nc / 8; i += T) dst[i] = make_uint4(0, 0, 0, 0);
  }
  const uint32_t nbits = sd.nbits;
  const bool scan_ok = sd.scan_off % 4 == 0 && sd.scan_off <= a.stage_cap && sd.scan_bytes <= a.stage_cap - sd.scan_off &&
                       (uint64_t)nbits <= 8ull * sd.scan_bytes && nbits < (1u << 30) && sd.nb >= 1 && sd.nb <= 6 &&
                       sd.mx >= 1;
  const uint32_t* words = reinterpret_cast<const uint32_t*>(a.stage + (scan_ok ? sd.scan_off : 0));
  const uint32_t nwords = scan_ok ? sd.scan_bytes / 4 : 0;
  const uint32_t nsub = scan_ok ? (nbits + S - 1) / S : 0;
  const uint32_t nchunk = (nsub + T - 1) / T;
  DevMem m{s_words, 0, s_tab, s_zz, a.coef, a.coef_cap};
  JpegHuffState entry{0, 0};
  uint32_t base = 0, most_rounds = 0, err = 0;

  for (uint32_t ch = 0; ch < nchunk; ++ch) {
    __syncthreads();                         // the planes are clear / the last chunk's readers are done
    m.w0 = ch * (uint32_t)kJpegHuffChunkWords;
    for (uint32_t r = tid; r < (uint32_t)kJpegHuffStaged; r += T) {
      const uint32_t w = m.w0 + r;
      s_words[jpeg_huff_lds_index(r)] = w < nwords ? words[w] : 0u;
    }
    __syncthreads();
    // subsequences that start behind the data decode nothing and stay out of the rounds: they
    // would hand a change on one thread per round (only the last chunk has any)
    const uint32_t left = nsub - ch * (uint32_t)T;
    const bool live = (uint32_t)tid < left;
    const uint32_t stop = (ch * (uint32_t)T + tid + 1) * S;
    const uint32_t end = stop < nbits ? stop : nbits;
    JpegHuffState last = tid ? JpegHuffState{(ch * (uint32_t)T + tid) * S, 0} : entry;
    JpegHuffState ex = last;
    uint32_t cnt = 0, unused = 0;
    if (live) cnt = jpeg_huff_run<false>(sd, m, &ex, end, 0, &unused);            // steps 1, 2
    s_p[tid] = ex.p;
    s_bk[tid] = ex.bk;
    __syncthreads();
    uint32_t r = 0;
    for (; r < (uint32_t)T; ++r) {                                                 // steps 3, 4
      const JpegHuffState in = tid ? JpegHuffState{s_p[tid - 1], s_bk[tid - 1]} : entry;
      __syncthreads();                       // everybody has read its input before anybody writes
      int changed = 0;
      if (tid && live && !(in == last)) {
        last = in;
        JpegHuffState e = in;
        cnt = jpeg_huff_run<false>(sd, m, &e, end, 0, &unused);
        changed = !(e == ex);
        ex = e;
        s_p[tid] = e.p;
        s_bk[tid] = e.bk;
      }
      if (!__syncthreads_or(changed)) break;                                       // uniform
    }
    most_rounds = r + 1 > most_rounds ? r + 1 : most_rounds;
    const uint32_t incl = block_scan(s_cnt, tid, cnt);                             // step 5
    const uint32_t total = s_cnt[T - 1];
    if (live) {                                                                    // step 6
      JpegHuffState st = tid ? JpegHuffState{s_p[tid - 1], s_bk[tid - 1]} : entry;
      jpeg_huff_run<true>(sd, m, &st, end, base + (incl - cnt), &err);
    }
    entry = JpegHuffState{s_p[T - 1], s_bk[T - 1]};
    base += total;
  }
  if (err) s_err = 1;
  __syncthreads();
  if (tid == 0) {
    a.status[2 * img] = (s_err || !scan_ok || base < sd.nblocks) ? 1u : 0u;   // data that ends before the last MCU
    a.status[2 * img + 1] = most_rounds;
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

// every offset the kernels will follow, checked against the capacities of the call
bool valid(const JpegHuffArgs& a) {
  if (!a.desc || !a.h_desc || !a.stage || !a.coef || !a.status) return false;
  if (a.n < 1 || a.n > 65535 || a.status_cap < 2 * a.n) return false;
  if (reinterpret_cast<uintptr_t>(a.stage) % 4 || reinterpret_cast<uintptr_t>(a.coef) % 16) return false;
  for (int i = 0; i < a.n; ++i)
    if (!jpeg_huff_desc_valid(a.h_desc[i], a.stage_cap, a.coef_cap)) return false;
  return true;
}

}  // namespace

hipError_t jpeg_huff_decode(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)a.n), dim3(T), 0, s, a);
  return hipGetLastError();
}

hipError_t jpeg_dc_scan(const JpegHuffArgs& a, hipStream_t s) {
  if (!valid(a)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(jpeg_dc_kernel, dim3((unsigned)a.n, 3), dim3(T), 0, s, a);
  return hipGetLastError();
}

}  // namespace kdl
