// Baseline JPEG Huffman decode, the part shared by the GPU kernels (kernels/jpeg_huff.hip) and
// their host emulation (jpeg_huff_cpu in runtime/jpeg.cpp): the table lookup, one symbol step
// (p, b, k) -> (p', b', k') with its optional coefficient write, and f_i, the decode of one
// subsequence. Written ONCE here, the way jpeg.h shares the IDCT, so the emulation that the
// CPU tests and the sanitizer fuzzer run is the code the device runs.
//
// The scan is cut into subsequences of kJpegHuffSubBits bits; one workgroup decodes one image in
// chunks of kJpegHuffChunk subsequences, one thread per subsequence: a cold decode from
// (i*S, 0, 0), then exit[i] = f_i(exit[i-1]) iterated to its fixed point (exit[-1] is the true
// entry of the chunk, so the fixed point is the sequential decode), an exclusive scan of the
// blocks-completed counts, and a write pass from the true entry states (after Weissenberger &
// Schmidt, "Massively Parallel Huffman Decoding on GPUs", ICPP 2018).
//
// Decoder state at a bit position: p = bit position in the unstuffed scan, b = block index
// inside the MCU (selects the component, hence the tables), k = zigzag index (0 = a DC category
// comes next). The host decoder of jpeg.cpp is the specification, quirks included: a ZRL that
// passes index 63 ends the block without an error, a run that passes it is an error.
#pragma once
#include "runtime/jpeg.h"

namespace kdl {

// S and T as measured in profiles/jpeg_entropy_gpu.txt; a tuning build may override them
#ifndef KDL_JPEG_HUFF_SUB_BITS
#define KDL_JPEG_HUFF_SUB_BITS 512
#endif
#ifndef KDL_JPEG_HUFF_CHUNK
#define KDL_JPEG_HUFF_CHUNK 512
#endif
constexpr int kJpegHuffSubBits = KDL_JPEG_HUFF_SUB_BITS;   // S: bits per subsequence
constexpr int kJpegHuffChunk = KDL_JPEG_HUFF_CHUNK;        // T: subsequences per chunk = threads per workgroup
static_assert(kJpegHuffSubBits >= 32 && kJpegHuffSubBits % 32 == 0, "a symbol is at most 16 + 15 bits; whole words");
static_assert(kJpegHuffChunk >= 64 && kJpegHuffChunk <= 1024 && (kJpegHuffChunk & (kJpegHuffChunk - 1)) == 0,
              "whole waves, and the block scan doubles its stride up to T");
constexpr int kJpegHuffSubWords = kJpegHuffSubBits / 32;
constexpr int kJpegHuffMargin = 4;       // words staged past a chunk: a symbol that starts in it ends there
// a chunk in LDS: one pad word per subsequence, so that the lanes of a wave, each at the same
// depth of its own subsequence, read distinct banks
constexpr int kJpegHuffChunkWords = kJpegHuffChunk * kJpegHuffSubWords;
constexpr int kJpegHuffStaged = kJpegHuffChunkWords + kJpegHuffMargin;      // words of one staged chunk
KDL_JPEG_HD uint32_t jpeg_huff_lds_index(uint32_t r) { return r + r / (uint32_t)kJpegHuffSubWords; }
constexpr int kJpegHuffLdsWords = kJpegHuffStaged + kJpegHuffStaged / kJpegHuffSubWords + 1;

// One Huffman table as the device reads it: 32-bit words, no byte order assumed.
//   [0, 256)    first level: 512 uint16 (length << 8 | symbol) of the 9-bit prefixes, 0 = longer
//   [256, 273)  maxcode[0..16]   [273, 290)  valoff[0..16]   [290]  number of symbols
//   [291, 355)  the symbols, four per word
constexpr int kJpegHuffFastBits = 9;
constexpr int kJpegHuffTabWords = 356;
constexpr int kJpegHuffTabBytes = kJpegHuffTabWords * 4;
constexpr int kHtMax = 256, kHtOff = 273, kHtN = 290, kHtVals = 291;

// What jpeg_scan_prepare found besides the header. The prepared buffer is
// [2 * ncomp tables (DC, AC per scan component) | the unstuffed scan as big-endian 32-bit words],
// and for a file with restart intervals [... | interval table | group table] behind it.
struct JpegHuffInfo {
  uint32_t nbits = 0;        // bits of entropy-coded data after unstuffing
  uint32_t scan_bytes = 0;   // staged scan: whole words, zero padded
  uint32_t scan_off = 0;     // bytes from the start of the prepared buffer (= 2 * ncomp tables)
  uint32_t nblocks = 0;      // blocks of all MCUs
  uint32_t nbytes = 0;       // bytes of the prepared buffer in use
  int32_t nb = 0;            // blocks per MCU: 1, 3, 4 or 6
  uint8_t comp[8] = {};      // component of each block of the MCU
  bool device_ok = false;    // false: restart intervals (jpeg_huff_decode does not take them)
  // A file with restart intervals (DRI): the scan words hold the intervals one after another, each
  // from a word boundary and followed by one zero word; behind the scan sit the interval table
  // (nint x {first scan word, bits}) and the group table (ngroup x {first interval, count}).
  bool restart_ok = false;   // the markers are RST0, RST1, ... in order and in number: jpeg_huff_rst_decode may run
  uint32_t ri = 0;           // MCUs per interval
  uint32_t nint = 0, ngroup = 0;
  uint32_t int_off = 0, grp_off = 0;   // bytes from the start of the prepared buffer
};

// One image of a GPU entropy-decode call (device memory; built and validated on the host).
struct JpegHuffDesc {
  uint64_t coef_off[3];      // int16 units from the call's coefficient base (JpegDesc's)
  uint64_t scan_off;         // bytes from the call's staging base: the scan words
  uint32_t tab_off[6];       // bytes from the staging base: DC, AC table of component 0, 1, 2
  uint32_t scan_bytes, nbits, nblocks;
  int32_t bw[3], bh[3], h[3], v[3];
  int32_t ncomp, nb, mx, my;
  uint8_t comp[8], bu[8], bv[8];   // per block of the MCU: component, column and row inside the MCU
  // restart intervals (all zero for a file without): MCUs per interval, the interval table
  // (nint x JpegHuffInterval) and the group table (ngroup x JpegHuffGroup), bytes from the staging base
  uint32_t ri, nint, ngroup, int_off, grp_off;
};
struct JpegHuffInterval {
  uint32_t word;             // its first scan word
  uint32_t bits;             // its length after unstuffing; one zero word follows its last word
};
// The intervals that one workgroup of jpeg_huff_rst_decode takes: consecutive ones whose
// subsequences ceil(bits / S) sum to at most T and whose words fit one staged chunk, or a single
// interval of any length, which the workgroup walks in chunks.
struct JpegHuffGroup {
  uint32_t first, count;
};
KDL_JPEG_HD uint32_t jpeg_huff_nsub(uint32_t bits) {
  return bits / (uint32_t)kJpegHuffSubBits + (bits % (uint32_t)kJpegHuffSubBits ? 1u : 0u);
}
KDL_JPEG_HD uint32_t jpeg_huff_interval_words(uint32_t bits) { return bits / 32u + (bits % 32u ? 1u : 0u) + 1u; }
// the rule of a group of more than one interval, over its running sums
KDL_JPEG_HD bool jpeg_huff_group_fits(uint64_t nsub, uint64_t words) {
  return nsub <= (uint64_t)kJpegHuffChunk && words <= (uint64_t)kJpegHuffChunkWords;
}
static_assert(sizeof(JpegHuffDesc) % 8 == 0, "JpegHuffDesc is copied as raw bytes");

// upper bound of the prepared buffer of an n-byte file; ``nint``: the restart intervals its header
// announces (0 without DRI). An interval adds its padding and its table entries, and the file holds
// at most one marker per two bytes, so a header cannot claim more than the file's size allows.
inline uint64_t jpeg_prepare_bound(uint64_t n, uint64_t nint = 0) {
  const uint64_t most = n / 2 + 1;
  return 6ull * kJpegHuffTabBytes + n + 16 + 24ull * (nint < most ? nint : most);
}

// Same marker walk, checks and statuses as jpeg_parse up to the scan; nothing is decoded.
// Writes the tables and the unstuffed scan into ``out`` (capacity ``cap`` bytes, 4-byte aligned).
JpegStatus jpeg_scan_prepare(const uint8_t* data, size_t n, uint64_t max_pixels, uint8_t* out, uint64_t cap,
                             JpegHeader* h, JpegHuffInfo* info);
// ``stage_base``: where the prepared buffer sits in the call's staging, in bytes
void jpeg_huff_fill_desc(const JpegHeader& h, const JpegHuffInfo& info, uint64_t stage_base, uint64_t coef_base,
                         JpegHuffDesc* d);
KDL_JPEG_HD bool jpeg_huff_desc_is_rst(const JpegHuffDesc& d) {
  return (d.ri | d.nint | d.ngroup | d.int_off | d.grp_off) != 0;
}
// every offset the kernels will follow against the capacities of the call (stage_cap bytes, coef_cap
// int16). A descriptor with restart intervals has tables in the staging: ``h_stage`` is the host's
// copy of it, and without one such a descriptor is refused.
inline bool jpeg_huff_desc_valid(const JpegHuffDesc& d, uint64_t stage_cap, uint64_t coef_cap,
                                 const uint8_t* h_stage = nullptr) {
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  if (d.mx < 1 || d.my < 1 || d.mx > 8192 || d.my > 8192) return false;
  int nb = 0;
  for (int c = 0; c < d.ncomp; ++c) {
    const int h = d.h[c], v = d.v[c];
    if (c == 0 ? !((h == 1 && v == 1) || (d.ncomp == 3 && h == 2 && (v == 1 || v == 2))) : (h != 1 || v != 1)) return false;
    if (d.bw[c] != d.mx * h || d.bh[c] != d.my * v || d.bw[c] > 8192 || d.bh[c] > 8192) return false;
    for (int y = 0; y < v; ++y)
      for (int x = 0; x < h; ++x, ++nb)
        if (d.comp[nb] != c || d.bu[nb] != x || d.bv[nb] != y) return false;
    const uint64_t nc = (uint64_t)d.bw[c] * d.bh[c] * 64;
    if (d.coef_off[c] % 8 || d.coef_off[c] > coef_cap || nc > coef_cap - d.coef_off[c]) return false;
  }
  if (d.nb != nb || (uint64_t)d.nblocks != (uint64_t)d.mx * d.my * nb) return false;
  if (d.scan_off % 4 || d.scan_bytes % 4 || d.scan_bytes < 4) return false;
  if (d.scan_off > stage_cap || d.scan_bytes > stage_cap - d.scan_off) return false;
  if (d.nbits >= (1u << 30) || (uint64_t)d.nbits > 8ull * d.scan_bytes) return false;
  for (int t = 0; t < 6; ++t)
    if (d.tab_off[t] % 4 || d.tab_off[t] > stage_cap || (uint64_t)kJpegHuffTabBytes > stage_cap - d.tab_off[t])
      return false;
  if (!jpeg_huff_desc_is_rst(d)) return true;
  if (!h_stage || reinterpret_cast<uintptr_t>(h_stage) % 4) return false;
  const uint64_t mcus = (uint64_t)d.mx * d.my;
  if (d.ri < 1 || (uint64_t)d.nint != (mcus + d.ri - 1) / d.ri || d.ngroup < 1 || d.ngroup > d.nint) return false;
  if (d.int_off % 4 || d.int_off > stage_cap || 8ull * d.nint > stage_cap - d.int_off) return false;
  if (d.grp_off % 4 || d.grp_off > stage_cap || 8ull * d.ngroup > stage_cap - d.grp_off) return false;
  const JpegHuffInterval* iv = reinterpret_cast<const JpegHuffInterval*>(h_stage + d.int_off);
  const JpegHuffGroup* gr = reinterpret_cast<const JpegHuffGroup*>(h_stage + d.grp_off);
  uint64_t next = 0;                           // the intervals follow each other inside the image's scan words
  for (uint32_t j = 0; j < d.nint; ++j) {
    if (iv[j].bits < 1 || iv[j].bits >= (1u << 30) || iv[j].word < next) return false;
    next = (uint64_t)iv[j].word + jpeg_huff_interval_words(iv[j].bits);
    if (next > d.scan_bytes / 4) return false;
  }
  next = 0;                                    // the groups tile the interval table
  for (uint32_t g = 0; g < d.ngroup; ++g) {
    if (gr[g].first != next || gr[g].count < 1 || gr[g].count > d.nint - gr[g].first) return false;
    next += gr[g].count;
    if (gr[g].count == 1) continue;
    uint64_t nsub = 0;
    for (uint32_t j = gr[g].first; j < next; ++j) nsub += jpeg_huff_nsub(iv[j].bits);
    const JpegHuffInterval& z = iv[next - 1];
    if (!jpeg_huff_group_fits(nsub, (uint64_t)z.word + jpeg_huff_interval_words(z.bits) - iv[gr[g].first].word))
      return false;
  }
  return next == d.nint;
}
// The kernels' procedure on the host, serially over the "threads": clears the planes, decodes
// ``stage`` (the call's staging, stage_cap bytes) into coef (coef_cap int16) and sums the DC.
// A descriptor with restart intervals takes the procedure of jpeg_huff_rst_decode and
// jpeg_dc_rst_scan: group after group, the same lanes, rounds, per-interval scans and checks.
// err: the error word (non-zero = ask jpeg_parse); rounds: most fixed-point rounds of a chunk;
// returns the number of indices that fell outside their buffer behind the checks (must be 0).
uint64_t jpeg_huff_cpu(const JpegHuffDesc& d, const uint8_t* stage, uint64_t stage_cap, int16_t* coef,
                       uint64_t coef_cap, uint32_t* err, uint32_t* rounds);

// ---------------------------------------------------------------------------------------------
// Shared decode code. ``Mem`` gives the three accesses, each bounds-checked by its owner:
//   uint32_t word(uint32_t w)            scan word w (big-endian bits), 0 past the staged words
//   const uint32_t* table(int t)         table t = 2 * component + (AC ? 1 : 0)
//   void store(uint64_t off, int16_t v)  coefficient at off (int16 units from the call's base)
//   uint32_t zz(uint32_t k)              natural-order position of zigzag index k < 64

// one symbol from the 16 bits ``pk``: its value, and its code length in *len; -1 = no code.
// A table with a zero or over-long length reads as "no code": every caller then moves one bit.
KDL_JPEG_HD int jpeg_huff_lookup(const uint32_t* t, uint32_t pk, int* len) {
  const uint32_t i = pk >> (16 - kJpegHuffFastBits);
  const uint32_t f = (t[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
  if (f) {
    *len = (int)(f >> 8);
    return (*len >= 1 && *len <= 16) ? (int)(f & 255u) : -1;
  }
  const int32_t nvals = (int32_t)t[kHtN];
  for (int l = kJpegHuffFastBits + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(pk >> (16 - l));
    if (code <= (int32_t)t[kHtMax + l]) {
      const int32_t idx = (int32_t)t[kHtOff + l] + code;
      if (idx < 0 || idx >= nvals || idx >= 256) return -1;
      *len = l;
      return (int)((t[kHtVals + (idx >> 2)] >> (8 * (idx & 3))) & 255u);
    }
  }
  return -1;
}

KDL_JPEG_HD int32_t jpeg_huff_extend(uint32_t v, int s) {
  return v < (1u << (s - 1)) ? (int32_t)v - (int32_t)(1u << s) + 1 : (int32_t)v;
}


// coefficient offset of block g (scan order) of the image, ~0 when there is no such block
KDL_JPEG_HD uint64_t jpeg_huff_block_off(const JpegHuffDesc& d, uint32_t g) {
  if (g >= d.nblocks) return ~0ull;
  const uint32_t mcu = g / (uint32_t)d.nb, j = g - mcu * (uint32_t)d.nb;
  const uint32_t y = mcu / (uint32_t)d.mx, x = mcu - y * (uint32_t)d.mx;
  const int c = d.comp[j];
  const uint64_t blk = (uint64_t)(y * (uint32_t)d.v[c] + d.bv[j]) * (uint64_t)d.bw[c] + (x * (uint32_t)d.h[c] + d.bu[j]);
  return d.coef_off[c] + blk * 64;
}

struct JpegHuffState {
  uint32_t p;    // bit position
  uint32_t bk;   // b << 8 | k
};
KDL_JPEG_HD bool operator==(const JpegHuffState& a, const JpegHuffState& b) { return a.p == b.p && a.bk == b.bk; }

// f_i: decode from ``st`` while p < end; returns the blocks completed. With kWrite the states are
// the true ones: g is the scan-order index of the block st stands in, coefficients (the DC as its
// difference) go to their planes, the pass stops behind the image's last block, and *err is set
// for what the host decoder rejects. Without it the pass runs on states that may be wrong: on a
// bit string that is no code it moves one bit and carries on, and reports nothing.
// Every iteration consumes at least one bit, so the loop ends after at most end - p of them.
// ``g_end`` / ``p_end``: the write pass stops behind block g_end - 1, which must not have used bits
// past p_end: the image's blocks and bits, or those of one restart interval.
template <bool kWrite, class Mem>
KDL_JPEG_HD uint32_t jpeg_huff_run_to(const JpegHuffDesc& d, Mem& m, JpegHuffState* st, uint32_t end, uint32_t g,
                                      uint32_t g_end, uint32_t p_end, uint32_t* err) {
  uint32_t p = st->p, b = st->bk >> 8, k = st->bk & 255u, done = 0;
  if (b >= (uint32_t)d.nb) b = 0;
  if (k > 63) k = 0;
  uint64_t off = kWrite ? jpeg_huff_block_off(d, g) : 0;
  // the two scan words around p stay in registers: one read per 32 bits, not two per symbol
  uint32_t wi = p >> 5, hi = m.word(wi), lo = m.word(wi + 1);
  const uint32_t* tdc = m.table(2 * d.comp[b]);       // the tables of the block's component
  const uint32_t* tac = m.table(2 * d.comp[b] + 1);
  while (p < end) {
    if (kWrite && g >= g_end) break;                  // bits after the last MCU are ignored
    if ((p >> 5) != wi) {                             // a step is at most 31 bits: the next word
      hi = (p >> 5) == wi + 1 ? lo : m.word(p >> 5);
      wi = p >> 5;
      lo = m.word(wi + 1);
    }
    const uint32_t win = (uint32_t)(((((uint64_t)hi << 32) | lo) << (p & 31u)) >> 32);   // 32 bits from p
    int len = 1;
    const int sym = jpeg_huff_lookup(k ? tac : tdc, win >> 16, &len);
    bool fin = false;
    if (sym < 0) {                                    // no code
      p += 1;
      if (kWrite) *err = 1;
      continue;
    }
    if (k == 0) {
      if (sym > 11) {                                 // DC category out of range
        p += (uint32_t)len;
        if (kWrite) *err = 1;
        continue;
      }
      if (kWrite && sym) m.store(off, (int16_t)jpeg_huff_extend((win << len) >> (32 - sym), sym));
      p += (uint32_t)(len + sym);
      k = 1;
    } else {
      const uint32_t r = (uint32_t)sym >> 4, sz = (uint32_t)sym & 15u;
      if (sz == 0) {
        p += (uint32_t)len;
        if (r == 15) {
          k += 16;
          fin = k > 63;                               // the host's loop simply ends
        } else {
          fin = true;                                 // end of block
        }
      } else {
        k += r;
        if (k > 63) {                                 // coefficient index past 63
          p += (uint32_t)len;
          if (kWrite) *err = 1;
          fin = true;
        } else {
          if (kWrite) m.store(off + m.zz(k), (int16_t)jpeg_huff_extend((win << len) >> (32 - sz), (int)sz));
          p += (uint32_t)len + sz;
          fin = ++k > 63;
        }
      }
    }
    if (fin) {
      k = 0;
      b = b + 1 == (uint32_t)d.nb ? 0 : b + 1;
      tdc = m.table(2 * d.comp[b]);
      tac = m.table(2 * d.comp[b] + 1);
      ++done;
      if (kWrite) {
        ++g;
        if (g == g_end && p > p_end) *err = 1;        // the last MCU used bits that are not there
        off = jpeg_huff_block_off(d, g);
      }
    }
  }
  st->p = p;
  st->bk = (b << 8) | k;
  return done;
}
template <bool kWrite, class Mem>
KDL_JPEG_HD uint32_t jpeg_huff_run(const JpegHuffDesc& d, Mem& m, JpegHuffState* st, uint32_t end, uint32_t g,
                                   uint32_t* err) {
  return jpeg_huff_run_to<kWrite>(d, m, st, end, g, d.nblocks, d.nbits, err);
}

// What one thread brings to a chunk. A head enters with a true state and never re-runs; the others
// start cold and take the exit of the thread before them. Threads from a head up to the next one
// form a segment: the whole chunk for jpeg_huff_decode, one restart interval for
// jpeg_huff_rst_decode, whose write pass stays inside the interval's own blocks and bits.
struct JpegHuffLane {
  uint32_t live, head;
  JpegHuffState in0;         // the true entry of a head, the cold start (its first bit, 0, 0) of the others
  uint32_t end;              // the bit behind its subsequence
  uint32_t seg;              // the thread of its segment's head
  uint32_t g0, g_end;        // the segment's first block, and the block behind its last
  uint32_t p_end;            // the bit behind the segment's data
};
// thread i of chunk ch of a walk over ``bits`` bits from bit p0: the scan of a file without restart
// intervals (p0 = 0), or a single interval longer than a chunk. ``entry``: the chunk's true entry.
KDL_JPEG_HD JpegHuffLane jpeg_huff_walk_lane(uint32_t p0, uint32_t bits, uint32_t ch, uint32_t i, JpegHuffState entry,
                                             uint32_t g0, uint32_t g_end) {
  const uint32_t sub = ch * (uint32_t)kJpegHuffChunk + i, nsub = jpeg_huff_nsub(bits);
  const uint64_t stop = ((uint64_t)sub + 1) * (uint32_t)kJpegHuffSubBits;
  JpegHuffLane l;
  l.live = sub < nsub;
  l.head = i == 0;
  l.in0 = i ? JpegHuffState{p0 + sub * (uint32_t)kJpegHuffSubBits, 0} : entry;
  l.end = p0 + (uint32_t)(stop < bits ? stop : bits);
  l.seg = 0;
  l.g0 = g0;
  l.g_end = g_end;
  l.p_end = p0 + bits;
  return l;
}
// [first block, the block behind the last) of the intervals [j, j + count) of a restart descriptor
KDL_JPEG_HD uint32_t jpeg_huff_interval_block(const JpegHuffDesc& d, uint64_t j) {
  const uint64_t g = j * d.ri * (uint32_t)d.nb;
  return (uint32_t)(g < d.nblocks ? g : d.nblocks);
}
// subsequence s of interval j (iv) of a group of several intervals; the thread is i
KDL_JPEG_HD JpegHuffLane jpeg_huff_group_lane(const JpegHuffDesc& d, const JpegHuffInterval& iv, uint32_t j, uint32_t s,
                                              uint32_t i) {
  const uint32_t p0 = iv.word * 32u;
  const uint64_t stop = ((uint64_t)s + 1) * (uint32_t)kJpegHuffSubBits;
  JpegHuffLane l;
  l.live = 1;
  l.head = s == 0;
  l.in0 = JpegHuffState{p0 + s * (uint32_t)kJpegHuffSubBits, 0};
  l.end = p0 + (uint32_t)(stop < iv.bits ? stop : iv.bits);
  l.seg = i - s;
  l.g0 = jpeg_huff_interval_block(d, j);
  l.g_end = jpeg_huff_interval_block(d, (uint64_t)j + 1);
  l.p_end = p0 + iv.bits;
  return l;
}

// DC differences -> DC values of one component: block n of its scan order
KDL_JPEG_HD uint64_t jpeg_huff_dc_off(const JpegHuffDesc& d, int c, uint32_t n) {
  const uint32_t per = (uint32_t)(d.h[c] * d.v[c]);
  const uint32_t mcu = n / per, r = n - mcu * per;
  const uint32_t vv = r / (uint32_t)d.h[c], uu = r - vv * (uint32_t)d.h[c];
  const uint32_t y = mcu / (uint32_t)d.mx, x = mcu - y * (uint32_t)d.mx;
  return d.coef_off[c] + ((uint64_t)(y * (uint32_t)d.v[c] + vv) * (uint64_t)d.bw[c] + (x * (uint32_t)d.h[c] + uu)) * 64;
}

}  // namespace kdl
