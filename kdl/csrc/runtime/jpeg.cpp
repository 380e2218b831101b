// Baseline JPEG: marker walk + Huffman decode on the host, and the CPU pixel path (jpeg.h).
// The input is untrusted: every read is bounded by the buffer and every index by its table.
#include "runtime/jpeg.h"
#include "runtime/jpeg_huff.h"

#include <cstring>
#include <memory>
#include <vector>

namespace kdl {
namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kFast = 9;

struct Huff {
  bool defined = false;
  int nvals = 0;
  uint16_t fast[1 << kFast];   // (length << 8) | symbol for codes of <= kFast bits, 0 = longer
  // AC shortcut: code and magnitude bits both inside the kFast-bit window:
  // (value << 8) | (run << 4) | (code length + magnitude bits), 0 = take the long way
  int16_t fast_ac[1 << kFast];
  int32_t maxcode[17];         // last code of each length (next free code - 1)
  int32_t valoff[17];          // vals index = valoff[len] + code
  uint8_t vals[256];
};

// canonical code from the 16 counts; false when the counts do not form a prefix code
bool build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, Huff* t) {
  std::memset(t->fast, 0, sizeof(t->fast));
  std::memcpy(t->vals, vals, (size_t)nvals);
  t->nvals = nvals;
  int32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    t->valoff[len] = k - code;
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
      if (code >= (1 << len)) return false;
      if (len <= kFast) {
        const int lo = code << (kFast - len);
        for (int j = 0; j < (1 << (kFast - len)); ++j) t->fast[lo + j] = (uint16_t)((len << 8) | vals[k]);
      }
    }
    t->maxcode[len] = code - 1;
    code <<= 1;
  }
  for (int i = 0; i < (1 << kFast); ++i) {
    t->fast_ac[i] = 0;
    const uint16_t f = t->fast[i];
    const int len = f >> 8, run = (f >> 4) & 15, mag = f & 15;
    if (!f || !mag || len + mag > kFast) continue;
    int v = ((i << len) & ((1 << kFast) - 1)) >> (kFast - mag);
    if (v < (1 << (mag - 1))) v += 1 - (1 << mag);
    if (v >= -128 && v <= 127) t->fast_ac[i] = (int16_t)(v * 256 + run * 16 + len + mag);
  }
  t->defined = true;
  return true;
}

// MSB-first bit reader over entropy-coded data: removes FF00 stuffing and fill bytes, stops at a
// marker (or the end of the buffer) and feeds zero bits from there on; a decoder that consumed
// any of those zero bits ran past the data (overrun())
struct Bits {
  const uint8_t* p;
  const uint8_t* end;
  uint64_t buf = 0;
  int cnt = 0;       // valid bits in buf (from the top)
  int npad = 0;      // zero bytes fed since the last reset
  bool stopped = false;

  // afterwards at least 32 bits are valid: one Huffman code (<= 16) and its magnitude bits (<= 15)
  void fill() {
    if (cnt > 32) return;
    if (!stopped && end - p >= 4) {      // four bytes without an FF: no stuffing, no marker
      const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
      const uint32_t x = ~w;
      if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {
        buf |= (uint64_t)w << (32 - cnt);
        cnt += 32;
        p += 4;
        return;
      }
    }
    while (cnt <= 56) {
      uint32_t b = 0;
      if (!stopped) {
        if (p >= end) {
          stopped = true;
        } else if (*p != 0xFF) {
          b = *p++;
        } else if (p + 1 >= end) {
          stopped = true;
        } else if (p[1] == 0x00) {
          b = 0xFF;
          p += 2;
        } else if (p[1] == 0xFF) {   // fill byte
          ++p;
          continue;
        } else {
          stopped = true;            // a marker: p stays on its FF
        }
      }
      if (stopped) ++npad;
      buf |= (uint64_t)b << (56 - cnt);
      cnt += 8;
    }
  }
  uint32_t peek16() const { return (uint32_t)(buf >> 48); }
  void skip(int n) { buf <<= n; cnt -= n; }
  uint32_t get(int n) {               // 1 <= n <= 16
    const uint32_t v = (uint32_t)(buf >> (64 - n));
    skip(n);
    return v;
  }
  bool overrun() const { return cnt < npad * 8; }
  void reset() { buf = 0; cnt = 0; npad = 0; stopped = false; }
};

// one Huffman symbol, or -1 for a bit string that is no code; needs >= 16 bits in the buffer
inline int decode(Bits& b, const Huff& t) {
  const uint32_t pk = b.peek16();
  const uint16_t f = t.fast[pk >> (16 - kFast)];
  if (f) {
    b.skip(f >> 8);
    return f & 255;
  }
  for (int len = kFast + 1; len <= 16; ++len) {
    const int32_t code = (int32_t)(pk >> (16 - len));
    if (code <= t.maxcode[len]) {
      const int32_t idx = t.valoff[len] + code;
      if (idx < 0 || idx >= t.nvals) return -1;
      b.skip(len);
      return t.vals[idx];
    }
  }
  return -1;
}

inline int extend(uint32_t v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

JpegStatus fail(JpegHeader* h, JpegStatus st, const char* why) {
  h->why = why;
  return st;
}

struct Parser {
  const uint8_t* data;
  size_t n;
  uint64_t max_pixels;
  JpegHeader* h;
  Huff dc[4], ac[4];
  bool have_qt[4] = {false, false, false, false};
  bool have_sof = false, jfif = false, adobe = false;
  int adobe_transform = 0;
  // jpeg_scan_prepare: stage the scan for the device decode instead of decoding it
  uint8_t* prep = nullptr;
  uint64_t prep_cap = 0;
  JpegHuffInfo* info = nullptr;

  JpegStatus sof0(const uint8_t* s, size_t sl) {
    if (have_sof) return fail(h, JPEG_MALFORMED, "two frame headers");
    if (sl < 6) return fail(h, JPEG_MALFORMED, "short SOF0");
    const int prec = s[0], nc = s[5];
    if (prec != 8) return fail(h, JPEG_UNSUPPORTED, "sample precision is not 8 bits");
    if (nc != 1 && nc != 3) return fail(h, JPEG_UNSUPPORTED, "not 1 or 3 components");
    if (sl != (size_t)(6 + 3 * nc)) return fail(h, JPEG_MALFORMED, "SOF0 length does not match its components");
    h->H = (int)be16(s + 1);
    h->W = (int)be16(s + 3);
    if (h->W == 0 || h->H == 0) return fail(h, JPEG_MALFORMED, "zero image dimension");
    if ((uint64_t)h->W * (uint64_t)h->H > max_pixels) return fail(h, JPEG_MALFORMED, "image exceeds the pixel limit");
    h->ncomp = nc;
    for (int c = 0; c < nc; ++c) {
      JpegComp& k = h->comp[c];
      k.id = s[6 + 3 * c];
      k.h = s[7 + 3 * c] >> 4;
      k.v = s[7 + 3 * c] & 15;
      k.tq = s[8 + 3 * c];
      if (k.h < 1 || k.h > 4 || k.v < 1 || k.v > 4) return fail(h, JPEG_MALFORMED, "sampling factor out of range");
      if (k.tq > 3) return fail(h, JPEG_MALFORMED, "quantisation table id out of range");
    }
    if (nc == 1) {      // a single-component scan is never interleaved: its factors mean nothing
      h->comp[0].h = h->comp[0].v = 1;
    } else {
      const JpegComp& y = h->comp[0];
      const bool luma = (y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2);
      if (!luma || h->comp[1].h != 1 || h->comp[1].v != 1 || h->comp[2].h != 1 || h->comp[2].v != 1)
        return fail(h, JPEG_UNSUPPORTED, "sampling other than 4:4:4, 4:2:2, 4:2:0");
    }
    h->hmax = h->comp[0].h;
    h->vmax = h->comp[0].v;
    const int mx = (h->W + 8 * h->hmax - 1) / (8 * h->hmax), my = (h->H + 8 * h->vmax - 1) / (8 * h->vmax);
    uint64_t off = 0;
    for (int c = 0; c < nc; ++c) {
      JpegComp& k = h->comp[c];
      k.bw = mx * k.h;
      k.bh = my * k.v;
      k.dw = (h->W * k.h + h->hmax - 1) / h->hmax;
      k.dh = (h->H * k.v + h->vmax - 1) / h->vmax;
      k.coef_off = off;
      off += (uint64_t)k.bw * (uint64_t)k.bh * 64;
    }
    h->ncoef = off;
    have_sof = true;
    return JPEG_OK;
  }

  JpegStatus dqt(const uint8_t* s, size_t sl) {
    size_t i = 0;
    while (i < sl) {
      const int pq = s[i] >> 4, tq = s[i] & 15;
      if (tq > 3) return fail(h, JPEG_MALFORMED, "quantisation table id out of range");
      if (pq == 1) return fail(h, JPEG_UNSUPPORTED, "16-bit quantisation table");
      if (pq != 0) return fail(h, JPEG_MALFORMED, "bad quantisation table precision");
      if (sl - i < 65) return fail(h, JPEG_MALFORMED, "short DQT");
      for (int k = 0; k < 64; ++k) h->qt[tq][kZigzag[k]] = s[i + 1 + k];
      have_qt[tq] = true;
      i += 65;
    }
    return JPEG_OK;
  }

  JpegStatus dht(const uint8_t* s, size_t sl) {
    size_t i = 0;
    while (i < sl) {
      const int tc = s[i] >> 4, th = s[i] & 15;
      if (tc > 1 || th > 3) return fail(h, JPEG_MALFORMED, "Huffman table id out of range");
      if (sl - i < 17) return fail(h, JPEG_MALFORMED, "short DHT");
      int total = 0;
      for (int k = 0; k < 16; ++k) total += s[i + 1 + k];
      if (total > 256 || sl - i - 17 < (size_t)total) return fail(h, JPEG_MALFORMED, "DHT symbols past its segment");
      if (!build_huff(s + i + 1, s + i + 17, total, tc ? &ac[th] : &dc[th]))
        return fail(h, JPEG_MALFORMED, "DHT counts are not a prefix code");
      i += 17 + (size_t)total;
    }
    return JPEG_OK;
  }

  JpegStatus scan(const uint8_t* s, size_t sl, size_t pos, int16_t* coef, uint64_t cap) {
    if (!have_sof) return fail(h, JPEG_MALFORMED, "scan before the frame header");
    if (sl < 1) return fail(h, JPEG_MALFORMED, "short SOS");
    const int ns = s[0];
    if (ns < 1 || ns > 4 || sl != (size_t)(4 + 2 * ns)) return fail(h, JPEG_MALFORMED, "SOS length does not match");
    if (ns != h->ncomp) return fail(h, JPEG_UNSUPPORTED, "more than one scan");
    const Huff* tdc[3];
    const Huff* tac[3];
    for (int c = 0; c < ns; ++c) {
      if (s[1 + 2 * c] != h->comp[c].id) return fail(h, JPEG_UNSUPPORTED, "scan components not in frame order");
      const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
      if (td > 3 || ta > 3) return fail(h, JPEG_MALFORMED, "Huffman table id out of range");
      if (!dc[td].defined || !ac[ta].defined) return fail(h, JPEG_MALFORMED, "scan uses a missing Huffman table");
      if (!have_qt[h->comp[c].tq]) return fail(h, JPEG_MALFORMED, "component uses a missing quantisation table");
      tdc[c] = &dc[td];
      tac[c] = &ac[ta];
    }
    if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
      return fail(h, JPEG_UNSUPPORTED, "spectral selection / approximation in a sequential scan");
    if (ns == 3) {   // colour rule: YCbCr with JFIF, with Adobe transform 1, or with ids 1,2,3
      if (adobe && adobe_transform != 1) return fail(h, JPEG_UNSUPPORTED, "Adobe colour transform is not YCbCr");
      const bool ids = h->comp[0].id == 1 && h->comp[1].id == 2 && h->comp[2].id == 3;
      if (!jfif && !adobe && !ids) return fail(h, JPEG_UNSUPPORTED, "colour space is not known to be YCbCr");
    }
    if (info) return prepare(tdc, tac, ns, pos);
    if (cap < h->ncoef || coef == nullptr) return fail(h, JPEG_MALFORMED, "coefficient buffer too small");

    Bits b{data + pos, data + n};
    const int mx = h->comp[0].bw / h->comp[0].h, my = h->comp[0].bh / h->comp[0].v;
    int pred[3] = {0, 0, 0};
    int left = h->restart, next_rst = 0;
    for (int y = 0; y < my; ++y) {
      for (int x = 0; x < mx; ++x) {
        if (h->restart && left == 0) {
          // the interval's data ends at a marker: drop the padding bits, expect RSTn
          if (!b.stopped) b.fill();
          const uint8_t* q = b.p;
          if (!b.stopped) {          // unread entropy bytes in front of the marker: skip to it
            while (q + 1 < b.end && !(q[0] == 0xFF && q[1] != 0x00 && q[1] != 0xFF)) ++q;
          }
          while (q + 1 < b.end && q[0] == 0xFF && q[1] == 0xFF) ++q;
          if (q + 1 >= b.end || q[0] != 0xFF || q[1] != 0xD0 + next_rst)
            return fail(h, JPEG_MALFORMED, "restart marker missing");
          b.p = q + 2;
          b.reset();
          next_rst = (next_rst + 1) & 7;
          left = h->restart;
          pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < ns; ++c) {
          const JpegComp& k = h->comp[c];
          for (int v = 0; v < k.v; ++v) {
            for (int u = 0; u < k.h; ++u) {
              const uint64_t blk = (uint64_t)(y * k.v + v) * (uint64_t)k.bw + (uint64_t)(x * k.h + u);
              int16_t* out = coef + k.coef_off + blk * 64;
              std::memset(out, 0, 128);
              b.fill();
              int s_ = decode(b, *tdc[c]);
              if (s_ < 0) return fail(h, JPEG_MALFORMED, "bad Huffman code");
              if (s_ > 11) return fail(h, JPEG_MALFORMED, "DC category out of range");
              if (s_) {
                b.fill();
                pred[c] = (int16_t)(pred[c] + extend(b.get(s_), s_));
              }
              out[0] = (int16_t)pred[c];
              for (int i = 1; i < 64;) {
                b.fill();
                const int16_t fa = tac[c]->fast_ac[b.buf >> (64 - kFast)];
                if (fa) {
                  i += (fa >> 4) & 15;
                  if (i > 63) return fail(h, JPEG_MALFORMED, "coefficient index past 63");
                  out[kZigzag[i++]] = (int16_t)(fa >> 8);
                  b.skip(fa & 15);
                  continue;
                }
                const int rs = decode(b, *tac[c]);
                if (rs < 0) return fail(h, JPEG_MALFORMED, "bad Huffman code");
                const int r = rs >> 4, sz = rs & 15;
                if (sz == 0) {
                  if (r != 15) break;     // end of block
                  i += 16;
                  continue;
                }
                i += r;
                if (i > 63) return fail(h, JPEG_MALFORMED, "coefficient index past 63");
                out[kZigzag[i]] = (int16_t)extend(b.get(sz), sz);
                ++i;
              }
              if (b.overrun()) return fail(h, JPEG_MALFORMED, "entropy-coded data is truncated");
            }
          }
        }
        if (h->restart) --left;
      }
    }
    return JPEG_OK;
  }

  // one table in the device's form (jpeg_huff.h)
  static void pack_table(const Huff& t, uint32_t* w) {
    std::memset(w, 0, kJpegHuffTabBytes);
    for (int i = 0; i < (1 << kFast); ++i) w[i >> 1] |= (uint32_t)t.fast[i] << (16 * (i & 1));
    for (int l = 1; l <= 16; ++l) {
      w[kHtMax + l] = (uint32_t)t.maxcode[l];
      w[kHtOff + l] = (uint32_t)t.valoff[l];
    }
    w[kHtMax] = (uint32_t)-1;
    w[kHtN] = (uint32_t)t.nvals;
    for (int i = 0; i < t.nvals; ++i) w[kHtVals + (i >> 2)] |= (uint32_t)t.vals[i] << (8 * (i & 3));
  }

  // tables + the scan with its byte stuffing removed, exactly the bytes that Bits would feed:
  // FF 00 -> FF, fill bytes dropped, the end at the first marker (or a lone FF at the end)
  JpegStatus prepare(const Huff* const* tdc, const Huff* const* tac, int ns, size_t pos) {
    static_assert(kFast == kJpegHuffFastBits, "the device tables mirror the host's first level");
    const uint64_t tabs = (uint64_t)2 * ns * kJpegHuffTabBytes;
    if (reinterpret_cast<uintptr_t>(prep) % 4 || prep_cap < tabs + 8)
      return fail(h, JPEG_MALFORMED, "prepare buffer too small");
    uint32_t* w = reinterpret_cast<uint32_t*>(prep);
    for (int c = 0; c < ns; ++c) {
      pack_table(*tdc[c], w + (2 * c) * kJpegHuffTabWords);
      pack_table(*tac[c], w + (2 * c + 1) * kJpegHuffTabWords);
    }
    uint32_t* sw = w + 2 * ns * kJpegHuffTabWords;
    const uint64_t room = (prep_cap - tabs) / 4;       // words
    const int mx = h->comp[0].bw / h->comp[0].h, my = h->comp[0].bh / h->comp[0].v;
    info->nb = 0;
    for (int c = 0; c < ns; ++c)
      for (int i = 0; i < h->comp[c].h * h->comp[c].v; ++i) info->comp[info->nb++] = (uint8_t)c;
    info->nblocks = (uint32_t)((uint64_t)mx * my * info->nb);
    info->scan_off = (uint32_t)tabs;
    if (h->restart > 0) return prepare_restart(sw, room, tabs, pos, (uint64_t)mx * my);
    uint64_t nbytes = 0;
    uint32_t acc = 0;
    const uint8_t* p = data + pos;
    const uint8_t* end = data + n;
    while (p < end) {
      uint32_t b = *p;
      if (b != 0xFF) {
        ++p;
      } else if (p + 1 >= end) {
        break;
      } else if (p[1] == 0x00) {
        p += 2;
      } else if (p[1] == 0xFF) {
        ++p;
        continue;
      } else {
        break;
      }
      acc = (acc << 8) | b;
      if ((++nbytes & 3) == 0) {
        if (nbytes / 4 > room) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
        sw[nbytes / 4 - 1] = acc;
        acc = 0;
      }
    }
    uint64_t nwords = nbytes / 4;
    if (nwords + 2 > room) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
    if (nbytes & 3) sw[nwords++] = acc << (8 * (4 - (nbytes & 3)));
    sw[nwords++] = 0;                                    // the zero bits behind the data
    info->nbits = (uint32_t)(nbytes * 8);
    info->scan_bytes = (uint32_t)(nwords * 4);
    info->nbytes = (uint32_t)(tabs + nwords * 4);
    info->device_ok = nbytes < (1u << 27);
    return JPEG_OK;
  }

  // The scan of a file with restart intervals: the same unstuffing, carried on through the RSTm
  // markers. Every interval starts on a word boundary (the padding bits in front of a marker are
  // dropped, as the host decoder drops them) and is followed by one zero word; behind the scan come
  // the interval table and the groups of the kernel (jpeg_huff.h). Markers that are not exactly
  // RST0, RST1, ... in order and in number, or an empty interval, leave restart_ok false: what such
  // a file means is for the host decoder to say.
  JpegStatus prepare_restart(uint32_t* sw, uint64_t room, uint64_t tabs, size_t pos, uint64_t mcus) {
    const uint64_t ri = (uint64_t)h->restart, expect = (mcus + ri - 1) / ri;
    std::vector<JpegHuffInterval> iv;
    uint64_t nwords = 0, nbytes = 0, total = 0, first = 0, nmark = 0;
    uint32_t acc = 0;
    bool ok = true;
    auto close = [&]() {                                 // false: out of room
      if (nwords + 2 > room) return false;
      if (nbytes & 3) sw[nwords++] = acc << (8 * (4 - (nbytes & 3)));
      sw[nwords++] = 0;                                  // the zero bits behind the interval
      if (nbytes == 0) ok = false;
      iv.push_back(JpegHuffInterval{(uint32_t)first, (uint32_t)(nbytes * 8)});
      total += nbytes;
      first = nwords;
      nbytes = 0;
      acc = 0;
      return true;
    };
    const uint8_t* p = data + pos;
    const uint8_t* end = data + n;
    while (p < end && ok) {
      uint32_t b = *p;
      if (b != 0xFF) {
        ++p;
      } else if (p + 1 >= end) {
        break;
      } else if (p[1] == 0x00) {
        p += 2;
      } else if (p[1] == 0xFF) {
        ++p;
        continue;
      } else if (p[1] >= 0xD0 && p[1] <= 0xD7) {
        if (p[1] != 0xD0 + (nmark & 7) || nmark + 1 >= expect) ok = false;     // misnumbered, or one too many
        if (!close()) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
        ++nmark;
        p += 2;
        continue;
      } else {
        break;
      }
      acc = (acc << 8) | b;
      if ((++nbytes & 3) == 0) {
        if (nwords + 1 > room) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
        sw[nwords++] = acc;
        acc = 0;
      }
    }
    if (ok && !close()) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
    info->scan_bytes = (uint32_t)(nwords * 4);
    info->nbytes = (uint32_t)(tabs + nwords * 4);
    info->nbits = (uint32_t)(total * 8);
    info->ri = (uint32_t)ri;
    if (!ok || iv.size() != expect || total >= (1u << 27)) {
      info->nbits = 0;
      return JPEG_OK;
    }
    std::vector<JpegHuffGroup> gr;                       // greedy, by the rule of jpeg_huff_group_fits
    uint64_t nsub = 0;
    for (uint32_t j = 0; j < (uint32_t)iv.size(); ++j) {
      const uint64_t s = jpeg_huff_nsub(iv[j].bits), wend = (uint64_t)iv[j].word + jpeg_huff_interval_words(iv[j].bits);
      if (!gr.empty() && jpeg_huff_group_fits(nsub + s, wend - iv[gr.back().first].word)) {
        ++gr.back().count;
        nsub += s;
      } else {
        gr.push_back(JpegHuffGroup{j, 1});
        nsub = s;
      }
    }
    const uint64_t need = 2 * (uint64_t)iv.size() + 2 * (uint64_t)gr.size();
    if (nwords + need > room) return fail(h, JPEG_MALFORMED, "prepare buffer too small");
    info->int_off = (uint32_t)(tabs + nwords * 4);
    std::memcpy(sw + nwords, iv.data(), iv.size() * sizeof(JpegHuffInterval));
    nwords += 2 * iv.size();
    info->grp_off = (uint32_t)(tabs + nwords * 4);
    std::memcpy(sw + nwords, gr.data(), gr.size() * sizeof(JpegHuffGroup));
    nwords += 2 * gr.size();
    info->nint = (uint32_t)iv.size();
    info->ngroup = (uint32_t)gr.size();
    info->nbytes = (uint32_t)(tabs + nwords * 4);
    info->restart_ok = true;
    return JPEG_OK;
  }

  JpegStatus run(int16_t* coef, uint64_t cap, bool probe) {
    if (n < 2 || data[0] != 0xFF || data[1] != 0xD8) return fail(h, JPEG_UNSUPPORTED, "not a JPEG");
    size_t pos = 2;
    for (;;) {
      if (pos >= n) return fail(h, JPEG_MALFORMED, "file ends before the scan");
      if (data[pos] != 0xFF) return fail(h, JPEG_MALFORMED, "bytes between segments");
      while (pos < n && data[pos] == 0xFF) ++pos;
      if (pos >= n) return fail(h, JPEG_MALFORMED, "file ends before the scan");
      const int m = data[pos++];
      if (m == 0x00 || m == 0xD8 || m == 0xD9) return fail(h, JPEG_MALFORMED, "unexpected marker before the scan");
      if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;   // stand-alone markers
      if (n - pos < 2) return fail(h, JPEG_MALFORMED, "segment length past the end");
      const size_t len = be16(data + pos);
      if (len < 2 || len > n - pos) return fail(h, JPEG_MALFORMED, "segment length past the end");
      const uint8_t* s = data + pos + 2;
      const size_t sl = len - 2;
      pos += len;
      JpegStatus st = JPEG_OK;
      switch (m) {
        case 0xC0:
          st = sof0(s, sl);
          if (st == JPEG_OK && probe) return st;
          break;
        case 0xC1: case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC8: case 0xC9: case 0xCA: case 0xCB:
        case 0xCC: case 0xCD: case 0xCE: case 0xCF:
          return fail(h, JPEG_UNSUPPORTED, "not baseline sequential Huffman (SOF0)");
        case 0xC4:
          if (!probe) st = dht(s, sl);
          break;
        case 0xDB:
          st = dqt(s, sl);
          break;
        case 0xDD:
          if (sl != 2) return fail(h, JPEG_MALFORMED, "bad DRI length");
          h->restart = (int)be16(s);
          break;
        case 0xE0:
          if (sl >= 5 && std::memcmp(s, "JFIF\0", 5) == 0) jfif = true;
          break;
        case 0xEE:
          if (sl >= 12 && std::memcmp(s, "Adobe", 5) == 0) {
            adobe = true;
            adobe_transform = s[11];
          }
          break;
        case 0xDA:
          if (probe) return fail(h, JPEG_MALFORMED, "scan before the frame header");
          return scan(s, sl, pos, coef, cap);
        default:      // APPn, COM and anything else with a length: skipped
          break;
      }
      if (st != JPEG_OK) return st;
    }
  }
};

void idct_block(const int16_t* c, const uint16_t* q, uint8_t* out, size_t stride) {
  uint32_t ws[64], in[8], o[8];
  for (int col = 0; col < 8; ++col) {
    for (int r = 0; r < 8; ++r) in[r] = (uint32_t)(int32_t)c[r * 8 + col] * (uint32_t)q[r * 8 + col];
    jpeg_idct_1d(in, o);
    for (int r = 0; r < 8; ++r) ws[r * 8 + col] = (uint32_t)jpeg_descale(o[r], 11);
  }
  for (int r = 0; r < 8; ++r) {
    jpeg_idct_1d(ws + r * 8, o);
    for (int col = 0; col < 8; ++col) out[r * stride + col] = jpeg_clamp(jpeg_descale(o[col], 18) + 128);
  }
}

}  // namespace

JpegStatus jpeg_probe(const uint8_t* data, size_t n, uint64_t max_pixels, JpegHeader* h) {
  *h = JpegHeader{};
  std::vector<Parser> p(1);       // the Huffman tables are too large for a handler thread's stack
  p[0].data = data; p[0].n = n; p[0].max_pixels = max_pixels; p[0].h = h;
  return p[0].run(nullptr, 0, true);
}

JpegStatus jpeg_parse(const uint8_t* data, size_t n, uint64_t max_pixels, int16_t* coef, uint64_t cap,
                      JpegHeader* h) {
  *h = JpegHeader{};
  std::vector<Parser> p(1);
  p[0].data = data; p[0].n = n; p[0].max_pixels = max_pixels; p[0].h = h;
  return p[0].run(coef, cap, false);
}

JpegStatus jpeg_scan_prepare(const uint8_t* data, size_t n, uint64_t max_pixels, uint8_t* out, uint64_t cap,
                             JpegHeader* h, JpegHuffInfo* info) {
  *h = JpegHeader{};
  *info = JpegHuffInfo{};
  if (n >= (1ull << 31)) return fail(h, JPEG_MALFORMED, "file too large");
  std::vector<Parser> p(1);
  p[0].data = data; p[0].n = n; p[0].max_pixels = max_pixels; p[0].h = h;
  p[0].prep = out; p[0].prep_cap = cap; p[0].info = info;
  return p[0].run(nullptr, 0, false);
}

void jpeg_huff_fill_desc(const JpegHeader& h, const JpegHuffInfo& info, uint64_t stage_base, uint64_t coef_base,
                         JpegHuffDesc* d) {
  std::memset(d, 0, sizeof(*d));
  int j = 0;
  for (int c = 0; c < 3; ++c) {
    const JpegComp& k = h.comp[c < h.ncomp ? c : 0];
    d->coef_off[c] = coef_base + k.coef_off;
    d->bw[c] = k.bw; d->bh[c] = k.bh; d->h[c] = k.h; d->v[c] = k.v;
    d->tab_off[2 * c] = (uint32_t)(stage_base + (uint64_t)(2 * c) * kJpegHuffTabBytes);
    d->tab_off[2 * c + 1] = (uint32_t)(stage_base + (uint64_t)(2 * c + 1) * kJpegHuffTabBytes);
    if (c >= h.ncomp) {
      d->tab_off[2 * c] = d->tab_off[0];
      d->tab_off[2 * c + 1] = d->tab_off[1];
      continue;
    }
    for (int v = 0; v < k.v; ++v)
      for (int u = 0; u < k.h; ++u, ++j) {
        if (j >= 8) continue;
        d->comp[j] = (uint8_t)c; d->bu[j] = (uint8_t)u; d->bv[j] = (uint8_t)v;
      }
  }
  d->scan_off = stage_base + info.scan_off;
  d->scan_bytes = info.scan_bytes; d->nbits = info.nbits; d->nblocks = info.nblocks;
  d->ncomp = h.ncomp; d->nb = info.nb;
  d->mx = h.comp[0].h ? h.comp[0].bw / h.comp[0].h : 0;
  d->my = h.comp[0].v ? h.comp[0].bh / h.comp[0].v : 0;
  if (info.restart_ok) {       // the tables of jpeg_huff_rst_decode; zero for every other file
    d->ri = info.ri; d->nint = info.nint; d->ngroup = info.ngroup;
    d->int_off = (uint32_t)(stage_base + info.int_off);
    d->grp_off = (uint32_t)(stage_base + info.grp_off);
  }
}

namespace {

// the kernels' memory as the emulation sees it: every index is checked a second time behind the
// check of the shared code, and counted when that one let it through
struct EmuMem {
  const uint32_t* lds;        // the staged chunk
  uint32_t w0;                // its first scan word
  const uint32_t* tabs[6];
  int16_t* coef;
  uint64_t coef_cap;
  uint64_t* bad;
  uint32_t word(uint32_t w) const {
    const uint32_t r = w - w0;
    if (r >= (uint32_t)kJpegHuffStaged) return 0;
    const uint32_t i = jpeg_huff_lds_index(r);
    if (i >= (uint32_t)kJpegHuffLdsWords) { ++*bad; return 0; }
    return lds[i];
  }
  const uint32_t* table(int t) const {
    if (t < 0 || t > 5) { ++*bad; return tabs[0]; }
    return tabs[t];
  }
  void store(uint64_t off, int16_t v) const {
    if (off >= coef_cap) { ++*bad; return; }
    coef[off] = v;
  }
  uint32_t zz(uint32_t k) const {
    if (k > 63) { ++*bad; return 0; }
    return kZigzag[k];
  }
};

}  // namespace

namespace {

constexpr int kT = kJpegHuffChunk;

// the state of the emulated workgroup
struct Emu {
  const JpegHuffDesc& d;
  EmuMem m;
  std::vector<uint32_t> lds;
  const uint32_t* words;      // the image's scan
  uint32_t nwords;
  std::vector<JpegHuffLane> lane;
  std::vector<JpegHuffState> ex, in, last;
  std::vector<uint32_t> cnt, incl;
  uint32_t* err;
  uint32_t* rounds;
  uint64_t* bad;

  Emu(const JpegHuffDesc& d_, const uint8_t* stage, int16_t* coef, uint64_t coef_cap, uint32_t* err_, uint32_t* rounds_,
      uint64_t* bad_)
      : d(d_), m{nullptr, 0, {}, coef, coef_cap, bad_}, lds(kJpegHuffLdsWords),
        words(reinterpret_cast<const uint32_t*>(stage + d_.scan_off)), nwords(d_.scan_bytes / 4), lane(kT), ex(kT),
        in(kT), last(kT), cnt(kT), incl(kT), err(err_), rounds(rounds_), bad(bad_) {
    m.lds = lds.data();
    for (int t = 0; t < 6; ++t) m.tabs[t] = reinterpret_cast<const uint32_t*>(stage + d.tab_off[t]);
  }

  // One chunk staged from scan word w0 (words from ``w_end`` on read as zero), lane[] filled in:
  // the cold pass, the rounds (at most ``bound``), the scan of the counts and the write pass.
  // Leaves the exit states in ex[] and the inclusive sums of the blocks completed in incl[].
  void chunk(uint32_t w0, uint32_t w_end, uint32_t bound) {
    m.w0 = w0;
    for (uint32_t r = 0; r < (uint32_t)kJpegHuffStaged; ++r) {
      const uint32_t i = jpeg_huff_lds_index(r);
      if (i >= (uint32_t)kJpegHuffLdsWords) { ++*bad; continue; }
      const uint64_t w = (uint64_t)w0 + r;
      if (w < w_end && w >= nwords) { ++*bad; continue; }
      lds[i] = w < w_end ? words[w] : 0;
    }
    // subsequences that start behind the data are not live: they decode nothing and stay out of
    // the rounds, where they would hand a change on one thread per round
    for (int i = 0; i < kT; ++i) {                                     // steps 1, 2: the cold pass
      cnt[i] = 0;
      last[i] = ex[i] = lane[i].in0;
      if (lane[i].live) cnt[i] = jpeg_huff_run<false>(d, m, &ex[i], lane[i].end, 0, err);
    }
    uint32_t r = 0;
    for (; r < bound; ++r) {                                           // steps 3, 4: to the fixed point
      for (int i = 1; i < kT; ++i) in[i] = ex[i - 1];
      bool any = false;
      for (int i = 1; i < kT; ++i) {
        if (lane[i].head || !lane[i].live || in[i] == last[i]) continue;
        last[i] = in[i];
        JpegHuffState e = in[i];
        cnt[i] = jpeg_huff_run<false>(d, m, &e, lane[i].end, 0, err);
        if (!(e == ex[i])) any = true;
        ex[i] = e;
      }
      if (!any) break;
    }
    if (r + 1 > *rounds) *rounds = r + 1;
    uint32_t sum = 0;                                                  // step 5
    for (int i = 0; i < kT; ++i) incl[i] = sum += cnt[i];
    for (int i = 0; i < kT; ++i) {                                     // step 6: the write pass
      const JpegHuffLane& l = lane[i];
      if (!l.live) continue;
      if (l.seg > (uint32_t)i) { ++*bad; continue; }
      JpegHuffState st = (l.head || i == 0) ? l.in0 : ex[i - 1];
      const uint32_t g = l.g0 + (incl[i] - cnt[i]) - (l.seg ? incl[l.seg - 1] : 0);
      jpeg_huff_run_to<true>(d, m, &st, l.end, g, l.g_end, l.p_end, err);
    }
  }

  // a walk in chunks over ``bits`` bits from scan word ``word``, into the blocks [g0, g_end)
  void walk(uint32_t word, uint32_t bits, uint32_t g0, uint32_t g_end) {
    const uint32_t nsub = jpeg_huff_nsub(bits), nchunk = (nsub + kT - 1) / kT;
    const uint64_t w_lim = (uint64_t)word + jpeg_huff_interval_words(bits);
    const uint32_t w_end = (uint32_t)(w_lim < nwords ? w_lim : nwords);
    JpegHuffState entry{word * 32u, 0};
    uint32_t base = g0;
    for (uint32_t ch = 0; ch < nchunk; ++ch) {
      for (int i = 0; i < kT; ++i) lane[i] = jpeg_huff_walk_lane(word * 32u, bits, ch, (uint32_t)i, entry, base, g_end);
      chunk(word + ch * (uint32_t)kJpegHuffChunkWords, w_end, (uint32_t)kT);
      entry = ex[kT - 1];
      base += incl[kT - 1];
    }
    if (base < g_end) *err = 1;                                        // the data ends before the last MCU
  }

  void clear(uint32_t g0, uint32_t g_end) {                            // step 8, the blocks of [g0, g_end)
    for (uint32_t g = g0; g < g_end; ++g) {
      const uint64_t off = jpeg_huff_block_off(d, g);
      for (int k = 0; k < 64; ++k) {
        if (off + k >= m.coef_cap) { ++*bad; break; }
        m.coef[off + k] = 0;
      }
    }
  }

  void group(const JpegHuffInterval* iv, const JpegHuffGroup& gr) {
    const uint32_t g0 = jpeg_huff_interval_block(d, gr.first);
    clear(g0, jpeg_huff_interval_block(d, (uint64_t)gr.first + gr.count));
    if (gr.count == 1) {
      walk(iv[gr.first].word, iv[gr.first].bits, g0, jpeg_huff_interval_block(d, (uint64_t)gr.first + 1));
      return;
    }
    uint32_t n = 0, most = 0;
    for (uint32_t j = gr.first; j < gr.first + gr.count; ++j) {
      const uint32_t nsub = jpeg_huff_nsub(iv[j].bits);
      most = nsub > most ? nsub : most;
      for (uint32_t s = 0; s < nsub; ++s, ++n) {
        if (n >= (uint32_t)kT) { ++*bad; continue; }
        lane[n] = jpeg_huff_group_lane(d, iv[j], j, s, n);
      }
    }
    for (uint32_t i = n; i < (uint32_t)kT; ++i) lane[i] = JpegHuffLane{};
    const JpegHuffInterval& z = iv[gr.first + gr.count - 1];
    const uint64_t w_lim = (uint64_t)z.word + jpeg_huff_interval_words(z.bits);
    chunk(iv[gr.first].word, (uint32_t)(w_lim < nwords ? w_lim : nwords), most);
    for (uint32_t i = 0; i < n && i < (uint32_t)kT; ++i) {             // an interval that ends before its last block
      if (i + 1 < n && !lane[i + 1].head) continue;
      const uint32_t total = incl[i] - (lane[i].seg ? incl[lane[i].seg - 1] : 0);
      if (total < lane[i].g_end - lane[i].g0) *err = 1;
    }
  }
};

// step 7, the DC sums of one segment of component c: blocks [lo, hi) of its scan order
void emu_dc(const JpegHuffDesc& d, int c, uint32_t lo, uint32_t hi, int16_t* coef, uint64_t coef_cap, uint64_t* bad) {
  uint32_t acc = 0;
  for (uint32_t k = lo; k < hi; ++k) {
    const uint64_t off = jpeg_huff_dc_off(d, c, k);
    if (off >= coef_cap) { ++*bad; continue; }
    acc += (uint16_t)coef[off];
    coef[off] = (int16_t)(uint16_t)acc;
  }
}

}  // namespace

uint64_t jpeg_huff_cpu(const JpegHuffDesc& d, const uint8_t* stage, uint64_t stage_cap, int16_t* coef,
                       uint64_t coef_cap, uint32_t* err, uint32_t* rounds) {
  *err = 1;
  *rounds = 0;
  if (!jpeg_huff_desc_valid(d, stage_cap, coef_cap, stage) || reinterpret_cast<uintptr_t>(stage) % 4) return 0;
  *err = 0;
  uint64_t bad = 0;
  const std::unique_ptr<Emu> emu(new Emu(d, stage, coef, coef_cap, err, rounds, &bad));   // its vectors are the LDS
  Emu& e = *emu;
  if (!jpeg_huff_desc_is_rst(d)) {
    e.clear(0, d.nblocks);
    e.walk(0, d.nbits, 0, d.nblocks);
    // the wrapping sums do not depend on how the kernel splits them over its threads
    for (int c = 0; c < d.ncomp; ++c) emu_dc(d, c, 0, (uint32_t)d.bw[c] * (uint32_t)d.bh[c], coef, coef_cap, &bad);
    return bad;
  }
  const JpegHuffInterval* iv = reinterpret_cast<const JpegHuffInterval*>(stage + d.int_off);
  const JpegHuffGroup* gr = reinterpret_cast<const JpegHuffGroup*>(stage + d.grp_off);
  for (uint32_t g = 0; g < d.ngroup; ++g) e.group(iv, gr[g]);
  for (int c = 0; c < d.ncomp; ++c) {                                  // the predictors start again at every interval
    const uint32_t n = (uint32_t)d.bw[c] * (uint32_t)d.bh[c];
    const uint64_t per = (uint64_t)d.ri * (uint32_t)(d.h[c] * d.v[c]);
    for (uint64_t lo = 0; lo < n; lo += per) emu_dc(d, c, (uint32_t)lo, (uint32_t)(lo + per < n ? lo + per : n), coef, coef_cap, &bad);
  }
  return bad;
}

void jpeg_fill_desc(const JpegHeader& h, uint64_t coef_base, uint64_t plane_base, int32_t qt_base, int32_t* wg,
                    int32_t out_row, uint64_t ytab, uint64_t xtab, JpegDesc* d) {
  std::memset(d, 0, sizeof(*d));
  for (int c = 0; c < 3; ++c) {
    const JpegComp& k = h.comp[c < h.ncomp ? c : 0];
    d->coef_off[c] = coef_base + k.coef_off;
    d->plane_off[c] = plane_base + k.coef_off;     // one byte per coefficient
    d->bw[c] = k.bw; d->bh[c] = k.bh; d->dw[c] = k.dw; d->dh[c] = k.dh;
    d->qoff[c] = qt_base + k.tq * 64;
    d->wg_start[c] = *wg;
    if (c < h.ncomp) *wg += (int32_t)(((uint64_t)k.bw * k.bh + kJpegBlocksPerWg - 1) / kJpegBlocksPerWg);
  }
  d->wg_start[3] = *wg;
  d->ncomp = h.ncomp; d->hs = h.hmax; d->vs = h.vmax;
  d->W = h.W; d->H = h.H; d->out_row = out_row;
  d->ytab = ytab; d->xtab = xtab;
}

void jpeg_pixels_cpu(const JpegHeader& h, const int16_t* coef, uint8_t* rgb) {
  std::vector<uint8_t> planes(h.ncoef);
  for (int c = 0; c < h.ncomp; ++c) {
    const JpegComp& k = h.comp[c];
    const size_t stride = (size_t)k.bw * 8;
    for (int by = 0; by < k.bh; ++by)
      for (int bx = 0; bx < k.bw; ++bx)
        idct_block(coef + k.coef_off + ((size_t)by * k.bw + bx) * 64, h.qt[k.tq],
                   planes.data() + k.coef_off + (size_t)by * 8 * stride + (size_t)bx * 8, stride);
  }
  JpegDesc d;
  int32_t wg = 0;
  jpeg_fill_desc(h, 0, 0, 0, &wg, 0, 0, 0, &d);
  for (int y = 0; y < h.H; ++y)
    for (int x = 0; x < h.W; ++x) jpeg_pixel(d, planes.data(), y, x, rgb + ((size_t)y * h.W + x) * 3);
}

}  // namespace kdl
