// Fuzz of the restart-interval entropy decode's host side under ASan+UBSan
// (tests/test_jpeg_rst_sanitize.py): jpeg_scan_prepare, which walks the RSTm markers and builds the
// interval and group tables, and jpeg_huff_cpu, the emulation that runs the kernels' own step code
// (runtime/jpeg_huff.h). Usage: jpeg_rst_fuzz <mutations per seed> <seed file>...
// Every seed file (written by the test with Pillow's encoder, with restart markers) must decode to
// jpeg_parse's coefficients; then fixed-seed mutations of the whole file -- headers, markers and
// scan -- are checked against the host decoder:
//   prepare refuses the file (a bad header, restart_ok false)  -> counted, the host decoder's
//   jpeg_parse says ok         -> the error word is clear and the coefficients are equal
//   jpeg_parse says malformed  -> the error word is set
// and no index may pass the emulation's second bounds check. The sanitizers watch every read and
// index on the way.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../runtime/jpeg_huff.h"

using namespace kdl;

static const uint64_t kMaxPixels = 1 << 20;

static std::string read_file(const char* path) {
  std::string s;
  FILE* f = fopen(path, "rb");
  if (!f) return s;
  char buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) s.append(buf, n);
  fclose(f);
  return s;
}

static size_t find_marker(const std::string& d, int marker) {
  size_t pos = 2;
  while (pos + 4 <= d.size() && (unsigned char)d[pos] == 0xFF) {
    const int m = (unsigned char)d[pos + 1];
    const size_t len = ((size_t)(unsigned char)d[pos + 2] << 8) | (unsigned char)d[pos + 3];
    if (m == marker) return pos;
    if (m == 0xDA || len < 2) break;
    pos += 2 + len;
  }
  return std::string::npos;
}

// the RSTm markers of a well-formed scan: inside it FF Dx occurs as nothing else
static std::vector<size_t> restart_markers(const std::string& d, size_t scan) {
  std::vector<size_t> at;
  for (size_t i = scan; i + 1 < d.size(); ++i)
    if ((unsigned char)d[i] == 0xFF && (unsigned char)d[i + 1] >= 0xD0 && (unsigned char)d[i + 1] <= 0xD7) at.push_back(i);
  return at;
}

enum { HOST_OK_EQUAL, HOST_BAD_ERR_SET, NOT_PREPARED, NCOUNT };

static void die(const char* what, int it) {
  fprintf(stderr, "MISMATCH: %s (mutation %d)\n", what, it);
  exit(3);
}

// the intervals the file can have at most: the bound that the serving path passes
static uint64_t most_intervals(const JpegHeader& h) {
  if (h.ncomp < 1 || h.comp[0].h < 1 || h.comp[0].v < 1) return 0;
  return (uint64_t)(h.comp[0].bw / h.comp[0].h) * (uint64_t)(h.comp[0].bh / h.comp[0].v);
}

static int check(const std::string& d, int it) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(d.data());
  JpegHeader h, h2;
  JpegHuffInfo info;
  int host = jpeg_probe(p, d.size(), kMaxPixels, &h2);
  const uint64_t bound = jpeg_prepare_bound(d.size(), host == JPEG_OK ? most_intervals(h2) : 0);
  std::vector<uint32_t> stage((bound + 3) / 4);
  uint8_t* sp = reinterpret_cast<uint8_t*>(stage.data());
  const int st = jpeg_scan_prepare(p, d.size(), kMaxPixels, sp, stage.size() * 4, &h, &info);
  std::vector<int16_t> want;
  if (host == JPEG_OK) {
    want.assign(h2.ncoef, (int16_t)0x5A5A);
    host = jpeg_parse(p, d.size(), kMaxPixels, want.data(), want.size(), &h2);
  } else {                                   // the probe skips the Huffman tables: the full walk's answer
    host = jpeg_parse(p, d.size(), kMaxPixels, nullptr, 0, &h2);
  }
  if (st != JPEG_OK) {                       // the header is bad: the same answer as the host decoder
    if (host != st || strcmp(h.why, h2.why)) die("prepare and jpeg_parse disagree about the headers", it);
    return NOT_PREPARED;
  }
  if (info.nbytes > stage.size() * 4) die("prepare wrote past its bound", it);
  if (info.device_ok && info.restart_ok) die("a file is of one kind", it);
  if (info.device_ok != (h.restart == 0)) die("device_ok for a file with restart intervals", it);
  if (!info.device_ok && !info.restart_ok) return NOT_PREPARED;      // markers out of order or number
  JpegHuffDesc desc;
  jpeg_huff_fill_desc(h, info, 0, 0, &desc);
  if (jpeg_huff_desc_is_rst(desc) != info.restart_ok) die("the descriptor is of the wrong kind", it);
  std::vector<int16_t> coef(h.ncoef, (int16_t)0x5A5A);
  uint32_t err = 0, rounds = 0;
  // the staging of the call ends with the image: anything read behind it is the sanitizer's
  std::vector<uint32_t> exact(stage.begin(), stage.begin() + info.nbytes / 4);
  const uint64_t bad = jpeg_huff_cpu(desc, reinterpret_cast<const uint8_t*>(exact.data()), info.nbytes, coef.data(),
                                     coef.size(), &err, &rounds);
  if (bad) die("an index passed the shared code's bounds check", it);
  if (host == JPEG_OK) {
    if (err) die("error word set for a file the host decoder accepts", it);
    if (coef != want) die("coefficients differ from jpeg_parse", it);
    return HOST_OK_EQUAL;
  }
  if (host != JPEG_MALFORMED) die("prepare accepted what jpeg_parse calls unsupported", it);
  if (!err) die("error word clear for a scan the host decoder rejects", it);
  return HOST_BAD_ERR_SET;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: jpeg_rst_fuzz <mutations per seed> <seed file>...\n");
    return 2;
  }
  const int iters = atoi(argv[1]);
  int counts[NCOUNT] = {0, 0, 0};
  for (int a = 2; a < argc; ++a) {
    const std::string seed = read_file(argv[a]);
    const size_t sos = seed.empty() ? std::string::npos : find_marker(seed, 0xDA);
    if (sos == std::string::npos || find_marker(seed, 0xDD) == std::string::npos || check(seed, -1) != HOST_OK_EQUAL) {
      fprintf(stderr, "seed %s does not decode as a file with restart intervals\n", argv[a]);
      return 2;
    }
    const size_t scan = sos + 2 + (((size_t)(unsigned char)seed[sos + 2] << 8) | (unsigned char)seed[sos + 3]);
    const size_t dri = find_marker(seed, 0xDD);
    const std::vector<size_t> rst = restart_markers(seed, scan);
    std::mt19937 rng(8765 + a);
    auto rnd = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    for (int it = 0; it < iters; ++it) {
      std::string d = seed;
      switch (it % 8) {
        case 0:                                   // one byte inside the scan
          d[scan + rnd(d.size() - scan)] = (char)rng();
          break;
        case 1:                                   // a few bit flips inside the scan
          for (int k = 0, n = 1 + (int)rnd(4); k < n; ++k) d[scan + rnd(d.size() - scan)] ^= (char)(1 << rnd(8));
          break;
        case 2:                                   // the file cut short inside the scan
          d.resize(scan + rnd(d.size() - scan));
          break;
        case 3:                                   // the restart interval of the DRI segment
          d[dri + 4 + rnd(2)] = (char)rng();
          break;
        case 4:                                   // a marker renumbered, removed or doubled
          if (!rst.empty()) {
            const size_t m = rst[rnd(rst.size())];
            const size_t kind = rnd(3);
            if (kind == 0) d[m + 1] = (char)(0xD0 + rnd(8));
            if (kind == 1) d.erase(m, 2);
            if (kind == 2) d.insert(m, d.substr(m, 2));
          }
          break;
        case 5:                                   // a few bit flips anywhere
          for (int k = 0, n = 1 + (int)rnd(3); k < n; ++k) d[rnd(d.size())] ^= (char)(1 << rnd(8));
          break;
        case 6:                                   // a marker of some kind written into the scan
          if (d.size() - scan > 2) {
            const size_t at = scan + rnd(d.size() - scan - 1);
            d[at] = (char)0xFF;
            d[at + 1] = (char)(rnd(2) ? 0xD0 + rnd(8) : rng());
          }
          break;
        case 7:                                   // a run of bytes inside the scan overwritten
          for (size_t k = scan + rnd(d.size() - scan), n = 0; k < d.size() && n < 1 + rnd(16); ++k, ++n) d[k] = (char)rng();
          break;
      }
      ++counts[check(d, it)];
    }
  }
  printf("equal %d rejected %d unprepared %d\n", counts[0], counts[1], counts[2]);
  return 0;
}
