// Fuzz of the device entropy decode's host side under ASan+UBSan (tests/test_jpeg_huff_sanitize.py):
// jpeg_scan_prepare and jpeg_huff_cpu, the emulation that runs the kernels' own step code
// (runtime/jpeg_huff.h). Usage: jpeg_huff_fuzz <mutations per seed> <seed file>...
// Every seed file (written by the test with Pillow's encoder) must decode to jpeg_parse's
// coefficients; then fixed-seed mutations of it -- bit flips anywhere, byte edits and truncations
// inside the scan, edited Huffman tables -- are checked against the host decoder:
//   jpeg_parse says ok         -> the error word is clear and the coefficients are equal
//   jpeg_parse says malformed  -> the error word is set (when prepare accepted the file)
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

enum { HOST_OK_EQUAL, HOST_BAD_ERR_SET, NOT_PREPARED, NCOUNT };

static void die(const char* what, int it) {
  fprintf(stderr, "MISMATCH: %s (mutation %d)\n", what, it);
  exit(3);
}

static int check(const std::string& d, int it) {
  const uint8_t* p = reinterpret_cast<const uint8_t*>(d.data());
  JpegHeader h, h2;
  JpegHuffInfo info;
  std::vector<uint32_t> stage((jpeg_prepare_bound(d.size()) + 3) / 4);
  uint8_t* sp = reinterpret_cast<uint8_t*>(stage.data());
  const int st = jpeg_scan_prepare(p, d.size(), kMaxPixels, sp, stage.size() * 4, &h, &info);
  int host = jpeg_probe(p, d.size(), kMaxPixels, &h2);
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
  if (!info.device_ok) return NOT_PREPARED;  // restart intervals: the host decoder's
  if (info.nbytes > stage.size() * 4) die("prepare wrote past its bound", it);
  JpegHuffDesc desc;
  jpeg_huff_fill_desc(h, info, 0, 0, &desc);
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
    fprintf(stderr, "usage: jpeg_huff_fuzz <mutations per seed> <seed file>...\n");
    return 2;
  }
  const int iters = atoi(argv[1]);
  int counts[NCOUNT] = {0, 0, 0};
  for (int a = 2; a < argc; ++a) {
    const std::string seed = read_file(argv[a]);
    const size_t sos = seed.empty() ? std::string::npos : find_marker(seed, 0xDA);
    if (sos == std::string::npos || check(seed, -1) != HOST_OK_EQUAL) {
      fprintf(stderr, "seed %s does not decode\n", argv[a]);
      return 2;
    }
    const size_t scan = sos + 2 + (((size_t)(unsigned char)seed[sos + 2] << 8) | (unsigned char)seed[sos + 3]);
    const size_t dht = find_marker(seed, 0xC4);
    std::mt19937 rng(4321 + a);
    auto rnd = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    for (int it = 0; it < iters; ++it) {
      std::string d = seed;
      switch (it % 6) {
        case 0:                                   // one byte inside the scan
          d[scan + rnd(d.size() - scan)] = (char)rng();
          break;
        case 1:                                   // a few bit flips inside the scan
          for (int k = 0, n = 1 + (int)rnd(4); k < n; ++k) d[scan + rnd(d.size() - scan)] ^= (char)(1 << rnd(8));
          break;
        case 2:                                   // the scan cut short
          d.resize(scan + rnd(d.size() - scan));
          break;
        case 3:                                   // Huffman table counts and symbols
          if (dht != std::string::npos) {
            const size_t at = dht + 4 + rnd(60);
            if (at < scan) d[at] = (char)rng();
          }
          break;
        case 4:                                   // a run of bytes inside the scan overwritten
          for (size_t k = scan + rnd(d.size() - scan), n = 0; k < d.size() && n < 1 + rnd(16); ++k, ++n) d[k] = (char)rng();
          break;
        case 5:                                   // a few bit flips anywhere
          for (int k = 0, n = 1 + (int)rnd(3); k < n; ++k) d[rnd(d.size())] ^= (char)(1 << rnd(8));
          break;
      }
      ++counts[check(d, it)];
    }
  }
  printf("equal %d rejected %d unprepared %d\n", counts[0], counts[1], counts[2]);
  return 0;
}
