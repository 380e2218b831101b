// Malformed-input fuzz of the baseline JPEG decoder (runtime/jpeg.cpp) under ASan+UBSan
// (tests/test_jpeg_sanitize.py). Usage: jpeg_fuzz <mutations per seed> <seed file>...
// Every seed file (written by the test with Pillow's encoder) must decode; then fixed-seed
// mutations of it -- bit flips, truncations, edited segment lengths, sampling bytes and table
// ids -- go through jpeg_probe, jpeg_parse and jpeg_pixels_cpu. Each must come back as ok,
// unsupported or malformed; the sanitizers watch every read and index on the way.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <string>
#include <vector>

#include "../runtime/jpeg.h"

using namespace kdl;

static const uint64_t kMaxPixels = 1 << 20;   // keeps a mutated frame header from asking for gigabytes

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

// positions of the segments of one marker (the byte after FF xx), up to the scan
static std::vector<size_t> segments(const std::string& d, int marker) {
  std::vector<size_t> out;
  size_t pos = 2;
  while (pos + 4 <= d.size() && (unsigned char)d[pos] == 0xFF) {
    const int m = (unsigned char)d[pos + 1];
    const size_t len = ((size_t)(unsigned char)d[pos + 2] << 8) | (unsigned char)d[pos + 3];
    if (m == marker) out.push_back(pos + 2);
    if (m == 0xDA || len < 2) break;
    pos += 2 + len;
  }
  return out;
}

static int decode(const std::string& d, int counts[3], bool pixels) {
  JpegHeader h;
  const uint8_t* p = reinterpret_cast<const uint8_t*>(d.data());
  int st = jpeg_probe(p, d.size(), kMaxPixels, &h);
  if (st == JPEG_OK) {
    std::vector<int16_t> coef(h.ncoef, (int16_t)0x5A5A);
    st = jpeg_parse(p, d.size(), kMaxPixels, coef.data(), coef.size(), &h);
    if (st == JPEG_OK && pixels) {
      std::vector<uint8_t> rgb((size_t)h.W * h.H * 3);
      jpeg_pixels_cpu(h, coef.data(), rgb.data());
    }
  }
  if (st != JPEG_OK && st != JPEG_UNSUPPORTED && st != JPEG_MALFORMED) {
    fprintf(stderr, "status %d is none of ok / unsupported / malformed\n", st);
    exit(2);
  }
  ++counts[st];
  return st;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: jpeg_fuzz <mutations per seed> <seed file>...\n");
    return 2;
  }
  const int iters = atoi(argv[1]);
  int counts[3] = {0, 0, 0};
  for (int a = 2; a < argc; ++a) {
    const std::string seed = read_file(argv[a]);
    int c0[3] = {0, 0, 0};
    if (seed.empty() || decode(seed, c0, true) != JPEG_OK) {
      fprintf(stderr, "seed %s does not decode\n", argv[a]);
      return 2;
    }
    const std::vector<size_t> sof = segments(seed, 0xC0), sos = segments(seed, 0xDA), dht = segments(seed, 0xC4),
                              dqt = segments(seed, 0xDB);
    std::mt19937 rng(1234 + a);
    auto rnd = [&](size_t n) { return (size_t)(rng() % (n ? n : 1)); };
    for (int it = 0; it < iters; ++it) {
      std::string d = seed;
      switch (it % 8) {
        case 0:                                   // a few bit flips anywhere
          for (int k = 0, n = 1 + (int)rnd(4); k < n; ++k) d[rnd(d.size())] ^= (char)(1 << rnd(8));
          break;
        case 1:                                   // bit flips in the headers only
          for (int k = 0, n = 1 + (int)rnd(3); k < n; ++k) d[rnd(sos.empty() ? d.size() : sos[0])] ^= (char)(1 << rnd(8));
          break;
        case 2:                                   // truncation
          d.resize(rnd(d.size()));
          break;
        case 3: {                                 // a segment length
          const std::vector<size_t>* v[4] = {&sof, &sos, &dht, &dqt};
          const std::vector<size_t>& s = *v[rnd(4)];
          if (s.empty()) break;
          const size_t at = s[rnd(s.size())];
          const unsigned len = (rng() & 1) ? (unsigned)rnd(65536) : (unsigned)rnd(40);
          d[at] = (char)(len >> 8);
          d[at + 1] = (char)len;
          break;
        }
        case 4:                                   // sampling byte / table id of a frame component
          if (!sof.empty()) {
            const int nc = (unsigned char)seed[sof[0] + 7];
            const size_t at = sof[0] + 8 + 3 * rnd(nc ? nc : 1) + 1 + rnd(2);
            if (at < d.size()) d[at] = (char)rng();
          }
          break;
        case 5:                                   // frame dimensions, precision, component count
          if (!sof.empty()) {
            const size_t at = sof[0] + 2 + rnd(6);
            if (at < d.size()) d[at] = (char)rng();
          }
          break;
        case 6:                                   // Huffman table selectors / scan parameters
          if (!sos.empty()) {
            const size_t at = sos[0] + 2 + rnd(10);
            if (at < d.size()) d[at] = (char)rng();
          }
          break;
        case 7:                                   // Huffman table class/id, counts and symbols
          if (!dht.empty()) {
            const size_t at = dht[rnd(dht.size())] + 2 + rnd(40);
            if (at < d.size()) d[at] = (char)rng();
          }
          break;
      }
      decode(d, counts, it % 3 == 0);
    }
  }
  printf("ok %d unsupported %d malformed %d\n", counts[0], counts[1], counts[2]);
  return 0;
}
