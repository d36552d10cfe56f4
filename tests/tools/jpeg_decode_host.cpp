// The decoding core of the GPU JPEG reader (audio2photoreal_amd/csrc/jpeg_decode_core.h) on the host, for a run under
// AddressSanitizer and UndefinedBehaviorSanitizer before anything runs on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I audio2photoreal_amd/csrc
//       tests/tools/jpeg_decode_host.cpp -o jpeg_decode_host
//   jpeg_decode_host decode FILE...            decodes every file; writes FILE.coef (int16, the layout of a2p_jpeg_coefficients) and
//                                              prints "FILE status=<s> rows=.. cols=.. bpm=.. intervals=.."
//   jpeg_decode_host fuzz SEED COUNT FILE...   COUNT seeded corruptions of every file's entropy-coded segment (byte flips, truncations,
//                                              inserted markers), each decoded from a heap copy of its exact length; prints a tally
// The entropy-coded bytes go through exactly the functions the kernels call: jpeg_restart_ranges (the sequential form of the scan)
// and jpeg_decode_interval.  A rejected stream is a result (status != 0, exit code 0); only a file this program cannot read or a
// header outside what the decoder takes exits with 2.  tests/test_video_decode_cpu.py builds and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "jpeg_decode_core.h"

struct Header {
  int H = 0, W = 0, ncomp = 0, hs = 1, vs = 1, ri = 0;
  int comp_id[3] = {0, 0, 0};
  bool have[JPEG_TABLES] = {false, false, false, false};
  int32_t tables[JPEG_TABLES * JPEG_TABLE_WORDS];
  JpegScan scan;
  size_t seg_begin = 0, seg_end = 0;
};

// Annex K.3, used when a file carries no DHT (the AVI convention)
static const uint8_t K_BITS[4][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0},
                                      {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static const uint8_t K_AC_LUMA[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
static const uint8_t K_AC_CHROMA[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

// BITS and HUFFVAL -> the decoder's table (include/a2p_hip.h); false for counts that are no prefix code
static bool build_table(const uint8_t* bits, const uint8_t* vals, int nvals, int32_t* t) {
  memset(t, 0, JPEG_TABLE_WORDS * 4);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t[l - 1] = -1;
    if (bits[l - 1]) {
      t[16 + l - 1] = k - code;
      code += bits[l - 1], k += bits[l - 1];
      if (code > (1 << l) || k > nvals || k > 256) return false;
      t[l - 1] = code - 1;
    }
    code <<= 1;
  }
  memcpy(t + 32, vals, (size_t)k);
  return true;
}

static bool parse(const std::vector<uint8_t>& d, Header& h, std::string& why) {
  auto fail = [&](const char* m) { why = m; return false; };
  if (d.size() < 4 || d[0] != 0xFF || d[1] != 0xD8) return fail("no SOI");
  memset(h.tables, 0, sizeof(h.tables));
  for (int i = 0; i < JPEG_TABLES; ++i)
    for (int l = 0; l < 16; ++l) h.tables[i * JPEG_TABLE_WORDS + l] = -1;
  bool any_dht = false;
  int tq[3] = {0, 0, 0};
  (void)tq;
  size_t at = 2;
  while (true) {
    if (at + 4 > d.size() || d[at] != 0xFF) return fail("no marker where one is due");
    const int code = d[at + 1];
    const size_t len = (size_t)d[at + 2] << 8 | d[at + 3];
    if (len < 2 || at + 2 + len > d.size()) return fail("a marker segment runs past the file");
    const uint8_t* b = d.data() + at + 4;
    const size_t n = len - 2;
    if (code == 0xC4) {
      size_t o = 0;
      while (o < n) {
        if (o + 17 > n) return fail("a DHT segment is cut short");
        const int tc = b[o] >> 4, th = b[o] & 15;
        int sum = 0;
        for (int l = 0; l < 16; ++l) sum += b[o + 1 + l];
        if (tc > 1 || th > 1) return fail("a Huffman table beyond DC / AC 0 and 1 (not baseline)");
        if (sum > 256 || o + 17 + (size_t)sum > n) return fail("a DHT segment is cut short");
        if (!build_table(b + o + 1, b + o + 17, sum, h.tables + (tc * 2 + th) * JPEG_TABLE_WORDS)) return fail("a DHT is no prefix code");
        h.have[tc * 2 + th] = any_dht = true;
        o += 17 + (size_t)sum;
      }
    } else if (code == 0xC0) {
      if (n < 6 || b[0] != 8) return fail("not 8-bit samples");
      h.H = b[1] << 8 | b[2], h.W = b[3] << 8 | b[4], h.ncomp = b[5];
      if ((h.ncomp != 1 && h.ncomp != 3) || n < 6 + 3 * (size_t)h.ncomp) return fail("neither 1 nor 3 components");
      if (h.H < 1 || h.W < 1) return fail("an empty frame");
      for (int c = 0; c < h.ncomp; ++c) {
        h.comp_id[c] = b[6 + 3 * c];
        const int hv = b[7 + 3 * c];
        if (c == 0) h.hs = hv >> 4, h.vs = hv & 15;
        else if (hv != 0x11) return fail("chrominance is not sampled 1 x 1");
      }
      if (h.ncomp == 1) h.hs = h.vs = 1;
      if (!((h.hs == 1 && h.vs == 1) || (h.hs == 2 && h.vs == 1) || (h.hs == 2 && h.vs == 2))) return fail("luminance sampling is not 1x1, 2x1 or 2x2");
    } else if (code >= 0xC1 && code <= 0xCF && code != 0xC8 && code != 0xCC) {
      return fail("not a baseline frame (SOF1 .. SOF15)");
    } else if (code == 0xDD) {
      if (n != 2) return fail("a DRI segment of the wrong length");
      h.ri = b[0] << 8 | b[1];
    } else if (code == 0xDA) {
      if (!h.ncomp) return fail("SOS before SOF0");
      if (n < 1 || b[0] != h.ncomp || n != 4 + 2 * (size_t)h.ncomp) return fail("the scan does not hold every component");
      for (int c = 0; c < h.ncomp; ++c) {
        if (b[1 + 2 * c] != h.comp_id[c]) return fail("the scan's components are not in the frame's order");
        h.scan.dc[c] = b[2 + 2 * c] >> 4, h.scan.ac[c] = b[2 + 2 * c] & 15;
        if (h.scan.dc[c] > 1 || h.scan.ac[c] > 1) return fail("a table selector above 1");
      }
      for (int c = h.ncomp; c < 3; ++c) h.scan.dc[c] = h.scan.ac[c] = 0;
      if (b[n - 3] != 0 || b[n - 2] != 63 || b[n - 1] != 0) return fail("not a sequential scan");
      h.seg_begin = at + 2 + len;
      h.seg_end = d.size();
      for (size_t i = d.size(); i >= h.seg_begin + 2; --i)
        if (d[i - 2] == 0xFF && d[i - 1] == 0xD9) {
          h.seg_end = i - 2;
          break;
        }
      break;
    }
    at += 2 + len;
  }
  if (!any_dht) {
    const uint8_t dcv[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    build_table(K_BITS[0], dcv, 12, h.tables), build_table(K_BITS[1], dcv, 12, h.tables + JPEG_TABLE_WORDS);
    build_table(K_BITS[2], K_AC_LUMA, 162, h.tables + 2 * JPEG_TABLE_WORDS), build_table(K_BITS[3], K_AC_CHROMA, 162, h.tables + 3 * JPEG_TABLE_WORDS);
  }
  h.scan.ny = h.ncomp == 1 ? 1 : h.hs * h.vs;
  h.scan.bpm = h.ncomp == 1 ? 1 : h.scan.ny + 2;
  return true;
}

// The whole integer stage on a heap copy of the segment's exact length; coef: [mcus][bpm][64], zeroed here.
static int32_t decode_segment(const Header& h, const uint8_t* seg, int64_t nbytes, std::vector<int16_t>& coef, int64_t& intervals) {
  const int64_t rows = (h.H + 8 * h.vs - 1) / (8 * h.vs), cols = (h.W + 8 * h.hs - 1) / (8 * h.hs), mcus = rows * cols;
  const int64_t ri = h.ri ? h.ri : mcus;
  intervals = (mcus + ri - 1) / ri;
  coef.assign((size_t)(mcus * h.scan.bpm * 64), 0);
  std::vector<int64_t> ranges((size_t)intervals + 1);
  int32_t status = jpeg_restart_ranges(seg, 0, nbytes, intervals, ranges.data());
  if (status) return status;
  for (int64_t iv = 0; iv < intervals; ++iv) {
    const int64_t end = ranges[(size_t)iv + 1] - (iv + 1 < intervals ? 2 : 0);
    const int64_t m0 = iv * ri, m1 = m0 + ri < mcus ? m0 + ri : mcus;
    const int cause = jpeg_decode_interval(seg, ranges[(size_t)iv], end, h.tables, h.scan, m0, m1, coef.data());
    if (cause && !status) status = JPEG_STATUS(iv, cause);
  }
  return status;
}

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t n;
  out.clear();
  while ((n = fread(buf, 1, sizeof(buf), f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

static uint64_t rng_state;
static uint32_t rng() {                                           // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int main(int argc, char** argv) {
  if (argc < 3 || (strcmp(argv[1], "decode") && strcmp(argv[1], "fuzz")) || (!strcmp(argv[1], "fuzz") && argc < 5)) {
    fprintf(stderr, "usage: %s decode FILE... | fuzz SEED COUNT FILE...\n", argv[0]);
    return 2;
  }
  const bool fuzz = !strcmp(argv[1], "fuzz");
  const long count = fuzz ? atol(argv[3]) : 0;
  if (fuzz) rng_state = strtoull(argv[2], nullptr, 10);
  for (int a = fuzz ? 4 : 2; a < argc; ++a) {
    std::vector<uint8_t> file;
    Header h;
    std::string why;
    if (!read_file(argv[a], file)) {
      fprintf(stderr, "%s: cannot read\n", argv[a]);
      return 2;
    }
    if (!parse(file, h, why)) {
      fprintf(stderr, "%s: %s\n", argv[a], why.c_str());
      return 2;
    }
    const size_t n = h.seg_end - h.seg_begin;
    std::vector<int16_t> coef;
    int64_t intervals = 0;
    if (!fuzz) {
      uint8_t* seg = (uint8_t*)malloc(n ? n : 1);                  // its exact length: one byte too many read is a report
      memcpy(seg, file.data() + h.seg_begin, n);
      const int32_t status = decode_segment(h, seg, (int64_t)n, coef, intervals);
      free(seg);
      const std::string out = std::string(argv[a]) + ".coef";
      FILE* f = fopen(out.c_str(), "wb");
      if (!f || fwrite(coef.data(), 2, coef.size(), f) != coef.size()) return 2;
      fclose(f);
      printf("%s status=%d rows=%d cols=%d bpm=%d intervals=%lld\n", argv[a], status, (h.H + 8 * h.vs - 1) / (8 * h.vs),
             (h.W + 8 * h.hs - 1) / (8 * h.hs), h.scan.bpm, (long long)intervals);
      continue;
    }
    std::map<int, long> tally;
    for (long i = 0; i < count; ++i) {
      std::vector<uint8_t> s(file.begin() + (long)h.seg_begin, file.begin() + (long)h.seg_end);
      const int kind = (int)(rng() % 4);
      if (kind == 0 && !s.empty()) {                               // byte flips
        for (int k = 1 + (int)(rng() % 4); k > 0; --k) s[rng() % s.size()] ^= (uint8_t)(1u << (rng() % 8));
      } else if (kind == 1) {                                      // truncation
        s.resize(s.empty() ? 0 : rng() % s.size());
      } else if (kind == 2) {                                      // an inserted marker: RSTm, EOI, a fill byte or a bare 0xFF
        const uint8_t second[] = {0xD0, 0xD3, 0xD7, 0xD9, 0xFF, 0xC4};
        const size_t at = s.empty() ? 0 : rng() % (s.size() + 1);
        const uint32_t pick = rng() % 7;
        s.insert(s.begin() + (long)at, (uint8_t)0xFF);
        if (pick < 6) s.insert(s.begin() + (long)at + 1, second[pick]);
      } else if (!s.empty()) {                                     // random bytes over a stretch
        const size_t at = rng() % s.size(), len = 1 + rng() % 16;
        for (size_t k = at; k < s.size() && k < at + len; ++k) s[k] = (uint8_t)rng();
      }
      uint8_t* seg = (uint8_t*)malloc(s.empty() ? 1 : s.size());
      if (!s.empty()) memcpy(seg, s.data(), s.size());
      const int32_t status = decode_segment(h, seg, (int64_t)s.size(), coef, intervals);
      free(seg);
      ++tally[status & 15];
    }
    printf("%s fuzz=%ld", argv[a], count);
    for (const auto& kv : tally) printf(" cause%d=%ld", kv.first, kv.second);
    printf("\n");
  }
  return 0;
}
