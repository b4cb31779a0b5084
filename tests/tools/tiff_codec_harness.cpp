// Stand-alone sanitizer harness for the host TIFF decoders (floodplanet_code_amd/csrc/fu_tiff_codec.cpp).  Not run by
// pytest, not for a GPU machine, nothing loaded into Python:
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Ifloodplanet_code_amd/csrc \
//       tests/tools/tiff_codec_harness.cpp floodplanet_code_amd/csrc/fu_tiff_codec.cpp -o tiff_codec_harness
//   ./tiff_codec_harness
//
// It encodes buffers with small encoders of its own, then feeds valid, truncated (every prefix length) and bit-flipped
// streams into EXACTLY sized heap buffers -- the source n_src bytes, the destination n_dst bytes -- so that one byte read
// or written out of bounds is an AddressSanitizer report.  A valid stream must decode to its data; a damaged one must
// return an error or at most n_dst bytes.  Exit status 0 and "harness ok" when nothing was reported.
#include "fu_tiff_codec.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <vector>

namespace {

typedef std::vector<uint8_t> Bytes;

struct BitWriter {
  Bytes out;
  uint64_t acc = 0;
  int n = 0;
  void put(int code, int nbits) {
    acc = (acc << nbits) | (uint64_t)code;
    n += nbits;
    while (n >= 8) {
      out.push_back((uint8_t)(acc >> (n - 8)));
      n -= 8;
    }
    acc &= (1ull << n) - 1;
  }
  void flush() {
    if (n) out.push_back((uint8_t)(acc << (8 - n)));
    n = 0;
  }
};

Bytes lzw_encode(const Bytes& data) {
  BitWriter w;
  int nbits = 9, free_ent = 258;
  std::map<uint32_t, int> table;
  w.put(256, nbits);
  if (!data.empty()) {
    int prefix = data[0];
    for (size_t i = 1; i < data.size(); ++i) {
      const uint32_t key = ((uint32_t)prefix << 8) | data[i];
      auto hit = table.find(key);
      if (hit != table.end()) {
        prefix = hit->second;
        continue;
      }
      w.put(prefix, nbits);
      table[key] = free_ent++;
      prefix = data[i];
      if (free_ent == 4094) {
        w.put(256, nbits);
        table.clear();
        nbits = 9, free_ent = 258;
      } else if (free_ent > (1 << nbits) - 1) {
        ++nbits;
      }
    }
    w.put(prefix, nbits);
    ++free_ent;
    if (free_ent == 4094) {
      w.put(256, nbits);
      nbits = 9;
    } else if (free_ent > (1 << nbits) - 1) {
      ++nbits;
    }
  }
  w.put(257, nbits);
  w.flush();
  return w.out;
}

Bytes packbits_encode(const Bytes& d) {
  Bytes out;
  size_t i = 0, n = d.size();
  while (i < n) {
    size_t run = 1;
    while (i + run < n && run < 128 && d[i + run] == d[i]) ++run;
    if (run >= 2) {
      out.push_back((uint8_t)(257 - run));
      out.push_back(d[i]);
      i += run;
      continue;
    }
    size_t j = i + 1;
    while (j < n && j - i < 128 && !(j + 1 < n && d[j] == d[j + 1])) ++j;
    out.push_back((uint8_t)(j - i - 1));
    out.insert(out.end(), d.begin() + i, d.begin() + j);
    i = j;
  }
  return out;
}

typedef int64_t (*Decoder)(const uint8_t*, int64_t, uint8_t*, int64_t);

// decode src[0, n_src) into a heap buffer of exactly n_dst bytes; the copies are exactly sized too
int64_t run(Decoder f, const uint8_t* src, size_t n_src, size_t n_dst, Bytes* result) {
  uint8_t* s = (uint8_t*)malloc(n_src ? n_src : 1);
  uint8_t* d = (uint8_t*)malloc(n_dst ? n_dst : 1);
  if (n_src) memcpy(s, src, n_src);
  // a zero-sized buffer is passed as its one-byte allocation with size 0: touching even that byte is checked below
  if (!n_src) s[0] = 0x5a;
  if (!n_dst) d[0] = 0x5a;
  const int64_t got = f(s, (int64_t)n_src, d, (int64_t)n_dst);
  if ((!n_dst && d[0] != 0x5a) || got > (int64_t)n_dst) {
    fprintf(stderr, "decoder wrote past n_dst = %zu (returned %lld)\n", n_dst, (long long)got);
    exit(1);
  }
  if (result) result->assign(d, d + (got > 0 ? got : 0));
  free(s);
  free(d);
  return got;
}

uint32_t g_state = 12345u;
uint32_t rnd() {
  g_state = g_state * 1664525u + 1013904223u;
  return g_state >> 8;
}

int check(const char* name, Decoder f, Bytes (*encode)(const Bytes&), const Bytes& data) {
  const Bytes enc = encode(data);
  Bytes back;
  if (run(f, enc.data(), enc.size(), data.size(), &back) != (int64_t)data.size() || back != data) {
    fprintf(stderr, "%s: a valid stream of %zu bytes did not decode to its data\n", name, data.size());
    return 1;
  }
  for (size_t n_dst : {(size_t)0, (size_t)1, data.size() / 3, data.size() + 7}) {   // stops at n_dst / at the end
    const int64_t got = run(f, enc.data(), enc.size(), n_dst, &back);
    const size_t want = n_dst < data.size() ? n_dst : data.size();
    if (got != (int64_t)want || (want && memcmp(back.data(), data.data(), want) != 0)) {
      fprintf(stderr, "%s: n_dst = %zu gave %lld\n", name, n_dst, (long long)got);
      return 1;
    }
  }
  const size_t prefixes = enc.size() < 600 ? enc.size() : 600;
  for (size_t cut = 0; cut < prefixes; ++cut) {                                      // truncated at every position
    const int64_t got = run(f, enc.data(), cut, data.size(), &back);
    if (got > 0 && memcmp(back.data(), data.data(), (size_t)got) != 0) {
      fprintf(stderr, "%s: a stream cut at %zu decoded to other bytes\n", name, cut);
      return 1;
    }
  }
  for (int trial = 0; trial < 3000 && !enc.empty(); ++trial) {                       // bit flips, some with truncation
    Bytes bad = enc;
    const int flips = 1 + (int)(rnd() % 4);
    for (int k = 0; k < flips; ++k) bad[rnd() % bad.size()] ^= (uint8_t)(1u << (rnd() % 8));
    const size_t keep = trial % 3 == 0 ? 1 + rnd() % bad.size() : bad.size();
    const size_t n_dst = trial % 5 == 0 ? rnd() % (data.size() + 1) : data.size();
    run(f, bad.data(), keep, n_dst, nullptr);                                        // any result; no bad access
  }
  return 0;
}

}  // namespace

int main() {
  std::vector<Bytes> inputs;
  inputs.push_back(Bytes());
  inputs.push_back(Bytes(1, 7));
  inputs.push_back(Bytes(50000, 0));                           // code == next free entry, all the way
  Bytes noise(9000), few(40000), mixed;
  for (auto& b : noise) b = (uint8_t)rnd();                    // fills the 12-bit table and clears it
  for (auto& b : few) b = (uint8_t)(rnd() % 3);
  for (int r = 0; r < 6; ++r) {
    for (int i = 0; i < 700; ++i) mixed.push_back((uint8_t)("ab"[i & 1]));
    for (int i = 0; i < 512; ++i) mixed.push_back((uint8_t)i);
    mixed.insert(mixed.end(), 900, 9);
    mixed.insert(mixed.end(), noise.begin(), noise.begin() + 300);
  }
  inputs.push_back(noise);
  inputs.push_back(few);
  inputs.push_back(mixed);
  int bad = 0;
  for (const Bytes& d : inputs) {
    bad += check("fu_tiff_lzw_decode", fu_tiff_lzw_decode, lzw_encode, d);
    bad += check("fu_tiff_packbits_decode", fu_tiff_packbits_decode, packbits_encode, d);
  }
  // raw garbage and the old LSB-first header
  for (int trial = 0; trial < 3000; ++trial) {
    Bytes junk(1 + rnd() % 300);
    for (auto& b : junk) b = (uint8_t)rnd();
    if (trial % 4 == 0) junk[0] = 0x80;                        // starts with a Clear, so the LZW decoder goes on
    run(fu_tiff_lzw_decode, junk.data(), junk.size(), rnd() % 5000, nullptr);
    run(fu_tiff_packbits_decode, junk.data(), junk.size(), rnd() % 5000, nullptr);
  }
  const uint8_t old_style[4] = {0x00, 0x01, 0x02, 0x03};
  if (run(fu_tiff_lzw_decode, old_style, 4, 16, nullptr) != FU_TIFF_CODEC_OLD_LZW) {
    fprintf(stderr, "the LSB-first variant was not rejected\n");
    ++bad;
  }
  if (bad) return 1;
  printf("harness ok\n");
  return 0;
}
