// TIFF entropy decoders for the host (fu_tiff_codec.h).  No HIP here: plain C++ that any host compiler takes.
//
// Both decoders are written against corrupt and truncated input: every read is checked against n_src, every write against
// n_dst, every LZW code against the table as it stands.  tests/tools/tiff_codec_harness.cpp feeds them valid, truncated and
// bit-flipped streams in exactly sized heap buffers under the address and undefined-behaviour sanitizers.
#include "fu_tiff_codec.h"

#include <string.h>

namespace {

constexpr int kLzwClear = 256, kLzwEoi = 257, kLzwFirst = 258, kLzwTable = 4096;

}  // namespace

extern "C" {

// TIFF 6.0 section 13.  Codes are packed MSB first, 9 to 12 bits wide; 256 clears the table, 257 ends the data.  The width
// grows "one code early": after the entry (1 << width) - 2 has been added the next code is one bit wider.  A code equal to
// the next free entry is the string of the previous code plus that string's first byte.  A string is kept as
// (prefix code, last byte, length, first byte) and written back to front into its place in dst.
int64_t fu_tiff_lzw_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst) {
  if (n_src < 0 || n_dst < 0 || (n_src > 0 && !src) || (n_dst > 0 && !dst)) return FU_TIFF_CODEC_BAD_ARGS;
  if (n_src >= 2 && src[0] == 0 && (src[1] & 1)) return FU_TIFF_CODEC_OLD_LZW;   // an LSB-first Clear: 0x00 0x01
  uint16_t prefix[kLzwTable];
  uint16_t length[kLzwTable];
  uint8_t suffix[kLzwTable], first[kLzwTable];
  for (int i = 0; i < 256; ++i) {
    prefix[i] = 0, length[i] = 1, suffix[i] = (uint8_t)i, first[i] = (uint8_t)i;
  }
  int nbits = 9, next = kLzwFirst, old = -1;
  uint64_t acc = 0;     // the low `have` bits are the stream's bits not consumed yet
  int have = 0;
  int64_t in = 0, out = 0;
  while (out < n_dst) {
    while (have < nbits && in < n_src) {
      acc = (acc << 8) | src[in++];
      have += 8;
    }
    if (have < nbits) break;                                   // the stream ends without an EOI: a short count
    const int code = (int)((acc >> (have - nbits)) & ((1u << nbits) - 1u));
    have -= nbits;
    if (code == kLzwEoi) break;
    if (code == kLzwClear) {
      nbits = 9, next = kLzwFirst, old = -1;
      continue;
    }
    if (old < 0) {                                             // the first code after a Clear is a literal
      if (code > 255) return FU_TIFF_CODEC_CORRUPT;
      dst[out++] = (uint8_t)code;
      old = code;
      continue;
    }
    int emit;                                                  // the table entry to write out
    uint8_t head;                                              // the first byte of the new entry's last position
    if (code < next && code != kLzwClear && code != kLzwEoi) {
      emit = code, head = first[code];
    } else if (code == next && next < kLzwTable) {
      emit = -1, head = first[old];                            // string(old) + first(old): the entry made just below
    } else {
      return FU_TIFF_CODEC_CORRUPT;
    }
    if (next < kLzwTable) {
      prefix[next] = (uint16_t)old, suffix[next] = head, first[next] = first[old];
      length[next] = (uint16_t)(length[old] + 1);
      if (emit < 0) emit = next;
      ++next;
    } else if (emit < 0) {
      return FU_TIFF_CODEC_CORRUPT;
    }
    // write string(emit) into dst[out, out + len), clipped to n_dst, walking the prefixes from its last byte
    int len = length[emit], c = emit;
    const int64_t room = n_dst - out;
    const int keep = (int64_t)len <= room ? len : (int)room;
    for (int k = len - 1; k >= 0; --k) {
      if (k < keep) dst[out + k] = suffix[c];
      c = prefix[c];
    }
    out += keep;
    old = code;
    if (next >= (1 << nbits) - 1 && nbits < 12) ++nbits;
  }
  return out;
}

// PackBits (TIFF 6.0 section 9): a header byte n; 0..127: n + 1 literal bytes follow; -127..-1: the next byte 1 - n times;
// -128: nothing.
int64_t fu_tiff_packbits_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst) {
  if (n_src < 0 || n_dst < 0 || (n_src > 0 && !src) || (n_dst > 0 && !dst)) return FU_TIFF_CODEC_BAD_ARGS;
  int64_t in = 0, out = 0;
  while (in < n_src && out < n_dst) {
    const int n = (int8_t)src[in++];
    if (n >= 0) {
      const int64_t run = n + 1;
      if (in + run > n_src) return FU_TIFF_CODEC_CORRUPT;      // literal bytes cut off
      const int64_t keep = run <= n_dst - out ? run : n_dst - out;
      memcpy(dst + out, src + in, (size_t)keep);
      in += run, out += keep;
    } else if (n != -128) {
      if (in >= n_src) return FU_TIFF_CODEC_CORRUPT;           // the run's byte is missing
      const int64_t run = 1 - n;
      const int64_t keep = run <= n_dst - out ? run : n_dst - out;
      memset(dst + out, src[in++], (size_t)keep);
      out += keep;
    }
  }
  return out;
}

}  // extern "C"
