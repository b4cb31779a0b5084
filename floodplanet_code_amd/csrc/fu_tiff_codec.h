// TIFF entropy decoders for the host: LZW (compression 5) and PackBits (32773).  Plain C++, no HIP include and no HIP
// call: the translation unit compiles with any host compiler, and calling it (from a DataLoader worker, say) never opens
// the GPU.  Declared again, with their documentation, in include/floodunet.h; datasets/geotiff.py holds the Python
// statements (lzw_decode_host, packbits_decode_host) they are tested against.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// negative returns of both decoders
#define FU_TIFF_CODEC_BAD_ARGS (-1)  /* a null buffer with a non-zero size, or a negative size */
#define FU_TIFF_CODEC_CORRUPT (-2)   /* a code that cannot occur, a run or literal cut off by the end of the input */
#define FU_TIFF_CODEC_OLD_LZW (-3)   /* the LSB-first LZW of TIFF 4.0 writers */

// Both read src[0, n_src) only, write dst[0, n_dst) only, stop at n_dst, and return the bytes written (which is less than
// n_dst when the stream ends first) or one of the codes above.
int64_t fu_tiff_lzw_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst);
int64_t fu_tiff_packbits_decode(const uint8_t* src, int64_t n_src, uint8_t* dst, int64_t n_dst);

#ifdef __cplusplus
}
#endif
