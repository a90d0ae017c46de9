// What the PNG kernels of csrc/png.hip and their host twins must agree on byte for byte, written once: the five scanline
// predictors, the conversion of a reconstructed pixel into B, G, R (or gray) frame bytes, and Adler-32 in pieces that are
// folded afterwards.  Plain C++; TBN_PNG_HD is `__host__ __device__` only under hipcc (the way tbn_inflate.h is shared).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TBN_PNG_HD __host__ __device__ __forceinline__
#else
#define TBN_PNG_HD inline
#endif

/* status of one image beyond the inflate core's 1..12 (include/tbn_hip.h documents them for callers) */
#define TBN_PNG_ST_ADLER 20     /* inflated completely, Adler-32 differs from the stream's */
#define TBN_PNG_ST_FILTER 21    /* a scanline's filter byte is above 4 (the row is then taken as filter 0) */
#define TBN_PNG_ST_PALETTE 22   /* a palette index at or beyond the entry count (the pixel is then 0, 0, 0) */

namespace tbn_png {

constexpr int kBandRows = 64;     // rows of one band of the unfilter kernel: one per lane
constexpr int kStepTile = 64;     // pixel steps between two staging passes of the unfilter kernel
constexpr int kModeGray = 0, kModeRgb = 1, kModePalette = 2;

// One byte of a scanline: the predictor of filter type `ft` (0..4; anything else predicts 0) from a (left), b (above),
// c (above left), selects instead of branches.  Average: 9-bit sum, floor.  Paeth: ties in the order a, b, c.
TBN_PNG_HD uint32_t predict(uint32_t ft, uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  int pa = p - (int)a, pb = p - (int)b, pc = p - (int)c;
  pa = pa < 0 ? -pa : pa;
  pb = pb < 0 ? -pb : pb;
  pc = pc < 0 ? -pc : pc;
  const uint32_t paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  uint32_t v = 0;
  v = ft == 1 ? a : v;
  v = ft == 2 ? b : v;
  v = ft == 3 ? (a + b) >> 1 : v;
  v = ft == 4 ? paeth : v;
  return v;
}

// A reconstructed pixel (its BPP bytes in the low bytes of `px`, first byte lowest) -> the bytes of its frame pixel, first
// channel lowest: B, G, R for out_channels 3, the gray value for 1.  MODE gray: byte 0 (alpha, byte 1, dropped); rgb: bytes
// 2, 1, 0 (alpha, byte 3, dropped); palette: entry `px` of the B, G, R table, 0 and *bad set when px >= entries.
template <int MODE>
TBN_PNG_HD uint32_t convert(uint32_t px, const uint8_t* palette, uint32_t entries, bool* bad) {
  if (MODE == kModeGray) {
    const uint32_t g = px & 255u;
    return g | (g << 8) | (g << 16);
  }
  if (MODE == kModeRgb) return ((px >> 16) & 255u) | (px & 0xFF00u) | ((px & 255u) << 16);
  const uint32_t i = px & 255u;
  if (i >= entries) {
    *bad = true;
    return 0;
  }
  return (uint32_t)palette[3 * i] | ((uint32_t)palette[3 * i + 1] << 8) | ((uint32_t)palette[3 * i + 2] << 16);
}

// ---- Adler-32 (RFC 1950) in pieces: a piece is (a, b) of its bytes started from a = 1, b = 0, and its length ----------
constexpr uint32_t kAdlerMod = 65521;
constexpr uint32_t kAdlerPieces = 256;    // pieces per image: the threads of the Adler kernel
TBN_PNG_HD uint32_t adler_piece_len(uint32_t n) { return (n + kAdlerPieces - 1) / kAdlerPieces; }

TBN_PNG_HD void adler_piece(const uint8_t* data, uint32_t begin, uint32_t end, uint32_t* a_out, uint32_t* b_out) {
  uint32_t a = 1, b = 0;
  for (uint32_t i = begin; i < end;) {
    const uint32_t stop = end - i > 4096u ? i + 4096u : end;      // below zlib's NMAX of 5552 bytes: b stays under 2^32
    for (; i < stop; ++i) {
      a += data[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
  }
  *a_out = a;
  *b_out = b;
}
// (a, b) of X || Y from X's and Y's, Y being `len` bytes long
TBN_PNG_HD void adler_fold(uint32_t* a, uint32_t* b, uint32_t ya, uint32_t yb, uint32_t len) {
  const uint64_t l = len % kAdlerMod;
  const uint64_t nb = (uint64_t)*b + yb + l * ((*a + kAdlerMod - 1u) % kAdlerMod);
  *b = (uint32_t)(nb % kAdlerMod);
  *a = (*a + ya + kAdlerMod - 1u) % kAdlerMod;
}
// the fold of the kAdlerPieces pieces of n bytes, piece k being bytes [k * piece, (k + 1) * piece) clamped to n
TBN_PNG_HD uint32_t adler_fold_all(const uint32_t* pa, const uint32_t* pb, uint32_t n) {
  const uint32_t piece = adler_piece_len(n);
  uint32_t a = 1, b = 0;
  for (uint32_t k = 0; k < kAdlerPieces; ++k) {
    const uint64_t lo = (uint64_t)k * piece, hi = lo + piece;
    const uint32_t len = (uint32_t)((hi < n ? hi : n) - (lo < n ? lo : n));
    adler_fold(&a, &b, pa[k], pb[k], len);
  }
  return (b << 16) | a;
}

}  // namespace tbn_png
