// Host half of the PNG decoder: the container, and (at the end) the host twins of the device half.  Signature, chunk walk,
// CRC-32 of the critical chunks, IHDR / PLTE, and the
// Plain C++, nothing from HIP, no global state: every function works on the caller's bytes and buffers, so any number of
// threads may run at once.  The bytes come from disk and are not trusted: every read is checked against `size`, every
// write against what the caller's geometry declared, and a refusal says why in `err`.
//
// Replaces the container half of cv2.imread in reference core/dataset/dataset.py:305 (RGB) and :360, :365 (Flow) for
// frames extracted as PNG (data.rgb.file_ext / data.flow.file_ext: "png").  Supported: bit depth 8, non-interlaced, colour
// types 0 (gray), 2 (RGB), 3 (palette), 4 (gray + alpha), 6 (RGBA).  Ancillary chunks (tRNS and gAMA among them) are
// skipped unread, as cv2.imread at its defaults ignores them.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>

#include "tbn_inflate.h"
#include "tbn_png_core.h"

#ifndef TBN_PNG_GEOMETRY_DEFINED
#define TBN_PNG_GEOMETRY_DEFINED
typedef struct tbn_png_geometry {
  int width, height;        /* image size in pixels */
  int colour_type;          /* 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGBA */
  int bpp;                  /* bytes per pixel in the scanlines: 1, 3, 1, 2, 4 */
  int palette_entries;      /* entries of PLTE (colour type 3; else 0).  Per file: not compared */
  int reserved;
  size_t raw_bytes;         /* the inflated scanlines: height * (1 + width * bpp) */
  size_t idat_bytes;        /* sum of the IDAT payloads: the zlib stream.  Per file: not compared */
} tbn_png_geometry;
#endif

#define TBN_PNG_OK 0
#define TBN_PNG_ERR_DATA (-1)          /* bad argument or corrupt / truncated file (TBN_ERR_ARG) */
#define TBN_PNG_ERR_UNSUPPORTED (-3)   /* a well-formed file of a kind this decoder does not take (TBN_ERR_UNSUPPORTED) */

/* the longest scanline (width * bpp bytes, without the filter byte) the unfilter kernel keeps on chip: 4096 RGBA pixels */
#define TBN_PNG_MAX_ROW_BYTES 16384
/* one image's palette slot: 256 x 3 bytes B, G, R (unused entries zero), the entry count as a little-endian uint32 at
 * byte 768, zeros up to 1024 */
#define TBN_PNG_PALETTE_BYTES 1024
/* tbn_png_gather writes the zlib stream from byte 2 of `zstream`, so that the deflate data behind the 2-byte zlib header
 * starts at byte 4: tbn_inflate_member.in_off and tbn_png_image.in_off must be multiples of 4 */
#define TBN_PNG_ZSTREAM_LEAD 2

namespace tbn_png {

#define TBN_PNG_FAIL(code, ...)                            \
  do {                                                     \
    if (err && errlen) snprintf(err, errlen, __VA_ARGS__); \
    return code;                                           \
  } while (0)

static inline uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// the CRC-32 of PNG (the zip polynomial, reflected), bitwise-free: a 256-entry table built on the stack of the caller
struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t i = 0; i < 256; ++i) {
      uint32_t c = i;
      for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
      t[i] = c;
    }
  }
  uint32_t run(const uint8_t* p, size_t n) const {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = t[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
    return c ^ 0xFFFFFFFFu;
  }
};

static const uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};

static inline bool is_type(const uint8_t* p, const char* name) { return memcmp(p, name, 4) == 0; }

// Walks the whole file.  `visit_idat(payload, len)` is called for every IDAT in order when non-null (gather), and
// `palette` receives PLTE's bytes (r, g, b as stored) when non-null.  `header_only`: the walk ends, successfully, behind IHDR.
template <class Visit>
static inline int walk(const uint8_t* d, size_t size, tbn_png_geometry* g, const uint8_t** plte, Visit&& visit_idat, char* err,
                       size_t errlen, bool header_only = false) {
  if (!d || !g) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: null argument");
  memset(g, 0, sizeof(*g));
  if (size < 8 || memcmp(d, kSignature, 8) != 0) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: no PNG signature (not a PNG file, %zu bytes)", size);
  const CrcTable crc;
  size_t pos = 8;
  bool first = true, have_plte = false, have_idat = false, idat_closed = false;
  for (;;) {
    if (pos + 8 > size) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: stream ends early at byte %zu, before IEND", size);
    const size_t len = be32(d + pos);
    const uint8_t* type = d + pos + 4;
    // length + type + payload + CRC
    if (len > 0x7FFFFFFFu || size - pos - 8 < 4 || len > size - pos - 12)
      TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: stream ends early: chunk %.4s at byte %zu declares %zu bytes, %zu remain", (const char*)type,
                   pos, len, size - pos - 8);
    const uint8_t* payload = d + pos + 8;
    const bool critical = is_type(type, "IHDR") || is_type(type, "PLTE") || is_type(type, "IDAT") || is_type(type, "IEND");
    if (first && !is_type(type, "IHDR")) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: first chunk is %.4s, not IHDR", (const char*)type);
    if (critical && crc.run(type, len + 4) != be32(payload + len))
      TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: CRC-32 mismatch in chunk %.4s at byte %zu", (const char*)type, pos);
    if (!critical && !(type[0] & 0x20))
      TBN_PNG_FAIL(TBN_PNG_ERR_UNSUPPORTED, "png: unknown critical chunk %.4s at byte %zu is not supported", (const char*)type, pos);
    if (have_idat && !is_type(type, "IDAT")) idat_closed = true;
    if (is_type(type, "IHDR")) {
      if (!first) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: second IHDR at byte %zu", pos);
      if (len != 13) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: IHDR is %zu bytes long, not 13", len);
      const uint32_t w = be32(payload), h = be32(payload + 4);
      const int depth = payload[8], ct = payload[9], comp = payload[10], filt = payload[11], lace = payload[12];
      if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: invalid image size %ux%u", w, h);
      if (ct != 0 && ct != 2 && ct != 3 && ct != 4 && ct != 6) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: invalid colour type %d", ct);
      if (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: invalid bit depth %d", depth);
      if (comp != 0 || filt != 0) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: invalid compression / filter method %d / %d", comp, filt);
      if (lace > 1) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: invalid interlace method %d", lace);
      if (depth != 8) TBN_PNG_FAIL(TBN_PNG_ERR_UNSUPPORTED, "png: bit depth %d is not supported (8 only)", depth);
      if (lace == 1) TBN_PNG_FAIL(TBN_PNG_ERR_UNSUPPORTED, "png: Adam7 interlace is not supported");
      const int bpp = ct == 0 ? 1 : ct == 2 ? 3 : ct == 3 ? 1 : ct == 4 ? 2 : 4;
      if ((uint64_t)w * bpp > TBN_PNG_MAX_ROW_BYTES)
        TBN_PNG_FAIL(TBN_PNG_ERR_UNSUPPORTED, "png: a scanline of %u pixels x %d bytes is not supported (at most %d bytes)", w, bpp,
                     TBN_PNG_MAX_ROW_BYTES);
      const uint64_t raw = (uint64_t)h * (1u + (uint64_t)w * bpp);
      if (raw >= (1ull << 31)) TBN_PNG_FAIL(TBN_PNG_ERR_UNSUPPORTED, "png: %ux%u is not supported (%llu scanline bytes, below 2^31 only)", w, h, (unsigned long long)raw);
      g->width = (int)w; g->height = (int)h; g->colour_type = ct; g->bpp = bpp;
      g->raw_bytes = (size_t)raw;
      if (header_only) return TBN_PNG_OK;
    } else if (is_type(type, "PLTE")) {
      if (have_plte) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: second PLTE at byte %zu", pos);
      if (have_idat) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: PLTE at byte %zu follows IDAT", pos);
      if (len == 0 || len % 3 != 0 || len > 768) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: PLTE is %zu bytes long, not 3 x (1..256)", len);
      have_plte = true;
      if (g->colour_type == 3) {
        g->palette_entries = (int)(len / 3);
        if (plte) *plte = payload;
      }
    } else if (is_type(type, "IDAT")) {
      if (idat_closed) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: IDAT at byte %zu is not consecutive with the IDAT chunks before it", pos);
      if (g->colour_type == 3 && !have_plte) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: colour type 3 without PLTE before IDAT");
      have_idat = true;
      g->idat_bytes += len;
      const int rc = visit_idat(payload, len);
      if (rc) return rc;
    } else if (is_type(type, "IEND")) {
      if (!have_idat) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: IEND without any IDAT");
      if (g->idat_bytes < 6) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: stream ends early: the zlib stream is %zu bytes long", g->idat_bytes);
      return TBN_PNG_OK;
    }
    first = false;
    pos += 12 + len;
  }
}

static inline int parse(const uint8_t* d, size_t size, tbn_png_geometry* g, char* err, size_t errlen) {
  return walk(d, size, g, nullptr, [](const uint8_t*, size_t) { return 0; }, err, errlen);
}

// what the first 33 bytes say (signature + IHDR with its CRC): the size of a frame whose file is not read further.
// Fills width, height, colour_type, bpp, raw_bytes; the IHDR checks and refusals are parse()'s own.
static inline int parse_header(const uint8_t* d, size_t size, tbn_png_geometry* g, char* err, size_t errlen) {
  if (d && size >= 8 && size < 33 && memcmp(d, kSignature, 8) == 0)
    TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: stream ends early at byte %zu, inside IHDR", size);
  return walk(d, size < 33 ? size : 33, g, nullptr, [](const uint8_t*, size_t) { return 0; }, err, errlen, true);
}

// Concatenates the IDAT payloads into zstream[TBN_PNG_ZSTREAM_LEAD, TBN_PNG_ZSTREAM_LEAD + idat_bytes) (zstream[0, 2) = 0;
// capacity: gather_bytes(expect->idat_bytes)), checks the zlib header, and says where the raw deflate data lies:
// [*deflate_begin, *deflate_end) of zstream, *deflate_begin == 4; *adler is the stream's trailing Adler-32.  palette (may be
// null unless colour type 3): TBN_PNG_PALETTE_BYTES.  Refuses a file whose geometry or IDAT byte count differs from `expect`.
static inline size_t gather_bytes(size_t idat_bytes) { return (TBN_PNG_ZSTREAM_LEAD + idat_bytes + 3) / 4 * 4 + 4; }

static inline int gather(const uint8_t* d, size_t size, const tbn_png_geometry* expect, uint8_t* zstream, uint8_t* palette,
                         uint32_t* deflate_begin, uint32_t* deflate_end, uint32_t* adler, char* err, size_t errlen) {
  if (!expect || !zstream || !deflate_begin || !deflate_end || !adler) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: null argument");
  tbn_png_geometry g;
  const uint8_t* plte = nullptr;
  const size_t cap = expect->idat_bytes;
  size_t at = 0;
  memset(zstream, 0, gather_bytes(cap));
  const int rc = walk(d, size, &g, &plte,
                      [&](const uint8_t* p, size_t n) {
                        if (n > cap - at) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: the IDAT chunks hold more than the %zu bytes expected", cap);
                        if (n) memcpy(zstream + TBN_PNG_ZSTREAM_LEAD + at, p, n);
                        at += n;
                        return 0;
                      },
                      err, errlen);
  if (rc) return rc;
  if (g.width != expect->width || g.height != expect->height || g.colour_type != expect->colour_type)
    TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: image is %dx%d colour type %d, expected %dx%d colour type %d", g.width, g.height, g.colour_type,
                 expect->width, expect->height, expect->colour_type);
  if (at != cap) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: the IDAT chunks hold %zu bytes, expected %zu", at, cap);
  const uint8_t* z = zstream + TBN_PNG_ZSTREAM_LEAD;
  const int cmf = z[0], flg = z[1];
  if ((cmf & 15) != 8) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: zlib header: compression method %d is not 8 (deflate)", cmf & 15);
  if ((cmf >> 4) > 7) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: zlib header: window of 2^%d bytes is above 32 K", (cmf >> 4) + 8);
  if (flg & 0x20) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: zlib header: a preset dictionary is not allowed");
  if ((cmf * 256 + flg) % 31 != 0) TBN_PNG_FAIL(TBN_PNG_ERR_DATA, "png: zlib header: FCHECK fails (0x%02X%02X)", cmf, flg);
  *deflate_begin = TBN_PNG_ZSTREAM_LEAD + 2;
  *deflate_end = (uint32_t)(TBN_PNG_ZSTREAM_LEAD + cap - 4);
  *adler = be32(z + cap - 4);
  if (palette) {
    memset(palette, 0, TBN_PNG_PALETTE_BYTES);
    if (g.colour_type == 3) {
      for (int i = 0; i < g.palette_entries; ++i) {
        palette[3 * i + 0] = plte[3 * i + 2];
        palette[3 * i + 1] = plte[3 * i + 1];
        palette[3 * i + 2] = plte[3 * i + 0];
      }
      palette[768] = (uint8_t)(g.palette_entries & 255);
      palette[769] = (uint8_t)(g.palette_entries >> 8);
    }
  }
  return TBN_PNG_OK;
}

// ---- the host twins of the device half (csrc/png.hip): the same predictor, conversion, decoder core and Adler pieces,
// serially.  tbn_png_unfilter_host / tbn_png_decode_host and scripts/png_check.cpp run them. --------------------------------
template <class F>
int dispatch_mode(int colour_type, F&& f) {   // f(bpp tag, mode tag)
  switch (colour_type) {
    case 0: return f(std::integral_constant<int, 1>(), std::integral_constant<int, kModeGray>());
    case 2: return f(std::integral_constant<int, 3>(), std::integral_constant<int, kModeRgb>());
    case 3: return f(std::integral_constant<int, 1>(), std::integral_constant<int, kModePalette>());
    case 4: return f(std::integral_constant<int, 2>(), std::integral_constant<int, kModeGray>());
    default: return f(std::integral_constant<int, 4>(), std::integral_constant<int, kModeRgb>());
  }
}

template <int BPP, int MODE>
static inline int unfilter_image_host(const uint8_t* raw, const uint8_t* palette, int W, int H, int oc, uint8_t* frame) {
  uint8_t rows[2][TBN_PNG_MAX_ROW_BYTES];
  memset(rows[0], 0, (size_t)W * BPP);
  uint32_t entries = 0;
  if (MODE == kModePalette) {
    entries = (uint32_t)palette[768] | ((uint32_t)palette[769] << 8);
    entries = entries > 256u ? 256u : entries;
  }
  bool bad_filter = false, bad_index = false;
  const size_t stride = 1u + (size_t)W * BPP;
  for (int y = 0; y < H; ++y) {
    const uint8_t* line = raw + (size_t)y * stride;
    const uint8_t* above = rows[y & 1];
    uint8_t* now = rows[(y + 1) & 1];
    uint32_t ft = line[0];
    if (ft > 4u) {
      bad_filter = true;
      ft = 0;
    }
    for (int x = 0; x < W; ++x) {
      uint32_t px = 0;
      for (int k = 0; k < BPP; ++k) {
        const uint32_t a = x > 0 ? now[(x - 1) * BPP + k] : 0u, b = above[x * BPP + k], c = x > 0 ? above[(x - 1) * BPP + k] : 0u;
        now[x * BPP + k] = (uint8_t)(line[1 + x * BPP + k] + predict(ft, a, b, c));
        px |= (uint32_t)now[x * BPP + k] << (8 * k);
      }
      const uint32_t o = convert<MODE>(px, palette, entries, &bad_index);
      for (int k = 0; k < oc; ++k) frame[((size_t)y * W + x) * oc + k] = (uint8_t)(o >> (8 * k));
    }
  }
  return bad_filter ? TBN_PNG_ST_FILTER : (bad_index ? TBN_PNG_ST_PALETTE : 0);
}

static inline uint32_t adler_host(const uint8_t* data, uint32_t n) {     // in kAdlerPieces pieces, as png_adler_kernel computes it
  uint32_t pa[kAdlerPieces], pb[kAdlerPieces];
  const uint32_t piece = adler_piece_len(n);
  for (uint32_t t = 0; t < kAdlerPieces; ++t) {
    const uint64_t lo = (uint64_t)t * piece, hi = lo + piece;
    adler_piece(data, (uint32_t)(lo < n ? lo : n), (uint32_t)(hi < n ? hi : n), &pa[t], &pb[t]);
  }
  return adler_fold_all(pa, pb, n);
}

// raw (height * (1 + width * bpp) scanline bytes) -> frame (height, width, oc); -> 0, 21 or 22
static inline int unfilter_host(int colour_type, const uint8_t* raw, const uint8_t* palette, int W, int H, int oc, uint8_t* frame) {
  return dispatch_mode(colour_type, [&](auto bpp, auto mode) {
    return unfilter_image_host<decltype(bpp)::value, decltype(mode)::value>(raw, palette, W, H, oc, frame);
  });
}

// One image as tbn_png_decode treats it: `in_len` bytes of raw deflate data -> raw[raw_bytes] (exactly), the Adler-32 of
// those bytes against `adler`, then the unfilter -> status 0, 1..9 (the core's), 20, 21 or 22; *produced: bytes inflated.
static inline int decode_image_host(const uint8_t* in, uint32_t in_len, uint32_t adler, const uint8_t* palette, int colour_type, int W,
                                    int H, int oc, uint8_t* raw, uint8_t* frame, uint32_t* produced) {
  const int bpp = colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 3 ? 1 : colour_type == 4 ? 2 : 4;
  const uint32_t raw_bytes = (uint32_t)((size_t)H * (1u + (size_t)W * bpp));
  tbn_inflate::Tables t;
  tbn_inflate::HostIO io{in, in_len, raw};
  const int st = tbn_inflate::inflate_stream(io, t, in_len, raw_bytes, produced);
  if (st != TBN_INF_OK) return st;
  if (adler_host(raw, raw_bytes) != adler) return TBN_PNG_ST_ADLER;
  return unfilter_host(colour_type, raw, palette, W, H, oc, frame);
}

}  // namespace tbn_png
