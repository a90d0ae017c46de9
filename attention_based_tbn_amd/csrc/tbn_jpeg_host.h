// Host stage of the baseline JPEG decoder: marker parsing and Huffman decoding, the serial part that stays on the CPU
// (csrc/jpeg.hip has the device stage: dequantisation, IDCT, upsampling, colour).  Plain C++, nothing from HIP, no
// global state: every function works on the caller's bytes and buffers, so any number of threads may decode at once.
// The bytes come from disk and are not trusted: every read is checked against `size`, every write against the extents
// the header itself declared, and a refusal says why in `err`.
//
// Replaces the entropy-decoding half of cv2.imread in reference core/dataset/dataset.py:303-305 (RGB) and :355-370
// (Flow).  Supported: SOF0, 8-bit, Huffman; 1 component, or 3 components with luma 1x1 / 2x1 / 2x2 and chroma 1x1;
// one interleaved scan; restart intervals, 0xFF00 stuffing, fill bytes in front of markers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#ifndef TBN_JPEG_GEOMETRY_DEFINED
#define TBN_JPEG_GEOMETRY_DEFINED
typedef struct tbn_jpeg_geometry {
  int width, height;          /* true image size in pixels */
  int components;             /* 1 (gray) or 3 (YCbCr) */
  int hsamp[3], vsamp[3];     /* sampling factors per component (a 1-component file: 1 x 1) */
  int blocks_w[3], blocks_h[3]; /* 8x8-block extents of each component plane, padded to whole MCUs */
  int restart_interval;       /* MCUs between restart markers, 0: none (informational, not compared) */
  size_t coef_count;          /* int16 coefficients of one image: 64 * sum(blocks_w * blocks_h) */
} tbn_jpeg_geometry;
#endif

#define TBN_JPEG_OK 0
#define TBN_JPEG_ERR_DATA (-1)          /* bad argument or corrupt / truncated stream (TBN_ERR_ARG) */
#define TBN_JPEG_ERR_UNSUPPORTED (-3)   /* a well-formed file of a kind this decoder does not take (TBN_ERR_UNSUPPORTED) */

namespace tbn_jpeg {

constexpr int kLookBits = 9;   // look-ahead width: codes up to 9 bits decode with one table read, as libjpeg's HUFF_LOOKAHEAD + 1

struct HuffTable {
  bool defined;
  uint8_t bits[17];            // bits[l]: number of codes of length l
  uint8_t vals[256];
  int nvals;
  int32_t maxcode[18];         // largest code of length l, -1 if none; [17] is a sentinel
  int32_t valoff[17];          // vals index of the first code of length l minus that code
  uint16_t look[1 << kLookBits];   // (length << 8) | symbol for codes of <= kLookBits bits, 0 otherwise
};

struct Header {
  tbn_jpeg_geometry geo;
  uint16_t quant[4][64];       // zigzag order, as stored in the file
  bool quant_defined[4];
  HuffTable dc[4], ac[4];
  int comp_id[3], comp_tq[3], comp_td[3], comp_ta[3];
  bool have_sof, have_sos;
  int mcus_x, mcus_y;
  size_t scan_pos;             // first byte of the entropy-coded data
};

static const uint8_t kZigzagToNatural[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define TBN_JPEG_FAIL(code, ...)              \
  do {                                        \
    if (err && errlen) snprintf(err, errlen, __VA_ARGS__); \
    return code;                              \
  } while (0)

static inline int build_huff(HuffTable* t, char* err, size_t errlen, const char* what, int id) {
  // JPEG Annex C: codes of each length are consecutive, starting at twice the end of the previous length
  int32_t code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    t->valoff[l] = k - code;
    if (t->bits[l]) {
      k += t->bits[l];
      code += t->bits[l];
      if (code > (1 << l)) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: %s Huffman table %d is over-subscribed at length %d", what, id, l);
      t->maxcode[l] = code - 1;
    } else {
      t->maxcode[l] = -1;
    }
    code <<= 1;
  }
  t->maxcode[17] = 0x7fffffff;
  memset(t->look, 0, sizeof(t->look));
  code = 0;
  k = 0;
  for (int l = 1; l <= kLookBits; ++l) {
    for (int i = 0; i < t->bits[l]; ++i, ++k, ++code) {
      const int first = code << (kLookBits - l), count = 1 << (kLookBits - l);
      for (int j = 0; j < count; ++j) t->look[first + j] = (uint16_t)((l << 8) | t->vals[k]);
    }
    code <<= 1;
  }
  return TBN_JPEG_OK;
}

static inline int parse_header(const uint8_t* d, size_t size, Header* h, char* err, size_t errlen) {
  if (!d || !h) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: null argument");
  memset(h, 0, sizeof(*h));
  if (size < 2 || d[0] != 0xFF || d[1] != 0xD8) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: no SOI marker (not a JPEG stream, %zu bytes)", size);
  size_t pos = 2;
  for (;;) {
    // a marker: 0xFF, any number of 0xFF fill bytes, the code
    if (pos >= size) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early at byte %zu, before the scan", pos);
    if (d[pos] != 0xFF) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: byte 0x%02X at %zu where a marker is expected", d[pos], pos);
    while (pos < size && d[pos] == 0xFF) ++pos;
    if (pos >= size) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early at byte %zu, inside a marker", pos);
    const int m = d[pos++];
    if (m == 0xD9) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: EOI before any scan (stream ends early)");
    if (m == 0x00 || m == 0x01 || m == 0xD8 || (m >= 0xD0 && m <= 0xD7))
      TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: unexpected marker 0xFF%02X at byte %zu", m, pos - 2);
    if (pos + 2 > size) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early at byte %zu, inside segment 0xFF%02X", pos, m);
    const size_t len = ((size_t)d[pos] << 8) | d[pos + 1];
    if (len < 2 || pos + len > size)
      TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early: segment 0xFF%02X at byte %zu declares %zu bytes, %zu remain", m, pos - 2, len, size - pos);
    const uint8_t* s = d + pos + 2;
    const size_t n = len - 2;
    pos += len;
    if (m == 0xC0) {
      if (h->have_sof) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: second SOF0");
      if (n < 6) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: SOF0 segment too short");
      const int prec = s[0], height = (s[1] << 8) | s[2], width = (s[3] << 8) | s[4], nc = s[5];
      if (prec != 8) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: %d-bit sample precision is not supported (8-bit only)", prec);
      if (nc == 4) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: 4 components (CMYK / YCCK) are not supported");
      if (nc != 1 && nc != 3) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: %d components are not supported (1 or 3)", nc);
      if (width == 0 || height == 0) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: empty image %dx%d (DNL-defined height is not supported)", width, height);
      if (n != (size_t)(6 + 3 * nc)) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: SOF0 segment length does not match %d components", nc);
      tbn_jpeg_geometry* g = &h->geo;
      g->width = width; g->height = height; g->components = nc;
      for (int c = 0; c < nc; ++c) {
        h->comp_id[c] = s[6 + 3 * c];
        g->hsamp[c] = s[7 + 3 * c] >> 4;
        g->vsamp[c] = s[7 + 3 * c] & 15;
        h->comp_tq[c] = s[8 + 3 * c];
        if (h->comp_tq[c] > 3) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: component %d names quantisation table %d", c, h->comp_tq[c]);
      }
      if (nc == 1) {
        g->hsamp[0] = g->vsamp[0] = 1;     // a single-component scan is never interleaved: the factors have no effect
      } else {
        const bool luma_ok = (g->hsamp[0] == 1 && g->vsamp[0] == 1) || (g->hsamp[0] == 2 && g->vsamp[0] == 1) ||
                             (g->hsamp[0] == 2 && g->vsamp[0] == 2);
        if (!luma_ok || g->hsamp[1] != 1 || g->vsamp[1] != 1 || g->hsamp[2] != 1 || g->vsamp[2] != 1)
          TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: sampling %dx%d,%dx%d,%dx%d is not supported (4:4:4, 4:2:2 and 4:2:0 only)",
                        g->hsamp[0], g->vsamp[0], g->hsamp[1], g->vsamp[1], g->hsamp[2], g->vsamp[2]);
      }
      h->mcus_x = (width + 8 * g->hsamp[0] - 1) / (8 * g->hsamp[0]);
      h->mcus_y = (height + 8 * g->vsamp[0] - 1) / (8 * g->vsamp[0]);
      g->coef_count = 0;
      for (int c = 0; c < nc; ++c) {
        g->blocks_w[c] = h->mcus_x * g->hsamp[c];
        g->blocks_h[c] = h->mcus_y * g->vsamp[c];
        g->coef_count += (size_t)64 * g->blocks_w[c] * g->blocks_h[c];
      }
      h->have_sof = true;
    } else if (m == 0xC2) {
      TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: progressive JPEG (SOF2) is not supported");
    } else if (m == 0xCC || (m >= 0xC9 && m <= 0xCF && m != 0xCC)) {
      TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: arithmetic coding (marker 0xFF%02X) is not supported", m);
    } else if (m == 0xC1 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || m == 0xC8) {
      TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: frame type SOF%d is not supported (baseline SOF0 only)", m - 0xC0);
    } else if (m == 0xDB) {
      size_t i = 0;
      while (i < n) {
        const int pq = s[i] >> 4, tq = s[i] & 15;
        if (pq > 1 || tq > 3) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: bad quantisation table header 0x%02X", s[i]);
        const size_t need = 1 + (pq ? 128 : 64);
        if (i + need > n) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: DQT segment too short for table %d", tq);
        for (int k = 0; k < 64; ++k)
          h->quant[tq][k] = pq ? (uint16_t)((s[i + 1 + 2 * k] << 8) | s[i + 2 + 2 * k]) : s[i + 1 + k];
        h->quant_defined[tq] = true;
        i += need;
      }
    } else if (m == 0xC4) {
      size_t i = 0;
      while (i < n) {
        const int tc = s[i] >> 4, th = s[i] & 15;
        if (tc > 1 || th > 3) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: bad Huffman table header 0x%02X", s[i]);
        if (i + 17 > n) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: DHT segment too short");
        HuffTable* t = tc ? &h->ac[th] : &h->dc[th];
        int total = 0;
        t->bits[0] = 0;
        for (int l = 1; l <= 16; ++l) {
          t->bits[l] = s[i + l];
          total += s[i + l];
        }
        if (total > 256 || i + 17 + (size_t)total > n) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: DHT segment too short for %d symbols", total);
        memset(t->vals, 0, sizeof(t->vals));
        memcpy(t->vals, s + i + 17, (size_t)total);
        t->nvals = total;
        if (!tc)
          for (int k = 0; k < total; ++k)
            if (t->vals[k] > 15) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: DC Huffman table %d has category %d", th, t->vals[k]);
        t->defined = false;
        const int rc = build_huff(t, err, errlen, tc ? "AC" : "DC", th);
        if (rc) return rc;
        t->defined = true;
        i += 17 + (size_t)total;
      }
    } else if (m == 0xDD) {
      if (n != 2) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: bad DRI segment");
      h->geo.restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xDA) {
      if (!h->have_sof) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: SOS before SOF0");
      const int nc = h->geo.components;
      if (n < 1) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: SOS segment too short");
      const int ns = s[0];
      if (ns < 1 || ns > 4 || n != (size_t)(4 + 2 * ns)) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: bad SOS segment");
      if (ns != nc)
        TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: more than one scan (this scan has %d of %d components) is not supported", ns, nc);
      for (int c = 0; c < nc; ++c) {
        if (s[1 + 2 * c] != h->comp_id[c]) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: scan component %d is not frame component %d", c, c);
        h->comp_td[c] = s[2 + 2 * c] >> 4;
        h->comp_ta[c] = s[2 + 2 * c] & 15;
        if (h->comp_td[c] > 3 || h->comp_ta[c] > 3) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: bad Huffman table selector in SOS");
        if (!h->dc[h->comp_td[c]].defined) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: missing DC Huffman table %d (component %d)", h->comp_td[c], c);
        if (!h->ac[h->comp_ta[c]].defined) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: missing AC Huffman table %d (component %d)", h->comp_ta[c], c);
        if (!h->quant_defined[h->comp_tq[c]]) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: missing quantisation table %d (component %d)", h->comp_tq[c], c);
      }
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
        TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: spectral selection / successive approximation (progressive scan) is not supported");
      h->have_sos = true;
      h->scan_pos = pos;
      return TBN_JPEG_OK;
    } else if ((m >= 0xE0 && m <= 0xEF) || m == 0xFE) {
      // APPn / COM: skipped
    } else {
      TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: marker 0xFF%02X is not supported", m);
    }
  }
}

// MSB-first bit reader over the entropy-coded segment.  `nbits` counts REAL bits only: a peek past them is padded with
// zeros, and consuming more than there are is the "stream ends early or hits a marker" refusal.
struct BitReader {
  const uint8_t* d;
  size_t size, pos;
  uint64_t acc;
  int nbits;
  bool stopped;      // pos is at a marker's 0xFF (or at the end): no more data bytes
};

static inline void br_fill(BitReader* b) {
  while (b->nbits <= 56 && !b->stopped) {
    if (b->pos >= b->size) { b->stopped = true; break; }
    const uint8_t c = b->d[b->pos];
    if (c != 0xFF) {
      b->acc = (b->acc << 8) | c;
      b->nbits += 8;
      ++b->pos;
      continue;
    }
    size_t q = b->pos + 1;                     // 0xFF, fill 0xFFs, then 0x00 (a stuffed data byte 0xFF) or a marker code
    while (q < b->size && b->d[q] == 0xFF) ++q;
    if (q < b->size && b->d[q] == 0x00) {
      b->acc = (b->acc << 8) | 0xFF;
      b->nbits += 8;
      b->pos = q + 1;
    } else {
      b->stopped = true;
    }
  }
}

static inline uint32_t br_peek(BitReader* b, int k) {   // k <= 16
  if (b->nbits < k) br_fill(b);
  if (b->nbits >= k) return (uint32_t)(b->acc >> (b->nbits - k)) & ((1u << k) - 1);
  return (uint32_t)(b->acc << (k - b->nbits)) & ((1u << k) - 1);
}

static inline bool br_skip(BitReader* b, int k) {
  if (k > b->nbits) return false;
  b->nbits -= k;
  return true;
}

// returns the symbol, -1: ran out of data, -2: no such code
static inline int huff_decode(BitReader* b, const HuffTable* t) {
  const uint32_t look = br_peek(b, kLookBits);
  const uint16_t e = t->look[look];
  if (e) return br_skip(b, e >> 8) ? (e & 255) : -1;
  const uint32_t w = br_peek(b, 16);
  for (int l = kLookBits + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(w >> (16 - l));
    if (code <= t->maxcode[l]) {
      if (!br_skip(b, l)) return -1;
      const int idx = t->valoff[l] + code;
      return (idx >= 0 && idx < t->nvals) ? t->vals[idx] : -2;
    }
  }
  return b->nbits < 16 && b->stopped ? -1 : -2;
}

// reads the marker the reader stopped at; -1 if the stream ends or data bytes are left in front of it
static inline int br_marker(BitReader* b) {
  b->nbits = 0;
  b->acc = 0;
  size_t p = b->pos;
  if (p >= b->size || b->d[p] != 0xFF) return -1;
  while (p < b->size && b->d[p] == 0xFF) ++p;
  if (p >= b->size || b->d[p] == 0x00) return -1;
  b->pos = p + 1;
  b->stopped = false;
  return b->d[p];
}

// one 8x8 block; 0, or -1: out of data, -2: no such code, -3: DC leaves int16, -4: AC run leaves the block
static inline int decode_block(BitReader* b, const HuffTable* dct, const HuffTable* act, int* pred, int16_t* blk) {
  memset(blk, 0, 64 * sizeof(int16_t));
  int s = huff_decode(b, dct);
  if (s < 0) return s;
  if (s) {
    const uint32_t r = br_peek(b, s);
    if (!br_skip(b, s)) return -1;
    *pred += r < (1u << (s - 1)) ? (int)r - (1 << s) + 1 : (int)r;     // |diff| < 2^15, |pred| <= 2^15: no overflow
  }
  if (*pred < -32768 || *pred > 32767) return -3;
  blk[0] = (int16_t)*pred;
  for (int k = 1; k < 64;) {
    s = huff_decode(b, act);
    if (s < 0) return s;
    const int run = s >> 4, cat = s & 15;
    if (cat == 0) {
      if (run != 15) break;        // EOB
      k += 16;                     // ZRL
      continue;
    }
    k += run;
    if (k > 63) return -4;
    const uint32_t r = br_peek(b, cat);
    if (!br_skip(b, cat)) return -1;
    // cat <= 15: |value| <= 32767 fits int16
    blk[kZigzagToNatural[k]] = (int16_t)(r < (1u << (cat - 1)) ? (int)r - (1 << cat) + 1 : (int)r);
    ++k;
  }
  return 0;
}

static inline bool same_geometry(const tbn_jpeg_geometry* a, const tbn_jpeg_geometry* b) {
  if (a->width != b->width || a->height != b->height || a->components != b->components) return false;
  for (int c = 0; c < a->components; ++c)
    if (a->hsamp[c] != b->hsamp[c] || a->vsamp[c] != b->vsamp[c]) return false;
  return true;
}

}  // namespace tbn_jpeg

// Geometry of one baseline JPEG: everything a caller needs to size the coefficient buffer and the frames.
static inline int tbn_jpeg_host_parse(const unsigned char* data, size_t size, tbn_jpeg_geometry* out, char* err, size_t errlen) {
  using namespace tbn_jpeg;
  if (!out) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: null argument");
  Header h;
  const int rc = parse_header(data, size, &h, err, errlen);
  if (rc) return rc;
  *out = h.geo;
  return TBN_JPEG_OK;
}

// Decodes the scan into coef[expect->coef_count] (quantised, natural order, per component plane
// [block_row][block_col][64]) and quant[components][64] (natural order).
static inline int tbn_jpeg_host_entropy_decode(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect,
                                               int16_t* coef, uint16_t* quant, char* err, size_t errlen) {
  using namespace tbn_jpeg;
  if (!expect || !coef || !quant) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: null argument");
  Header h;
  int rc = parse_header(data, size, &h, err, errlen);
  if (rc) return rc;
  const tbn_jpeg_geometry& g = h.geo;
  if (!same_geometry(&g, expect))
    TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: geometry mismatch: image is %dx%d with %d components (luma %dx%d), expected %dx%d with %d (luma %dx%d)",
                  g.width, g.height, g.components, g.hsamp[0], g.vsamp[0], expect->width, expect->height, expect->components,
                  expect->hsamp[0], expect->vsamp[0]);
  const int nc = g.components;
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < 64; ++k) quant[c * 64 + kZigzagToNatural[k]] = h.quant[h.comp_tq[c]][k];
  int16_t* plane[3];
  {
    size_t off = 0;
    for (int c = 0; c < nc; ++c) {
      plane[c] = coef + off;
      off += (size_t)64 * g.blocks_w[c] * g.blocks_h[c];
    }
  }
  BitReader b;
  b.d = data; b.size = size; b.pos = h.scan_pos; b.acc = 0; b.nbits = 0; b.stopped = false;
  int pred[3] = {0, 0, 0};
  const int ri = g.restart_interval;
  int until_restart = ri, next_rst = 0;
  const long long total_mcus = (long long)h.mcus_x * h.mcus_y;
  long long mcu = 0;
  for (int my = 0; my < h.mcus_y; ++my) {
    for (int mx = 0; mx < h.mcus_x; ++mx, ++mcu) {
      if (ri && until_restart == 0) {
        const int m = br_marker(&b);
        if (m < 0)
          TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early or has stray data where RST%d is expected (MCU %lld of %lld)", next_rst, mcu, total_mcus);
        if (m != 0xD0 + next_rst)
          TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: RST%d expected at MCU %lld of %lld, found marker 0xFF%02X", next_rst, mcu, total_mcus, m);
        next_rst = (next_rst + 1) & 7;
        until_restart = ri;
        pred[0] = pred[1] = pred[2] = 0;
      }
      for (int c = 0; c < nc; ++c) {
        const HuffTable* dct = &h.dc[h.comp_td[c]];
        const HuffTable* act = &h.ac[h.comp_ta[c]];
        for (int v = 0; v < g.vsamp[c]; ++v) {
          for (int hh = 0; hh < g.hsamp[c]; ++hh) {
            const size_t brow = (size_t)my * g.vsamp[c] + v, bcol = (size_t)mx * g.hsamp[c] + hh;   // inside blocks_h x blocks_w
            int16_t* blk = plane[c] + (brow * g.blocks_w[c] + bcol) * 64;
            const int e = decode_block(&b, dct, act, &pred[c], blk);
            if (e == -1)
              TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early or hits a marker inside the scan data (MCU %lld of %lld, byte %zu)", mcu, total_mcus, b.pos);
            if (e == -2)
              TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: invalid Huffman code in the scan data (MCU %lld of %lld, byte %zu)", mcu, total_mcus, b.pos);
            if (e == -3)
              TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: DC coefficient %d leaves the int16 range (MCU %lld, component %d)", pred[c], mcu, c);
            if (e == -4)
              TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: AC run leaves the block (MCU %lld, component %d)", mcu, c);
          }
        }
      }
      if (ri) --until_restart;
    }
  }
  const int m = br_marker(&b);
  if (m == 0xD9) return TBN_JPEG_OK;
  if (m < 0) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early: no EOI marker after the scan (byte %zu of %zu)", b.pos, size);
  if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD)
    TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: more than one scan (marker 0xFF%02X after the first) is not supported", m);
  TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: marker 0xFF%02X where EOI is expected", m);
}
