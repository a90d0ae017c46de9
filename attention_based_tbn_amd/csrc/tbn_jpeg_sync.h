// Self-synchronising Huffman decoding of a baseline JPEG scan: the host pack stage and the decoder core that the
// kernel (csrc/jpeg_entropy.hip) and the CPU check program (scripts/jpeg_sync_check.cpp) share.  Plain C++, nothing
// from HIP: the core is marked TBN_JPEG_HD, which is `__host__ __device__` only under hipcc.
//
// Algorithm (Weissenberger & Schmidt, ICPP 2018 / HiPC 2021, in fixed-point form): the unstuffed scan is cut into
// INTERVALS (the whole scan, or one restart interval: byte-aligned, known start state) and every interval into
// SUBSEQUENCES of S bits, one lane each.  The state at a codeword boundary is (p, b, z): bit position, block inside
// the MCU, zigzag index (0: the DC symbol is next).  Lane i decodes from entry[i] until p >= the end of its
// subsequence and leaves exit[i]; entry[i + 1] = exit[i]; repeat until no entry changes.  Lane k is right after at
// most k rounds, and at the fixed point every entry is the exit of its predecessor back to a true start, so the
// result IS the sequential decode.
//
// Nothing here trusts the bytes: every read of the stream is clamped to the packed length and to the interval (past
// either it reads zeros), every coefficient address is checked against the geometry's block extents, and every loop
// consumes at least one bit per iteration or counts down.
#pragma once
#include "tbn_jpeg_host.h"

#if defined(__HIPCC__)
#define TBN_JPEG_HD __host__ __device__ __forceinline__
#else
#define TBN_JPEG_HD inline
#endif

#define TBN_JPEG_SYNC_MAX_LANES 1024        /* lanes (subsequences) of one image; also the most intervals it may have */
#define TBN_JPEG_SYNC_DEFAULT_BITS 1024     /* subsequence size when the caller passes 0 */
#define TBN_JPEG_SYNC_MAGIC 0x4A4E4254u     /* "TBNJ" */
#define TBN_JPEG_SYNC_NO_RECORD 0xFFFFFFFFu /* offsets[i]: image i has no record (it takes the host stage) */

/* status bits of one image */
#define TBN_JPEG_ST_CODE 1       /* invalid Huffman code on the true chain */
#define TBN_JPEG_ST_RUN 2        /* AC run leaves the block */
#define TBN_JPEG_ST_BLOCKS 4     /* an interval's block total differs from the geometry's */
#define TBN_JPEG_ST_END 8        /* an interval ends more than 7 bits after its last block, or inside one / out of bits */
#define TBN_JPEG_ST_DC 16        /* a DC value leaves int16 */
#define TBN_JPEG_ST_RECORD 32    /* the packed record is inconsistent (not from tbn_jpeg_scan_pack, or cut short) */
#define TBN_JPEG_ST_SKIPPED 64   /* no record was given for this image */

namespace tbn_jpeg {

// One Huffman table in the form the lanes read: the host decoder's 9-bit look table, then maxcode / valoff / vals for
// the longer codes.  1424 bytes, a multiple of 16.
struct DevHuff {
  uint16_t look[1 << kLookBits];
  int32_t maxcode[18];
  int32_t valoff[17];
  int32_t nvals;
  uint8_t vals[256];
};

// The tables of ONE image (files with optimised tables carry their own): up to four distinct ones, and which of them
// each component's DC and AC symbols use.  5728 bytes, a multiple of 16.
struct DevTables {
  DevHuff t[4];
  int32_t dc_slot[3], ac_slot[3];
  int32_t pad[2];
};

// Head of a packed record.  The record is [PackedHeader][DevTables][intervals: n x {start bit, bit length}][scan bytes],
// every part 16-byte aligned, offsets counted from the record's first byte.
struct PackedHeader {
  uint32_t magic;
  uint32_t n_intervals;
  uint32_t scan_bytes;        // unstuffed entropy-coded bytes, all intervals back to back; zero-padded to 16
  uint32_t intervals_off;
  uint32_t scan_off;
  uint32_t record_bytes;      // bytes used
  uint32_t restart_interval;  // MCUs per interval, 0: one interval
  uint32_t reserved;
};

static_assert(sizeof(DevHuff) == 1424 && sizeof(DevTables) == 5728 && sizeof(PackedHeader) == 32, "record layout");

constexpr size_t kPackedTablesOff = sizeof(PackedHeader);
constexpr size_t kPackedIntervalsOff = kPackedTablesOff + sizeof(DevTables);

static inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }

// capacity of the record of a file of `file_size` bytes with `n_intervals` intervals (the scan is shorter than the file)
static inline size_t packed_capacity(size_t file_size, size_t n_intervals) {
  return kPackedIntervalsOff + round16(8 * n_intervals) + round16(file_size);
}

static inline long long expected_intervals(const Header* h) {
  const long long mcus = (long long)h->mcus_x * h->mcus_y;
  const int ri = h->geo.restart_interval;
  return ri ? (mcus + ri - 1) / ri : 1;
}

// ---------------------------------------------------------------- decoder core (host and device) ----------------------
struct SyncState {
  uint32_t p;      // bit position in the packed scan
  uint32_t bz;     // (block inside the MCU << 8) | zigzag index
};

// what a lane needs of the geometry: the blocks of one MCU in scan order and where each lands
struct SyncGeom {
  int bpm;                       // blocks per MCU: 1 (gray), 3, 4 or 6
  int mcus_x;
  uint32_t total_mcus;
  uint8_t comp[8], bv[8], bh[8]; // per block of the MCU: component, row and column inside the MCU
  int hs[3], vs[3], bw[3], bh_[3];
  uint32_t coef_off[3];
  uint32_t coef_count;
};

TBN_JPEG_HD void sync_geom(const tbn_jpeg_geometry* g, SyncGeom* s) {
  s->bpm = 0;
  uint32_t off = 0;
  for (int c = 0; c < 3; ++c) { s->hs[c] = s->vs[c] = 1; s->bw[c] = s->bh_[c] = 0; s->coef_off[c] = 0; }
  for (int i = 0; i < 8; ++i) s->comp[i] = s->bv[i] = s->bh[i] = 0;
  for (int c = 0; c < g->components && c < 3; ++c) {
    s->hs[c] = g->hsamp[c]; s->vs[c] = g->vsamp[c];
    s->bw[c] = g->blocks_w[c]; s->bh_[c] = g->blocks_h[c];
    s->coef_off[c] = off;
    off += 64u * (uint32_t)g->blocks_w[c] * (uint32_t)g->blocks_h[c];
    for (int v = 0; v < g->vsamp[c]; ++v)
      for (int h = 0; h < g->hsamp[c]; ++h)
        if (s->bpm < 8) {
          s->comp[s->bpm] = (uint8_t)c; s->bv[s->bpm] = (uint8_t)v; s->bh[s->bpm] = (uint8_t)h;
          ++s->bpm;
        }
  }
  s->coef_count = off;
  s->mcus_x = (g->width + 8 * g->hsamp[0] - 1) / (8 * g->hsamp[0]);
  const int mcus_y = (g->height + 8 * g->vsamp[0] - 1) / (8 * g->vsamp[0]);
  s->total_mcus = (uint32_t)s->mcus_x * (uint32_t)mcus_y;
}

// first coefficient of block `n` (blocks counted in scan order over the whole image); false if it is outside the image
TBN_JPEG_HD bool sync_block_offset(const SyncGeom& g, uint32_t n, uint32_t* off) {
  const uint32_t mcu = n / (uint32_t)g.bpm, b = n - mcu * (uint32_t)g.bpm;
  if (mcu >= g.total_mcus) return false;
  const uint32_t my = mcu / (uint32_t)g.mcus_x, mx = mcu - my * (uint32_t)g.mcus_x;
  const int c = g.comp[b];
  const uint32_t brow = my * (uint32_t)g.vs[c] + g.bv[b], bcol = mx * (uint32_t)g.hs[c] + g.bh[b];
  if (brow >= (uint32_t)g.bh_[c] || bcol >= (uint32_t)g.bw[c]) return false;
  *off = g.coef_off[c] + (brow * (uint32_t)g.bw[c] + bcol) * 64u;
  return *off + 64u <= g.coef_count;
}

TBN_JPEG_HD uint32_t sync_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}

// 32 bits at bit `p` of the stream, MSB first; bits at or past `end`, and words past `nwords`, read as zeros.
// words[0, nwords): the bytes in file order (kSwapped false), or dwords already swapped to MSB-first values (true: the
// kernel swaps once when it stages the scan in LDS)
template <bool kSwapped>
TBN_JPEG_HD uint32_t sync_peek32(const uint32_t* words, uint32_t nwords, uint32_t p, uint32_t end) {
  if (p >= end) return 0;
  const uint32_t i = p >> 5, s = p & 31;
  uint32_t w0 = i < nwords ? words[i] : 0u, w1 = i + 1 < nwords ? words[i + 1] : 0u;
  if (!kSwapped) { w0 = sync_bswap(w0); w1 = sync_bswap(w1); }
  uint32_t x = (uint32_t)((((unsigned long long)w0 << 32) | w1) >> (32 - s));       // s = 0: w0
  const uint32_t avail = end - p;
  if (avail < 32) x &= ~(0xFFFFFFFFu >> avail);
  return x;
}

// table slot of every block of the MCU: slots[2 b] for its DC symbol, slots[2 b + 1] for its AC symbols
TBN_JPEG_HD void sync_block_slots(const DevTables* tab, const SyncGeom& g, uint8_t* slots /* 16 */) {
  for (int b = 0; b < 8; ++b) {
    const int c = g.comp[b] < 3 ? g.comp[b] : 0;
    slots[2 * b] = (uint8_t)(tab->dc_slot[c] & 3);
    slots[2 * b + 1] = (uint8_t)(tab->ac_slot[c] & 3);
  }
}

// the symbol whose code starts the window `x`; -2: no such code.  *len: the code's length (1..16)
TBN_JPEG_HD int sync_symbol(const DevHuff* t, uint32_t x, int* len) {
  const uint16_t e = t->look[x >> (32 - kLookBits)];
  if (e) {
    *len = e >> 8;
    return e & 255;
  }
  const uint32_t w = x >> 16;
  for (int l = kLookBits + 1; l <= 16; ++l) {
    const int32_t code = (int32_t)(w >> (16 - l));
    if (code <= t->maxcode[l]) {
      *len = l;
      const int idx = t->valoff[l] + code;
      return (idx >= 0 && idx < t->nvals && idx < 256) ? t->vals[idx] : -2;
    }
  }
  *len = 16;
  return -2;
}

TBN_JPEG_HD int sync_extend(uint32_t r, int cat) {     // cat 1..15
  return r < (1u << (cat - 1)) ? (int)r - (1 << cat) + 1 : (int)r;
}

// events of one subsequence decode
#define TBN_JPEG_EV_CODE 1      /* no such code */
#define TBN_JPEG_EV_RUN 2       /* AC run past coefficient 63 */
#define TBN_JPEG_EV_OVERRUN 4   /* the next symbol does not fit into the interval: the lane stopped in front of it */

// A sink that drops the coefficients: the relaxation rounds.
struct SyncNoSink {
  TBN_JPEG_HD void put(uint32_t, int, int) {}
};

// A sink that stores into coef[0, coef_count) of one image: block `first_block + k` for the k-th block the lane works
// on, nothing for a block at or past `block_limit` or outside the geometry.  The DC is stored as the difference.
struct SyncCoefSink {
  int16_t* coef;
  const SyncGeom* g;
  const uint8_t* natural;      // zigzag -> natural order
  uint32_t first_block, block_limit;
  uint32_t cached_k, cached_off;
  bool cached_ok;
  TBN_JPEG_HD void put(uint32_t k, int z, int value) {
    if (k != cached_k) {
      cached_k = k;
      const uint32_t n = first_block + k;
      cached_ok = n >= first_block && n < block_limit && sync_block_offset(*g, n, &cached_off);
    }
    if (cached_ok) coef[cached_off + natural[z & 63]] = (int16_t)value;
  }
};

// Decodes from *st until p >= sub_end (or an event).  int_end: end of the interval; guess: the state a lane leaves
// after an invalid code or a run past 63.  *blocks: blocks COMPLETED here (the k-th block a lane works on is the one it
// completes k-th; the last may stay open).  Returns the events.  One path for DC and AC symbols (a DC symbol is a run of
// 0 with its category), so that the lanes of a wavefront, which are at different places of their blocks, diverge less.
template <bool kSwapped, class Sink>
TBN_JPEG_HD uint32_t sync_decode(const DevTables* tab, const uint32_t* words, uint32_t nwords, uint32_t sub_end,
                                 uint32_t int_end, int bpm, const uint8_t* slots, SyncState guess, SyncState* st,
                                 uint32_t* blocks, Sink& sink) {
  uint32_t p = st->p, b = st->bz >> 8, z = st->bz & 255u, done = 0;
  if (b >= (uint32_t)bpm || b >= 8) b = 0;
  if (z > 63) z = 0;
  if (sub_end > int_end) sub_end = int_end;
  uint32_t ev = 0;
  while (p < sub_end) {                              // every pass consumes len >= 1 bits or leaves the loop
    const uint32_t x = sync_peek32<kSwapped>(words, nwords, p, int_end);
    const bool dc = z == 0;
    int len;
    const int s = sync_symbol(&tab->t[slots[2 * b + (dc ? 0 : 1)] & 3], x, &len);
    if (s < 0 || (dc && s > 15)) {                   // as the host stage: no code in fewer than 16 real bits is "out of
      ev = int_end - p < 16 ? TBN_JPEG_EV_OVERRUN : TBN_JPEG_EV_CODE;     // data" (the padding of an interval), not an invalid code
      break;
    }
    const uint32_t run = dc ? 0u : (uint32_t)s >> 4, cat = (uint32_t)s & 15u;
    const uint32_t total = (uint32_t)len + cat;      // <= 31: inside the window
    if (total > int_end - p) { ev = TBN_JPEG_EV_OVERRUN; break; }
    bool close = false;
    if (cat == 0) {
      if (dc) z = 1;                                 // a zero difference
      else if (run == 15) { z += 16; close = z > 63; }    // ZRL; the host stage lets it close the block too
      else close = true;                             // EOB
    } else {
      z += run;
      if (z > 63) { ev = TBN_JPEG_EV_RUN; break; }
      sink.put(done, (int)z, sync_extend((x << len) >> (32 - cat), (int)cat));
      ++z;
      close = z > 63;
    }
    p += total;
    if (close) {
      z = 0;
      ++done;
      if (++b >= (uint32_t)bpm) b = 0;
    }
  }
  if (ev & (TBN_JPEG_EV_CODE | TBN_JPEG_EV_RUN)) {
    *st = guess;
  } else {
    st->p = p;
    st->bz = (b << 8) | z;
  }
  *blocks = done;
  return ev;
}

// lanes of an interval of `bits` bits at subsequence size S
TBN_JPEG_HD uint32_t sync_interval_lanes(uint32_t bits, uint32_t S) { return (bits + S - 1) / S; }

// blocks the geometry gives interval i
TBN_JPEG_HD uint32_t sync_interval_blocks(const SyncGeom& g, uint32_t ri, uint32_t i) {
  if (ri == 0) return i == 0 ? g.total_mcus * (uint32_t)g.bpm : 0u;
  const unsigned long long first = (unsigned long long)i * ri;
  if (first >= g.total_mcus) return 0u;
  const uint32_t left = g.total_mcus - (uint32_t)first;
  return (left < ri ? left : ri) * (uint32_t)g.bpm;
}

// status bits of an interval at the fixed point: the blocks its lanes completed, the state its last lane left
TBN_JPEG_HD uint32_t sync_interval_status(uint32_t blocks, uint32_t expected, bool has_lanes, SyncState last_exit,
                                          uint32_t int_end) {
  uint32_t st = 0;
  if (blocks != expected) st |= TBN_JPEG_ST_BLOCKS;
  if (!has_lanes) return expected ? st | TBN_JPEG_ST_END : st;
  if (last_exit.bz != 0 || last_exit.p > int_end || int_end - last_exit.p > 7) st |= TBN_JPEG_ST_END;
  return st;
}

// ---------------------------------------------------------------- host pack stage -------------------------------------
static inline void pack_huff(const HuffTable* s, DevHuff* d) {
  memcpy(d->look, s->look, sizeof(d->look));
  memcpy(d->maxcode, s->maxcode, sizeof(d->maxcode));
  d->valoff[0] = 0;
  for (int l = 1; l <= 16; ++l) d->valoff[l] = s->valoff[l];
  d->nvals = s->nvals;
  memcpy(d->vals, s->vals, sizeof(d->vals));
}

}  // namespace tbn_jpeg

// bytes of the record tbn_jpeg_host_scan_pack writes for a file of `file_size` bytes with `n_intervals` intervals, at most
static inline size_t tbn_jpeg_host_scan_pack_bytes(size_t file_size, size_t n_intervals) {
  return tbn_jpeg::packed_capacity(file_size, n_intervals);
}

// Parses as tbn_jpeg_host_entropy_decode does, then in one pass over the bytes copies the entropy-coded segment into
// the record (0xFF00 stuffing and fill bytes removed), cut at the RSTn markers, whose order it checks; writes the
// interval table, the image's Huffman tables in device form and quant[components][64] (natural order, the layout
// tbn_jpeg_reconstruct takes).  *n_intervals: ceil(MCUs / restart interval), or 1.  If that is more than
// `max_intervals`, NOTHING is packed, *used = 0 and the return is TBN_JPEG_OK: such an image takes the host stage.
// Writes nothing outside record[0, record_bytes) and quant[0, components * 64).
static inline int tbn_jpeg_host_scan_pack(const unsigned char* data, size_t size, const tbn_jpeg_geometry* expect,
                                          void* record, size_t record_bytes, int max_intervals, uint16_t* quant,
                                          int* n_intervals, size_t* used, char* err, size_t errlen) {
  using namespace tbn_jpeg;
  if (!expect || !record || !quant || !n_intervals || !used) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: null argument");
  *n_intervals = 0;
  *used = 0;
  Header h;
  int rc = parse_header(data, size, &h, err, errlen);
  if (rc) return rc;
  const tbn_jpeg_geometry& g = h.geo;
  if (!same_geometry(&g, expect))
    TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: geometry mismatch: image is %dx%d with %d components (luma %dx%d), expected %dx%d with %d (luma %dx%d)",
                  g.width, g.height, g.components, g.hsamp[0], g.vsamp[0], expect->width, expect->height, expect->components,
                  expect->hsamp[0], expect->vsamp[0]);
  if (((uintptr_t)record & 15) != 0) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: the pack record must be 16-byte aligned");
  if (size >= ((size_t)1 << 28)) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: a file of %zu bytes is too large to pack", size);
  const int nc = g.components;
  const long long total_mcus = (long long)h.mcus_x * h.mcus_y;
  const long long want = expected_intervals(&h);
  *n_intervals = want > 0x7fffffff ? 0x7fffffff : (int)want;
  if (max_intervals < 1 || want > max_intervals) return TBN_JPEG_OK;       // not packed: *used stays 0
  const size_t intervals_off = kPackedIntervalsOff, scan_off = intervals_off + round16(8 * (size_t)want);
  if (record_bytes < scan_off) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: pack record of %zu bytes is too small", record_bytes);
  const size_t scan_cap = (record_bytes - scan_off) & ~(size_t)15;          // whole 16-byte groups only: room for the padding
  unsigned char* rec = (unsigned char*)record;
  // the tables: at most four distinct ones
  DevTables* tab = (DevTables*)(rec + kPackedTablesOff);
  memset(tab, 0, sizeof(*tab));
  {
    int ids[4], used_slots = 0;              // id: class << 2 | table number
    for (int c = 0; c < nc; ++c)
      for (int cls = 0; cls < 2; ++cls) {
        const int id = (cls << 2) | (cls ? h.comp_ta[c] : h.comp_td[c]);
        int slot = -1;
        for (int k = 0; k < used_slots; ++k)
          if (ids[k] == id) slot = k;
        if (slot < 0) {
          if (used_slots == 4) TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: more than four distinct Huffman tables in one scan cannot be packed");
          slot = used_slots++;
          ids[slot] = id;
          pack_huff(cls ? &h.ac[h.comp_ta[c]] : &h.dc[h.comp_td[c]], &tab->t[slot]);
        }
        (cls ? tab->ac_slot : tab->dc_slot)[c] = slot;
      }
  }
  for (int c = 0; c < nc; ++c)
    for (int k = 0; k < 64; ++k) quant[c * 64 + kZigzagToNatural[k]] = h.quant[h.comp_tq[c]][k];
  uint32_t* iv = (uint32_t*)(rec + intervals_off);
  unsigned char* out = rec + scan_off;
  const int ri = g.restart_interval;
  size_t o = 0, start = 0, pos = h.scan_pos;
  long long done = 0;                        // intervals closed
  int next_rst = 0;
  for (;;) {
    if (pos >= size) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early: no EOI marker after the scan (byte %zu of %zu)", pos, size);
    const unsigned char c = data[pos];
    if (c != 0xFF) {
      if (o >= scan_cap) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: pack record of %zu bytes is too small", record_bytes);
      out[o++] = c;
      ++pos;
      continue;
    }
    size_t q = pos + 1;                      // 0xFF, fill 0xFFs, then 0x00 (a stuffed data byte 0xFF) or a marker code
    while (q < size && data[q] == 0xFF) ++q;
    if (q >= size) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early: no EOI marker after the scan (byte %zu of %zu)", pos, size);
    const int m = data[q];
    if (m == 0x00) {
      if (o >= scan_cap) TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: pack record of %zu bytes is too small", record_bytes);
      out[o++] = 0xFF;
      pos = q + 1;
      continue;
    }
    const long long mcu = ri ? (done + 1) * ri : total_mcus;
    if (m >= 0xD0 && m <= 0xD7) {
      if (!ri || done + 1 >= want)
        TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early or hits a marker inside the scan data (marker 0xFF%02X, byte %zu)", m, pos);
      if (m != 0xD0 + next_rst)
        TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: RST%d expected at MCU %lld of %lld, found marker 0xFF%02X", next_rst, mcu, total_mcus, m);
      next_rst = (next_rst + 1) & 7;
      iv[2 * done] = (uint32_t)(8 * start);
      iv[2 * done + 1] = (uint32_t)(8 * (o - start));
      ++done;
      start = o;
      pos = q + 1;
      continue;
    }
    if (m == 0xD9) {
      if (done + 1 != want)
        TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early or has stray data where RST%d is expected (MCU %lld of %lld)", next_rst, mcu, total_mcus);
      iv[2 * done] = (uint32_t)(8 * start);
      iv[2 * done + 1] = (uint32_t)(8 * (o - start));
      ++done;
      break;
    }
    if (done + 1 != want)
      TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: stream ends early or hits a marker inside the scan data (marker 0xFF%02X, byte %zu)", m, pos);
    if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD)
      TBN_JPEG_FAIL(TBN_JPEG_ERR_UNSUPPORTED, "jpeg: more than one scan (marker 0xFF%02X after the first) is not supported", m);
    TBN_JPEG_FAIL(TBN_JPEG_ERR_DATA, "jpeg: marker 0xFF%02X where EOI is expected", m);
  }
  for (size_t k = 2 * (size_t)want; k < round16(8 * (size_t)want) / 4; ++k) iv[k] = 0;
  const size_t padded = round16(o);          // <= scan_cap, a multiple of 16
  memset(out + o, 0, padded - o);
  PackedHeader* ph = (PackedHeader*)rec;
  ph->magic = TBN_JPEG_SYNC_MAGIC;
  ph->n_intervals = (uint32_t)want;
  ph->scan_bytes = (uint32_t)o;
  ph->intervals_off = (uint32_t)intervals_off;
  ph->scan_off = (uint32_t)scan_off;
  ph->record_bytes = (uint32_t)(scan_off + padded);
  ph->restart_interval = (uint32_t)ri;
  ph->reserved = 0;
  *used = scan_off + padded;
  return TBN_JPEG_OK;
}
