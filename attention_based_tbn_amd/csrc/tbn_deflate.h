// RFC 1951 (raw deflate) ENCODER core, shared by the kernels in csrc/deflate.hip, the host twin tbn_deflate_host and the
// stand-alone memory checks scripts/deflate_check.cpp and scripts/inflate_chunks_check.cpp.  Plain C++: no HIP, no global state; the core is marked TBN_DEF_HD,
// which is `__host__ __device__` only under hipcc (the way tbn_inflate.h is shared).  Replaces the zlib level 6 run inside
// np.savez_compressed of reference preprocessing/create_epic_flow_pickle.py:203.
//
// THE STREAM FORMAT (fixed: the host and the device produce the same bytes, and so does every later version unless one of
// the constants below changes)
//   * A member's raw bytes are cut into chunks of kChunk = 32 768 bytes (tbn_deflate_chunk()); the last may be shorter.
//     Chunks are compressed independently and joined on byte boundaries (the pigz construction).
//   * A chunk is parsed greedily into literals and matches (length 3..258).  A match never reaches before the chunk's
//     first byte, so distances are at most kChunk - 1.  The match finder is a hash table of kBuckets = 2048 buckets over
//     the next 3 bytes; a bucket holds the kWays = 4 most recent positions with that hash, and ALL FOUR are tried at every
//     position, newest first (the constant search depth).  The longest match wins, the newest among equals; a match of
//     length 3 further back than 4096 bytes is dropped (a literal is cheaper).  Every position a match covers is
//     entered into the table.
//   * The parse is cut into blocks of at most kBlockTokens = 4096 tokens.  Per block the exact bit cost of the three
//     block types is computed -- stored (from the current bit position: padding, LEN, NLEN, the bytes), fixed, dynamic
//     (header included) -- and the cheapest is written; equal costs prefer stored, then fixed.
//   * Dynamic blocks: code lengths by the in-place minimum-redundancy construction of Moffat and Katajainen over the
//     symbols sorted by (frequency, symbol), then limited to 15 bits (literal/length, distance) or 7 bits (the
//     code-length code) by moving codes down from the over-long tail until the Kraft sum is 1; a code with fewer than
//     two used symbols gets symbol 0 or 1 added (as zlib does), so every code written is complete.  The header is the
//     run-length coded length sequence of RFC 1951 3.2.7 (symbols 16, 17, 18).
//   * A chunk whose blocks would need as many bytes as its stored form or more is written as ONE stored block instead (5
//     bytes + the raw bytes, since every chunk starts on a byte boundary): no stream is longer than
//     tbn_deflate_bound(n) = n + 5 * max(1, ceil(n / kChunk)).
//   * Every chunk but the last ends byte-aligned: when its last block does not end on a byte boundary an empty stored
//     block follows (bits 000, padding, 00 00 FF FF).  The last chunk's last block carries BFINAL; its last byte is padded
//     with zero bits and nothing follows.  An empty member is the one final fixed block `03 00`.
//
// Why every loop ends: each step of the parse consumes at least one input byte; the candidate search has kWays trips and a
// match comparison at most 258; block, header and code construction loop over at most kBlockTokens tokens, 320 code
// lengths and 288 symbols.  A chunk depends on nothing outside itself: no flags, no look-back, no waiting.
//
// The core is a template over an IO policy with one member, IO::put(pos, byte): compressed byte `pos` of the chunk's
// slot.  The writer checks `pos` against the slot's capacity before every call.  Everything else -- the chunk's input
// bytes included -- lives in `State` (LDS on the device, the heap on the host).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TBN_DEF_HD __host__ __device__ __forceinline__
#else
#define TBN_DEF_HD inline
#endif

/* status of one member (include/tbn_hip.h documents them for callers) */
#define TBN_DEF_OK 0
#define TBN_DEF_CAPACITY 1   /* out_cap < tbn_deflate_bound(in_len) */
#define TBN_DEF_ROW 2        /* the row is inconsistent: a range outside the buffers, in_len >= 2^31, in_off not a multiple of 4 */
#define TBN_DEF_SKIPPED 3    /* the row carries the skip marker: nothing read, nothing written */

namespace tbn_deflate {

constexpr uint32_t kChunk = 32768;        // raw bytes per chunk: part of the format
constexpr uint32_t kBuckets = 2048;       // hash buckets (11 bits)
constexpr int kWays = 4;                  // positions per bucket = candidates tried per position (16 bits each in a uint64)
constexpr uint32_t kBlockTokens = 4096;   // tokens per block
constexpr uint32_t kTooFar = 4096;        // a length-3 match further back than this is dropped
constexpr uint32_t kMinMatch = 3, kMaxMatch = 258;
constexpr uint32_t kStoredHeader = 5;     // a stored block from a byte boundary: 3 bits + 5 padding, LEN, NLEN
// the slot of one chunk in the workspace: 16 bytes of header (the size in the first 4), then the compressed bytes.  The
// blocks of a chunk are abandoned before they pass its stored form (kChunk + 5), the terminator adds at most 6 bytes.
constexpr uint32_t kSlotHeader = 16;
constexpr uint32_t kSlotData = kChunk + 32;
constexpr uint32_t kSlot = kSlotHeader + kSlotData;
constexpr uint32_t kUseStored = 0xFFFFFFFFu;   // compress_chunk: write the chunk as one stored block
static_assert(kChunk <= 32768, "distances are at most kChunk - 1 and must be below 32 769; positions fit 15 bits");
static_assert(kWays * 16 == 64, "a bucket is one uint64");

TBN_DEF_HD uint64_t chunks_of(uint64_t n) { return n == 0 ? 1 : (n + kChunk - 1) / kChunk; }
TBN_DEF_HD uint64_t bound(uint64_t n) { return n + kStoredHeader * chunks_of(n); }

struct State {
  uint8_t in[kChunk];               // the chunk's raw bytes
  uint64_t head[kBuckets];          // kWays positions per bucket, newest in the low 16 bits; 0xFFFF: none
  uint32_t tok[kBlockTokens];       // literal: the byte; match: (length << 16) | distance
  uint32_t work[288];               // code construction: (frequency, then parent / depth) of the sorted symbols
  uint16_t order[288];              // symbols sorted by (frequency, symbol)
  uint16_t lfreq[288], dfreq[32], cfreq[19];
  uint16_t lcode[288], dcode[32], ccode[19];   // bit-reversed codes, ready for the writer
  uint8_t lens[288 + 32];           // literal/length lengths, then distance lengths from [288]
  uint8_t clen[19];
  uint8_t seq[320], hsym[320], hext[320];      // the header's length sequence and its run-length coding
  uint32_t count[33], next[16];     // codes per length, next code per length (here, not in locals: on the device an
                                    // indexed local array lives in scratch memory, a global-memory round trip per access)
};

struct Writer {
  uint64_t hold = 0;
  uint32_t nbits = 0;
  uint32_t pos = 0;       // bytes handed to the IO policy
  uint32_t cap = 0;
  bool overflow = false;  // a byte did not fit: the chunk is written stored (never happens: the budget check comes first)
  template <class IO>
  TBN_DEF_HD void byte(IO& io, uint32_t b) {
    if (pos < cap)
      io.put(pos, (uint8_t)b);
    else
      overflow = true;
    ++pos;
  }
  template <class IO>
  TBN_DEF_HD void bits(IO& io, uint32_t v, uint32_t n) {      // n <= 16
    hold |= (uint64_t)v << nbits;
    nbits += n;
    while (nbits >= 8) {
      byte(io, (uint32_t)hold & 0xFFu);
      hold >>= 8;
      nbits -= 8;
    }
  }
  template <class IO>
  TBN_DEF_HD void align(IO& io) {                              // zero bits up to the next byte boundary
    if (nbits) bits(io, 0, 8 - nbits);
  }
  TBN_DEF_HD uint64_t bitpos() const { return (uint64_t)pos * 8u + nbits; }
};

TBN_DEF_HD uint32_t load_u32(const uint8_t* p) {     // little endian, any alignment
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
TBN_DEF_HD uint32_t floor_log2(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }   // v > 0

// length 3..258 -> literal/length symbol, number of extra bits, their value
TBN_DEF_HD void length_symbol(uint32_t len, uint32_t* sym, uint32_t* nextra, uint32_t* extra) {
  const uint32_t l = len - 3;
  if (l < 8) {
    *sym = 257 + l, *nextra = 0, *extra = 0;
  } else if (len == 258) {
    *sym = 285, *nextra = 0, *extra = 0;
  } else {
    const uint32_t e = floor_log2(l) - 2;
    *sym = 257 + 4 * (e + 1) + ((l >> e) & 3u), *nextra = e, *extra = l & ((1u << e) - 1u);
  }
}
// distance 1..32768 -> distance symbol, number of extra bits, their value
TBN_DEF_HD void distance_symbol(uint32_t dist, uint32_t* sym, uint32_t* nextra, uint32_t* extra) {
  const uint32_t d = dist - 1;
  if (d < 4) {
    *sym = d, *nextra = 0, *extra = 0;
  } else {
    const uint32_t e = floor_log2(d) - 1;
    *sym = 2 * (e + 1) + ((d >> e) & 1u), *nextra = e, *extra = d & ((1u << e) - 1u);
  }
}
TBN_DEF_HD uint32_t length_extra_bits(uint32_t sym) { return sym < 265 || sym == 285 ? 0 : (sym - 261) >> 2; }
TBN_DEF_HD uint32_t distance_extra_bits(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
TBN_DEF_HD uint32_t fixed_length(uint32_t sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

TBN_DEF_HD uint32_t reverse_bits(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// Code lengths (<= maxbits) of the n symbols with frequencies freq[] into lens[]; unused symbols get 0.  A code with
// fewer than two used symbols gets symbol 0 or 1 added so that it is complete.  n <= 288.
TBN_DEF_HD void code_lengths(State& s, const uint16_t* freq, int n, uint32_t maxbits, uint8_t* lens) {
  int used = 0;
  for (int i = 0; i < n; ++i) {
    lens[i] = 0;
    if (freq[i]) {                              // insertion sort by (frequency, symbol): symbols arrive in order
      const uint32_t f = freq[i];
      int k = used++;
      while (k > 0 && s.work[k - 1] > f) {
        s.work[k] = s.work[k - 1];
        s.order[k] = s.order[k - 1];
        --k;
      }
      s.work[k] = f;
      s.order[k] = (uint16_t)i;
    }
  }
  if (used < 2) {                               // length 1 for the used symbol (if any) and for symbol 0 or 1
    const int have = used ? (int)s.order[0] : -1;
    lens[have == 0 ? 1 : 0] = 1;
    if (used) lens[have] = 1;
    if (!used) lens[1] = 1;
    return;
  }
  uint32_t* A = s.work;
  // Moffat & Katajainen, "In-place calculation of minimum-redundancy codes": A ascending frequencies -> A code lengths
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < used - 1; ++next) {
    if (leaf >= used || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= used || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  A[used - 2] = 0;
  for (int next = used - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
  int avail = 1, taken = 0, next = used - 1;
  uint32_t depth = 0;
  root = used - 2;
  while (avail > 0) {                           // at most `used` levels: every level places a leaf or has an internal node
    while (root >= 0 && A[root] == depth) {
      ++taken;
      --root;
    }
    while (avail > taken) {
      A[next--] = depth;
      --avail;
    }
    avail = 2 * taken;
    ++depth;
    taken = 0;
  }
  // limit to maxbits: codes longer than that are cut to it, then codes move down one level until the Kraft sum is 1
  uint32_t* count = s.count;
  for (uint32_t l = 0; l <= 32; ++l) count[l] = 0;
  for (int i = 0; i < used; ++i) ++count[A[i] < maxbits ? A[i] : maxbits];    // depths are < 288, but 32 bounds the table
  uint32_t total = 0;
  for (uint32_t l = 1; l <= maxbits; ++l) total += count[l] << (maxbits - l);
  while (total > (1u << maxbits)) {             // each trip lowers total by one
    --count[maxbits];
    for (uint32_t l = maxbits - 1; l >= 1; --l) {
      if (count[l]) {
        --count[l];
        count[l + 1] += 2;
        break;
      }
    }
    --total;
  }
  int at = 0;                                   // the rarest symbols take the longest codes
  for (uint32_t l = maxbits; l >= 1; --l)
    for (uint32_t c = 0; c < count[l]; ++c) lens[s.order[at++]] = (uint8_t)l;
}

// canonical codes of lens[0, n), bit-reversed
TBN_DEF_HD void make_codes(State& s, const uint8_t* lens, int n, uint16_t* codes) {
  uint32_t *count = s.count, *next = s.next;
  for (int l = 0; l < 16; ++l) count[l] = 0;
  for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
  count[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int l = 1; l < 16; ++l) {
    c = (c + count[l - 1]) << 1;
    next[l] = c;
  }
  for (int i = 0; i < n; ++i) {
    const uint32_t l = lens[i] & 15;
    codes[i] = l ? (uint16_t)reverse_bits(next[l]++, l) : 0;
  }
}

TBN_DEF_HD int cl_order(int i) {      // RFC 1951 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
  return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 8 - (i - 3) / 2 : 8 + (i - 4) / 2 ;
}

// The header of a dynamic block for s.lens: fills s.seq / hsym / hext / cfreq / clen / ccode.  -> its bits (the 3 block
// bits not included); *n_l, *n_d, *n_cl, *n_h: HLIT + 257, HDIST + 1, HCLEN + 4, header symbols.
TBN_DEF_HD uint32_t plan_header(State& s, int* n_l, int* n_d, int* n_cl, int* n_h) {
  int nl = 286, nd = 30;
  while (nl > 257 && s.lens[nl - 1] == 0) --nl;
  while (nd > 1 && s.lens[288 + nd - 1] == 0) --nd;
  for (int i = 0; i < nl; ++i) s.seq[i] = s.lens[i];
  for (int i = 0; i < nd; ++i) s.seq[nl + i] = s.lens[288 + i];
  const int total = nl + nd;
  for (int i = 0; i < 19; ++i) s.cfreq[i] = 0;
  int nh = 0, i = 0;
  uint32_t extra_bits = 0;
  while (i < total) {                           // every trip consumes run >= 1 lengths
    const uint32_t v = s.seq[i];
    int run = 1;
    while (i + run < total && s.seq[i + run] == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        s.hsym[nh] = 18, s.hext[nh++] = (uint8_t)(r - 11), extra_bits += 7, run -= r;
      }
      if (run >= 3) s.hsym[nh] = 17, s.hext[nh++] = (uint8_t)(run - 3), extra_bits += 3, run = 0;
    } else {
      s.hsym[nh] = (uint8_t)v, s.hext[nh++] = 0, --run;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        s.hsym[nh] = 16, s.hext[nh++] = (uint8_t)(r - 3), extra_bits += 2, run -= r;
      }
    }
    for (; run > 0; --run) s.hsym[nh] = (uint8_t)v, s.hext[nh++] = 0;
  }
  for (int k = 0; k < nh; ++k) ++s.cfreq[s.hsym[k]];
  code_lengths(s, s.cfreq, 19, 7, s.clen);
  make_codes(s, s.clen, 19, s.ccode);
  int ncl = 19;
  while (ncl > 4 && s.clen[cl_order(ncl - 1)] == 0) --ncl;
  uint32_t bits = 5 + 5 + 4 + 3 * (uint32_t)ncl + extra_bits;
  for (int k = 0; k < 19; ++k) bits += (uint32_t)s.cfreq[k] * s.clen[k];
  *n_l = nl, *n_d = nd, *n_cl = ncl, *n_h = nh;
  return bits;
}

// the tokens of one block with the codes in s.lcode / s.dcode and the lengths lens[0, 288) / lens[288, 320), then EOB
template <class IO>
TBN_DEF_HD void write_tokens(IO& io, State& s, Writer& w, uint32_t ntok, const uint8_t* lens) {
  for (uint32_t k = 0; k < ntok; ++k) {
    const uint32_t t = s.tok[k];
    if (t < 65536u) {
      w.bits(io, s.lcode[t], lens[t]);
    } else {
      uint32_t sym, ne, ev;
      length_symbol(t >> 16, &sym, &ne, &ev);
      w.bits(io, s.lcode[sym], lens[sym]);
      w.bits(io, ev, ne);
      distance_symbol(t & 0xFFFFu, &sym, &ne, &ev);
      w.bits(io, s.dcode[sym], lens[288 + sym]);
      w.bits(io, ev, ne);
    }
  }
  w.bits(io, s.lcode[256], lens[256]);
}

// Compresses the n bytes (1 <= n <= kChunk) in s.in into the slot behind `io` (capacity kSlotData); `last`: the member's
// last chunk.  s.head must be all ones.  -> the slot's bytes, or kUseStored: write stored_header() and the raw bytes.
template <class IO>
TBN_DEF_HD uint32_t compress_chunk(IO& io, State& s, uint32_t n, bool last) {
  Writer w;
  w.cap = kSlotData;
  const uint64_t budget = 8ull * (kStoredHeader + n);      // the chunk's stored form
  uint32_t pos = 0;
  for (;;) {
    const uint32_t block_start = pos;
    uint32_t ntok = 0;
    for (int i = 0; i < 288; ++i) s.lfreq[i] = 0;
    for (int i = 0; i < 32; ++i) s.dfreq[i] = 0;
    uint32_t extra_bits = 0;                                // of the block's matches: the same under both codes
    while (pos < n && ntok < kBlockTokens) {                // each trip consumes at least one byte
      uint32_t best_len = 0, best_dist = 0;
      const uint32_t room = n - pos;
      if (room >= kMinMatch) {
        const uint32_t maxlen = room < kMaxMatch ? room : kMaxMatch;
        const uint32_t h = (((uint32_t)s.in[pos] | (uint32_t)s.in[pos + 1] << 8 | (uint32_t)s.in[pos + 2] << 16) * 0x9E3779B1u) >> 21;
        const uint64_t bucket = s.head[h];
        s.head[h] = (bucket << 16) | pos;
        for (int wy = 0; wy < kWays; ++wy) {
          const uint32_t cand = (uint32_t)(bucket >> (16 * wy)) & 0xFFFFu;
          if (cand >= pos) continue;                        // 0xFFFF: empty (positions are < 32 768 and older than pos)
          if (best_len >= maxlen) break;
          if (s.in[cand + best_len] != s.in[pos + best_len]) continue;     // cannot be longer than the best so far
          uint32_t len = 0;
          while (len + 4 <= maxlen) {                       // four bytes a trip: the loads of one trip do not wait for each other
            const uint32_t x = load_u32(s.in + cand + len) ^ load_u32(s.in + pos + len);
            if (x) {
              len += (uint32_t)__builtin_ctz(x) >> 3;
              break;
            }
            len += 4;
          }
          if (len + 4 > maxlen)                             // the last 0..3 bytes (after a mismatch the first comparison ends it)
            while (len < maxlen && s.in[cand + len] == s.in[pos + len]) ++len;
          if (len > best_len) best_len = len, best_dist = pos - cand;
        }
        if (best_len < kMinMatch || (best_len == kMinMatch && best_dist > kTooFar)) best_len = 0;
      }
      if (best_len) {
        uint32_t sym, ne, ev;
        length_symbol(best_len, &sym, &ne, &ev);
        ++s.lfreq[sym];
        extra_bits += ne;
        distance_symbol(best_dist, &sym, &ne, &ev);
        ++s.dfreq[sym];
        extra_bits += ne;
        s.tok[ntok++] = best_len << 16 | best_dist;
        for (uint32_t p = pos + 1; p < pos + best_len; ++p) {       // at most 257 trips
          if (n - p < kMinMatch) break;
          const uint32_t h = (((uint32_t)s.in[p] | (uint32_t)s.in[p + 1] << 8 | (uint32_t)s.in[p + 2] << 16) * 0x9E3779B1u) >> 21;
          s.head[h] = (s.head[h] << 16) | p;
        }
        pos += best_len;
      } else {
        ++s.lfreq[s.in[pos]];
        s.tok[ntok++] = s.in[pos];
        ++pos;
      }
    }
    const bool last_block = pos >= n;
    const uint32_t final_bit = last && last_block ? 1u : 0u;
    s.lfreq[256] = 1;
    // exact costs, the 3 block bits included
    const uint32_t raw = pos - block_start;
    const uint64_t at = w.bitpos();
    const uint64_t cost_stored = 3 + ((8 - ((at + 3) & 7u)) & 7u) + 32 + 8ull * raw;
    uint64_t cost_fixed = 3 + extra_bits;
    for (uint32_t i = 0; i < 286; ++i) cost_fixed += (uint64_t)s.lfreq[i] * fixed_length(i);
    for (uint32_t i = 0; i < 30; ++i) cost_fixed += 5ull * s.dfreq[i];
    code_lengths(s, s.lfreq, 286, 15, s.lens);
    code_lengths(s, s.dfreq, 30, 15, s.lens + 288);
    int nl, nd, ncl, nh;
    uint64_t cost_dynamic = 3 + extra_bits + plan_header(s, &nl, &nd, &ncl, &nh);
    for (uint32_t i = 0; i < 286; ++i) cost_dynamic += (uint64_t)s.lfreq[i] * s.lens[i];
    for (uint32_t i = 0; i < 30; ++i) cost_dynamic += (uint64_t)s.dfreq[i] * s.lens[288 + i];
    const uint64_t cost = cost_stored <= cost_fixed && cost_stored <= cost_dynamic ? cost_stored
                          : cost_fixed <= cost_dynamic ? cost_fixed : cost_dynamic;
    if (at + cost > budget) return kUseStored;              // nothing is written past the chunk's stored form
    if (cost == cost_stored) {
      w.bits(io, final_bit, 3);
      w.align(io);
      w.bits(io, raw, 16);
      w.bits(io, ~raw & 0xFFFFu, 16);
      for (uint32_t i = 0; i < raw; ++i) w.byte(io, s.in[block_start + i]);
    } else if (cost == cost_fixed) {
      w.bits(io, final_bit | 2u, 3);
      for (uint32_t i = 0; i < 288; ++i) s.lens[i] = (uint8_t)fixed_length(i);
      for (uint32_t i = 0; i < 32; ++i) s.lens[288 + i] = 5;
      make_codes(s, s.lens, 288, s.lcode);
      make_codes(s, s.lens + 288, 32, s.dcode);
      write_tokens(io, s, w, ntok, s.lens);
    } else {
      w.bits(io, final_bit | 4u, 3);
      w.bits(io, (uint32_t)(nl - 257), 5);
      w.bits(io, (uint32_t)(nd - 1), 5);
      w.bits(io, (uint32_t)(ncl - 4), 4);
      for (int i = 0; i < ncl; ++i) w.bits(io, s.clen[cl_order(i)], 3);
      for (int k = 0; k < nh; ++k) {
        const uint32_t hs = s.hsym[k];
        w.bits(io, s.ccode[hs], s.clen[hs]);
        if (hs >= 16) w.bits(io, s.hext[k], hs == 16 ? 2 : hs == 17 ? 3 : 7);
      }
      make_codes(s, s.lens, 286, s.lcode);
      make_codes(s, s.lens + 288, 30, s.dcode);
      write_tokens(io, s, w, ntok, s.lens);
    }
    if (last_block) break;
  }
  if (last) {
    w.align(io);
  } else if (w.nbits) {                                     // an empty stored block brings the next chunk to a byte boundary
    w.bits(io, 0, 3);
    w.align(io);
    w.bits(io, 0, 16);
    w.bits(io, 0xFFFFu, 16);
  }
  if (w.overflow || w.pos >= kStoredHeader + n) return kUseStored;
  return w.pos;
}

// the 5 bytes in front of a chunk written stored
TBN_DEF_HD void stored_header(uint32_t n, bool last, uint8_t* h) {
  h[0] = last ? 1 : 0;
  h[1] = (uint8_t)(n & 0xFFu), h[2] = (uint8_t)(n >> 8);
  h[3] = (uint8_t)(~n & 0xFFu), h[4] = (uint8_t)((~n >> 8) & 0xFFu);
}

// ---- the host side ----------------------------------------------------------------------------------------------------
struct HostIO {
  uint8_t* slot;
  void put(uint32_t pos, uint8_t b) { slot[pos] = b; }
};

// One member on the host: n raw bytes at `raw` into the out_cap bytes at `out`.  `s` and `slot` (kSlotData bytes) are
// scratch.  -> status; *out_len: the stream's length.  Nothing is written unless out_cap >= bound(n).  `chunk_end`
// (chunks_of(n) entries, or null): THE CHUNK INDEX, the offset inside the stream at which each chunk's bytes end -- what
// lets a reader inflate the chunks of a member side by side (csrc/inflate.hip, tbn_inflate_chunks); zeros for a refused row.
inline int deflate_member_host(const uint8_t* raw, uint32_t n, uint8_t* out, uint64_t out_cap, State& s, uint8_t* slot,
                               uint64_t* out_len, uint32_t* chunk_end = nullptr) {
  *out_len = 0;
  if (chunk_end)
    for (uint64_t k = 0; k < chunks_of(n); ++k) chunk_end[k] = 0;
  if (out_cap < bound(n)) return TBN_DEF_CAPACITY;
  if (n == 0) {
    out[0] = 0x03, out[1] = 0x00;      // BFINAL, fixed, end of block
    *out_len = 2;
    if (chunk_end) chunk_end[0] = 2;
    return TBN_DEF_OK;
  }
  uint64_t at = 0;
  for (uint32_t begin = 0; begin < n; begin += kChunk) {
    const uint32_t len = n - begin < kChunk ? n - begin : kChunk;
    const bool last = begin + len == n;
    memcpy(s.in, raw + begin, len);
    memset(s.head, 0xFF, sizeof(s.head));
    HostIO io{slot};
    const uint32_t size = compress_chunk(io, s, len, last);
    if (size == kUseStored) {
      stored_header(len, last, out + at);
      memcpy(out + at + kStoredHeader, raw + begin, len);
      at += kStoredHeader + len;
    } else {
      memcpy(out + at, slot, size);
      at += size;
    }
    if (chunk_end) chunk_end[begin / kChunk] = (uint32_t)at;
  }
  *out_len = at;
  return TBN_DEF_OK;
}

}  // namespace tbn_deflate
