// RFC 1951 (raw deflate) decoder core and the zip CRC-32, shared by the kernels in csrc/inflate.hip, their host twins
// tbn_inflate_host / tbn_inflate_chunks_host and the stand-alone memory checks scripts/inflate_check.cpp and
// scripts/inflate_chunks_check.cpp.  Plain C++: no HIP, no global state; the
// core is marked TBN_INF_HD, which is `__host__ __device__` only under hipcc (the way tbn_jpeg_sync.h is shared).
//
// The core is a template over an IO policy that fetches input, stores literals and copies matches; everything that
// DECIDES -- the bit reader, block headers, code-length checks, symbol decoding, and every bound -- is here and is the same
// code on both sides.  The policy only carries out reads and writes the core has already checked.
//
//   IO::in_u32(pos)                 4 stream bytes from `pos`, little endian; bytes at or behind the member's compressed
//                                   length read as 0 (every stream read is clamped to that length)
//   IO::put(pos, byte)              output byte `pos`
//   IO::copy_match(pos, dist, len)  output [pos, pos + len) from [pos - dist, ...), the period replicated when dist < len
//   IO::copy_stored(src, pos, len)  output [pos, pos + len) from stream bytes [src, src + len)
//   IO::leader(), lane(), lanes(), sync()   who writes the tables (one lane), who fills them (all), and the barrier
//   IO::uni(v)                      v, which every lane holds alike, as ONE value (the device keeps it in a scalar
//                                   register, and with it the reader state and every branch of the symbol loop)
//
// Why a damaged stream costs a status and can neither fault nor hang:
//   * every iteration of every loop consumes at least one input bit or produces at least one output byte, or returns:
//     a block header takes 3 bits, a code-length symbol and a literal/length symbol at least 1 bit; the loops over code
//     lengths and table entries have fixed trip counts (<= 320, <= 1024);
//   * bits consumed are compared with 8 * compressed length after every symbol and header field, so the zeros that
//     in_u32 returns behind the end are decoded for at most one symbol before TBN_INF_INPUT;
//   * every store is checked first: pos + len <= declared size (TBN_INF_OUTPUT_FULL), a match source starts at or after
//     output byte 0 (TBN_INF_DISTANCE), a stored block lies inside the compressed bytes (TBN_INF_INPUT);
//   * table indices are masked or bounded by construction: code lengths are 0..15, at most 286 + 30 of them, sorted
//     symbol slots are offsets of a histogram of exactly those lengths, root indices are masked to the root size.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TBN_INF_HD __host__ __device__ __forceinline__
#else
#define TBN_INF_HD inline
#endif

/* status of one member (include/tbn_hip.h documents them for callers) */
#define TBN_INF_OK 0
#define TBN_INF_BLOCK_TYPE 1    /* reserved block type 3 */
#define TBN_INF_STORED_LEN 2    /* stored block: LEN != ~NLEN */
#define TBN_INF_CODE_LENGTHS 3  /* HLIT > 286, HDIST > 30, a repeat with nothing before it or past the end, an
                                   over-subscribed code, or an incomplete one where zlib refuses it */
#define TBN_INF_SYMBOL 4        /* literal/length symbol 286 / 287, distance symbol 30 / 31, or a code no symbol has */
#define TBN_INF_NO_EOB 5        /* a dynamic block without an end-of-block code */
#define TBN_INF_DISTANCE 6      /* a distance before the start of the member's output (segment mode: of the chunk's) */
#define TBN_INF_INPUT 7         /* input exhausted before the final block's end of block */
#define TBN_INF_OUTPUT_FULL 8   /* output would pass the declared size */
#define TBN_INF_OUTPUT_SHORT 9  /* output ends short of the declared size */
#define TBN_INF_CRC 10          /* inflated completely, CRC-32 differs from the directory's */
#define TBN_INF_SKIPPED 11      /* the row carries the skip marker: nothing read, nothing written */
#define TBN_INF_ROW 12          /* the row is inconsistent: a range outside the buffers, a misaligned offset, a method
                                   other than 0 / 8, a size of 2^31 or more */
#define TBN_INF_SEGMENT 13      /* segment mode only: the segment does not end where the chunk index says (input left over,
                                   BFINAL in a chunk that is not the member's last, no BFINAL in the last one) */

namespace tbn_inflate {

constexpr int kRootL = 10;          // literal/length codes of up to 10 bits decode with one lookup
constexpr int kRootD = 8;           // distance codes of up to 8 bits
constexpr int kMaxLens = 320;       // 286 + 30 lengths of a dynamic block; 288 + 32 of the fixed one
// what inflate_stream is given: a whole stream, or one chunk's slice of a stream written by csrc/tbn_deflate.h (chunks
// compressed independently and joined on byte boundaries) -- a chunk that is not the member's last, or the last one
constexpr int kSegWhole = 0, kSegInner = 1, kSegLast = 2;

// decode tables of the current block: 4.2 KB (LDS on the device, the stack on the host)
struct Tables {
  uint16_t lroot[1 << kRootL];      // (symbol << 4) | length, 0: not a code of <= root bits (the count / symbol walk decides)
  uint16_t droot[1 << kRootD];
  uint16_t lsym[288], dsym[32];     // symbols sorted by (length, symbol): canonical order
  uint16_t lcount[16], dcount[16];  // codes per length
  uint16_t code[kMaxLens];          // build scratch: each symbol's canonical code
  uint16_t offs[16], next[16];      // build scratch
  uint8_t lens[kMaxLens];           // code lengths as read
};

struct BitReader {
  uint64_t hold = 0;
  uint32_t nbits = 0;
  uint32_t in_pos = 0;     // next stream byte to fetch
  template <class IO>
  TBN_INF_HD void refill(IO& io) {        // afterwards nbits >= 33
    if (nbits <= 32) {
      hold |= (uint64_t)io.in_u32(in_pos) << nbits;
      in_pos += 4;
      nbits += 32;
    }
  }
  TBN_INF_HD uint32_t peek() const { return (uint32_t)hold; }
  TBN_INF_HD void drop(uint32_t n) {
    hold >>= n;
    nbits -= n;
  }
  TBN_INF_HD uint32_t get(uint32_t n) {    // n <= 16, n == 0 gives 0
    const uint32_t v = (uint32_t)hold & ((1u << n) - 1u);
    drop(n);
    return v;
  }
  TBN_INF_HD bool past(uint32_t clen) const { return (uint64_t)in_pos * 8u - nbits > (uint64_t)clen * 8u; }
};

TBN_INF_HD uint32_t rev_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// Canonical Huffman tables of lens[0, n) (each 0..15).  -> 0: complete; 1: over-subscribed; 2: incomplete (the tables
// are still valid: unused codes decode to -1); 3: incomplete with a single code of length 1; 4: no code at all.
template <class IO>
TBN_INF_HD int build_tables(IO& io, Tables& t, const uint8_t* lens, int n, uint16_t* count, uint16_t* sym, uint16_t* root,
                            int rootbits) {
  io.sync();
  if (io.leader()) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[lens[i] & 15] = (uint16_t)(count[lens[i] & 15] + 1);
    uint32_t c = 0, o = 0;
    t.offs[0] = t.next[0] = 0;
    for (int l = 1; l < 16; ++l) {
      c = (c + (l > 1 ? count[l - 1] : 0u)) << 1;
      t.next[l] = (uint16_t)c;
      t.offs[l] = (uint16_t)o;
      o += count[l];
    }
    for (int i = 0; i < n; ++i) {
      const int l = lens[i] & 15;
      if (l) {
        sym[t.offs[l]] = (uint16_t)i;      // offs[l] < (number of non-zero lengths) <= n
        t.offs[l] = (uint16_t)(t.offs[l] + 1);
        t.code[i] = t.next[l];
        t.next[l] = (uint16_t)(t.next[l] + 1);
      }
    }
  }
  for (int i = io.lane(); i < (1 << rootbits); i += io.lanes()) root[i] = 0;
  io.sync();
  int left = 1, codes = 0, maxlen = 0;
  for (int l = 1; l < 16; ++l) {
    const int cnt = (int)io.uni(count[l]);
    left = (left << 1) - cnt;
    if (left < 0) return 1;
    if (cnt) maxlen = l;
    codes += cnt;
  }
  for (int i = io.lane(); i < n; i += io.lanes()) {
    const int l = lens[i] & 15;
    if (l && l <= rootbits) {
      const uint32_t r = rev_bits(t.code[i] & ((1u << l) - 1u), l);
      for (uint32_t k = r; k < (1u << rootbits); k += 1u << l) root[k] = (uint16_t)((i << 4) | l);
    }
  }
  io.sync();
  if (codes == 0) return 4;
  if (left > 0) return maxlen == 1 ? 3 : 2;
  return 0;
}

// one symbol; -1: the bits are no code (possible only in an incomplete set).  Needs 15 bits in the reader.
template <class IO>
TBN_INF_HD int decode_symbol(IO& io, BitReader& br, const uint16_t* root, int rootbits, const uint16_t* count,
                             const uint16_t* sym) {
  const uint32_t bits = br.peek();
  const uint32_t e = io.uni(root[bits & ((1u << rootbits) - 1u)]);
  if (e & 15u) {
    br.drop(e & 15u);
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int len = 1; len <= 15; ++len) {
    code |= (int)((bits >> (len - 1)) & 1u);
    const int cnt = (int)io.uni(count[len]);
    if (code - cnt < first) {
      br.drop((uint32_t)len);
      return (int)io.uni(sym[index + (code - first)]);
    }
    index += cnt;
    first += cnt;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

// the order in which the code-length code's lengths are stored (RFC 1951, 3.2.7), 5 bits each
constexpr uint64_t pack_order(const int* o, int from, int to) {
  uint64_t v = 0;
  for (int i = from; i < to; ++i) v |= (uint64_t)o[i] << (5 * (i - from));
  return v;
}
constexpr int kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
constexpr uint64_t kClOrderLo = pack_order(kClOrder, 0, 12), kClOrderHi = pack_order(kClOrder, 12, 19);
TBN_INF_HD int cl_order(int i) { return (int)(((i < 12 ? kClOrderLo >> (5 * i) : kClOrderHi >> (5 * (i - 12)))) & 31u); }

// Inflates one raw deflate stream of `clen` bytes into exactly `declared` bytes.  -> status; *produced: bytes written.
// SEGMENT MODE (`seg` != kSegWhole): the `clen` bytes are one chunk's slice and output byte 0 is the chunk's first byte, so
// a distance reaching before the chunk is TBN_INF_DISTANCE like any distance before the output: a wrong index, or a
// foreign stream carrying an index, costs a status.
//   kSegInner  a run of non-final blocks.  Ends OK exactly when a block ends with ALL 8 * clen bits consumed (the writer
//              ends the chunk on a byte boundary, with an empty stored block where its last block does not) and
//              `declared` bytes produced; a block that sets BFINAL is TBN_INF_SEGMENT.
//   kSegLast   ends at BFINAL as a whole stream does; then nothing but zero padding may follow in the last byte, and that
//              byte is byte clen - 1, or the status is TBN_INF_SEGMENT.  So is a non-final block that ends with all
//              input consumed.
// Every other status and every bound is the whole stream's: the checks below do not depend on the mode.
template <class IO>
TBN_INF_HD int inflate_stream(IO& io, Tables& t, uint32_t clen, uint32_t declared, uint32_t* produced, int seg = kSegWhole) {
  BitReader br;
  uint32_t pos = 0;
  *produced = 0;
  for (;;) {
    br.refill(io);
    const uint32_t bfinal = br.get(1), type = br.get(2);
    if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
    if (seg == kSegInner && bfinal) return *produced = pos, TBN_INF_SEGMENT;
    if (type == 3) return *produced = pos, TBN_INF_BLOCK_TYPE;
    if (type == 0) {
      br.drop(br.nbits & 7u);
      br.refill(io);
      const uint32_t len = br.get(16), nlen = br.get(16);
      if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
      if (len != (~nlen & 0xFFFFu)) return *produced = pos, TBN_INF_STORED_LEN;
      const uint32_t src = br.in_pos - br.nbits / 8u;       // nbits is a multiple of 8 here
      if ((uint64_t)src + len > clen) return *produced = pos, TBN_INF_INPUT;
      if (len > declared - pos) return *produced = pos, TBN_INF_OUTPUT_FULL;
      if (len) io.copy_stored(src, pos, len);
      pos += len;
      br.hold = 0;
      br.nbits = 0;
      br.in_pos = src + len;
    } else {
      int nl, nd;
      if (type == 1) {
        nl = 288;
        nd = 32;
        io.sync();
        if (io.leader()) {
          for (int i = 0; i < 288; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
          for (int i = 288; i < 320; ++i) t.lens[i] = 5;
        }
      } else {
        br.refill(io);
        nl = (int)br.get(5) + 257;
        nd = (int)br.get(5) + 1;
        const int ncl = (int)br.get(4) + 4;
        if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
        if (nl > 286 || nd > 30) return *produced = pos, TBN_INF_CODE_LENGTHS;
        io.sync();
        if (io.leader())
          for (int i = 0; i < 19; ++i) t.lens[i] = 0;
        for (int i = 0; i < ncl; ++i) {
          br.refill(io);
          const uint32_t v = br.get(3);
          if (io.leader()) t.lens[cl_order(i)] = (uint8_t)v;
        }
        if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
        // the code-length code must be complete (zlib: type CODES)
        if (build_tables(io, t, t.lens, 19, t.lcount, t.lsym, t.lroot, 7) != 0) return *produced = pos, TBN_INF_CODE_LENGTHS;
        const int total = nl + nd;
        int i = 0;
        uint32_t prev = 0;
        while (i < total) {
          br.refill(io);
          const int s = decode_symbol(io, br, t.lroot, 7, t.lcount, t.lsym);
          if (s < 0) return *produced = pos, TBN_INF_CODE_LENGTHS;
          uint32_t v = (uint32_t)s;
          int rep = 1;
          if (s == 16) {
            if (i == 0) return *produced = pos, TBN_INF_CODE_LENGTHS;
            v = prev;
            rep = 3 + (int)br.get(2);
          } else if (s == 17) {
            v = 0;
            rep = 3 + (int)br.get(3);
          } else if (s == 18) {
            v = 0;
            rep = 11 + (int)br.get(7);
          }
          if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
          if (i + rep > total) return *produced = pos, TBN_INF_CODE_LENGTHS;
          // a repeat may run from the literal/length lengths into the distance lengths: they are one sequence
          if (io.leader())
            for (int k = 0; k < rep; ++k) t.lens[i + k] = (uint8_t)v;
          i += rep;
          prev = v;
        }
        io.sync();
        if (io.uni(t.lens[256]) == 0) return *produced = pos, TBN_INF_NO_EOB;
      }
      // zlib accepts an incomplete set only when it is a single code of length 1; no distance code at all is fine too
      // (a block of literals only)
      const int rl = build_tables(io, t, t.lens, nl, t.lcount, t.lsym, t.lroot, kRootL);
      if (rl == 1 || rl == 2 || rl == 4) return *produced = pos, TBN_INF_CODE_LENGTHS;
      const int rd = build_tables(io, t, t.lens + nl, nd, t.dcount, t.dsym, t.droot, kRootD);
      if (rd == 1 || rd == 2) return *produced = pos, TBN_INF_CODE_LENGTHS;
      for (;;) {
        br.refill(io);
        int s = decode_symbol(io, br, t.lroot, kRootL, t.lcount, t.lsym);
        if (s < 0) return *produced = pos, br.past(clen) ? TBN_INF_INPUT : TBN_INF_SYMBOL;
        if (s < 256) {
          if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
          if (pos >= declared) return *produced = pos, TBN_INF_OUTPUT_FULL;
          io.put(pos, (uint8_t)s);
          ++pos;
          continue;
        }
        if (s == 256) {
          if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
          break;
        }
        s -= 257;
        if (s >= 29) return *produced = pos, br.past(clen) ? TBN_INF_INPUT : TBN_INF_SYMBOL;
        uint32_t len;
        if (s < 8) {
          len = 3u + (uint32_t)s;
        } else if (s == 28) {
          len = 258;
        } else {
          const uint32_t e = ((uint32_t)s >> 2) - 1u;
          len = 3u + ((4u + ((uint32_t)s & 3u)) << e) + br.get(e);
        }
        br.refill(io);
        const int d = decode_symbol(io, br, t.droot, kRootD, t.dcount, t.dsym);
        if (d < 0 || d >= 30) return *produced = pos, br.past(clen) ? TBN_INF_INPUT : TBN_INF_SYMBOL;
        uint32_t dist;
        if (d < 4) {
          dist = 1u + (uint32_t)d;
        } else {
          const uint32_t e = ((uint32_t)d >> 1) - 1u;
          dist = 1u + ((2u + ((uint32_t)d & 1u)) << e) + br.get(e);
        }
        if (br.past(clen)) return *produced = pos, TBN_INF_INPUT;
        if (dist > pos) return *produced = pos, TBN_INF_DISTANCE;
        if (len > declared - pos) return *produced = pos, TBN_INF_OUTPUT_FULL;
        io.copy_match(pos, dist, len);
        pos += len;
      }
    }
    if (bfinal) break;
    if (seg != kSegWhole && (uint64_t)br.in_pos * 8u - br.nbits == (uint64_t)clen * 8u) {     // a block ended at the slice's end
      if (seg == kSegLast) return *produced = pos, TBN_INF_SEGMENT;
      *produced = pos;
      return pos == declared ? TBN_INF_OK : TBN_INF_OUTPUT_SHORT;
    }
  }
  *produced = pos;
  if (seg == kSegLast) {
    // the final block ended inside byte clen - 1 (in_pos * 8 is a multiple of 8: nbits & 7 bits of that byte are left)
    const uint64_t used = (uint64_t)br.in_pos * 8u - br.nbits;
    const uint32_t pad = br.nbits & 7u;
    if ((used + 7u) / 8u != clen || ((uint32_t)br.hold & ((1u << pad) - 1u)) != 0) return TBN_INF_SEGMENT;
  }
  return pos == declared ? TBN_INF_OK : TBN_INF_OUTPUT_SHORT;
}

// ---- CRC-32 of the zip format (reflected polynomial 0xEDB88320), in chunks that are combined afterwards ----------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;

TBN_INF_HD uint32_t crc_table_entry(uint32_t i) {
  uint32_t c = i;
  for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}
// a * b mod P, both reflected (bit 31 is x^0)
TBN_INF_HD uint32_t crc_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    if (a & (0x80000000u >> i)) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
  }
  return p;
}
// x^(8 * nbytes) mod P
TBN_INF_HD uint32_t crc_x8pow(uint64_t nbytes) {
  uint32_t p = 0x80000000u, base = 0x00800000u;     // x^0, x^8
  while (nbytes) {
    if (nbytes & 1u) p = crc_mulmod(p, base);
    base = crc_mulmod(base, base);
    nbytes >>= 1;
  }
  return p;
}
// the CRC-32 of chunk [begin, end) of a message of n bytes, moved to its place in the whole: the CRC of the message is the
// XOR of these over any partition into chunks (CRCs are linear: crc(A || B) = crc(A) * x^(8 |B|) + crc(B))
TBN_INF_HD uint32_t crc_chunk(const uint8_t* data, uint32_t begin, uint32_t end, uint32_t n, const uint32_t* table) {
  if (begin >= end) return 0;
  uint32_t c = 0xFFFFFFFFu;
  for (uint32_t i = begin; i < end; ++i) c = table[(c ^ data[i]) & 0xFFu] ^ (c >> 8);
  c ^= 0xFFFFFFFFu;
  return end == n ? c : crc_mulmod(crc_x8pow((uint64_t)(n - end)), c);
}
constexpr uint32_t kCrcChunks = 256;    // chunks per member: the threads of the CRC kernel
TBN_INF_HD uint32_t crc_chunk_len(uint32_t n) { return (n + kCrcChunks - 1) / kCrcChunks; }

// ---- the host side: plain buffers -------------------------------------------------------------------------------------
struct HostIO {
  const uint8_t* in;
  uint32_t clen;
  uint8_t* out;
  bool leader() const { return true; }
  int lane() const { return 0; }
  int lanes() const { return 1; }
  uint32_t uni(uint32_t v) const { return v; }
  void sync() {}
  uint32_t in_u32(uint32_t pos) const {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if ((uint64_t)pos + k < clen) v |= (uint32_t)in[pos + k] << (8 * k);
    return v;
  }
  void put(uint32_t pos, uint8_t b) { out[pos] = b; }
  void copy_match(uint32_t pos, uint32_t dist, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos - dist + i];
  }
  void copy_stored(uint32_t src, uint32_t pos, uint32_t len) { memcpy(out + pos, in + src, len); }
};

// the zip CRC-32 of out[0, n) in kCrcChunks chunks, as inflate_crc_kernel computes it
inline uint32_t crc_member_host(const uint8_t* out, uint32_t n) {
  uint32_t table[256];
  for (uint32_t i = 0; i < 256; ++i) table[i] = crc_table_entry(i);
  const uint32_t chunk = crc_chunk_len(n);
  uint32_t c = 0;
  for (uint32_t k = 0; k < kCrcChunks; ++k) {
    const uint64_t b = (uint64_t)k * chunk, e = b + chunk;
    c ^= crc_chunk(out, (uint32_t)(b < n ? b : n), (uint32_t)(e < n ? e : n), n, table);
  }
  return c;
}

// One chunk's slice on the host (segment mode): `clen` bytes at `in` into `declared` bytes at `out`.
inline int inflate_chunk_host(const uint8_t* in, uint32_t clen, uint8_t* out, uint32_t declared, bool last, uint32_t* produced) {
  Tables t;
  HostIO io{in, clen, out};
  return inflate_stream(io, t, clen, declared, produced, last ? kSegLast : kSegInner);
}

// One member on the host: method 0 (stored) or 8 (deflate), `clen` bytes at `in` into `declared` bytes at `out`, then the
// CRC in kCrcChunks chunks as the kernel computes it.  -> status; *produced: bytes written.
inline int inflate_member_host(const uint8_t* in, uint32_t clen, uint32_t method, uint8_t* out, uint32_t declared,
                               uint32_t crc, uint32_t* produced) {
  *produced = 0;
  int st;
  if (method == 0) {
    if (clen > declared) return TBN_INF_OUTPUT_FULL;
    if (clen) memcpy(out, in, clen);
    *produced = clen;
    st = clen == declared ? TBN_INF_OK : TBN_INF_OUTPUT_SHORT;
  } else if (method == 8) {
    Tables t;
    HostIO io{in, clen, out};
    st = inflate_stream(io, t, clen, declared, produced);
  } else {
    return TBN_INF_ROW;
  }
  if (st != TBN_INF_OK) return st;
  return crc_member_host(out, declared) == crc ? TBN_INF_OK : TBN_INF_CRC;
}

}  // namespace tbn_inflate
