// Flow pickles on the device: the members of a batch of .npz files (zip members, stored or raw deflate, RFC 1951) are
// inflated by ONE launch, one wavefront per member, and their CRC-32 is checked by a second launch over the staged bytes.
// Replaces np.load of reference core/dataset/dataset.py:342-343.  The decoder core -- every decision and every bound -- is
// csrc/tbn_inflate.h, the same code the host twin tbn_inflate_host and scripts/inflate_check.cpp run.
//
// inflate_kernel, 64 threads (one wavefront) per member.  The bit buffer and the symbol loop are wave-uniform: every lane
// holds the same reader state (in scalar registers: DevIO::uni) and takes the same branches, so every fence is reached
// by all lanes and every early exit is workgroup-uniform.  What the lanes share out:
//   * the compressed bytes come through an 8-KB LDS ring filled 4 KB at a time by all lanes (dword loads, clamped to the
//     member's compressed length; what lies behind it reads as zero);
//   * the decode tables (tbn_inflate::Tables, 4.2 KB of LDS) are rebuilt at each block: lane 0 sorts the symbols, all lanes
//     fill the root tables;
//   * a match is copied by all lanes at once, the period replicated when distance < length; a stored block likewise.
// The last 64 KB of output live in an LDS ring as well: it is the LZ77 window (distances reach 32 768, a match is at most
// 258 bytes, so a match's source and destination never alias in the ring).  LDS operations of one wavefront complete in
// order, so a match reads what the previous symbol wrote without waiting for a global store to become visible; the
// global staging buffer is only ever written here, in stream order.  76 KB of LDS: two members per CU.
//
// inflate_chunk_kernel, 64 threads (one wavefront) per CHUNK of a member that carries a chunk index (tbn_inflate_chunks):
// streams written by csrc/tbn_deflate.h are chunks of 32 KB raw bytes compressed independently and joined on byte
// boundaries, and the index (a zip extra field, core/dataset/npz_file.py) says where each chunk's bytes end, so a stack of
// 1.1 MB is 36 wavefronts instead of one.  The same core in segment mode (tbn_inflate.h), the same ring and tables; what
// differs is ChunkIO: the slice starts at ANY byte offset (aligned dword loads, shifted, clamped to the slice), the
// window is the chunk itself (32 KB: a distance before the chunk is status 6), and the finished chunk is flushed from the
// window to global memory by all lanes -- dwords when the destination is 4-byte aligned -- so the symbol loop issues no
// global store at all.  With a ring of 2 x 1 KB that is 38.2 KB of LDS: four workgroups per CU, a wavefront per SIMD.  inflate_fold_kernel then makes a member's status (the
// first non-zero chunk status in chunk order, 12 for a chunk range that does not tile the member) and info (the sum),
// and inflate_crc_kernel proves the bytes whatever the index said.
//
// crc_kernel, 256 threads per member: the 256-entry table in LDS, one chunk of equal length per thread, each chunk's CRC
// multiplied by x^(8 * bytes behind it) mod P and XOR-reduced; a mismatch turns status 0 into TBN_INF_CRC.  The body is
// crc_workgroup (csrc/tbn_crc_dev.h), which deflate_crc_kernel of csrc/deflate.hip calls too.
#include "tbn_common.h"
#include "tbn_crc_dev.h"
#include "tbn_deflate.h"
#include "tbn_inflate.h"
#include "tbn_inflate_dev.h"
#include "../../include/tbn_hip.h"

using namespace tbn_inflate;

static_assert(sizeof(tbn_inflate_member) == 40, "the member row is 40 bytes");
static_assert(sizeof(tbn_inflate_chunk) == 32, "the chunk row is 32 bytes");

namespace {

// true when the row may be read and written as it says
__host__ __device__ __forceinline__ bool row_ok(const tbn_inflate_member& m, size_t in_bytes, size_t out_bytes) {
  return (m.method == 0 || m.method == 8) && m.in_len < (1u << 31) && m.out_len < (1u << 31) && (m.in_off & 3u) == 0 &&
         m.in_off <= in_bytes && m.in_len <= in_bytes - m.in_off && m.out_off <= out_bytes && m.out_len <= out_bytes - m.out_off;
}

__global__ __launch_bounds__(kInfThreads) void inflate_kernel(const uint8_t* __restrict__ in, size_t in_bytes,
                                                              const tbn_inflate_member* __restrict__ members,
                                                              uint8_t* __restrict__ out, size_t out_bytes,
                                                              int* __restrict__ status, int* __restrict__ info) {
  __shared__ Tables tables;
  __shared__ uint32_t ring[2 * kChunk / 4];
  __shared__ uint8_t win[kWin];
  const int m_no = blockIdx.x, ln = threadIdx.x;
  const tbn_inflate_member m = members[m_no];
  int st;
  uint32_t produced = 0;
  if (m.skip) {                                   // every branch here depends on the row alone: workgroup-uniform
    st = TBN_INF_SKIPPED;
  } else if (!row_ok(m, in_bytes, out_bytes)) {
    st = TBN_INF_ROW;
  } else if (m.method == 0) {
    if (m.in_len > m.out_len) {
      st = TBN_INF_OUTPUT_FULL;
    } else {
      const uint8_t* src = in + m.in_off;
      uint8_t* dst = out + m.out_off;
      for (uint32_t i = (uint32_t)ln; i < m.in_len; i += kInfThreads) dst[i] = src[i];
      produced = m.in_len;
      st = m.in_len == m.out_len ? TBN_INF_OK : TBN_INF_OUTPUT_SHORT;
    }
  } else {
    DevIO io{in + m.in_off, m.in_len, out + m.out_off, win, ring, kNoBase, ln};
    st = inflate_stream(io, tables, m.in_len, m.out_len, &produced);
  }
  if (ln == 0) {
    status[m_no] = st;
    info[m_no] = (int)produced;
  }
}

// ---- chunk-indexed members ---------------------------------------------------------------------------------------------
constexpr uint32_t kSeg = 32768;           // raw bytes per chunk = tbn_deflate_chunk(): the window of one chunk
// The A/B arm of profiles/flow_pickle_chunks.md, never the shipped build (TBN_EXTRA_FLAGS=-DTBN_INFLATE_CHUNK_DIRECT_STORES
// with TBN_BUILD_VARIANT): every literal and match also goes to global memory as it is decoded, as inflate_kernel does it,
// and there is no flush.
#ifdef TBN_INFLATE_CHUNK_DIRECT_STORES
constexpr bool kChunkDirectStores = true;
#else
constexpr bool kChunkDirectStores = false;
#endif
// the input ring of a chunk: two halves of 1 KB (inflate_kernel: 4 KB).  With Tables and the window that is 39 104 bytes of
// LDS, FOUR workgroups per CU -- one wavefront for each SIMD; with 4-KB halves it is three, and a SIMD of every CU idles
// (profiles/flow_pickle_chunks.md).
constexpr uint32_t kSegRing = 1024;
static_assert(kSeg == tbn_deflate::kChunk && (kSeg & (kSeg - 1)) == 0, "the writer's chunk; window positions are masked");

struct ChunkIO {
  const uint8_t* in;       // the whole packed buffer (4-byte aligned)
  uint64_t lo, hi;         // the slice: bytes [lo, hi) of `in`; nothing else is read
  uint8_t* win;            // LDS, kSeg bytes: the chunk's output
  uint32_t* ring;          // LDS, 2 * kSegRing bytes
  uint32_t base;           // slice offset of the older resident ring chunk
  int ln;
  uint8_t* out;            // the chunk's bytes in global memory: written by flush() (or, in the A/B build, as they are decoded)

  __device__ __forceinline__ bool leader() const { return ln == 0; }
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return kInfThreads; }
  __device__ __forceinline__ uint32_t uni(uint32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
  __device__ __forceinline__ void sync() {                 // as DevIO::sync
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // the dword at byte offset g of `in` (g a multiple of 4, any value): bytes outside the slice read as zero and are not read
  __device__ __forceinline__ uint32_t fetch(uint64_t g) const {
    if (g >= lo && g + 4 <= hi) return *(const uint32_t*)(in + g);
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k)
      if (g + k >= lo && g + k < hi) v |= (uint32_t)in[g + k] << (8 * k);
    return v;
  }
  __device__ __forceinline__ void load_chunk(uint32_t cb) {      // slice bytes [cb, cb + kSegRing) into their ring slot
    uint32_t* slot = ring + (cb & (2 * kSegRing - 1)) / 4;
    const uint32_t a = (uint32_t)lo & 3u;                         // the slice starts `a` bytes into an aligned dword
    const uint64_t g0 = (lo - a) + cb;
    for (uint32_t i = (uint32_t)ln; i < kSegRing / 4; i += kInfThreads) {
      const uint64_t g = g0 + 4ull * i;
      uint32_t v = 0;
      if (g < hi) {
        v = fetch(g);
        if (a) v = (v >> (8 * a)) | (fetch(g + 4) << (32 - 8 * a));
      }
      slot[i] = v;
    }
  }
  __device__ __forceinline__ uint32_t in_u32(uint32_t pos) {     // as DevIO::in_u32
    const uint32_t want = pos & ~(kSegRing - 1);
    if (want != base) {
      sync();
      if (base != kNoBase && want == base + kSegRing) {
        load_chunk(want + kSegRing);
      } else {
        load_chunk(want);
        load_chunk(want + kSegRing);
      }
      base = want;
      sync();
    }
    const uint32_t w = (pos & (2 * kSegRing - 1)) >> 2;
    const uint64_t two = (uint64_t)ring[w] | ((uint64_t)ring[(w + 1) & (2 * kSegRing / 4 - 1)] << 32);
    return uni((uint32_t)(two >> (8 * (pos & 3u))));
  }
  // the core has checked pos + len <= declared <= kSeg and dist <= pos; the masks keep a slip inside the window
  __device__ __forceinline__ void store(uint32_t pos, uint8_t b) {
    win[pos & (kSeg - 1)] = b;
    if (kChunkDirectStores) out[pos] = b;
  }
  __device__ __forceinline__ void put(uint32_t pos, uint8_t b) {
    if (ln == 0) store(pos, b);
  }
  __device__ __forceinline__ void copy_match(uint32_t pos, uint32_t dist, uint32_t len) {
    sync();
    const uint32_t from = pos - dist;
    if (dist >= len) {
      for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) store(pos + i, win[(from + i) & (kSeg - 1)]);
    } else {
      for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) store(pos + i, win[(from + i % dist) & (kSeg - 1)]);
    }
    sync();
  }
  __device__ __forceinline__ void copy_stored(uint32_t src, uint32_t pos, uint32_t len) {     // [src, src + len) is inside the slice
    sync();
    for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) store(pos + i, in[lo + src + i]);
    sync();
  }
  // the finished chunk from the window to global memory, by all lanes: dwords when the destination is 4-byte aligned.
  // produced <= the chunk's out_len <= kSeg, and [out, out + out_len) is inside the member's slot.
  __device__ __forceinline__ void flush(uint32_t produced) {
    sync();
    if (kChunkDirectStores) return;
    if (((uintptr_t)out & 3) == 0) {
      const uint32_t words = produced / 4;
      for (uint32_t i = (uint32_t)ln; i < words; i += kInfThreads) ((uint32_t*)out)[i] = ((const uint32_t*)win)[i];
      for (uint32_t i = 4 * words + (uint32_t)ln; i < produced; i += kInfThreads) out[i] = win[i];
    } else {
      for (uint32_t i = (uint32_t)ln; i < produced; i += kInfThreads) out[i] = win[i];
    }
  }
};

// What chunk row c may do, from the tables alone: 0 inflate it; 11 its member is skipped; 12 the row, its member's row or
// its place among the member's chunks is inconsistent.  Status 0 for all chunks of a member's range means: they tile the
// member's compressed bytes and its output exactly, in order, and only the last one is marked last.
__host__ __device__ __forceinline__ int chunk_row_status(const tbn_inflate_member* members, int n_members,
                                                         const tbn_inflate_chunk* chunks, const uint32_t* chunk_begin,
                                                         int n_chunks, uint32_t c, size_t in_bytes, size_t out_bytes) {
  const tbn_inflate_chunk ch = chunks[c];
  if (ch.member >= (uint32_t)n_members) return TBN_INF_ROW;
  const tbn_inflate_member m = members[ch.member];
  if (m.skip) return TBN_INF_SKIPPED;
  if (!row_ok(m, in_bytes, out_bytes) || m.method != 8) return TBN_INF_ROW;
  const uint32_t b = chunk_begin[ch.member], e = chunk_begin[ch.member + 1];
  const uint32_t count = m.out_len == 0 ? 1u : (m.out_len + kSeg - 1) / kSeg;
  if (b > e || e > (uint32_t)n_chunks || e - b != count || c < b || c >= e) return TBN_INF_ROW;
  const uint32_t k = c - b;
  const bool last = k + 1 == count;
  const uint32_t want_len = last ? m.out_len - k * kSeg : kSeg;
  if (ch.out_off != m.out_off + (uint64_t)k * kSeg || ch.out_len != want_len || (ch.last != 0) != last) return TBN_INF_ROW;
  // the slices follow each other from the member's first byte to its last
  uint64_t start = m.in_off;
  if (k > 0) {
    const tbn_inflate_chunk prev = chunks[c - 1];
    start = prev.in_off + prev.in_len;
  }
  if (ch.in_off != start || ch.in_off < m.in_off || ch.in_off > m.in_off + m.in_len ||
      ch.in_len > m.in_off + m.in_len - ch.in_off)
    return TBN_INF_ROW;
  if (last && ch.in_off + ch.in_len != m.in_off + m.in_len) return TBN_INF_ROW;
  return TBN_INF_OK;
}

// A member's chunk range [*b, *e) for the fold of its chunks' statuses (chunk_status[n_chunks], then the bytes each
// produced); 11 / 12: there is nothing to fold.
__host__ __device__ __forceinline__ int fold_range(const tbn_inflate_member& m, const uint32_t* chunk_begin, int m_no,
                                                   int n_chunks, uint32_t* b, uint32_t* e) {
  if (m.skip) return TBN_INF_SKIPPED;
  *b = chunk_begin[m_no], *e = chunk_begin[m_no + 1];
  if (*b >= *e || *e > (uint32_t)n_chunks) return TBN_INF_ROW;
  return TBN_INF_OK;
}

__global__ __launch_bounds__(kInfThreads) void inflate_chunk_kernel(const uint8_t* __restrict__ in, size_t in_bytes,
                                                                    const tbn_inflate_member* __restrict__ members, int n_members,
                                                                    const tbn_inflate_chunk* __restrict__ chunks,
                                                                    const uint32_t* __restrict__ chunk_begin, int n_chunks,
                                                                    uint8_t* __restrict__ out, size_t out_bytes,
                                                                    int* __restrict__ chunk_status) {
  __shared__ Tables tables;
  __shared__ uint32_t ring[2 * kSegRing / 4];
  __shared__ __attribute__((aligned(16))) uint8_t win[kSeg];
  const uint32_t c = blockIdx.x;
  const int ln = threadIdx.x;
  // every branch here depends on the tables alone: workgroup-uniform
  int st = chunk_row_status(members, n_members, chunks, chunk_begin, n_chunks, c, in_bytes, out_bytes);
  uint32_t produced = 0;
  if (st == TBN_INF_OK) {
    const tbn_inflate_chunk ch = chunks[c];
    ChunkIO io{in, ch.in_off, ch.in_off + ch.in_len, win, ring, kNoBase, ln, out + ch.out_off};
    st = inflate_stream(io, tables, ch.in_len, ch.out_len, &produced, ch.last ? kSegLast : kSegInner);
    io.flush(produced);
  }
  if (ln == 0) {
    chunk_status[c] = st;
    chunk_status[n_chunks + c] = (int)produced;
  }
}

__global__ __launch_bounds__(kInfThreads) void inflate_fold_kernel(const tbn_inflate_member* __restrict__ members,
                                                                   const tbn_inflate_chunk* __restrict__ chunks,
                                                                   const uint32_t* __restrict__ chunk_begin, int n_chunks,
                                                                   const int* __restrict__ chunk_status, int* __restrict__ status,
                                                                   int* __restrict__ info) {
  const int m_no = blockIdx.x, ln = threadIdx.x;
  const tbn_inflate_member m = members[m_no];
  uint32_t b = 0, e = 0;
  int st = fold_range(m, chunk_begin, m_no, n_chunks, &b, &e);       // one value for the wavefront
  uint32_t first = 0xFFFFFFFFu, bytes = 0;
  if (st == TBN_INF_OK) {
    for (uint32_t c = b + (uint32_t)ln; c < e; c += kInfThreads) {
      const bool mine = chunks[c].member == (uint32_t)m_no;
      if ((!mine || chunk_status[c] != 0) && c - b < first) first = c - b;
      if (mine) bytes += (uint32_t)chunk_status[n_chunks + c];
    }
    for (int o = kInfThreads / 2; o > 0; o >>= 1) {
      const uint32_t f = __shfl_xor(first, o, kInfThreads), s = __shfl_xor(bytes, o, kInfThreads);
      first = f < first ? f : first;
      bytes += s;
    }
    if (first != 0xFFFFFFFFu) st = chunks[b + first].member == (uint32_t)m_no ? chunk_status[b + first] : TBN_INF_ROW;
  }
  if (ln == 0) {
    status[m_no] = st;
    info[m_no] = (int)bytes;
  }
}

__global__ __launch_bounds__(kCrcThreads) void inflate_crc_kernel(const tbn_inflate_member* __restrict__ members,
                                                                  const uint8_t* __restrict__ out, int* __restrict__ status) {
  __shared__ uint32_t table[256];
  __shared__ uint32_t part[kCrcThreads];
  const int m_no = blockIdx.x;
  const tbn_inflate_member m = members[m_no];
  const bool run = status[m_no] == TBN_INF_OK;       // one value for the workgroup: the inflate launch has completed
  // status 0: the row was checked and out_len bytes were written
  const uint32_t crc = crc_workgroup(out + m.out_off, m.out_len, run, table, part);     // csrc/tbn_crc_dev.h
  if (threadIdx.x == 0 && run && crc != m.crc) status[m_no] = TBN_INF_CRC;
}

int check_args(const char* fn, const void* in, size_t in_bytes, const tbn_inflate_member* members, int n, const void* out,
               const int* status, const int* info) {
  TBN_REQUIRE(n >= 0, "%s: n_members %d is negative", fn, n);
  if (n == 0) return TBN_OK;
  TBN_REQUIRE(in != nullptr && members != nullptr && out != nullptr && status != nullptr && info != nullptr,
              "%s: null argument", fn);
  TBN_REQUIRE(((uintptr_t)in & 3) == 0 && ((uintptr_t)members & 7) == 0 && ((uintptr_t)status & 3) == 0 &&
                  ((uintptr_t)info & 3) == 0, "%s: `in`, status and info must be 4-byte aligned, the member table 8-byte aligned", fn);
  (void)in_bytes;
  return TBN_OK;
}

}  // namespace

extern "C" int tbn_inflate_batch(const void* in_dev, size_t in_bytes, const tbn_inflate_member* members_dev, int n_members,
                                 void* out_dev, size_t out_bytes, int* status_dev, int* info_dev, void* stream) {
  const char* fn = "inflate_batch";
  const int rc = check_args(fn, in_dev, in_bytes, members_dev, n_members, out_dev, status_dev, info_dev);
  if (rc != TBN_OK || n_members == 0) return rc;
  hipStream_t st = (hipStream_t)stream;
  TBN_KLAUNCH(inflate_kernel, dim3((unsigned)n_members), dim3(kInfThreads), 0, st, (const uint8_t*)in_dev, in_bytes, members_dev,
              (uint8_t*)out_dev, out_bytes, status_dev, info_dev);
  TBN_CHECK_LAUNCH(fn);
  TBN_KLAUNCH(inflate_crc_kernel, dim3((unsigned)n_members), dim3(kCrcThreads), 0, st, members_dev, (const uint8_t*)out_dev,
              status_dev);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}

// the host twin: the same core, serially, over the same member table; no GPU call
extern "C" int tbn_inflate_host(const void* in, size_t in_bytes, const tbn_inflate_member* members, int n_members, void* out,
                                size_t out_bytes, int* status, int* info) {
  const char* fn = "inflate_host";
  const int rc = check_args(fn, in, in_bytes, members, n_members, out, status, info);
  if (rc != TBN_OK) return rc;
  for (int i = 0; i < n_members; ++i) {
    const tbn_inflate_member& m = members[i];
    uint32_t produced = 0;
    int st;
    if (m.skip) {
      st = TBN_INF_SKIPPED;
    } else if (!row_ok(m, in_bytes, out_bytes)) {
      st = TBN_INF_ROW;
    } else {
      st = inflate_member_host((const uint8_t*)in + m.in_off, m.in_len, m.method, (uint8_t*)out + m.out_off, m.out_len, m.crc,
                               &produced);
    }
    status[i] = st;
    info[i] = (int)produced;
  }
  return TBN_OK;
}

// ---- chunk-indexed members: one wavefront per chunk --------------------------------------------------------------------
static int check_chunk_args(const char* fn, const tbn_inflate_chunk* chunks, const uint32_t* chunk_begin, int n_chunks,
                            const int* chunk_status) {
  TBN_REQUIRE(n_chunks >= 0, "%s: n_chunks %d is negative", fn, n_chunks);
  TBN_REQUIRE(chunk_begin != nullptr && ((uintptr_t)chunk_begin & 3) == 0, "%s: chunk_begin must be a 4-byte aligned array", fn);
  TBN_REQUIRE(n_chunks == 0 || (chunks != nullptr && chunk_status != nullptr && ((uintptr_t)chunks & 7) == 0 &&
                                ((uintptr_t)chunk_status & 3) == 0),
              "%s: the chunk table must be 8-byte aligned, chunk_status 4-byte aligned", fn);
  return TBN_OK;
}

extern "C" int tbn_inflate_chunks(const void* in_dev, size_t in_bytes, const tbn_inflate_member* members_dev, int n_members,
                                  const tbn_inflate_chunk* chunks_dev, const uint32_t* chunk_begin_dev, int n_chunks,
                                  void* out_dev, size_t out_bytes, int* status_dev, int* info_dev, int* chunk_status_dev,
                                  void* stream) {
  const char* fn = "inflate_chunks";
  int rc = check_args(fn, in_dev, in_bytes, members_dev, n_members, out_dev, status_dev, info_dev);
  if (rc != TBN_OK || n_members == 0) return rc;
  rc = check_chunk_args(fn, chunks_dev, chunk_begin_dev, n_chunks, chunk_status_dev);
  if (rc != TBN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (n_chunks > 0) {
    TBN_KLAUNCH(inflate_chunk_kernel, dim3((unsigned)n_chunks), dim3(kInfThreads), 0, st, (const uint8_t*)in_dev, in_bytes, members_dev,
                n_members, chunks_dev, chunk_begin_dev, n_chunks, (uint8_t*)out_dev, out_bytes, chunk_status_dev);
    TBN_CHECK_LAUNCH(fn);
  }
  TBN_KLAUNCH(inflate_fold_kernel, dim3((unsigned)n_members), dim3(kInfThreads), 0, st, members_dev, chunks_dev, chunk_begin_dev,
              n_chunks, (const int*)chunk_status_dev, status_dev, info_dev);
  TBN_CHECK_LAUNCH(fn);
  TBN_KLAUNCH(inflate_crc_kernel, dim3((unsigned)n_members), dim3(kCrcThreads), 0, st, members_dev, (const uint8_t*)out_dev,
              status_dev);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}

// the host twin: the same core in segment mode, the same row checks and the same fold, serially; no GPU call
extern "C" int tbn_inflate_chunks_host(const void* in, size_t in_bytes, const tbn_inflate_member* members, int n_members,
                                       const tbn_inflate_chunk* chunks, const uint32_t* chunk_begin, int n_chunks, void* out,
                                       size_t out_bytes, int* status, int* info, int* chunk_status) {
  const char* fn = "inflate_chunks_host";
  int rc = check_args(fn, in, in_bytes, members, n_members, out, status, info);
  if (rc != TBN_OK || n_members == 0) return rc;
  rc = check_chunk_args(fn, chunks, chunk_begin, n_chunks, chunk_status);
  if (rc != TBN_OK) return rc;
  for (int c = 0; c < n_chunks; ++c) {
    int st = chunk_row_status(members, n_members, chunks, chunk_begin, n_chunks, (uint32_t)c, in_bytes, out_bytes);
    uint32_t produced = 0;
    if (st == TBN_INF_OK)
      st = inflate_chunk_host((const uint8_t*)in + chunks[c].in_off, chunks[c].in_len, (uint8_t*)out + chunks[c].out_off,
                              chunks[c].out_len, chunks[c].last != 0, &produced);
    chunk_status[c] = st;
    chunk_status[n_chunks + c] = (int)produced;
  }
  for (int i = 0; i < n_members; ++i) {
    const tbn_inflate_member& m = members[i];
    uint32_t b = 0, e = 0, bytes = 0;
    int st = fold_range(m, chunk_begin, i, n_chunks, &b, &e);
    if (st == TBN_INF_OK) {
      for (uint32_t c = b; c < e; ++c) {                   // the first non-zero status in chunk order, the sum of all bytes
        const bool mine = chunks[c].member == (uint32_t)i;
        if (st == TBN_INF_OK) st = mine ? chunk_status[c] : TBN_INF_ROW;
        if (mine) bytes += (uint32_t)chunk_status[n_chunks + c];
      }
    }
    if (st == TBN_INF_OK && crc_member_host((const uint8_t*)out + m.out_off, m.out_len) != m.crc) st = TBN_INF_CRC;
    status[i] = st;
    info[i] = (int)bytes;
  }
  return TBN_OK;
}
