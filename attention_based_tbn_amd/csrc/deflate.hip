// Flow pickles written on the device: the raw bytes of a batch of .npy members are compressed to raw deflate streams
// (RFC 1951) and their zip CRC-32 computed, in three launches.  Replaces the zlib run inside np.savez_compressed of
// reference preprocessing/create_epic_flow_pickle.py:203.  The encoder core -- the stream format and every decision -- is
// csrc/tbn_deflate.h, the same code the host twin tbn_deflate_host and scripts/deflate_check.cpp run.
//
// deflate_chunk_kernel, 64 threads (one wavefront) per chunk of kChunk = 32 KB.  A member is cut into chunks that are
// compressed independently (matches never leave the chunk), so a batch of 96 stacks of 1.1 MB is 3456 wavefronts where the
// decoder has 96.  The wavefront finds its member by a prefix sum over the member table (64 rows per step, no table in
// memory), loads the chunk into LDS with all lanes and clears the hash table; then LANE 0 ALONE runs the serial core
// (compress_chunk: greedy LZ77 over an LDS hash table, block costs, Huffman construction, the bit writer) into the
// chunk's slot of the workspace.  The other lanes wait at the barrier and come back for the one thing that is wide: the
// copy of a chunk that is written stored.  tbn_deflate::State is 69.8 KB of LDS: two workgroups per CU (160 KB), as for
// inflate_kernel.  No wavefront waits for another one: the slot of chunk c is at c * kSlot, whatever the others produce.
//
// deflate_join_kernel, 256 threads per member: walks the member's slots in order, adds up their sizes and copies each
// slot's bytes behind the previous one (the chunks end on byte boundaries); writes out_len and the status -- and, for
// tbn_deflate_batch_indexed, the chunk index: the stream offset at which each chunk ends, one entry per chunk of every
// row in table order (zeros for a row that is skipped or refused).
//
// deflate_crc_kernel, 256 threads per member: crc_workgroup of csrc/tbn_crc_dev.h (shared with inflate_crc_kernel) over
// the member's raw bytes.
#include "tbn_common.h"
#include "tbn_crc_dev.h"
#include "tbn_deflate.h"
#include "../../include/tbn_hip.h"

#include <vector>

using namespace tbn_deflate;

static_assert(sizeof(tbn_deflate_member) == 32, "the member row is 32 bytes");

namespace {

constexpr int kDefThreads = 64;       // one wavefront
constexpr int kJoinThreads = 256;

// the status of a row from the row and the buffer sizes alone
__host__ __device__ __forceinline__ int row_status(const tbn_deflate_member& m, size_t raw_bytes, size_t out_bytes) {
  if (m.skip) return TBN_DEF_SKIPPED;
  if (m.in_len >= (1u << 31) || (m.in_off & 3u) != 0 || m.in_off > raw_bytes || m.in_len > raw_bytes - m.in_off ||
      m.out_off > out_bytes || m.out_cap > out_bytes - m.out_off)
    return TBN_DEF_ROW;
  if (m.out_cap < bound(m.in_len)) return TBN_DEF_CAPACITY;
  return TBN_DEF_OK;
}
// chunks (= workspace slots) of a row: none unless it will be compressed
__host__ __device__ __forceinline__ uint32_t row_chunks(const tbn_deflate_member& m, size_t raw_bytes, size_t out_bytes) {
  return row_status(m, raw_bytes, out_bytes) == TBN_DEF_OK ? (uint32_t)chunks_of(m.in_len) : 0u;
}

struct DevIO {
  uint8_t* slot;
  __device__ __forceinline__ void put(uint32_t pos, uint8_t b) { slot[pos] = b; }
};

__global__ __launch_bounds__(kDefThreads) void deflate_chunk_kernel(const uint8_t* __restrict__ raw, size_t raw_bytes,
                                                                    const tbn_deflate_member* __restrict__ members, int n_members,
                                                                    size_t out_bytes, uint8_t* __restrict__ workspace) {
  __shared__ State s;
  __shared__ uint32_t result;
  const int ln = threadIdx.x;
  // chunk c of the batch, in table order.  Every value the loop branches on is the same in all lanes.
  for (uint64_t c = blockIdx.x;; c += gridDim.x) {
    // which member, which of its chunks: a prefix sum of the rows' chunk counts, 64 rows per step
    int member = -1;
    uint32_t local = 0;
    uint64_t before = 0;
    for (int base = 0; base < n_members && member < 0; base += kDefThreads) {
      const int i = base + ln;
      const uint32_t cnt = i < n_members ? row_chunks(members[i], raw_bytes, out_bytes) : 0u;
      uint32_t incl = cnt;
      for (int o = 1; o < kDefThreads; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, kDefThreads);
        if (ln >= o) incl += up;
      }
      const uint64_t first = before + incl - cnt;
      const unsigned long long hit = __ballot(cnt > 0 && c >= first && c < first + cnt);
      if (hit) {
        const int src = __ffsll(hit) - 1;
        member = base + src;
        local = (uint32_t)(c - before) - (__shfl(incl, src, kDefThreads) - __shfl(cnt, src, kDefThreads));
      }
      before += __shfl(incl, kDefThreads - 1, kDefThreads);
    }
    if (member < 0) return;                     // c is past the batch's last chunk
    const tbn_deflate_member m = members[member];
    const uint32_t begin = local * kChunk;      // local < chunks_of(in_len) <= 65 536
    const uint32_t len = m.in_len - begin < kChunk ? m.in_len - begin : kChunk;     // 0 only for an empty member
    const bool last = begin + len == m.in_len;
    const uint8_t* src = raw + m.in_off + begin;                                     // 4-byte aligned
    uint8_t* slot = workspace + c * kSlot;
    __syncthreads();                            // the previous chunk's lane 0 is done with s
    for (uint32_t i = (uint32_t)ln; i < (len + 3) / 4; i += kDefThreads) {
      uint32_t v = 0;
      if (4 * i + 4 <= len) {
        v = *(const uint32_t*)(src + 4 * i);
      } else {
        for (uint32_t k = 0; 4 * i + k < len; ++k) v |= (uint32_t)src[4 * i + k] << (8 * k);
      }
      ((uint32_t*)s.in)[i] = v;
    }
    for (uint32_t i = (uint32_t)ln; i < kBuckets; i += kDefThreads) s.head[i] = ~0ull;
    __syncthreads();
    if (ln == 0) {
      uint32_t size;
      if (len == 0) {                           // an empty member: the final fixed block
        slot[kSlotHeader] = 0x03, slot[kSlotHeader + 1] = 0x00;
        size = 2;
      } else {
        DevIO io{slot + kSlotHeader};
        size = compress_chunk(io, s, len, last);
      }
      result = size;
    }
    __syncthreads();
    uint32_t size = result;
    if (size == kUseStored) {
      if (ln == 0) stored_header(len, last, slot + kSlotHeader);
      for (uint32_t i = (uint32_t)ln; i < len; i += kDefThreads) slot[kSlotHeader + kStoredHeader + i] = s.in[i];
      size = kStoredHeader + len;
    }
    if (ln == 0) *(uint32_t*)slot = size;       // size <= kStoredHeader + kChunk < kSlotData
  }
}

__global__ __launch_bounds__(kJoinThreads) void deflate_join_kernel(const tbn_deflate_member* __restrict__ members, size_t raw_bytes,
                                                                    const uint8_t* __restrict__ workspace, uint8_t* __restrict__ out,
                                                                    size_t out_bytes, uint32_t* __restrict__ out_len,
                                                                    int* __restrict__ status, uint32_t* __restrict__ chunk_end) {
  __shared__ unsigned long long part[kJoinThreads], part_all[kJoinThreads];
  const int m_no = blockIdx.x, t = threadIdx.x;
  const tbn_deflate_member m = members[m_no];
  int st = row_status(m, raw_bytes, out_bytes);           // one value for the workgroup
  // the member's first slot: the chunks of the rows in front of it that are compressed; its first index entry: the
  // chunks of ALL rows in front of it
  unsigned long long mine = 0, mine_all = 0;
  for (int i = t; i < m_no; i += kJoinThreads) {
    mine += row_chunks(members[i], raw_bytes, out_bytes);
    mine_all += chunks_of(members[i].in_len);
  }
  part[t] = mine;
  part_all[t] = mine_all;
  __syncthreads();
  for (int k = kJoinThreads / 2; k > 0; k >>= 1) {
    if (t < k) part[t] += part[t + k], part_all[t] += part_all[t + k];
    __syncthreads();
  }
  const uint64_t first = part[0];
  const uint32_t chunks = (uint32_t)chunks_of(m.in_len);
  uint32_t* ends = chunk_end ? chunk_end + part_all[0] : nullptr;
  if (ends)
    for (uint32_t k = (uint32_t)t; k < chunks; k += kJoinThreads) ends[k] = 0;
  __syncthreads();                                        // the zeros are in place before thread 0 writes an end
  uint64_t at = 0;
  if (st == TBN_DEF_OK) {
    uint8_t* dst = out + m.out_off;
    for (uint32_t k = 0; k < chunks; ++k) {
      const uint8_t* slot = workspace + (first + k) * kSlot;
      const uint32_t size = *(const uint32_t*)slot;
      if (size > kStoredHeader + kChunk || at + size > m.out_cap) {      // never: at + size <= bound(in_len) <= out_cap
        st = TBN_DEF_ROW;
        break;
      }
      for (uint32_t i = (uint32_t)t; i < size; i += kJoinThreads) dst[at + i] = slot[kSlotHeader + i];
      at += size;
      if (ends && t == 0) ends[k] = (uint32_t)at;
    }
    if (ends && st != TBN_DEF_OK) {                       // never (see above): a refused row's entries are 0
      __syncthreads();
      for (uint32_t k = (uint32_t)t; k < chunks; k += kJoinThreads) ends[k] = 0;
    }
  }
  if (t == 0) {
    status[m_no] = st;
    out_len[m_no] = st == TBN_DEF_OK ? (uint32_t)at : 0u;
  }
}

__global__ __launch_bounds__(tbn_inflate::kCrcThreads) void deflate_crc_kernel(const uint8_t* __restrict__ raw,
                                                                               const tbn_deflate_member* __restrict__ members,
                                                                               const int* __restrict__ status,
                                                                               uint32_t* __restrict__ crc) {
  __shared__ uint32_t table[256];
  __shared__ uint32_t part[tbn_inflate::kCrcThreads];
  const int m_no = blockIdx.x;
  const tbn_deflate_member m = members[m_no];
  const bool run = status[m_no] == TBN_DEF_OK;            // the join launch has completed; the row was checked there
  const uint32_t c = tbn_inflate::crc_workgroup(raw + m.in_off, m.in_len, run, table, part);
  if (threadIdx.x == 0) crc[m_no] = c;
}

int check_args(const char* fn, const void* raw, const tbn_deflate_member* members, int n, const void* out, const void* out_len,
               const void* crc, const void* status) {
  TBN_REQUIRE(n >= 0, "%s: n_members %d is negative", fn, n);
  if (n == 0) return TBN_OK;
  TBN_REQUIRE(raw != nullptr && members != nullptr && out != nullptr && out_len != nullptr && crc != nullptr && status != nullptr,
              "%s: null argument", fn);
  TBN_REQUIRE(((uintptr_t)raw & 3) == 0 && ((uintptr_t)members & 7) == 0 && ((uintptr_t)out_len & 3) == 0 &&
                  ((uintptr_t)crc & 3) == 0 && ((uintptr_t)status & 3) == 0,
              "%s: `raw`, out_len, crc and status must be 4-byte aligned, the member table 8-byte aligned", fn);
  return TBN_OK;
}

}  // namespace

extern "C" size_t tbn_deflate_chunk(void) { return kChunk; }

extern "C" size_t tbn_deflate_bound(size_t n) { return (size_t)bound(n); }

// every row that is not skipped counts, consistent or not: the kernels give slots to at most these
extern "C" size_t tbn_deflate_workspace_bytes(const tbn_deflate_member* members, int n_members) {
  size_t slots = 0;
  for (int i = 0; members != nullptr && i < n_members; ++i)
    if (!members[i].skip && members[i].in_len < (1u << 31)) slots += (size_t)chunks_of(members[i].in_len);
  return (slots ? slots : 1) * (size_t)kSlot;
}

namespace {

int deflate_batch(const char* fn, const void* raw_dev, size_t raw_bytes, const tbn_deflate_member* members_dev, int n_members,
                  void* out_dev, size_t out_bytes, uint32_t* out_len_dev, uint32_t* crc_dev, int* status_dev, void* workspace,
                  void* stream, uint32_t* chunk_end_dev) {
  const int rc = check_args(fn, raw_dev, members_dev, n_members, out_dev, out_len_dev, crc_dev, status_dev);
  if (rc != TBN_OK || n_members == 0) return rc;
  TBN_REQUIRE(workspace != nullptr && ((uintptr_t)workspace & 15) == 0, "%s: the workspace must be 16-byte aligned", fn);
  hipStream_t st = (hipStream_t)stream;
  // one workgroup per chunk when the rows do not overlap in `raw`; a workgroup takes further chunks when they do
  const size_t most = raw_bytes / kChunk + (size_t)n_members;
  const unsigned grid = (unsigned)(most < (1u << 20) ? most : (1u << 20));
  TBN_KLAUNCH(deflate_chunk_kernel, dim3(grid), dim3(kDefThreads), 0, st, (const uint8_t*)raw_dev, raw_bytes, members_dev, n_members,
              out_bytes, (uint8_t*)workspace);
  TBN_CHECK_LAUNCH(fn);
  TBN_KLAUNCH(deflate_join_kernel, dim3((unsigned)n_members), dim3(kJoinThreads), 0, st, members_dev, raw_bytes,
              (const uint8_t*)workspace, (uint8_t*)out_dev, out_bytes, out_len_dev, status_dev, chunk_end_dev);
  TBN_CHECK_LAUNCH(fn);
  TBN_KLAUNCH(deflate_crc_kernel, dim3((unsigned)n_members), dim3(tbn_inflate::kCrcThreads), 0, st, (const uint8_t*)raw_dev,
              members_dev, (const int*)status_dev, crc_dev);
  TBN_CHECK_LAUNCH(fn);
  return TBN_OK;
}

int deflate_host(const char* fn, const void* raw, size_t raw_bytes, const tbn_deflate_member* members, int n_members, void* out,
                 size_t out_bytes, uint32_t* out_len, uint32_t* crc, int* status, uint32_t* chunk_end) {
  const int rc = check_args(fn, raw, members, n_members, out, out_len, crc, status);
  if (rc != TBN_OK || n_members == 0) return rc;
  std::vector<State> state(1);          // 70 KB: not on the caller's stack
  std::vector<uint8_t> slot(kSlotData);
  State& s = state[0];
  uint32_t table[256];
  for (uint32_t i = 0; i < 256; ++i) table[i] = tbn_inflate::crc_table_entry(i);
  for (int i = 0; i < n_members; ++i) {
    const tbn_deflate_member& m = members[i];
    const int st = row_status(m, raw_bytes, out_bytes);
    status[i] = st;
    out_len[i] = 0;
    crc[i] = 0;
    uint32_t* ends = chunk_end;                           // this row's entries: chunks_of(in_len) of them, refused or not
    if (chunk_end) chunk_end += chunks_of(m.in_len);
    if (st != TBN_DEF_OK) {
      if (ends)
        for (uint64_t k = 0; k < chunks_of(m.in_len); ++k) ends[k] = 0;
      continue;
    }
    const uint8_t* src = (const uint8_t*)raw + m.in_off;
    uint64_t produced = 0;
    status[i] = deflate_member_host(src, m.in_len, (uint8_t*)out + m.out_off, m.out_cap, s, slot.data(), &produced, ends);
    out_len[i] = (uint32_t)produced;
    // the CRC in kCrcChunks chunks, as the kernel computes it
    const uint32_t n = m.in_len, chunk = tbn_inflate::crc_chunk_len(n);
    uint32_t c = 0;
    for (uint32_t k = 0; k < tbn_inflate::kCrcChunks; ++k) {
      const uint64_t b = (uint64_t)k * chunk, e = b + chunk;
      c ^= tbn_inflate::crc_chunk(src, (uint32_t)(b < n ? b : n), (uint32_t)(e < n ? e : n), n, table);
    }
    crc[i] = c;
  }
  return TBN_OK;
}

}  // namespace

extern "C" int tbn_deflate_batch(const void* raw_dev, size_t raw_bytes, const tbn_deflate_member* members_dev, int n_members,
                                 void* out_dev, size_t out_bytes, uint32_t* out_len_dev, uint32_t* crc_dev, int* status_dev,
                                 void* workspace, void* stream) {
  return deflate_batch("deflate_batch", raw_dev, raw_bytes, members_dev, n_members, out_dev, out_bytes, out_len_dev, crc_dev,
                       status_dev, workspace, stream, nullptr);
}

// the same launches; the join launch also writes the chunk index
extern "C" int tbn_deflate_batch_indexed(const void* raw_dev, size_t raw_bytes, const tbn_deflate_member* members_dev,
                                         int n_members, void* out_dev, size_t out_bytes, uint32_t* out_len_dev, uint32_t* crc_dev,
                                         int* status_dev, void* workspace, void* stream, uint32_t* chunk_end_dev) {
  const char* fn = "deflate_batch_indexed";
  TBN_REQUIRE(n_members <= 0 || (chunk_end_dev != nullptr && ((uintptr_t)chunk_end_dev & 3) == 0),
              "%s: chunk_end must be a 4-byte aligned array", fn);
  return deflate_batch(fn, raw_dev, raw_bytes, members_dev, n_members, out_dev, out_bytes, out_len_dev, crc_dev, status_dev,
                       workspace, stream, chunk_end_dev);
}

// the host twins: the same core, serially, over the same member table; no GPU call
extern "C" int tbn_deflate_host(const void* raw, size_t raw_bytes, const tbn_deflate_member* members, int n_members, void* out,
                                size_t out_bytes, uint32_t* out_len, uint32_t* crc, int* status) {
  return deflate_host("deflate_host", raw, raw_bytes, members, n_members, out, out_bytes, out_len, crc, status, nullptr);
}

extern "C" int tbn_deflate_host_indexed(const void* raw, size_t raw_bytes, const tbn_deflate_member* members, int n_members,
                                        void* out, size_t out_bytes, uint32_t* out_len, uint32_t* crc, int* status,
                                        uint32_t* chunk_end) {
  const char* fn = "deflate_host_indexed";
  TBN_REQUIRE(n_members <= 0 || (chunk_end != nullptr && ((uintptr_t)chunk_end & 3) == 0),
              "%s: chunk_end must be a 4-byte aligned array", fn);
  return deflate_host(fn, raw, raw_bytes, members, n_members, out, out_bytes, out_len, crc, status, chunk_end);
}
