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
// crc_kernel, 256 threads per member: the 256-entry table in LDS, one chunk of equal length per thread, each chunk's CRC
// multiplied by x^(8 * bytes behind it) mod P and XOR-reduced; a mismatch turns status 0 into TBN_INF_CRC.  The body is
// crc_workgroup (csrc/tbn_crc_dev.h), which deflate_crc_kernel of csrc/deflate.hip calls too.
#include "tbn_common.h"
#include "tbn_crc_dev.h"
#include "tbn_inflate.h"
#include "../../include/tbn_hip.h"

using namespace tbn_inflate;

static_assert(sizeof(tbn_inflate_member) == 40, "the member row is 40 bytes");

namespace {

constexpr int kInfThreads = 64;            // one wavefront: DevIO::sync relies on it
constexpr uint32_t kWin = 1u << 16;        // output ring (window) bytes
constexpr uint32_t kChunk = 4096;          // input ring: two chunks
constexpr uint32_t kNoBase = 0xFFFFFFFFu;
static_assert(kInfThreads == 64, "DevIO::sync is a wavefront-scope fence: the workgroup must be one wavefront");

struct DevIO {
  const uint8_t* in;       // the member's compressed bytes (4-byte aligned)
  uint32_t clen;
  uint8_t* out;            // the member's staged bytes
  uint8_t* win;            // LDS, kWin bytes
  uint32_t* ring;          // LDS, 2 * kChunk bytes
  uint32_t base;           // stream offset of the older resident chunk: [base, base + 2 * kChunk) is in the ring
  int ln;

  __device__ __forceinline__ bool leader() const { return ln == 0; }
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return kInfThreads; }
  __device__ __forceinline__ uint32_t uni(uint32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
  // The workgroup IS one wavefront, so lanes exchange data through LDS under a wavefront-scope fence: the compiler keeps
  // the order of the accesses, the LDS executes one wavefront's operations in order, and nothing waits for the global
  // stores of the staged bytes in flight (a workgroup-scope barrier drains them: vmcnt(0) at every match).
  __device__ __forceinline__ void sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  __device__ __forceinline__ void load_chunk(uint32_t cb) {      // stream bytes [cb, cb + kChunk) into their slot
    uint32_t* slot = ring + (cb & (2 * kChunk - 1)) / 4;
    for (uint32_t i = (uint32_t)ln; i < kChunk / 4; i += kInfThreads) {
      const uint64_t g = (uint64_t)cb + 4ull * i;
      uint32_t v = 0;
      if (g + 4 <= clen) {
        v = *(const uint32_t*)(in + g);
      } else {
        for (uint32_t k = 0; k < 4; ++k)
          if (g + k < clen) v |= (uint32_t)in[g + k] << (8 * k);
      }
      slot[i] = v;
    }
  }
  __device__ __forceinline__ uint32_t in_u32(uint32_t pos) {
    const uint32_t want = pos & ~(kChunk - 1);
    if (want != base) {                                           // wave-uniform: pos is
      sync();
      if (base != kNoBase && want == base + kChunk) {
        load_chunk(want + kChunk);
      } else {
        load_chunk(want);
        load_chunk(want + kChunk);
      }
      base = want;
      sync();
    }
    const uint32_t w = (pos & (2 * kChunk - 1)) >> 2;
    const uint64_t two = (uint64_t)ring[w] | ((uint64_t)ring[(w + 1) & (2 * kChunk / 4 - 1)] << 32);
    return uni((uint32_t)(two >> (8 * (pos & 3u))));
  }
  __device__ __forceinline__ void put(uint32_t pos, uint8_t b) {
    if (ln == 0) {
      win[pos & (kWin - 1)] = b;
      out[pos] = b;
    }
  }
  __device__ __forceinline__ void copy_match(uint32_t pos, uint32_t dist, uint32_t len) {
    sync();
    const uint32_t from = pos - dist;
    if (dist >= len) {
      for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) {
        const uint8_t b = win[(from + i) & (kWin - 1)];
        win[(pos + i) & (kWin - 1)] = b;
        out[pos + i] = b;
      }
    } else {
      for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) {
        const uint8_t b = win[(from + i % dist) & (kWin - 1)];
        win[(pos + i) & (kWin - 1)] = b;
        out[pos + i] = b;
      }
    }
    sync();
  }
  __device__ __forceinline__ void copy_stored(uint32_t src, uint32_t pos, uint32_t len) {
    sync();
    for (uint32_t i = (uint32_t)ln; i < len; i += kInfThreads) {
      const uint8_t b = in[src + i];
      win[(pos + i) & (kWin - 1)] = b;
      out[pos + i] = b;
    }
    sync();
  }
};

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
