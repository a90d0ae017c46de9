// The device IO policy of the RFC 1951 decoder core (csrc/tbn_inflate.h) for ONE wavefront per stream: the compressed bytes
// through an LDS ring, the last 64 KB of output in an LDS window, every literal and match also stored to global memory in
// stream order.  Shared by inflate_kernel (csrc/inflate.hip: zip members) and png_inflate_kernel (csrc/png.hip: the zlib
// stream of a PNG file); both declare the LDS (Tables, 2 * kChunk ring bytes, kWin window bytes) and hand it in.
#pragma once
#include "tbn_inflate.h"

namespace tbn_inflate {

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

}  // namespace tbn_inflate
