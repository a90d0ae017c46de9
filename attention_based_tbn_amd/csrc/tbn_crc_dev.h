// The zip CRC-32 of one byte range by one workgroup: the chunk-and-combine scheme of tbn_inflate.h (crc_chunk) as the body
// shared by inflate_crc_kernel (csrc/inflate.hip: the inflated bytes against the directory's CRC) and deflate_crc_kernel
// (csrc/deflate.hip: the raw bytes' CRC for the zip directory).
#pragma once
#include "tbn_inflate.h"

namespace tbn_inflate {

constexpr int kCrcThreads = (int)kCrcChunks;

// Called by all kCrcThreads threads of the workgroup with `run` one value for all of them.  table[256] and
// part[kCrcThreads] are LDS.  -> the CRC-32 of data[0, n) (0 when !run), the same in every thread.
__device__ __forceinline__ uint32_t crc_workgroup(const uint8_t* data, uint32_t n, bool run, uint32_t* table, uint32_t* part) {
  const int t = threadIdx.x;
  table[t] = crc_table_entry((uint32_t)t);
  __syncthreads();
  uint32_t c = 0;
  if (run) {
    const uint32_t chunk = crc_chunk_len(n);
    const uint64_t b = (uint64_t)t * chunk, e = b + chunk;
    c = crc_chunk(data, (uint32_t)(b < n ? b : n), (uint32_t)(e < n ? e : n), n, table);
  }
  part[t] = c;
  __syncthreads();
  for (int s = kCrcThreads / 2; s > 0; s >>= 1) {
    if (t < s) part[t] ^= part[t + s];
    __syncthreads();
  }
  return part[0];
}

}  // namespace tbn_inflate
