// Memory check of the chunk-indexed inflate path (attention_based_tbn_amd/csrc/tbn_inflate.h in SEGMENT MODE: the code
// inflate_chunk_kernel of csrc/inflate.hip and tbn_inflate_chunks_host are built from; the index comes from
// csrc/tbn_deflate.h) as a plain executable.  Nothing of HIP is involved.
//
//   python scripts/make_deflate_golden.py --dump /tmp/deflate_cases
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iattention_based_tbn_amd/csrc
//       scripts/inflate_chunks_check.cpp -o /tmp/inflate_chunks_check                  (one command line)
//   /tmp/inflate_chunks_check /tmp/deflate_cases/*.raw
//
// Per NAME.raw (at most its first kMaxRaw bytes): the bytes are compressed with the chunk index (deflate_member_host); the
// index must have chunks_of(n) strictly increasing entries, the last the stream's length.  Then every chunk's slice, in a
// heap block of EXACTLY its length, is inflated into a heap block of EXACTLY the chunk's raw size -- a read or write past
// either is a report -- and must give status 0 and the chunk's bytes.  Then
//   * EVERY truncation of every slice: a non-zero status, produced <= the chunk's size, nothing written behind `produced`;
//   * the slice one byte long (the next chunk's first byte, or a zero): a non-zero status;
//   * the wrong mode (the last chunk as an inner one and the reverse): TBN_INF_SEGMENT;
//   * 200 seeded single-byte corruptions of the stream and 200 seeded corruptions of the index (an end moved by -3..3, or
//     put anywhere in the stream), each run chunk by chunk as tbn_inflate_chunks_host does: every status is one of 0..13,
//     and whenever all chunks report 0 with the member's CRC-32 intact the bytes are the member's.
// Every run has to return at all.  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tbn_deflate.h"
#include "tbn_inflate.h"

using namespace tbn_inflate;

constexpr uint32_t kSeg = tbn_deflate::kChunk;
constexpr uint32_t kMaxRaw = 3 * kSeg + 5;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {    // xorshift64*: seeded, no library state
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static bool read_file(const std::string& path, std::vector<uint8_t>* out) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize((size_t)n);
  const bool ok = n == 0 || fread(out->data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

static int fail(const std::string& name, const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "FAIL %s: %s (%ld, %ld)\n", name.c_str(), what, a, b);
  return 1;
}

struct Run {
  int status;
  uint32_t produced;
  std::vector<uint8_t> out;
};

static long runs = 0;

// one slice: exact-size heap copies of the input and the output
static Run run(const uint8_t* slice, size_t n, uint32_t declared, bool last) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(in, slice, n);
  uint8_t* out = (uint8_t*)malloc(declared ? declared : 1);
  memset(out, 0xCD, declared ? declared : 1);
  Run r;
  r.status = inflate_chunk_host(in, (uint32_t)n, out, declared, last, &r.produced);
  r.out.assign(out, out + declared);
  free(in);
  free(out);
  ++runs;
  return r;
}

static bool equal_bytes(const uint8_t* a, const uint8_t* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }

static bool untouched_behind(const Run& r) {
  for (size_t i = r.produced; i < r.out.size(); ++i)
    if (r.out[i] != 0xCD) return false;
  return true;
}

// the member chunk by chunk with the index `ends` -> the first non-zero status in chunk order (12 for an entry that is
// no slice of the stream); *same: every byte is the member's
static int run_member(const std::vector<uint8_t>& stream, const std::vector<uint32_t>& ends, const std::vector<uint8_t>& raw,
                      bool* same, int* worst) {
  int first = 0;
  *same = true;
  uint32_t prev = 0;
  for (size_t k = 0; k < ends.size(); ++k) {
    const uint32_t begin = (uint32_t)k * kSeg, size = k + 1 == ends.size() ? (uint32_t)raw.size() - begin : kSeg;
    int st = TBN_INF_ROW;
    if (ends[k] >= prev && ends[k] <= stream.size() && (k + 1 < ends.size() || ends[k] == stream.size())) {
      const Run r = run(stream.data() + prev, ends[k] - prev, size, k + 1 == ends.size());
      st = r.status;
      if (r.produced > size || !untouched_behind(r)) *worst = -1;
      if (st == TBN_INF_OK && !equal_bytes(r.out.data(), raw.data() + begin, size)) *same = false;
      prev = ends[k];
    }
    if (st < 0 || st > TBN_INF_SEGMENT) *worst = -1;
    if (st != TBN_INF_OK) *same = false;
    if (first == 0) first = st;
  }
  return first;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: inflate_chunks_check FILE.raw ...\n");
    return 2;
  }
  std::vector<tbn_deflate::State> state(1);
  std::vector<uint8_t> slot(tbn_deflate::kSlotData);
  for (int a = 1; a < argc; ++a) {
    const std::string path = argv[a];
    std::vector<uint8_t> raw;
    if (!read_file(path, &raw)) return fail(path, "cannot read");
    const size_t slash = path.find_last_of('/');
    const std::string name = path.substr(slash == std::string::npos ? 0 : slash + 1);
    if (raw.size() > kMaxRaw) raw.resize(kMaxRaw);
    const uint32_t n = (uint32_t)raw.size();
    // 1. compress with the index
    const size_t chunks = (size_t)tbn_deflate::chunks_of(n);
    std::vector<uint8_t> stream((size_t)tbn_deflate::bound(n));
    std::vector<uint32_t> ends(chunks, 0xCDCDCDCDu);
    uint64_t len = 0;
    if (tbn_deflate::deflate_member_host(raw.data(), n, stream.data(), stream.size(), state[0], slot.data(), &len, ends.data()) !=
        TBN_DEF_OK)
      return fail(name, "deflate status");
    stream.resize((size_t)len);
    for (size_t k = 0; k < chunks; ++k)
      if (ends[k] <= (k ? ends[k - 1] : 0u)) return fail(name, "the index does not increase", (long)k, ends[k]);
    if (ends.back() != len) return fail(name, "the last end is not the stream's length", ends.back(), (long)len);
    // 2. chunk by chunk, 3. every truncation of every slice
    uint32_t prev = 0;
    for (size_t k = 0; k < chunks; ++k) {
      const bool last = k + 1 == chunks;
      const uint32_t begin = (uint32_t)k * kSeg, size = last ? n - begin : kSeg, clen = ends[k] - prev;
      const uint8_t* slice = stream.data() + prev;
      const Run r = run(slice, clen, size, last);
      if (r.status != TBN_INF_OK) return fail(name, "chunk status", (long)k, r.status);
      if (r.produced != size || !equal_bytes(r.out.data(), raw.data() + begin, size)) return fail(name, "chunk bytes differ", (long)k);
      const Run w = run(slice, clen, size, !last);
      if (w.status != TBN_INF_SEGMENT) return fail(name, "the wrong mode was not noticed", (long)k, w.status);
      std::vector<uint8_t> longer(slice, slice + clen);
      longer.push_back(last ? 0 : stream[ends[k]]);
      const Run l = run(longer.data(), longer.size(), size, last);
      if (l.status == TBN_INF_OK) return fail(name, "a slice one byte long was accepted", (long)k);
      if (l.produced > size || !untouched_behind(l)) return fail(name, "one byte long: output", (long)k);
      if (size > 0) {
        const Run s = run(slice, clen, size - 1, last);
        if (s.status == TBN_INF_OK || s.produced > size - 1) return fail(name, "declared size one short", (long)k, s.status);
      }
      for (uint32_t cut = 0; cut < clen; ++cut) {
        const Run t = run(slice, cut, size, last);
        if (t.status == TBN_INF_OK) return fail(name, "truncation: status 0", (long)k, cut);
        if (t.status < 0 || t.status > TBN_INF_SEGMENT) return fail(name, "truncation: unknown status", t.status);
        if (t.produced > size || !untouched_behind(t)) return fail(name, "truncation: output", (long)k, cut);
      }
      prev = ends[k];
    }
    // 4. seeded corruptions of the stream and of the index
    for (int trial = 0; trial < 400; ++trial) {
      std::vector<uint8_t> s2(stream);
      std::vector<uint32_t> e2(ends);
      if (trial < 200) {
        const uint32_t off = rnd((uint32_t)s2.size());
        s2[off] = (uint8_t)(s2[off] ^ (1u + rnd(255)));
      } else {
        const uint32_t k = rnd((uint32_t)e2.size());
        const uint32_t moved = trial & 1 ? rnd((uint32_t)s2.size() + 1) : e2[k] + rnd(7) - 3;
        if (moved == e2[k]) continue;
        e2[k] = moved;
      }
      bool same = false;
      int worst = 0;
      const int st = run_member(s2, e2, raw, &same, &worst);
      if (worst < 0) return fail(name, "corruption: a status out of range or bytes written out of range", trial, st);
      // a damaged stream may inflate to other bytes with every chunk at status 0 (a flipped byte of a stored chunk):
      // the CRC-32 pass of tbn_inflate_chunks is what refuses those.  A wrong index over the right stream may not.
      if (st == TBN_INF_OK && !same && trial >= 200) return fail(name, "a wrong index gave status 0 with other bytes", trial);
    }
    printf("%-28s ok (%u -> %u bytes, %u chunks)\n", name.c_str(), n, (unsigned)len, (unsigned)chunks);
  }
  printf("ok: %ld runs\n", runs);
  return 0;
}
