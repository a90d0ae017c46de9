// Memory and round-trip check of the deflate encoder core (attention_based_tbn_amd/csrc/tbn_deflate.h: the code the kernels
// in csrc/deflate.hip and tbn_deflate_host are built from) as a plain executable.  Nothing of HIP is involved.
//
//   python scripts/make_deflate_golden.py --dump /tmp/deflate_cases
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iattention_based_tbn_amd/csrc
//       scripts/deflate_check.cpp -o /tmp/deflate_check                                (one command line)
//   /tmp/deflate_check /tmp/deflate_cases/*.raw
//
// Per NAME.raw: the bytes in a heap block of EXACTLY their length are compressed into a heap block of EXACTLY
// tbn_deflate::bound(n) bytes, so that a read or write past either is a report; the stream must not be longer than the
// bound, must inflate (tbn_inflate.h, into a block of exactly n bytes) with status 0 to the input, and a second run must
// give the same bytes.  Then with an output block one byte short of the bound: the status must be TBN_DEF_CAPACITY and
// the block untouched.  Every prefix length 0..600 of the file and 40 seeded ones are run the same way, so that chunk and
// block ends fall everywhere.  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tbn_deflate.h"
#include "tbn_inflate.h"

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

static tbn_deflate::State* state;
static uint8_t* slot;

// -> 0: clean; *size: the stream's length
static int one(const std::string& name, const uint8_t* data, uint32_t n, uint64_t* size) {
  using namespace tbn_deflate;
  uint8_t* raw = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(raw, data, n);
  const uint64_t cap = bound(n);
  uint8_t* out = (uint8_t*)malloc(cap);
  memset(out, 0xCD, cap);
  uint64_t len = 0;
  int st = deflate_member_host(raw, n, out, cap, *state, slot, &len);
  if (st != TBN_DEF_OK) return fail(name, "status", st, n);
  if (len > cap || len == 0) return fail(name, "length", (long)len, (long)cap);
  {
    uint8_t* again = (uint8_t*)malloc(cap);
    uint64_t len2 = 0;
    deflate_member_host(raw, n, again, cap, *state, slot, &len2);
    if (len2 != len || memcmp(out, again, len) != 0) return fail(name, "a second run gives other bytes", (long)len, (long)len2);
    free(again);
  }
  {
    uint8_t* stream = (uint8_t*)malloc(len);      // exactly the stream: the decoder must not want more
    memcpy(stream, out, len);
    uint8_t* back = (uint8_t*)malloc(n ? n : 1);
    tbn_inflate::Tables t;
    tbn_inflate::HostIO io{stream, (uint32_t)len, back};
    uint32_t produced = 0;
    const int ist = tbn_inflate::inflate_stream(io, t, (uint32_t)len, n, &produced);
    if (ist != TBN_INF_OK || produced != n) return fail(name, "the stream does not inflate", ist, produced);
    if (n && memcmp(back, raw, n) != 0) return fail(name, "the inflated bytes differ", n);
    free(stream);
    free(back);
  }
  {
    uint8_t* small = (uint8_t*)malloc(cap - 1);
    memset(small, 0xCD, cap - 1);
    uint64_t len3 = 77;
    st = deflate_member_host(raw, n, small, cap - 1, *state, slot, &len3);
    if (st != TBN_DEF_CAPACITY || len3 != 0) return fail(name, "one byte short of the bound is not refused", st, (long)len3);
    for (uint64_t i = 0; i + 1 < cap; ++i)
      if (small[i] != 0xCD) return fail(name, "a refused member was written", (long)i);
    free(small);
  }
  free(raw);
  free(out);
  *size = len;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: deflate_check FILE.raw ...\n");
    return 2;
  }
  state = (tbn_deflate::State*)malloc(sizeof(tbn_deflate::State));
  slot = (uint8_t*)malloc(tbn_deflate::kSlotData);        // exactly the slot: the writer must stay inside
  long runs = 0;
  for (int a = 1; a < argc; ++a) {
    const std::string path = argv[a];
    std::vector<uint8_t> data;
    if (!read_file(path, &data)) return fail(path, "cannot read");
    const size_t slash = path.find_last_of('/');
    const std::string name = path.substr(slash == std::string::npos ? 0 : slash + 1);
    const uint32_t n = (uint32_t)data.size();
    uint64_t size = 0, ignored = 0;
    if (one(name, data.data(), n, &size)) return 1;
    ++runs;
    for (uint32_t k = 0; k <= 600 && k < n; ++k, ++runs)
      if (one(name + " prefix", data.data(), k, &ignored)) return 1;
    for (int k = 0; k < 40 && n > 600; ++k, ++runs)
      if (one(name + " prefix", data.data(), 600 + rnd(n - 600), &ignored)) return 1;
    printf("%-28s ok (%u -> %llu bytes, bound %llu)\n", name.c_str(), n, (unsigned long long)size,
           (unsigned long long)tbn_deflate::bound(n));
  }
  free(state);
  free(slot);
  printf("ok: %ld runs\n", runs);
  return 0;
}
