// Memory and equality check of the inflate decoder core (attention_based_tbn_amd/csrc/tbn_inflate.h: the code the kernel in
// csrc/inflate.hip and tbn_inflate_host are built from) as a plain executable.  Nothing of HIP is involved.
//
//   python scripts/make_inflate_golden.py --dump /tmp/inflate_cases
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iattention_based_tbn_amd/csrc
//       scripts/inflate_check.cpp -o /tmp/inflate_check                                (one command line)
//   /tmp/inflate_check /tmp/inflate_cases/*.deflate
//
// Per NAME.deflate (with NAME.out beside it, zlib's output, unless NAME starts with bad_): the stream in a heap block of
// EXACTLY its length is inflated into a heap block of EXACTLY the declared size, so that a read or write past either is
// a report.  A good case must give status 0, NAME.out's bytes and its length; a bad_ case a non-zero status.  Then, with
// the declared size one byte short and one byte long (statuses 8 and 9), every truncation (every length of streams up to
// 4 KiB, 400 seeded lengths of larger ones) and 300 seeded single-byte corruptions: each run must end in the exact output
// with status 0 or 10 (a corruption may leave the bytes alone or not), or in another status -- and return at all.
// `--pick NAME` prints, for the file whose path contains NAME, seeded corruptions by outcome: the first the decoder
// refuses mid-stream and the first that inflates to the declared size and fails only the CRC (the damaged inputs of
// tests/test_inflate_gpu.py).  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "tbn_inflate.h"

using namespace tbn_inflate;

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

static uint32_t crc_plain(const std::vector<uint8_t>& v) {     // byte by byte, the textbook way: checks the chunked one
  uint32_t c = 0xFFFFFFFFu;
  for (uint8_t b : v) c = crc_table_entry((c ^ b) & 0xFFu) ^ (c >> 8);
  return c ^ 0xFFFFFFFFu;
}

struct Run {
  int status;
  uint32_t produced;
  std::vector<uint8_t> out;
};

// exact-size heap copies of the input and the output
static Run run(const uint8_t* stream, size_t n, uint32_t declared, uint32_t crc) {
  uint8_t* in = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(in, stream, n);
  uint8_t* out = (uint8_t*)malloc(declared ? declared : 1);
  memset(out, 0xCD, declared ? declared : 1);
  Run r;
  r.status = inflate_member_host(n ? in : in, (uint32_t)n, 8, out, declared, crc, &r.produced);
  r.out.assign(out, out + declared);
  free(in);
  free(out);
  return r;
}

static int fail(const std::string& name, const char* what, long a = 0, long b = 0) {
  fprintf(stderr, "FAIL %s: %s (%ld, %ld)\n", name.c_str(), what, a, b);
  return 1;
}

int main(int argc, char** argv) {
  std::string pick;
  std::vector<std::string> files;
  for (int i = 1; i < argc; ++i) {
    if (std::string(argv[i]) == "--pick" && i + 1 < argc)
      pick = argv[++i];
    else
      files.push_back(argv[i]);
  }
  if (files.empty()) {
    fprintf(stderr, "usage: inflate_check [--pick NAME] FILE.deflate ...\n");
    return 2;
  }
  long runs = 0;
  for (const std::string& path : files) {
    if (!pick.empty() && path.find(pick) == std::string::npos) continue;
    std::vector<uint8_t> stream, want;
    if (!read_file(path, &stream)) return fail(path, "cannot read");
    const size_t slash = path.find_last_of('/');
    const std::string name = path.substr(slash == std::string::npos ? 0 : slash + 1);
    const bool bad = name.rfind("bad_", 0) == 0;
    if (!bad && !read_file(path.substr(0, path.size() - 8) + ".out", &want)) return fail(path, "no .out beside it");
    const uint32_t n = (uint32_t)want.size(), crc = crc_plain(want);
    if (bad) {
      for (uint32_t declared : {0u, 1u, 64u, 100000u}) {
        const Run r = run(stream.data(), stream.size(), declared, 0);
        ++runs;
        if (r.status == TBN_INF_OK || r.status == TBN_INF_CRC) return fail(name, "a refused stream was inflated", r.status, declared);
      }
      if (pick.empty()) printf("%-36s refused with status %d\n", name.c_str(), run(stream.data(), stream.size(), 64, 0).status);
      continue;
    }
    {
      const Run r = run(stream.data(), stream.size(), n, crc);
      ++runs;
      if (r.status != TBN_INF_OK) return fail(name, "status", r.status);
      if (r.produced != n || r.out != want) return fail(name, "output differs", r.produced, n);
      const Run w = run(stream.data(), stream.size(), n, crc ^ 1u);
      if (w.status != TBN_INF_CRC) return fail(name, "a wrong CRC was not noticed", w.status);
      if (n > 0) {
        const Run s = run(stream.data(), stream.size(), n - 1, crc);
        if (s.status != TBN_INF_OUTPUT_FULL) return fail(name, "declared size one short", s.status);
      }
      const Run l = run(stream.data(), stream.size(), n + 1, crc);
      if (l.status != TBN_INF_OUTPUT_SHORT || l.produced != n) return fail(name, "declared size one long", l.status);
      runs += 3;
    }
    if (pick.empty()) {
      // truncations: never the whole output with status 0 unless the cut only removed padding behind the last block
      const size_t total = stream.size();
      const uint32_t cuts = total <= 4096 ? (uint32_t)total : 400;
      for (uint32_t k = 0; k < cuts; ++k) {
        const size_t len = total <= 4096 ? k : rnd((uint32_t)total);
        const Run r = run(stream.data(), len, n, crc);
        ++runs;
        if (r.status == TBN_INF_OK && r.out != want) return fail(name, "truncation: status 0 with other bytes", (long)len);
        if (r.status == TBN_INF_OK && len + 1 < total) return fail(name, "truncation: status 0 more than a byte short", (long)len);
      }
    }
    // single-byte corruptions
    bool have_refused = false, have_crc = false;
    for (int k = 0; k < 300 && !stream.empty(); ++k) {
      const uint32_t off = rnd((uint32_t)stream.size());
      const uint8_t value = (uint8_t)rnd(256);
      if (value == stream[off]) continue;
      std::vector<uint8_t> changed(stream);
      changed[off] = value;
      const Run r = run(changed.data(), changed.size(), n, crc);
      ++runs;
      if (r.status == TBN_INF_OK && r.out != want) return fail(name, "corruption: status 0 with other bytes", off, value);
      if (r.status < 0 || r.status > TBN_INF_CRC) return fail(name, "corruption: unknown status", r.status);
      if (!pick.empty()) {
        const bool mid = r.status >= TBN_INF_BLOCK_TYPE && r.status <= TBN_INF_INPUT && r.produced > 0 && r.produced < n;
        if (mid && !have_refused) {
          printf("%s refused mid-stream: offset %u value %u -> status %d after %u of %u bytes\n", name.c_str(), off, value, r.status,
                 r.produced, n);
          have_refused = true;
        }
        if (r.status == TBN_INF_CRC && !have_crc) {
          printf("%s inflates fully, CRC fails: offset %u value %u -> status %d, %u bytes\n", name.c_str(), off, value, r.status,
                 r.produced);
          have_crc = true;
        }
      }
    }
    if (pick.empty()) printf("%-36s ok (%u -> %u bytes)\n", name.c_str(), (unsigned)stream.size(), n);
  }
  printf("ok: %ld runs\n", runs);
  return 0;
}
