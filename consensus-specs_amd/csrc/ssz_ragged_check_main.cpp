// Stand-alone check of the ragged root programs of bls381_ssz.hpp for sanitizer builds
// (g++ -fsanitize=address,undefined): reads cases with their expected results from the file named
// on the command line (whitespace-separated tokens, written by tests/test_ssz_ragged_host.py from
// the model), runs them through the host exports of host_check_ssz_ragged.hpp and exits 1 on a
// mismatch.
//   P plen word[plen]                  the program of the items that follow
//   I len hex|- rc root_hex            one item: its bytes, the expected return and root
//   K max_field_bytes want plen word[plen]   a program for the host check, accepted (1) or not (0)
// An item lives in a heap block of exactly its bytes, so a read outside it is a heap overflow the
// sanitizer reports, not luck.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "host_check_ssz_ragged.hpp"

namespace {
std::ifstream in;
std::string tok() {
  std::string t;
  if (!(in >> t)) { std::fprintf(stderr, "unexpected end of input\n"); std::exit(2); }
  return t;
}
uint64_t num() { return std::strtoull(tok().c_str(), nullptr, 10); }
std::vector<uint32_t> words() {
  std::vector<uint32_t> v(num());
  for (uint32_t& w : v) w = (uint32_t)num();
  return v;
}
int nib(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }
void unhex(uint8_t* out, const std::string& h, size_t n) {
  for (size_t i = 0; i < n; ++i) out[i] = (uint8_t)(nib(h[2 * i]) << 4 | nib(h[2 * i + 1]));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  in.open(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::vector<uint32_t> prog;
  std::string tag;
  size_t label = 0;
  int fails = 0;
  for (; in >> tag; ++label) {
    if (tag == "P") {
      prog = words();
    } else if (tag == "K") {
      const uint64_t max_field = num();
      const int want = (int)num();
      const std::vector<uint32_t> p = words();
      uint32_t* heap = new uint32_t[p.size()];
      std::memcpy(heap, p.data(), 4 * p.size());
      const int got = hc_ssz_ragged_prog_ok(heap, (uint32_t)p.size(), max_field);
      delete[] heap;
      if (got != want) { std::fprintf(stderr, "case %zu: prog_ok = %d, expected %d\n", label, got, want); ++fails; }
    } else if (tag == "I") {
      const size_t len = num();
      const std::string hex = tok();
      const int want_rc = (int)num();
      const std::string root_hex = tok();
      if ((hex == "-" ? 0 : hex.size()) != 2 * len || root_hex.size() != 64) {
        std::fprintf(stderr, "case %zu: bad case line\n", label);
        return 2;
      }
      uint8_t* item = new uint8_t[len];
      unhex(item, hex, len);
      uint8_t want[32], got[32];
      unhex(want, root_hex, 32);
      const int rc = hc_ssz_ragged_root(item, (uint32_t)len, prog.data(), (uint32_t)prog.size(), got);
      delete[] item;
      if (rc != want_rc || std::memcmp(got, want, 32)) {
        std::fprintf(stderr, "case %zu: rc = %d (expected %d), root %s\n", label, rc, want_rc,
                     std::memcmp(got, want, 32) ? "differs" : "equal");
        ++fails;
      }
    } else {
      std::fprintf(stderr, "unknown case tag %s\n", tag.c_str());
      return 2;
    }
  }
  std::printf("%zu cases, %d mismatches\n", label, fails);
  return fails ? 1 : 0;
}
