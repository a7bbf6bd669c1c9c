// Stand-alone check of bls381_regupd.hpp for sanitizer builds (g++ -fsanitize=address,undefined):
// reads cases with their expected results from the file named on the command line (whitespace-
// separated decimal numbers, written by tests/test_registry_updates_host.py from the model), runs
// them through the host exports of host_check_regupd.hpp and exits 1 on a mismatch.
//   R n stride cur fin k[6] elig[n] act[n] exit[n] wd[n] eff[n] rc indices[n] values[4n] summary[8]
//   Q n stride cur k[6] act[n] exit[n] rc queue[4]
// stride 8: plain arrays of exactly n entries; stride 121: records of exactly 121 n bytes, so a
// load past a field's last byte is a heap overflow the sanitizer reports.  The expected arrays
// follow rc only when rc is 0.  Every R case runs on one thread and on three.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>

#include "host_check_regupd.hpp"

namespace {
std::ifstream in;
uint64_t num() {
  std::string t;
  if (!(in >> t)) { std::fprintf(stderr, "unexpected end of input\n"); std::exit(2); }
  return std::strtoull(t.c_str(), nullptr, 10);
}
template <class T> std::vector<T> arr(size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (T)num();
  return v;
}
int fails = 0;
template <class T> void same(const char* what, size_t label, const std::vector<T>& got, const std::vector<T>& want) {
  for (size_t i = 0; i < want.size(); ++i)
    if (got[i] != want[i]) {
      std::fprintf(stderr, "case %zu: %s[%zu] = %llu, expected %llu\n", label, what, i, (unsigned long long)got[i],
                   (unsigned long long)want[i]);
      ++fails;
      return;
    }
}
const size_t OFFSET[5] = {80, 88, 96, 104, 113};   // eligibility, activation, exit, withdrawable, effective

// the fields as the call reads them: heap blocks of exactly the bytes they span
struct Fields {
  std::vector<uint8_t*> owned;
  const uint8_t* base[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~Fields() { for (uint8_t* p : owned) delete[] p; }
  void set(size_t n, size_t stride, const std::vector<uint64_t>* field[5]) {
    if (stride == 8) {
      for (int x = 0; x < 5; ++x) {
        if (!field[x]) continue;
        uint8_t* p = new uint8_t[n ? 8 * n : 1];   // never a zero-sized block
        if (n) std::memcpy(p, field[x]->data(), 8 * n);
        owned.push_back(p);
        base[x] = p;
      }
      return;
    }
    uint8_t* rec = new uint8_t[n ? stride * n : 1];
    std::memset(rec, 0xA5, n ? stride * n : 1);
    owned.push_back(rec);
    for (int x = 0; x < 5; ++x) {
      base[x] = rec + OFFSET[x];
      if (field[x])
        for (size_t i = 0; i < n; ++i) std::memcpy(rec + i * stride + OFFSET[x], &(*field[x])[i], 8);
    }
  }
};

void read_updates(size_t label) {
  const size_t n = num(), stride = num();
  const uint64_t cur = num(), fin = num();
  auto k = arr<uint64_t>(6);
  auto elig = arr<uint64_t>(n), act = arr<uint64_t>(n), ext = arr<uint64_t>(n), wd = arr<uint64_t>(n), eff = arr<uint64_t>(n);
  const int want_rc = (int)(int64_t)num();
  const std::vector<uint64_t>* field[5] = {&elig, &act, &ext, &wd, &eff};
  Fields f;
  f.set(n, stride, field);
  const std::vector<uint32_t> want_idx = want_rc ? std::vector<uint32_t>() : arr<uint32_t>(n);
  const std::vector<uint64_t> want_val = want_rc ? std::vector<uint64_t>() : arr<uint64_t>(4 * n);
  const std::vector<uint64_t> want_sum = want_rc ? std::vector<uint64_t>() : arr<uint64_t>(8);
  for (uint32_t threads : {1u, 3u}) {   // the sequential form, and slices that do not divide n
    std::vector<uint32_t> idx(n);
    std::vector<uint64_t> val(4 * n), sum(8);
    uint32_t* pi = new uint32_t[n ? n : 1];
    uint64_t* pv = new uint64_t[n ? 4 * n : 1];
    const int rc = hc_registry_updates_threads(n, f.base[0], f.base[1], f.base[2], f.base[3], f.base[4], stride, cur, fin,
                                               k.data(), threads, pi, pv, sum.data());
    if (n) std::memcpy(idx.data(), pi, 4 * n), std::memcpy(val.data(), pv, 32 * n);
    delete[] pi;
    delete[] pv;
    if ((rc != 0) != (want_rc != 0)) {
      std::fprintf(stderr, "case %zu: rc = %d, expected %d\n", label, rc, want_rc);
      ++fails;
    }
    if (want_rc) continue;
    same("indices", label, idx, want_idx);
    same("values", label, val, want_val);
    same("summary", label, sum, want_sum);
  }
}

void read_queue(size_t label) {
  const size_t n = num(), stride = num();
  const uint64_t cur = num();
  auto k = arr<uint64_t>(6);
  auto act = arr<uint64_t>(n), ext = arr<uint64_t>(n);
  const int want_rc = (int)(int64_t)num();
  const std::vector<uint64_t>* field[5] = {nullptr, &act, &ext, nullptr, nullptr};
  Fields f;
  f.set(n, stride, field);
  std::vector<uint64_t> q(4);
  const int rc = hc_exit_queue(n, f.base[1], f.base[2], stride, cur, k.data(), q.data());
  if ((rc != 0) != (want_rc != 0)) {
    std::fprintf(stderr, "case %zu: rc = %d, expected %d\n", label, rc, want_rc);
    ++fails;
  }
  if (want_rc) return;
  same("queue", label, q, arr<uint64_t>(4));
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  in.open(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string tag;
  size_t label = 0;
  while (in >> tag) {
    if (tag == "R") read_updates(label);
    else if (tag == "Q") read_queue(label);
    else { std::fprintf(stderr, "unknown case tag %s\n", tag.c_str()); return 2; }
    ++label;
  }
  std::printf("%zu cases, %d mismatches\n", label, fails);
  return fails ? 1 : 0;
}
