// Stand-alone check of bls381_forkchoice.hpp for sanitizer builds (g++ -fsanitize=address,undefined):
// reads a script of calls with their expected results from the file named on the command line
// (whitespace-separated decimal numbers, written by tests/test_fork_choice_host.py from the model),
// runs them through the host exports of host_check_forkchoice.hpp and exits 1 on a mismatch.
//   S vcap bcap                                              a new store (the one before is destroyed)
//   B n roots[32 n] parents[32 n] slots[n] rc ids[n]
//   A n_att att_off[n_att + 1] n_entries entries[n_entries] slots[n_att] targets[n_att] has_ok ok[n_att] rc skipped
//   L first n rc slots[n] targets[n]
//   P node rc
//   H start n stride epoch act[n] exit[n] eff[n] rc head root[32] n_blocks weights[n_blocks] status
// stride 8: plain arrays of exactly n entries; stride 121: records of exactly 121 n bytes, so a
// load past a field's last byte is a heap overflow the sanitizer reports.  Every input array is a
// heap block of exactly its size.  The expected values follow rc only when rc is 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>

#include "host_check_forkchoice.hpp"

namespace {
std::ifstream in;
uint64_t num() {
  std::string t;
  if (!(in >> t)) { std::fprintf(stderr, "unexpected end of input\n"); std::exit(2); }
  return std::strtoull(t.c_str(), nullptr, 10);
}
// a heap block of exactly n entries (never zero-sized)
template <class T> struct Block {
  size_t n;
  T* p;
  explicit Block(size_t count) : n(count), p(new T[count ? count : 1]) {}
  ~Block() { delete[] p; }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
  void read() { for (size_t i = 0; i < n; ++i) p[i] = (T)num(); }
};
int fails = 0;
size_t label = 0;
template <class T> void same(const char* what, const T* got, const T* want, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (got[i] != want[i]) {
      std::fprintf(stderr, "call %zu: %s[%zu] = %llu, expected %llu\n", label, what, i, (unsigned long long)got[i],
                   (unsigned long long)want[i]);
      ++fails;
      return;
    }
}
bool same_rc(int rc, int want_rc) {
  if ((rc != 0) != (want_rc != 0)) {
    std::fprintf(stderr, "call %zu: rc = %d, expected %d\n", label, rc, want_rc);
    ++fails;
  }
  return rc == 0 && want_rc == 0;
}
const size_t OFFSET[3] = {88, 96, 113};   // activation, exit, effective balance

void* store = nullptr;

void blocks() {
  const size_t n = num();
  Block<uint8_t> roots(32 * n), parents(32 * n);
  Block<uint64_t> slots(n);
  Block<uint32_t> ids(n), want(n);
  roots.read(), parents.read(), slots.read();
  const int want_rc = (int)(int64_t)num();
  if (!same_rc(hc_fork_choice_add_blocks(store, n, roots.p, parents.p, slots.p, ids.p), want_rc)) return;
  want.read();
  same("ids", ids.p, want.p, n);
  for (size_t k = 0; k < n; ++k)
    if (hc_fork_choice_node(store, roots.p + 32 * k) != want.p[k]) {
      std::fprintf(stderr, "call %zu: the lookup of block %zu differs\n", label, k);
      ++fails;
    }
}

void attestations() {
  const size_t n_att = num();
  Block<uint32_t> off(n_att + 1);
  off.read();
  const size_t n_entries = num();
  Block<uint32_t> entries(n_entries), targets(n_att);
  Block<uint64_t> slots(n_att);
  entries.read(), slots.read(), targets.read();
  const bool has_ok = num() != 0;
  Block<uint8_t> ok(has_ok ? n_att : 0);
  ok.read();
  const int want_rc = (int)(int64_t)num();
  uint64_t skipped = ~(uint64_t)0;
  if (!same_rc(hc_fork_choice_on_attestations(store, n_att, off.p, entries.p, slots.p, targets.p, has_ok ? ok.p : nullptr,
                                              &skipped),
               want_rc))
    return;
  const uint64_t want = num();
  same("skipped", &skipped, &want, 1);
}

void latest() {
  const size_t first = num(), n = num();
  const int want_rc = (int)(int64_t)num();
  Block<uint64_t> slots(n), want_slots(n);
  Block<uint32_t> targets(n), want_targets(n);
  if (!same_rc(hc_fork_choice_read_latest(store, first, n, slots.p, targets.p), want_rc)) return;
  want_slots.read(), want_targets.read();
  same("latest slots", slots.p, want_slots.p, n);
  same("latest targets", targets.p, want_targets.p, n);
}

void prune() {
  const uint32_t node = (uint32_t)num();
  const int want_rc = (int)(int64_t)num();
  same_rc(hc_fork_choice_prune(store, node), want_rc);
}

void head() {
  const uint32_t start = (uint32_t)num();
  const size_t n = num(), stride = num();
  const uint64_t epoch = num();
  Block<uint64_t> field[3] = {Block<uint64_t>(n), Block<uint64_t>(n), Block<uint64_t>(n)};
  for (auto& f : field) f.read();
  // the fields as the call reads them: blocks of exactly the bytes they span
  std::unique_ptr<Block<uint8_t>> rec;
  const uint8_t* base[3];
  if (stride == 8) {
    for (int x = 0; x < 3; ++x) base[x] = (const uint8_t*)field[x].p;
  } else {
    rec.reset(new Block<uint8_t>(stride * n));
    std::memset(rec->p, 0xA5, n ? stride * n : 1);
    for (int x = 0; x < 3; ++x) {
      base[x] = rec->p + OFFSET[x];
      for (size_t i = 0; i < n; ++i) std::memcpy(rec->p + i * stride + OFFSET[x], &field[x].p[i], 8);
    }
  }
  const int want_rc = (int)(int64_t)num();
  const size_t B = (size_t)hc_fork_choice_block_count(store);
  uint32_t got_head = 0;
  uint64_t status[bls381::FCS_WORDS] = {0};
  Block<uint8_t> root(32), want_root(32);
  Block<uint64_t> weights(B);
  if (!same_rc(hc_fork_choice_head(store, start, n, base[0], base[1], base[2], stride, epoch, &got_head, root.p, weights.p,
                                   status),
               want_rc))
    return;
  const uint32_t want_head = (uint32_t)num();
  want_root.read();
  const size_t want_blocks = num();
  Block<uint64_t> want_weights(want_blocks);
  want_weights.read();
  const uint64_t want_status = num();
  same("head", &got_head, &want_head, 1);
  same("root", root.p, want_root.p, 32);
  same("block count", &B, &want_blocks, 1);
  if (B == want_blocks) same("weights", weights.p, want_weights.p, B);
  same("status", status, &want_status, 1);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s script.txt\n", argv[0]); return 2; }
  in.open(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string tag;
  while (in >> tag) {
    if (tag == "S") {
      hc_fork_choice_destroy(store);
      const uint64_t vcap = num(), bcap = num();
      store = hc_fork_choice_create(vcap, bcap);
      if (!store) { std::fprintf(stderr, "call %zu: no store\n", label); return 2; }
    } else if (!store) { std::fprintf(stderr, "call %zu: no store yet\n", label); return 2; }
    else if (tag == "B") blocks();
    else if (tag == "A") attestations();
    else if (tag == "L") latest();
    else if (tag == "P") prune();
    else if (tag == "H") head();
    else { std::fprintf(stderr, "unknown tag %s\n", tag.c_str()); return 2; }
    ++label;
  }
  hc_fork_choice_destroy(store);
  std::printf("%zu calls, %d mismatches\n", label, fails);
  return fails ? 1 : 0;
}
