// Stand-alone check of bls381_rewards.hpp for sanitizer builds (g++ -fsanitize=address,undefined):
// reads cases with their expected results from the file named on the command line (whitespace-
// separated decimal numbers, written by tests/test_rewards_host.py from the model), runs them
// through the host exports of host_check_rewards.hpp and exits 1 on the first mismatch.
//   M a b d q ovf                         mul_div_u64
//   S n r                                 isqrt_u64
//   V / D / L / H ...                     votes / deltas / slashings / hysteresis (read_* below)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>

#include "host_check_rewards.hpp"

namespace {
std::ifstream in;
uint64_t num() {
  std::string t;
  if (!(in >> t)) { std::fprintf(stderr, "unexpected end of input\n"); std::exit(2); }
  return std::strtoull(t.c_str(), nullptr, 10);
}
template <class T> std::vector<T> arr(size_t n) {
  std::vector<T> v(n + 1);   // never empty: data() is a valid pointer
  for (size_t i = 0; i < n; ++i) v[i] = (T)num();
  v.resize(n);
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

void read_votes(size_t label) {
  const size_t nc = num(), n_sh = num(), nv = num();
  auto coff = arr<uint32_t>(nc), clen = arr<uint32_t>(nc), sh = arr<uint32_t>(n_sh);
  auto slashed = arr<uint8_t>(nv);
  auto eff = arr<uint64_t>(nv);
  auto att_off = arr<uint32_t>(nc + 1);
  const size_t n_att = num();
  auto bits_off = arr<uint32_t>(n_att + 1);
  const size_t nbits = num();
  auto bits = arr<uint8_t>(nbits);
  auto flags = arr<uint8_t>(n_att);
  auto delay = arr<uint64_t>(n_att);
  auto prop = arr<uint32_t>(n_att), cand = arr<uint32_t>(n_att), cand_count = arr<uint32_t>(nc);
  auto want_votes = arr<uint32_t>(nv), want_cof = arr<uint32_t>(nv);
  auto want_delay = arr<uint64_t>(nv);
  auto want_prop = arr<uint32_t>(nv), want_win = arr<uint32_t>(nc);
  auto want_wbal = arr<uint64_t>(nc), want_cbal = arr<uint64_t>(nc), want_tot = arr<uint64_t>(3);
  std::vector<uint32_t> votes(nv), cof(nv), iprop(nv), win(nc);
  std::vector<uint64_t> idelay(nv), wbal(nc), cbal(nc), tot(3);
  const int rc = hc_epoch_votes(nc, coff.data(), clen.data(), sh.data(), nv, slashed.data(), 1, (const uint8_t*)eff.data(),
                                8, att_off.data(), bits_off.data(), bits.data(), flags.data(), delay.data(), prop.data(),
                                cand.data(), cand_count.data(), votes.data(), idelay.data(), iprop.data(), cof.data(),
                                win.data(), wbal.data(), cbal.data(), tot.data());
  if (rc) { std::fprintf(stderr, "case %zu: hc_epoch_votes returned %d\n", label, rc); ++fails; return; }
  for (size_t i = 0; i < nv; ++i)
    if (!(votes[i] & 1u)) { idelay[i] = want_delay[i]; iprop[i] = want_prop[i]; }   // written only with bit 0
  same("votes", label, votes, want_votes);
  same("committee_of", label, cof, want_cof);
  same("incl_delay", label, idelay, want_delay);
  same("incl_proposer", label, iprop, want_prop);
  same("winner", label, win, want_win);
  same("winner_balance", label, wbal, want_wbal);
  same("committee_balance", label, cbal, want_cbal);
  same("totals", label, tot, want_tot);
}

void read_deltas(size_t label) {
  const size_t n = num(), nc = num();
  auto act = arr<uint64_t>(n), ext = arr<uint64_t>(n), wd = arr<uint64_t>(n), eff = arr<uint64_t>(n);
  auto slashed = arr<uint8_t>(n);
  auto votes = arr<uint32_t>(n);
  auto delay = arr<uint64_t>(n);
  auto prop = arr<uint32_t>(n), cof = arr<uint32_t>(n);
  auto wbal = arr<uint64_t>(nc), cbal = arr<uint64_t>(nc), tot = arr<uint64_t>(3), bal = arr<uint64_t>(n);
  const uint64_t prev = num(), fin = num(), total = num();
  auto k = arr<uint64_t>(6);
  const uint32_t which = (uint32_t)num();
  auto want_r = arr<uint64_t>(n), want_p = arr<uint64_t>(n), want_b = arr<uint64_t>(n);
  const uint64_t want_ovf = num();
  std::vector<uint64_t> r(n), p(n);
  uint64_t ovf = 0;
  // new_balances aliases balances, as the engine allows
  const int rc = hc_epoch_deltas(n, (const uint8_t*)act.data(), (const uint8_t*)ext.data(), (const uint8_t*)wd.data(),
                                 (const uint8_t*)eff.data(), 8, slashed.data(), 1, votes.data(), delay.data(), prop.data(),
                                 cof.data(), nc, wbal.data(), cbal.data(), tot.data(), bal.data(), prev, fin, total,
                                 k.data(), which, r.data(), p.data(), bal.data(), &ovf);
  if (rc) { std::fprintf(stderr, "case %zu: hc_epoch_deltas returned %d\n", label, rc); ++fails; return; }
  same("rewards", label, r, want_r);
  same("penalties", label, p, want_p);
  same("new_balances", label, bal, want_b);
  same("overflows", label, std::vector<uint64_t>{ovf}, std::vector<uint64_t>{want_ovf});
}

void read_slashings(size_t label) {
  const size_t n = num();
  auto slashed = arr<uint8_t>(n);
  auto wd = arr<uint64_t>(n), eff = arr<uint64_t>(n), bal = arr<uint64_t>(n);
  const uint64_t cur = num(), tp = num(), total = num(), len = num(), q = num();
  auto want = arr<uint64_t>(n);
  const int rc = hc_epoch_slashings(n, slashed.data(), 1, (const uint8_t*)wd.data(), (const uint8_t*)eff.data(), 8, cur, tp,
                                    total, len, q, bal.data());
  if (rc) { std::fprintf(stderr, "case %zu: hc_epoch_slashings returned %d\n", label, rc); ++fails; return; }
  same("balances", label, bal, want);
}

void read_hysteresis(size_t label) {
  const size_t n = num();
  auto bal = arr<uint64_t>(n), eff = arr<uint64_t>(n);
  const uint64_t inc = num(), max = num();
  auto want_idx = arr<uint32_t>(n);
  auto want_val = arr<uint64_t>(n);
  const uint64_t want_changed = num();
  std::vector<uint32_t> idx(n);
  std::vector<uint64_t> val(n);
  uint64_t changed = 0;
  const int rc = hc_effective_balances(n, bal.data(), (const uint8_t*)eff.data(), 8, inc, max, idx.data(), val.data(), &changed);
  if (rc) { std::fprintf(stderr, "case %zu: hc_effective_balances returned %d\n", label, rc); ++fails; return; }
  same("indices", label, idx, want_idx);
  same("values", label, val, want_val);
  same("changed", label, std::vector<uint64_t>{changed}, std::vector<uint64_t>{want_changed});
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.txt\n", argv[0]); return 2; }
  in.open(argv[1]);
  if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  std::string cmd;
  size_t label = 0, ran = 0;
  while (in >> cmd) {
    ++label;
    if (cmd == "M") {
      const uint64_t a = num(), b = num(), d = num(), q = num(), want_ovf = num();
      uint32_t ovf = 0;
      const uint64_t got = hc_mul_div_u64(a, b, d, &ovf);
      if (got != q || ovf != want_ovf) {
        std::fprintf(stderr, "case %zu: mul_div_u64(%llu, %llu, %llu) = %llu / %u\n", label, (unsigned long long)a,
                     (unsigned long long)b, (unsigned long long)d, (unsigned long long)got, ovf);
        ++fails;
      }
    } else if (cmd == "S") {
      const uint64_t n = num(), r = num();
      if (hc_isqrt_u64(n) != r) {
        std::fprintf(stderr, "case %zu: isqrt_u64(%llu) = %llu\n", label, (unsigned long long)n,
                     (unsigned long long)hc_isqrt_u64(n));
        ++fails;
      }
    } else if (cmd == "V") {
      read_votes(label);
    } else if (cmd == "D") {
      read_deltas(label);
    } else if (cmd == "L") {
      read_slashings(label);
    } else if (cmd == "H") {
      read_hysteresis(label);
    } else {
      std::fprintf(stderr, "case %zu: unknown command %s\n", label, cmd.c_str());
      return 2;
    }
    ++ran;
  }
  std::printf("%zu cases, %d failed\n", ran, fails);
  return fails ? 1 : 0;
}
