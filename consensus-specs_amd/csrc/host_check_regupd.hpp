// Host exports over bls381_regupd.hpp: the kernels' per-item functions, the exit queue's closed
// form and the radix select in the kernels' order, over contiguous slices of the registry: one
// slice is the plain sequential form, more run a thread each (the slices' counts and candidate
// lists are joined in index order, as the tile scan joins the tiles').  Included once by
// host_check.cpp (lib/libbls381_hostcheck.so) and once by regupd_check_main.cpp (the stand-alone
// sanitizer program).
#pragma once
#include <cstdint>
#include <thread>
#include <vector>

#include "bls381_regupd.hpp"

namespace hc_regupd {
using namespace bls381;

inline bool setup(uint64_t n, size_t stride, uint64_t current_epoch, const uint64_t* finalized_epoch,
                  const uint64_t* constants6, registry_constants* kc, regupd_epochs* e) {
  *kc = registry_constants{constants6[0], constants6[1], constants6[2], constants6[3], constants6[4], constants6[5]};
  if (n > 0xFFFFFFFFull || stride < 8 || kc->churn_limit_quotient == 0) return false;
  e->cur = current_epoch;
  e->delayed_fin = 0;
  if (!delayed_epoch(current_epoch, kc->activation_exit_delay, &e->delayed_cur)) return false;
  if (finalized_epoch && !delayed_epoch(*finalized_epoch, kc->activation_exit_delay, &e->delayed_fin)) return false;
  return true;
}

// body(t) for slice t of `slices`, on a thread each when there is more than one
template <class Body> inline void run_slices(uint32_t slices, Body body) {
  if (slices <= 1) {
    body(0u);
    return;
  }
  std::vector<std::thread> pool;
  for (uint32_t t = 0; t < slices; ++t) pool.emplace_back(body, t);
  for (auto& th : pool) th.join();
}
inline uint64_t slice_begin(uint64_t n, uint32_t slices, uint32_t t) { return n / slices * t + (n % slices < t ? n % slices : t); }

// the L-th smallest composite of K > L entries: twelve histogram passes, as k_regupd_select (a
// slice's histogram is a workgroup's, their sum the global one)
inline void select(const std::vector<uint64_t>& keys, const std::vector<uint32_t>& idx, uint64_t L, uint32_t slices,
                   uint64_t* tkey, uint64_t* tidx) {
  uint64_t pkey = 0, rank = L - 1;
  uint32_t pidx = 0;
  std::vector<uint32_t> part((size_t)slices * REGUPD_BINS);
  for (uint32_t pass = 0; pass < REGUPD_DIGITS; ++pass) {
    run_slices(slices, [&](uint32_t t) {
      uint32_t* bins = part.data() + (size_t)t * REGUPD_BINS;
      for (uint32_t d = 0; d < REGUPD_BINS; ++d) bins[d] = 0;
      for (size_t j = slice_begin(keys.size(), slices, t), end = slice_begin(keys.size(), slices, t + 1); j < end; ++j)
        if (regupd_prefix_match(keys[j], idx[j], pkey, pidx, pass)) ++bins[regupd_digit(keys[j], idx[j], pass)];
    });
    uint64_t excl = 0;
    for (uint32_t d = 0; d < REGUPD_BINS; ++d) {
      uint64_t bin = 0;
      for (uint32_t t = 0; t < slices; ++t) bin += part[(size_t)t * REGUPD_BINS + d];
      if (rank < excl + bin) {
        regupd_prefix_push(&pkey, &pidx, pass, d);
        rank -= excl;
        break;
      }
      excl += bin;
    }
  }
  *tkey = pkey;
  *tidx = pidx;
}

// bls381_registry_updates over host arrays in `slices` slices
inline int registry_updates(uint64_t n, const regupd_fields& f, const regupd_epochs& e, const registry_constants& kc,
                            uint32_t slices, uint32_t* indices, uint64_t* values, uint64_t* summary) {
  struct Slice {
    uint64_t active = 0, ejected = 0, first_rank = 0, counts[4] = {0, 0, 0, 0};
    exit_peak peak{0, 0};
    std::vector<uint64_t> keys;
    std::vector<uint32_t> idx;
  };
  std::vector<Slice> sl(slices);
  // k_regupd_count and k_regupd_compact
  run_slices(slices, [&](uint32_t t) {
    Slice& s = sl[t];
    for (uint64_t i = slice_begin(n, slices, t), end = slice_begin(n, slices, t + 1); i < end; ++i) {
      const regupd_item it = regupd_load(f, (size_t)i, e, kc);
      s.active += it.active;
      s.ejected += it.ejected;
      s.peak = peak_combine(s.peak, peak_of(it.ext));
      if (it.candidate) {
        s.keys.push_back(it.new_elig);
        s.idx.push_back((uint32_t)i);
      }
    }
  });
  // k_regupd_scan
  uint64_t active = 0, ejected = 0;
  exit_peak peak{0, 0};
  std::vector<uint64_t> keys;
  std::vector<uint32_t> idx;
  for (Slice& s : sl) {
    s.first_rank = ejected;
    active += s.active;
    ejected += s.ejected;
    peak = peak_combine(peak, s.peak);
    keys.insert(keys.end(), s.keys.begin(), s.keys.end());
    idx.insert(idx.end(), s.idx.begin(), s.idx.end());
  }
  const regupd_queue q = regupd_derive(active, peak, e.delayed_cur, kc);
  if (q.L == 0) return -1;
  uint64_t tkey = ~(uint64_t)0, tidx = ~(uint64_t)0;
  if (keys.size() > q.L) select(keys, idx, q.L, slices, &tkey, &tidx);
  // k_regupd_apply
  run_slices(slices, [&](uint32_t t) {
    Slice& s = sl[t];
    uint64_t rank = s.first_rank;
    for (uint64_t i = slice_begin(n, slices, t), end = slice_begin(n, slices, t + 1); i < end; ++i) {
      const regupd_item it = regupd_load(f, (size_t)i, e, kc);
      const regupd_result r = regupd_apply_item(it, (uint32_t)i, rank, q, tkey, tidx, e, kc);
      rank += it.ejected;
      indices[i] = r.changed ? (uint32_t)i : REGUPD_NONE;
      for (int x = 0; x < 4; ++x) values[4 * i + x] = r.v[x];
      s.counts[0] += r.eligible_set;
      s.counts[1] += r.activated;
      s.counts[2] += r.changed;
      s.counts[3] += r.wrapped;
    }
  });
  for (uint32_t x = 0; x < RS_WORDS; ++x) summary[x] = 0;
  summary[RS_EJECTED] = ejected;
  summary[RS_ACTIVE] = active;
  summary[RS_CHURN] = q.L;
  summary[RS_E0] = q.E0;
  for (const Slice& s : sl) {
    summary[RS_ELIGIBLE] += s.counts[0];
    summary[RS_ACTIVATED] += s.counts[1];
    summary[RS_CHANGED] += s.counts[2];
    summary[RS_STATUS] += s.counts[3];
  }
  return 0;
}
}  // namespace hc_regupd

extern "C" {

// bls381_exit_queue over host arrays: queue4 = E0, c0, L, the active count.  constants6: the six
// fields of bls381_registry_constants in their order.  0, or -1 for arguments the call rejects.
int hc_exit_queue(uint64_t n, const uint8_t* activation, const uint8_t* exit_, size_t stride, uint64_t current_epoch,
                  const uint64_t* constants6, uint64_t* queue4) {
  using namespace bls381;
  registry_constants kc;
  regupd_epochs e;
  if (!hc_regupd::setup(n, stride, current_epoch, nullptr, constants6, &kc, &e)) return -1;
  const u64_field act = make_u64_field(activation, stride), ext = make_u64_field(exit_, stride);
  uint64_t active = 0;
  exit_peak peak{0, 0};
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t x = field_load(ext, (size_t)i);
    active += field_load(act, (size_t)i) <= current_epoch && current_epoch < x;
    peak = peak_combine(peak, peak_of(x));
  }
  const regupd_queue q = regupd_derive(active, peak, e.delayed_cur, kc);
  if (q.L == 0) return -1;
  queue4[0] = q.E0;
  queue4[1] = q.c0;
  queue4[2] = q.L;
  queue4[3] = active;
  return 0;
}

// bls381_registry_updates over host arrays: indices (n), values (4 n), summary (8); `threads`
// slices of the registry, a thread each (0 or 1: the calling thread alone; at most 64)
int hc_registry_updates_threads(uint64_t n, const uint8_t* eligibility, const uint8_t* activation, const uint8_t* exit_,
                                const uint8_t* withdrawable, const uint8_t* effective_balance, size_t stride,
                                uint64_t current_epoch, uint64_t finalized_epoch, const uint64_t* constants6,
                                uint32_t threads, uint32_t* indices, uint64_t* values, uint64_t* summary) {
  using namespace bls381;
  registry_constants kc;
  regupd_epochs e;
  if (threads > 64 || !hc_regupd::setup(n, stride, current_epoch, &finalized_epoch, constants6, &kc, &e)) return -1;
  const regupd_fields f{make_u64_field(eligibility, stride), make_u64_field(activation, stride),
                        make_u64_field(exit_, stride), make_u64_field(withdrawable, stride),
                        make_u64_field(effective_balance, stride)};
  return hc_regupd::registry_updates(n, f, e, kc, threads ? threads : 1u, indices, values, summary);
}

int hc_registry_updates(uint64_t n, const uint8_t* eligibility, const uint8_t* activation, const uint8_t* exit_,
                        const uint8_t* withdrawable, const uint8_t* effective_balance, size_t stride,
                        uint64_t current_epoch, uint64_t finalized_epoch, const uint64_t* constants6, uint32_t* indices,
                        uint64_t* values, uint64_t* summary) {
  return hc_registry_updates_threads(n, eligibility, activation, exit_, withdrawable, effective_balance, stride,
                                     current_epoch, finalized_epoch, constants6, 1, indices, values, summary);
}

}  // extern "C"
