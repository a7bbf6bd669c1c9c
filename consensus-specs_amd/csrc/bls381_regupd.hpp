// Registry updates on gfx950: eligibility, ejections through the exit queue, and the activation
// queue: process_registry_updates computed where the validator records are.
//
// Reference: specs/core/0_beacon-chain.md:1480-1502 (process_registry_updates), :1110-1128
// (initiate_validator_exit), :1081-1088 (get_churn_limit) and :1071-1075
// (get_delayed_activation_exit_epoch).
//
// Validator fields are read through u64_field (bls381_epoch.hpp): offsets 80 / 88 / 96 / 104 / 113
// of the 121-byte records for activation_eligibility_epoch / activation_epoch / exit_epoch /
// withdrawable_epoch / effective_balance, or stride 8 over plain arrays.
//
// Both queues of the spec read as sequential loops and both have closed forms.
//
// The exit queue.  initiate_validator_exit looks at the largest exit_epoch in the registry (or
// delayed(cur) if that is larger) and at how many validators hold it; when that count has reached
// the churn limit L the epoch moves on by one.  With (E0, c0) that pair before the call, the k-th
// ejected validator in index order therefore gets E0 + (min(c0, L) + k) / L: a count above L
// behaves as L (the first exit moves on, and the new epoch starts at 1).  L itself does not move
// during the call, because every epoch the call writes lies above cur.  (max, count at max) is an
// associative pair, so one reduction finds both; k is an exclusive rank that ballots give.
//
// The activation queue.  The spec sorts the candidates by eligibility epoch -- a stable sort over
// ascending indices, so by the pair (eligibility, index) -- and takes the first L.  Taking the first
// L of a sort is a selection: the L-th smallest pair is a threshold and a candidate is dequeued
// when its own pair is at or below it.  The pair is a 96-bit composite (64-bit key, 32-bit index)
// and unique, so a radix select over twelve 8-bit digits from the top finds it without a tie pass.
// With at most L candidates the threshold stays at all-ones and everyone is dequeued.
//
// Overflow: delayed(cur) and delayed(finalized) are checked by the caller.  An exit_epoch or
// withdrawable_epoch that would pass 2^64 - 1 becomes 2^64 - 1, and the validator adds 1 to the
// call's status word (once, whichever of the two wrapped).
#pragma once
#include "bls381_epoch.hpp"

namespace bls381 {

constexpr uint64_t FAR_FUTURE = ~(uint64_t)0;
constexpr uint32_t REGUPD_NONE = 0xFFFFFFFFu;
constexpr uint32_t REGUPD_DIGITS = 12;   // 8 of the key, 4 of the index, most significant first
constexpr uint32_t REGUPD_BINS = 256;
// the device form cannot return an error for a churn limit of 0 that only the data shows: it
// writes no change and sets this bit of the status word
constexpr uint64_t REGUPD_STATUS_NO_CHURN = (uint64_t)1 << 63;

struct registry_constants {
  uint64_t max_effective_balance, ejection_balance, activation_exit_delay, min_validator_withdrawability_delay,
      min_per_epoch_churn_limit, churn_limit_quotient;
};
struct regupd_fields {
  u64_field eligibility, activation, exit_, withdrawable, effective;
};
struct regupd_epochs {
  uint64_t cur, delayed_cur, delayed_fin;   // delayed(e) = e + 1 + activation_exit_delay
};
// e + 1 + delay, false when it wraps
inline bool delayed_epoch(uint64_t e, uint64_t delay, uint64_t* out) {
  const uint64_t a = e + 1, b = a + delay;
  *out = b;
  return a != 0 && b >= a;
}

// ---- the scalars of a call, in the workspace (uint64 each) -----------------------------------
enum : uint32_t {
  RU_L = 0,        // the churn limit
  RU_E0 = 1,       // the exit queue's epoch before the call
  RU_C0 = 2,       // how many validators hold it
  RU_K = 3,        // candidates of the activation queue
  RU_TKEY = 4,     // the threshold pair
  RU_TIDX = 5,
  RU_ACTIVE = 6,   // active validators at cur
  RU_EJECTED = 7,
  RU_SEL = 8,      // 13 x (prefix key, prefix index, rank left): entry q has q digits fixed
  RU_SCALARS = RU_SEL + 3 * (REGUPD_DIGITS + 1)
};
// the summary a call hands back
enum : uint32_t { RS_ELIGIBLE = 0, RS_EJECTED, RS_ACTIVATED, RS_CHANGED, RS_ACTIVE, RS_CHURN, RS_E0, RS_STATUS, RS_WORDS };

// ---- per-validator facts ---------------------------------------------------------------------
struct regupd_item {
  uint64_t elig, act, ext, wd;   // the four epochs as they are
  uint64_t new_elig;             // elig' (:1483-1487)
  bool active, ejected, candidate;
};
BLS_DEV_INLINE regupd_item regupd_load(const regupd_fields& f, size_t i, const regupd_epochs& e,
                                       const registry_constants& k) {
  regupd_item it;
  it.elig = field_load(f.eligibility, i);
  it.act = field_load(f.activation, i);
  it.ext = field_load(f.exit_, i);
  it.wd = field_load(f.withdrawable, i);
  const uint64_t eff = field_load(f.effective, i);
  it.new_elig = (it.elig == FAR_FUTURE && eff >= k.max_effective_balance) ? e.cur : it.elig;
  it.active = it.act <= e.cur && e.cur < it.ext;
  it.ejected = it.active && eff <= k.ejection_balance && it.ext == FAR_FUTURE;
  it.candidate = it.new_elig != FAR_FUTURE && it.act >= e.delayed_fin;
  return it;
}

// ---- the exit queue: (largest exit_epoch != FAR, how many hold it) ---------------------------
struct exit_peak {
  uint64_t epoch;
  uint32_t count;   // 0: no exited validator
};
BLS_INLINE exit_peak peak_combine(const exit_peak& a, const exit_peak& b) {
  if (b.count == 0) return a;
  if (a.count == 0 || b.epoch > a.epoch) return b;
  if (a.epoch > b.epoch) return a;
  return exit_peak{a.epoch, a.count + b.count};
}
BLS_INLINE exit_peak peak_of(uint64_t exit_epoch) {
  return exit_peak{exit_epoch, exit_epoch != FAR_FUTURE ? 1u : 0u};
}
struct regupd_queue {
  uint64_t L, E0, c0;
};
BLS_INLINE regupd_queue regupd_derive(uint64_t active_count, const exit_peak& peak, uint64_t delayed_cur,
                                      const registry_constants& k) {
  regupd_queue q;
  q.L = active_count / k.churn_limit_quotient;
  if (q.L < k.min_per_epoch_churn_limit) q.L = k.min_per_epoch_churn_limit;
  const bool held = peak.count != 0 && peak.epoch >= delayed_cur;
  q.E0 = held ? peak.epoch : delayed_cur;
  q.c0 = held ? peak.count : 0;
  return q;
}
// the epochs of the rank-th exit after the queue q (rank from 0, q.L != 0); true when one wrapped
BLS_INLINE bool regupd_exit_epochs(const regupd_queue& q, uint64_t rank, uint64_t withdrawability_delay,
                                   uint64_t* exit_epoch, uint64_t* withdrawable_epoch) {
  const uint64_t place = (q.c0 < q.L ? q.c0 : q.L) + rank;   // below 2^33 + 2^32
  const uint64_t e = q.E0 + place / q.L;
  bool wrapped = e < q.E0;
  const uint64_t ex = wrapped ? FAR_FUTURE : e;
  const uint64_t w = ex + withdrawability_delay;
  if (w < ex) wrapped = true;
  *exit_epoch = ex;
  *withdrawable_epoch = w < ex ? FAR_FUTURE : w;
  return wrapped;
}

// ---- the activation queue: digits and prefixes of the composite (key, index) ------------------
BLS_INLINE uint32_t regupd_digit(uint64_t key, uint32_t idx, uint32_t p) {
  return p < 8 ? (uint32_t)(key >> (56 - 8 * p)) & 255u : (idx >> (24 - 8 * (p - 8))) & 255u;
}
// the first q digits of (key, idx) equal those of (pkey, pidx), whose other digits are 0
BLS_INLINE bool regupd_prefix_match(uint64_t key, uint32_t idx, uint64_t pkey, uint32_t pidx, uint32_t q) {
  if (q == 0) return true;
  if (q <= 8) return (key >> (64 - 8 * q)) == (pkey >> (64 - 8 * q));
  if (key != pkey) return false;
  if (q >= 12) return idx == pidx;
  return (idx >> (32 - 8 * (q - 8))) == (pidx >> (32 - 8 * (q - 8)));
}
// the prefix with digit d appended as digit q
BLS_INLINE void regupd_prefix_push(uint64_t* pkey, uint32_t* pidx, uint32_t q, uint32_t d) {
  if (q < 8) *pkey |= (uint64_t)d << (56 - 8 * q);
  else *pidx |= d << (24 - 8 * (q - 8));
}
BLS_INLINE bool regupd_dequeued(uint64_t key, uint32_t idx, uint64_t tkey, uint64_t tidx) {
  return key < tkey || (key == tkey && (uint64_t)idx <= tidx);
}

// ---- one validator's result ------------------------------------------------------------------
struct regupd_result {
  uint64_t v[4];   // eligibility, activation, exit, withdrawable: new or old
  bool changed, eligible_set, activated, wrapped;
};
// rank: the validator's place among the ejected (read only when it.ejected)
BLS_DEV_INLINE regupd_result regupd_apply_item(const regupd_item& it, uint32_t i, uint64_t rank, const regupd_queue& q,
                                               uint64_t tkey, uint64_t tidx, const regupd_epochs& e,
                                               const registry_constants& k) {
  regupd_result r;
  r.v[0] = it.new_elig;
  r.v[1] = it.act;
  r.v[2] = it.ext;
  r.v[3] = it.wd;
  r.wrapped = false;
  if (it.ejected) r.wrapped = regupd_exit_epochs(q, rank, k.min_validator_withdrawability_delay, &r.v[2], &r.v[3]);
  if (it.candidate && it.act == FAR_FUTURE && regupd_dequeued(it.new_elig, i, tkey, tidx)) r.v[1] = e.delayed_cur;
  r.eligible_set = r.v[0] != it.elig;
  r.activated = r.v[1] != it.act;
  r.changed = r.eligible_set || r.activated || r.v[2] != it.ext || r.v[3] != it.wd;
  return r;
}

}  // namespace bls381
