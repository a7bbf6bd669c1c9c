// Host exports over bls381_rewards.hpp: the kernels' per-item functions and the committee walk
// run by one thread.  Included once by host_check.cpp (lib/libbls381_hostcheck.so) and once by
// rewards_check_main.cpp (the stand-alone sanitizer program).
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "bls381_rewards.hpp"

extern "C" {

// floor(a * b / d); *ovf_out = 1 when the quotient is 2^64 or more (the value is then 2^64 - 1)
uint64_t hc_mul_div_u64(uint64_t a, uint64_t b, uint64_t d, uint32_t* ovf_out) {
  *ovf_out = 0;
  return bls381::mul_div_u64(a, b, d, ovf_out);
}

uint64_t hc_isqrt_u64(uint64_t n) { return bls381::isqrt_u64(n); }

// bls381_epoch_votes over host arrays (votes_walk with one lane per committee, then the totals).
// 0, or -1 for a committee over 4,096 members or a bitfield that fails verify_bitfield.
int hc_epoch_votes(uint64_t n_committees, const uint32_t* committee_off, const uint32_t* committee_len,
                   const uint32_t* shuffled, uint64_t n_validators, const uint8_t* slashed, size_t slashed_stride,
                   const uint8_t* effective_balance, size_t stride, const uint32_t* att_off, const uint32_t* bits_off,
                   const uint8_t* bits, const uint8_t* att_flags, const uint64_t* att_delay, const uint32_t* att_proposer,
                   const uint32_t* att_candidate, const uint32_t* cand_count, uint32_t* votes, uint64_t* incl_delay,
                   uint32_t* incl_proposer, uint32_t* committee_of, uint32_t* winner, uint64_t* winner_balance,
                   uint64_t* committee_balance, uint64_t* totals) {
  using namespace bls381;
  for (uint64_t i = 0; i < n_validators; ++i) {
    votes[i] = 0;
    committee_of[i] = VOTES_NONE;
  }
  totals[0] = totals[1] = totals[2] = 0;
  if (n_committees == 0) return 0;
  const size_t n_att = att_off[n_committees];
  std::vector<votes_att> att(n_att);
  for (uint64_t c = 0; c < n_committees; ++c) {
    if (committee_len[c] > ATT_MAX_COMMITTEE) return -1;
    for (size_t a = att_off[c]; a < att_off[c + 1]; ++a) {
      const size_t nbytes = bits_off[a + 1] - bits_off[a];
      if (nbytes != ((size_t)committee_len[c] + 7) / 8 || (nbytes && !bitfield_ok(bits + bits_off[a], nbytes, committee_len[c])))
        return -1;
      att[a] = votes_att{att_delay[a], bits_off[a], att_flags[a], att_proposer[a], att_candidate[a]};
    }
  }
  std::unique_ptr<votes_lds> lds(new votes_lds);
  std::vector<uint64_t> partial(3 * n_committees);
  const u8_field sl = make_u8_field(slashed, slashed_stride);
  const u64_field eff = make_u64_field(effective_balance, stride);
  const auto no_sync = [] {};
  for (uint64_t c = 0; c < n_committees; ++c) {
    const votes_committee cm{committee_off[c], committee_len[c], att_off[c], att_off[c + 1] - att_off[c], cand_count[c]};
    votes_walk(lds.get(), 0u, 1u, no_sync, (uint32_t)c, cm, shuffled, (const votes_att*)att.data(), bits, sl, eff,
               n_validators, votes, incl_delay, incl_proposer, committee_of, winner, winner_balance, committee_balance,
               partial.data());
    for (int g = 0; g < 3; ++g) totals[g] += partial[3 * c + g];
  }
  return 0;
}

// bls381_epoch_deltas over host arrays: the per-validator function, the proposers' scatter as
// plain additions, then the application.  constants6: the six fields of bls381_reward_constants
// in their order.  *overflows_out = the status word.
int hc_epoch_deltas(uint64_t n, const uint8_t* activation, const uint8_t* exit_, const uint8_t* withdrawable,
                    const uint8_t* effective_balance, size_t stride, const uint8_t* slashed, size_t slashed_stride,
                    const uint32_t* votes, const uint64_t* incl_delay, const uint32_t* incl_proposer,
                    const uint32_t* committee_of, uint64_t n_committees, const uint64_t* winner_balance,
                    const uint64_t* committee_balance, const uint64_t* totals, const uint64_t* balances,
                    uint64_t previous_epoch, uint64_t finalized_epoch, uint64_t total_balance, const uint64_t* constants6,
                    uint32_t which, uint64_t* rewards, uint64_t* penalties, uint64_t* new_balances,
                    uint64_t* overflows_out) {
  using namespace bls381;
  *overflows_out = 0;
  if (stride < 8 || slashed_stride < 1 || which < 1 || which > 3 || previous_epoch == ~(uint64_t)0 ||
      finalized_epoch > previous_epoch || !constants6[1] || !constants6[2] || !constants6[5])
    return -1;
  deltas_in in;
  in.activation = make_u64_field(activation, stride);
  in.exit_ = make_u64_field(exit_, stride);
  in.withdrawable = make_u64_field(withdrawable, stride);
  in.effective = make_u64_field(effective_balance, stride);
  in.slashed = make_u8_field(slashed, slashed_stride);
  in.votes = votes;
  in.incl_delay = incl_delay;
  in.incl_proposer = incl_proposer;
  in.committee_of = committee_of;
  in.winner_balance = winner_balance;
  in.committee_balance = committee_balance;
  in.totals = totals;
  in.n = n;
  in.n_committees = n_committees;
  in.previous_epoch = previous_epoch;
  in.finalized_epoch = finalized_epoch;
  in.k = reward_constants{constants6[0], constants6[1], constants6[2], constants6[3], constants6[4], constants6[5]};
  in.which = which;
  const uint64_t total = floor_one(total_balance), root = isqrt_u64(total);
  std::vector<uint64_t> proposer_reward(n, 0);
  uint64_t overflows = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const validator_delta d = validator_deltas(in, total, root, (size_t)i);
    rewards[i] = d.reward;
    penalties[i] = d.penalty;
    if (d.proposer != VOTES_NONE) proposer_reward[d.proposer] += d.proposer_addend;
    overflows += d.overflows;
  }
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t ovf = 0;
    uint64_t reward;
    const uint64_t nb = apply_deltas(balances[i], rewards[i], proposer_reward[i], penalties[i], &reward, &ovf);
    rewards[i] = reward;
    new_balances[i] = nb;
    overflows += ovf;
  }
  *overflows_out = overflows;
  return 0;
}

// bls381_epoch_slashings over host arrays, balances in place
int hc_epoch_slashings(uint64_t n, const uint8_t* slashed, size_t slashed_stride, const uint8_t* withdrawable,
                       const uint8_t* effective_balance, size_t stride, uint64_t current_epoch, uint64_t total_penalties,
                       uint64_t total_balance, uint64_t latest_slashed_exit_length,
                       uint64_t min_slashing_penalty_quotient, uint64_t* balances) {
  using namespace bls381;
  if (stride < 8 || slashed_stride < 1 || min_slashing_penalty_quotient == 0) return -1;
  const u8_field sl = make_u8_field(slashed, slashed_stride);
  const u64_field wd = make_u64_field(withdrawable, stride), eff = make_u64_field(effective_balance, stride);
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t penalty = slashing_penalty(flag_load(sl, (size_t)i), field_load(wd, (size_t)i), field_load(eff, (size_t)i),
                                              current_epoch, total_penalties, floor_one(total_balance),
                                              latest_slashed_exit_length, min_slashing_penalty_quotient);
    balances[i] = balances[i] > penalty ? balances[i] - penalty : 0;
  }
  return 0;
}

// bls381_effective_balances over host arrays
int hc_effective_balances(uint64_t n, const uint64_t* balances, const uint8_t* effective_balance, size_t stride,
                          uint64_t increment, uint64_t max_effective_balance, uint32_t* indices, uint64_t* values,
                          uint64_t* changed_out) {
  using namespace bls381;
  *changed_out = 0;
  if (stride < 8 || increment == 0) return -1;
  const u64_field eff = make_u64_field(effective_balance, stride);
  for (uint64_t i = 0; i < n; ++i) {
    const bool moved = effective_balance_update(balances[i], field_load(eff, (size_t)i), increment, max_effective_balance,
                                                &values[i]);
    indices[i] = moved ? (uint32_t)i : VOTES_NONE;
    *changed_out += moved;
  }
  return 0;
}

}  // extern "C"
