// Epoch rewards on gfx950: votes, deltas, slashings and the effective-balance hysteresis
// (DESIGN.md §7g): the whole-registry work of process_epoch, computed where the records are.
//
// Reference: specs/core/0_beacon-chain.md:1294-1321 (get_unslashed_attesting_indices,
// get_attesting_balance, get_winning_crosslink_and_attesting_indices), :1389-1475
// (get_base_reward, get_attestation_deltas, get_crosslink_deltas,
// process_rewards_and_penalties), :1505-1524 (process_slashings) and :1535-1540 (the hysteresis
// of process_final_updates).
//
// Validator fields are read through u64_field (bls381_epoch.hpp); the `slashed` flag is one byte
// at base + i * stride (u8_field): stride 121 with base = records + 112 over the serialized
// Validator records, stride 1 over a plain array.  Any non-zero byte counts as slashed.
//
// Votes (votes_walk, one workgroup per committee): a validator sits in exactly one committee of
// an epoch -- the committees are disjoint slices of one shuffled list, which is a permutation --
// so what a committee's workgroup writes about its members no other workgroup writes: no atomics,
// no de-duplication.  The union of the attesters of a group of a committee's attestations is the
// bitwise OR of their bitfields, and position j of the OR is validator shuffled[off + j].  The
// group bitmaps (source, target, head, then one candidate at a time; at most 4,096 bits = 512
// bytes each) are built in LDS, each lane ORs whole words of its own, and the members are walked
// against them.  The sums (the committee's balance, its three attesting balances, each
// candidate's balance) are workgroup reductions of 64-bit integers: their order does not matter.
//
// Deltas, slashings, hysteresis: one lane per validator over the per-item functions below, which
// the kernels and the g++ host build share.
//
// Arithmetic: the spec's integers are unbounded.  Every product that can pass 2^64 goes through
// mul_div_u64 (a 128-bit product); a quotient of 2^64 or more, a per-validator sum that wraps and
// an increase_balance that wraps saturate at 2^64 - 1 and count as overflows; a proposer addend
// of 2^32 or more is not added and counts; so do a proposer index at or above n, an inclusion
// delay of 0 and a committee index at or above n_committees, which add nothing.
#pragma once
#include "bls381_epoch.hpp"

namespace bls381 {

typedef unsigned __int128 u128_t;

constexpr uint32_t VOTE_SOURCE = 1u, VOTE_TARGET = 2u, VOTE_HEAD = 4u, VOTE_WINNER = 8u, VOTE_MEMBER = 16u;
constexpr uint32_t VOTES_NONE = 0xFFFFFFFFu;
constexpr uint32_t VOTES_MASK_WORDS = ATT_MASK_WORDS;   // 4,096 members: 128 words
constexpr uint32_t ATT_FLAG_TARGET = 1u, ATT_FLAG_HEAD = 2u;
constexpr uint32_t DELTAS_ATTESTATION = 1u, DELTAS_CROSSLINK = 2u;
constexpr uint64_t PROPOSER_ADDEND_LIMIT = (uint64_t)1 << 32;

// ---- the slashed flag -------------------------------------------------------------------------
struct u8_field {
  const uint8_t* base;
  size_t stride;
};
inline u8_field make_u8_field(const void* base, size_t stride) { return u8_field{(const uint8_t*)base, stride}; }
BLS_DEV_INLINE bool flag_load(const u8_field& f, size_t i) { return f.base[i * f.stride] != 0; }
inline size_t flag_span(size_t n, size_t stride) { return n ? (n - 1) * stride + 1 : 0; }

// ---- arithmetic -------------------------------------------------------------------------------
// floor(a * b / d) for d != 0 over the 128-bit product; a quotient of 2^64 or more counts in *ovf
// and gives 2^64 - 1
BLS_DEV_INLINE uint64_t mul_div_u64(uint64_t a, uint64_t b, uint64_t d, uint32_t* ovf) {
  const u128_t p = (u128_t)a * b;
  if ((uint64_t)(p >> 64) == 0) return (uint64_t)p / d;
  const u128_t q = p / d;
  if ((uint64_t)(q >> 64) != 0) {
    ++*ovf;
    return ~(uint64_t)0;
  }
  return (uint64_t)q;
}
// a + b, saturating; a wrap counts in *ovf
BLS_DEV_INLINE uint64_t sat_add_u64(uint64_t a, uint64_t b, uint32_t* ovf) {
  const uint64_t s = a + b;
  if (s < a) {
    ++*ovf;
    return ~(uint64_t)0;
  }
  return s;
}
// integer_squareroot (:1055-1066): the largest r with r * r <= n, bit by bit (r < 2^32, so t * t
// below fits), exact for every uint64
BLS_DEV_INLINE uint64_t isqrt_u64(uint64_t n) {
  uint64_t r = 0;
  for (int b = 31; b >= 0; --b) {
    const uint64_t t = r | ((uint64_t)1 << b);
    if (t * t <= n) r = t;
  }
  return r;
}
BLS_INLINE uint64_t floor_one(uint64_t x) { return x ? x : 1; }   // get_total_balance's max(1, .)

// ---- votes ------------------------------------------------------------------------------------
// one committee: its slice of the shuffled list, its attestations (CSR), its candidate count
struct votes_committee {
  uint32_t off, len, att_first, att_count, cand_count;
};
// one attestation: the byte offset of its bitfield, flags (ATT_FLAG_*), proposer and candidate
struct votes_att {
  uint64_t delay;
  uint32_t bits_off, flags, proposer, cand;
};
// a workgroup's LDS (the host build: a heap block)
struct votes_lds {
  uint32_t src[VOTES_MASK_WORDS], tgt[VOTES_MASK_WORDS], head[VOTES_MASK_WORDS], cand[VOTES_MASK_WORDS];
  uint64_t eff[ATT_MAX_COMMITTEE];   // member j's effective balance, 0 when slashed or out of range
  uint64_t red[EPOCH_BLOCK];
};

// bits [32 w, 32 w + 32) of a bitfield of nbytes bytes; bytes past its end read as zero
template <class B>
BLS_DEV_INLINE uint32_t votes_bits_word(B bits, uint32_t nbytes, uint32_t w) {
  uint32_t m = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = 4 * w + k;
    if (i < nbytes) m |= (uint32_t)bits[i] << (8 * k);
  }
  return m;
}
template <class B>
BLS_DEV_INLINE bool votes_bit(B bits, uint32_t j) { return (bits[j >> 3] >> (j & 7u)) & 1u; }

// the sum of x over the nt lanes (a power of two; the host build: 1)
template <class Sync>
BLS_DEV_INLINE uint64_t votes_reduce(uint64_t* red, uint32_t tid, uint32_t nt, Sync sync, uint64_t x) {
  red[tid] = x;
  for (uint32_t s = nt >> 1; s > 0; s >>= 1) {
    sync();
    if (tid < s) red[tid] += red[tid + s];
  }
  sync();
  const uint64_t r = red[0];
  sync();   // red is free for the next sum
  return r;
}

// Committee c by the nt lanes of a workgroup (lane tid; sync() is the workgroup barrier; the host
// build runs it with nt = 1 and an empty sync).  Writes votes / incl_delay / incl_proposer /
// committee_of of the members below n_validators, winner[c], winner_balance[c],
// committee_balance[c] and partial[3 c .. 3 c + 2] (the committee's share of the three attesting
// balances).  A member at or above n_validators is passed over.
template <class Sync, class S, class A, class B>
BLS_DEV_INLINE void votes_walk(votes_lds* L, uint32_t tid, uint32_t nt, Sync sync, uint32_t c, const votes_committee& cm,
                               S shuffled, A atts, B bits, const u8_field& slashed, const u64_field& effective,
                               uint64_t n_validators, uint32_t* votes, uint64_t* incl_delay, uint32_t* incl_proposer,
                               uint32_t* committee_of, uint32_t* winner, uint64_t* winner_balance,
                               uint64_t* committee_balance, uint64_t* partial) {
  const uint32_t nbytes = (cm.len + 7) / 8, nwords = (cm.len + 31) / 32;
  for (uint32_t w = tid; w < nwords; w += nt) {
    uint32_t s = 0, t = 0, h = 0;
    for (uint32_t a = 0; a < cm.att_count; ++a) {
      const votes_att at = atts[cm.att_first + a];
      const uint32_t m = votes_bits_word(bits + at.bits_off, nbytes, w);
      s |= m;
      if (at.flags & ATT_FLAG_TARGET) t |= m;
      if (at.flags & ATT_FLAG_HEAD) h |= m;
    }
    L->src[w] = s;
    L->tgt[w] = t;
    L->head[w] = h;
  }
  sync();
  uint64_t sum_committee = 0, sum_s = 0, sum_t = 0, sum_h = 0;
  for (uint32_t j = tid; j < cm.len; j += nt) {
    const uint32_t v = shuffled[cm.off + j];
    uint64_t e = 0;
    if (v < n_validators) {
      const uint64_t full = field_load(effective, v);
      uint32_t vt = VOTE_MEMBER;
      sum_committee += full;
      if (!flag_load(slashed, v)) {
        e = full;
        const uint32_t w = j >> 5, b = j & 31u;
        if ((L->src[w] >> b) & 1u) { vt |= VOTE_SOURCE; sum_s += full; }
        if ((L->tgt[w] >> b) & 1u) { vt |= VOTE_TARGET; sum_t += full; }
        if ((L->head[w] >> b) & 1u) { vt |= VOTE_HEAD; sum_h += full; }
      }
      votes[v] = vt;
      committee_of[v] = c;
      if (vt & VOTE_SOURCE) {
        // min(..., key=inclusion_delay): the smallest delay, the first in list order among equals
        bool found = false;
        uint64_t delay = 0;
        uint32_t proposer = 0;
        for (uint32_t a = 0; a < cm.att_count; ++a) {
          const votes_att at = atts[cm.att_first + a];
          if (votes_bit(bits + at.bits_off, j) && (!found || at.delay < delay)) {
            found = true;
            delay = at.delay;
            proposer = at.proposer;
          }
        }
        incl_delay[v] = delay;
        incl_proposer[v] = proposer;
      }
    }
    L->eff[j] = e;
  }
  const uint64_t cb = votes_reduce(L->red, tid, nt, sync, sum_committee);
  const uint64_t ps = votes_reduce(L->red, tid, nt, sync, sum_s);
  const uint64_t pt = votes_reduce(L->red, tid, nt, sync, sum_t);
  const uint64_t ph = votes_reduce(L->red, tid, nt, sync, sum_h);
  // the winner: the largest balance, then the largest candidate id
  uint32_t best = VOTES_NONE;
  uint64_t best_balance = 0;
  const uint32_t passes = cm.cand_count > 1 ? cm.cand_count + 1 : cm.cand_count;
  for (uint32_t p = 0; p < passes; ++p) {
    const uint32_t k = p < cm.cand_count ? p : best;   // the last pass rebuilds the winner's bitmap
    for (uint32_t w = tid; w < nwords; w += nt) {
      uint32_t m = 0;
      for (uint32_t a = 0; a < cm.att_count; ++a) {
        const votes_att at = atts[cm.att_first + a];
        if (at.cand == k) m |= votes_bits_word(bits + at.bits_off, nbytes, w);
      }
      L->cand[w] = m;
    }
    sync();
    if (p < cm.cand_count) {
      uint64_t x = 0;
      for (uint32_t j = tid; j < cm.len; j += nt)
        if ((L->cand[j >> 5] >> (j & 31u)) & 1u) x += L->eff[j];
      const uint64_t balance = votes_reduce(L->red, tid, nt, sync, x);   // its barriers also free L->cand
      if (best == VOTES_NONE || balance >= best_balance) {
        best = k;
        best_balance = balance;
      }
    }
  }
  if (best != VOTES_NONE)
    for (uint32_t j = tid; j < cm.len; j += nt)
      if ((L->cand[j >> 5] >> (j & 31u)) & 1u) {
        const uint32_t v = shuffled[cm.off + j];
        if (v < n_validators && !flag_load(slashed, v)) votes[v] |= VOTE_WINNER;   // this lane wrote votes[v] above
      }
  if (tid == 0) {
    winner[c] = best;
    winner_balance[c] = best_balance;
    committee_balance[c] = cb;
    partial[3 * (size_t)c] = ps;
    partial[3 * (size_t)c + 1] = pt;
    partial[3 * (size_t)c + 2] = ph;
  }
}

// ---- deltas -----------------------------------------------------------------------------------
struct reward_constants {
  uint64_t base_reward_factor, base_rewards_per_epoch, proposer_reward_quotient, min_attestation_inclusion_delay,
      min_epochs_to_inactivity_penalty, inactivity_penalty_quotient;
};
// what one call reads: the record fields, the outputs of the votes call and the scalars
struct deltas_in {
  u64_field activation, exit_, withdrawable, effective;
  u8_field slashed;
  const uint32_t* votes;
  const uint64_t* incl_delay;
  const uint32_t* incl_proposer;
  const uint32_t* committee_of;
  const uint64_t *winner_balance, *committee_balance, *totals;
  uint64_t n, n_committees, previous_epoch, finalized_epoch;
  reward_constants k;
  uint32_t which;
};
// validator i's own rewards and penalties, and the micro-reward it sends to a proposer
// (proposer == VOTES_NONE: none)
struct validator_delta {
  uint64_t reward, penalty, proposer_addend;
  uint32_t proposer, overflows;
};
// total_balance: get_total_active_balance, floored at 1; sqrt_total = isqrt_u64(total_balance)
BLS_DEV_INLINE validator_delta validator_deltas(const deltas_in& in, uint64_t total_balance, uint64_t sqrt_total, size_t i) {
  validator_delta d{0, 0, 0, VOTES_NONE, 0};
  const reward_constants& k = in.k;
  const uint64_t eff = field_load(in.effective, i);
  const bool slashed = flag_load(in.slashed, i);
  const uint32_t vt = in.votes[i];
  // get_base_reward
  const uint64_t base = mul_div_u64(eff, k.base_reward_factor, sqrt_total, &d.overflows) / k.base_rewards_per_epoch;
  if (in.which & DELTAS_ATTESTATION) {
    const bool eligible = validator_active(in.activation, in.exit_, in.previous_epoch, i) ||
                          (slashed && in.previous_epoch + 1 < field_load(in.withdrawable, i));
    if (eligible)
      for (uint32_t g = 0; g < 3; ++g) {
        if (vt & (1u << g))
          d.reward = sat_add_u64(d.reward, mul_div_u64(base, floor_one(in.totals[g]), total_balance, &d.overflows), &d.overflows);
        else
          d.penalty = sat_add_u64(d.penalty, base, &d.overflows);
      }
    // proposer and inclusion delay micro-rewards: every unslashed source attester, eligible or not
    if (vt & VOTE_SOURCE) {
      const uint64_t addend = base / k.proposer_reward_quotient;
      const uint32_t proposer = in.incl_proposer[i];
      if (proposer >= in.n || addend >= PROPOSER_ADDEND_LIMIT) {
        ++d.overflows;
      } else {
        d.proposer = proposer;
        d.proposer_addend = addend;
      }
      const uint64_t delay = in.incl_delay[i];
      if (delay == 0)
        ++d.overflows;
      else
        d.reward = sat_add_u64(d.reward, mul_div_u64(base, k.min_attestation_inclusion_delay, delay, &d.overflows), &d.overflows);
    }
    const uint64_t finality_delay = in.previous_epoch - in.finalized_epoch;
    if (eligible && finality_delay > k.min_epochs_to_inactivity_penalty) {
      d.penalty = sat_add_u64(d.penalty, mul_div_u64(k.base_rewards_per_epoch, base, 1, &d.overflows), &d.overflows);
      if (!(vt & VOTE_TARGET))
        d.penalty = sat_add_u64(d.penalty, mul_div_u64(eff, finality_delay, k.inactivity_penalty_quotient, &d.overflows), &d.overflows);
    }
  }
  if (in.which & DELTAS_CROSSLINK) {
    const uint32_t c = in.committee_of[i];
    if (c != VOTES_NONE) {
      if (c >= in.n_committees) {
        ++d.overflows;
      } else if (vt & VOTE_WINNER) {
        d.reward = sat_add_u64(d.reward,
                               mul_div_u64(base, floor_one(in.winner_balance[c]), floor_one(in.committee_balance[c]), &d.overflows),
                               &d.overflows);
      } else {
        d.penalty = sat_add_u64(d.penalty, base, &d.overflows);
      }
    }
  }
  return d;
}
// rewards[i] with what the proposers' scatter brought, then increase_balance and decrease_balance
BLS_DEV_INLINE uint64_t apply_deltas(uint64_t balance, uint64_t own_reward, uint64_t proposer_reward, uint64_t penalty,
                                     uint64_t* reward_out, uint32_t* ovf) {
  const uint64_t reward = sat_add_u64(own_reward, proposer_reward, ovf);
  *reward_out = reward;
  const uint64_t up = sat_add_u64(balance, reward, ovf);
  return up > penalty ? up - penalty : 0;
}

// ---- slashings --------------------------------------------------------------------------------
// process_slashings for one validator: the penalty, 0 when the validator is not due
BLS_DEV_INLINE uint64_t slashing_penalty(bool slashed, uint64_t withdrawable_epoch, uint64_t effective_balance,
                                         uint64_t current_epoch, uint64_t total_penalties, uint64_t total_balance,
                                         uint64_t latest_slashed_exit_length, uint64_t min_slashing_penalty_quotient) {
  const uint64_t half = latest_slashed_exit_length / 2;
  if (!slashed || withdrawable_epoch < half || current_epoch != withdrawable_epoch - half) return 0;
  const u128_t tripled = (u128_t)total_penalties * 3;
  const uint64_t m = tripled < total_balance ? (uint64_t)tripled : total_balance;
  uint32_t none = 0;   // m <= total_balance: the quotient is at most effective_balance
  const uint64_t a = mul_div_u64(effective_balance, m, total_balance, &none);
  const uint64_t b = effective_balance / min_slashing_penalty_quotient;
  return a > b ? a : b;
}

// ---- hysteresis -------------------------------------------------------------------------------
// the new effective balance of one validator; true when it differs from the old one
BLS_DEV_INLINE bool effective_balance_update(uint64_t balance, uint64_t effective_balance, uint64_t increment,
                                             uint64_t max_effective_balance, uint64_t* value) {
  const u128_t upper = (u128_t)effective_balance + (u128_t)3 * (increment / 2);
  *value = effective_balance;
  if (balance < effective_balance || upper < balance) {
    const uint64_t floored = balance - balance % increment;
    *value = floored < max_effective_balance ? floored : max_effective_balance;
  }
  return *value != effective_balance;
}

}  // namespace bls381
