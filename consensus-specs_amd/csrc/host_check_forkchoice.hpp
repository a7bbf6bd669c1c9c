// Host exports over bls381_forkchoice.hpp: the fork-choice store with its latest messages in host
// memory, and the head by the kernels' own steps (direct weights in two words, the preorder prefix
// sum, the counts, the best child in three passes, the pointer doubling) over host arrays.
// Included once by host_check.cpp (lib/libbls381_hostcheck.so) and once by
// forkchoice_check_main.cpp (the stand-alone sanitizer program).
#pragma once
#include <cstdint>
#include <vector>

#include "bls381_forkchoice.hpp"

namespace hc_forkchoice {
using namespace bls381;

struct Store {
  uint64_t validator_capacity, block_capacity, seq = 0;
  fc_tree tree;
  std::vector<uint64_t> key;      // per validator: 0 = never attested
  std::vector<uint32_t> target;   // FC_NONE: no message (or its block was pruned)
};

// k_fc_att_max, then k_fc_att_write: the order of the entries within a pass does not matter
inline uint64_t apply_batch(Store& s, const std::vector<fc_att>& att, const uint32_t* entries, const uint8_t* ok) {
  uint64_t skipped = 0;
  for (int pass = 0; pass < 2; ++pass)
    for (size_t a = 0; a < att.size(); ++a) {
      if (ok && !ok[a]) continue;
      for (uint32_t j = att[a].first; j < att[a].end; ++j) {
        const uint32_t v = entries[j];
        if (v >= s.validator_capacity) {
          skipped += pass == 0;
          continue;
        }
        if (pass == 0) s.key[v] = std::max(s.key[v], att[a].key);
        else if (s.key[v] == att[a].key) s.target[v] = att[a].target;
      }
    }
  return skipped;
}

// the head and the counts; false for arguments the call rejects
inline bool head(const Store& s, uint32_t start, uint64_t n, const u64_field& act, const u64_field& ext,
                 const u64_field& eff, uint64_t epoch, uint32_t* head_out, uint64_t* weights_out, uint64_t* status_out) {
  const size_t B = s.tree.size();
  if (start >= B || n > s.validator_capacity) return false;
  std::vector<uint32_t> pre, sub, node_at, rank;
  s.tree.number(&pre, &sub, &node_at, &rank);
  // k_fc_direct
  std::vector<fc_sum> direct(B, fc_sum{0, 0});
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t t = s.target[i];
    if (t == FC_NONE) continue;   // the fields of a validator without a message are not read
    if (fc_votes(field_load(act, (size_t)i), field_load(ext, (size_t)i), epoch, t))
      direct[t] = fc_sum_add(direct[t], fc_sum_of(field_load(eff, (size_t)i)));
  }
  // k_fc_scan: exclusive prefix sums in preorder
  std::vector<fc_sum> prefix(B + 1, fc_sum{0, 0});
  for (size_t p = 0; p < B; ++p) prefix[p + 1] = fc_sum_add(prefix[p], direct[node_at[p]]);
  // k_fc_count, k_fc_best_rank, k_fc_best_child
  std::vector<uint64_t> count(B), best_count(B, 0);
  std::vector<uint32_t> best_rank(B, 0), jump(B), next(B);
  uint64_t overflows = 0;
  for (size_t b = 0; b < B; ++b) {
    bool ovf;
    count[b] = fc_sum_value(fc_sum_sub(prefix[pre[b] + sub[b]], prefix[pre[b]]), &ovf);
    overflows += ovf;
    jump[b] = (uint32_t)b;
    if (b) best_count[s.tree.parent[b]] = std::max(best_count[s.tree.parent[b]], count[b]);
  }
  for (size_t b = 1; b < B; ++b) {
    const uint32_t p = s.tree.parent[b];
    if (count[b] == best_count[p]) best_rank[p] = std::max(best_rank[p], rank[b]);
  }
  for (size_t b = 1; b < B; ++b) {
    const uint32_t p = s.tree.parent[b];
    if (count[b] == best_count[p] && rank[b] == best_rank[p]) jump[p] = (uint32_t)b;
  }
  // k_fc_jump
  for (uint32_t r = 0, rounds = fc_rounds((uint32_t)s.block_capacity); r < rounds; ++r) {
    for (size_t b = 0; b < B; ++b) next[b] = jump[jump[b]];
    jump.swap(next);
  }
  *head_out = jump[start];
  if (weights_out)
    for (size_t b = 0; b < B; ++b) weights_out[b] = count[b];
  status_out[FCS_OVERFLOWS] = overflows;
  return true;
}
}  // namespace hc_forkchoice

extern "C" {

// The calls of include/bls381.h's fork choice over host memory; 0, or -1 for arguments the call
// rejects (which then writes nothing).
void* hc_fork_choice_create(uint64_t validator_capacity, uint64_t block_capacity) {
  using namespace bls381;
  if (validator_capacity == 0 || validator_capacity > 0xFFFFFFFFull || block_capacity == 0 || block_capacity > FC_BLOCK_LIMIT)
    return nullptr;
  hc_forkchoice::Store* s = new hc_forkchoice::Store();
  s->validator_capacity = validator_capacity;
  s->block_capacity = block_capacity;
  s->key.assign((size_t)validator_capacity, 0);
  s->target.assign((size_t)validator_capacity, FC_NONE);
  return s;
}
void hc_fork_choice_destroy(void* fc) { delete (hc_forkchoice::Store*)fc; }
uint64_t hc_fork_choice_block_count(const void* fc) { return fc ? ((const hc_forkchoice::Store*)fc)->tree.size() : 0; }

int hc_fork_choice_add_blocks(void* fc, uint64_t n, const uint8_t* roots32, const uint8_t* parent_roots32,
                              const uint64_t* slots, uint32_t* node_out) {
  hc_forkchoice::Store* s = (hc_forkchoice::Store*)fc;
  if (!s || (n && (!roots32 || !parent_roots32 || !slots))) return -1;
  std::vector<uint32_t> ids((size_t)n);
  if (!s->tree.add((size_t)n, roots32, parent_roots32, slots, (size_t)s->block_capacity, ids.data())) return -1;
  if (node_out)
    for (size_t k = 0; k < n; ++k) node_out[k] = ids[k];
  return 0;
}
uint32_t hc_fork_choice_node(const void* fc, const uint8_t* root32) {
  return fc && root32 ? ((const hc_forkchoice::Store*)fc)->tree.find(root32) : bls381::FC_NONE;
}

int hc_fork_choice_on_attestations(void* fc, uint64_t n_att, const uint32_t* att_off, const uint32_t* entries,
                                   const uint64_t* slots, const uint32_t* target_nodes, const uint8_t* ok,
                                   uint64_t* skipped_out) {
  using namespace bls381;
  hc_forkchoice::Store* s = (hc_forkchoice::Store*)fc;
  if (!s || !skipped_out || (n_att && (!att_off || !slots || !target_nodes))) return -1;
  std::vector<fc_att> att;
  if (n_att && !fc_plan_batch((size_t)n_att, att_off, slots, target_nodes, s->tree.size(), s->seq, &att)) return -1;
  if (n_att && att_off[n_att] != att_off[0] && !entries) return -1;
  *skipped_out = hc_forkchoice::apply_batch(*s, att, entries, ok);
  s->seq += n_att;
  return 0;
}

int hc_fork_choice_read_latest(const void* fc, uint64_t first, uint64_t n, uint64_t* slots_out, uint32_t* targets_out) {
  const hc_forkchoice::Store* s = (const hc_forkchoice::Store*)fc;
  if (!s || first > s->validator_capacity || n > s->validator_capacity - first || (n && (!slots_out || !targets_out)))
    return -1;
  for (uint64_t k = 0; k < n; ++k) {
    slots_out[k] = bls381::fc_key_slot(s->key[(size_t)(first + k)]);
    targets_out[k] = s->target[(size_t)(first + k)];
  }
  return 0;
}

int hc_fork_choice_prune(void* fc, uint32_t new_anchor_node) {
  using namespace bls381;
  hc_forkchoice::Store* s = (hc_forkchoice::Store*)fc;
  if (!s || new_anchor_node >= s->tree.size()) return -1;
  std::vector<uint32_t> map;
  s->tree.prune(new_anchor_node, &map);
  for (uint32_t& t : s->target)   // k_fc_remap
    if (t != FC_NONE) t = map[t];
  return 0;
}

int hc_fork_choice_head(const void* fc, uint32_t start_node, uint64_t n, const uint8_t* activation_epoch,
                        const uint8_t* exit_epoch, const uint8_t* effective_balance, size_t stride, uint64_t epoch,
                        uint32_t* head_out, uint8_t* head_root32, uint64_t* weights_out, uint64_t* status_out) {
  using namespace bls381;
  const hc_forkchoice::Store* s = (const hc_forkchoice::Store*)fc;
  if (!s || stride < 8 || !head_out || !status_out || (n && (!activation_epoch || !exit_epoch || !effective_balance)))
    return -1;
  uint32_t h = FC_NONE;
  uint64_t status[FCS_WORDS];
  if (!hc_forkchoice::head(*s, start_node, n, make_u64_field(activation_epoch, stride), make_u64_field(exit_epoch, stride),
                           make_u64_field(effective_balance, stride), epoch, &h, weights_out, status))
    return -1;
  *head_out = h;
  if (head_root32) std::memcpy(head_root32, s->tree.root[h].data(), 32);
  for (uint32_t x = 0; x < FCS_WORDS; ++x) status_out[x] = status[x];
  return 0;
}

}  // extern "C"
