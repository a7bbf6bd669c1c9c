// Fork choice on gfx950: latest messages and the LMD-GHOST head: lmd_ghost computed
// where the validator records and the attesting indices already are.
//
// Reference: specs/core/0_fork-choice.md:78-103 (lmd_ghost with get_vote_count), :56-69
// (get_ancestor) and :71-72 (the latest attestation: the highest slot, and among equal slots the
// one observed first).
//
// The block tree is the host's: thousands of nodes, appended in an order that puts every parent
// before its children (parent[id] < id).  The per-validator state is the device's: one latest
// message per validator, a 64-bit key and a 32-bit target node.
//
// The key.  (slot << 32) | (0xFFFFFFFF - seq), seq the attestation's number over the life of the
// store in the order it was handed in.  The larger key wins: the higher slot, and among equal slots
// the smaller seq, which is the one observed first.  Keys are unique per attestation, so "my key is
// the validator's key" names one attestation whatever the order lanes ran in: the first launch
// takes the maximum per validator, the second writes the target where the key is the writer's own.
//
// The vote counts.  get_vote_count(block) sums the balances of the votes whose target has `block`
// as its ancestor at block.slot; slots rise strictly from parent to child, so that is "the target
// is the block or one of its descendants".  In a preorder numbering the descendants of a node are
// the contiguous range [pre, pre + size), so with the direct weights (the balance that names a
// node itself) laid out in preorder, every count is a difference of two entries of one prefix
// sum: one scan instead of the walk per validator and level.
//
// Sums are kept as two 64-bit words, the sum of the balances' low halves and of their high
// halves: with at most 2^32 - 1 validators neither wraps, a prefix sum of them neither, and the
// count lo + (hi << 32) is exact or known to pass 2^64 - 1.  By §7g's rule such a count becomes
// 2^64 - 1 and its node adds 1 to the call's status word.
//
// The descent.  The best child of a node is its child with the largest (count, rank of root); the
// host ranks the roots (byte-string order) whenever the tree changes, so no 32-byte string is
// compared on the device.  jump[b] = best child, or b itself at a leaf; squaring that map
// ceil(log2(block_capacity)) times reaches every node's leaf, the head being jump[start].
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <map>
#include <vector>

#include "bls381_epoch.hpp"

namespace bls381 {

constexpr uint32_t FC_NONE = 0xFFFFFFFFu;
constexpr uint32_t FC_BINS = 2048;              // nodes a workgroup sums in LDS: 2 x 8 bytes each, 32 KiB
constexpr uint32_t FC_SCAN_TILE = EPOCH_BLOCK;  // nodes the scan's one workgroup takes a round
constexpr uint64_t FC_SLOT_LIMIT = (uint64_t)1 << 32;
constexpr uint64_t FC_SEQ_LIMIT = 0xFFFFFFFFull;   // seq stays below: a key is never 0
constexpr uint32_t FC_BLOCK_LIMIT = 1u << 24;      // block_capacity at most
// the status words of a head call
enum : uint32_t { FCS_OVERFLOWS = 0, FCS_WORDS = 1 };

BLS_INLINE uint64_t fc_key(uint64_t slot, uint64_t seq) { return (slot << 32) | (0xFFFFFFFFull - seq); }
BLS_INLINE uint64_t fc_key_slot(uint64_t key) { return key >> 32; }

// one attestation of a batch as the kernels read it
struct fc_att {
  uint32_t first, end;   // its members: entries[first .. end)
  uint32_t target;       // a node of the tree
  uint32_t pad;
  uint64_t key;
};
// the attestation of entry j (att[0].first <= j < att[n_att - 1].end): the last a with
// att[a].first <= j.  The offsets do not descend, so that one's range holds j, and attestations
// without members are passed over.  ceil(log2(n_att)) steps, whatever the data.
template <class A> BLS_DEV_INLINE uint32_t fc_att_of(A att, uint32_t n_att, uint32_t j) {
  uint32_t lo = 0, hi = n_att;   // first(lo) <= j < first(hi), first(n_att) = the last end
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (att[mid].first <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// The host half of a batch: att[a] for attestation a, numbered seq, seq + 1, ...  False for
// arguments the call rejects: descending offsets, a slot at 2^32 or above, a target node that is
// not in the tree, more than 2^32 - 1 attestations over the life of the store.
inline bool fc_plan_batch(size_t n_att, const uint32_t* att_off, const uint64_t* slots, const uint32_t* target_nodes,
                          size_t n_blocks, uint64_t seq, std::vector<fc_att>* att) {
  if (n_att > FC_SEQ_LIMIT || seq + n_att > FC_SEQ_LIMIT) return false;
  att->resize(n_att);
  for (size_t a = 0; a < n_att; ++a) {
    if (att_off[a + 1] < att_off[a] || slots[a] >= FC_SLOT_LIMIT || target_nodes[a] >= n_blocks) return false;
    (*att)[a] = fc_att{att_off[a], att_off[a + 1], target_nodes[a], 0, fc_key(slots[a], seq + a)};
  }
  return true;
}

// does validator i vote: active at `epoch` with a message
BLS_INLINE bool fc_votes(uint64_t activation, uint64_t exit_, uint64_t epoch, uint32_t target) {
  return target != FC_NONE && activation <= epoch && epoch < exit_;
}

// ---- sums in two words ------------------------------------------------------------------------
struct fc_sum {
  uint64_t lo, hi;   // sums of the addends' low and high 32 bits
};
BLS_INLINE fc_sum fc_sum_of(uint64_t balance) { return fc_sum{balance & 0xFFFFFFFFull, balance >> 32}; }
BLS_INLINE fc_sum fc_sum_add(const fc_sum& a, const fc_sum& b) { return fc_sum{a.lo + b.lo, a.hi + b.hi}; }
BLS_INLINE fc_sum fc_sum_sub(const fc_sum& a, const fc_sum& b) { return fc_sum{a.lo - b.lo, a.hi - b.hi}; }
// lo + (hi << 32), or 2^64 - 1 and *overflow = true where that passes 2^64 - 1
BLS_INLINE uint64_t fc_sum_value(const fc_sum& s, bool* overflow) {
  const uint64_t top = s.hi + (s.lo >> 32);   // below 2^33 for at most 2^32 addends
  *overflow = top > 0xFFFFFFFFull;
  return *overflow ? ~(uint64_t)0 : (top << 32) | (s.lo & 0xFFFFFFFFull);
}

// (count, rank) of a beats (count, rank) of b; ranks are distinct
BLS_INLINE bool fc_better(uint64_t count_a, uint32_t rank_a, uint64_t count_b, uint32_t rank_b) {
  return count_a > count_b || (count_a == count_b && rank_a > rank_b);
}
// rounds of pointer doubling that cover a chain of `capacity` nodes
inline uint32_t fc_rounds(uint32_t capacity) {
  uint32_t r = 0;
  while (((uint64_t)1 << r) < capacity) ++r;
  return r ? r : 1;
}
inline size_t fc_node_tiles(size_t n_blocks) { return (n_blocks + FC_BINS - 1) / FC_BINS; }

// ---- the block tree (host) --------------------------------------------------------------------
struct fc_tree {
  typedef std::array<uint8_t, 32> root_t;
  std::vector<root_t> root;
  std::vector<uint32_t> parent;   // FC_NONE for the anchor
  std::vector<uint64_t> slot;
  std::map<root_t, uint32_t> ids;

  size_t size() const { return root.size(); }
  static root_t make_root(const uint8_t* p) {
    root_t r;
    std::memcpy(r.data(), p, 32);
    return r;
  }
  uint32_t find(const uint8_t* root32) const {
    const auto it = ids.find(make_root(root32));
    return it == ids.end() ? FC_NONE : it->second;
  }
  // Appends n blocks (a known root returns its id; the first block ever is the anchor and its
  // parent root is not looked at).  False, and nothing changes, when a parent is unknown, a slot
  // is not above its parent's or at 2^32 or more, or the tree would pass `capacity`.
  bool add(size_t n, const uint8_t* roots32, const uint8_t* parent_roots32, const uint64_t* slots, size_t capacity,
           uint32_t* node_out) {
    const size_t before = size();
    bool ok = true;
    for (size_t k = 0; k < n && ok; ++k) {
      const root_t r = make_root(roots32 + 32 * k);
      const auto known = ids.find(r);
      if (known != ids.end()) {
        if (node_out) node_out[k] = known->second;
        continue;
      }
      uint32_t p = FC_NONE;
      if (size() != 0) {
        p = find(parent_roots32 + 32 * k);
        ok = p != FC_NONE && slots[k] > slot[p];
      }
      ok = ok && slots[k] < FC_SLOT_LIMIT && size() < capacity;
      if (!ok) break;
      const uint32_t id = (uint32_t)size();
      root.push_back(r);
      parent.push_back(p);
      slot.push_back(slots[k]);
      ids[r] = id;
      if (node_out) node_out[k] = id;
    }
    if (!ok) truncate(before);
    return ok;
  }
  void truncate(size_t count) {
    while (size() > count) {
      ids.erase(root.back());
      root.pop_back();
      parent.pop_back();
      slot.pop_back();
    }
  }
  // The numbering the device works in, O(blocks) without recursion (parent[id] < id): pre[id] the
  // preorder position with children in id order, sub[id] the subtree size, node_at the inverse of
  // pre, rank[id] the place of the root in byte-string order.
  void number(std::vector<uint32_t>* pre, std::vector<uint32_t>* sub, std::vector<uint32_t>* node_at,
              std::vector<uint32_t>* rank) const {
    const size_t B = size();
    pre->assign(B, 0);
    sub->assign(B, 1);
    node_at->assign(B, 0);
    rank->assign(B, 0);
    for (size_t i = B; i-- > 1;) (*sub)[parent[i]] += (*sub)[i];
    std::vector<uint32_t> next(B, 1);   // the position the node's next child takes
    for (size_t i = 1; i < B; ++i) {
      const uint32_t p = parent[i];
      (*pre)[i] = next[p];
      next[p] += (*sub)[i];
      next[i] = (*pre)[i] + 1;
    }
    for (size_t i = 0; i < B; ++i) (*node_at)[(*pre)[i]] = (uint32_t)i;
    std::vector<uint32_t> order(B);
    for (size_t i = 0; i < B; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return root[a] < root[b]; });
    for (size_t k = 0; k < B; ++k) (*rank)[order[k]] = (uint32_t)k;
  }
  // Keeps the subtree of `anchor`, renumbered in insertion order; map[old id] = new id or FC_NONE.
  void prune(uint32_t anchor, std::vector<uint32_t>* map) {
    const size_t B = size();
    map->assign(B, FC_NONE);
    fc_tree kept;
    for (size_t i = anchor; i < B; ++i) {
      const bool in = i == anchor || (parent[i] != FC_NONE && parent[i] >= anchor && (*map)[parent[i]] != FC_NONE);
      if (!in) continue;
      const uint32_t id = (uint32_t)kept.size();
      (*map)[i] = id;
      kept.root.push_back(root[i]);
      kept.parent.push_back(i == anchor ? FC_NONE : (*map)[parent[i]]);
      kept.slot.push_back(slot[i]);
      kept.ids[root[i]] = id;
    }
    *this = std::move(kept);
  }
};

}  // namespace bls381
