// The deposit tree kept in memory: a tree of 2^depth leaves (depth <= 32) that grows by appends
// and answers, at any count k up to the current one, what the deposit contract answers at that
// count -- get_deposit_root() (the reference's get_merkle_root(leaves[:k])) and every leaf's
// proof under it (get_merkle_proof).  Reference: specs/core/0_beacon-chain.md:1630, :1742
// (proofs are against state.latest_eth1_data.deposit_root, the root at the voted count) and the
// contract's incremental tree (deposit_contract.v.py: branch[], get_deposit_root).
//
// Storage.  Rows h = 0 .. H are stored, H the first level at which the capacity fits one node;
// row h has ceil(capacity / 2^h) nodes of 32 bytes, rows back to back (about 64 bytes per leaf
// of capacity).  Stored node (h, j) holds its value under the current count for every
// j <= (count - 1) >> h; a node is COMPLETE at count c when (j + 1) 2^h <= c, and a complete node
// never changes again.
//
// Append of leaves [c, c + n).  Per level, nodes c >> (h+1) .. (c+n-1) >> (h+1) are recomputed
// from row h; a child beyond the row's new node count is Z[h].  This is the tile reduction of
// bls381_merkle.hpp (merkle_first_step, the LDS halving; k_merkle_reduce's body) with the nodes
// left of the window read from the stored row instead of Z: deptree_in is the level a tile
// reads -- every node of the row up to the new count -- and deptree_out the level it writes --
// the nodes that were not complete before the append, no other.  The tree's shape and the two
// counts reach the kernel by value.
//
// Query at count k.  The boundary node of level h is b_h = k >> h and its value is P[h]:
//   P[0] = Z[0];  P[h+1] = H(stored(h, b_h - 1) || P[h]) when bit h of k is set, else H(P[h] || Z[h])
// (the contract's get_deposit_root with branch[h] = the stored complete node); Root(k) = P[depth].
// Rows above H hold no node other than node 0, so no bit of k is set there and the fold is with Z.
// Sibling h of index i, with s = (i >> h) ^ 1, is stored(h, s) if s < b_h, P[h] if s == b_h and
// Z[h] if s > b_h.  Every stored node read this way is complete at k, so appends after k do not
// disturb a query at k.
//
// One source, two compilers (as bls381_merkle.hpp): the kernels k_deptree_append,
// k_deptree_roots, k_deptree_chain and k_deptree_gather (bls381_kernels.hpp) and the host build
// (host_check.cpp hc_deptree_*).
#pragma once
#include "bls381_merkle.hpp"

namespace bls381 {

constexpr uint32_t DEPTREE_DEPTH_MAX = 32;

// by value into every kernel: off[h] is the byte offset of row h in the tree's store, h <= top
struct deptree_shape {
  uint64_t capacity;
  uint32_t depth, top;
  uint64_t off[DEPTREE_DEPTH_MAX + 1];
};

// nodes of row h: ceil(capacity / 2^h)
BLS_INLINE uint64_t deptree_row_nodes(uint64_t capacity, uint32_t h) { return ((capacity - 1) >> h) + 1; }

// the contract's MAX_DEPOSIT_COUNT assert: 0 < capacity <= 2^depth - 1, depth <= 32 (which also
// keeps count == 2^depth out of the query rule)
inline bool deptree_args_ok(uint64_t capacity, uint32_t depth) {
  return depth <= DEPTREE_DEPTH_MAX && capacity != 0 && capacity <= ((uint64_t)1 << depth) - 1;
}
// the shape, and the store's size in bytes
inline deptree_shape deptree_make_shape(uint64_t capacity, uint32_t depth, uint64_t* store_bytes) {
  deptree_shape sh{};
  sh.capacity = capacity;
  sh.depth = depth;
  uint64_t off = 0;
  for (uint32_t h = 0;; ++h) {
    sh.off[h] = off;
    off += 32 * deptree_row_nodes(capacity, h);
    if (deptree_row_nodes(capacity, h) == 1) { sh.top = h; break; }
  }
  *store_bytes = off;
  return sh;
}

// The passes of an append of n leaves at count c: pass k takes the tiles of level h0 = k
// MERKLE_TILE_LOG that hold nodes c >> h0 .. (c+n-1) >> h0 up to level h0 + steps, until `top`.
// At most ceil((ceil(n / 2^h0) + 1) / W) + 1 tiles a pass, whatever c is.
inline std::vector<merkle_pass> deptree_append_plan(const deptree_shape& sh, uint64_t c, uint64_t n) {
  std::vector<merkle_pass> passes;
  for (uint32_t h = 0; n && h < sh.top; h += MERKLE_TILE_LOG) {
    const uint64_t tile0 = (c >> h) / MERKLE_TILE;
    passes.push_back({h, std::min(MERKLE_TILE_LOG, sh.top - h), tile0, ((c + n - 1) >> h) / MERKLE_TILE - tile0 + 1});
  }
  return passes;
}

// The levels of an append that takes the count from c0 to c1 > c0, as the tile reduction takes
// them (merkle_level: real nodes [base, base + count), the row's byte offset at node `base`).
struct deptree_levels {
  deptree_shape sh;
  uint64_t c0, c1;
  // read: the stored row up to its new node count; beyond it Z[h]
  BLS_DEV_INLINE merkle_level in(uint32_t h) const { return {0, ((c1 - 1) >> h) + 1, sh.off[h]}; }
  // written: the nodes that were not complete at c0, up to the new node count; rows above `top`
  // are not stored
  BLS_DEV_INLINE merkle_level out(uint32_t h) const {
    if (h > sh.top) return {0, 0, MERKLE_NONE};
    const uint64_t base = c0 >> h;
    return {base, ((c1 - 1) >> h) - base + 1, sh.off[h] + 32 * base};
  }
};

// One step of the P chain at count k: v = P[h] becomes P[h+1].  store: the tree's rows as words,
// ztab: Z[0 ..] as words.
template <class P>
BLS_DEV_INLINE void deptree_chain_step(uint32_t v[8], const deptree_shape& sh, P store, uint64_t k, uint32_t h,
                                       P ztab) {
  const bool left_stored = (k >> h) & 1;   // then k >= 2^h: row h is stored and node b_h - 1 complete
  uint32_t o[8], l[8], r[8];
  merkle_load(o, left_stored ? store + sh.off[h] / 4 + 8 * ((k >> h) - 1) : ztab + 8 * h);
  for (int w = 0; w < 8; ++w) {
    l[w] = left_stored ? o[w] : v[w];
    r[w] = left_stored ? v[w] : o[w];
  }
  sha256_pair(v, l, r);
}

// where sibling h of leaf index i lives at count k: a stored complete node, P[h] (ptab: P[0 ..]
// as words) or Z[h]
template <class P>
BLS_DEV_INLINE P deptree_sibling_src(const deptree_shape& sh, P store, uint64_t k, uint64_t i, uint32_t h, P ptab,
                                     P ztab) {
  const uint64_t s = (i >> h) ^ 1, b = k >> h;
  if (s < b) return store + sh.off[h] / 4 + 8 * s;   // b >= 1: k >= 2^h, row h is stored
  return s == b ? ptab + 8 * h : ztab + 8 * h;
}
}  // namespace bls381
