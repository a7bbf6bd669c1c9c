// Merkle trees across items: tree(leaves[0..n), first, depth) is the tree with 2^depth leaves of
// which leaves first .. first+n-1 are given and every other one is the zero chunk.
//
// Reference: test_libs/pyspec/eth2spec/utils/merkle_minimal.py (calc_merkle_tree_from_leaves,
// get_merkle_root, get_merkle_proof, merkleize_chunks) and ssz_impl.py:122-124 (mix_in_length).
// With Z[0] = 32 zero bytes, Z[h+1] = H(Z[h] || Z[h]), H = SHA-256:
//   node (h, j) covers leaves [j 2^h, (j+1) 2^h); it is Z[h] when that span misses the window
//     [first, first+n), so level h has real nodes only for j in [first >> h, (first+n-1) >> h];
//   the root is node (depth, 0);
//   sibling h of leaf index i is node (h, (i >> h) ^ 1) -- the stored node if it is real, else
//     Z[h] -- for every i < 2^depth, so an index outside the window gets the proof of a zero leaf;
//   mix_in_length(root, L) = H(root || L as 32 bytes little-endian).
// get_merkle_root / get_merkle_proof are first = 0, depth = 32; merkleize_chunks is first = 0,
// depth = ceil(log2 n).  Extension: n = 0 gives Z[depth] (the deposit contract's empty root; the
// reference's get_merkle_root([]) raises).
//
// One source, two compilers: the node rules below run in the kernels (k_merkle_reduce,
// k_merkle_finish, k_merkle_proofs: bls381_kernels.hpp) and, with the tile loop as plain loops,
// in the host build (host_check.cpp hc_merkle_root / hc_merkle_proofs).  Nodes are kept in
// memory as their 32 digest bytes and in registers as 8 big-endian words.  P is a pointer to
// const 32-bit words, Q to 32-bit words: global-address-space ones on the device.
#pragma once
#include "bls381_plan.hpp"
#include "bls381_ssz.hpp"

namespace bls381 {

// (merkle_level, MERKLE_TILE, MERKLE_NONE, the plan: bls381_plan.hpp)

constexpr size_t MERKLE_ZERO_TABLE_BYTES = 32 * (MERKLE_DEPTH_MAX + 1);

// where node idx of a level lives: in the level's row (real nodes [base, base + count), 8 words
// each) or, outside it, the level's zero node z
template <class P>
BLS_DEV_INLINE P merkle_node_src(P row, uint64_t base, uint64_t count, uint64_t idx, P z) {
  return idx - base < count ? row + 8 * (idx - base) : z;   // idx < base wraps far above any count
}
template <class P>
BLS_DEV_INLINE void merkle_load(uint32_t v[8], P src) {
  for (int w = 0; w < 8; ++w) v[w] = __builtin_bswap32(src[w]);
}
template <class Q>
BLS_DEV_INLINE void merkle_store(Q dst, const uint32_t v[8]) {
  for (int w = 0; w < 8; ++w) dst[w] = __builtin_bswap32(v[w]);
}
// keeps node idx of a level (real nodes [base, base + count), row at byte `off` of the node slice, in
// words at `nodes`) when the level is kept and the node real
template <class Q>
BLS_DEV_INLINE void merkle_keep(Q nodes, uint64_t base, uint64_t count, uint64_t off, uint64_t idx,
                                const uint32_t v[8]) {
  if (off != MERKLE_NONE && idx - base < count) merkle_store(nodes + off / 4 + 8 * (idx - base), v);
}

// the lane of a tile's first step: node j of level h0 + 1 from nodes 2j and 2j + 1 of level h0
template <class P>
BLS_DEV_INLINE void merkle_first_step(uint32_t v[8], P row, uint64_t base, uint64_t count, uint64_t j, P z) {
  uint32_t l[8], r[8];
  merkle_load(l, merkle_node_src(row, base, count, 2 * j, z));
  merkle_load(r, merkle_node_src(row, base, count, 2 * j + 1, z));
  sha256_pair(v, l, r);
}

// one level of the final fold: v, node first >> g of level g (the only real one), becomes node
// first >> (g + 1) of level g + 1; a set bit g of `first` puts Z[g] on the left
template <class P>
BLS_DEV_INLINE void merkle_fold_step(uint32_t v[8], uint64_t first, uint32_t g, P ztab) {
  const bool z_left = g < 64 && ((first >> g) & 1);
  uint32_t z[8], l[8], r[8];
  merkle_load(z, ztab + 8 * g);
  for (int w = 0; w < 8; ++w) {
    l[w] = z_left ? z[w] : v[w];
    r[w] = z_left ? v[w] : z[w];
  }
  sha256_pair(v, l, r);
}

// (merkle_mix_in_length: bls381_ssz.hpp, whose ragged programs mix a field's length in)

// where the tile keeps node i (i < MERKLE_TILE / 2) of a step, in words of one 8-plane row: even
// nodes, 16 words of padding, odd nodes.  A lane's pair (2l, 2l + 1) is then at l and l + 80, and
// the 32 lanes of a half wave, writing node l, at l / 2 and 80 + l / 2: LDS banks (word mod 32)
// 0..15 and 16..31.  Nodes side by side (8 words each) would put every fourth lane on one bank.
constexpr uint32_t MERKLE_LDS_ODD = MERKLE_TILE / 4 + 16;
constexpr uint32_t MERKLE_LDS_ROW = MERKLE_LDS_ODD + MERKLE_TILE / 4;
BLS_INLINE uint32_t merkle_lds_slot(uint32_t i) { return (i >> 1) + (i & 1) * MERKLE_LDS_ODD; }

// Z[0 .. 64], 32 bytes each (made once per context; the host build of sha256_compress computes it)
inline void merkle_zero_table(uint8_t out[MERKLE_ZERO_TABLE_BYTES]) {
  uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t h = 0; h <= MERKLE_DEPTH_MAX; ++h) {
    for (int w = 0; w < 8; ++w)
      for (int b = 0; b < 4; ++b) out[32 * h + 4 * w + b] = (uint8_t)(z[w] >> (24 - 8 * b));
    uint32_t nx[8];
    sha256_pair(nx, z, z);
    for (int w = 0; w < 8; ++w) z[w] = nx[w];
  }
}
}  // namespace bls381
