// The epoch context on gfx950: the producer of what the shuffle consumes.
//
// Reference: specs/core/0_beacon-chain.md:660-684 (is_active_validator,
// get_active_validator_indices), :1545 (hash_tree_root of the active index list, an input of
// generate_seed, :807-816) and :822-840 (get_beacon_proposer_index).
//
// A validator field is a little-endian uint64 at base + i * stride bytes: stride 8 is a plain
// array, stride 121 with base = records + 88 / 96 / 113 is activation_epoch / exit_epoch /
// effective_balance of the serialized Validator records (:284-298) that
// bls381_ssz_list_root_device hashes, so one buffer of records serves both.  Loads are 8 bytes
// wide when base and stride are multiples of 8 and byte-wise otherwise; none passes
// base + (n - 1) * stride + 8.
//
// Active indices: validator i is active when activation_epoch <= epoch < exit_epoch, compared as
// unsigned 64-bit numbers (FAR_FUTURE_EPOCH is 2^64 - 1).  The ascending list is compacted by a
// scan in three launches over tiles of ACTIVE_TILE validators (the kernels: bls381_kernels.hpp):
//   k_active_count    item (tile, k, lane) = validator tile * 2048 + k * 256 + lane of a 256-lane
//                     workgroup; the 64-bit __ballot of wave w in round k is ballot 4 k + w of the
//                     tile's 32, kept in the workspace (n / 8 bytes), and the tile's count and
//                     balance sum are their popcounts and the workgroup's LDS sum
//   k_active_scan     one workgroup: the exclusive scan of the tile counts, 256 at a time
//                     (ceil(tiles / 256) rounds, known at launch); writes the count and the sum
//   k_active_scatter  position = tile offset + ballots before + mbcnt over the lane's own ballot;
//                     it reads the ballots, not the fields again
// The balance sum is 64-bit and cannot overflow while n * max balance < 2^64 (2^32 validators of
// less than 2^32 Gwei each; MAX_EFFECTIVE_BALANCE is 32 * 10^9 < 2^35, so 2^29 validators at the
// maximum, far above any registry, stay exact).  Above that it wraps modulo 2^64.
//
// Index chunks: hash_tree_root(List[uint64]) packs four indices per 32-byte chunk, the last chunk
// zero-padded (ssz_impl.py pack); k_index_chunks widens the uint32 list and the Merkle kernels
// hash it at depth merkle_chunk_depth(ceil(n / 4)) with the length n mixed in.
//
// Proposers: try i of a slot looks at candidate = committee[(epoch + i) % len] with
// random_byte = SHA-256(seed || u64le(i / 32))[i % 32] and accepts when
// effective_balance * 255 >= MAX_EFFECTIVE_BALANCE * random_byte.  The balance is clamped to
// max_effective_balance first: the verdict is the same (random_byte <= 255) and with
// max_effective_balance < 2^56 both products fit 64 bits.  (epoch + i) % len is computed as
// (epoch % len + i) % len on the host-reduced epoch % len.  One 256-lane workgroup per slot
// evaluates a window of PROPOSER_WINDOW tries at once (8 digests, one per 32 lanes, shared
// through LDS) and the lowest accepting try wins.
// Divergence: the spec's `while True` stops here after PROPOSER_MAX_TRIES = 2^20 tries with
// 0xFFFFFFFF.  A committee whose members all have balance 0 accepts a try with probability
// 1 / 256 (random_byte == 0), so it reaches the cap with probability (255/256)^(2^20) < 2^-5900.
// A try whose candidate is not below n_validators ends the search with 0xFFFFFFFF as well (the
// spec would index past the registry); its balance is not read.
#pragma once
#include "bls381_shuffle.hpp"

namespace bls381 {

constexpr int EPOCH_BLOCK = 256;                       // lanes of every workgroup here
constexpr uint32_t ACTIVE_ROUNDS = 8;                  // validators per lane of a tile
constexpr uint32_t ACTIVE_TILE = ACTIVE_ROUNDS * EPOCH_BLOCK;
constexpr uint32_t ACTIVE_TILE_BALLOTS = ACTIVE_TILE / 64;
constexpr uint32_t PROPOSER_WINDOW = EPOCH_BLOCK;      // tries evaluated at once
constexpr uint32_t PROPOSER_MAX_TRIES = 1u << 20;
constexpr uint32_t PROPOSER_NONE = 0xFFFFFFFFu;
constexpr uint64_t PROPOSER_BALANCE_LIMIT = (uint64_t)1 << 56;   // max_effective_balance stays below

inline size_t active_tiles(uint64_t n) { return (size_t)((n + ACTIVE_TILE - 1) / ACTIVE_TILE); }

// ---- field access ---------------------------------------------------------------------------
struct u64_field {
  const uint8_t* base;
  size_t stride;
  int wide;   // base and stride are multiples of 8: one 8-byte load
};
inline u64_field make_u64_field(const void* base, size_t stride) {
  return u64_field{(const uint8_t*)base, stride, (((uintptr_t)base | stride) & 7u) == 0 ? 1 : 0};
}
BLS_DEV_INLINE uint64_t field_load(const u64_field& f, size_t i) {
  const uint8_t* p = f.base + i * f.stride;
  if (f.wide) return *(const uint64_t*)p;
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k);
  return v;
}
// bytes a field of n entries spans (what a caller's buffer holds from base on)
inline size_t field_span(size_t n, size_t stride) { return n ? (n - 1) * stride + 8 : 0; }

// ---- active indices -------------------------------------------------------------------------
BLS_DEV_INLINE bool validator_active(const u64_field& activation, const u64_field& exit, uint64_t epoch, size_t i) {
  return field_load(activation, i) <= epoch && epoch < field_load(exit, i);
}
// the validator of lane `lane` (0 .. 255) in round k of a tile
BLS_INLINE uint64_t active_item(size_t tile, uint32_t k, uint32_t lane) {
  return (uint64_t)tile * ACTIVE_TILE + (uint64_t)k * EPOCH_BLOCK + lane;
}
// members of a ballot below lane `lane` (0 .. 63): what mbcnt gives on the device
BLS_INLINE uint32_t ballot_before(uint64_t ballot, uint32_t lane) {
  return (uint32_t)__builtin_popcountll(ballot & (((uint64_t)1 << lane) - 1));
}

// ---- index chunks ---------------------------------------------------------------------------
// word t of the packed chunks of n indices: 4 * ceil(n / 4) words
BLS_INLINE size_t index_chunk_count(uint64_t n) { return (size_t)((n + 3) / 4); }
template <class I>
BLS_DEV_INLINE uint64_t index_chunk_word(I indices, size_t n, size_t t) {
  return t < n ? (uint64_t)indices[t] : 0;
}

// ---- proposers ------------------------------------------------------------------------------
// SHA-256(seed || u64le(q)), the digest that tries 32 q .. 32 q + 31 share: a 40-byte, one-block
// message.  d: 8 big-endian words.
BLS_DEV_INLINE void proposer_digest(uint32_t d[8], const shuffle_seed& seed, uint64_t q) {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t blk[16];
  for (int i = 0; i < 8; ++i) blk[i] = seed.w[i];
  for (int i = 8; i < 16; ++i) blk[i] = 0;
  blk[8] = shuffle_bswap((uint32_t)q);           // bytes 32..39: q least significant byte first
  blk[9] = shuffle_bswap((uint32_t)(q >> 32));
  blk[10] = 0x80000000u;
  blk[15] = 40 * 8;
  sha256_compress(h, blk);
  for (int i = 0; i < 8; ++i) d[i] = h[i];
}
// byte j (0 .. 31) of a digest of 8 big-endian words
BLS_INLINE uint32_t proposer_digest_byte(const uint32_t* d, uint32_t j) {
  return (d[j >> 2] >> (24 - 8 * (j & 3u))) & 0xffu;
}
BLS_INLINE bool proposer_accepts(uint64_t effective_balance, uint64_t max_effective_balance, uint32_t random_byte) {
  const uint64_t eb = effective_balance < max_effective_balance ? effective_balance : max_effective_balance;
  return eb * 255u >= max_effective_balance * random_byte;
}
// a slot's first committee: a slice of the shuffled list, and epoch % len
struct proposer_slot { uint32_t off, len, start; };

enum { PROPOSER_REJECT = 0, PROPOSER_ACCEPT = 1, PROPOSER_OUT_OF_RANGE = 2 };
// Try i of a slot with its random byte: the candidate goes to *candidate.
template <class C>
BLS_DEV_INLINE int proposer_try(C committee, const proposer_slot& sl, uint32_t i, uint32_t random_byte,
                                const u64_field& balance, uint64_t n_validators, uint64_t max_effective_balance,
                                uint32_t* candidate) {
  const uint32_t pos = (uint32_t)(((uint64_t)sl.start + i) % sl.len);
  const uint32_t c = committee[pos];
  *candidate = c;
  if (c >= n_validators) return PROPOSER_OUT_OF_RANGE;
  return proposer_accepts(field_load(balance, c), max_effective_balance, random_byte) ? PROPOSER_ACCEPT : PROPOSER_REJECT;
}

}  // namespace bls381
