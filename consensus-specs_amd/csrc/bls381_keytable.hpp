// The hash and key comparison of the two pubkey tables (the registry's, k_reg_insert / k_reg_lookup,
// and the batch-local one of process_deposits, k_deposit_insert / k_deposit_resolve): u32 entry per
// slot, REG_EMPTY when free, linear probing from reg_hash & mask, power-of-two size.  Shared by
// the kernels and the host check build, so a test can place keys on chosen slots.
#pragma once
#include "bls381_defs.hpp"

namespace bls381 {

constexpr uint32_t REG_EMPTY = 0xFFFFFFFFu;

// 48 key bytes -> 32-bit hash (all 12 words mixed; the x bytes are uniform)
BLS_DEV_INLINE uint32_t reg_hash(const uint8_t* k) {
  uint32_t h = 0x9E3779B9u;
  for (int w = 0; w < 12; ++w) {
    const uint32_t v = (uint32_t)k[4 * w] | ((uint32_t)k[4 * w + 1] << 8) | ((uint32_t)k[4 * w + 2] << 16) |
                       ((uint32_t)k[4 * w + 3] << 24);
    h = (h ^ v) * 0x85EBCA6Bu;
    h ^= h >> 15;
  }
  return h;
}
BLS_DEV_INLINE bool reg_key_eq(const uint8_t* a, const uint8_t* b) {
  uint32_t d = 0;
  for (int i = 0; i < 48; ++i) d |= (uint32_t)(a[i] ^ b[i]);
  return d == 0;
}

}  // namespace bls381
