// Host exports over the ragged root programs of bls381_ssz.hpp: what one lane of
// k_ssz_ragged_root runs for one item, and the host check of a program.  Included once by
// host_check.cpp (lib/libbls381_hostcheck.so) and once by ssz_ragged_check_main.cpp (the
// stand-alone sanitizer program).
#pragma once
#include <cstdint>

#include "bls381_merkle.hpp"

extern "C" {

// the root of the item_len bytes at item under the ragged program: 0 and the root in out32; 1 for
// an item that breaks a rule (out32 all zero, as the kernel leaves it); 2 for a program that is
// not well formed
int hc_ssz_ragged_root(const uint8_t* item, uint32_t item_len, const uint32_t* prog, uint32_t plen, uint8_t* out32) {
  using namespace bls381;
  static const struct Ztab {
    uint32_t w[8 * (MERKLE_DEPTH_MAX + 1)];
    Ztab() { merkle_zero_table((uint8_t*)w); }
  } z;
  uint32_t stk[SSZ_STACK][8];
  uint32_t r[8];
  const int rc = ssz_run_ragged(r, item, item_len, prog, plen, stk, (const uint32_t*)z.w);
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) out32[4 * w + b] = rc == SSZ_OK ? (uint8_t)(r[w] >> (24 - 8 * b)) : 0;
  return rc;
}
// max_field_bytes 0: the longest field a 32-bit offset admits
int hc_ssz_ragged_prog_ok(const uint32_t* prog, uint32_t plen, uint64_t max_field_bytes) {
  return bls381::ssz_ragged_prog_ok(prog, plen, max_field_bytes);
}

}  // extern "C"
