// Committee selection on gfx950: the producer of the grouped verify's member entries.
//
// Reference: specs/core/0_beacon-chain.md:860-882 (get_shuffled_index, the swap-or-not shuffle),
// :887-890 (compute_committee), :905-917 (get_attesting_indices), :960-982 (get_bitfield_bit,
// verify_bitfield) and :988-1001 (convert_to_indexed).
//
// One round of the shuffle moves `index` to flip = (pivot + n - index) mod n when a bit of
//   source = SHA-256(seed || round || u32le(position / 256)),  position = max(index, flip),
// is set: bit position % 8 of source byte (position % 256) / 8.  The 256 positions of one block
// share a source digest, so a whole list needs rounds * ceil(n / 256) source hashes, all
// independent (the table form: shuffle_source_words per (round, block), then shuffle_walk reads
// one bit per round), while a position that hashes its own blocks needs `rounds` hashes in sequence
// and no table (the direct form: a few positions of a very long list; the rule is in
// bls381_capi.hip).  Both forms and the host unit-test build (host_check.cpp) build their SHA-256
// blocks with shuffle_digest below.
//
// index_count is at most 2^32 - 1 here (the spec allows 2^40): registry entries are 32-bit.
#pragma once
#include "bls381_hash.hpp"

namespace bls381 {

constexpr uint32_t SHUFFLE_ROUNDS_MAX = 255;        // the round is one byte of the hash input
constexpr uint32_t ATT_MAX_COMMITTEE = 4096;        // MAX_INDICES_PER_ATTESTATION
constexpr uint32_t ATT_MASK_WORDS = ATT_MAX_COMMITTEE / 32;
constexpr int ATT_BLOCK = 256;                      // lanes of k_attesting_entries' workgroup

// the seed as the 8 big-endian words of its SHA-256 block (passed to the kernels by value)
struct shuffle_seed { uint32_t w[8]; };
BLS_INLINE shuffle_seed shuffle_seed_from_bytes(const uint8_t* s) {
  shuffle_seed r;
  for (int i = 0; i < 8; ++i)
    r.w[i] = ((uint32_t)s[4 * i] << 24) | ((uint32_t)s[4 * i + 1] << 16) | ((uint32_t)s[4 * i + 2] << 8) | s[4 * i + 3];
  return r;
}

// SHA-256 of the single-block inputs of get_shuffled_index: seed || round (33 bytes, the pivot
// input) or seed || round || u32le(block) (37 bytes, the source input).  d: 8 big-endian words.
BLS_DEV_INLINE void shuffle_digest(uint32_t d[8], const shuffle_seed& seed, uint32_t round, bool source, uint32_t block) {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t blk[16];
  for (int i = 0; i < 8; ++i) blk[i] = seed.w[i];
  for (int i = 8; i < 16; ++i) blk[i] = 0;
  if (source) {
    // bytes 32..37: round, block's four bytes least significant first, 0x80
    blk[8] = (round << 24) | ((block & 0xffu) << 16) | (((block >> 8) & 0xffu) << 8) | ((block >> 16) & 0xffu);
    blk[9] = ((block >> 24) << 24) | 0x00800000u;
    blk[15] = 37 * 8;
  } else {
    blk[8] = (round << 24) | 0x00800000u;
    blk[15] = 33 * 8;
  }
  sha256_compress(h, blk);
  for (int i = 0; i < 8; ++i) d[i] = h[i];
}

BLS_INLINE uint32_t shuffle_bswap(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24);
}

// pivot = bytes_to_int(hash(seed || round)[0:8]) % index_count, in plain 64-bit arithmetic
BLS_DEV_INLINE uint32_t shuffle_pivot(const shuffle_seed& seed, uint32_t round, uint32_t n) {
  uint32_t d[8];
  shuffle_digest(d, seed, round, false, 0);
  const uint64_t v = (uint64_t)shuffle_bswap(d[0]) | ((uint64_t)shuffle_bswap(d[1]) << 32);
  return (uint32_t)(v % n);
}

// The source digest of (round, block) as 8 words whose bit p % 32 of word (p % 256) / 32 is the
// spec's bit of position p (the digest's bytes in memory order on a little-endian machine): the
// table's unit, 32 bytes.
BLS_DEV_INLINE void shuffle_source_words(uint32_t out[8], const shuffle_seed& seed, uint32_t round, uint32_t block) {
  uint32_t d[8];
  shuffle_digest(d, seed, round, true, block);
  for (int i = 0; i < 8; ++i) out[i] = shuffle_bswap(d[i]);
}

// flip = (pivot + n - index) % n without a division: index < n and pivot < n put the sum in
// [1, 2n), which needs 33 bits when n is close to 2^32
BLS_INLINE uint32_t shuffle_flip(uint32_t index, uint32_t pivot, uint32_t n) {
  uint64_t f = (uint64_t)pivot + n - index;
  if (f >= n) f -= n;
  return (uint32_t)f;
}

// The rounds of get_shuffled_index for one index.  pivots[r] from shuffle_pivot; bit(r, position)
// returns the source bit of a position in round r.
template <class P, class Bit>
BLS_DEV_INLINE uint32_t shuffle_walk(uint32_t index, uint32_t n, uint32_t rounds, P pivots, Bit bit) {
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t flip = shuffle_flip(index, pivots[r], n);
    const uint32_t position = index > flip ? index : flip;
    if (bit(r, position)) index = flip;
  }
  return index;
}

// the direct form's bit: the position's own source block, hashed on the spot
struct shuffle_direct_bit {
  shuffle_seed seed;
  BLS_DEV_INLINE bool operator()(uint32_t r, uint32_t position) const {
    uint32_t w[8];
    shuffle_source_words(w, seed, r, position >> 8);
    return (w[(position & 255u) >> 5] >> (position & 31u)) & 1u;
  }
};

// the table form's bit: row r of the table holds blocks_per_row digests of 8 words
// (shuffle_source_words), so position p's bit is bit p % 32 of the row's word p / 32
template <class T>
struct shuffle_table_bit {
  T table;
  size_t row_words;   // 8 * ceil(n / 256)
  BLS_DEV_INLINE bool operator()(uint32_t r, uint32_t position) const {
    return (table[(size_t)r * row_words + (position >> 5)] >> (position & 31u)) & 1u;
  }
};

inline size_t shuffle_blocks(uint64_t n) { return (size_t)((n + 255) / 256); }

// ---- attesting entries: convert_to_indexed's two index sets -------------------------------

// verify_bitfield (0_beacon-chain.md:970-982): the length, and zero padding bits
inline bool bitfield_ok(const uint8_t* bits, size_t nbytes, uint32_t committee_len) {
  if (nbytes != ((size_t)committee_len + 7) / 8) return false;
  if (committee_len % 8 && (bits[nbytes - 1] >> (committee_len % 8))) return false;
  return true;
}

// members of the two groups of one attestation whose bitfields passed bitfield_ok: custody bit 0
// (aggregation bit set, custody bit clear) and custody bit 1 (custody bit set)
inline void attesting_counts(const uint8_t* agg, const uint8_t* cust, size_t nbytes, uint32_t* n0, uint32_t* n1) {
  uint32_t c0 = 0, c1 = 0;
  for (size_t i = 0; i < nbytes; ++i) {
    c0 += (uint32_t)__builtin_popcount((unsigned)(agg[i] & (uint8_t)~cust[i]));
    c1 += (uint32_t)__builtin_popcount((unsigned)cust[i]);
  }
  *n0 = c0;
  *n1 = c1;
}

// what the kernel needs to know about one attestation (built on the host from the popcounts)
struct att_desc {
  uint32_t committee_off, committee_len;   // the slice of the shuffled list
  uint32_t bits_off;                       // byte offset into both bitfield buffers
  uint32_t out_off, n0, n1;                // group 2a at out_off (n0 entries), group 2a+1 right after (n1)
};

// 32 bits of a group's member mask, bits [32 w, 32 w + 32) of the committee: group 0 is
// aggregation & ~custody, group 1 is custody.  Bytes past the bitfield's end read as zero.
template <class B>
BLS_DEV_INLINE uint32_t att_mask_word(B agg, B cust, uint32_t nbytes, uint32_t w, int group) {
  uint32_t m = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = 4 * w + k;
    if (i < nbytes) {
      const uint32_t a = agg[i], c = cust[i];
      m |= (group ? c : (a & ~c & 0xffu)) << (8 * k);
    }
  }
  return m;
}

// One group of one attestation, by the `nt` lanes of a workgroup (lane `tid`; sync() is the
// workgroup barrier; the host build runs it with nt = 1 and an empty sync): compacts the
// committee's members whose mask bit is set into buf (prefix popcount over the mask words in
// cnt), sorts them ascending (bitonic, padded to a power of two with 0xFFFFFFFF, which sorts
// last) and writes the n of them to out.  buf: ATT_MAX_COMMITTEE words, cnt: ATT_MASK_WORDS
// words (LDS on the device); committee_len <= ATT_MAX_COMMITTEE; n = the mask's popcount.
template <class Sync, class C, class B, class O>
BLS_DEV_INLINE void attesting_group(uint32_t* buf, uint32_t* cnt, uint32_t tid, uint32_t nt, Sync sync, C committee,
                                   uint32_t committee_len, B agg, B cust, int group, uint32_t n, O out) {
  const uint32_t nbytes = (committee_len + 7) / 8, nwords = (committee_len + 31) / 32;
  uint32_t p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (uint32_t w = tid; w < nwords; w += nt) cnt[w] = (uint32_t)__builtin_popcount(att_mask_word(agg, cust, nbytes, w, group));
  for (uint32_t i = n + tid; i < p2; i += nt) buf[i] = 0xFFFFFFFFu;
  sync();
  for (uint32_t w = tid; w < nwords; w += nt) {
    uint32_t at = 0;
    for (uint32_t v = 0; v < w; ++v) at += cnt[v];
    uint32_t m = att_mask_word(agg, cust, nbytes, w, group);
    while (m) {
      const uint32_t b = (uint32_t)__builtin_ctz(m);
      m &= m - 1;
      buf[at++] = committee[32 * w + b];   // 32 w + b < committee_len: the padding bits are zero
    }
  }
  sync();
  for (uint32_t k = 2; k <= p2; k <<= 1)
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t i = tid; i < p2; i += nt) {
        const uint32_t l = i ^ j;
        if (l > i) {
          const uint32_t a = buf[i], b = buf[l];
          const bool up = (i & k) == 0;
          if (up ? a > b : a < b) { buf[i] = b; buf[l] = a; }
        }
      }
      sync();
    }
  for (uint32_t i = tid; i < n; i += nt) out[i] = buf[i];
  sync();   // buf is free for the next group
}

}  // namespace bls381
