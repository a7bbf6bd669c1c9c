// SSZ hash_tree_root / signing_root of fixed-size containers on gfx950: the
// message_hash producer in front of bls_verify.
//
// Reference: test_libs/pyspec/eth2spec/utils/ssz/ssz_impl.py:143-163
// (hash_tree_root, signing_root), :110-123 (pack, chunkify), and
// utils/merkle_minimal.py merkleize_chunks (zero-chunk padding to a power of
// two, a single chunk is its own root).  A fixed-size SSZ value serializes to
// the concatenation of its fields, so a root is a small program over the
// item's serialized bytes; bls381_amd/ssz.py compiles a type into it:
//   SSZ_CHUNK off len : push bytes [off, off+len) zero-padded to 32 (len <= 32)
//   SSZ_MERKLE k      : pop k chunks, pad with zero chunks to a power of two,
//                       merkleize, push the root
// One lane runs the program for one item; the chunk stack lives in scratch.
// A variable-size container compiles into a ragged program (ssz_run_ragged below): the same two
// ops over the fixed part of a scope, and ops that follow the item's offsets.
// merkle_branch_root folds a Merkle proof into a leaf (the spec's verify_merkle_branch).
#pragma once
#include "bls381_hash.hpp"

namespace bls381 {

// SSZ_CHUNK, SSZ_MERKLE, SSZ_STACK (chunks) and SSZ_PROG_MAX (u32 words): bls381_defs.hpp

// SHA-256 of two 32-byte chunks (one data block + the constant padding block)
BLS_DEV_INLINE void sha256_pair(uint32_t out[8], const uint32_t l[8], const uint32_t r[8]) {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au,
                   0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  uint32_t blk[16];
  for (int i = 0; i < 8; ++i) { blk[i] = l[i]; blk[8 + i] = r[i]; }
  sha256_compress(h, blk);
  for (int i = 0; i < 16; ++i) blk[i] = 0;
  blk[0] = 0x80000000u;
  blk[15] = 512;                 // bit length of the 64-byte message
  sha256_compress(h, blk);
  for (int i = 0; i < 8; ++i) out[i] = h[i];
}

// Runs `prog` over one serialized item; the root (8 big-endian words) is left in
// root.  Returns false on a malformed program (stack over/underflow).
BLS_DEV_INLINE bool ssz_run(uint32_t root[8], const uint8_t* item, const uint32_t* prog, uint32_t plen,
                           uint32_t (*stk)[8]) {
  int sp = 0;
  for (uint32_t pc = 0; pc < plen;) {
    const uint32_t op = prog[pc];
    if (op == SSZ_CHUNK && pc + 2 < plen) {
      const uint32_t off = prog[pc + 1], len = prog[pc + 2];
      pc += 3;
      if (sp >= SSZ_STACK || len > 32) return false;
      for (int w = 0; w < 8; ++w) {
        uint32_t v = 0;
        for (int b = 0; b < 4; ++b) {
          const uint32_t k = 4 * w + b;
          v = (v << 8) | (k < len ? item[off + k] : 0u);
        }
        stk[sp][w] = v;
      }
      ++sp;
    } else if (op == SSZ_MERKLE && pc + 1 < plen) {
      const uint32_t k = prog[pc + 1];
      pc += 2;
      if (k == 0 || (int)k > sp) return false;
      uint32_t p = 1;
      while (p < k) p <<= 1;
      const int base = sp - (int)k;
      if (base + (int)p > SSZ_STACK) return false;
      for (uint32_t j = k; j < p; ++j)
        for (int w = 0; w < 8; ++w) stk[base + j][w] = 0;
      for (uint32_t width = p; width > 1; width >>= 1)
        for (uint32_t j = 0; j < width / 2; ++j) sha256_pair(stk[base + j], stk[base + 2 * j], stk[base + 2 * j + 1]);
      sp = base + 1;
    } else {
      return false;
    }
  }
  if (sp != 1) return false;
  for (int w = 0; w < 8; ++w) root[w] = stk[0][w];
  return true;
}

// mix_in_length (ssz_impl.py:122-124): v = H(v || length as 32 bytes little-endian)
BLS_DEV_INLINE void merkle_mix_in_length(uint32_t v[8], uint64_t length) {
  uint32_t l[8], r[8];
  for (int w = 0; w < 8; ++w) { l[w] = v[w]; r[w] = 0; }
  r[0] = __builtin_bswap32((uint32_t)length);
  r[1] = __builtin_bswap32((uint32_t)(length >> 32));
  sha256_pair(v, l, r);
}

// ---- ragged programs: the root of a variable-size container from its serialization --
// An item is what ssz_impl.py:72-103 (encode_series) writes for a container: the fixed parts in
// field order with a 4-byte little-endian offset in place of every variable-size field, then the
// variable parts in field order.  A scope is a byte range of the item that holds one such
// container: the item itself, or a variable-size field that is a container.  Offsets are relative
// to their scope.  A ragged program is
//   SSZ_RAGGED fixed           : first op; the item's scope has a fixed part of `fixed` bytes
//   SSZ_CHUNK off len          : as above, off relative to the scope (inside its fixed part)
//   SSZ_MERKLE k               : as above
//   SSZ_FIELD pos next esz     : the basic-list field whose offset word is at `pos` of the scope;
//                                it ends at the offset at `next`, or with the scope (SSZ_NO_NEXT);
//                                pushes mix_in_length(merkleize_chunks(chunkify(bytes)), len / esz)
//   SSZ_ENTER pos next fixed   : the field's byte range becomes the scope (fixed part `fixed`)
//   SSZ_LEAVE                  : back to the enclosing scope
// Fields are visited in order, so the rules an item must keep are checked
// field by field before a byte is read through an offset: a scope is at least as long as its fixed
// part; the first offset equals the fixed part's size; an offset is not below the one before it
// (a field's end is the next field's offset, so "equals the previous end" says both); the last end
// is at most the scope's length; a field's length is a multiple of esz.
//
// The field's merkleisation streams: stk[sp + h] holds the finished node of level h that still
// waits for its right sibling, chunk c merges upward while bit h of c is set, and the end folds the
// waiting nodes with the zero nodes up to chunk_depth(chunks).  A field of C chunks takes
// chunk_depth(C) + 1 stack entries.
enum : int { SSZ_OK = 0, SSZ_BAD_ITEM = 1, SSZ_BAD_PROG = 2 };

BLS_DEV_INLINE uint32_t ssz_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
// ceil(log2 n), 0 for n <= 1 (merkle_minimal.py merkleize_chunks' depth)
BLS_DEV_INLINE uint32_t ssz_chunk_depth(uint32_t n) {
  uint32_t d = 0;
  while (d < 32 && ((uint32_t)1 << d) < n) ++d;
  return d;
}

// pushes the root of the basic list in bytes [lo, hi) of the item (elements of esz bytes) at
// stk[sp]; levels above it are the stream's.  false: the stack cannot hold the field.
// Z is a pointer to the zero-node table's 32-bit words (Z[h] at + 8 h), a global one on the device.
template <class Z>
BLS_DEV_INLINE bool ssz_field_root(uint32_t (*stk)[8], int sp, const uint8_t* item, uint32_t lo, uint32_t hi,
                                   uint32_t esz, Z ztab) {
  const uint32_t nbytes = hi - lo, chunks = nbytes / 32 + (nbytes % 32 != 0);
  const uint32_t depth = ssz_chunk_depth(chunks);
  if (sp + (int)depth + 1 > SSZ_STACK) return false;
  uint32_t v[8];
  for (uint32_t c = 0; c < chunks; ++c) {
    const uint32_t at = lo + 32 * c, left = hi - at;
    for (int w = 0; w < 8; ++w) {
      uint32_t x = 0;
      for (int b = 0; b < 4; ++b) {
        const uint32_t k = 4 * w + b;
        x = (x << 8) | (k < left ? item[at + k] : 0u);
      }
      v[w] = x;
    }
    uint32_t h = 0;
    for (; (c >> h) & 1; ++h) sha256_pair(v, stk[sp + h], v);
    for (int w = 0; w < 8; ++w) stk[sp + h][w] = v[w];
  }
  if (chunks == 0) {
    for (int w = 0; w < 8; ++w) v[w] = 0;          // merkleize_chunks([]) is the zero chunk
  } else if (chunks == (uint32_t)1 << depth) {
    for (int w = 0; w < 8; ++w) v[w] = stk[sp + depth][w];
  } else {
    bool have = false;                             // v: the zero-padded right edge, one level at a time
    for (uint32_t h = 0; h < depth; ++h) {
      uint32_t z[8];
      for (int w = 0; w < 8; ++w) z[w] = __builtin_bswap32(ztab[8 * h + w]);
      if ((chunks >> h) & 1) {
        if (have) {
          for (int w = 0; w < 8; ++w) z[w] = v[w];
        }
        sha256_pair(v, stk[sp + h], z);
        have = true;
      } else if (have) {
        sha256_pair(v, v, z);
      }
    }
  }
  merkle_mix_in_length(v, nbytes / esz);
  for (int w = 0; w < 8; ++w) stk[sp][w] = v[w];
  return true;
}

// Runs a ragged program over the item_len bytes at item.  SSZ_OK: the root (8 big-endian words)
// is in root.  SSZ_BAD_ITEM: the item breaks a rule; nothing outside [item, item + item_len) was
// read.  SSZ_BAD_PROG: a program ssz_ragged_prog_ok (bls381_plan.hpp) rejects.
template <class Z>
BLS_DEV_INLINE int ssz_run_ragged(uint32_t root[8], const uint8_t* item, uint32_t item_len, const uint32_t* prog,
                                  uint32_t plen, uint32_t (*stk)[8], Z ztab) {
  if (plen < 2 || prog[0] != SSZ_RAGGED) return SSZ_BAD_PROG;
  // the scopes: base in the item, length, fixed part, and where the next variable field must begin
  uint32_t base[SSZ_SCOPE_MAX], len[SSZ_SCOPE_MAX], fixed[SSZ_SCOPE_MAX], expect[SSZ_SCOPE_MAX];
  int d = 0, sp = 0;
  base[0] = 0; len[0] = item_len; fixed[0] = expect[0] = prog[1];
  if (item_len < prog[1]) return SSZ_BAD_ITEM;
  for (uint32_t pc = 2; pc < plen;) {
    const uint32_t op = prog[pc];
    if (op == SSZ_CHUNK && pc + 2 < plen) {
      const uint32_t off = prog[pc + 1], n = prog[pc + 2];
      pc += 3;
      if (sp >= SSZ_STACK || n > 32 || off > fixed[d] || n > fixed[d] - off) return SSZ_BAD_PROG;
      const uint8_t* src = item + base[d] + off;
      for (int w = 0; w < 8; ++w) {
        uint32_t v = 0;
        for (int b = 0; b < 4; ++b) {
          const uint32_t k = 4 * w + b;
          v = (v << 8) | (k < n ? src[k] : 0u);
        }
        stk[sp][w] = v;
      }
      ++sp;
    } else if (op == SSZ_MERKLE && pc + 1 < plen) {
      const uint32_t k = prog[pc + 1];
      pc += 2;
      if (k == 0 || (int)k > sp) return SSZ_BAD_PROG;
      uint32_t p = 1;
      while (p < k) p <<= 1;
      const int b0 = sp - (int)k;
      if (b0 + (int)p > SSZ_STACK) return SSZ_BAD_PROG;
      for (uint32_t j = k; j < p; ++j)
        for (int w = 0; w < 8; ++w) stk[b0 + j][w] = 0;
      for (uint32_t width = p; width > 1; width >>= 1)
        for (uint32_t j = 0; j < width / 2; ++j) sha256_pair(stk[b0 + j], stk[b0 + 2 * j], stk[b0 + 2 * j + 1]);
      sp = b0 + 1;
    } else if ((op == SSZ_FIELD || op == SSZ_ENTER) && pc + 3 < plen) {
      const uint32_t pos = prog[pc + 1], next = prog[pc + 2], arg = prog[pc + 3];
      pc += 4;
      if (pos > fixed[d] || fixed[d] - pos < 4 || (next != SSZ_NO_NEXT && (next > fixed[d] || fixed[d] - next < 4)))
        return SSZ_BAD_PROG;
      const uint32_t lo = ssz_le32(item + base[d] + pos);
      const uint32_t hi = next == SSZ_NO_NEXT ? len[d] : ssz_le32(item + base[d] + next);
      if (lo != expect[d] || hi < lo || hi > len[d]) return SSZ_BAD_ITEM;
      expect[d] = hi;
      if (op == SSZ_FIELD) {
        if (arg == 0 || arg > 32 || (arg & (arg - 1))) return SSZ_BAD_PROG;
        if ((hi - lo) & (arg - 1)) return SSZ_BAD_ITEM;
        if (!ssz_field_root(stk, sp, item, base[d] + lo, base[d] + hi, arg, ztab)) return SSZ_BAD_PROG;
        ++sp;
      } else {
        if (d + 1 >= SSZ_SCOPE_MAX) return SSZ_BAD_PROG;
        if (hi - lo < arg) return SSZ_BAD_ITEM;
        base[d + 1] = base[d] + lo; len[d + 1] = hi - lo; fixed[d + 1] = expect[d + 1] = arg;
        ++d;
      }
    } else if (op == SSZ_LEAVE) {
      pc += 1;
      if (d == 0) return SSZ_BAD_PROG;
      --d;
    } else {
      return SSZ_BAD_PROG;
    }
  }
  if (sp != 1 || d != 0) return SSZ_BAD_PROG;
  for (int w = 0; w < 8; ++w) root[w] = stk[0][w];
  return SSZ_OK;
}

// The fold of verify_merkle_branch (specs/core/0_beacon-chain.md:846-857): v holds the leaf
// (8 big-endian words) and is left holding the root of the branch; sibling i is the 32 bytes
// at proof + 32 i, and bit i of `index` puts it on the left (set) or on the right (clear).
// depth <= 64.  P is a byte pointer: a global-address-space one on the device.
template <class P>
BLS_DEV_INLINE void merkle_branch_root(uint32_t v[8], P proof, uint32_t depth, uint64_t index) {
  for (uint32_t i = 0; i < depth; ++i) {
    const bool sib_left = (index >> i) & 1;
    uint32_t l[8], r[8];
    for (int w = 0; w < 8; ++w) {
      const size_t o = 32 * (size_t)i + 4 * w;
      const uint32_t s = ((uint32_t)proof[o] << 24) | ((uint32_t)proof[o + 1] << 16) | ((uint32_t)proof[o + 2] << 8) |
                         (uint32_t)proof[o + 3];
      l[w] = sib_left ? s : v[w];
      r[w] = sib_left ? v[w] : s;
    }
    sha256_pair(v, l, r);
  }
}

}  // namespace bls381
