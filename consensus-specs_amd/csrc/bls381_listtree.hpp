// An SSZ list kept in memory with the Merkle tree over its chunks: `count <= capacity` items of
// item_size bytes, packed, that take in-place updates as well as appends, and answer
// hash_tree_root of the list (ssz_impl.py:143-155: merkleize_chunks over the chunks, with
// mix_in_length for a list) and proofs of its chunks at the current count.
//
// Two modes.  COMPOSITE: chunk i is the root program (bls381_ssz.hpp) over item i -- List[Validator]
// and every list or vector of fixed-size containers.  PACKED: item_size is 1, 2, 4, 8, 16 or 32
// and chunk j is bytes [32 j, 32 j + 32) of the packed items, zero behind the last item --
// List[uint64], Vector[Bytes32, N].  An item of a packed list lies inside one chunk.
//
// Storage.  The item store (zero-filled at creation; a packed list keeps it zero behind the
// count at all times), then rows 0 .. H of 32-byte nodes back to back, H the first level at
// which the chunks of `capacity` items fit one node; row h has ceil(chunk capacity / 2^h) nodes.
// A packed list has no row 0 of its own: its row 0 IS the item store (off[0] = 0).  Bytes per
// item of capacity: composite item_size + 64; packed 2 item_size.
// Stored node (h, j) holds its value under the current count for every j <= (chunks - 1) >> h and
// every h <= H, so with d = ceil(log2 chunks) the root, node (d, 0), is always there.
//
// Re-hashing is the tile reduction of bls381_merkle.hpp (k_merkle_reduce's body) over the stored
// rows: listtree_levels reads a row up to its node count at the current number of chunks, Z[h]
// beyond it, and writes the same nodes.  TILES ARE THE UNIT OF DIRT: pass k re-hashes the tiles of
// level h0 = k MERKLE_TILE_LOG that hold an ancestor of a changed chunk, tile (chunk >> h0) /
// MERKLE_TILE, up MERKLE_TILE_LOG levels; one dirty leaf costs the dependent chain of its path
// either way.  An append's tiles are contiguous and known to the host.  An update's are found on
// the device, the host never seeing the indices: one flag word per tile of each pass's level,
// listtree_mark (one lane per update) sets them, listtree_compact (one workgroup per pass) turns
// a flag row into the ascending list of its set tiles and the list's length, and the pass runs
// min(n_upd, tiles of the row) workgroups of which those at or above the length return at once.
//
// One source, two compilers (as bls381_merkle.hpp): the kernels k_listtree_* (bls381_kernels.hpp)
// and the host build (host_check.cpp hc_listtree_*).
#pragma once
#include "bls381_merkle.hpp"

namespace bls381 {

// capacity <= 2^31 - 1 items of at most 32 B a chunk: at most 2^31 chunks, H <= 31
constexpr uint32_t LISTTREE_ROWS_MAX = 32;
constexpr uint32_t LISTTREE_PASSES_MAX = (LISTTREE_ROWS_MAX + MERKLE_TILE_LOG - 1) / MERKLE_TILE_LOG;
constexpr uint32_t LISTTREE_COMPACT_LANES = 256;

// by value into every kernel: off[h] is the byte offset of row h in the tree's store, h <= top
struct listtree_shape {
  uint64_t capacity, chunk_cap;   // items; chunks at `capacity` items
  uint32_t item_size, packed, top;
  uint64_t off[LISTTREE_ROWS_MAX];
};

inline bool listtree_packed_size_ok(size_t item_size) {
  return item_size == 1 || item_size == 2 || item_size == 4 || item_size == 8 || item_size == 16 || item_size == 32;
}
// create's checks other than the program's
inline bool listtree_args_ok(uint64_t capacity, uint64_t item_size, bool packed) {
  if (capacity == 0 || capacity > (uint64_t)INT32_MAX || item_size == 0 || item_size > UINT32_MAX) return false;
  return !packed || listtree_packed_size_ok(item_size);
}
// chunks of `count` items
BLS_INLINE uint64_t listtree_chunks(const listtree_shape& sh, uint64_t count) {
  return sh.packed ? (count * sh.item_size + 31) / 32 : count;
}
// the chunk that holds item i (packed: the whole item lies in it)
BLS_INLINE uint64_t listtree_chunk_of(const listtree_shape& sh, uint64_t i) {
  return sh.packed ? i * sh.item_size / 32 : i;
}
// nodes of stored row h: ceil(chunk capacity / 2^h)
BLS_INLINE uint64_t listtree_row_nodes(const listtree_shape& sh, uint32_t h) { return ((sh.chunk_cap - 1) >> h) + 1; }

// the shape, and the store's size in bytes
inline listtree_shape listtree_make_shape(uint64_t capacity, uint32_t item_size, bool packed, uint64_t* store_bytes) {
  listtree_shape sh{};
  sh.capacity = capacity;
  sh.item_size = item_size;
  sh.packed = packed;
  sh.chunk_cap = listtree_chunks(sh, capacity);
  // composite: the items, padded to a 32-byte boundary, then row 0; packed: the items are row 0
  uint64_t off = packed ? 0 : (capacity * item_size + 31) / 32 * 32;
  for (uint32_t h = 0;; ++h) {
    sh.off[h] = off;
    off += 32 * listtree_row_nodes(sh, h);
    if (listtree_row_nodes(sh, h) == 1) { sh.top = h; break; }
  }
  *store_bytes = off;
  return sh;
}

// The levels of a re-hash at `chunks` chunks, as the tile reduction takes them: a row is read
// and written up to its node count, and rows above `top` are not stored.
struct listtree_levels {
  listtree_shape sh;
  uint64_t chunks;
  BLS_DEV_INLINE merkle_level in(uint32_t h) const { return {0, ((chunks - 1) >> h) + 1, sh.off[h]}; }
  BLS_DEV_INLINE merkle_level out(uint32_t h) const {
    if (h > sh.top) return {0, 0, MERKLE_NONE};
    return in(h);
  }
};

// number of passes of any re-hash: levels 0 .. top in steps of MERKLE_TILE_LOG
inline uint32_t listtree_passes(const listtree_shape& sh) { return (sh.top + MERKLE_TILE_LOG - 1) / MERKLE_TILE_LOG; }
// tiles of pass k's level that hold a node at `chunks` chunks (its flag row's length)
inline uint64_t listtree_pass_tiles(uint64_t chunks, uint32_t k) {
  return chunks ? (((chunks - 1) >> (k * MERKLE_TILE_LOG)) / MERKLE_TILE) + 1 : 0;
}

// The passes that re-hash chunks [c0, c1) of a tree with `chunks` >= c1 chunks: contiguous tiles
// (an append; a host-side update of a range).
inline std::vector<merkle_pass> listtree_range_plan(const listtree_shape& sh, uint64_t c0, uint64_t c1) {
  std::vector<merkle_pass> passes;
  for (uint32_t h = 0; c1 > c0 && h < sh.top; h += MERKLE_TILE_LOG) {
    const uint64_t tile0 = (c0 >> h) / MERKLE_TILE;
    passes.push_back({h, std::min(MERKLE_TILE_LOG, sh.top - h), tile0, ((c1 - 1) >> h) / MERKLE_TILE - tile0 + 1});
  }
  return passes;
}

// The workspace of an update of n_upd items, in 32-bit words: per pass a flag row (sized by the
// capacity, so a size asked once holds at every count), a tile list of min(n_upd, row) entries
// and the list's length; then one word for the root program's error flag.
struct listtree_update_ws {
  uint32_t passes;
  uint64_t flags[LISTTREE_PASSES_MAX], list[LISTTREE_PASSES_MAX];   // word offsets
  uint64_t lens, err, flag_words, words;                             // lens: `passes` words
};
inline listtree_update_ws listtree_update_layout(const listtree_shape& sh, uint64_t n_upd) {
  listtree_update_ws w{};
  w.passes = listtree_passes(sh);
  uint64_t at = 0;
  for (uint32_t k = 0; k < w.passes; ++k) {
    w.flags[k] = at;
    at += listtree_pass_tiles(sh.chunk_cap, k);
  }
  w.flag_words = at;
  for (uint32_t k = 0; k < w.passes; ++k) {
    w.list[k] = at;
    at += std::min<uint64_t>(n_upd, listtree_pass_tiles(sh.chunk_cap, k));
  }
  w.lens = at;
  at += w.passes;
  w.err = at;
  w.words = at + 1;
  return w;
}
// Launches an update queues, whatever n_upd is: the scatter, the leaves of a composite list, and
// in a tree with P > 0 passes the mark, the compaction and the P passes.  (An append: the leaves
// of a composite list and the P passes.)
inline uint32_t listtree_update_launches(const listtree_shape& sh) {
  const uint32_t P = listtree_passes(sh);
  return 1 + (sh.packed ? 0 : 1) + (P ? 2 + P : 0);
}
// what travels to the mark and compact kernels by value
struct listtree_marks {
  uint32_t passes;
  uint32_t flags[LISTTREE_PASSES_MAX], list[LISTTREE_PASSES_MAX], tiles[LISTTREE_PASSES_MAX];
  uint32_t lens;
};
// tiles[k]: the flag row's length at the current number of chunks
inline listtree_marks listtree_make_marks(const listtree_update_ws& w, uint64_t chunks) {
  listtree_marks m{};
  m.passes = w.passes;
  for (uint32_t k = 0; k < w.passes; ++k) {
    m.flags[k] = (uint32_t)w.flags[k];
    m.list[k] = (uint32_t)w.list[k];
    m.tiles[k] = (uint32_t)listtree_pass_tiles(chunks, k);
  }
  m.lens = (uint32_t)w.lens;
  return m;
}

// One lane of the scatter: byte b of update t.  An index at or above the count is skipped.
template <class I, class V, class Q>
BLS_DEV_INLINE void listtree_scatter_byte(const listtree_shape& sh, uint64_t count, I indices, V values, uint32_t off,
                                          uint32_t len, uint64_t t, uint32_t b, Q store) {
  const uint64_t i = indices[t];
  if (i < count) store[i * sh.item_size + off + b] = values[t * len + b];
}

// One lane of the mark: update t sets the flag of its chunk's tile in every pass's row.  Equal
// plain stores from many lanes: no atomics.
template <class I, class Q>
BLS_DEV_INLINE void listtree_mark(const listtree_shape& sh, uint64_t count, const listtree_marks& m, I indices, uint64_t t,
                                  Q ws) {
  const uint64_t i = indices[t];
  if (i >= count) return;
  const uint64_t c = listtree_chunk_of(sh, i);
  for (uint32_t k = 0; k < m.passes; ++k) ws[m.flags[k] + (uint32_t)((c >> (k * MERKLE_TILE_LOG)) / MERKLE_TILE)] = 1;
}

// The compaction of one flag row by LISTTREE_COMPACT_LANES lanes: lane l owns the contiguous
// segment [lo, hi) of the row, counts its set flags, and, once every lane's count is known,
// writes its tiles behind those of the lanes before it -- the list is ascending.
BLS_INLINE void listtree_segment(uint32_t tiles, uint32_t lane, uint32_t* lo, uint32_t* hi) {
  const uint32_t per = (tiles + LISTTREE_COMPACT_LANES - 1) / LISTTREE_COMPACT_LANES;
  *lo = lane * per < tiles ? lane * per : tiles;
  *hi = *lo + per < tiles ? *lo + per : tiles;
}
template <class P>
BLS_DEV_INLINE uint32_t listtree_segment_count(P flags, uint32_t lo, uint32_t hi) {
  uint32_t n = 0;
  for (uint32_t t = lo; t < hi; ++t) n += flags[t] != 0;
  return n;
}
template <class P, class Q>
BLS_DEV_INLINE void listtree_segment_write(P flags, uint32_t lo, uint32_t hi, Q list) {
  for (uint32_t t = lo; t < hi; ++t)
    if (flags[t] != 0) *list++ = t;
}

// where sibling h of chunk index i lives at `chunks` chunks: a stored node or Z[h]
template <class P>
BLS_DEV_INLINE P listtree_sibling_src(const listtree_shape& sh, P store, uint64_t chunks, uint64_t i, uint32_t h,
                                      P ztab) {
  const uint64_t s = (i >> h) ^ 1;
  const bool stored = chunks != 0 && h <= sh.top && s <= (chunks - 1) >> h;
  return stored ? store + sh.off[h] / 4 + 8 * s : ztab + 8 * h;
}
}  // namespace bls381
