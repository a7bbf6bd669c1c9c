// Host-side planning of the launch pipelines in bls381_capi.hip: workspace carving, chunk
// plans for the aggregation trees and the segmented Fp12 products, the verify_multiple
// grouping (py_ecc's semantics), the levels and passes of the Merkle trees across items, and
// the workspace bounds.  Pure host C++ -- no HIP call,
// no device code -- so the unit-test build (host_check.cpp) compiles it with g++ and
// tests/test_host_plan.py reaches it without a GPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "bls381_defs.hpp"

namespace bls381 {

// Bump allocator over a workspace (256-byte aligned slices).  Exceeding the
// capacity throws before anything is launched on the overflowing buffer; ABI
// entry points map it to an error.  With a null base and no capacity it only
// counts: a carve function run over it leaves in `off` the bytes the same carve
// consumes from a real workspace (its pointers are not to be used).
struct Bump {
  uint8_t* base;
  size_t off = 0, cap;
  explicit Bump(void* b = nullptr, size_t c = SIZE_MAX) : base((uint8_t*)b), cap(c) {}
  template <class T> T* take(size_t count) {
    off = (off + 255) & ~(size_t)255;
    if (count * sizeof(T) > cap || off > cap - count * sizeof(T)) throw std::length_error("workspace bound exceeded");
    T* p = (T*)((uintptr_t)base + off);
    off += count * sizeof(T);
    return p;
  }
  size_t left() const { return off < cap ? cap - off : 0; }
};
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
// bytes `carve(Bump&)` consumes, to the next 256-byte boundary
template <class Carve> size_t carved_bytes(Carve&& carve) {
  Bump count;
  carve(count);
  return align256(count.off);
}
constexpr size_t FPW = 4 * FP_LIMBS;   // bytes per Fp element in SoA buffers

// ----------------------------------------------------- verify_batch (C2) --
struct VerifyWs {
  uint32_t *pk_aff, *sig_aff, *h_aff, *f, *koff, *ml_L;
  uint8_t *pk_st, *sig_st, *f_st, *ml_st;
};
// bls_verify batches of at most this many items run each Miller pair on its own lane
// quad or octet (k_miller_verify_lg, 8 or 16 lanes per item: the lowest latency), up to
// BLS_ML_QUAD_MAX_N both pairs of an item on one quad (k_miller_verify_q), above that
// the split loop (k_ml_lines -> k_ml_accum: the least work per item)
#ifndef BLS_ML_OCT_MAX_N
#define BLS_ML_OCT_MAX_N 8192
#endif
// Below ~2^16 items the pair kernels leave SIMDs with one latency-bound wave, so the quads
// win: r02t, wall ms pair -> quad at 16,385 / 32,768 / 49,152 items: 28.7 -> 18.7 / 20.7 /
// 27.7; at 65,536 the pairs win (32.4 vs 35.2).  BLS_FE_QUAD_MAX_N follows the same curve.
#ifndef BLS_ML_QUAD_MAX_N
#define BLS_ML_QUAD_MAX_N 49152
#endif
// the split Miller loop of the throughput path runs in chunks of at most this many items; its
// line products take ML_L_WORDS_PER_ITEM words per item of a chunk
#ifndef BLS_ML_SPLIT_CHUNK
#define BLS_ML_SPLIT_CHUNK 65536
#endif
// Fp12 values the Miller stage of a verify batch writes (two per item on the octet path)
inline size_t verify_nf(size_t n) { return n <= BLS_ML_OCT_MAX_N ? 2 * n : n; }
inline bool verify_split(size_t n) { return n > BLS_ML_QUAD_MAX_N; }
inline size_t verify_split_chunk(size_t n) { return verify_split(n) ? std::min<size_t>(n, BLS_ML_SPLIT_CHUNK) : 0; }
// lines = false: a workspace for the decodes and the hash only (no split-loop line buffer;
// the randomized path's own decode/hash workspace, whose pairings run elsewhere)
inline VerifyWs carve_verify(Bump& b, size_t n, bool lines = true) {
  VerifyWs w;
  const size_t ch = lines ? verify_split_chunk(n) : 0;
  w.ml_L = ch ? b.take<uint32_t>(ML_L_WORDS_PER_ITEM * ch) : nullptr;
  w.ml_st = ch ? b.take<uint8_t>(ch) : nullptr;
  w.pk_aff = b.take<uint32_t>(2 * FP_LIMBS * n);
  w.sig_aff = b.take<uint32_t>(4 * FP_LIMBS * n);
  w.h_aff = b.take<uint32_t>(4 * FP_LIMBS * n);
  w.f = b.take<uint32_t>(12 * FP_LIMBS * verify_nf(n));
  w.pk_st = b.take<uint8_t>(n);
  w.sig_st = b.take<uint8_t>(n);
  w.f_st = b.take<uint8_t>(verify_nf(n));
  w.koff = b.take<uint32_t>(n);
  return w;
}
inline VerifyWs carve_verify(void* ws, size_t n, bool lines = true) {
  Bump b(ws);
  return carve_verify(b, n, lines);
}
inline size_t verify_ws_size(size_t n, bool lines = true) {
  return carved_bytes([&](Bump& b) { carve_verify(b, n, lines); }) + 1024;
}

// --------------------------------------------------------- aggregation --
// plan chunk levels for groups given by host offsets
struct AggPlan {
  std::vector<std::vector<agg_chunk>> levels;   // chunks per level
};
// Level-1 chunks hold 1-4 rounds of one input per lane slot (KBLOCK / lanes-per-point inputs per
// round): as few rounds as still give AGG_WG_TARGET workgroups (two waves per SIMD over the whole
// chip), so a large single group (C4: 2^17 keys) is not summed four keys per lane on half the SIMDs.
// CHUNK_MIN bounds the chunk count for the workspace sizes (G2 points: 64 per round).
constexpr uint32_t CHUNK_MIN = KBLOCK / 2;
constexpr size_t AGG_WG_TARGET = 1024;
// level-1 chunks averaging fewer inputs than this are summed one lane per chunk (k_agg_lanes)
constexpr size_t AGG_LANE_AVG_MAX = 8;
constexpr uint32_t CHUNK_LN = 4 * KBLOCK;

inline AggPlan plan_agg(size_t ng, const uint32_t* offsets, int lanes_per_point = 1) {
  AggPlan p;
  std::vector<uint32_t> cur_off(offsets, offsets + ng + 1);
  const uint32_t per_round = KBLOCK / (uint32_t)lanes_per_point;
  const size_t total = ng ? (size_t)offsets[ng] - offsets[0] : 0;
  const size_t rounds = std::min<size_t>(4, std::max<size_t>(1, (total + AGG_WG_TARGET * per_round - 1) /
                                                                     (AGG_WG_TARGET * per_round)));
  uint32_t chunk = per_round * (uint32_t)rounds;
  while (true) {
    std::vector<agg_chunk> lv;
    std::vector<uint32_t> next_off(ng + 1, 0);
    bool multi = false;
    for (size_t g = 0; g < ng; ++g) {
      next_off[g] = (uint32_t)lv.size();
      const uint32_t b0 = cur_off[g], e0 = cur_off[g + 1];
      if (e0 <= b0) { lv.push_back({b0, b0}); continue; }
      uint32_t cnt = 0;
      for (uint32_t x = b0; x < e0; x += chunk) { lv.push_back({x, x + chunk < e0 ? x + chunk : e0}); ++cnt; }
      if (cnt > 1) multi = true;
    }
    next_off[ng] = (uint32_t)lv.size();
    p.levels.push_back(lv);
    if (!multi) break;
    cur_off = next_off;
    chunk = CHUNK_LN;
  }
  return p;
}

// one level of n chunks: the chunk list, n values of ncomp Fp components, n statuses (an
// aggregation level: 3 or 6 components; a product pass: 12)
inline size_t chunk_level_bytes(size_t n, size_t ncomp) {
  return align256(n * sizeof(agg_chunk)) + align256(n * ncomp * FPW) + align256(n);
}
inline size_t agg_ws_size(const AggPlan& p, int ncomp) {
  size_t s = 1024;
  for (auto& lv : p.levels) s += chunk_level_bytes(lv.size(), ncomp);
  return s;
}
// the G1 bound from sizes alone (bls381_aggregate_pubkeys_batch_workspace_size): worst case
// chunking, every group splits into ceil(size/CHUNK) chunks, plus levels
inline size_t agg_ws_bound_sizes(size_t n_groups, size_t n_pks) {
  const size_t chunks = n_groups + n_pks / CHUNK_MIN + 1;
  return 8192 + 3 * chunk_level_bytes(chunks, 3);
}

// ------------------------------------------------- verify_multiple pieces --
// Host plan for a batch of bls_verify_multiple calls.  Within each call the
// pubkeys are grouped by distinct message (first-appearance order), as py_ecc's
// verify_multiple does; every group becomes one pair
// (hash_to_G2(m), sum of its pubkeys) and each call adds (sig, -g1).  When the
// key bytes are on the host, a group whose keys are all the canonical infinity
// encoding and an infinite signature are dropped (py_ecc's pairing with an
// infinite point is 1).  A call's pairs run two at a time on lane quads
// (k_miller_quads: one pair per half, shared squarings); a call with several
// quads multiplies them in segmented product passes; one final exponentiation
// per call.
constexpr int32_t PAIR_NONE = INT32_MIN;

// verify_multiple batches of at most this many Miller pairs run one pair per lane quad
// (the latency path of small batches: an epoch's attestations, single calls)
#ifndef BLS_VM_TASK_MAX
#define BLS_VM_TASK_MAX 8192
#endif
using ProductPasses = std::vector<std::vector<agg_chunk>>;
struct VmPlan {
  size_t n_calls = 0, n_keys = 0, G = 0, nquads = 0;
  std::vector<uint32_t> key_idx;        // caller key index of every group member, in group order
  std::vector<uint32_t> group_off;      // G + 1 offsets into key_idx
  std::vector<uint8_t> group_msg;       // G x mlen
  std::vector<uint32_t> group_call;     // G: owning call (whose domain hashes the message)
  std::vector<int32_t> quad_pair;       // 2 per quad: group >= 0, -(call + 1) = the signature pair, or PAIR_NONE
  std::vector<uint32_t> call_quad_off;  // n_calls + 1 offsets into the quads
  ProductPasses passes;                 // segmented Fp12 products (empty: one quad per call)
  // latency path (small batches): one quad or octet per Miller pair (k_miller_tasks); the pair
  // tasks are the quad_pair entries, and these passes multiply them per call
  bool tasks = false;
  ProductPasses task_passes;
  // large batches: the signature pairs leave the quads (each call's group pairs fill whole
  // quads; its signature pair runs on a side stream beside hash_to_G2).  Miller values sit
  // in per-call slot ranges [quads of call c][signature of call c]: quad q writes slot
  // quad_slot[q], call c's signature slot sig_slot[c] (task sig_task[c]); passes multiply them.
  std::vector<uint32_t> quad_slot, sig_slot;
  std::vector<int32_t> sig_task;
  size_t nslots = 0;
  AggPlan agg;                                 // group pubkey sums over key_idx order
  const ProductPasses& product_passes() const { return tasks ? task_passes : passes; }
};

constexpr uint32_t PROD_CHUNK = 8;

// Segmented product passes over segments off[c]..off[c+1]: each pass multiplies
// runs of <= PROD_CHUNK values; it ends when every segment is one value.  An
// empty segment yields one chunk {b, b} (product 1).  At least one pass runs.
inline ProductPasses plan_products(std::vector<uint32_t> off) {
  ProductPasses passes;
  const size_t ns = off.size() - 1;
  while (true) {
    std::vector<agg_chunk> chunks;
    std::vector<uint32_t> next(ns + 1, 0);
    bool more = false;
    for (size_t c = 0; c < ns; ++c) {
      next[c] = (uint32_t)chunks.size();
      const uint32_t b0 = off[c], e0 = off[c + 1];
      if (e0 <= b0) { chunks.push_back({b0, b0}); continue; }
      for (uint32_t x = b0; x < e0; x += PROD_CHUNK) chunks.push_back({x, x + PROD_CHUNK < e0 ? x + PROD_CHUNK : e0});
      if (e0 - b0 > PROD_CHUNK) more = true;
    }
    next[ns] = (uint32_t)chunks.size();
    passes.push_back(std::move(chunks));
    off = std::move(next);
    if (!more) break;
  }
  return passes;
}

inline bool is_inf_encoding(const uint8_t* b, size_t len) {
  if (b[0] != 0xC0) return false;
  for (size_t i = 1; i < len; ++i)
    if (b[i]) return false;
  return true;
}

// 64-bit mix of a message (8-byte words, multiply-xorshift), for the grouping table
inline uint64_t msg_hash(const uint8_t* m, size_t len) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ len;
  size_t i = 0;
  for (; i + 8 <= len; i += 8) {
    uint64_t w;
    std::memcpy(&w, m + i, 8);
    h = (h ^ w) * 0xbf58476d1ce4e5b9ull;
    h ^= h >> 31;
  }
  uint64_t t = 0;
  for (size_t k = 0; i + k < len; ++k) t |= (uint64_t)m[i + k] << (8 * k);
  h = (h ^ t) * 0x94d049bb133111ebull;
  return h ^ (h >> 29);
}

// Shared tail of the planners: small batches run every pair (signatures included) as a
// lane-quad task; large ones take the signature pairs out of the quads (VmPlan comments).
inline void finish_plan(VmPlan& pl) {
  const size_t n_calls = pl.n_calls;
  pl.nquads = pl.quad_pair.size() / 2;
  pl.tasks = 2 * pl.nquads <= BLS_VM_TASK_MAX;
  if (pl.tasks) {
    std::vector<uint32_t> toff(pl.call_quad_off.size());
    for (size_t k = 0; k < toff.size(); ++k) toff[k] = 2 * pl.call_quad_off[k];
    pl.task_passes = plan_products(toff);
    return;
  }
  std::vector<int32_t> qp;
  std::vector<uint32_t> cqo{0}, foff{0};
  pl.sig_task.assign(n_calls, PAIR_NONE);
  std::vector<int32_t> groups;
  for (size_t c = 0; c < n_calls; ++c) {
    groups.clear();
    for (uint32_t e = 2 * pl.call_quad_off[c]; e < 2 * pl.call_quad_off[c + 1]; ++e) {
      const int32_t v = pl.quad_pair[e];
      if (v >= 0) groups.push_back(v);
      else if (v != PAIR_NONE) pl.sig_task[c] = v;
    }
    for (size_t k = 0; k < groups.size(); k += 2) {
      qp.push_back(groups[k]);
      qp.push_back(k + 1 < groups.size() ? groups[k + 1] : PAIR_NONE);
    }
    cqo.push_back((uint32_t)(qp.size() / 2));
    foff.push_back(cqo.back() + (uint32_t)(c + 1));
  }
  pl.quad_pair = std::move(qp);
  pl.call_quad_off = std::move(cqo);
  pl.nquads = pl.quad_pair.size() / 2;
  pl.nslots = pl.nquads + n_calls;
  pl.quad_slot.resize(pl.nquads);
  pl.sig_slot.resize(n_calls);
  for (size_t c = 0; c < n_calls; ++c) {
    for (uint32_t q = pl.call_quad_off[c]; q < pl.call_quad_off[c + 1]; ++q) pl.quad_slot[q] = q + (uint32_t)c;
    pl.sig_slot[c] = foff[c + 1] - 1;
  }
  pl.passes = plan_products(foff);
}

// a call's pairs two per quad (the last quad's second half idle), and the call's quad offset
inline void push_call_quads(VmPlan& pl, const std::vector<int32_t>& pairs) {
  for (size_t k = 0; k < pairs.size(); k += 2) {
    pl.quad_pair.push_back(pairs[k]);
    pl.quad_pair.push_back(k + 1 < pairs.size() ? pairs[k + 1] : PAIR_NONE);
  }
  pl.call_quad_off.push_back((uint32_t)(pl.quad_pair.size() / 2));
}

// Host plan of a verify_multiple batch: per call, pubkeys grouped by distinct message
// (py_ecc's verify_multiple: groups in first-occurrence order, members in index order).
// One flat open-addressing table (generation-stamped, reused across calls) and a
// counting sort per call: linear in the number of keys.
// h_pks / h_sigs may be NULL (device-resident keys / signatures: nothing is dropped)
inline VmPlan plan_vm(size_t n_calls, const uint32_t* call_off, const uint8_t* msgs, size_t mlen, const uint8_t* h_pks,
                      const uint8_t* h_sigs, const int* with_sig) {
  VmPlan pl;
  pl.n_calls = n_calls;
  pl.n_keys = call_off[n_calls];
  pl.group_off.push_back(0);
  pl.call_quad_off.push_back(0);
  pl.key_idx.reserve(pl.n_keys);
  size_t maxc = 0;
  for (size_t c = 0; c < n_calls; ++c) maxc = std::max<size_t>(maxc, call_off[c + 1] - call_off[c]);
  size_t cap = 16;
  while (cap < 2 * maxc) cap <<= 1;
  std::vector<uint32_t> slot(cap), stamp(cap, 0), gid(maxc), first, cnt, pos, flat(maxc);
  std::vector<int32_t> pairs;
  auto same = [&](uint32_t a, uint32_t b) { return mlen == 0 || std::memcmp(msgs + mlen * a, msgs + mlen * b, mlen) == 0; };
  for (size_t c = 0; c < n_calls; ++c) {
    const uint32_t b0 = call_off[c], e0 = call_off[c + 1], gen = (uint32_t)c + 1;
    first.clear();
    cnt.clear();
    for (uint32_t i = b0; i < e0; ++i) {
      size_t h = mlen ? (size_t)msg_hash(msgs + mlen * (size_t)i, mlen) & (cap - 1) : 0;
      while (true) {
        if (stamp[h] != gen) {
          stamp[h] = gen;
          slot[h] = (uint32_t)first.size();
          first.push_back(i);
          cnt.push_back(0);
          break;
        }
        if (same(first[slot[h]], i)) break;
        h = (h + 1) & (cap - 1);
      }
      gid[i - b0] = slot[h];
      ++cnt[slot[h]];
    }
    const size_t ng = first.size();
    pos.assign(ng + 1, 0);
    for (size_t g = 0; g < ng; ++g) pos[g + 1] = pos[g] + cnt[g];
    for (uint32_t i = b0; i < e0; ++i) flat[pos[gid[i - b0]]++] = i;   // pos[g] ends at group g's end
    pairs.clear();
    for (size_t g = 0; g < ng; ++g) {
      const uint32_t* m = flat.data() + pos[g] - cnt[g];
      if (h_pks) {
        bool all_inf = true;
        for (uint32_t k = 0; k < cnt[g] && all_inf; ++k) all_inf = is_inf_encoding(h_pks + 48 * (size_t)m[k], 48);
        if (all_inf) continue;
      }
      pl.key_idx.insert(pl.key_idx.end(), m, m + cnt[g]);
      pl.group_off.push_back((uint32_t)pl.key_idx.size());
      pl.group_msg.insert(pl.group_msg.end(), msgs + mlen * first[g], msgs + mlen * (first[g] + 1));
      pl.group_call.push_back((uint32_t)c);
      pairs.push_back((int32_t)pl.G);
      ++pl.G;
    }
    if (with_sig[c] && !(h_sigs && is_inf_encoding(h_sigs + 96 * c, 96))) pairs.push_back(-(int32_t)c - 1);
    if (pairs.empty()) pairs.push_back(PAIR_NONE);   // the empty product: one idle quad, f = 1
    push_call_quads(pl, pairs);
  }
  finish_plan(pl);
  if (pl.G) pl.agg = plan_agg(pl.G, pl.group_off.data());
  return pl;
}

// Host plan from caller-given groups (bls381_verify_multiple_grouped_device): the same
// VmPlan as plan_vm, with key_idx the caller's key order; groups of one call with equal
// messages are merged (first-occurrence order), empty groups dropped.
inline VmPlan plan_vm_grouped(size_t n_calls, const uint32_t* call_group_off, const uint32_t* group_key_off,
                              const uint8_t* msgs, size_t mlen) {
  VmPlan pl;
  pl.n_calls = n_calls;
  const size_t ng_all = call_group_off[n_calls];
  pl.n_keys = group_key_off[ng_all];
  pl.group_off.push_back(0);
  pl.call_quad_off.push_back(0);
  pl.key_idx.reserve(pl.n_keys);
  size_t maxc = 0;
  for (size_t c = 0; c < n_calls; ++c) maxc = std::max<size_t>(maxc, call_group_off[c + 1] - call_group_off[c]);
  size_t cap = 16;
  while (cap < 2 * maxc) cap <<= 1;
  std::vector<uint32_t> slot(cap), stamp(cap, 0), first;
  std::vector<std::vector<uint32_t>> extra;   // later groups merged into a distinct message (rare)
  std::vector<int32_t> pairs;
  auto same = [&](uint32_t a, uint32_t b) { return mlen == 0 || std::memcmp(msgs + mlen * a, msgs + mlen * b, mlen) == 0; };
  for (size_t c = 0; c < n_calls; ++c) {
    const uint32_t gen = (uint32_t)c + 1;
    first.clear();
    extra.clear();
    for (uint32_t g = call_group_off[c]; g < call_group_off[c + 1]; ++g) {
      if (group_key_off[g + 1] == group_key_off[g]) continue;   // the empty aggregate: pairing 1
      size_t h = mlen ? (size_t)msg_hash(msgs + mlen * (size_t)g, mlen) & (cap - 1) : 0;
      while (true) {
        if (stamp[h] != gen) {
          stamp[h] = gen;
          slot[h] = (uint32_t)first.size();
          first.push_back(g);
          extra.emplace_back();
          break;
        }
        if (same(first[slot[h]], g)) { extra[slot[h]].push_back(g); break; }
        h = (h + 1) & (cap - 1);
      }
    }
    pairs.clear();
    for (size_t d = 0; d < first.size(); ++d) {
      for (uint32_t k = group_key_off[first[d]]; k < group_key_off[first[d] + 1]; ++k) pl.key_idx.push_back(k);
      for (uint32_t g : extra[d])
        for (uint32_t k = group_key_off[g]; k < group_key_off[g + 1]; ++k) pl.key_idx.push_back(k);
      pl.group_off.push_back((uint32_t)pl.key_idx.size());
      pl.group_msg.insert(pl.group_msg.end(), msgs + mlen * first[d], msgs + mlen * (first[d] + 1));
      pl.group_call.push_back((uint32_t)c);
      pairs.push_back((int32_t)pl.G);
      ++pl.G;
    }
    pairs.push_back(-(int32_t)c - 1);   // the signature pair (an infinite signature is idle on the device)
    push_call_quads(pl, pairs);
  }
  finish_plan(pl);
  if (pl.G) pl.agg = plan_agg(pl.G, pl.group_off.data());
  return pl;
}

// run_vm_batch's allocations for G groups, nq quads, nc calls and nk member keys (each one
// above its count), plus the final verdict bytes; agg_bytes / pass_bytes: the group-sum levels
// and the product passes
inline size_t vm_ws_terms(size_t G, size_t nq, size_t nc, size_t nk, size_t mlen, size_t agg_bytes, size_t pass_bytes) {
  size_t s = 1 << 16;
  s += align256(4 * nk) + align256(G * mlen + 1) + align256(4 * G) + align256(8 * G + 1) + align256(48 * nk) +
       align256(8 * nq);
  s += align256(2 * FPW * G) + align256(G) + align256(4 * FPW * G) + align256(G) + align256(4 * G);
  s += agg_bytes + 256;
  s += align256(4 * FPW * nc) + align256(nc);
  // Miller values: quads, or two pair tasks per quad on the latency path
  s += align256(12 * FPW * (2 * nq + nc)) + align256(2 * nq + nc) + align256(4 * nq) + 2 * align256(4 * nc);
  s += pass_bytes;
  s += align256(nc);
  return s;
}

// workspace bound of run_vm_batch for a plan
inline size_t vm_ws_bound(const VmPlan& pl, size_t mlen) {
  size_t pass_bytes = 0;
  for (const auto& ch : pl.product_passes()) pass_bytes += chunk_level_bytes(ch.size(), 12);
  return vm_ws_terms(pl.G + 1, pl.nquads + 1, pl.n_calls + 1, pl.key_idx.size() + 1, mlen, agg_ws_size(pl.agg, 3),
                     pass_bytes);
}

// the same bound from sizes alone (device entry point: the caller sizes the workspace before the plan exists)
inline size_t vm_ws_bound_sizes(size_t n_calls, size_t n_keys, size_t mlen) {
  const size_t G = n_keys + 1, nq = n_keys / 2 + n_calls + 1, nc = n_calls + 1, nk = n_keys + 1;
  // group-sum levels: chunks <= groups + keys / CHUNK per level, three levels at most below 2^27 keys
  const size_t chunks = G + n_keys / CHUNK_MIN + 1;
  // product passes: <= nt / 8 + n_calls chunks per pass over nt <= 2 nq values, and the
  // sizes shrink 8x per pass
  const size_t pc = nq / 2 + 2 * nc;
  return vm_ws_terms(G, nq, nc, nk, mlen, 3 * chunk_level_bytes(chunks, 3), 8 * chunk_level_bytes(pc, 12));
}

// ------------------------------------------------------------- SSZ roots --
// host check of a program: balanced stack, chunk reads inside the item, sizes in bounds (the kernel
// re-checks the stack; reads past the item are what this rules out)
inline bool ssz_prog_ok(const uint32_t* prog, uint32_t plen, size_t item_size) {
  if (!prog || plen == 0 || plen > SSZ_PROG_MAX) return false;
  int sp = 0, peak = 0;
  for (uint32_t pc = 0; pc < plen;) {
    if (prog[pc] == SSZ_CHUNK && pc + 2 < plen) {
      if (prog[pc + 2] > 32 || (size_t)prog[pc + 1] + prog[pc + 2] > item_size) return false;
      ++sp; pc += 3;
    } else if (prog[pc] == SSZ_MERKLE && pc + 1 < plen) {
      const uint32_t k = prog[pc + 1];
      if (k == 0 || (int)k > sp) return false;
      uint32_t p = 1;
      while (p < k) p <<= 1;
      if (sp - (int)k + (int)p > peak) peak = sp - (int)k + (int)p;
      sp = sp - (int)k + 1; pc += 2;
    } else {
      return false;
    }
    if (sp > peak) peak = sp;
  }
  return sp == 1 && peak <= SSZ_STACK;
}
// the ragged counterpart (ssz_run_ragged): the same walk with the scopes.  Chunk reads and offset
// words lie inside the fixed part of their scope (the item's bytes past it are the item's to
// bound, at run time), scopes nest SSZ_SCOPE_MAX deep at most, a fixed part is at most
// SSZ_FIXED_MAX bytes, and the stack holds the stream of the longest field the call admits:
// max_field_bytes, or with 0 what a 32-bit offset can span (2^27 chunks, 28 entries).
inline bool ssz_ragged_prog_ok(const uint32_t* prog, uint32_t plen, uint64_t max_field_bytes) {
  if (!prog || plen < 2 || plen > SSZ_PROG_MAX || prog[0] != SSZ_RAGGED || prog[1] > SSZ_FIXED_MAX) return false;
  if (max_field_bytes == 0 || max_field_bytes > 0xffffffffull) max_field_bytes = 0xffffffffull;
  const uint64_t max_chunks = (max_field_bytes + 31) / 32;
  int stream = 1;                                  // chunk_depth(max_chunks) + 1
  while (((uint64_t)1 << (stream - 1)) < max_chunks) ++stream;
  uint32_t fixed[SSZ_SCOPE_MAX] = {prog[1]};
  int d = 0, sp = 0, peak = 0;
  const auto word_in = [&](uint32_t pos) { return pos <= fixed[d] && fixed[d] - pos >= 4; };
  for (uint32_t pc = 2; pc < plen;) {
    const uint32_t op = prog[pc];
    if (op == SSZ_CHUNK && pc + 2 < plen) {
      if (prog[pc + 2] > 32 || (uint64_t)prog[pc + 1] + prog[pc + 2] > fixed[d]) return false;
      ++sp; pc += 3;
    } else if (op == SSZ_MERKLE && pc + 1 < plen) {
      const uint32_t k = prog[pc + 1];
      if (k == 0 || (int)k > sp) return false;
      uint32_t p = 1;
      while (p < k) p <<= 1;
      if (sp - (int)k + (int)p > peak) peak = sp - (int)k + (int)p;
      sp = sp - (int)k + 1; pc += 2;
    } else if ((op == SSZ_FIELD || op == SSZ_ENTER) && pc + 3 < plen) {
      const uint32_t next = prog[pc + 2], arg = prog[pc + 3];
      if (!word_in(prog[pc + 1]) || (next != SSZ_NO_NEXT && !word_in(next))) return false;
      if (op == SSZ_FIELD) {
        if (arg == 0 || arg > 32 || (arg & (arg - 1))) return false;
        if (sp + stream > peak) peak = sp + stream;
        ++sp;
      } else {
        if (d + 1 >= SSZ_SCOPE_MAX || arg > SSZ_FIXED_MAX) return false;
        fixed[++d] = arg;
      }
      pc += 4;
    } else if (op == SSZ_LEAVE) {
      if (d == 0) return false;
      --d; pc += 1;
    } else {
      return false;
    }
    if (sp > peak) peak = sp;
  }
  return sp == 1 && d == 0 && peak <= SSZ_STACK;
}
// signing_root(DepositData) (0_beacon-chain.md:394-403; ssz_impl.py:158-163): pubkey Bytes48 (2 chunks),
// withdrawal_credentials Bytes32, amount uint64; the signature field is left out
constexpr uint32_t DEPOSIT_SIGNING_PROG[] = {SSZ_CHUNK, 0, 32, SSZ_CHUNK, 32, 16, SSZ_MERKLE, 2,
                                             SSZ_CHUNK, 48, 32, SSZ_CHUNK, 80, 8, SSZ_MERKLE, 3};
constexpr uint32_t DEPOSIT_SIGNING_PROG_LEN = sizeof(DEPOSIT_SIGNING_PROG) / 4;
constexpr size_t DEPOSIT_DATA_BYTES = 48 + 32 + 8 + 96;
// hash_tree_root(DepositData), the leaf of the deposit tree (0_beacon-chain.md:1742-1748): the four
// fields, the signature Bytes96 as 3 chunks padded to 4
constexpr uint32_t DEPOSIT_ROOT_PROG[] = {SSZ_CHUNK, 0, 32, SSZ_CHUNK, 32, 16, SSZ_MERKLE, 2,
                                          SSZ_CHUNK, 48, 32, SSZ_CHUNK, 80, 8,
                                          SSZ_CHUNK, 88, 32, SSZ_CHUNK, 120, 32, SSZ_CHUNK, 152, 32, SSZ_MERKLE, 3,
                                          SSZ_MERKLE, 4};
constexpr uint32_t DEPOSIT_ROOT_PROG_LEN = sizeof(DEPOSIT_ROOT_PROG) / 4;
// a serialized Deposit (0_beacon-chain.md:457-461): the proof, Vector[Bytes32, 32], then the data
constexpr uint32_t DEPOSIT_PROOF_DEPTH = 32;
constexpr size_t DEPOSIT_PROOF_BYTES = 32 * DEPOSIT_PROOF_DEPTH;
constexpr size_t DEPOSIT_BYTES = DEPOSIT_PROOF_BYTES + DEPOSIT_DATA_BYTES;
// slots of process_deposits' batch-local key table: a power of two >= 2 n
inline size_t deposit_table_slots(size_t n) {
  size_t t = 16;
  while (t < 2 * n) t <<= 1;
  return t;
}
// slots of the registry's key table: the smallest power of two >= 2 capacity
inline size_t registry_table_slots(size_t capacity) {
  size_t t = 1;
  while (t < 2 * capacity) t <<= 1;
  return t;
}

// ----------------------------------------------------------- Merkle trees --
// The plan of tree(leaves[0..n), first, depth) (bls381_merkle.hpp): the tree with 2^depth leaves
// of which first .. first+n-1 are given and every other one is the zero chunk.  Level h has real
// nodes [first >> h, (first+n-1) >> h]; a pass of k_merkle_reduce takes tiles of MERKLE_TILE
// nodes of one level, aligned in absolute node index, up MERKLE_TILE_LOG levels (or to `depth`),
// and passes repeat until one real node is left at level `top`; one lane folds that node with
// zero nodes up to `depth`.  Kept rows lie back to back in one slice of the workspace, row h
// starting at node first >> h: every level 1 .. depth with keep (the proofs' source), else only
// the levels a pass ends on (the next pass's input).
constexpr uint32_t MERKLE_TILE_LOG = 8;
constexpr uint32_t MERKLE_TILE = 1u << MERKLE_TILE_LOG;   // W: nodes of a tile, two per lane
constexpr uint32_t MERKLE_DEPTH_MAX = 64;
constexpr uint64_t MERKLE_NONE = UINT64_MAX;
// real nodes [base, base + count) of a level; off: the row's byte offset in the node slice, or
// MERKLE_NONE when the level is not kept (level 0 is the caller's leaves)
struct merkle_level {
  uint64_t base, count, off;
};
struct merkle_pass {
  uint32_t h0, steps;     // input level, levels climbed
  uint64_t tile0, tiles;  // absolute index of the first tile, tile count (= workgroups)
};
struct MerklePlan {
  uint64_t n = 0, first = 0;
  uint32_t depth = 0, top = 0;   // top: the level the passes end on, with one real node
  merkle_level lv[MERKLE_DEPTH_MAX + 1];
  std::vector<merkle_pass> passes;
  size_t node_bytes = 0;
};
inline uint64_t merkle_shr(uint64_t x, uint32_t h) { return h >= 64 ? 0 : x >> h; }
// the tree's shape: depth <= 64, first + n neither overflowing nor above 2^depth
inline bool merkle_shape_ok(uint64_t n, uint64_t first, uint32_t depth) {
  if (depth > MERKLE_DEPTH_MAX || first + n < first) return false;
  return depth == 64 || first + n <= (uint64_t)1 << depth;
}
// what the entry points take: the shape, and at most 2^31 - 1 leaves
inline bool merkle_args_in_range(uint64_t n, uint64_t first, uint32_t depth) {
  return merkle_shape_ok(n, first, depth) && n <= (uint64_t)INT32_MAX;
}
inline MerklePlan plan_merkle(uint64_t n, uint64_t first, uint32_t depth, bool keep) {
  if (!merkle_shape_ok(n, first, depth)) throw std::invalid_argument("merkle tree shape");
  MerklePlan p;
  p.n = n; p.first = first; p.depth = depth;
  for (uint32_t h = 0; h <= MERKLE_DEPTH_MAX; ++h) {
    const uint64_t base = merkle_shr(first, h);
    p.lv[h] = {base, n && h <= depth ? merkle_shr(first + n - 1, h) - base + 1 : 0, MERKLE_NONE};
  }
  uint32_t h = 0;
  while (n && h < depth && p.lv[h].count > 1) {
    const uint32_t steps = std::min(MERKLE_TILE_LOG, depth - h);
    const uint64_t tile0 = p.lv[h].base / MERKLE_TILE;
    p.passes.push_back({h, steps, tile0, (p.lv[h].base + p.lv[h].count - 1) / MERKLE_TILE - tile0 + 1});
    h += steps;
    if (!keep) p.lv[h].off = 0;   // marked; offsets below
  }
  p.top = h;
  size_t off = 0;
  for (uint32_t g = 1; g <= depth; ++g) {
    if (!(keep ? n != 0 : p.lv[g].off == 0)) continue;
    p.lv[g].off = off;
    off += 32 * (size_t)p.lv[g].count;
  }
  p.node_bytes = off;
  return p;
}
// the device copy of the level table, then the node slice
struct MerkleWs {
  merkle_level* lv;
  uint8_t* nodes;
};
inline MerkleWs carve_merkle(Bump& b, size_t node_bytes) {
  MerkleWs w;
  w.lv = b.take<merkle_level>(MERKLE_DEPTH_MAX + 1);
  w.nodes = b.take<uint8_t>(node_bytes);
  return w;
}
inline size_t merkle_ws_size(uint64_t n, uint64_t first, uint32_t depth, bool keep) {
  const MerklePlan p = plan_merkle(n, first, depth, keep);
  return carved_bytes([&](Bump& b) { carve_merkle(b, p.node_bytes); });
}
// the kept rows of n leaves wherever the window starts: level h has at most ((n-1) >> h) + 2 real
// nodes (a caller that sizes its workspace before the first index is known: the deposits builder)
inline size_t merkle_node_bound(uint64_t n, uint32_t depth) {
  size_t s = 0;
  for (uint32_t h = 1; n && h <= depth; ++h) s += 32 * (size_t)(merkle_shr(n - 1, h) + 2);
  return s;
}
// depth of merkleize_chunks over n chunks (merkle_minimal.py): ceil(log2 n), 0 for n <= 1
inline uint32_t merkle_chunk_depth(uint64_t n) {
  uint32_t d = 0;
  while (d < 64 && ((uint64_t)1 << d) < n) ++d;
  return d;
}

}  // namespace bls381
