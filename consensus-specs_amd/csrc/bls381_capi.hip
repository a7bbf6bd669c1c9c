// C ABI of the MI355X BLS12-381 engine (include/bls381.h).
//
// Host runtime: one context per device (stream + grow-only workspace), the
// launch pipelines for each entry point, HIP-event kernel accounting for
// bench.py.  No CPU fallback: without a gfx950 device every entry point
// returns BLS381_ENODEV.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <stdexcept>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <type_traits>
#include <vector>

#include "bls381.h"
#include "bls381_kernels.hpp"
#include "bls381_plan.hpp"
#include "bls381_scope.hpp"

using namespace bls381;

namespace {

thread_local std::string t_err;
thread_local int t_device = -1;

// Subgroup policy of the verify paths (bls381_set_subgroup_policy); read when a
// pipeline is queued.  Default: py_ecc 1.7.0's behaviour.
// A thread may override it for its own calls (bls381_set_thread_subgroup_policy).
std::atomic<int> g_policy{BLS381_POLICY_PYECC};
thread_local int t_policy = -1;
int current_policy() { return t_policy >= 0 ? t_policy : g_policy.load(std::memory_order_relaxed); }
int check_subgroups() { return current_policy() == BLS381_POLICY_STRICT ? 1 : 0; }
// decode / aggregation kernel flags (bls381_kernels.hpp CHK_*) for subgroup mode `sub`
// under the current policy: the py_ecc policy decodes with py_ecc 1.7.0's lax codec
// (SURVEY.md A.4), the strict policy with the spec's (bls_signature.md:47-52,58-64)
int policy_flags(int sub) { return sub | (current_policy() == BLS381_POLICY_PYECC ? CHK_LAX : 0); }

// (Streams, Fork, KeepList, Held: bls381_scope.hpp)
struct Ctx {
  int device = -1;
  size_t simds = 0;   // CUs x 4
  Streams q;
  void* ws = nullptr;
  size_t ws_cap = 0;
  std::mutex mu;
  KeepList keep;
  uint8_t* ztab = nullptr;   // the zero nodes Z[0 .. 64] of the Merkle trees (bls381_merkle.hpp), made with the context
  ~Ctx() { streams_destroy(q); }
};
// the SIMD count of the device this thread's last get_ctx selected (256 CUs until then)
thread_local size_t t_simds = 1024;

std::mutex g_mu;
std::vector<Ctx*> g_ctx;

// ---- profiling: per-kernel HIP events on the launch stream
struct ProfEv { const char* name; hipEvent_t a, b; };
std::mutex g_prof_mu;
std::atomic<bool> g_prof_on{false};
std::vector<ProfEv> g_prof_pending;
std::map<std::string, std::pair<long, double>> g_prof_acc;

int fail(const char* what, hipError_t e) {
  t_err = std::string(what) + ": " + hipGetErrorString(e);
  return BLS381_EHIP;
}

#define HIPC(x)                                   \
  do {                                            \
    hipError_t e__ = (x);                         \
    if (e__ != hipSuccess) return fail(#x, e__);  \
  } while (0)

Ctx* get_ctx(int* rc) {
  int dev = t_device;
  if (dev < 0) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0) {
      t_err = "no HIP device";
      *rc = BLS381_ENODEV;
      return nullptr;
    }
    dev = 0;
    t_device = 0;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  if ((int)g_ctx.size() <= dev) g_ctx.resize(dev + 1, nullptr);
  if (!g_ctx[dev]) {
    if (hipSetDevice(dev) != hipSuccess) { t_err = "hipSetDevice failed"; *rc = BLS381_ENODEV; return nullptr; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
      t_err = std::string("device is not gfx950: ") + prop.gcnArchName;
      *rc = BLS381_ENODEV;
      return nullptr;
    }
    std::unique_ptr<Ctx> c(new Ctx());
    c->device = dev;
    c->simds = (size_t)(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256) * 4;
    if (streams_create(c->q) != hipSuccess) { t_err = "stream create failed"; *rc = BLS381_EHIP; return nullptr; }
    uint8_t zeros[MERKLE_ZERO_TABLE_BYTES];
    merkle_zero_table(zeros);
    if (hipMalloc(&c->ztab, sizeof(zeros)) != hipSuccess ||
        hipMemcpy(c->ztab, zeros, sizeof(zeros), hipMemcpyHostToDevice) != hipSuccess) {
      if (c->ztab) (void)hipFree(c->ztab);
      t_err = "zero-node table failed";
      *rc = BLS381_EHIP;
      return nullptr;
    }
    g_ctx[dev] = c.release();
  }
  if (hipSetDevice(dev) != hipSuccess) { t_err = "hipSetDevice failed"; *rc = BLS381_ENODEV; return nullptr; }
  t_simds = g_ctx[dev]->simds;
  *rc = 0;
  return g_ctx[dev];
}

int ensure_ws(Ctx* c, size_t bytes) {
  if (c->ws_cap >= bytes) return 0;
  if (c->ws) { HIPC(hipStreamSynchronize(c->q.main)); HIPC(hipFree(c->ws)); c->ws = nullptr; c->ws_cap = 0; }
  size_t cap = bytes + bytes / 4 + (1 << 20);
  HIPC(hipMalloc(&c->ws, cap));
  c->ws_cap = cap;
  return 0;
}

// Runs an entry point's body (or a rank's local stage of a collective call); exceptions --
// a workspace bound exceeded, an allocation -- become error codes.
template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const std::exception& e) {
    t_err = e.what();
    return BLS381_EARG;
  }
}

// Sizes the context workspace by the caller's own carve: run once over a counting Bump, then,
// with that many bytes ensured, for real.  The carve only takes slices.
template <class Carve>
int carve_ws(Ctx* c, Carve&& carve) {
  if (int rc = ensure_ws(c, carved_bytes(carve))) return rc;
  Bump b(c->ws, c->ws_cap);
  carve(b);
  return 0;
}

// The frame of a host-pointer entry point: the context with its lock held, the context
// workspace carved by the entry, copies in and out on the context stream, one synchronise --
// finish(), or the destructor on every other way out, so the lock is never released with copies
// from or to the caller's buffers still queued.
struct HostCall {
  Ctx* c;
  std::unique_lock<std::mutex> lk;
  hipStream_t s;
  bool finished = false;
  explicit HostCall(Ctx* ctx) : c(ctx), lk(ctx->mu), s(ctx->q.main) {}
  ~HostCall() {
    if (!finished) (void)hipStreamSynchronize(s);
  }
  template <class Carve> int carve(Carve&& cv) { return carve_ws(c, cv); }
  int upload(void* dst, const void* src, size_t bytes) {
    if (bytes) HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  int download(void* dst, const void* src, size_t bytes) {
    if (bytes) HIPC(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    return 0;
  }
  int finish() {
    HIPC(hipStreamSynchronize(s));
    finished = true;
    return 0;
  }
};
// returns a failing step's code from the enclosing function
#define TRY(x)                  \
  do {                          \
    int rc__ = (x);             \
    if (rc__) return rc__;      \
  } while (0)

// device copies of a host-pointer verify batch (bls381_verify_batch[_randomized]) and the
// pipeline's own workspace of ws_bytes
struct VerifyIn {
  uint8_t *pks, *msgs, *sigs, *doms, *v;
  void* ws;
  void carve(Bump& b, size_t n, size_t ws_bytes) {
    pks = b.take<uint8_t>(48 * n);
    msgs = b.take<uint8_t>(32 * n);
    sigs = b.take<uint8_t>(96 * n);
    doms = b.take<uint8_t>(8 * n);
    v = b.take<uint8_t>(n);
    ws = b.take<uint8_t>(ws_bytes);
  }
  int upload(HostCall& hc, size_t n, const uint8_t* h_pks, const uint8_t* h_msgs, const uint8_t* h_sigs,
             const uint8_t* h_doms) {
    TRY(hc.upload(pks, h_pks, 48 * n));
    TRY(hc.upload(msgs, h_msgs, 32 * n));
    TRY(hc.upload(sigs, h_sigs, 96 * n));
    return hc.upload(doms, h_doms, 8 * n);
  }
};

unsigned grid_for(size_t n, int block = KBLOCK) { return (unsigned)((n + block - 1) / block); }

// The clock-based wave balance (bls381_pair.hpp, wave_balance) runs in a launch with no LDS
// allocation; launch() gives every other launch 256 B of dynamic LDS (no kernel reads it) as the
// switch, which the device tests with one s_getreg.  Balanced: launches that put two waves on every
// SIMD, all resident from the start (CUs x 4 SIMDs x 64 < lanes <= CUs x 4 x 2 x 64) -- in a
// longer launch a finished wave's slot takes the next wave, in a smaller one a SIMD holds one --
// outside a NoBalanceScope.  The randomized path opens one: its hash and item Miller loops share
// SIMDs with the signature branch on another stream, which the balance would delay (B = 64:
// 2.59-2.63 M/s with it against 2.70-2.71, profiles/ab_r06o_balance.txt).
thread_local bool g_no_balance = false;
struct NoBalanceScope {
  bool prev;
  NoBalanceScope() : prev(g_no_balance) { g_no_balance = true; }
  ~NoBalanceScope() { g_no_balance = prev; }
};
size_t chip_simds() { return t_simds; }
unsigned balance_lds(dim3 grid, dim3 block) {
  const size_t simds = chip_simds();
  const size_t lanes = (size_t)grid.x * grid.y * grid.z * block.x * block.y * block.z;
  const bool on = !g_no_balance && lanes > simds * 64 && lanes <= simds * 128;
  return on ? 0u : 256u;
}

template <class K, class... A>
int launch(const char* name, hipStream_t s, dim3 grid, dim3 block, K kern, A... args) {
  if (grid.x == 0) return 0;
  ProfEv ev{name, nullptr, nullptr};
  const bool prof = g_prof_on.load(std::memory_order_relaxed);
  if (prof) {
    HIPC(hipEventCreate(&ev.a));
    HIPC(hipEventCreate(&ev.b));
    HIPC(hipEventRecord(ev.a, s));
  }
  hipLaunchKernelGGL(kern, grid, block, balance_lds(grid, block), s, args...);
  HIPC(hipGetLastError());
  if (prof) {
    HIPC(hipEventRecord(ev.b, s));
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_pending.push_back(ev);
  }
  return 0;
}

#define LAUNCH(name, s, grid, block, kern, ...) TRY(launch(name, s, grid, block, kern, __VA_ARGS__))

// final exponentiation + verdict of n Fp12 values (lane-pair SoA): on lane quads while
// the batch leaves SIMDs idle (k_final_exp_verdict_q: half the per-item latency, more
// lane work), on lane pairs above that
#ifndef BLS_FE_QUAD_MAX_N
#define BLS_FE_QUAD_MAX_N 49152
#endif
// final exponentiations of at most this many values run on lane octets (k_final_exp_verdict_oq)
// -- BLS381_FE_OCT=0 keeps them on quads (measurement knob)
#ifndef BLS_FE_OCT_MAX_N
#define BLS_FE_OCT_MAX_N 8192
#endif
// measurement knobs read once from the environment (the defaults are the shipped layout)
int env_knob(const char* name, int def) {
  const char* v = std::getenv(name);
  return v ? std::atoi(v) : def;
}
// BLS381_FE_OCT: 0 = quads (k_final_exp_verdict_q), 2 = octets with the Fp12 products split
// (k_final_exp_verdict_oq<.., 0>), 3 (default) = the compressed squarings split four ways as well
// (k_final_exp_verdict_oq<.., 1>).  (1, the squarings split without the products, measured
// slower than 2 and was removed in r06.)
int fe_oct_mode() {
  static const int m = env_knob("BLS381_FE_OCT", 3);
  return m;
}
bool fe_oct(size_t n) { return fe_oct_mode() && n <= BLS_FE_OCT_MAX_N; }
// The throughput form is k_final_exp_verdict followed by k_final_exp_redo (the exact pass over
// the items whose wave met the compressed squarings' g2 = 0 case; a wave with none exits at once).
// (r04d measured the throughput FE as six launches with HBM intermediates, BLS_FE_SPLIT: 9.99 ms
// per 2^16 against ~9.1 in one kernel; removed in r06)
// vpi: Fp12 values per item (2: the octet Miller path of small verify batches wrote one value per
// pair, and the latency kernels multiply them first; such batches never reach the throughput form)
static_assert(BLS_ML_OCT_MAX_N <= BLS_FE_QUAD_MAX_N, "two values per item only on the latency kernels");
int launch_final_exp(hipStream_t s, size_t n, const uint32_t* f, const uint8_t* st, uint8_t* verdicts, int vpi = 1) {
  const dim3 b(KBLOCK);
  const bool two = vpi == 2;
  if (fe_oct(n) && fe_oct_mode() == 3)
    LAUNCH("final_exp_oo", s, dim3(grid_for(8 * n)), b, (two ? k_final_exp_verdict_oq<2, 1> : k_final_exp_verdict_oq<1, 1>),
           n, f, st, verdicts);
  else if (fe_oct(n) && fe_oct_mode() == 2)
    LAUNCH("final_exp_oq", s, dim3(grid_for(8 * n)), b, (two ? k_final_exp_verdict_oq<2> : k_final_exp_verdict_oq<1>), n, f,
           st, verdicts);
  else if (two || n <= BLS_FE_QUAD_MAX_N)
    LAUNCH("final_exp_q", s, dim3(grid_for(4 * n)), b, (two ? k_final_exp_verdict_q<2> : k_final_exp_verdict_q<1>), n, f, st,
           verdicts);
  else {
    LAUNCH("final_exp", s, dim3(grid_for(2 * n)), b, k_final_exp_verdict, n, f, st, verdicts);
    LAUNCH("final_exp_redo", s, dim3(grid_for(2 * n)), b, k_final_exp_redo, n, f, verdicts);
  }
  return 0;
}
#define LAUNCH_FE(s, n, f, st, v) TRY(launch_final_exp(s, n, (const uint32_t*)(f), (const uint8_t*)(st), v))

// ----------------------------------------------------- verify_batch (C2) --
// (VerifyWs, its carve and the Miller-stage thresholds: bls381_plan.hpp)
// hash_to_G2 of batches of at most this many messages runs the wide candidate search first
// (k_hash_search: 16 lanes per message, one Legendre symbol each)
#ifndef BLS_HASH_WIDE_MAX_N
#define BLS_HASH_WIDE_MAX_N 8192
#endif
// with the search offsets known, up to this many messages the cofactor map runs on lane octets or
// quads (k_hash_g2_lg, its independent products two at a time), above on lane pairs
#ifndef BLS_HASH_QUAD_MAX_N
#define BLS_HASH_QUAD_MAX_N 8192
#endif
// BLS381_ML_OCTET (default 1): the latency Miller loops run one octet per Miller pair
// (k_miller_verify_lg<on_octet>, k_miller_tasks<8>: 10 product steps per doubling iteration against 19
// on a quad); 0 = one quad per pair (k_miller_verify_lg<on_quad>, k_miller_tasks<4>)
int ml_octet() {
  static const int v = env_knob("BLS381_ML_OCTET", 1);
  return v;
}
// hash_to_G2 of n messages (throughput form, no precomputed search offsets) into h_aff, status
// into st (may be null): k_hash_cand_1 (search + root, one lane per item), then k_hash_bp (cofactor
// map, lane pairs)
int launch_hash_g2(hipStream_t s, size_t n, const uint8_t* msgs, uint32_t mlen, const uint8_t* doms, int dom_stride,
                   uint32_t* h_aff, uint8_t* st) {
  LAUNCH("hash_cand", s, dim3(grid_for(n)), dim3(KBLOCK), k_hash_cand_1, n, msgs, mlen, doms, dom_stride, h_aff);
  LAUNCH("hash_bp", s, dim3(grid_for(2 * n)), dim3(KBLOCK), k_hash_bp, n, h_aff, st);
  return 0;
}
// hash_to_G2 with the search offsets known (koff from k_hash_search, or nullptr): the latency
// batches.  BLS381_HASH_OCT (default 1): the doublings on octets (k_hash_g2_lg<on_octet>), 0 = on quads.
int launch_hash_koff(hipStream_t s, size_t n, const uint8_t* msgs, uint32_t mlen, const uint8_t* doms, int dom_stride,
                     uint32_t* h_aff, uint8_t* st, const uint32_t* koff, int prio) {
  static const int oct = env_knob("BLS381_HASH_OCT", 1);
  if (n <= BLS_HASH_QUAD_MAX_N && oct)
    LAUNCH("hash_to_g2_o", s, dim3(grid_for(8 * n)), dim3(KBLOCK), k_hash_g2_lg<on_octet>, n, msgs, mlen, doms, dom_stride, h_aff,
           st, koff, prio);
  else if (n <= BLS_HASH_QUAD_MAX_N)
    LAUNCH("hash_to_g2_q", s, dim3(grid_for(4 * n)), dim3(KBLOCK), k_hash_g2_lg<on_quad>, n, msgs, mlen, doms, dom_stride, h_aff,
           st, koff, prio);
  else
    LAUNCH("hash_to_g2", s, dim3(grid_for(2 * n)), dim3(KBLOCK), k_hash_g2, n, msgs, mlen, doms, dom_stride, h_aff,
           st, koff, prio);
  return 0;
}

int run_verify_pairings(size_t n, const VerifyWs& w, uint8_t* verdicts, hipStream_t s, bool sig_in_loop);

// Decodes and hash_to_G2 of a verify batch, then its pairings.  Three schedules (measured in
// DESIGN.md §10): the one-lane stages (hash search + root, decode_g1, decode_g2) share the chip,
// the full-chip cofactor map runs alone.
int run_verify_batch(Ctx* c, size_t n, const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs,
                     const uint8_t* doms, uint8_t* verdicts, void* ws, hipStream_t s) {
  VerifyWs w = carve_verify(ws, n);
  const dim3 g(grid_for(n)), g2(grid_for(2 * n)), b(KBLOCK);   // G1: lane per item; G2/Fp12: lane pair
  const int chk = check_subgroups();
  // throughput path under the strict policy: the signature's G2 test moves from decode_g2 into
  // the Miller loop, which computes [|x|] sig anyway (k_ml_lines' sig_check)
  const bool sig_in_loop = chk && n > BLS_ML_QUAD_MAX_N;
  const int pk_flags = policy_flags(chk), sig_flags = policy_flags(sig_in_loop ? 0 : chk);
  const bool wide = n <= BLS_HASH_WIDE_MAX_N;
  Fork fk(c->q, s);
  if (!chk && !wide) {
    // py_ecc, throughput: the three one-lane stages as ONE launch whose workgroups take the three
    // roles in dispatch order, the hash search first (k_prologue_1); then the cofactor map
    LAUNCH("prologue", s, dim3(3 * grid_for(n)), b, k_prologue_1<0>, n, pks, sigs, msgs, (uint32_t)32, doms, 8,
           (const uint8_t*)nullptr, w.pk_aff, w.pk_st, w.sig_aff, w.sig_st, w.h_aff, (uint32_t*)nullptr,
           (uint8_t*)nullptr, pk_flags, sig_flags);
    LAUNCH("hash_bp", s, g2, b, k_hash_bp, n, w.h_aff, (uint8_t*)nullptr);
    return run_verify_pairings(n, w, verdicts, s, sig_in_loop);
  }
  HIPC(fk.branch(c->q.side));
  LAUNCH("decode_g1", c->q.side.stream, g, b, k_decode_g1, n, pks, w.pk_aff, w.pk_st, pk_flags);
  if (!chk) {
    // py_ecc, small batches: decode_g2 on a second side stream, and the wide search first (16
    // candidates per message in one round), so the hash does not wait for the batch's slowest
    // sequential search
    HIPC(fk.branch(c->q.side2));
    LAUNCH("decode_g2_1", c->q.side2.stream, g, b, k_decode_g2_1, n, sigs, w.sig_aff, w.sig_st, sig_flags);
    LAUNCH("hash_search", s, dim3(grid_for(16 * n)), b, k_hash_search<16>, n, msgs, (uint32_t)32, doms, 8, w.koff);
    TRY(launch_hash_koff(s, n, msgs, 32u, doms, 8, w.h_aff, (uint8_t*)nullptr, (const uint32_t*)w.koff, 0));
    HIPC(fk.join());
    return run_verify_pairings(n, w, verdicts, s, sig_in_loop);
  }
  // strict: both decodes in sequence on the side stream beside hash_to_G2 (decode_g1 carries the G1
  // subgroup test, and waiting for it before the cofactor map costs more than sharing the chip)
  LAUNCH("decode_g2_1", c->q.side.stream, g, b, k_decode_g2_1, n, sigs, w.sig_aff, w.sig_st, sig_flags);
  if (wide) {
    LAUNCH("hash_search", s, dim3(grid_for(16 * n)), b, k_hash_search<16>, n, msgs, (uint32_t)32, doms, 8, w.koff);
    TRY(launch_hash_koff(s, n, msgs, 32u, doms, 8, w.h_aff, (uint8_t*)nullptr, (const uint32_t*)w.koff, 0));
  } else {
    TRY(launch_hash_g2(s, n, msgs, 32u, doms, 8, w.h_aff, (uint8_t*)nullptr));
  }
  HIPC(fk.join());
  return run_verify_pairings(n, w, verdicts, s, sig_in_loop);
}

// The verify batch after its decodes and hash: Miller loops and final exponentiation over
// the decoded points in `w` (statuses pk_st / sig_st, hash points h_aff), verdicts out.
// sig_in_loop: the strict policy's G2 test of the signatures is still to be done (in the loop).
int run_verify_pairings(size_t n, const VerifyWs& w, uint8_t* verdicts, hipStream_t s, bool sig_in_loop) {
  const dim3 b(KBLOCK);
  if (n <= BLS_ML_OCT_MAX_N) {
    // lowest latency: one octet (or quad) per Miller pair; the FE multiplies the two values of each item
    if (ml_octet())
      LAUNCH("miller_loop_2oo", s, dim3(grid_for(16 * n)), b, k_miller_verify_lg<on_octet>, n, (const uint32_t*)w.sig_aff,
             (const uint8_t*)w.sig_st, (const uint32_t*)w.pk_aff, (const uint8_t*)w.pk_st, (const uint32_t*)w.h_aff,
             w.f, w.f_st);
    else
      LAUNCH("miller_loop_2o", s, dim3(grid_for(8 * n)), b, k_miller_verify_lg<on_quad>, n, (const uint32_t*)w.sig_aff,
             (const uint8_t*)w.sig_st, (const uint32_t*)w.pk_aff, (const uint8_t*)w.pk_st, (const uint32_t*)w.h_aff,
             w.f, w.f_st);
    return launch_final_exp(s, n, w.f, w.f_st, verdicts, 2);
  }
  if (n <= BLS_ML_QUAD_MAX_N) {
    // latency path: one item per lane quad, its two pairs side by side (half the per-item latency,
    // ~13% more work per item -- the better trade while the batch leaves SIMDs idle)
    LAUNCH("miller_loop_2q", s, dim3(grid_for(4 * n)), b, k_miller_verify_q, n, (const uint32_t*)w.sig_aff,
           (const uint8_t*)w.sig_st, (const uint32_t*)w.pk_aff, (const uint8_t*)w.pk_st, (const uint32_t*)w.h_aff,
           w.f, w.f_st);
  } else {
    // the split Miller loop, in chunks: running points and line products on quads, then the
    // f accumulation on lane pairs
    const size_t ch = verify_split_chunk(n);
    for (size_t i0 = 0; i0 < n; i0 += ch) {
      const size_t cnt = std::min(ch, n - i0);
      // the line loop in launches of at most one round of two-wave slots on quads (CUs x 4 x 32
      // items), each balanced by the clock when it fills the chip (its static LDS keeps the generic
      // switch off; the launch passes it instead)
      const size_t part = chip_simds() * 32;
      for (size_t l0 = 0; l0 < cnt; l0 += part) {
        const size_t lc = std::min(part, cnt - l0);
        const int bal = (!g_no_balance && 4 * lc > chip_simds() * 64) ? 1 : 0;
        LAUNCH("miller_lines", s, dim3(grid_for(4 * lc)), b, k_ml_lines, n, i0, cnt, (const uint32_t*)w.sig_aff,
               (const uint8_t*)w.sig_st, (const uint32_t*)w.pk_aff, (const uint8_t*)w.pk_st, (const uint32_t*)w.h_aff,
               w.ml_L, w.ml_st, sig_in_loop ? 1 : 0, l0, lc, bal);
      }
      // (r05: the accumulation on lane quads, k_ml_accum_q, measured 8.09-8.18 against 6.96-7.00 ms)
      LAUNCH("miller_accum", s, dim3(grid_for(2 * cnt)), b, k_ml_accum, n, i0, cnt, (const uint32_t*)w.ml_L,
             (const uint8_t*)w.ml_st, w.f, w.f_st, (size_t)0);
    }
  }
  return launch_final_exp(s, n, w.f, w.f_st, verdicts);
}

// --------------------------------------------------------- aggregation --
// (the chunk plan, AggPlan / plan_agg, and its workspace size: bls381_plan.hpp)

// runs the plan; returns device pointers to the final per-group Jacobian sums / bad flags.
// Level 0 decodes compressed points (d_in), reads registry entries (reg), or -- with
// jac_in -- sums Jacobian SoA points (n_jac_in of them, bad flags bad_in).
template <class F>
int run_agg(const AggPlan& p, size_t ng, const uint8_t* d_in, void* ws, hipStream_t s,
            const uint32_t** out_jac, const uint8_t** out_bad, size_t* used, size_t cap = SIZE_MAX,
            const agg_reg_src* reg = nullptr, int check = 0, const uint32_t* jac_in = nullptr,
            const uint8_t* bad_in = nullptr, size_t n_jac_in = 0) {
  Bump b(ws, cap);
  const uint32_t* prev_jac = jac_in;
  const uint8_t* prev_bad = bad_in;
  size_t prev_n = n_jac_in;
  for (size_t l = 0; l < p.levels.size(); ++l) {
    const auto& lv = p.levels[l];
    agg_chunk* d_chunks = b.take<agg_chunk>(lv.size());
    uint32_t* jac = b.take<uint32_t>(lv.size() * soa_jac<F>::NC * FP_LIMBS);
    uint8_t* bad = b.take<uint8_t>(lv.size());
    HIPC(hipMemcpyAsync(d_chunks, lv.data(), lv.size() * sizeof(agg_chunk), hipMemcpyHostToDevice, s));
    const agg_reg_src none{nullptr, nullptr, nullptr, 0, 0};
    size_t n_in_total = 0;
    for (const auto& ch : lv) n_in_total += ch.end - ch.begin;
    const bool lanes = std::is_same<F, fp_t>::value && l == 0 && !jac_in && n_in_total < AGG_LANE_AVG_MAX * lv.size();
    if (l > 0 || jac_in) {
      LAUNCH("agg_sum", s, dim3((unsigned)lv.size()), dim3(KBLOCK), (k_agg_chunks<F, AGG_JAC>), (size_t)lv.size(),
             (const agg_chunk*)d_chunks, (const uint8_t*)nullptr, prev_jac, prev_n, prev_bad, jac, bad, none, 0);
    } else if (lanes) {
      LAUNCH("agg_lane_sum", s, dim3(grid_for(lv.size())), dim3(KBLOCK), k_agg_lanes<AGG_REGISTRY>, (size_t)lv.size(),
             (const agg_chunk*)d_chunks, d_in, jac, bad, reg ? *reg : none, check);
    } else if (l == 0 && reg) {
      LAUNCH("agg_registry_sum", s, dim3((unsigned)lv.size()), dim3(KBLOCK), (k_agg_chunks<F, AGG_REGISTRY>),
             (size_t)lv.size(), (const agg_chunk*)d_chunks, d_in, (const uint32_t*)nullptr, (size_t)0,
             (const uint8_t*)nullptr, jac, bad, *reg, check);
    } else {
      LAUNCH("agg_decode_sum", s, dim3((unsigned)lv.size()), dim3(KBLOCK), (k_agg_chunks<F, AGG_BYTES>), (size_t)lv.size(),
             (const agg_chunk*)d_chunks, d_in, (const uint32_t*)nullptr, (size_t)0, (const uint8_t*)nullptr, jac, bad,
             none, check);
    }
    prev_jac = jac;
    prev_bad = bad;
    prev_n = lv.size();
  }
  (void)ng;
  *out_jac = prev_jac;
  *out_bad = prev_bad;
  *used = b.off;
  return 0;
}

// ------------------------------------------------- verify_multiple pieces --
// (the host plan of a batch, VmPlan / plan_vm / plan_vm_grouped, and the segmented product
// passes, plan_products: bls381_plan.hpp)

// Each lane quad runs (up to) two pairs of one call, one per half (bls381_quad.hpp).
// A half's pair is idle for PAIR_NONE or an infinite operand (py_ecc: pairing 1);
// any undecodable / bad operand makes the quad BAD; so does a degenerate loop.
__global__ void __launch_bounds__(KBLOCK, BLS_ML_WAVES_PER_EU) k_miller_quads(size_t nq, const int32_t* __restrict__ quad_pair,
                                                        size_t G, const uint32_t* __restrict__ h_aff,
                                                        const uint8_t* __restrict__ h_st,
                                                        const uint32_t* __restrict__ agg_aff,
                                                        const uint8_t* __restrict__ agg_st, size_t ncalls,
                                                        const uint32_t* __restrict__ sig_aff,
                                                        const uint8_t* __restrict__ sig_st,
                                                        const uint32_t* __restrict__ slot, size_t nslots,
                                                        uint32_t* __restrict__ f_out, uint8_t* __restrict__ st_out) {
  const size_t q = item_index<4>();
  if (q >= nq) return;
  const size_t o = slot ? slot[q] : q;   // output slot (stride nslots)
  const bool hi = qd_hi();
  const bool lead = (threadIdx.x & 3u) == 0;
  const int p = pr_odd() ? 1 : 0;
  auto status = [&](int32_t src, bool& bad) -> bool {   // active?
    uint8_t sq = ST_INF, sp = ST_INF;
    if (src >= 0) { sq = h_st[src]; sp = agg_st[src]; }
    else if (src != PAIR_NONE) { sq = sig_st[(size_t)(-src - 1)]; sp = ST_OK; }
    bad = sq == ST_BAD || sp == ST_BAD;
    return sq == ST_OK && sp == ST_OK;
  };
  const int32_t mine = quad_pair[2 * q + (hi ? 1 : 0)], other = quad_pair[2 * q + (hi ? 0 : 1)];
  bool bad_m, bad_o;
  const bool act_m = status(mine, bad_m), act_o = status(other, bad_o);
  if (bad_m || bad_o) { if (lead) st_out[o] = ST_BAD; return; }   // same on all four lanes
  aff_t<fp2p_t> Q;
  aff_t<fp_t> P;
  if (act_m || act_o) {
    // an idle half runs a copy of the active half's operands with its lines masked to 1
    const int32_t src = act_m ? mine : other;
    if (src >= 0) {
      Q.x = pr_make(soa_ld(h_aff, 2 * G, 2 * (size_t)src + p, 0));
      Q.y = pr_make(soa_ld(h_aff, 2 * G, 2 * (size_t)src + p, 1));
      P = soa_ld_g1(agg_aff, G, (size_t)src);
    } else {
      const size_t c = (size_t)(-src - 1);
      Q.x = pr_make(soa_ld(sig_aff, 2 * ncalls, 2 * c + p, 0));
      Q.y = pr_make(soa_ld(sig_aff, 2 * ncalls, 2 * c + p, 1));
      P.x = G1_VGEN_X_M; P.y = G1_VGEN_NEGY_M;
    }
  }
  miller_quad_store(act_m || act_o, Q, P, act_m, true, lead, f_out, st_out, nslots, o);
}

// The latency form of k_miller_quads: pair task t (entry t of quad_pair) on lane group t
// (miller_pair_store, bls381_kernels.hpp: every step's products split over the group).  Writes one
// Fp12 (pair SoA over nt values) and status per task: PAIR_NONE or an infinite
// operand is f = 1; a bad operand or a degenerate loop is ST_BAD.
// LPI = 4: one quad per pair task; LPI = 8: one octet per task (quad A stores)
template <int LPI>
__global__ void __launch_bounds__(KBLOCK, BLS_ML_WAVES_PER_EU) k_miller_tasks(size_t nt, const int32_t* __restrict__ tasks,
                                                           size_t G, const uint32_t* __restrict__ h_aff,
                                                           const uint8_t* __restrict__ h_st,
                                                           const uint32_t* __restrict__ agg_aff,
                                                           const uint8_t* __restrict__ agg_st, size_t ncalls,
                                                           const uint32_t* __restrict__ sig_aff,
                                                           const uint8_t* __restrict__ sig_st,
                                                           const uint32_t* __restrict__ slot, size_t nslots,
                                                           uint32_t* __restrict__ f_out, uint8_t* __restrict__ st_out) {
  static_assert(LPI == 4 || LPI == 8, "quad or octet tasks");
  using LG = std::conditional_t<LPI == 8, on_octet, on_quad>;
  size_t t;
  bool live;
  if (!lat_unit<LPI>(nt, t, live)) return;
  const bool lead = (threadIdx.x & (LPI - 1u)) == 0 && live;
  const int32_t src = tasks[t];
  const size_t o = slot ? slot[t] : t;   // output slot (stride nslots)
  uint8_t sq = ST_INF, sp = ST_INF;
  if (src >= 0) { sq = h_st[src]; sp = agg_st[src]; }
  else if (src != PAIR_NONE) { sq = sig_st[(size_t)(-src - 1)]; sp = ST_OK; }
  if (sq == ST_BAD || sp == ST_BAD) { if (lead) st_out[o] = ST_BAD; return; }
  // group src >= 0: (H of the group, its aggregate key); else call ~src = -src - 1: (its signature, -[c] g1)
  const bool grp = src >= 0;
  miller_pair_store<LG>(sq == ST_OK && sp == ST_OK, grp ? h_aff : sig_aff, grp ? agg_aff : nullptr, grp ? G : ncalls,
                        (size_t)(grp ? src : ~src), live, lead, f_out, st_out, nslots, o);
}

// each lane multiplies one chunk [begin, end) of Fp12 values (statuses OR-ed);
// an empty chunk yields 1 (the empty product of an empty call)
__global__ void __launch_bounds__(KBLOCK, BLS_WAVES_PER_EU) k_fp12_chunk_product(size_t nchunks, const agg_chunk* __restrict__ chunks,
                                                              const uint32_t* __restrict__ in, size_t n_in,
                                                              const uint8_t* __restrict__ in_st,
                                                              uint32_t* __restrict__ out, uint8_t* __restrict__ out_st) {
  const size_t c = item_index<2>();
  if (c >= nchunks) return;
  const agg_chunk ch = chunks[c];
  fp12p_t a = fp12_one<fp2p_t>();
  uint8_t st = ST_OK;
  for (uint32_t e = ch.begin; e < ch.end; ++e) {
    a = (e == ch.begin) ? soa_ld12(in, n_in, e) : fp12_mul(a, soa_ld12(in, n_in, e));
    if (in_st[e] != ST_OK) st = ST_BAD;
  }
  soa_st12(out, nchunks, c, a);
  if (!pr_odd()) out_st[c] = st;
}

// Queues the segmented product passes over the n_in values f / st; f and st become the last
// pass's outputs (one value per segment).  The chunk lists are async-copy sources: the caller
// keeps `passes` alive until the stream has passed them.
int run_product_passes(Bump& b, hipStream_t s, const ProductPasses& passes, uint32_t*& f, uint8_t*& st, size_t n_in) {
  for (const auto& chunks : passes) {
    agg_chunk* d_ch = b.take<agg_chunk>(chunks.size());
    uint32_t* nf = b.take<uint32_t>(12 * FP_LIMBS * chunks.size());
    uint8_t* nst = b.take<uint8_t>(chunks.size());
    HIPC(hipMemcpyAsync(d_ch, chunks.data(), chunks.size() * sizeof(agg_chunk), hipMemcpyHostToDevice, s));
    LAUNCH("fp12_product", s, dim3(grid_for(2 * chunks.size())), dim3(KBLOCK), k_fp12_chunk_product, chunks.size(),
           (const agg_chunk*)d_ch, (const uint32_t*)f, n_in, (const uint8_t*)st, nf, nst);
    f = nf;
    st = nst;
    n_in = chunks.size();
  }
  return 0;
}

// rows idx[k] of `src` (row_bytes each) -> dst row k
__global__ void __launch_bounds__(KBLOCK) k_gather_rows(size_t n, const uint32_t* __restrict__ idx,
                                                        const uint8_t* __restrict__ src, uint32_t row_bytes,
                                                        uint8_t* __restrict__ dst) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * row_bytes) return;
  const size_t k = t / row_bytes, b = t % row_bytes;
  dst[t] = src[(size_t)idx[k] * row_bytes + b];
}

// items idx[k] of SoA arrays with `rows` rows of n*e words (e words per item: 1 for G1
// coordinates, 2 for the lane-pair G2 layout) -> item k of the same layout over m items
__global__ void __launch_bounds__(KBLOCK) k_gather_soa(size_t m, const uint32_t* __restrict__ idx,
                                                       const uint32_t* __restrict__ src, size_t n, uint32_t rows,
                                                       uint32_t e, uint32_t* __restrict__ dst) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * e * rows) return;
  const size_t r = t / (m * e), ke = t % (m * e), k = ke / e, j = ke % e;
  dst[t] = src[r * n * e + (size_t)idx[k] * e + j];
}
// statuses of the gathered items; a signature outside G2 that decoded (ST_NOSUB, py_ecc
// policy) is an ordinary point to the per-item loops, as in the default decode
__global__ void __launch_bounds__(KBLOCK) k_gather_st(size_t m, const uint32_t* __restrict__ idx,
                                                      const uint8_t* __restrict__ pk_st,
                                                      const uint8_t* __restrict__ sig_st,
                                                      uint8_t* __restrict__ pk_out, uint8_t* __restrict__ sig_out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const size_t i = idx[k];
  pk_out[k] = pk_st[i];
  const uint8_t ss = sig_st[i];
  sig_out[k] = ss == ST_NOSUB ? ST_OK : ss;
}

// Runs a planned batch up to (and excluding) the final exponentiation: keys,
// signatures and domains are device buffers (d_pks indexed by the caller's key
// numbering); the plan's own arrays are copied here.  Returns per-call Fp12
// products and statuses (SoA over n_calls) on the device.
// reg != nullptr: the member keys are registry entries (d_pks holds one int32 entry per key,
// 4 bytes, numbered like the keys), summed from the registry's decoded points.
int run_vm_batch(Ctx* c, const VmPlan& pl, size_t mlen, const uint8_t* d_pks, const uint8_t* d_sigs,
                 const uint8_t* d_doms, Bump& b, hipStream_t s, uint32_t** out_f, uint8_t** out_st,
                 const agg_reg_src* reg = nullptr) {
  const size_t G = pl.G, ncalls = pl.n_calls, nq = pl.nquads;
  const int chk = check_subgroups();   // STRICT: every member key and signature is checked
  uint32_t* d_kidx = b.take<uint32_t>(pl.key_idx.size() + 1);
  uint8_t* d_gmsg = b.take<uint8_t>(pl.group_msg.size() + 1);
  uint32_t* d_gcall = b.take<uint32_t>(G + 1);
  uint8_t* d_gdom = b.take<uint8_t>(8 * G + 1);
  uint8_t* d_gpks = b.take<uint8_t>(48 * pl.key_idx.size() + 1);
  int32_t* d_qp = b.take<int32_t>(2 * nq);
  if (!pl.key_idx.empty())
    HIPC(hipMemcpyAsync(d_kidx, pl.key_idx.data(), 4 * pl.key_idx.size(), hipMemcpyHostToDevice, s));
  if (G) {
    HIPC(hipMemcpyAsync(d_gmsg, pl.group_msg.data(), pl.group_msg.size(), hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_gcall, pl.group_call.data(), 4 * G, hipMemcpyHostToDevice, s));
  }
  HIPC(hipMemcpyAsync(d_qp, pl.quad_pair.data(), 8 * nq, hipMemcpyHostToDevice, s));
  uint32_t* agg_aff = b.take<uint32_t>(2 * FP_LIMBS * (G + 1));
  uint8_t* agg_st = b.take<uint8_t>(G + 1);
  uint32_t* h_aff = b.take<uint32_t>(4 * FP_LIMBS * (G + 1));
  uint8_t* h_st = b.take<uint8_t>(G + 1);
  uint32_t* d_koff = b.take<uint32_t>(G + 1);
  uint32_t* sig_aff = b.take<uint32_t>(4 * FP_LIMBS * ncalls);
  uint8_t* sig_st = b.take<uint8_t>(ncalls);
  // Miller values: one per pair task (small batches), or the quads' and the signatures' slots
  const size_t nf = pl.tasks ? 2 * nq : pl.nslots;
  uint32_t* f = b.take<uint32_t>(12 * FP_LIMBS * nf);
  uint8_t* st = b.take<uint8_t>(nf);
  uint32_t *d_qslot = nullptr, *d_sslot = nullptr;
  int32_t* d_stask = nullptr;
  if (!pl.tasks) {
    d_qslot = b.take<uint32_t>(nq + 1);
    d_sslot = b.take<uint32_t>(ncalls);
    d_stask = b.take<int32_t>(ncalls);
    if (nq) HIPC(hipMemcpyAsync(d_qslot, pl.quad_slot.data(), 4 * nq, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_sslot, pl.sig_slot.data(), 4 * ncalls, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(d_stask, pl.sig_task.data(), 4 * ncalls, hipMemcpyHostToDevice, s));
  }
  // Small batches (an epoch's attestations, one custody call) leave most of the
  // GPU idle, so the independent stages overlap: the pubkey-group sums and the
  // signature decodes run on the side stream while the main stream hashes the
  // messages; the Miller loops wait for both.
  {
    Fork fk(c->q, s);
    hipStream_t side = c->q.side.stream, side2 = c->q.side2.stream;
    HIPC(fk.branch(c->q.side));
    if (G > 0) {
      // members in group order, then group sums -> affine
      const size_t nk = pl.key_idx.size();
      const uint32_t row = reg ? 4u : 48u;   // registry entries or compressed keys
      if (nk) LAUNCH("gather_pubkeys", side, dim3(grid_for(row * nk)), dim3(KBLOCK), k_gather_rows, nk,
                     (const uint32_t*)d_kidx, d_pks, row, d_gpks);
      const uint32_t* jac;
      const uint8_t* bad;
      size_t used = 0;
      uint8_t* sub = b.take<uint8_t>(0);
      agg_reg_src rs{};
      if (reg) { rs = *reg; rs.entry = (const int32_t*)d_gpks; }
      int rc = run_agg<fp_t>(pl.agg, G, reg ? nullptr : d_gpks, sub, side, &jac, &bad, &used, b.left(),
                             reg ? &rs : nullptr, policy_flags(chk));
      if (rc) return rc;
      b.off += used;
      LAUNCH("agg_g1_affine", side, dim3(grid_for(G)), dim3(KBLOCK), k_agg_g1_affine, G, jac, bad, agg_aff, agg_st);
    }
    // the signature decodes on a second side stream: for an epoch of attestations the group
    // sums and the decodes are each about as long as the hash, so in sequence they would
    // outlast it
    HIPC(fk.branch(c->q.side2));
    LAUNCH("decode_g2", side2, dim3(grid_for(2 * ncalls)), dim3(KBLOCK), k_decode_g2, ncalls, d_sigs, sig_aff,
           sig_st, policy_flags(chk));
    if (!pl.tasks) {
      // large batches: the signature pairs run here, beside hash_to_G2, so the group pairs fill
      // whole quads and the main Miller launch has no partial last round of waves
      LAUNCH("miller_sig_tasks", side2, dim3(grid_for(4 * ncalls)), dim3(KBLOCK), k_miller_tasks<4>, ncalls,
             (const int32_t*)d_stask, G, (const uint32_t*)h_aff, (const uint8_t*)h_st, (const uint32_t*)agg_aff,
             (const uint8_t*)agg_st, ncalls, (const uint32_t*)sig_aff, (const uint8_t*)sig_st,
             (const uint32_t*)d_sslot, nf, f, st);
    }
    if (G > 0) {
      LAUNCH("gather_domains", s, dim3(grid_for(8 * G)), dim3(KBLOCK), k_gather_rows, G, (const uint32_t*)d_gcall,
             d_doms, 8u, d_gdom);
      const bool wide = pl.tasks && G <= BLS_HASH_WIDE_MAX_N;
      if (wide)
        LAUNCH("hash_search", s, dim3(grid_for(16 * G)), dim3(KBLOCK), k_hash_search<16>, G, (const uint8_t*)d_gmsg,
               (uint32_t)mlen, (const uint8_t*)d_gdom, 8, d_koff);
      if (!wide && !pl.tasks)
        TRY(launch_hash_g2(s, G, (const uint8_t*)d_gmsg, (uint32_t)mlen, (const uint8_t*)d_gdom, 8, h_aff, h_st));
      else if (int rc_h = launch_hash_koff(s, G, (const uint8_t*)d_gmsg, (uint32_t)mlen, (const uint8_t*)d_gdom, 8,
                                           h_aff, h_st, (const uint32_t*)(wide ? d_koff : nullptr), pl.tasks ? 1 : 0))
        return rc_h;
    }
    HIPC(fk.join());
  }
  if (pl.tasks) {
    // one octet per pair task while the tasks fit one wave per SIMD, else (or BLS381_ML_OCTET=0) one quad
    const bool oct = ml_octet() && nf <= 8192;
    LAUNCH(oct ? "miller_tasks_o1" : "miller_tasks_q1", s, dim3(grid_for((oct ? 8 : 4) * nf)), dim3(KBLOCK),
           (oct ? k_miller_tasks<8> : k_miller_tasks<4>), nf, (const int32_t*)d_qp, G, (const uint32_t*)h_aff,
           (const uint8_t*)h_st, (const uint32_t*)agg_aff, (const uint8_t*)agg_st, ncalls, (const uint32_t*)sig_aff,
           (const uint8_t*)sig_st, (const uint32_t*)nullptr, nf, f, st);
  } else {
    LAUNCH("miller_quads", s, dim3(grid_for(4 * nq)), dim3(KBLOCK), k_miller_quads, nq, (const int32_t*)d_qp, G,
           (const uint32_t*)h_aff, (const uint8_t*)h_st, (const uint32_t*)agg_aff, (const uint8_t*)agg_st, ncalls,
           (const uint32_t*)sig_aff, (const uint8_t*)sig_st, (const uint32_t*)d_qslot, nf, f, st);
  }
  // segmented products (chunk lists live in the plan, which outlives the stream work)
  TRY(run_product_passes(b, s, pl.product_passes(), f, st, nf));
  *out_f = f;
  *out_st = st;
  return 0;
}

}  // namespace

// ====================================================================== ABI
extern "C" {

int bls381_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}

int bls381_init(int device) {
  int cnt = bls381_device_count();
  if (cnt <= 0) { t_err = "no HIP device"; return BLS381_ENODEV; }
  if (device < 0 || device >= cnt) { t_err = "device ordinal out of range"; return BLS381_EARG; }
  t_device = device;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  return c ? 0 : rc;
}

int bls381_init_devices(int n_devices) {
  const int cnt = bls381_device_count();
  if (cnt <= 0) { t_err = "no HIP device"; return BLS381_ENODEV; }
  if (n_devices < 1 || n_devices > cnt) { t_err = "device count out of range"; return BLS381_EARG; }
  const int keep = t_device;
  for (int d = n_devices - 1; d >= 0; --d) {
    const int rc = bls381_init(d);
    if (rc) return rc;
  }
  return keep >= 0 && keep < n_devices ? bls381_init(keep) : 0;   // device 0 stays selected otherwise
}

void bls381_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (Ctx* c : g_ctx) {
    if (!c) continue;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->q.main);
    (void)hipDeviceSynchronize();
    keep_clear(c->keep);
    if (c->ws) (void)hipFree(c->ws);
    if (c->ztab) (void)hipFree(c->ztab);
    delete c;
  }
  g_ctx.clear();
}

const char* bls381_last_error(void) { return t_err.c_str(); }

int bls381_set_subgroup_policy(int policy) {
  if (policy != BLS381_POLICY_PYECC && policy != BLS381_POLICY_STRICT) return BLS381_EARG;
  g_policy.store(policy, std::memory_order_relaxed);
  return 0;
}

int bls381_get_subgroup_policy(void) { return g_policy.load(std::memory_order_relaxed); }

int bls381_set_thread_subgroup_policy(int policy) {
  if (policy != -1 && policy != BLS381_POLICY_PYECC && policy != BLS381_POLICY_STRICT) return BLS381_EARG;
  t_policy = policy;
  return 0;
}

int bls381_get_thread_subgroup_policy(void) { return current_policy(); }

int bls381_profile_enable(int on) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof_on.store(on != 0, std::memory_order_relaxed);
  g_prof_acc.clear();
  for (auto& e : g_prof_pending) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  g_prof_pending.clear();
  return 0;
}

int bls381_profile_read(char* out, size_t cap) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (auto& e : g_prof_pending) {
    float ms = 0;
    if (hipEventSynchronize(e.b) != hipSuccess) return BLS381_EHIP;
    if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return BLS381_EHIP;
    auto& acc = g_prof_acc[e.name];
    acc.first += 1;
    acc.second += ms;
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  g_prof_pending.clear();
  std::string js = "{";
  bool first = true;
  for (auto& kv : g_prof_acc) {
    char buf[256];
    std::snprintf(buf, sizeof(buf), "%s\"%s\": {\"count\": %ld, \"total_ms\": %.6f}", first ? "" : ", ",
                  kv.first.c_str(), kv.second.first, kv.second.second);
    js += buf;
    first = false;
  }
  js += "}";
  if (js.size() + 1 > cap) return BLS381_EARG;
  std::memcpy(out, js.c_str(), js.size() + 1);
  return (int)js.size();
}

size_t bls381_verify_batch_workspace_size(size_t n) { return verify_ws_size(n); }

int bls381_verify_batch_device(size_t n, const uint8_t* d_pks, const uint8_t* d_msgs32, const uint8_t* d_sigs,
                               const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace, void* stream) {
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  if (n == 0) return 0;
  if (!d_pks || !d_msgs32 || !d_sigs || !d_dom8s || !d_verdicts || !d_workspace) return BLS381_EARG;
  hipStream_t s = (hipStream_t)stream;   // NULL = the HIP null stream (torch's default stream)
  return run_verify_batch(c, n, d_pks, d_msgs32, d_sigs, d_dom8s, d_verdicts, d_workspace, s);
}

int bls381_verify_batch(size_t n, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs,
                        const uint8_t* dom8s, uint8_t* verdicts_out) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n == 0) return 0;
    if (!pks || !msgs32 || !sigs || !dom8s || !verdicts_out) return BLS381_EARG;
    HostCall hc(c);
    VerifyIn d;
    TRY(hc.carve([&](Bump& b) { d.carve(b, n, verify_ws_size(n)); }));
    TRY(d.upload(hc, n, pks, msgs32, sigs, dom8s));
    TRY(run_verify_batch(c, n, d.pks, d.msgs, d.sigs, d.doms, d.v, d.ws, hc.s));
    TRY(hc.download(verdicts_out, d.v, n));
    return hc.finish();
  });
}

// BLS381_LAT_PAD = k > 1 (measurement knob, default 1 = off): a single call runs as a batch of k
// identical copies.
// Same kernels, same per-item work and the same verdict, but measured on MI355X (r04t/r04u, one box,
// three alternating rounds of 40 calls): bls_verify through the shim 9.95-10.06 ms median as one item,
// 8.93-8.95 ms as 32 copies (min 8.88-8.90), 9.44-9.59 as 8, 9.05 as 128.  The per-kernel times of
// a lone wave vary from run to run and are slower than the same wave among 32; the
// cause is not established -- it behaves like a clock policy that reads an almost idle GPU.  The
// padding multiplies the device work of every single call by k for any other stream or process
// sharing the GPU, so it is opt-in.
static int lat_pad() {
  static const int pad = std::max(1, std::min(1024, env_knob("BLS381_LAT_PAD", 1)));
  return pad;
}

int bls381_verify(const uint8_t pk[48], const uint8_t* msg, size_t msg_len, const uint8_t sig[96],
                  const uint8_t dom8[8]) {
  if (!pk || !sig || !dom8 || (!msg && msg_len)) return BLS381_EARG;
  if (msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  if (msg_len == 32) {
    const int pad = lat_pad();
    if (pad > 1) {
      std::vector<uint8_t> P((size_t)pad * 48), M((size_t)pad * 32), S((size_t)pad * 96), D((size_t)pad * 8), V(pad);
      for (int k = 0; k < pad; ++k) {
        std::memcpy(&P[48 * k], pk, 48); std::memcpy(&M[32 * k], msg, 32);
        std::memcpy(&S[96 * k], sig, 96); std::memcpy(&D[8 * k], dom8, 8);
      }
      int rc = bls381_verify_batch((size_t)pad, P.data(), M.data(), S.data(), D.data(), V.data());
      return rc ? rc : V[0];
    }
    uint8_t v = 0;
    int rc = bls381_verify_batch(1, pk, msg, sig, dom8, &v);
    return rc ? rc : v;
  }
  // general message length: one-pair-per-lane path of verify_multiple
  return bls381_verify_multiple(1, pk, msg, msg_len, sig, dom8);
}

// host buffers -> device copies -> the planned pipeline (keys dropped from the plan when all-infinite);
// `b` becomes the pipeline's workspace (vm_ws_bound bytes), from which the caller takes its outputs
static int vm_host(HostCall& hc, size_t n_calls, const uint32_t* call_off, const uint8_t* pks, const uint8_t* msgs,
                   size_t msg_len, const uint8_t* sigs, const uint8_t* dom8s, const int* with_sig, Bump& b,
                   uint32_t** f, uint8_t** st) {
  const size_t nk = call_off[n_calls];
  // the plan's arrays are async copy sources
  Held<VmPlan> pl(hc.c->keep, hc.s, plan_vm(n_calls, call_off, msgs, msg_len, pks, sigs, with_sig));
  const size_t ws_bytes = vm_ws_bound(*pl, msg_len);
  uint8_t *d_pks, *d_sigs, *d_doms, *ws;
  TRY(hc.carve([&](Bump& in) {
    d_pks = in.take<uint8_t>(48 * nk + 1);
    d_sigs = in.take<uint8_t>(96 * n_calls);
    d_doms = in.take<uint8_t>(8 * n_calls);
    ws = in.take<uint8_t>(ws_bytes);
  }));
  b = Bump(ws, ws_bytes);
  TRY(hc.upload(d_pks, pks, 48 * nk));
  TRY(hc.upload(d_sigs, sigs, 96 * n_calls));
  TRY(hc.upload(d_doms, dom8s, 8 * n_calls));
  return run_vm_batch(hc.c, *pl, msg_len, d_pks, d_sigs, d_doms, b, hc.s, f, st);
}

int bls381_verify_multiple_batch(size_t n_calls, const uint32_t* call_off, const uint8_t* pks,
                                 const uint8_t* msgs, size_t msg_len, const uint8_t* sigs, const uint8_t* dom8s,
                                 uint8_t* verdicts) {
  return guarded([&]() -> int {
    if (n_calls == 0) return 0;
    if (!call_off || !sigs || !dom8s || !verdicts || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
    if (call_off[n_calls] && (!pks || (!msgs && msg_len))) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    std::vector<int> with_sig(n_calls, 1);
    Bump b;
    uint32_t* f;
    uint8_t* st;
    TRY(vm_host(hc, n_calls, call_off, pks, msgs, msg_len, sigs, dom8s, with_sig.data(), b, &f, &st));
    uint8_t* d_v = b.take<uint8_t>(n_calls);
    LAUNCH_FE(hc.s, n_calls, f, st, d_v);
    TRY(hc.download(verdicts, d_v, n_calls));
    return hc.finish();
  });
}

size_t bls381_verify_multiple_batch_workspace_size(size_t n_calls, size_t n_pks, size_t msg_len) {
  return vm_ws_bound_sizes(n_calls, n_pks, msg_len) + align256(n_calls) + 4096;
}

int bls381_verify_multiple_batch_device(size_t n_calls, const uint32_t* h_call_off, const uint8_t* h_msgs,
                                        size_t msg_len, const uint8_t* d_pks, const uint8_t* d_sigs,
                                        const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                        void* stream) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n_calls == 0) return 0;
    if (!h_call_off || !d_sigs || !d_dom8s || !d_verdicts || !d_workspace || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
    const size_t nk = h_call_off[n_calls];
    if (h_call_off[0] != 0 || (nk && (!d_pks || (!h_msgs && msg_len)))) return BLS381_EARG;
    for (size_t k = 0; k < n_calls; ++k)
      if (h_call_off[k + 1] < h_call_off[k]) return BLS381_EARG;
    std::vector<int> with_sig(n_calls, 1);
    hipStream_t s = (hipStream_t)stream;
    Held<VmPlan> pl(c->keep, s, plan_vm(n_calls, h_call_off, h_msgs, msg_len, nullptr, nullptr, with_sig.data()));
    Bump b(d_workspace, bls381_verify_multiple_batch_workspace_size(n_calls, nk, msg_len));
    uint32_t* f;
    uint8_t* st;
    if ((rc = run_vm_batch(c, *pl, msg_len, d_pks, d_sigs, d_dom8s, b, s, &f, &st))) return rc;
    LAUNCH_FE(s, n_calls, f, st, d_verdicts);
    return 0;
  });
}

size_t bls381_verify_multiple_grouped_workspace_size(size_t n_calls, size_t n_groups, size_t n_pks, size_t msg_len) {
  return vm_ws_bound_sizes(n_calls, std::max(n_pks, n_groups), msg_len) + align256(n_calls) + 4096;
}

// argument check shared by the grouped device entries (d_keys: compressed keys or registry entries)
static bool grouped_args_ok(size_t n_calls, const uint32_t* h_call_group_off, size_t n_groups,
                            const uint32_t* h_group_key_off, const uint8_t* h_group_msgs, size_t msg_len,
                            const void* d_keys, const uint8_t* d_sigs, const uint8_t* d_dom8s,
                            const uint8_t* d_verdicts, const void* d_workspace) {
  if (!h_call_group_off || !h_group_key_off || !d_sigs || !d_dom8s || !d_verdicts || !d_workspace ||
      msg_len > BLS381_MSG_MAX)
    return false;
  if (h_call_group_off[0] != 0 || h_call_group_off[n_calls] != n_groups || h_group_key_off[0] != 0) return false;
  for (size_t k = 0; k < n_calls; ++k)
    if (h_call_group_off[k + 1] < h_call_group_off[k]) return false;
  for (size_t g = 0; g < n_groups; ++g)
    if (h_group_key_off[g + 1] < h_group_key_off[g]) return false;
  const size_t nk = h_group_key_off[n_groups];
  return !((nk && !d_keys) || (n_groups && msg_len && !h_group_msgs));
}

// plan and queue a grouped batch on `stream`; reg: the keys are registry entries
static int vm_grouped_device(Ctx* c, size_t n_calls, const uint32_t* h_call_group_off, size_t n_groups,
                             const uint32_t* h_group_key_off, const uint8_t* h_group_msgs, size_t msg_len,
                             const uint8_t* d_keys, const uint8_t* d_sigs, const uint8_t* d_dom8s, uint8_t* d_verdicts,
                             void* d_workspace, void* stream, const agg_reg_src* reg) {
  hipStream_t s = (hipStream_t)stream;
  Held<VmPlan> pl(c->keep, s, plan_vm_grouped(n_calls, h_call_group_off, h_group_key_off, h_group_msgs, msg_len));
  Bump b(d_workspace, bls381_verify_multiple_grouped_workspace_size(n_calls, n_groups, h_group_key_off[n_groups], msg_len));
  uint32_t* f;
  uint8_t* st;
  TRY(run_vm_batch(c, *pl, msg_len, d_keys, d_sigs, d_dom8s, b, s, &f, &st, reg));
  LAUNCH_FE(s, n_calls, f, st, d_verdicts);
  return 0;
}

int bls381_verify_multiple_grouped_device(size_t n_calls, const uint32_t* h_call_group_off, size_t n_groups,
                                          const uint32_t* h_group_key_off, const uint8_t* h_group_msgs,
                                          size_t msg_len, const uint8_t* d_pks, const uint8_t* d_sigs,
                                          const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                          void* stream) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n_calls == 0) return 0;
    if (!grouped_args_ok(n_calls, h_call_group_off, n_groups, h_group_key_off, h_group_msgs, msg_len, d_pks, d_sigs,
                         d_dom8s, d_verdicts, d_workspace))
      return BLS381_EARG;
    return vm_grouped_device(c, n_calls, h_call_group_off, n_groups, h_group_key_off, h_group_msgs, msg_len, d_pks,
                             d_sigs, d_dom8s, d_verdicts, d_workspace, stream, nullptr);
  });
}

int bls381_verify_multiple(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len, const uint8_t sig[96],
                           const uint8_t dom8[8]) {
  if ((n && (!pks || (!msgs && msg_len))) || !sig || !dom8 || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  const int pad = lat_pad();
  if (pad > 1 && n <= 64 && msg_len <= 64) {   // a single call as lat_pad() identical calls
    const size_t P = (size_t)pad;
    std::vector<uint32_t> off(P + 1);
    std::vector<uint8_t> K(48 * n * P + 1), M(msg_len * n * P + 1), S(96 * P), D(8 * P), V(P);
    for (size_t k = 0; k < P; ++k) {
      off[k] = (uint32_t)(k * n);
      if (n) std::memcpy(&K[48 * n * k], pks, 48 * n);
      if (n && msg_len) std::memcpy(&M[msg_len * n * k], msgs, msg_len * n);
      std::memcpy(&S[96 * k], sig, 96);
      std::memcpy(&D[8 * k], dom8, 8);
    }
    off[P] = (uint32_t)(P * n);
    const int rc = bls381_verify_multiple_batch(P, off.data(), K.data(), M.data(), msg_len, S.data(), D.data(),
                                                V.data());
    return rc ? rc : V[0];
  }
  const uint32_t off[2] = {0, (uint32_t)n};
  uint8_t v = 0;
  const int rc = bls381_verify_multiple_batch(1, off, pks, msgs, msg_len, sig, dom8, &v);
  return rc ? rc : v;
}

int bls381_miller_partial(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len, const uint8_t sig[96],
                          int include_sig, const uint8_t dom8[8], uint8_t out576[576]) {
  return guarded([&]() -> int {
    if ((n && (!pks || (!msgs && msg_len))) || !sig || !dom8 || !out576 || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const uint32_t off[2] = {0, (uint32_t)n};
    const int with_sig = include_sig ? 1 : 0;
    Bump b;
    uint32_t* f;
    uint8_t* st;
    TRY(vm_host(hc, 1, off, pks, msgs, msg_len, sig, dom8, &with_sig, b, &f, &st));
    uint8_t* d_out = b.take<uint8_t>(576);
    LAUNCH("fp12_to_bytes", hc.s, dim3(1), dim3(KBLOCK), k_fp12_to_bytes, (size_t)1, (const uint32_t*)f, d_out);
    uint8_t h_st = 0;
    TRY(hc.download(out576, d_out, 576));
    TRY(hc.download(&h_st, st, 1));
    TRY(hc.finish());
    return h_st == ST_OK ? 0 : 1;
  });
}

int bls381_final_verify(size_t k, const uint8_t* parts576) {
  return guarded([&]() -> int {
    if (k == 0 || !parts576) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    const auto passes = plan_products({0u, (uint32_t)k});   // outlives hc, which synchronises on every way out
    HostCall hc(c);
    uint8_t *d_in, *st, *d_v;
    uint32_t* f;
    Bump pb;   // the product passes' slices
    TRY(hc.carve([&](Bump& b) {
      d_in = b.take<uint8_t>(576 * k);
      f = b.take<uint32_t>(12 * FP_LIMBS * k);
      st = b.take<uint8_t>(k);
      d_v = b.take<uint8_t>(1);
      size_t pass_bytes = 0;
      for (const auto& ch : passes) pass_bytes += chunk_level_bytes(ch.size(), 12);
      pb = Bump(b.take<uint8_t>(pass_bytes), pass_bytes);
    }));
    hipStream_t s = hc.s;
    TRY(hc.upload(d_in, parts576, 576 * k));
    HIPC(hipMemsetAsync(st, 0, k, s));
    LAUNCH("fp12_from_bytes", s, dim3(grid_for(2 * k)), dim3(KBLOCK), k_fp12_from_bytes, k, (const uint8_t*)d_in, f);
    TRY(run_product_passes(pb, s, passes, f, st, k));
    LAUNCH_FE(s, (size_t)1, f, st, d_v);
    uint8_t v = 0;
    TRY(hc.download(&v, d_v, 1));
    TRY(hc.finish());
    return v;
  });
}

// ---- aggregation
// flags: the decode flags (CHK_*) -- policy_flags(0) for a bls_aggregate_* call, 0 (strict codec) for
// partials this library encoded itself
static int agg_batch_impl(Ctx* c, int is_g2, size_t ng, const uint32_t* offsets, size_t n_pts, const uint8_t* d_pts,
                          uint8_t* d_out, int32_t* d_status, void* ws, size_t ws_cap, hipStream_t s, int flags) {
  // the offsets must describe exactly the n_pts points given, in order
  if (offsets[0] != 0 || offsets[ng] != n_pts) { t_err = "offsets disagree with n_pks"; return BLS381_EARG; }
  for (size_t g = 0; g < ng; ++g)
    if (offsets[g + 1] < offsets[g]) { t_err = "offsets not monotone"; return BLS381_EARG; }
  // the chunk lists are async-copy sources: they live until the stream passes them
  Held<AggPlan> hold(c->keep, s, plan_agg(ng, offsets, is_g2 ? 2 : 1));
  const AggPlan& plan = *hold;
  const uint32_t* jac;
  const uint8_t* bad;
  size_t used = 0;
  int rc;
  if (is_g2) {
    if ((rc = run_agg<fp2p_t>(plan, ng, d_pts, ws, s, &jac, &bad, &used, ws_cap, nullptr, flags))) return rc;
    LAUNCH("agg_compress", s, dim3(grid_for(2 * ng)), dim3(KBLOCK), k_agg_compress<fp2p_t>, ng, jac, bad, d_out, d_status);
  } else {
    if ((rc = run_agg<fp_t>(plan, ng, d_pts, ws, s, &jac, &bad, &used, ws_cap, nullptr, flags))) return rc;
    LAUNCH("agg_compress", s, dim3(grid_for(ng)), dim3(KBLOCK), k_agg_compress<fp_t>, ng, jac, bad, d_out, d_status);
  }
  return 0;
}

static size_t agg_ws_bytes(int is_g2, size_t ng, const uint32_t* offsets) {
  AggPlan plan = plan_agg(ng, offsets, is_g2 ? 2 : 1);
  return agg_ws_size(plan, is_g2 ? 6 : 3);
}

size_t bls381_aggregate_pubkeys_batch_workspace_size(size_t n_groups, size_t n_pks) {
  return agg_ws_bound_sizes(n_groups, n_pks);
}

int bls381_aggregate_pubkeys_batch_device(size_t n_groups, const uint32_t* h_offsets, size_t n_pks,
                                          const uint8_t* d_pks, uint8_t* d_out48, int32_t* d_status,
                                          void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n_groups == 0) return 0;
    if (!h_offsets || !d_out48 || !d_status || !d_workspace || (n_pks && !d_pks)) return BLS381_EARG;
    hipStream_t s = (hipStream_t)stream;   // NULL = the HIP null stream (torch's default stream)
    return agg_batch_impl(c, 0, n_groups, h_offsets, n_pks, d_pks, d_out48, d_status, d_workspace,
                          bls381_aggregate_pubkeys_batch_workspace_size(n_groups, n_pks), s, policy_flags(0));
  });
}

// The host form of a grouped aggregation (plain or registry): in_bytes of input copied in, `run(d_in,
// d_out, d_status, ws)` queued on the context stream with a workspace of ws_bytes, then ng results of
// out_bytes each and ng statuses copied back.
extern "C++" template <class Run>
int agg_host_call(HostCall& hc, size_t ng, const void* in, size_t in_bytes, size_t out_bytes, size_t ws_bytes,
                         uint8_t* out, int32_t* status, Run&& run) {
  uint8_t *d_in, *d_out, *d_ws;
  int32_t* d_st;
  TRY(hc.carve([&](Bump& b) {
    d_in = b.take<uint8_t>(in_bytes + 1);
    d_out = b.take<uint8_t>(ng * out_bytes);
    d_st = b.take<int32_t>(ng);
    d_ws = b.take<uint8_t>(ws_bytes);
  }));
  TRY(hc.upload(d_in, in, in_bytes));
  TRY(run(d_in, d_out, d_st, d_ws));
  TRY(hc.download(out, d_out, ng * out_bytes));
  TRY(hc.download(status, d_st, ng * 4));
  return hc.finish();
}

static int agg_host(int is_g2, size_t ng, const uint32_t* offsets, const uint8_t* pts, uint8_t* out, int32_t* status) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t bytes = is_g2 ? 96 : 48, npts = offsets[ng], wsb = agg_ws_bytes(is_g2, ng, offsets);
    return agg_host_call(hc, ng, pts, npts * bytes, bytes, wsb, out, status,
                         [&](uint8_t* d_pts, uint8_t* d_out, int32_t* d_st, uint8_t* d_ws) {
                           return agg_batch_impl(c, is_g2, ng, offsets, npts, d_pts, d_out, d_st, d_ws, wsb, hc.s,
                                                 policy_flags(0));
                         });
  });
}

int bls381_aggregate_pubkeys_batch(size_t n_groups, const uint32_t* offsets, const uint8_t* pks, uint8_t* out48,
                                   int32_t* status) {
  if (n_groups == 0) return 0;
  if (!offsets || !out48 || !status || (offsets[n_groups] && !pks)) return BLS381_EARG;
  return agg_host(0, n_groups, offsets, pks, out48, status);
}

int bls381_aggregate_pubkeys(size_t n, const uint8_t* pks, uint8_t out[48]) {
  if (!out || (n && !pks)) return BLS381_EARG;
  uint32_t off[2] = {0, (uint32_t)n};
  int32_t st = 0;
  int rc = agg_host(0, 1, off, pks, out, &st);
  return rc ? rc : st;
}

int bls381_aggregate_signatures(size_t n, const uint8_t* sigs, uint8_t out[96]) {
  if (!out || (n && !sigs)) return BLS381_EARG;
  uint32_t off[2] = {0, (uint32_t)n};
  int32_t st = 0;
  int rc = agg_host(1, 1, off, sigs, out, &st);
  return rc ? rc : st;
}

int bls381_aggregate_g1(size_t n, const uint8_t* pks, uint8_t out[48]) { return bls381_aggregate_pubkeys(n, pks, out); }
int bls381_aggregate_g2(size_t n, const uint8_t* sigs, uint8_t out[96]) {
  return bls381_aggregate_signatures(n, sigs, out);
}

// ---- signing / key / hash helpers (fixtures / reference API); the single-item forms are one-item batches
static int sign_impl(size_t n, const uint8_t* msgs, size_t msg_len, const uint8_t* sks, const uint8_t* dom8s,
                     uint8_t* out96) {
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  HostCall hc(c);
  uint8_t *d_msg, *d_sk, *d_dom, *d_out;
  TRY(hc.carve([&](Bump& b) {
    d_msg = b.take<uint8_t>(msg_len * n + 1);
    d_sk = b.take<uint8_t>(32 * n);
    d_dom = b.take<uint8_t>(8 * n);
    d_out = b.take<uint8_t>(96 * n);
  }));
  TRY(hc.upload(d_msg, msgs, msg_len * n));
  TRY(hc.upload(d_sk, sks, 32 * n));
  TRY(hc.upload(d_dom, dom8s, 8 * n));
  LAUNCH("sign", hc.s, dim3(grid_for(2 * n)), dim3(KBLOCK), k_sign, n, (const uint8_t*)d_msg, (uint32_t)msg_len,
         (const uint8_t*)d_sk, (const uint8_t*)d_dom, d_out);
  TRY(hc.download(out96, d_out, 96 * n));
  return hc.finish();
}

int bls381_sign(const uint8_t* msg, size_t msg_len, const uint8_t sk[32], const uint8_t dom8[8], uint8_t out[96]) {
  if ((!msg && msg_len) || !sk || !dom8 || !out || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  return guarded([&] { return sign_impl(1, msg, msg_len, sk, dom8, out); });
}

int bls381_sign_batch(size_t n, const uint8_t* msgs32, const uint8_t* sks, const uint8_t* dom8s, uint8_t* out96) {
  if (n == 0) return 0;
  if (!msgs32 || !sks || !dom8s || !out96) return BLS381_EARG;
  return guarded([&] { return sign_impl(n, msgs32, 32, sks, dom8s, out96); });
}

int bls381_privtopub_batch(size_t n, const uint8_t* sks, uint8_t* out48) {
  if (n == 0) return 0;
  if (!sks || !out48) return BLS381_EARG;
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t *d_sk, *d_out;
    TRY(hc.carve([&](Bump& b) {
      d_sk = b.take<uint8_t>(32 * n);
      d_out = b.take<uint8_t>(48 * n);
    }));
    TRY(hc.upload(d_sk, sks, 32 * n));
    LAUNCH("privtopub", hc.s, dim3(grid_for(n)), dim3(KBLOCK), k_privtopub, n, (const uint8_t*)d_sk, d_out);
    TRY(hc.download(out48, d_out, 48 * n));
    return hc.finish();
  });
}

int bls381_privtopub(const uint8_t sk[32], uint8_t out[48]) {
  if (!sk || !out) return BLS381_EARG;
  return bls381_privtopub_batch(1, sk, out);
}

int bls381_hash_to_g2(const uint8_t* msg, size_t msg_len, const uint8_t dom8[8], uint8_t out_compressed[96],
                      uint8_t out_affine[192]) {
  if ((!msg && msg_len) || !dom8 || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t *d_msg, *d_dom, *d_comp, *d_aff;
    TRY(hc.carve([&](Bump& b) {
      d_msg = b.take<uint8_t>(msg_len + 1);
      d_dom = b.take<uint8_t>(8);
      d_comp = b.take<uint8_t>(96);
      d_aff = b.take<uint8_t>(192);
    }));
    TRY(hc.upload(d_msg, msg, msg_len));
    TRY(hc.upload(d_dom, dom8, 8));
    LAUNCH("hash_to_g2", hc.s, dim3(1), dim3(KBLOCK), k_hash_g2_out, (size_t)1, (const uint8_t*)d_msg,
           (uint32_t)msg_len, (const uint8_t*)d_dom, d_comp, d_aff);
    if (out_compressed) TRY(hc.download(out_compressed, d_comp, 96));
    if (out_affine) TRY(hc.download(out_affine, d_aff, 192));
    return hc.finish();
  });
}

int bls381_hash_to_g2_pyecc_projective(size_t n, const uint8_t* msgs32, const uint8_t* dom8s, uint8_t* out288) {
  if (n == 0) return 0;
  if (!msgs32 || !dom8s || !out288) return BLS381_EARG;
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t scratch = (size_t)n * H2_BITS * 6 * FPW;
    uint8_t *d_msgs, *d_doms, *d_out;
    uint32_t* d_scr;
    TRY(hc.carve([&](Bump& b) {
      d_msgs = b.take<uint8_t>(32 * n);
      d_doms = b.take<uint8_t>(8 * n);
      d_out = b.take<uint8_t>(288 * n);
      d_scr = b.take<uint32_t>(scratch / 4);
    }));
    TRY(hc.upload(d_msgs, msgs32, 32 * n));
    TRY(hc.upload(d_doms, dom8s, 8 * n));
    LAUNCH("hash_to_g2_pyecc", hc.s, dim3(grid_for(2 * n, 64)), dim3(64), k_hash_g2_pyecc, n, (const uint8_t*)d_msgs,
           (const uint8_t*)d_doms, d_scr, d_out);
    TRY(hc.download(out288, d_out, 288 * n));
    return hc.finish();
  });
}

// ---- pubkey registry
struct bls381_registry {
  int device = -1;
  size_t cap = 0, size = 0;
  uint32_t tmask = 0;
  uint8_t* keys = nullptr;    // cap x 48 B
  uint32_t* aff = nullptr;    // SoA affine, 2 x 14 words x cap
  uint8_t* st = nullptr;      // cap entry statuses
  uint32_t* table = nullptr;  // tmask + 1 slots
  int32_t* tmp = nullptr;     // cap scratch entries (add / lookup results)
  std::mutex mu;
};

static void registry_free(bls381_registry* r) {
  if (!r) return;
  (void)hipFree(r->keys); (void)hipFree(r->aff); (void)hipFree(r->st); (void)hipFree(r->table); (void)hipFree(r->tmp);
  delete r;
}

int bls381_registry_create(size_t capacity, bls381_registry** out) {
  if (!out || capacity == 0 || capacity > (size_t)INT32_MAX / 2) return BLS381_EARG;
  *out = nullptr;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  auto* r = new bls381_registry();
  r->device = c->device;
  r->cap = capacity;
  const size_t t = registry_table_slots(capacity);
  r->tmask = (uint32_t)(t - 1);
  if (hipMalloc(&r->keys, 48 * capacity) != hipSuccess || hipMalloc(&r->aff, 2 * FPW * capacity) != hipSuccess ||
      hipMalloc(&r->st, capacity) != hipSuccess || hipMalloc(&r->table, 4 * t) != hipSuccess ||
      hipMalloc(&r->tmp, 4 * capacity) != hipSuccess) {
    registry_free(r);
    t_err = "registry allocation failed";
    return BLS381_EHIP;
  }
  if (hipMemsetAsync(r->table, 0xFF, 4 * t, c->q.main) != hipSuccess || hipStreamSynchronize(c->q.main) != hipSuccess) {
    registry_free(r);
    t_err = "registry init failed";
    return BLS381_EHIP;
  }
  *out = r;
  return 0;
}

void bls381_registry_destroy(bls381_registry* reg) {
  if (!reg) return;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (c) (void)hipStreamSynchronize(c->q.main);
  registry_free(reg);
}

size_t bls381_registry_size(const bls381_registry* reg) { return reg ? reg->size : 0; }

static Ctx* registry_ctx(bls381_registry* reg, int* rc) {
  Ctx* c = get_ctx(rc);
  if (c && c->device != reg->device) { t_err = "registry belongs to another device"; *rc = BLS381_EARG; return nullptr; }
  return c;
}

int bls381_registry_add(bls381_registry* reg, size_t n, const uint8_t* pks48, int32_t* entry_out) {
  if (!reg || (n && !pks48)) return BLS381_EARG;
  if (n == 0) return 0;
  int rc = 0;
  Ctx* c = registry_ctx(reg, &rc);
  if (!c) return rc;
  std::lock_guard<std::mutex> lr(reg->mu);
  std::vector<int32_t> res(n);   // outlives hc, which synchronises on every way out
  HostCall hc(c);
  if (reg->size + n > reg->cap) { t_err = "registry capacity exceeded"; return BLS381_EARG; }
  hipStream_t s = hc.s;
  const size_t first = reg->size;
  TRY(hc.upload(reg->keys + 48 * first, pks48, 48 * n));
  LAUNCH("registry_decode", s, dim3(grid_for(n)), dim3(KBLOCK), k_reg_decode, first, n, reg->cap,
         (const uint8_t*)reg->keys, reg->aff, reg->st);
  LAUNCH("registry_insert", s, dim3(grid_for(n)), dim3(KBLOCK), k_reg_insert, first, n, (const uint8_t*)reg->keys,
         (const uint8_t*)reg->st, reg->table, reg->tmask);
  LAUNCH("registry_lookup", s, dim3(grid_for(n)), dim3(KBLOCK), k_reg_lookup, n,
         (const uint8_t*)(reg->keys + 48 * first), (const uint8_t*)reg->keys, (const uint32_t*)reg->table, reg->tmask,
         reg->tmp);
  TRY(hc.download(res.data(), reg->tmp, 4 * n));
  TRY(hc.finish());
  reg->size += n;
  int nbad = 0;
  for (size_t i = 0; i < n; ++i) nbad += res[i] < 0;
  if (entry_out) std::memcpy(entry_out, res.data(), 4 * n);
  return nbad;
}

int bls381_registry_lookup(bls381_registry* reg, size_t n, const uint8_t* pks48, int32_t* entry_out) {
  return guarded([&]() -> int {
    if (!reg || (n && (!pks48 || !entry_out))) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    HostCall hc(c);
    uint8_t* d_q;
    int32_t* d_e;
    TRY(hc.carve([&](Bump& b) {
      d_q = b.take<uint8_t>(48 * n);
      d_e = b.take<int32_t>(n);
    }));
    TRY(hc.upload(d_q, pks48, 48 * n));
    LAUNCH("registry_lookup", hc.s, dim3(grid_for(n)), dim3(KBLOCK), k_reg_lookup, n, (const uint8_t*)d_q,
           (const uint8_t*)reg->keys, (const uint32_t*)reg->table, reg->tmask, d_e);
    TRY(hc.download(entry_out, d_e, 4 * n));
    TRY(hc.finish());
    int hits = 0;
    for (size_t i = 0; i < n; ++i) hits += entry_out[i] >= 0;
    return hits;
  });
}

// groups of registry entries (d_entry, device) or of compressed keys looked up first (d_pks); one pass of the
// chunked tree, then compression.  Returns once queued on s.
static int registry_agg_impl(Ctx* c, bls381_registry* reg, size_t ng, const uint32_t* offsets, size_t n_in,
                             const int32_t* d_entry, const uint8_t* d_pks, uint8_t* d_out, int32_t* d_status,
                             void* ws, size_t ws_cap, hipStream_t s) {
  Bump b(ws, ws_cap);
  if (!d_entry) {
    int32_t* e = b.take<int32_t>(n_in + 1);
    LAUNCH("registry_lookup", s, dim3(grid_for(n_in)), dim3(KBLOCK), k_reg_lookup, n_in, d_pks,
           (const uint8_t*)reg->keys, (const uint32_t*)reg->table, reg->tmask, e);
    d_entry = e;
  }
  Held<AggPlan> hold(c->keep, s, plan_agg(ng, offsets));
  const agg_reg_src src{d_entry, reg->aff, reg->st, reg->cap, reg->size};
  const uint32_t* jac;
  const uint8_t* bad;
  size_t used = 0;
  int rc = run_agg<fp_t>(*hold, ng, d_pks, b.base + align256(b.off), s, &jac, &bad, &used, b.left() - 256, &src,
                         policy_flags(0));
  if (rc) return rc;
  LAUNCH("agg_compress", s, dim3(grid_for(ng)), dim3(KBLOCK), k_agg_compress<fp_t>, ng, jac, bad, d_out, d_status);
  return 0;
}

size_t bls381_registry_aggregate_workspace_size(size_t n_groups, size_t n_in) {
  return align256(4 * (n_in + 1)) + bls381_aggregate_pubkeys_batch_workspace_size(n_groups, n_in) + 4096;
}

int bls381_registry_aggregate_indices_device(bls381_registry* reg, size_t n_groups, const uint32_t* h_offsets,
                                             size_t n_idx, const uint32_t* d_indices, uint8_t* d_out48,
                                             int32_t* d_status, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!reg || !h_offsets || !d_out48 || !d_status || !d_workspace || (n_idx && !d_indices)) return BLS381_EARG;
    if (n_groups == 0) return 0;
    if (h_offsets[n_groups] != n_idx) return BLS381_EARG;
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    return registry_agg_impl(c, reg, n_groups, h_offsets, n_idx, (const int32_t*)d_indices, nullptr, d_out48, d_status,
                             d_workspace, bls381_registry_aggregate_workspace_size(n_groups, n_idx), (hipStream_t)stream);
  });
}

int bls381_registry_verify_multiple_grouped_device(bls381_registry* reg, size_t n_calls,
                                                   const uint32_t* h_call_group_off, size_t n_groups,
                                                   const uint32_t* h_group_key_off, const uint8_t* h_group_msgs,
                                                   size_t msg_len, const uint32_t* d_entries, const uint8_t* d_sigs,
                                                   const uint8_t* d_dom8s, uint8_t* d_verdicts, void* d_workspace,
                                                   void* stream) {
  return guarded([&]() -> int {
    if (!reg) return BLS381_EARG;
    if (n_calls == 0) return 0;
    if (!grouped_args_ok(n_calls, h_call_group_off, n_groups, h_group_key_off, h_group_msgs, msg_len, d_entries, d_sigs,
                         d_dom8s, d_verdicts, d_workspace))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    const agg_reg_src src{nullptr, reg->aff, reg->st, reg->cap, reg->size};
    return vm_grouped_device(c, n_calls, h_call_group_off, n_groups, h_group_key_off, h_group_msgs, msg_len,
                             (const uint8_t*)d_entries, d_sigs, d_dom8s, d_verdicts, d_workspace, stream, &src);
  });
}

static int registry_agg_host(bls381_registry* reg, size_t ng, const uint32_t* offsets, const uint32_t* indices,
                             const uint8_t* pks, uint8_t* out48, int32_t* status) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    HostCall hc(c);
    const size_t n_in = offsets[ng], wsb = bls381_registry_aggregate_workspace_size(ng, n_in);
    return agg_host_call(hc, ng, indices ? (const void*)indices : (const void*)pks, n_in * (indices ? 4 : 48), 48, wsb,
                         out48, status, [&](uint8_t* d_in, uint8_t* d_out, int32_t* d_st, uint8_t* d_ws) {
                           return registry_agg_impl(c, reg, ng, offsets, n_in, indices ? (const int32_t*)d_in : nullptr,
                                                    indices ? nullptr : d_in, d_out, d_st, d_ws, wsb, hc.s);
                         });
  });
}

int bls381_registry_aggregate_indices(bls381_registry* reg, size_t n_groups, const uint32_t* offsets,
                                      const uint32_t* indices, uint8_t* out48, int32_t* status) {
  if (!reg || !offsets || !out48 || !status || (offsets[n_groups] && !indices)) return BLS381_EARG;
  if (n_groups == 0) return 0;
  return registry_agg_host(reg, n_groups, offsets, indices, nullptr, out48, status);
}

int bls381_registry_aggregate_pubkeys_batch(bls381_registry* reg, size_t n_groups, const uint32_t* offsets,
                                            const uint8_t* pks, uint8_t* out48, int32_t* status) {
  if (!reg || !offsets || !out48 || !status || (offsets[n_groups] && !pks)) return BLS381_EARG;
  if (n_groups == 0) return 0;
  return registry_agg_host(reg, n_groups, offsets, nullptr, pks, out48, status);
}

// ---- SSZ roots and the deposit pipeline
// (ssz_prog_ok and the deposit signing program: bls381_plan.hpp)
struct SszWs {
  uint32_t* prog;
  int32_t* err;
};
static SszWs carve_ssz(Bump& b) {
  SszWs w;
  w.prog = b.take<uint32_t>(SSZ_PROG_MAX);
  w.err = b.take<int32_t>(1);
  return w;
}
size_t bls381_ssz_root_workspace_size(void) {
  return carved_bytes([](Bump& b) { carve_ssz(b); });
}

static int ssz_root_impl(size_t n, const uint8_t* d_items, size_t stride, const uint32_t* h_prog, uint32_t plen,
                         uint8_t* d_roots, const SszWs& w, hipStream_t s, Ctx* c) {
  Held<std::vector<uint32_t>> prog(c->keep, s, std::vector<uint32_t>(h_prog, h_prog + plen));
  HIPC(hipMemcpyAsync(w.prog, prog->data(), 4 * plen, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(w.err, 0, 4, s));
  LAUNCH("ssz_root", s, dim3(grid_for(n)), dim3(KBLOCK), k_ssz_root, n, d_items, stride, (const uint32_t*)w.prog,
         plen, d_roots, w.err);
  return 0;
}

int bls381_ssz_root_batch_device(size_t n, const uint8_t* d_items, size_t stride, size_t item_size,
                                 const uint32_t* h_prog, uint32_t prog_len, uint8_t* d_roots32, void* d_workspace,
                                 void* stream) {
  return guarded([&]() -> int {
    if (n == 0) return 0;
    if (!d_items || !d_roots32 || !d_workspace || stride < item_size || !ssz_prog_ok(h_prog, prog_len, item_size))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    Bump b(d_workspace, bls381_ssz_root_workspace_size());
    return ssz_root_impl(n, d_items, stride, h_prog, prog_len, d_roots32, carve_ssz(b), (hipStream_t)stream, c);
  });
}

int bls381_ssz_root_batch(size_t n, const uint8_t* items, size_t item_size, const uint32_t* prog, uint32_t prog_len,
                          uint8_t* roots32) {
  return guarded([&]() -> int {
    if (n == 0) return 0;
    if (!items || !roots32 || item_size == 0 || !ssz_prog_ok(prog, prog_len, item_size)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t *d_items, *d_roots;
    SszWs w;
    TRY(hc.carve([&](Bump& b) {
      d_items = b.take<uint8_t>(n * item_size);
      d_roots = b.take<uint8_t>(32 * n);
      w = carve_ssz(b);
    }));
    TRY(hc.upload(d_items, items, n * item_size));
    TRY(ssz_root_impl(n, d_items, item_size, prog, prog_len, d_roots, w, hc.s, c));
    TRY(hc.download(roots32, d_roots, 32 * n));
    return hc.finish();
  });
}

// the deposit pipeline's workspace: the gathered keys and signatures, the signing roots, the root
// program's and the verify batch's own
struct DepositWs {
  uint8_t *pks, *sigs, *roots;
  SszWs ssz;
  void* verify;
};
static DepositWs carve_deposits(Bump& b, size_t n) {
  DepositWs w;
  w.pks = b.take<uint8_t>(48 * n);
  w.sigs = b.take<uint8_t>(96 * n);
  w.roots = b.take<uint8_t>(32 * n);
  w.ssz = carve_ssz(b);
  w.verify = b.take<uint8_t>(verify_ws_size(n));
  return w;
}
size_t bls381_verify_deposits_workspace_size(size_t n) {
  return carved_bytes([&](Bump& b) { carve_deposits(b, n); });
}

int bls381_verify_deposits_device(size_t n, const uint8_t* d_deposit_data, const uint8_t* d_dom8s,
                                  uint8_t* d_verdicts, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (n == 0) return 0;
    if (!d_deposit_data || !d_dom8s || !d_verdicts || !d_workspace) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_verify_deposits_workspace_size(n));
    const DepositWs w = carve_deposits(b, n);
    LAUNCH("gather_pubkeys", s, dim3(grid_for(48 * n)), dim3(KBLOCK), k_gather_field, n, d_deposit_data,
           DEPOSIT_DATA_BYTES, 0u, 48u, w.pks);
    LAUNCH("gather_signatures", s, dim3(grid_for(96 * n)), dim3(KBLOCK), k_gather_field, n, d_deposit_data,
           DEPOSIT_DATA_BYTES, 88u, 96u, w.sigs);
    TRY(ssz_root_impl(n, d_deposit_data, DEPOSIT_DATA_BYTES, DEPOSIT_SIGNING_PROG, DEPOSIT_SIGNING_PROG_LEN, w.roots,
                      w.ssz, s, c));
    return run_verify_batch(c, n, w.pks, w.roots, w.sigs, d_dom8s, d_verdicts, w.verify, s);
  });
}

int bls381_verify_deposits(size_t n, const uint8_t* deposit_data, const uint8_t* dom8s, uint8_t* verdicts) {
  return guarded([&]() -> int {
    if (n == 0) return 0;
    if (!deposit_data || !dom8s || !verdicts) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_verify_deposits_workspace_size(n);
    uint8_t *d_dd, *d_dom, *d_ver, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_dd = b.take<uint8_t>(DEPOSIT_DATA_BYTES * n);
      d_dom = b.take<uint8_t>(8 * n);
      d_ver = b.take<uint8_t>(n);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_dd, deposit_data, DEPOSIT_DATA_BYTES * n));
    TRY(hc.upload(d_dom, dom8s, 8 * n));
    TRY(bls381_verify_deposits_device(n, d_dd, d_dom, d_ver, d_ws, hc.s));
    TRY(hc.download(verdicts, d_ver, n));
    return hc.finish();
  });
}

// ---- verify_merkle_branch batches and process_deposit over the registry
static bool merkle_args_ok(size_t n, const void* leaves, const void* proofs, uint32_t depth, const void* indices,
                           const void* roots, size_t root_stride, const void* ok_out) {
  if (depth > 64 || (root_stride != 0 && root_stride != 32) || n > (size_t)INT32_MAX) return false;
  return n == 0 || (leaves && (proofs || depth == 0) && indices && roots && ok_out);
}

int bls381_merkle_branch_batch_device(size_t n, const uint8_t* d_leaves32, const uint8_t* d_proofs, uint32_t depth,
                                      const uint64_t* d_indices, const uint8_t* d_roots32, size_t root_stride,
                                      uint8_t* d_ok, void* stream) {
  return guarded([&]() -> int {
    if (!merkle_args_ok(n, d_leaves32, d_proofs, depth, d_indices, d_roots32, root_stride, d_ok)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    LAUNCH("merkle_branch", (hipStream_t)stream, dim3(grid_for(n)), dim3(KBLOCK), k_merkle_branch, n, d_leaves32,
           d_proofs, (size_t)32 * depth, depth, d_indices, (uint64_t)0, d_roots32, root_stride, d_ok,
           (uint32_t*)nullptr);
    return 0;
  });
}

int bls381_merkle_branch_batch(size_t n, const uint8_t* leaves32, const uint8_t* proofs, uint32_t depth,
                               const uint64_t* indices, const uint8_t* roots32, size_t root_stride, uint8_t* ok_out) {
  return guarded([&]() -> int {
    if (!merkle_args_ok(n, leaves32, proofs, depth, indices, roots32, root_stride, ok_out)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t proof_bytes = (size_t)32 * depth * n, root_bytes = root_stride ? 32 * n : 32;
    uint8_t *d_leaves, *d_proofs, *d_roots, *d_ok;
    uint64_t* d_idx;
    TRY(hc.carve([&](Bump& b) {
      d_leaves = b.take<uint8_t>(32 * n);
      d_proofs = b.take<uint8_t>(proof_bytes + 1);
      d_idx = b.take<uint64_t>(n);
      d_roots = b.take<uint8_t>(root_bytes);
      d_ok = b.take<uint8_t>(n);
    }));
    TRY(hc.upload(d_leaves, leaves32, 32 * n));
    TRY(hc.upload(d_proofs, proofs, proof_bytes));
    TRY(hc.upload(d_idx, indices, 8 * n));
    TRY(hc.upload(d_roots, roots32, root_bytes));
    TRY(bls381_merkle_branch_batch_device(n, d_leaves, d_proofs, depth, d_idx, d_roots, root_stride, d_ok, hc.s));
    TRY(hc.download(ok_out, d_ok, n));
    return hc.finish();
  });
}

// ---- Merkle trees across items: roots, proofs, list roots, the deposits builder
// (the plan, the level table and the workspace carve: bls381_plan.hpp)
// Queues the tree of `p` over d_leaves: the passes, then the last step, which writes d_root.
static int merkle_tree_impl(Ctx* c, const MerklePlan& p, const uint8_t* d_leaves, const MerkleWs& w, int mix,
                            uint64_t length, uint8_t* d_root, hipStream_t s) {
  Held<std::vector<merkle_level>> lv(c->keep, s, std::vector<merkle_level>(p.lv, p.lv + MERKLE_DEPTH_MAX + 1));
  HIPC(hipMemcpyAsync(w.lv, lv->data(), sizeof(p.lv), hipMemcpyHostToDevice, s));
  auto row = [&](uint32_t h) -> const uint8_t* { return h == 0 ? d_leaves : w.nodes + p.lv[h].off; };
  for (const merkle_pass& ps : p.passes)
    LAUNCH("merkle_reduce", s, dim3((unsigned)ps.tiles), dim3(MERKLE_TILE / 2), k_merkle_reduce, row(ps.h0), w.nodes,
           (const merkle_level*)w.lv, (const uint8_t*)c->ztab, ps.h0, ps.steps, ps.tile0);
  LAUNCH("merkle_finish", s, dim3(1), dim3(64), k_merkle_finish, p.n ? row(p.top) : (const uint8_t*)nullptr, w.nodes,
         (const merkle_level*)w.lv, (const uint8_t*)c->ztab, p.top, p.depth, p.first, mix, length, d_root);
  return 0;
}
static int merkle_proofs_impl(Ctx* c, const MerklePlan& p, const uint8_t* d_leaves, const MerkleWs& w, size_t n_idx,
                              const uint64_t* d_indices, uint64_t index_base, uint8_t* d_proofs, size_t stride,
                              hipStream_t s) {
  LAUNCH("merkle_proofs", s, dim3(grid_for(n_idx * p.depth)), dim3(KBLOCK), k_merkle_proofs, n_idx, d_indices,
         index_base, p.depth, d_leaves, (const uint8_t*)w.nodes, (const merkle_level*)w.lv, (const uint8_t*)c->ztab,
         d_proofs, stride);
  return 0;
}
static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

size_t bls381_merkle_root_workspace_size(size_t n, uint64_t first, uint32_t depth) {
  return merkle_args_in_range(n, first, depth) ? merkle_ws_size(n, first, depth, false) : 0;
}
size_t bls381_merkle_proofs_workspace_size(size_t n, uint64_t first, uint32_t depth) {
  return merkle_args_in_range(n, first, depth) ? merkle_ws_size(n, first, depth, true) : 0;
}

int bls381_merkle_root_device(size_t n, const uint8_t* d_leaves32, uint64_t first, uint32_t depth, int mix_length,
                              uint64_t length, uint8_t* d_root32, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!merkle_args_in_range(n, first, depth) || !d_root32 || !d_workspace || (n && !d_leaves32) ||
        !aligned4(d_leaves32))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    const MerklePlan p = plan_merkle(n, first, depth, false);
    Bump b(d_workspace, bls381_merkle_root_workspace_size(n, first, depth));
    const MerkleWs w = carve_merkle(b, p.node_bytes);
    return merkle_tree_impl(c, p, d_leaves32, w, mix_length, length, d_root32, (hipStream_t)stream);
  });
}

int bls381_merkle_root(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, int mix_length,
                       uint64_t length, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (!merkle_args_in_range(n, first, depth) || !root || (n && !leaves32)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_merkle_root_workspace_size(n, first, depth);
    uint8_t *d_leaves, *d_root, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_leaves = b.take<uint8_t>(32 * n);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_leaves, leaves32, 32 * n));
    TRY(bls381_merkle_root_device(n, d_leaves, first, depth, mix_length, length, d_root, d_ws, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

static bool merkle_proofs_args_ok(size_t n, const void* leaves, uint64_t first, uint32_t depth, size_t n_idx,
                                  const void* indices, const void* proofs, size_t proof_stride, const void* root) {
  if (!merkle_args_in_range(n, first, depth) || n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * depth)
    return false;
  return root && (n == 0 || leaves) && (n_idx == 0 || (indices && (proofs || depth == 0)));
}

int bls381_merkle_proofs_device(size_t n, const uint8_t* d_leaves32, uint64_t first, uint32_t depth, size_t n_idx,
                                const uint64_t* d_indices, uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32,
                                void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!merkle_proofs_args_ok(n, d_leaves32, first, depth, n_idx, d_indices, d_proofs, proof_stride, d_root32) ||
        !d_workspace || !aligned4(d_leaves32) || !aligned4(d_proofs) || (proof_stride & 3) ||
        ((uintptr_t)d_indices & 7))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MerklePlan p = plan_merkle(n, first, depth, true);
    Bump b(d_workspace, bls381_merkle_proofs_workspace_size(n, first, depth));
    const MerkleWs w = carve_merkle(b, p.node_bytes);
    TRY(merkle_tree_impl(c, p, d_leaves32, w, 0, 0, d_root32, s));
    return merkle_proofs_impl(c, p, d_leaves32, w, n_idx, d_indices, 0, d_proofs, proof_stride, s);
  });
}

int bls381_merkle_proofs(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, size_t n_idx,
                         const uint64_t* indices, uint8_t* proofs, size_t proof_stride, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (!merkle_proofs_args_ok(n, leaves32, first, depth, n_idx, indices, proofs, proof_stride, root))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_merkle_proofs_workspace_size(n, first, depth), row = (size_t)32 * depth;
    uint8_t *d_leaves, *d_proofs, *d_root, *d_ws;
    uint64_t* d_idx;
    TRY(hc.carve([&](Bump& b) {
      d_leaves = b.take<uint8_t>(32 * n);
      d_idx = b.take<uint64_t>(n_idx);
      d_proofs = b.take<uint8_t>(row * n_idx);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_leaves, leaves32, 32 * n));
    TRY(hc.upload(d_idx, indices, 8 * n_idx));
    TRY(bls381_merkle_proofs_device(n, d_leaves, first, depth, n_idx, d_idx, d_proofs, row, d_root, d_ws, hc.s));
    // packed on the device; the caller's rows are proof_stride apart and only their proofs are written
    if (row && n_idx)
      HIPC(hipMemcpy2DAsync(proofs, proof_stride, d_proofs, row, row, n_idx, hipMemcpyDeviceToHost, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

// hash_tree_root of a List / Vector of n fixed-size composite elements: the elements' roots, the
// tree of depth ceil(log2 n) over them, mix_in_length(n) for a list
struct ListRootWs {
  uint8_t* roots;
  SszWs ssz;
  MerkleWs merkle;
};
static ListRootWs carve_list_root(Bump& b, const MerklePlan& p) {
  ListRootWs w;
  w.roots = b.take<uint8_t>(32 * (size_t)p.n);
  w.ssz = carve_ssz(b);
  w.merkle = carve_merkle(b, p.node_bytes);
  return w;
}
size_t bls381_ssz_list_root_workspace_size(size_t n) {
  if (n > (size_t)INT32_MAX) return 0;
  const MerklePlan p = plan_merkle(n, 0, merkle_chunk_depth(n), false);
  return carved_bytes([&](Bump& b) { carve_list_root(b, p); });
}

int bls381_ssz_list_root_device(size_t n, const uint8_t* d_items, size_t stride, size_t item_size,
                                const uint32_t* h_prog, uint32_t prog_len, int mix_length, uint8_t* d_root32,
                                void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !d_root32 || !d_workspace || (n && !d_items) || item_size == 0 ||
        stride < item_size || !ssz_prog_ok(h_prog, prog_len, item_size))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MerklePlan p = plan_merkle(n, 0, merkle_chunk_depth(n), false);
    Bump b(d_workspace, bls381_ssz_list_root_workspace_size(n));
    const ListRootWs w = carve_list_root(b, p);
    if (n) TRY(ssz_root_impl(n, d_items, stride, h_prog, prog_len, w.roots, w.ssz, s, c));
    return merkle_tree_impl(c, p, w.roots, w.merkle, mix_length, n, d_root32, s);
  });
}

int bls381_ssz_list_root(size_t n, const uint8_t* items, size_t item_size, const uint32_t* prog, uint32_t prog_len,
                         int mix_length, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !root || (n && !items) || item_size == 0 || !ssz_prog_ok(prog, prog_len, item_size))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_ssz_list_root_workspace_size(n);
    uint8_t *d_items, *d_root, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_items = b.take<uint8_t>(n * item_size);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_items, items, n * item_size));
    TRY(bls381_ssz_list_root_device(n, d_items, item_size, item_size, prog, prog_len, mix_length, d_root, d_ws, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

// ---- roots of variable-size items (the program and the rules: bls381_ssz.hpp)
// the workspace of the ragged root kernel: the program and its error flag
size_t bls381_ssz_ragged_roots_workspace_size(size_t n) {
  return n > (size_t)INT32_MAX ? 0 : bls381_ssz_root_workspace_size();
}

// what the host can tell of a host-side `starts`: n + 1 non-decreasing offsets, every item below 2^32 bytes
static bool ragged_starts_ok(size_t n, const uint64_t* starts) {
  for (size_t i = 0; i < n; ++i)
    if (starts[i + 1] < starts[i] || starts[i + 1] - starts[i] >= ((uint64_t)1 << 32)) return false;
  return true;
}

// one launch whatever the items hold; d_n_bad (a device word, zeroed here) receives the count of bad items
static int ragged_roots_impl(size_t n, const uint8_t* d_items, size_t items_bytes, const uint64_t* d_starts,
                             const uint32_t* h_prog, uint32_t plen, uint8_t* d_roots, uint8_t* d_status,
                             uint32_t* d_n_bad, const SszWs& w, hipStream_t s, Ctx* c) {
  HIPC(hipMemsetAsync(d_n_bad, 0, 4, s));
  if (n == 0) return 0;
  Held<std::vector<uint32_t>> prog(c->keep, s, std::vector<uint32_t>(h_prog, h_prog + plen));
  HIPC(hipMemcpyAsync(w.prog, prog->data(), 4 * plen, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(w.err, 0, 4, s));
  LAUNCH("ssz_ragged_root", s, dim3(grid_for(n)), dim3(KBLOCK), k_ssz_ragged_root, n, d_items, items_bytes, d_starts,
         (const uint32_t*)w.prog, plen, (const uint8_t*)c->ztab, d_roots, d_status, d_n_bad, w.err);
  return 0;
}

int bls381_ssz_ragged_roots_device(size_t n, const uint8_t* d_items, size_t items_bytes, const uint64_t* d_starts,
                                   const uint32_t* h_prog, uint32_t prog_len, uint8_t* d_roots32, uint8_t* d_status,
                                   uint32_t* d_n_bad, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !ssz_ragged_prog_ok(h_prog, prog_len, 0) || !d_n_bad || !aligned4(d_n_bad) ||
        !d_workspace || (n && (!d_starts || !d_roots32 || !d_status || (items_bytes && !d_items))) ||
        !aligned4(d_roots32) || ((uintptr_t)d_starts & 7))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    Bump b(d_workspace, bls381_ssz_ragged_roots_workspace_size(n));
    return ragged_roots_impl(n, d_items, items_bytes, d_starts, h_prog, prog_len, d_roots32, d_status, d_n_bad,
                             carve_ssz(b), (hipStream_t)stream, c);
  });
}

int bls381_ssz_ragged_roots(size_t n, const uint8_t* items, const uint64_t* starts, const uint32_t* prog,
                            uint32_t prog_len, uint8_t* roots32, uint8_t* status) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !ssz_ragged_prog_ok(prog, prog_len, 0) || (n && (!starts || !roots32 || !status)) ||
        (n && !ragged_starts_ok(n, starts)) || (n && starts[n] != starts[0] && !items))
      return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t bytes = (size_t)starts[n];
    uint8_t *d_items, *d_roots, *d_status;
    uint64_t* d_starts;
    uint32_t* d_bad;
    SszWs w;
    TRY(hc.carve([&](Bump& b) {
      d_items = b.take<uint8_t>(bytes);
      d_starts = b.take<uint64_t>(n + 1);
      d_roots = b.take<uint8_t>(32 * n);
      d_status = b.take<uint8_t>(n);
      d_bad = b.take<uint32_t>(1);
      w = carve_ssz(b);
    }));
    TRY(hc.upload(d_items, items, bytes));
    TRY(hc.upload(d_starts, starts, 8 * (n + 1)));
    TRY(ragged_roots_impl(n, d_items, bytes, d_starts, prog, prog_len, d_roots, d_status, d_bad, w, hc.s, c));
    TRY(hc.download(roots32, d_roots, 32 * n));
    TRY(hc.download(status, d_status, n));
    return hc.finish();
  });
}

// hash_tree_root of a List / Vector of n variable-size elements: their roots, then the tiled tree
// and the finish of bls381_ssz_list_root.  The launches depend on n alone.
struct RaggedListWs {
  uint8_t *roots, *status;
  SszWs ssz;
  MerkleWs merkle;
};
static RaggedListWs carve_ragged_list(Bump& b, const MerklePlan& p) {
  RaggedListWs w;
  w.roots = b.take<uint8_t>(32 * (size_t)p.n);
  w.status = b.take<uint8_t>((size_t)p.n);
  w.ssz = carve_ssz(b);
  w.merkle = carve_merkle(b, p.node_bytes);
  return w;
}
size_t bls381_ssz_ragged_list_root_workspace_size(size_t n) {
  if (n > (size_t)INT32_MAX) return 0;
  const MerklePlan p = plan_merkle(n, 0, merkle_chunk_depth(n), false);
  return carved_bytes([&](Bump& b) { carve_ragged_list(b, p); });
}

int bls381_ssz_ragged_list_root_device(size_t n, const uint8_t* d_items, size_t items_bytes, const uint64_t* d_starts,
                                       const uint32_t* h_prog, uint32_t prog_len, int mix_length, uint8_t* d_root32,
                                       uint32_t* d_n_bad, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !ssz_ragged_prog_ok(h_prog, prog_len, 0) || !d_root32 || !aligned4(d_root32) ||
        !d_n_bad || !aligned4(d_n_bad) || !d_workspace || (n && (!d_starts || (items_bytes && !d_items))) ||
        ((uintptr_t)d_starts & 7))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MerklePlan p = plan_merkle(n, 0, merkle_chunk_depth(n), false);
    Bump b(d_workspace, bls381_ssz_ragged_list_root_workspace_size(n));
    const RaggedListWs w = carve_ragged_list(b, p);
    TRY(ragged_roots_impl(n, d_items, items_bytes, d_starts, h_prog, prog_len, w.roots, w.status, d_n_bad, w.ssz, s, c));
    return merkle_tree_impl(c, p, w.roots, w.merkle, mix_length, n, d_root32, s);
  });
}

int bls381_ssz_ragged_list_root(size_t n, const uint8_t* items, const uint64_t* starts, const uint32_t* prog,
                                uint32_t prog_len, int mix_length, uint8_t root[32], uint32_t* n_bad) {
  return guarded([&]() -> int {
    if (n > (size_t)INT32_MAX || !ssz_ragged_prog_ok(prog, prog_len, 0) || !root || (n && !starts) ||
        (n && !ragged_starts_ok(n, starts)) || (n && starts[n] != starts[0] && !items))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t bytes = n ? (size_t)starts[n] : 0, wsb = bls381_ssz_ragged_list_root_workspace_size(n);
    uint8_t *d_items, *d_root, *d_ws;
    uint64_t* d_starts;
    uint32_t* d_bad;
    TRY(hc.carve([&](Bump& b) {
      d_items = b.take<uint8_t>(bytes);
      d_starts = b.take<uint64_t>(n + 1);
      d_root = b.take<uint8_t>(32);
      d_bad = b.take<uint32_t>(1);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_items, items, bytes));
    if (n) TRY(hc.upload(d_starts, starts, 8 * (n + 1)));
    TRY(bls381_ssz_ragged_list_root_device(n, d_items, bytes, d_starts, prog, prog_len, mix_length, d_root, d_bad, d_ws,
                                           hc.s));
    uint32_t bad = 0;
    uint8_t r[32];
    TRY(hc.download(r, d_root, 32));
    TRY(hc.download(&bad, d_bad, 4));
    TRY(hc.finish());
    if (n_bad) *n_bad = bad;
    if (bad) return BLS381_EARG;   // a malformed item: the root is not the list's, and is not handed out
    memcpy(root, r, 32);
    return 0;
  });
}

// n DepositData -> n Deposits under one root: the leaves hash_tree_root(data), the depth-32 tree
// with every level kept, each leaf's proof written into its Deposit, the data copied behind it
struct DepositsBuildWs {
  uint8_t* leaves;
  SszWs ssz;
  MerkleWs merkle;
};
// (the rows' sizes depend on first_index, by at most one node per level: merkle_node_bound)
static DepositsBuildWs carve_deposits_build(Bump& b, size_t n) {
  DepositsBuildWs w;
  w.leaves = b.take<uint8_t>(32 * n);
  w.ssz = carve_ssz(b);
  w.merkle = carve_merkle(b, merkle_node_bound(n, DEPOSIT_PROOF_DEPTH));
  return w;
}
size_t bls381_deposits_build_workspace_size(size_t n) {
  if (n > (size_t)INT32_MAX) return 0;
  return carved_bytes([&](Bump& b) { carve_deposits_build(b, n); });
}

int bls381_deposits_build_device(size_t n, const uint8_t* d_deposit_data, uint64_t first_index, uint8_t* d_deposits,
                                 uint8_t* d_deposit_root32, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!merkle_args_in_range(n, first_index, DEPOSIT_PROOF_DEPTH) || !d_deposit_root32 || !d_workspace ||
        (n && (!d_deposit_data || !d_deposits)) || !aligned4(d_deposits))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const MerklePlan p = plan_merkle(n, first_index, DEPOSIT_PROOF_DEPTH, true);
    Bump b(d_workspace, bls381_deposits_build_workspace_size(n));
    const DepositsBuildWs w = carve_deposits_build(b, n);
    if (n)
      TRY(ssz_root_impl(n, d_deposit_data, DEPOSIT_DATA_BYTES, DEPOSIT_ROOT_PROG, DEPOSIT_ROOT_PROG_LEN, w.leaves,
                        w.ssz, s, c));
    TRY(merkle_tree_impl(c, p, w.leaves, w.merkle, 0, 0, d_deposit_root32, s));
    TRY(merkle_proofs_impl(c, p, w.leaves, w.merkle, n, nullptr, first_index, d_deposits, DEPOSIT_BYTES, s));
    LAUNCH("deposit_data_copy", s, dim3(grid_for(DEPOSIT_DATA_BYTES * n)), dim3(KBLOCK), k_scatter_field, n,
           d_deposit_data, (uint32_t)DEPOSIT_DATA_BYTES, d_deposits, DEPOSIT_BYTES, (uint32_t)DEPOSIT_PROOF_BYTES);
    return 0;
  });
}

int bls381_deposits_build(size_t n, const uint8_t* deposit_data, uint64_t first_index, uint8_t* deposits,
                          uint8_t deposit_root[32]) {
  return guarded([&]() -> int {
    if (!merkle_args_in_range(n, first_index, DEPOSIT_PROOF_DEPTH) || !deposit_root ||
        (n && (!deposit_data || !deposits)))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_deposits_build_workspace_size(n);
    uint8_t *d_data, *d_dep, *d_root, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_data = b.take<uint8_t>(DEPOSIT_DATA_BYTES * n);
      d_dep = b.take<uint8_t>(DEPOSIT_BYTES * n);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_data, deposit_data, DEPOSIT_DATA_BYTES * n));
    TRY(bls381_deposits_build_device(n, d_data, first_index, d_dep, d_root, d_ws, hc.s));
    TRY(hc.download(deposits, d_dep, DEPOSIT_BYTES * n));
    TRY(hc.download(deposit_root, d_root, 32));
    return hc.finish();
  });
}

// ---- the deposit tree kept on the device (storage and rules: bls381_deptree.hpp)
// `count` is the host's: it moves when an append is queued, and every query checks against it.
struct bls381_deposit_tree {
  int device = -1;
  deptree_shape sh{};
  uint64_t count = 0;
  uint8_t* store = nullptr;
};

int bls381_deposit_tree_create(size_t capacity, uint32_t depth, bls381_deposit_tree** out) {
  if (!out) return BLS381_EARG;
  *out = nullptr;
  if (!deptree_args_ok(capacity, depth)) return BLS381_EARG;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  std::unique_ptr<bls381_deposit_tree> t(new bls381_deposit_tree());
  uint64_t bytes = 0;
  t->device = c->device;
  t->sh = deptree_make_shape(capacity, depth, &bytes);
  if (hipMalloc(&t->store, bytes) != hipSuccess) {
    (void)hipGetLastError();
    t_err = "deposit tree allocation failed";
    return BLS381_EHIP;
  }
  *out = t.release();
  return 0;
}

void bls381_deposit_tree_destroy(bls381_deposit_tree* tree) {
  if (!tree) return;
  (void)hipSetDevice(tree->device);
  (void)hipDeviceSynchronize();   // calls queued on the caller's streams may still read the store
  (void)hipFree(tree->store);
  delete tree;
}

size_t bls381_deposit_tree_count(const bls381_deposit_tree* tree) { return tree ? (size_t)tree->count : 0; }
size_t bls381_deposit_tree_capacity(const bls381_deposit_tree* tree) { return tree ? (size_t)tree->sh.capacity : 0; }

static Ctx* deptree_ctx(const bls381_deposit_tree* tree, int* rc) {
  Ctx* c = get_ctx(rc);
  if (c && c->device != tree->device) { t_err = "deposit tree belongs to another device"; *rc = BLS381_EARG; return nullptr; }
  return c;
}
static bool deptree_fits(const bls381_deposit_tree* tree, size_t n) {
  return n <= tree->sh.capacity - tree->count;
}
static uint8_t* deptree_leaf_row(bls381_deposit_tree* tree) { return tree->store + 32 * tree->count; }

// Queues the passes of an append of n leaves that already sit in row 0 behind the count, then moves the count.
static int deptree_append_impl(Ctx* c, bls381_deposit_tree* tree, size_t n, hipStream_t s) {
  const deptree_levels lv{tree->sh, tree->count, tree->count + n};
  for (const merkle_pass& ps : deptree_append_plan(tree->sh, tree->count, n))
    LAUNCH("deptree_append", s, dim3((unsigned)ps.tiles), dim3(MERKLE_TILE / 2), k_deptree_append, tree->store, lv,
           (const uint8_t*)c->ztab, ps.h0, ps.steps, ps.tile0);
  tree->count += n;
  return 0;
}

int bls381_deposit_tree_append_device(bls381_deposit_tree* tree, size_t n, const uint8_t* d_leaves32, void* stream) {
  return guarded([&]() -> int {
    if (!tree || !deptree_fits(tree, n) || (n && !d_leaves32) || !aligned4(d_leaves32)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemcpyAsync(deptree_leaf_row(tree), d_leaves32, 32 * n, hipMemcpyDeviceToDevice, s));
    return deptree_append_impl(c, tree, n, s);
  });
}

int bls381_deposit_tree_append(bls381_deposit_tree* tree, size_t n, const uint8_t* leaves32) {
  return guarded([&]() -> int {
    if (!tree || !deptree_fits(tree, n) || (n && !leaves32)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    TRY(hc.upload(deptree_leaf_row(tree), leaves32, 32 * n));
    TRY(deptree_append_impl(c, tree, n, hc.s));
    return hc.finish();
  });
}

size_t bls381_deposit_tree_append_data_workspace_size(size_t n) {
  return n > (size_t)INT32_MAX ? 0 : bls381_ssz_root_workspace_size();
}

// the leaves hash_tree_root(DepositData) written straight into row 0
int bls381_deposit_tree_append_data_device(bls381_deposit_tree* tree, size_t n, const uint8_t* d_deposit_data,
                                           void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!tree || n > (size_t)INT32_MAX || !deptree_fits(tree, n) || (n && (!d_deposit_data || !d_workspace)))
      return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_ssz_root_workspace_size());
    TRY(ssz_root_impl(n, d_deposit_data, DEPOSIT_DATA_BYTES, DEPOSIT_ROOT_PROG, DEPOSIT_ROOT_PROG_LEN,
                      deptree_leaf_row(tree), carve_ssz(b), s, c));
    return deptree_append_impl(c, tree, n, s);
  });
}

int bls381_deposit_tree_append_data(bls381_deposit_tree* tree, size_t n, const uint8_t* deposit_data) {
  return guarded([&]() -> int {
    if (!tree || n > (size_t)INT32_MAX || !deptree_fits(tree, n) || (n && !deposit_data)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t *d_data, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_data = b.take<uint8_t>(DEPOSIT_DATA_BYTES * n);
      d_ws = b.take<uint8_t>(bls381_deposit_tree_append_data_workspace_size(n));
    }));
    TRY(hc.upload(d_data, deposit_data, DEPOSIT_DATA_BYTES * n));
    TRY(bls381_deposit_tree_append_data_device(tree, n, d_data, d_ws, hc.s));
    return hc.finish();
  });
}

static bool deptree_counts_ok(const bls381_deposit_tree* tree, size_t m, const uint64_t* counts) {
  for (size_t q = 0; q < m; ++q)
    if (counts[q] > tree->count) return false;
  return true;
}

int bls381_deposit_tree_roots_device(bls381_deposit_tree* tree, size_t m, const uint64_t* h_counts, uint8_t* d_roots32,
                                     void* stream) {
  return guarded([&]() -> int {
    if (!tree || m > (size_t)INT32_MAX || (m && (!h_counts || !d_roots32)) || !aligned4(d_roots32) ||
        !deptree_counts_ok(tree, m, h_counts))
      return BLS381_EARG;
    if (m == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    // the counts travel as kernel arguments, DEPTREE_ROOTS_CHUNK a launch: nothing to keep alive
    for (size_t q0 = 0; q0 < m; q0 += DEPTREE_ROOTS_CHUNK) {
      const uint32_t mm = (uint32_t)std::min<size_t>(DEPTREE_ROOTS_CHUNK, m - q0);
      deptree_counts ck{};
      for (uint32_t q = 0; q < mm; ++q) ck.k[q] = (uint32_t)h_counts[q0 + q];
      LAUNCH("deptree_roots", (hipStream_t)stream, dim3(grid_for(mm, 64)), dim3(64), k_deptree_roots, mm, ck,
             (const uint8_t*)tree->store, tree->sh, (const uint8_t*)c->ztab, d_roots32 + 32 * q0);
    }
    return 0;
  });
}

int bls381_deposit_tree_roots(bls381_deposit_tree* tree, size_t m, const uint64_t* counts, uint8_t* roots32) {
  return guarded([&]() -> int {
    if (!tree || m > (size_t)INT32_MAX || (m && (!counts || !roots32)) || !deptree_counts_ok(tree, m, counts))
      return BLS381_EARG;
    if (m == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t* d_roots;
    TRY(hc.carve([&](Bump& b) { d_roots = b.take<uint8_t>(32 * m); }));
    TRY(bls381_deposit_tree_roots_device(tree, m, counts, d_roots, hc.s));
    TRY(hc.download(roots32, d_roots, 32 * m));
    return hc.finish();
  });
}

// the workspace of a proofs query: P[0 .. depth]
size_t bls381_deposit_tree_proofs_workspace_size(uint32_t depth) {
  if (depth == 0 || depth > DEPTREE_DEPTH_MAX) return 0;
  return carved_bytes([&](Bump& b) { b.take<uint8_t>(32 * (size_t)(depth + 1)); });
}

// the P chain of count k into the workspace and d_root, then the siblings
static int deptree_proofs_impl(Ctx* c, const bls381_deposit_tree* tree, uint64_t k, size_t n_idx,
                               const uint64_t* d_indices, uint64_t index_base, uint8_t* d_proofs, size_t stride,
                               uint8_t* d_root, void* ws, hipStream_t s) {
  Bump b(ws, bls381_deposit_tree_proofs_workspace_size(tree->sh.depth));
  uint8_t* ptab = b.take<uint8_t>(32 * (size_t)(tree->sh.depth + 1));
  LAUNCH("deptree_chain", s, dim3(1), dim3(64), k_deptree_chain, k, (const uint8_t*)tree->store, tree->sh,
         (const uint8_t*)c->ztab, ptab, d_root);
  LAUNCH("deptree_gather", s, dim3(grid_for(n_idx * tree->sh.depth)), dim3(KBLOCK), k_deptree_gather, n_idx, d_indices,
         index_base, k, (const uint8_t*)tree->store, tree->sh, (const uint8_t*)ptab, (const uint8_t*)c->ztab, d_proofs,
         stride);
  return 0;
}
static bool deptree_proofs_args_ok(const bls381_deposit_tree* tree, uint64_t k, size_t n_idx, const void* indices,
                                   const void* proofs, size_t proof_stride, const void* root) {
  if (!tree || k > tree->count || n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * tree->sh.depth) return false;
  return root && (n_idx == 0 || (indices && proofs));
}

int bls381_deposit_tree_proofs_device(bls381_deposit_tree* tree, uint64_t k, size_t n_idx, const uint64_t* d_indices,
                                      uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32, void* d_workspace,
                                      void* stream) {
  return guarded([&]() -> int {
    if (!deptree_proofs_args_ok(tree, k, n_idx, d_indices, d_proofs, proof_stride, d_root32) || !d_workspace ||
        !aligned4(d_proofs) || (proof_stride & 3) || ((uintptr_t)d_indices & 7))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    return deptree_proofs_impl(c, tree, k, n_idx, d_indices, 0, d_proofs, proof_stride, d_root32, d_workspace,
                               (hipStream_t)stream);
  });
}

int bls381_deposit_tree_proofs(bls381_deposit_tree* tree, uint64_t k, size_t n_idx, const uint64_t* indices,
                               uint8_t* proofs, size_t proof_stride, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (!deptree_proofs_args_ok(tree, k, n_idx, indices, proofs, proof_stride, root)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_deposit_tree_proofs_workspace_size(tree->sh.depth), row = (size_t)32 * tree->sh.depth;
    uint8_t *d_proofs, *d_root, *d_ws;
    uint64_t* d_idx;
    TRY(hc.carve([&](Bump& b) {
      d_idx = b.take<uint64_t>(n_idx);
      d_proofs = b.take<uint8_t>(row * n_idx);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_idx, indices, 8 * n_idx));
    TRY(bls381_deposit_tree_proofs_device(tree, k, n_idx, d_idx, d_proofs, row, d_root, d_ws, hc.s));
    // packed on the device; the caller's rows are proof_stride apart and only their proofs are written
    if (n_idx) HIPC(hipMemcpy2DAsync(proofs, proof_stride, d_proofs, row, row, n_idx, hipMemcpyDeviceToHost, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

// Deposits for leaves first_index .. first_index + n - 1 under the root at count k: each proof
// into its record, the data copied behind it.  The workspace: the root (unused by the caller),
// then the proofs query's own.
size_t bls381_deposit_tree_deposits_workspace_size(size_t n) {
  if (n > (size_t)INT32_MAX) return 0;
  return carved_bytes([&](Bump& b) {
    b.take<uint8_t>(32);
    b.take<uint8_t>(bls381_deposit_tree_proofs_workspace_size(DEPOSIT_PROOF_DEPTH));
  });
}
static bool deptree_deposits_args_ok(const bls381_deposit_tree* tree, uint64_t k, uint64_t first_index, size_t n,
                                     const void* data, const void* deposits) {
  if (!tree || tree->sh.depth != DEPOSIT_PROOF_DEPTH || n > (size_t)INT32_MAX || k > tree->count) return false;
  return first_index <= k && n <= k - first_index && (n == 0 || (data && deposits));
}

int bls381_deposit_tree_deposits_device(bls381_deposit_tree* tree, uint64_t k, uint64_t first_index, size_t n,
                                        const uint8_t* d_deposit_data, uint8_t* d_deposits, void* d_workspace,
                                        void* stream) {
  return guarded([&]() -> int {
    if (!deptree_deposits_args_ok(tree, k, first_index, n, d_deposit_data, d_deposits) || !d_workspace ||
        !aligned4(d_deposits))
      return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_deposit_tree_deposits_workspace_size(n));
    uint8_t* d_root = b.take<uint8_t>(32);
    void* ws = b.take<uint8_t>(bls381_deposit_tree_proofs_workspace_size(DEPOSIT_PROOF_DEPTH));
    TRY(deptree_proofs_impl(c, tree, k, n, nullptr, first_index, d_deposits, DEPOSIT_BYTES, d_root, ws, s));
    LAUNCH("deposit_data_copy", s, dim3(grid_for(DEPOSIT_DATA_BYTES * n)), dim3(KBLOCK), k_scatter_field, n,
           d_deposit_data, (uint32_t)DEPOSIT_DATA_BYTES, d_deposits, DEPOSIT_BYTES, (uint32_t)DEPOSIT_PROOF_BYTES);
    return 0;
  });
}

int bls381_deposit_tree_deposits(bls381_deposit_tree* tree, uint64_t k, uint64_t first_index, size_t n,
                                 const uint8_t* deposit_data, uint8_t* deposits) {
  return guarded([&]() -> int {
    if (!deptree_deposits_args_ok(tree, k, first_index, n, deposit_data, deposits)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = deptree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t *d_data, *d_dep, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_data = b.take<uint8_t>(DEPOSIT_DATA_BYTES * n);
      d_dep = b.take<uint8_t>(DEPOSIT_BYTES * n);
      d_ws = b.take<uint8_t>(bls381_deposit_tree_deposits_workspace_size(n));
    }));
    TRY(hc.upload(d_data, deposit_data, DEPOSIT_DATA_BYTES * n));
    TRY(bls381_deposit_tree_deposits_device(tree, k, first_index, n, d_data, d_dep, d_ws, hc.s));
    TRY(hc.download(deposits, d_dep, DEPOSIT_BYTES * n));
    return hc.finish();
  });
}

// ---- SSZ list trees kept on the device (storage and rules: bls381_listtree.hpp)
// `count` is the host's: it moves when an append is queued.  The root program lives beside the store.
struct bls381_list_tree {
  int device = -1;
  listtree_shape sh{};
  uint64_t count = 0;
  uint8_t* store = nullptr;
  uint32_t* prog = nullptr;   // device copy; null for a packed list
  uint32_t plen = 0;
};

int bls381_list_tree_create(size_t capacity, size_t item_size, const uint32_t* prog, uint32_t prog_len,
                            bls381_list_tree** out) {
  if (!out) return BLS381_EARG;
  *out = nullptr;
  const bool packed = !prog && prog_len == 0;
  if (!listtree_args_ok(capacity, item_size, packed) || (!packed && !ssz_prog_ok(prog, prog_len, item_size)))
    return BLS381_EARG;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  std::unique_ptr<bls381_list_tree> t(new bls381_list_tree());
  uint64_t bytes = 0;
  t->device = c->device;
  t->sh = listtree_make_shape(capacity, (uint32_t)item_size, packed, &bytes);
  t->plen = prog_len;
  bool ok = hipMalloc(&t->store, bytes) == hipSuccess && hipMemset(t->store, 0, bytes) == hipSuccess;
  if (ok && !packed)
    ok = hipMalloc(&t->prog, 4 * (size_t)prog_len) == hipSuccess &&
         hipMemcpy(t->prog, prog, 4 * (size_t)prog_len, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok || hipDeviceSynchronize() != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(t->store);
    (void)hipFree(t->prog);
    t_err = "list tree allocation failed";
    return BLS381_EHIP;
  }
  *out = t.release();
  return 0;
}

void bls381_list_tree_destroy(bls381_list_tree* tree) {
  if (!tree) return;
  (void)hipSetDevice(tree->device);
  (void)hipDeviceSynchronize();   // calls queued on the caller's streams may still read the store
  (void)hipFree(tree->store);
  (void)hipFree(tree->prog);
  delete tree;
}

static uint64_t listtree_chunks_now(const bls381_list_tree* tree) { return listtree_chunks(tree->sh, tree->count); }
size_t bls381_list_tree_count(const bls381_list_tree* tree) { return tree ? (size_t)tree->count : 0; }
size_t bls381_list_tree_capacity(const bls381_list_tree* tree) { return tree ? (size_t)tree->sh.capacity : 0; }
uint32_t bls381_list_tree_depth(const bls381_list_tree* tree) {
  return tree ? merkle_chunk_depth(listtree_chunks_now(tree)) : 0;
}
const uint8_t* bls381_list_tree_items_device(const bls381_list_tree* tree) { return tree ? tree->store : nullptr; }

static Ctx* listtree_ctx(const bls381_list_tree* tree, int* rc) {
  Ctx* c = get_ctx(rc);
  if (c && c->device != tree->device) { t_err = "list tree belongs to another device"; *rc = BLS381_EARG; return nullptr; }
  return c;
}
static bool listtree_fits(const bls381_list_tree* tree, size_t n) { return n <= tree->sh.capacity - tree->count; }
static uint8_t* listtree_item(bls381_list_tree* tree, uint64_t i) { return tree->store + i * tree->sh.item_size; }

int bls381_list_tree_read(bls381_list_tree* tree, size_t first, size_t n, uint8_t* items_out) {
  return guarded([&]() -> int {
    if (!tree || first > tree->count || n > tree->count - first || (n && !items_out)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    TRY(hc.download(items_out, listtree_item(tree, first), n * tree->sh.item_size));
    return hc.finish();
  });
}

// the workspace of an append: the root program's error flag (composite lists)
size_t bls381_list_tree_append_workspace_size(const bls381_list_tree* tree, size_t n) {
  if (!tree || n == 0 || !listtree_fits(tree, n) || tree->sh.packed) return 0;
  return carved_bytes([&](Bump& b) { b.take<int32_t>(1); });
}

// Queues the re-hash of n items that already sit in the store behind the count -- composite: their
// roots into row 0; then the passes over the contiguous tiles of their chunks (a packed append
// that starts inside a chunk takes that chunk along) -- and moves the count.
static int listtree_append_impl(Ctx* c, bls381_list_tree* tree, size_t n, void* ws, hipStream_t s) {
  const listtree_shape& sh = tree->sh;
  const uint64_t c0 = listtree_chunk_of(sh, tree->count), c1 = listtree_chunks(sh, tree->count + n);
  if (!sh.packed) {
    Bump b(ws, bls381_list_tree_append_workspace_size(tree, n));
    int32_t* err = b.take<int32_t>(1);
    HIPC(hipMemsetAsync(err, 0, 4, s));
    LAUNCH("listtree_leaves", s, dim3(grid_for(n)), dim3(KBLOCK), k_ssz_root, n, (const uint8_t*)listtree_item(tree, tree->count),
           (size_t)sh.item_size, (const uint32_t*)tree->prog, tree->plen, tree->store + sh.off[0] + 32 * tree->count, err);
  }
  const listtree_levels lv{sh, c1};
  for (const merkle_pass& ps : listtree_range_plan(sh, c0, c1))
    LAUNCH("listtree_reduce", s, dim3((unsigned)ps.tiles), dim3(MERKLE_TILE / 2), k_listtree_reduce, tree->store, lv,
           (const uint8_t*)c->ztab, ps.h0, ps.steps, ps.tile0, (const uint32_t*)nullptr, (const uint32_t*)nullptr);
  tree->count += n;
  return 0;
}

int bls381_list_tree_append_device(bls381_list_tree* tree, size_t n, const uint8_t* d_items, void* d_workspace,
                                   void* stream) {
  return guarded([&]() -> int {
    if (!tree || !listtree_fits(tree, n) || (n && !d_items) ||
        (bls381_list_tree_append_workspace_size(tree, n) && !d_workspace))
      return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemcpyAsync(listtree_item(tree, tree->count), d_items, n * tree->sh.item_size, hipMemcpyDeviceToDevice, s));
    return listtree_append_impl(c, tree, n, d_workspace, s);
  });
}

int bls381_list_tree_append(bls381_list_tree* tree, size_t n, const uint8_t* items) {
  return guarded([&]() -> int {
    if (!tree || !listtree_fits(tree, n) || (n && !items)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t* d_ws = nullptr;
    TRY(hc.carve([&](Bump& b) { d_ws = b.take<uint8_t>(bls381_list_tree_append_workspace_size(tree, n)); }));
    TRY(hc.upload(listtree_item(tree, tree->count), items, n * tree->sh.item_size));
    TRY(listtree_append_impl(c, tree, n, d_ws, hc.s));
    return hc.finish();
  });
}

// the workspace of an update: flag rows, tile lists and their lengths (listtree_update_layout)
size_t bls381_list_tree_update_workspace_size(const bls381_list_tree* tree, size_t n_upd) {
  if (!tree || n_upd == 0 || n_upd > (size_t)INT32_MAX) return 0;
  if (tree->sh.packed && listtree_passes(tree->sh) == 0) return 0;
  return align256(4 * (size_t)listtree_update_layout(tree->sh, n_upd).words);
}

// launches of an update, whatever n_upd is: the scatter, [composite: the leaves], and, in a tree
// with P = listtree_passes() > 0 passes, the mark, the compaction and the P passes
int bls381_list_tree_update_device(bls381_list_tree* tree, size_t n_upd, const uint32_t* d_indices, size_t off,
                                   size_t len, const uint8_t* d_values, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!tree || n_upd > (size_t)INT32_MAX || off > tree->sh.item_size || len > tree->sh.item_size - off)
      return BLS381_EARG;
    if (n_upd == 0 || len == 0) return 0;
    if (!d_indices || !d_values || ((uintptr_t)d_indices & 3) ||
        (bls381_list_tree_update_workspace_size(tree, n_upd) && !d_workspace))
      return BLS381_EARG;
    if (tree->count == 0) return 0;   // every index is at or above the count
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const listtree_shape& sh = tree->sh;
    const uint64_t chunks = listtree_chunks_now(tree);
    const listtree_update_ws w = listtree_update_layout(sh, n_upd);
    uint32_t* ws = (uint32_t*)d_workspace;
    LAUNCH("listtree_scatter", s, dim3(grid_for(n_upd * len)), dim3(KBLOCK), k_listtree_scatter, n_upd, d_indices,
           d_values, (uint32_t)off, (uint32_t)len, tree->store, sh, tree->count);
    if (!sh.packed) {
      int32_t* err = (int32_t*)(ws + w.err);
      HIPC(hipMemsetAsync(err, 0, 4, s));
      LAUNCH("listtree_leaves_idx", s, dim3(grid_for(n_upd)), dim3(KBLOCK), k_listtree_leaves, n_upd, d_indices,
             tree->store, sh, tree->count, (const uint32_t*)tree->prog, tree->plen, err);
    }
    if (w.passes == 0) return 0;
    const listtree_marks m = listtree_make_marks(w, chunks);
    HIPC(hipMemsetAsync(ws, 0, 4 * (size_t)w.flag_words, s));
    LAUNCH("listtree_mark", s, dim3(grid_for(n_upd)), dim3(KBLOCK), k_listtree_mark, n_upd, d_indices, sh, tree->count,
           m, ws);
    LAUNCH("listtree_compact", s, dim3(w.passes), dim3(LISTTREE_COMPACT_LANES), k_listtree_compact, m, ws);
    const listtree_levels lv{sh, chunks};
    for (uint32_t k = 0; k < w.passes; ++k) {
      const uint32_t h0 = k * MERKLE_TILE_LOG;
      LAUNCH("listtree_reduce", s, dim3((unsigned)std::min<uint64_t>(n_upd, m.tiles[k])), dim3(MERKLE_TILE / 2),
             k_listtree_reduce, tree->store, lv, (const uint8_t*)c->ztab, h0, std::min(MERKLE_TILE_LOG, sh.top - h0),
             (uint64_t)0, (const uint32_t*)(ws + m.list[k]), (const uint32_t*)(ws + m.lens + k));
    }
    return 0;
  });
}

int bls381_list_tree_update(bls381_list_tree* tree, size_t n_upd, const uint32_t* indices, size_t off, size_t len,
                            const uint8_t* values) {
  return guarded([&]() -> int {
    if (!tree || n_upd > (size_t)INT32_MAX || off > tree->sh.item_size || len > tree->sh.item_size - off)
      return BLS381_EARG;
    if (n_upd == 0 || len == 0) return 0;
    if (!indices || !values) return BLS381_EARG;
    for (size_t t = 0; t < n_upd; ++t)
      if (indices[t] >= tree->count) return BLS381_EARG;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    // repeated indices are applied in order: the last one wins, the earlier ones are dropped here
    std::vector<uint32_t> idx;
    std::vector<uint8_t> vals;
    {
      std::unordered_set<uint32_t> seen;
      std::vector<size_t> keep;
      for (size_t t = n_upd; t-- > 0;)
        if (seen.insert(indices[t]).second) keep.push_back(t);
      idx.reserve(keep.size());
      vals.reserve(keep.size() * len);
      for (size_t q = keep.size(); q-- > 0;) {
        idx.push_back(indices[keep[q]]);
        vals.insert(vals.end(), values + keep[q] * len, values + (keep[q] + 1) * len);
      }
    }
    const size_t m = idx.size();
    HostCall hc(c);
    uint32_t* d_idx;
    uint8_t *d_vals, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_idx = b.take<uint32_t>(m);
      d_vals = b.take<uint8_t>(m * len);
      d_ws = b.take<uint8_t>(bls381_list_tree_update_workspace_size(tree, m));
    }));
    TRY(hc.upload(d_idx, idx.data(), 4 * m));
    TRY(hc.upload(d_vals, vals.data(), m * len));
    TRY(bls381_list_tree_update_device(tree, m, d_idx, off, len, d_vals, d_ws, hc.s));
    return hc.finish();   // idx and vals outlive the copies: finish() synchronises
  });
}

// node (d, 0) -- the item bytes of a packed list with one chunk, Z[0] of an empty list -- with
// the optional mix_in_length(count): k_merkle_finish with nothing left to fold
static int listtree_root_impl(Ctx* c, const bls381_list_tree* tree, int mix, uint8_t* d_root, hipStream_t s) {
  const uint32_t d = bls381_list_tree_depth(tree);
  const uint8_t* node = tree->count ? tree->store + tree->sh.off[d] : nullptr;
  LAUNCH("listtree_root", s, dim3(1), dim3(64), k_merkle_finish, node, (uint8_t*)nullptr, (const merkle_level*)nullptr,
         (const uint8_t*)c->ztab, d, d, (uint64_t)0, mix, tree->count, d_root);
  return 0;
}

int bls381_list_tree_root_device(bls381_list_tree* tree, int mix_length, uint8_t* d_root32, void* stream) {
  return guarded([&]() -> int {
    if (!tree || !d_root32 || !aligned4(d_root32)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    return listtree_root_impl(c, tree, mix_length, d_root32, (hipStream_t)stream);
  });
}

int bls381_list_tree_root(bls381_list_tree* tree, int mix_length, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (!tree || !root) return BLS381_EARG;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    uint8_t* d_root;
    TRY(hc.carve([&](Bump& b) { d_root = b.take<uint8_t>(32); }));
    TRY(listtree_root_impl(c, tree, mix_length, d_root, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

static bool listtree_proofs_args_ok(const bls381_list_tree* tree, size_t n_idx, const void* indices, const void* proofs,
                                    size_t proof_stride, const void* root) {
  if (!tree || n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * bls381_list_tree_depth(tree)) return false;
  return root && (n_idx == 0 || (indices && (proofs || bls381_list_tree_depth(tree) == 0)));
}

int bls381_list_tree_proofs_device(bls381_list_tree* tree, size_t n_idx, const uint64_t* d_chunk_indices,
                                   uint8_t* d_proofs, size_t proof_stride, uint8_t* d_root32, void* stream) {
  return guarded([&]() -> int {
    if (!listtree_proofs_args_ok(tree, n_idx, d_chunk_indices, d_proofs, proof_stride, d_root32) ||
        !aligned4(d_proofs) || !aligned4(d_root32) || (proof_stride & 3) || ((uintptr_t)d_chunk_indices & 7))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t d = bls381_list_tree_depth(tree);
    TRY(listtree_root_impl(c, tree, 0, d_root32, s));
    LAUNCH("listtree_proofs", s, dim3(grid_for(n_idx * d)), dim3(KBLOCK), k_listtree_proofs, n_idx, d_chunk_indices, d,
           listtree_chunks_now(tree), (const uint8_t*)tree->store, tree->sh, (const uint8_t*)c->ztab, d_proofs,
           proof_stride);
    return 0;
  });
}

int bls381_list_tree_proofs(bls381_list_tree* tree, size_t n_idx, const uint64_t* chunk_indices, uint8_t* proofs,
                            size_t proof_stride, uint8_t root[32]) {
  return guarded([&]() -> int {
    if (!listtree_proofs_args_ok(tree, n_idx, chunk_indices, proofs, proof_stride, root)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = listtree_ctx(tree, &rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t row = (size_t)32 * bls381_list_tree_depth(tree);
    uint8_t *d_proofs, *d_root;
    uint64_t* d_idx;
    TRY(hc.carve([&](Bump& b) {
      d_idx = b.take<uint64_t>(n_idx);
      d_proofs = b.take<uint8_t>(row * n_idx);
      d_root = b.take<uint8_t>(32);
    }));
    TRY(hc.upload(d_idx, chunk_indices, 8 * n_idx));
    TRY(bls381_list_tree_proofs_device(tree, n_idx, d_idx, d_proofs, row, d_root, hc.s));
    // packed on the device; the caller's rows are proof_stride apart and only their proofs are written
    if (row && n_idx)
      HIPC(hipMemcpy2DAsync(proofs, proof_stride, d_proofs, row, row, n_idx, hipMemcpyDeviceToHost, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

static_assert(BLS381_DEPOSIT_SKIPPED == DEP_SKIPPED && BLS381_DEPOSIT_NEW == DEP_NEW &&
                  BLS381_DEPOSIT_TOPUP == DEP_TOPUP && BLS381_DEPOSIT_BYTES == DEPOSIT_BYTES,
              "include/bls381.h and the kernels agree on the deposit constants");

// process_deposits' workspace: the gathered keys and signatures, the leaves and the signing roots,
// the replicated domain, the per-deposit verdicts / registry entries / winners, the batch-local key
// table, {first bad proof, NEW count}, the deposit root and the domain, and the root program's and
// the verify batch's own
struct ProcessDepositsWs {
  uint8_t *pks, *sigs, *leaves, *sroots, *doms, *verdicts, *proof_ok, *consts;
  int32_t *entry, *win;
  uint32_t *table, *meta;
  size_t slots;
  SszWs ssz;
  void* verify;
};
static ProcessDepositsWs carve_process_deposits(Bump& b, size_t n) {
  ProcessDepositsWs w;
  w.pks = b.take<uint8_t>(48 * n);
  w.sigs = b.take<uint8_t>(96 * n);
  w.leaves = b.take<uint8_t>(32 * n);
  w.sroots = b.take<uint8_t>(32 * n);
  w.doms = b.take<uint8_t>(8 * n);
  w.verdicts = b.take<uint8_t>(n);
  w.proof_ok = b.take<uint8_t>(n);
  w.consts = b.take<uint8_t>(40);
  w.entry = b.take<int32_t>(n);
  w.win = b.take<int32_t>(n);
  w.slots = deposit_table_slots(n);
  w.table = b.take<uint32_t>(w.slots);
  w.meta = b.take<uint32_t>(2);
  w.ssz = carve_ssz(b);
  w.verify = b.take<uint8_t>(verify_ws_size(n));
  return w;
}
size_t bls381_registry_process_deposits_workspace_size(size_t n) {
  return carved_bytes([&](Bump& b) { carve_process_deposits(b, n); });
}

// Both forms, with reg->mu held: everything on `s`, synchronised before the registry's size moves.
static int process_deposits_impl(Ctx* c, bls381_registry* reg, size_t n, const uint8_t* d_deposits,
                                 uint64_t first_index, const uint8_t* deposit_root, const uint8_t* dom8, int commit,
                                 uint8_t* d_outcome, int32_t* d_vidx, int64_t* first_bad_proof, void* ws,
                                 hipStream_t s) {
  Bump b(ws, bls381_registry_process_deposits_workspace_size(n));
  const ProcessDepositsWs w = carve_process_deposits(b, n);
  const dim3 g(grid_for(n)), blk(KBLOCK);
  const uint32_t mask = (uint32_t)(w.slots - 1);
  Held<std::vector<uint8_t>> consts(c->keep, s, std::vector<uint8_t>(40));
  std::memcpy(consts->data(), deposit_root, 32);
  std::memcpy(consts->data() + 32, dom8, 8);
  HIPC(hipMemcpyAsync(w.consts, consts->data(), 40, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(w.table, 0xFF, 4 * w.slots, s));
  HIPC(hipMemsetAsync(w.meta, 0xFF, 8, s));
  const uint8_t* d_data = d_deposits + DEPOSIT_PROOF_BYTES;
  LAUNCH("gather_pubkeys", s, dim3(grid_for(48 * n)), blk, k_gather_field, n, d_data, DEPOSIT_BYTES, 0u, 48u, w.pks);
  LAUNCH("gather_signatures", s, dim3(grid_for(96 * n)), blk, k_gather_field, n, d_data, DEPOSIT_BYTES, 88u, 96u,
         w.sigs);
  LAUNCH("gather_domain", s, dim3(grid_for(8 * n)), blk, k_gather_field, n, (const uint8_t*)w.consts, (size_t)0, 32u,
         8u, w.doms);
  // the spec's assert: the leaf hash_tree_root(deposit.data) under index first_index + i
  TRY(ssz_root_impl(n, d_data, DEPOSIT_BYTES, DEPOSIT_ROOT_PROG, DEPOSIT_ROOT_PROG_LEN, w.leaves, w.ssz, s, c));
  LAUNCH("merkle_branch", s, g, blk, k_merkle_branch, n, (const uint8_t*)w.leaves, d_deposits, DEPOSIT_BYTES,
         DEPOSIT_PROOF_DEPTH, (const uint64_t*)nullptr, first_index, (const uint8_t*)w.consts, (size_t)0, w.proof_ok,
         w.meta);
  // pubkey in validator_pubkeys, then the proof of possession of every deposit
  LAUNCH("registry_lookup", s, g, blk, k_reg_lookup, n, (const uint8_t*)w.pks, (const uint8_t*)reg->keys,
         (const uint32_t*)reg->table, reg->tmask, w.entry);
  TRY(ssz_root_impl(n, d_data, DEPOSIT_BYTES, DEPOSIT_SIGNING_PROG, DEPOSIT_SIGNING_PROG_LEN, w.sroots, w.ssz, s, c));
  TRY(run_verify_batch(c, n, w.pks, w.sroots, w.sigs, w.doms, w.verdicts, w.verify, s));
  // the in-order rule
  LAUNCH("deposit_insert", s, g, blk, k_deposit_insert, n, (const uint8_t*)w.pks, (const int32_t*)w.entry,
         (const uint8_t*)w.verdicts, w.table, mask);
  LAUNCH("deposit_resolve", s, g, blk, k_deposit_resolve, n, (const uint8_t*)w.pks, (const int32_t*)w.entry,
         (const uint32_t*)w.table, mask, d_outcome, w.win);
  LAUNCH("deposit_scan", s, dim3(1), blk, k_deposit_scan, n, (uint32_t)reg->size, (const uint8_t*)d_outcome,
         (const int32_t*)w.entry, (const int32_t*)w.win, d_vidx, w.meta + 1);
  uint32_t meta[2];
  HIPC(hipMemcpyAsync(meta, w.meta, 8, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  *first_bad_proof = meta[0] == REG_EMPTY ? -1 : (int64_t)meta[0];
  const size_t n_new = meta[1];
  if (*first_bad_proof >= 0) return 0;
  if (!commit || n_new == 0) return (int)n_new;
  if (reg->size + n_new > reg->cap) { t_err = "registry capacity exceeded"; return BLS381_EARG; }
  const size_t first = reg->size;
  LAUNCH("deposit_compact", s, g, blk, k_deposit_compact, n, (const uint8_t*)w.pks, (const uint8_t*)d_outcome,
         (const int32_t*)d_vidx, reg->cap, reg->keys);
  LAUNCH("registry_decode", s, dim3(grid_for(n_new)), blk, k_reg_decode, first, n_new, reg->cap,
         (const uint8_t*)reg->keys, reg->aff, reg->st);
  LAUNCH("registry_insert", s, dim3(grid_for(n_new)), blk, k_reg_insert, first, n_new, (const uint8_t*)reg->keys,
         (const uint8_t*)reg->st, reg->table, reg->tmask);
  HIPC(hipStreamSynchronize(s));
  reg->size += n_new;
  return (int)n_new;
}

static bool process_deposits_args_ok(const bls381_registry* reg, size_t n, const void* deposits,
                                     const uint8_t* deposit_root, const uint8_t* dom8, const void* outcome,
                                     const void* vidx, const int64_t* first_bad_proof) {
  if (!reg || !first_bad_proof || n > (size_t)INT32_MAX / 2) return false;
  return n == 0 || (deposits && deposit_root && dom8 && outcome && vidx);
}

int bls381_registry_process_deposits_device(bls381_registry* reg, size_t n, const uint8_t* d_deposits,
                                            uint64_t first_index, const uint8_t deposit_root[32],
                                            const uint8_t dom8[8], int commit, uint8_t* d_outcome,
                                            int32_t* d_validator_index, int64_t* first_bad_proof, void* d_workspace,
                                            void* stream) {
  return guarded([&]() -> int {
    if (!process_deposits_args_ok(reg, n, d_deposits, deposit_root, dom8, d_outcome, d_validator_index,
                                  first_bad_proof) || (n && !d_workspace))
      return BLS381_EARG;
    *first_bad_proof = -1;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    return process_deposits_impl(c, reg, n, d_deposits, first_index, deposit_root, dom8, commit, d_outcome,
                                 d_validator_index, first_bad_proof, d_workspace, (hipStream_t)stream);
  });
}

int bls381_registry_process_deposits(bls381_registry* reg, size_t n, const uint8_t* deposits, uint64_t first_index,
                                     const uint8_t deposit_root[32], const uint8_t dom8[8], int commit,
                                     uint8_t* outcome, int32_t* validator_index, int64_t* first_bad_proof) {
  return guarded([&]() -> int {
    if (!process_deposits_args_ok(reg, n, deposits, deposit_root, dom8, outcome, validator_index, first_bad_proof))
      return BLS381_EARG;
    *first_bad_proof = -1;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = registry_ctx(reg, &rc);
    if (!c) return rc;
    std::lock_guard<std::mutex> lr(reg->mu);
    HostCall hc(c);
    const size_t wsb = bls381_registry_process_deposits_workspace_size(n);
    uint8_t *d_dep, *d_out, *d_ws;
    int32_t* d_vi;
    TRY(hc.carve([&](Bump& b) {
      d_dep = b.take<uint8_t>(DEPOSIT_BYTES * n);
      d_out = b.take<uint8_t>(n);
      d_vi = b.take<int32_t>(n);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_dep, deposits, DEPOSIT_BYTES * n));
    const int n_new = process_deposits_impl(c, reg, n, d_dep, first_index, deposit_root, dom8, commit, d_out, d_vi,
                                            first_bad_proof, d_ws, hc.s);
    if (n_new < 0) return n_new;
    TRY(hc.download(outcome, d_out, n));
    TRY(hc.download(validator_index, d_vi, 4 * n));
    TRY(hc.finish());
    return n_new;
  });
}

// ---- committees: get_shuffled_index / compute_committee and convert_to_indexed
// BLS381_SHUFFLE_PATH (measurement knob): 1 = always the direct path, 2 = always the table path,
// 0 (default) = by the rule below
static int shuffle_path_knob() {
  static const int v = env_knob("BLS381_SHUFFLE_PATH", 0);
  return v;
}
// Direct (every position hashes its own source block each round: rounds * count hashes, `rounds`
// of them in sequence on each lane) only where the table (rounds * ceil(n / 256) hashes, all
// independent) is both more hashes and a long build: count <= ceil(n / 256) and a list of at least
// SHUFFLE_DIRECT_MIN_BLOCKS blocks.  Measured at 90 rounds (profiles/shuffle_bench.json, kernel
// ms, direct / table): a window of 64 takes 0.41 / 0.09 at n = 2^20, 0.41 / 0.17 at 2^22,
// 0.41 / 0.53 at 2^24 and 0.40 / 1.91 at 2^26 -- the direct path's time is its 90 hashes in
// sequence whatever the list, the table's grows with the list -- and the window
// count = ceil(n / 256) takes 0.51 / 0.09 at 2^20, 0.66 / 0.54 at 2^24 and 1.80 / 2.07 at 2^26.
constexpr size_t SHUFFLE_DIRECT_MIN_BLOCKS = 65536;   // n > 2^24 - 256
static bool shuffle_direct(uint64_t n, uint64_t count) {
  const int k = shuffle_path_knob();
  const size_t blocks = shuffle_blocks(n);
  return k == 1 || (k != 2 && blocks >= SHUFFLE_DIRECT_MIN_BLOCKS && count <= blocks);
}
struct ShuffleWs {
  uint32_t *pivots, *table;
};
static ShuffleWs carve_shuffle(Bump& b, uint64_t n, uint64_t count, uint32_t rounds) {
  ShuffleWs w;
  w.pivots = b.take<uint32_t>(SHUFFLE_ROUNDS_MAX + 1);
  w.table = shuffle_direct(n, count) ? nullptr : b.take<uint32_t>((size_t)rounds * shuffle_blocks(n) * 8);
  return w;
}
static bool shuffle_args_ok(uint64_t n, const uint8_t* seed, uint32_t rounds, uint64_t first, uint64_t count,
                            const void* out) {
  if (n > 0xFFFFFFFFull || rounds > SHUFFLE_ROUNDS_MAX || first > n || count > n - first) return false;
  return count == 0 || (seed && out);
}
size_t bls381_shuffle_workspace_size(uint64_t index_count, uint64_t count, uint32_t rounds) {
  if (index_count > 0xFFFFFFFFull || rounds > SHUFFLE_ROUNDS_MAX || count > index_count) return 0;
  return carved_bytes([&](Bump& b) { carve_shuffle(b, index_count, count, rounds); });
}

int bls381_shuffle_device(uint64_t index_count, const uint8_t seed[32], uint32_t rounds, uint64_t first,
                          uint64_t count, const uint32_t* d_indices, uint32_t* d_out, void* d_workspace,
                          void* stream) {
  return guarded([&]() -> int {
    if (!shuffle_args_ok(index_count, seed, rounds, first, count, d_out) || (count && !d_workspace))
      return BLS381_EARG;
    if (count == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_shuffle_workspace_size(index_count, count, rounds));
    const ShuffleWs w = carve_shuffle(b, index_count, count, rounds);
    const uint32_t n = (uint32_t)index_count, f = (uint32_t)first;
    const shuffle_seed sd = shuffle_seed_from_bytes(seed);
    const dim3 g(grid_for(count)), blk(KBLOCK);
    LAUNCH("shuffle_pivots", s, dim3(grid_for(rounds)), blk, k_shuffle_pivots, n, sd, rounds, w.pivots);
    if (w.table) {
      const size_t blocks = shuffle_blocks(n);
      LAUNCH("shuffle_table", s, dim3(grid_for((size_t)rounds * blocks)), blk, k_shuffle_table, sd, rounds, blocks, w.table);
      LAUNCH("shuffle_walk", s, g, blk, k_shuffle_walk, n, rounds, (const uint32_t*)w.pivots, (const uint32_t*)w.table,
             blocks, f, (size_t)count, d_indices, d_out);
    } else {
      LAUNCH("shuffle_direct", s, g, blk, k_shuffle_direct, n, sd, rounds, (const uint32_t*)w.pivots, f, (size_t)count,
             d_indices, d_out);
    }
    return 0;
  });
}

int bls381_shuffle(uint64_t index_count, const uint8_t seed[32], uint32_t rounds, uint64_t first, uint64_t count,
                   const uint32_t* indices, uint32_t* out) {
  return guarded([&]() -> int {
    if (!shuffle_args_ok(index_count, seed, rounds, first, count, out)) return BLS381_EARG;
    if (count == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_shuffle_workspace_size(index_count, count, rounds);
    uint32_t *d_idx = nullptr, *d_out;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      if (indices) d_idx = b.take<uint32_t>(index_count);
      d_out = b.take<uint32_t>(count);
      d_ws = b.take<uint8_t>(wsb);
    }));
    if (indices) TRY(hc.upload(d_idx, indices, 4 * index_count));
    TRY(bls381_shuffle_device(index_count, seed, rounds, first, count, d_idx, d_out, d_ws, hc.s));
    TRY(hc.download(out, d_out, 4 * count));
    return hc.finish();
  });
}

// the attesting-entries workspace: one descriptor per attestation and both bitfield buffers
struct AttWs {
  att_desc* desc;
  uint8_t *agg, *cust;
};
static AttWs carve_att(Bump& b, size_t n_att, size_t bitfield_bytes) {
  AttWs w;
  w.desc = b.take<att_desc>(n_att);
  w.agg = b.take<uint8_t>(bitfield_bytes + 1);
  w.cust = b.take<uint8_t>(bitfield_bytes + 1);
  return w;
}
size_t bls381_attesting_entries_workspace_size(size_t n_att, size_t bitfield_bytes) {
  return carved_bytes([&](Bump& b) { carve_att(b, n_att, bitfield_bytes); });
}

// The host half of both forms: verify_bitfield and the popcounts.  Fills h_ok, h_group_key_off and
// desc; EARG for a committee outside the shuffled list or over MAX_INDICES_PER_ATTESTATION,
// descending bit offsets, or more members than entries_cap.
static int att_plan(size_t n_att, const uint32_t* coff, const uint32_t* clen, const uint32_t* boff, const uint8_t* agg,
                    const uint8_t* cust, size_t n_shuffled, uint32_t* gko, uint8_t* ok, size_t entries_cap,
                    att_desc* desc) {
  uint64_t total = 0;
  gko[0] = 0;
  for (size_t a = 0; a < n_att; ++a) {
    if (clen[a] > ATT_MAX_COMMITTEE || (uint64_t)coff[a] + clen[a] > n_shuffled || boff[a + 1] < boff[a])
      return BLS381_EARG;
    const size_t nbytes = boff[a + 1] - boff[a];
    if (nbytes && (!agg || !cust)) return BLS381_EARG;
    uint32_t n0 = 0, n1 = 0;
    ok[a] = bitfield_ok(agg + boff[a], nbytes, clen[a]) && bitfield_ok(cust + boff[a], nbytes, clen[a]);
    if (ok[a]) attesting_counts(agg + boff[a], cust + boff[a], nbytes, &n0, &n1);
    desc[a] = att_desc{coff[a], clen[a], boff[a], (uint32_t)total, n0, n1};
    total += (uint64_t)n0 + n1;
    if (total > entries_cap || total > 0xFFFFFFFFull) return BLS381_EARG;
    gko[2 * a + 1] = desc[a].out_off + n0;
    gko[2 * a + 2] = (uint32_t)total;
  }
  return 0;
}

int bls381_attesting_entries_device(size_t n_att, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                                    const uint32_t* h_bits_off, const uint8_t* h_aggregation_bits,
                                    const uint8_t* h_custody_bits, const uint32_t* d_shuffled, size_t n_shuffled,
                                    uint32_t* h_group_key_off, uint8_t* h_ok, uint32_t* d_entries, size_t entries_cap,
                                    void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!h_group_key_off) return BLS381_EARG;
    h_group_key_off[0] = 0;
    if (n_att == 0) return 0;
    if (!h_committee_off || !h_committee_len || !h_bits_off || !h_ok || !d_workspace || n_att > (size_t)INT32_MAX / 2 ||
        (n_shuffled && !d_shuffled))
      return BLS381_EARG;
    const size_t bitfield_bytes = h_bits_off[n_att];
    // the descriptors, and below the bitfields, in host blocks of the call's own: async copy sources
    std::vector<att_desc> desc(n_att);
    TRY(att_plan(n_att, h_committee_off, h_committee_len, h_bits_off, h_aggregation_bits, h_custody_bits, n_shuffled,
                 h_group_key_off, h_ok, entries_cap, desc.data()));
    const size_t total = h_group_key_off[2 * n_att];
    if (total == 0) return 0;
    if (!d_entries) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_attesting_entries_workspace_size(n_att, bitfield_bytes));
    const AttWs w = carve_att(b, n_att, bitfield_bytes);
    Held<std::vector<att_desc>> hold(c->keep, s, std::move(desc));
    Held<std::vector<uint8_t>> bits(c->keep, s, std::vector<uint8_t>(2 * bitfield_bytes));
    std::memcpy(bits->data(), h_aggregation_bits, bitfield_bytes);
    std::memcpy(bits->data() + bitfield_bytes, h_custody_bits, bitfield_bytes);
    HIPC(hipMemcpyAsync(w.desc, hold->data(), n_att * sizeof(att_desc), hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(w.agg, bits->data(), bitfield_bytes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(w.cust, bits->data() + bitfield_bytes, bitfield_bytes, hipMemcpyHostToDevice, s));
    LAUNCH("attesting_entries", s, dim3((unsigned)n_att), dim3(ATT_BLOCK), k_attesting_entries, (const att_desc*)w.desc,
           (const uint8_t*)w.agg, (const uint8_t*)w.cust, d_shuffled, d_entries);
    return 0;
  });
}

int bls381_attesting_entries(size_t n_att, const uint32_t* committee_off, const uint32_t* committee_len,
                             const uint32_t* bits_off, const uint8_t* aggregation_bits, const uint8_t* custody_bits,
                             const uint32_t* shuffled, size_t n_shuffled, uint32_t* group_key_off, uint8_t* ok,
                             uint32_t* entries, size_t entries_cap) {
  return guarded([&]() -> int {
    if (!group_key_off) return BLS381_EARG;
    group_key_off[0] = 0;
    if (n_att == 0) return 0;
    if (!bits_off || !committee_len || (n_shuffled && !shuffled)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_attesting_entries_workspace_size(n_att, bits_off[n_att]);
    size_t most = 0;   // the two groups of an attestation are disjoint
    for (size_t a = 0; a < n_att; ++a) most += committee_len[a];
    const size_t ent_words = std::min(entries_cap, most);
    uint32_t *d_sh, *d_ent;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_sh = b.take<uint32_t>(n_shuffled + 1);
      d_ent = b.take<uint32_t>(ent_words + 1);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_sh, shuffled, 4 * n_shuffled));
    TRY(bls381_attesting_entries_device(n_att, committee_off, committee_len, bits_off, aggregation_bits, custody_bits,
                                        d_sh, n_shuffled, group_key_off, ok, entries ? d_ent : nullptr, entries_cap, d_ws,
                                        hc.s));
    TRY(hc.download(entries, d_ent, 4 * (size_t)group_key_off[2 * n_att]));
    return hc.finish();
  });
}

// ---- epoch context: active indices, their root, proposers (bls381_epoch.hpp)
static bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }
// a field of n entries whose span does not overflow
static bool field_ok(size_t n, size_t stride) { return stride >= 8 && (n < 2 || stride <= (SIZE_MAX - 8) / (n - 1)); }
struct ActiveWs {
  uint64_t *ballots, *tile_balance;
  uint32_t *tile_count, *tile_offset;
};
static ActiveWs carve_active(Bump& b, size_t n) {
  const size_t tiles = active_tiles(n);
  ActiveWs w;
  w.ballots = b.take<uint64_t>(tiles * ACTIVE_TILE_BALLOTS);
  w.tile_balance = b.take<uint64_t>(tiles);
  w.tile_count = b.take<uint32_t>(tiles);
  w.tile_offset = b.take<uint32_t>(tiles);
  return w;
}
size_t bls381_active_indices_workspace_size(size_t n) {
  if ((uint64_t)n > 0xFFFFFFFFull) return 0;
  return carved_bytes([&](Bump& b) { carve_active(b, n); });
}

int bls381_active_indices_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch, size_t stride,
                                 uint64_t epoch, const uint8_t* d_effective_balance, size_t balance_stride,
                                 uint32_t* d_indices, uint64_t* d_count_and_total, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || (d_effective_balance && !field_ok(n, balance_stride)) ||
        !d_count_and_total || !aligned8(d_count_and_total) || !aligned4(d_indices))
      return BLS381_EARG;
    if (n && (!d_activation_epoch || !d_exit_epoch || !d_indices || !d_workspace)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
      HIPC(hipMemsetAsync(d_count_and_total, 0, 16, s));
      return 0;
    }
    Bump b(d_workspace, bls381_active_indices_workspace_size(n));
    const ActiveWs w = carve_active(b, n);
    const size_t tiles = active_tiles(n);
    const int has_balance = d_effective_balance ? 1 : 0;
    const u64_field act = make_u64_field(d_activation_epoch, stride), ext = make_u64_field(d_exit_epoch, stride);
    const u64_field bal = has_balance ? make_u64_field(d_effective_balance, balance_stride) : act;
    const dim3 blk(EPOCH_BLOCK);
    LAUNCH("active_count", s, dim3((unsigned)tiles), blk, k_active_count, (uint64_t)n, act, ext, epoch, has_balance, bal,
           w.ballots, w.tile_count, w.tile_balance);
    LAUNCH("active_scan", s, dim3(1), blk, k_active_scan, tiles, (const uint32_t*)w.tile_count,
           (const uint64_t*)w.tile_balance, w.tile_offset, d_count_and_total);
    LAUNCH("active_scatter", s, dim3((unsigned)tiles), blk, k_active_scatter, (const uint64_t*)w.ballots,
           (const uint32_t*)w.tile_offset, d_indices);
    return 0;
  });
}

// Host fields to the device: fields that interleave in one buffer of records (the same stride, bases
// less than a stride apart) travel as one copy of their union, any other field as its own span.
// Each copy keeps its base's offset within 8 bytes, so the device loads are as wide as the
// host's would be.
namespace {
struct HostFields {
  static constexpr int MAXF = 5;
  const uint8_t* h[MAXF];
  size_t stride[MAXF], width[MAXF];  // width: bytes of one entry (8; 1 for the slashed flag)
  int nf = 0, group[MAXF];           // group: the copy a field travels in
  const uint8_t* lo[MAXF];           // per copy: host range
  size_t bytes[MAXF];
  uint8_t* d[MAXF];                  // per copy: device block (bytes + 8)
  int ncopies = 0;
  void add(const uint8_t* p, size_t st, size_t wd = 8) { h[nf] = p; stride[nf] = st; width[nf] = wd; ++nf; }
  void plan(size_t n) {
    for (int f = 0; f < nf; ++f) {
      group[f] = -1;
      for (int g = 0; g < f && group[f] < 0; ++g) {
        const uintptr_t a = (uintptr_t)h[f], o = (uintptr_t)h[g];
        if (stride[f] == stride[g] && stride[f] > 8 && (a > o ? a - o : o - a) < stride[f]) group[f] = group[g];
      }
      if (group[f] < 0) {
        group[f] = ncopies;
        lo[ncopies] = h[f];
        bytes[ncopies] = 0;
        ++ncopies;
      }
    }
    for (int f = 0; f < nf; ++f) {
      const int g = group[f];
      const uint8_t* end = std::max(lo[g] + bytes[g], h[f] + (n ? (n - 1) * stride[f] + width[f] : 0));
      lo[g] = std::min(lo[g], h[f]);
      bytes[g] = (size_t)(end - lo[g]);
    }
  }
  void carve(Bump& b) {
    for (int g = 0; g < ncopies; ++g) d[g] = b.take<uint8_t>(bytes[g] + 8);
  }
  uint8_t* dev_lo(int g) const { return d[g] + ((uintptr_t)lo[g] & 7u); }
  const uint8_t* dev(int f) const { return dev_lo(group[f]) + (h[f] - lo[group[f]]); }
};
}  // namespace

int bls381_active_indices(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch, size_t stride,
                          uint64_t epoch, const uint8_t* effective_balance, size_t balance_stride,
                          uint32_t* indices_out, uint64_t* count_out, uint64_t* total_balance_out) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || (effective_balance && !field_ok(n, balance_stride)) ||
        !count_out)
      return BLS381_EARG;
    if (n && (!activation_epoch || !exit_epoch || !indices_out)) return BLS381_EARG;
    *count_out = 0;
    if (total_balance_out) *total_balance_out = 0;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(activation_epoch, stride);
    hf.add(exit_epoch, stride);
    if (effective_balance) hf.add(effective_balance, balance_stride);
    hf.plan(n);
    const size_t wsb = bls381_active_indices_workspace_size(n);
    uint32_t* d_idx;
    uint64_t* d_out;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_idx = b.take<uint32_t>(n);
      d_out = b.take<uint64_t>(2);
      d_ws = b.take<uint8_t>(wsb);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(bls381_active_indices_device(n, hf.dev(0), hf.dev(1), stride, epoch, effective_balance ? hf.dev(2) : nullptr,
                                     balance_stride, d_idx, d_out, d_ws, hc.s));
    uint64_t out[2];
    TRY(hc.download(out, d_out, 16));
    HIPC(hipStreamSynchronize(hc.s));   // the count decides how much of the list comes back
    TRY(hc.download(indices_out, d_idx, 4 * (size_t)out[0]));
    TRY(hc.finish());
    *count_out = out[0];
    if (total_balance_out) *total_balance_out = out[1];
    return 0;
  });
}

struct IndexRootWs {
  uint64_t* chunks;
  uint8_t* merkle;
};
static IndexRootWs carve_index_root(Bump& b, size_t n) {
  const size_t chunks = index_chunk_count(n);
  IndexRootWs w;
  w.chunks = b.take<uint64_t>(4 * chunks);
  w.merkle = b.take<uint8_t>(bls381_merkle_root_workspace_size(chunks, 0, merkle_chunk_depth(chunks)));
  return w;
}
size_t bls381_active_index_root_workspace_size(size_t n) {
  if ((uint64_t)n > 0xFFFFFFFFull) return 0;
  return carved_bytes([&](Bump& b) { carve_index_root(b, n); });
}

int bls381_active_index_root_device(size_t n, const uint32_t* d_indices, uint8_t* d_root32, void* d_workspace,
                                    void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !d_root32 || !d_workspace || (n && !d_indices) || !aligned4(d_indices))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_active_index_root_workspace_size(n));
    const IndexRootWs w = carve_index_root(b, n);
    const size_t chunks = index_chunk_count(n);
    LAUNCH("index_chunks", s, dim3(grid_for(4 * chunks, EPOCH_BLOCK)), dim3(EPOCH_BLOCK), k_index_chunks, n, d_indices,
           w.chunks);
    // n == 0: no chunk, depth 0, so the root is mix_in_length(zero chunk, 0)
    return bls381_merkle_root_device(chunks, (const uint8_t*)w.chunks, 0, merkle_chunk_depth(chunks), 1, n, d_root32,
                                     w.merkle, stream);
  });
}

int bls381_active_index_root(size_t n, const uint32_t* indices, uint8_t root[32]) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !root || (n && !indices)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_active_index_root_workspace_size(n);
    uint32_t* d_idx;
    uint8_t *d_root, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_idx = b.take<uint32_t>(n);
      d_root = b.take<uint8_t>(32);
      d_ws = b.take<uint8_t>(wsb);
    }));
    TRY(hc.upload(d_idx, indices, 4 * n));
    TRY(bls381_active_index_root_device(n, d_idx, d_root, d_ws, hc.s));
    TRY(hc.download(root, d_root, 32));
    return hc.finish();
  });
}

size_t bls381_proposer_indices_workspace_size(size_t n_slots) {
  if (n_slots > (size_t)INT32_MAX) return 0;
  return carved_bytes([&](Bump& b) { b.take<proposer_slot>(n_slots); });
}
static bool proposer_args_ok(size_t n_slots, const uint32_t* off, const uint32_t* len, const void* shuffled,
                             size_t n_shuffled, const void* balance, size_t balance_stride, size_t n_validators,
                             const uint8_t* seed, uint64_t max_effective_balance, const void* out) {
  if (n_slots > (size_t)INT32_MAX || (uint64_t)n_validators > 0xFFFFFFFFull || !field_ok(n_validators, balance_stride) ||
      max_effective_balance == 0 || max_effective_balance >= PROPOSER_BALANCE_LIMIT)
    return false;
  if (n_slots == 0) return true;
  if (!off || !len || !shuffled || !seed || !out || (n_validators && !balance)) return false;
  for (size_t k = 0; k < n_slots; ++k)
    if (len[k] == 0 || (uint64_t)off[k] + len[k] > n_shuffled) return false;
  return true;
}

int bls381_proposer_indices_device(size_t n_slots, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                                   const uint32_t* d_shuffled, size_t n_shuffled, const uint8_t* d_effective_balance,
                                   size_t balance_stride, size_t n_validators, const uint8_t seed[32], uint64_t epoch,
                                   uint64_t max_effective_balance, uint32_t* d_proposer_out, void* d_workspace,
                                   void* stream) {
  return guarded([&]() -> int {
    if (!proposer_args_ok(n_slots, h_committee_off, h_committee_len, d_shuffled, n_shuffled, d_effective_balance,
                          balance_stride, n_validators, seed, max_effective_balance, d_proposer_out) ||
        !aligned4(d_shuffled) || !aligned4(d_proposer_out) || (n_slots && !d_workspace))
      return BLS381_EARG;
    if (n_slots == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_proposer_indices_workspace_size(n_slots));
    proposer_slot* d_slots = b.take<proposer_slot>(n_slots);
    std::vector<proposer_slot> slots(n_slots);
    for (size_t k = 0; k < n_slots; ++k)
      slots[k] = proposer_slot{h_committee_off[k], h_committee_len[k], (uint32_t)(epoch % h_committee_len[k])};
    Held<std::vector<proposer_slot>> hold(c->keep, s, std::move(slots));
    HIPC(hipMemcpyAsync(d_slots, hold->data(), n_slots * sizeof(proposer_slot), hipMemcpyHostToDevice, s));
    LAUNCH("proposers", s, dim3((unsigned)n_slots), dim3(EPOCH_BLOCK), k_proposers, (const proposer_slot*)d_slots,
           d_shuffled, make_u64_field(d_effective_balance, balance_stride), (uint64_t)n_validators,
           shuffle_seed_from_bytes(seed), max_effective_balance, d_proposer_out);
    return 0;
  });
}

int bls381_proposer_indices(size_t n_slots, const uint32_t* committee_off, const uint32_t* committee_len,
                            const uint32_t* shuffled, size_t n_shuffled, const uint8_t* effective_balance,
                            size_t balance_stride, size_t n_validators, const uint8_t seed[32], uint64_t epoch,
                            uint64_t max_effective_balance, uint32_t* proposer_out) {
  return guarded([&]() -> int {
    if (!proposer_args_ok(n_slots, committee_off, committee_len, shuffled, n_shuffled, effective_balance, balance_stride,
                          n_validators, seed, max_effective_balance, proposer_out))
      return BLS381_EARG;
    if (n_slots == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_proposer_indices_workspace_size(n_slots);
    const size_t span = field_span(n_validators, balance_stride);
    uint32_t *d_sh, *d_out;
    uint8_t *d_bal, *d_ws;
    TRY(hc.carve([&](Bump& b) {
      d_sh = b.take<uint32_t>(n_shuffled);
      d_bal = b.take<uint8_t>(span + 8);
      d_out = b.take<uint32_t>(n_slots);
      d_ws = b.take<uint8_t>(wsb);
    }));
    d_bal += (uintptr_t)effective_balance & 7u;   // the host base's offset within 8 bytes
    TRY(hc.upload(d_sh, shuffled, 4 * n_shuffled));
    TRY(hc.upload(d_bal, effective_balance, span));
    TRY(bls381_proposer_indices_device(n_slots, committee_off, committee_len, d_sh, n_shuffled, d_bal, balance_stride,
                                       n_validators, seed, epoch, max_effective_balance, d_out, d_ws, hc.s));
    TRY(hc.download(proposer_out, d_out, 4 * n_slots));
    return hc.finish();
  });
}

// ---- epoch rewards: votes, deltas, slashings, hysteresis (bls381_rewards.hpp)
static bool flag_ok(size_t n, size_t stride) { return stride >= 1 && (n < 2 || stride <= (SIZE_MAX - 1) / (n - 1)); }
struct VotesWs {
  votes_committee* cm;
  votes_att* att;
  uint8_t* bits;
  uint64_t* partial;
};
static VotesWs carve_votes(Bump& b, size_t n_committees, size_t n_att, size_t bitfield_bytes) {
  VotesWs w;
  w.cm = b.take<votes_committee>(n_committees);
  w.att = b.take<votes_att>(n_att);
  w.bits = b.take<uint8_t>(bitfield_bytes + 1);
  w.partial = b.take<uint64_t>(3 * n_committees);
  return w;
}
size_t bls381_epoch_votes_workspace_size(size_t n_committees, size_t n_att, size_t bitfield_bytes) {
  if (n_committees > (size_t)INT32_MAX || n_att > (size_t)INT32_MAX || bitfield_bytes > 0xFFFFFFFFull) return 0;
  return carved_bytes([&](Bump& b) { carve_votes(b, n_committees, n_att, bitfield_bytes); });
}

// The host half of both forms: the slices (inside the shuffled list, disjoint, at most 4,096
// members), the CSR offsets, verify_bitfield on every bitfield, the flags and the candidate ids.
static int votes_plan(size_t nc, const uint32_t* coff, const uint32_t* clen, size_t n_shuffled, const uint32_t* att_off,
                      const uint32_t* bits_off, const uint8_t* bits, const uint8_t* flags, const uint64_t* delay,
                      const uint32_t* proposer, const uint32_t* cand, const uint32_t* cand_count,
                      std::vector<votes_committee>& cm, std::vector<votes_att>& att) {
  if (nc > (size_t)INT32_MAX || (uint64_t)n_shuffled > 0xFFFFFFFFull) return BLS381_EARG;
  if (nc == 0) return 0;
  if (!coff || !clen || !att_off || !cand_count) return BLS381_EARG;
  const size_t n_att = att_off[nc];
  if (n_att > (size_t)INT32_MAX) return BLS381_EARG;
  if (n_att && (!bits_off || !flags || !delay || !proposer || !cand)) return BLS381_EARG;
  cm.resize(nc);
  att.resize(n_att);
  std::vector<uint32_t> order(nc);
  for (size_t c = 0; c < nc; ++c) {
    if (clen[c] > ATT_MAX_COMMITTEE || (uint64_t)coff[c] + clen[c] > n_shuffled || att_off[c + 1] < att_off[c] ||
        att_off[c + 1] > n_att)
      return BLS381_EARG;
    order[c] = (uint32_t)c;
    cm[c] = votes_committee{coff[c], clen[c], att_off[c], att_off[c + 1] - att_off[c], cand_count[c]};
    for (size_t a = att_off[c]; a < att_off[c + 1]; ++a) {
      if (bits_off[a + 1] < bits_off[a]) return BLS381_EARG;
      const size_t nbytes = bits_off[a + 1] - bits_off[a];
      if (nbytes && !bits) return BLS381_EARG;
      if (nbytes != ((size_t)clen[c] + 7) / 8 || (nbytes && !bitfield_ok(bits + bits_off[a], nbytes, clen[c])))
        return BLS381_EARG;
      if (flags[a] > 3 || (cand[a] != VOTES_NONE && cand[a] >= cand_count[c])) return BLS381_EARG;
      att[a] = votes_att{delay[a], bits_off[a], flags[a], proposer[a], cand[a]};
    }
  }
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return coff[x] < coff[y]; });
  uint64_t end = 0;
  for (size_t k = 0; k < nc; ++k) {
    const uint32_t c = order[k];
    if (clen[c] == 0) continue;
    if (coff[c] < end) return BLS381_EARG;
    end = (uint64_t)coff[c] + clen[c];
  }
  return 0;
}

int bls381_epoch_votes_device(size_t n_committees, const uint32_t* h_committee_off, const uint32_t* h_committee_len,
                              const uint32_t* d_shuffled, size_t n_shuffled, size_t n_validators,
                              const uint8_t* d_slashed, size_t slashed_stride, const uint8_t* d_effective_balance,
                              size_t stride, const uint32_t* h_att_off, const uint32_t* h_bits_off,
                              const uint8_t* h_aggregation_bits, const uint8_t* h_att_flags,
                              const uint64_t* h_att_inclusion_delay, const uint32_t* h_att_proposer,
                              const uint32_t* h_att_candidate, const uint32_t* h_cand_count, uint32_t* d_votes,
                              uint64_t* d_incl_delay, uint32_t* d_incl_proposer, uint32_t* d_committee_of,
                              uint32_t* d_winner, uint64_t* d_winner_balance, uint64_t* d_committee_balance,
                              uint64_t* d_totals, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n_validators > 0xFFFFFFFFull || !field_ok(n_validators, stride) ||
        !flag_ok(n_validators, slashed_stride) || !d_totals || !aligned8(d_totals) || !aligned4(d_shuffled) ||
        !aligned4(d_votes) || !aligned8(d_incl_delay) || !aligned4(d_incl_proposer) || !aligned4(d_committee_of) ||
        !aligned4(d_winner) || !aligned8(d_winner_balance) || !aligned8(d_committee_balance))
      return BLS381_EARG;
    if (n_validators && (!d_slashed || !d_effective_balance || !d_votes || !d_incl_delay || !d_incl_proposer ||
                         !d_committee_of))
      return BLS381_EARG;
    if (n_committees && (!d_winner || !d_winner_balance || !d_committee_balance || !d_workspace ||
                         (n_shuffled && !d_shuffled)))
      return BLS381_EARG;
    std::vector<votes_committee> cm;
    std::vector<votes_att> att;
    TRY(votes_plan(n_committees, h_committee_off, h_committee_len, n_shuffled, h_att_off, h_bits_off, h_aggregation_bits,
                   h_att_flags, h_att_inclusion_delay, h_att_proposer, h_att_candidate, h_cand_count, cm, att));
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blk(EPOCH_BLOCK);
    LAUNCH("votes_clear", s, dim3(grid_for(n_validators, EPOCH_BLOCK)), blk, k_votes_clear, (uint64_t)n_validators, d_votes,
           d_committee_of);
    if (n_committees == 0) {
      HIPC(hipMemsetAsync(d_totals, 0, 24, s));
      return 0;
    }
    const size_t n_att = att.size(), bitfield_bytes = n_att ? h_bits_off[n_att] : 0;
    Bump b(d_workspace, bls381_epoch_votes_workspace_size(n_committees, n_att, bitfield_bytes));
    const VotesWs w = carve_votes(b, n_committees, n_att, bitfield_bytes);
    Held<std::vector<votes_committee>> hold_cm(c->keep, s, std::move(cm));
    Held<std::vector<votes_att>> hold_att(c->keep, s, std::move(att));
    Held<std::vector<uint8_t>> hold_bits(c->keep, s, std::vector<uint8_t>(bitfield_bytes));
    if (bitfield_bytes) std::memcpy(hold_bits->data(), h_aggregation_bits, bitfield_bytes);
    HIPC(hipMemcpyAsync(w.cm, hold_cm->data(), n_committees * sizeof(votes_committee), hipMemcpyHostToDevice, s));
    if (n_att) HIPC(hipMemcpyAsync(w.att, hold_att->data(), n_att * sizeof(votes_att), hipMemcpyHostToDevice, s));
    if (bitfield_bytes) HIPC(hipMemcpyAsync(w.bits, hold_bits->data(), bitfield_bytes, hipMemcpyHostToDevice, s));
    LAUNCH("votes_committees", s, dim3((unsigned)n_committees), blk, k_votes_committees, (const votes_committee*)w.cm,
           (const votes_att*)w.att, (const uint8_t*)w.bits, d_shuffled, make_u8_field(d_slashed, slashed_stride),
           make_u64_field(d_effective_balance, stride), (uint64_t)n_validators, d_votes, d_incl_delay, d_incl_proposer,
           d_committee_of, d_winner, d_winner_balance, d_committee_balance, w.partial);
    LAUNCH("votes_totals", s, dim3(1), blk, k_votes_totals, n_committees, (const uint64_t*)w.partial, d_totals);
    return 0;
  });
}

int bls381_epoch_votes(size_t n_committees, const uint32_t* committee_off, const uint32_t* committee_len,
                       const uint32_t* shuffled, size_t n_shuffled, size_t n_validators, const uint8_t* slashed,
                       size_t slashed_stride, const uint8_t* effective_balance, size_t stride, const uint32_t* att_off,
                       const uint32_t* bits_off, const uint8_t* aggregation_bits, const uint8_t* att_flags,
                       const uint64_t* att_inclusion_delay, const uint32_t* att_proposer, const uint32_t* att_candidate,
                       const uint32_t* cand_count, uint32_t* votes, uint64_t* incl_delay, uint32_t* incl_proposer,
                       uint32_t* committee_of, uint32_t* winner, uint64_t* winner_balance, uint64_t* committee_balance,
                       uint64_t totals[3]) {
  return guarded([&]() -> int {
    if ((uint64_t)n_validators > 0xFFFFFFFFull || (uint64_t)n_shuffled > 0xFFFFFFFFull ||
        n_committees > (size_t)INT32_MAX || !field_ok(n_validators, stride) || !flag_ok(n_validators, slashed_stride) ||
        !totals)
      return BLS381_EARG;
    if (n_validators && (!slashed || !effective_balance || !votes || !incl_delay || !incl_proposer || !committee_of))
      return BLS381_EARG;
    if (n_committees && (!att_off || !winner || !winner_balance || !committee_balance || (n_shuffled && !shuffled)))
      return BLS381_EARG;
    totals[0] = totals[1] = totals[2] = 0;
    if (n_validators == 0 && n_committees == 0) return 0;
    const size_t n_att = n_committees ? att_off[n_committees] : 0;
    if (n_att > (size_t)INT32_MAX || (n_att && !bits_off)) return BLS381_EARG;
    const size_t bitfield_bytes = n_att ? bits_off[n_att] : 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(slashed, slashed_stride, 1);
    hf.add(effective_balance, stride);
    hf.plan(n_validators);
    const size_t wsb = bls381_epoch_votes_workspace_size(n_committees, n_att, bitfield_bytes);
    uint32_t *d_sh, *d_votes, *d_prop, *d_cof, *d_win;
    uint64_t *d_delay, *d_wbal, *d_cbal, *d_tot;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_sh = b.take<uint32_t>(n_shuffled + 1);
      d_votes = b.take<uint32_t>(n_validators + 1);
      d_prop = b.take<uint32_t>(n_validators + 1);
      d_cof = b.take<uint32_t>(n_validators + 1);
      d_delay = b.take<uint64_t>(n_validators + 1);
      d_win = b.take<uint32_t>(n_committees + 1);
      d_wbal = b.take<uint64_t>(n_committees + 1);
      d_cbal = b.take<uint64_t>(n_committees + 1);
      d_tot = b.take<uint64_t>(3);
      d_ws = b.take<uint8_t>(wsb + 1);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(hc.upload(d_sh, shuffled, 4 * n_shuffled));
    // entries the call does not write come back as zero
    if (n_validators) {
      HIPC(hipMemsetAsync(d_delay, 0, 8 * n_validators, hc.s));
      HIPC(hipMemsetAsync(d_prop, 0, 4 * n_validators, hc.s));
    }
    TRY(bls381_epoch_votes_device(n_committees, committee_off, committee_len, d_sh, n_shuffled, n_validators, hf.dev(0),
                                  slashed_stride, hf.dev(1), stride, att_off, bits_off, aggregation_bits, att_flags,
                                  att_inclusion_delay, att_proposer, att_candidate, cand_count, d_votes, d_delay, d_prop,
                                  d_cof, d_win, d_wbal, d_cbal, d_tot, d_ws, hc.s));
    TRY(hc.download(votes, d_votes, 4 * n_validators));
    TRY(hc.download(incl_delay, d_delay, 8 * n_validators));
    TRY(hc.download(incl_proposer, d_prop, 4 * n_validators));
    TRY(hc.download(committee_of, d_cof, 4 * n_validators));
    TRY(hc.download(winner, d_win, 4 * n_committees));
    TRY(hc.download(winner_balance, d_wbal, 8 * n_committees));
    TRY(hc.download(committee_balance, d_cbal, 8 * n_committees));
    TRY(hc.download(totals, d_tot, 24));
    return hc.finish();
  });
}

size_t bls381_epoch_deltas_workspace_size(size_t n) {
  if ((uint64_t)n > 0xFFFFFFFFull) return 0;
  return carved_bytes([&](Bump& b) { b.take<uint64_t>(n); });
}
static bool deltas_scalars_ok(const bls381_reward_constants* k, uint32_t which, uint64_t previous_epoch,
                              uint64_t finalized_epoch) {
  return k && which >= 1 && which <= 3 && previous_epoch != ~(uint64_t)0 && finalized_epoch <= previous_epoch &&
         k->base_rewards_per_epoch && k->proposer_reward_quotient && k->inactivity_penalty_quotient;
}

int bls381_epoch_deltas_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch,
                               const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                               const uint8_t* d_slashed, size_t slashed_stride, const uint32_t* d_votes,
                               const uint64_t* d_incl_delay, const uint32_t* d_incl_proposer,
                               const uint32_t* d_committee_of, size_t n_committees, const uint64_t* d_winner_balance,
                               const uint64_t* d_committee_balance, const uint64_t* d_totals, const uint64_t* d_balances,
                               uint64_t previous_epoch, uint64_t finalized_epoch, const uint64_t* d_total_balance,
                               const bls381_reward_constants* constants, uint32_t which, uint64_t* d_rewards,
                               uint64_t* d_penalties, uint64_t* d_new_balances, uint64_t* d_status, void* d_workspace,
                               void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || n_committees > (size_t)INT32_MAX || !field_ok(n, stride) ||
        !flag_ok(n, slashed_stride) || !deltas_scalars_ok(constants, which, previous_epoch, finalized_epoch) ||
        !d_total_balance || !d_status || !d_totals || !aligned8(d_total_balance) || !aligned8(d_status) ||
        !aligned8(d_totals) || !aligned4(d_votes) || !aligned8(d_incl_delay) || !aligned4(d_incl_proposer) ||
        !aligned4(d_committee_of) || !aligned8(d_winner_balance) || !aligned8(d_committee_balance) ||
        !aligned8(d_balances) || !aligned8(d_rewards) || !aligned8(d_penalties) || !aligned8(d_new_balances))
      return BLS381_EARG;
    if (n && (!d_activation_epoch || !d_exit_epoch || !d_withdrawable_epoch || !d_effective_balance || !d_slashed ||
              !d_votes || !d_incl_delay || !d_incl_proposer || !d_committee_of || !d_balances || !d_rewards ||
              !d_penalties || !d_new_balances || !d_workspace))
      return BLS381_EARG;
    if (n_committees && (!d_winner_balance || !d_committee_balance)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemsetAsync(d_status, 0, 8, s));
    if (n == 0) return 0;
    Bump b(d_workspace, bls381_epoch_deltas_workspace_size(n));
    uint64_t* proposer_reward = b.take<uint64_t>(n);
    HIPC(hipMemsetAsync(proposer_reward, 0, 8 * n, s));
    deltas_in in;
    in.activation = make_u64_field(d_activation_epoch, stride);
    in.exit_ = make_u64_field(d_exit_epoch, stride);
    in.withdrawable = make_u64_field(d_withdrawable_epoch, stride);
    in.effective = make_u64_field(d_effective_balance, stride);
    in.slashed = make_u8_field(d_slashed, slashed_stride);
    in.votes = d_votes;
    in.incl_delay = d_incl_delay;
    in.incl_proposer = d_incl_proposer;
    in.committee_of = d_committee_of;
    in.winner_balance = d_winner_balance;
    in.committee_balance = d_committee_balance;
    in.totals = d_totals;
    in.n = n;
    in.n_committees = n_committees;
    in.previous_epoch = previous_epoch;
    in.finalized_epoch = finalized_epoch;
    in.k = reward_constants{constants->base_reward_factor,
                            constants->base_rewards_per_epoch,
                            constants->proposer_reward_quotient,
                            constants->min_attestation_inclusion_delay,
                            constants->min_epochs_to_inactivity_penalty,
                            constants->inactivity_penalty_quotient};
    in.which = which;
    const dim3 grid(grid_for(n, EPOCH_BLOCK)), blk(EPOCH_BLOCK);
    LAUNCH("epoch_deltas", s, grid, blk, k_epoch_deltas, in, d_total_balance, d_rewards, d_penalties,
           (unsigned long long*)proposer_reward, (unsigned long long*)d_status);
    LAUNCH("epoch_deltas_apply", s, grid, blk, k_epoch_deltas_apply, (uint64_t)n, d_balances, d_rewards,
           (const uint64_t*)d_penalties, (const uint64_t*)proposer_reward, d_new_balances, (unsigned long long*)d_status);
    return 0;
  });
}

int bls381_epoch_deltas(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch,
                        const uint8_t* withdrawable_epoch, const uint8_t* effective_balance, size_t stride,
                        const uint8_t* slashed, size_t slashed_stride, const uint32_t* votes, const uint64_t* incl_delay,
                        const uint32_t* incl_proposer, const uint32_t* committee_of, size_t n_committees,
                        const uint64_t* winner_balance, const uint64_t* committee_balance, const uint64_t totals[3],
                        const uint64_t* balances, uint64_t previous_epoch, uint64_t finalized_epoch,
                        uint64_t total_balance, const bls381_reward_constants* constants, uint32_t which,
                        uint64_t* rewards, uint64_t* penalties, uint64_t* new_balances, uint64_t* overflows_out) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || n_committees > (size_t)INT32_MAX || !field_ok(n, stride) ||
        !flag_ok(n, slashed_stride) || !deltas_scalars_ok(constants, which, previous_epoch, finalized_epoch) ||
        !overflows_out || !totals)
      return BLS381_EARG;
    if (n && (!activation_epoch || !exit_epoch || !withdrawable_epoch || !effective_balance || !slashed || !votes ||
              !incl_delay || !incl_proposer || !committee_of || !balances || !rewards || !penalties || !new_balances))
      return BLS381_EARG;
    if (n_committees && (!winner_balance || !committee_balance)) return BLS381_EARG;
    *overflows_out = 0;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(activation_epoch, stride);
    hf.add(exit_epoch, stride);
    hf.add(withdrawable_epoch, stride);
    hf.add(effective_balance, stride);
    hf.add(slashed, slashed_stride, 1);
    hf.plan(n);
    const size_t wsb = bls381_epoch_deltas_workspace_size(n);
    uint32_t *d_votes, *d_prop, *d_cof;
    uint64_t *d_delay, *d_wbal, *d_cbal, *d_scal, *d_bal, *d_rew, *d_pen;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_votes = b.take<uint32_t>(n);
      d_prop = b.take<uint32_t>(n);
      d_cof = b.take<uint32_t>(n);
      d_delay = b.take<uint64_t>(n);
      d_wbal = b.take<uint64_t>(n_committees + 1);
      d_cbal = b.take<uint64_t>(n_committees + 1);
      d_scal = b.take<uint64_t>(5);   // totals[3], the total balance, the status word
      d_bal = b.take<uint64_t>(n);
      d_rew = b.take<uint64_t>(n);
      d_pen = b.take<uint64_t>(n);
      d_ws = b.take<uint8_t>(wsb);
    }));
    const uint64_t scal[4] = {totals[0], totals[1], totals[2], total_balance};
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(hc.upload(d_votes, votes, 4 * n));
    TRY(hc.upload(d_prop, incl_proposer, 4 * n));
    TRY(hc.upload(d_cof, committee_of, 4 * n));
    TRY(hc.upload(d_delay, incl_delay, 8 * n));
    TRY(hc.upload(d_wbal, winner_balance, 8 * n_committees));
    TRY(hc.upload(d_cbal, committee_balance, 8 * n_committees));
    TRY(hc.upload(d_scal, scal, 32));
    TRY(hc.upload(d_bal, balances, 8 * n));
    TRY(bls381_epoch_deltas_device(n, hf.dev(0), hf.dev(1), hf.dev(2), hf.dev(3), stride, hf.dev(4), slashed_stride,
                                   d_votes, d_delay, d_prop, d_cof, n_committees, d_wbal, d_cbal, d_scal, d_bal,
                                   previous_epoch, finalized_epoch, d_scal + 3, constants, which, d_rew, d_pen, d_bal,
                                   d_scal + 4, d_ws, hc.s));
    TRY(hc.download(rewards, d_rew, 8 * n));
    TRY(hc.download(penalties, d_pen, 8 * n));
    TRY(hc.download(new_balances, d_bal, 8 * n));
    TRY(hc.download(overflows_out, d_scal + 4, 8));
    return hc.finish();
  });
}

int bls381_epoch_slashings_device(size_t n, const uint8_t* d_slashed, size_t slashed_stride,
                                  const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                                  uint64_t current_epoch, uint64_t total_penalties, const uint64_t* d_total_balance,
                                  uint64_t latest_slashed_exit_length, uint64_t min_slashing_penalty_quotient,
                                  uint64_t* d_balances, void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !flag_ok(n, slashed_stride) || !d_total_balance ||
        !aligned8(d_total_balance) || !aligned8(d_balances) || min_slashing_penalty_quotient == 0)
      return BLS381_EARG;
    if (n && (!d_slashed || !d_withdrawable_epoch || !d_effective_balance || !d_balances)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH("epoch_slashings", s, dim3(grid_for(n, EPOCH_BLOCK)), dim3(EPOCH_BLOCK), k_epoch_slashings, (uint64_t)n,
           make_u8_field(d_slashed, slashed_stride), make_u64_field(d_withdrawable_epoch, stride),
           make_u64_field(d_effective_balance, stride), current_epoch, total_penalties, d_total_balance,
           latest_slashed_exit_length, min_slashing_penalty_quotient, d_balances);
    return 0;
  });
}

int bls381_epoch_slashings(size_t n, const uint8_t* slashed, size_t slashed_stride, const uint8_t* withdrawable_epoch,
                           const uint8_t* effective_balance, size_t stride, uint64_t current_epoch,
                           uint64_t total_penalties, uint64_t total_balance, uint64_t latest_slashed_exit_length,
                           uint64_t min_slashing_penalty_quotient, uint64_t* balances) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !flag_ok(n, slashed_stride) ||
        min_slashing_penalty_quotient == 0)
      return BLS381_EARG;
    if (n && (!slashed || !withdrawable_epoch || !effective_balance || !balances)) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(slashed, slashed_stride, 1);
    hf.add(withdrawable_epoch, stride);
    hf.add(effective_balance, stride);
    hf.plan(n);
    uint64_t *d_total, *d_bal;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_total = b.take<uint64_t>(1);
      d_bal = b.take<uint64_t>(n);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(hc.upload(d_total, &total_balance, 8));
    TRY(hc.upload(d_bal, balances, 8 * n));
    TRY(bls381_epoch_slashings_device(n, hf.dev(0), slashed_stride, hf.dev(1), hf.dev(2), stride, current_epoch,
                                      total_penalties, d_total, latest_slashed_exit_length, min_slashing_penalty_quotient,
                                      d_bal, hc.s));
    TRY(hc.download(balances, d_bal, 8 * n));
    return hc.finish();
  });
}

int bls381_effective_balances_device(size_t n, const uint64_t* d_balances, const uint8_t* d_effective_balance,
                                     size_t stride, uint64_t increment, uint64_t max_effective_balance,
                                     uint32_t* d_indices, uint64_t* d_values, uint64_t* d_changed, void* stream) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || increment == 0 || !d_changed || !aligned8(d_changed) ||
        !aligned8(d_balances) || !aligned4(d_indices) || !aligned8(d_values))
      return BLS381_EARG;
    if (n && (!d_balances || !d_effective_balance || !d_indices || !d_values)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemsetAsync(d_changed, 0, 8, s));
    LAUNCH("effective_balances", s, dim3(grid_for(n, EPOCH_BLOCK)), dim3(EPOCH_BLOCK), k_effective_balances, (uint64_t)n,
           d_balances, make_u64_field(d_effective_balance, stride), increment, max_effective_balance, d_indices, d_values,
           (unsigned long long*)d_changed);
    return 0;
  });
}

int bls381_effective_balances(size_t n, const uint64_t* balances, const uint8_t* effective_balance, size_t stride,
                              uint64_t increment, uint64_t max_effective_balance, uint32_t* indices, uint64_t* values,
                              uint64_t* changed_out) {
  return guarded([&]() -> int {
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || increment == 0 || !changed_out) return BLS381_EARG;
    if (n && (!balances || !effective_balance || !indices || !values)) return BLS381_EARG;
    *changed_out = 0;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(effective_balance, stride);
    hf.plan(n);
    uint64_t *d_bal, *d_val, *d_changed;
    uint32_t* d_idx;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_bal = b.take<uint64_t>(n);
      d_val = b.take<uint64_t>(n);
      d_idx = b.take<uint32_t>(n);
      d_changed = b.take<uint64_t>(1);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(hc.upload(d_bal, balances, 8 * n));
    TRY(bls381_effective_balances_device(n, d_bal, hf.dev(0), stride, increment, max_effective_balance, d_idx, d_val,
                                         d_changed, hc.s));
    TRY(hc.download(indices, d_idx, 4 * n));
    TRY(hc.download(values, d_val, 8 * n));
    TRY(hc.download(changed_out, d_changed, 8));
    return hc.finish();
  });
}

// ---- registry updates: ejections, exit queue, activations (bls381_regupd.hpp)
struct RegupdWs {
  uint64_t *ballots_ejected, *ballots_candidate, *tile_peak_epoch, *sc, *keys;
  uint32_t *tile_count, *tile_peak_count, *offset_ejected, *offset_candidate, *cand_index, *hist;
};
static RegupdWs carve_regupd(Bump& b, size_t n) {
  const size_t tiles = active_tiles(n);
  RegupdWs w;
  w.ballots_ejected = b.take<uint64_t>(tiles * ACTIVE_TILE_BALLOTS);
  w.ballots_candidate = b.take<uint64_t>(tiles * ACTIVE_TILE_BALLOTS);
  w.tile_peak_epoch = b.take<uint64_t>(tiles);
  w.sc = b.take<uint64_t>(RU_SCALARS);
  w.keys = b.take<uint64_t>(n);
  w.tile_count = b.take<uint32_t>(3 * tiles);
  w.tile_peak_count = b.take<uint32_t>(tiles);
  w.offset_ejected = b.take<uint32_t>(tiles);
  w.offset_candidate = b.take<uint32_t>(tiles);
  w.cand_index = b.take<uint32_t>(n);
  w.hist = b.take<uint32_t>((size_t)REGUPD_DIGITS * REGUPD_BINS);
  return w;
}
size_t bls381_registry_updates_workspace_size(size_t n) {
  if ((uint64_t)n > 0xFFFFFFFFull) return 0;
  return carved_bytes([&](Bump& b) { carve_regupd(b, n); });
}

// the constants and the two delayed epochs of a call, or false for arguments it rejects
static bool regupd_scalars_ok(size_t n, const bls381_registry_constants* constants, uint64_t current_epoch,
                              const uint64_t* finalized_epoch, registry_constants* kc, regupd_epochs* e) {
  if (!constants || constants->churn_limit_quotient == 0) return false;
  *kc = registry_constants{constants->max_effective_balance,      constants->ejection_balance,
                           constants->activation_exit_delay,      constants->min_validator_withdrawability_delay,
                           constants->min_per_epoch_churn_limit,  constants->churn_limit_quotient};
  // at most n validators are active: a limit of 0 that the arguments alone show
  if (kc->min_per_epoch_churn_limit == 0 && (uint64_t)n / kc->churn_limit_quotient == 0) return false;
  e->cur = current_epoch;
  e->delayed_fin = 0;
  if (!delayed_epoch(current_epoch, kc->activation_exit_delay, &e->delayed_cur)) return false;
  if (finalized_epoch && !delayed_epoch(*finalized_epoch, kc->activation_exit_delay, &e->delayed_fin)) return false;
  return true;
}

int bls381_exit_queue_device(size_t n, const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch, size_t stride,
                             uint64_t current_epoch, const bls381_registry_constants* constants, uint64_t* d_queue,
                             void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    registry_constants kc;
    regupd_epochs e;
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !d_queue || !aligned8(d_queue) || !d_workspace ||
        !regupd_scalars_ok(n, constants, current_epoch, nullptr, &kc, &e))
      return BLS381_EARG;
    if (n && (!d_activation_epoch || !d_exit_epoch)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_registry_updates_workspace_size(n));
    const RegupdWs w = carve_regupd(b, n);
    const size_t tiles = active_tiles(n);
    const dim3 blk(EPOCH_BLOCK);
    const u64_field act = make_u64_field(d_activation_epoch, stride), ext = make_u64_field(d_exit_epoch, stride);
    const regupd_fields f{act, act, ext, ext, act};   // queue_only reads activation and exit alone
    if (tiles)
      LAUNCH("regupd_count", s, dim3((unsigned)tiles), blk, k_regupd_count, (uint64_t)n, f, e, kc, 1, w.ballots_ejected,
             w.ballots_candidate, w.tile_count, w.tile_peak_epoch, w.tile_peak_count);
    LAUNCH("regupd_scan", s, dim3(1), blk, k_regupd_scan, tiles, (const uint32_t*)w.tile_count,
           (const uint64_t*)w.tile_peak_epoch, (const uint32_t*)w.tile_peak_count, w.offset_ejected, w.offset_candidate, kc,
           e.delayed_cur, w.sc, (uint64_t*)nullptr, d_queue);
    return 0;
  });
}

int bls381_exit_queue(size_t n, const uint8_t* activation_epoch, const uint8_t* exit_epoch, size_t stride,
                      uint64_t current_epoch, const bls381_registry_constants* constants, uint64_t queue_out[4]) {
  return guarded([&]() -> int {
    registry_constants kc;
    regupd_epochs e;
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !queue_out ||
        !regupd_scalars_ok(n, constants, current_epoch, nullptr, &kc, &e))
      return BLS381_EARG;
    if (n && (!activation_epoch || !exit_epoch)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(activation_epoch, stride);
    hf.add(exit_epoch, stride);
    hf.plan(n);
    const size_t wsb = bls381_registry_updates_workspace_size(n);
    uint64_t* d_queue;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_queue = b.take<uint64_t>(4);
      d_ws = b.take<uint8_t>(wsb);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(bls381_exit_queue_device(n, hf.dev(0), hf.dev(1), stride, current_epoch, constants, d_queue, d_ws, hc.s));
    uint64_t q[4];
    TRY(hc.download(q, d_queue, 32));
    TRY(hc.finish());
    if (q[2] == 0) return BLS381_EARG;   // no minimum and too few active validators: no churn limit
    for (int x = 0; x < 4; ++x) queue_out[x] = q[x];
    return 0;
  });
}

int bls381_registry_updates_device(size_t n, const uint8_t* d_activation_eligibility_epoch,
                                   const uint8_t* d_activation_epoch, const uint8_t* d_exit_epoch,
                                   const uint8_t* d_withdrawable_epoch, const uint8_t* d_effective_balance, size_t stride,
                                   uint64_t current_epoch, uint64_t finalized_epoch,
                                   const bls381_registry_constants* constants, uint32_t* d_indices, uint8_t* d_values,
                                   uint64_t* d_summary, void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    registry_constants kc;
    regupd_epochs e;
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !d_summary || !aligned8(d_summary) || !d_workspace ||
        !aligned4(d_indices) || !aligned8(d_values) ||
        !regupd_scalars_ok(n, constants, current_epoch, &finalized_epoch, &kc, &e))
      return BLS381_EARG;
    if (n && (!d_activation_eligibility_epoch || !d_activation_epoch || !d_exit_epoch || !d_withdrawable_epoch ||
              !d_effective_balance || !d_indices || !d_values))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    Bump b(d_workspace, bls381_registry_updates_workspace_size(n));
    const RegupdWs w = carve_regupd(b, n);
    const size_t tiles = active_tiles(n);
    const dim3 blk(EPOCH_BLOCK), grid((unsigned)tiles);
    const regupd_fields f{make_u64_field(d_activation_eligibility_epoch, stride), make_u64_field(d_activation_epoch, stride),
                          make_u64_field(d_exit_epoch, stride), make_u64_field(d_withdrawable_epoch, stride),
                          make_u64_field(d_effective_balance, stride)};
    HIPC(hipMemsetAsync(d_summary, 0, 8 * RS_WORDS, s));
    if (tiles)
      LAUNCH("regupd_count", s, grid, blk, k_regupd_count, (uint64_t)n, f, e, kc, 0, w.ballots_ejected,
             w.ballots_candidate, w.tile_count, w.tile_peak_epoch, w.tile_peak_count);
    LAUNCH("regupd_scan", s, dim3(1), blk, k_regupd_scan, tiles, (const uint32_t*)w.tile_count,
           (const uint64_t*)w.tile_peak_epoch, (const uint32_t*)w.tile_peak_count, w.offset_ejected, w.offset_candidate, kc,
           e.delayed_cur, w.sc, d_summary, (uint64_t*)nullptr);
    if (n == 0) return 0;
    HIPC(hipMemsetAsync(w.hist, 0, 4 * (size_t)REGUPD_DIGITS * REGUPD_BINS, s));
    LAUNCH("regupd_compact", s, grid, blk, k_regupd_compact, (const uint64_t*)w.ballots_candidate,
           (const uint32_t*)w.offset_candidate, f.eligibility, f.effective, e.cur, kc.max_effective_balance, w.keys,
           w.cand_index);
    // the grid covers n entries; the workgroups past the K candidates leave at once
    for (uint32_t pass = 0; pass <= REGUPD_DIGITS; ++pass)
      LAUNCH("regupd_select", s, pass < REGUPD_DIGITS ? grid : dim3(1), blk, k_regupd_select, pass,
             (const uint64_t*)w.keys, (const uint32_t*)w.cand_index, w.sc, w.hist);
    LAUNCH("regupd_apply", s, grid, blk, k_regupd_apply, (uint64_t)n, f, e, kc, (const uint64_t*)w.ballots_ejected,
           (const uint32_t*)w.offset_ejected, (const uint64_t*)w.sc, d_indices, (uint64_t*)d_values,
           (unsigned long long*)d_summary);
    return 0;
  });
}

int bls381_registry_updates(size_t n, const uint8_t* activation_eligibility_epoch, const uint8_t* activation_epoch,
                            const uint8_t* exit_epoch, const uint8_t* withdrawable_epoch, const uint8_t* effective_balance,
                            size_t stride, uint64_t current_epoch, uint64_t finalized_epoch,
                            const bls381_registry_constants* constants, uint32_t* indices, uint8_t* values,
                            uint64_t summary[8]) {
  return guarded([&]() -> int {
    registry_constants kc;
    regupd_epochs e;
    if ((uint64_t)n > 0xFFFFFFFFull || !field_ok(n, stride) || !summary ||
        !regupd_scalars_ok(n, constants, current_epoch, &finalized_epoch, &kc, &e))
      return BLS381_EARG;
    if (n && (!activation_eligibility_epoch || !activation_epoch || !exit_epoch || !withdrawable_epoch ||
              !effective_balance || !indices || !values))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(activation_eligibility_epoch, stride);
    hf.add(activation_epoch, stride);
    hf.add(exit_epoch, stride);
    hf.add(withdrawable_epoch, stride);
    hf.add(effective_balance, stride);
    hf.plan(n);
    const size_t wsb = bls381_registry_updates_workspace_size(n);
    uint64_t *d_val, *d_sum;
    uint32_t* d_idx;
    uint8_t* d_ws;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_val = b.take<uint64_t>(4 * n);
      d_sum = b.take<uint64_t>(RS_WORDS);
      d_idx = b.take<uint32_t>(n);
      d_ws = b.take<uint8_t>(wsb);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(bls381_registry_updates_device(n, hf.dev(0), hf.dev(1), hf.dev(2), hf.dev(3), hf.dev(4), stride, current_epoch,
                                       finalized_epoch, constants, d_idx, (uint8_t*)d_val, d_sum, d_ws, hc.s));
    uint64_t sum[RS_WORDS];
    TRY(hc.download(sum, d_sum, 8 * RS_WORDS));
    HIPC(hipStreamSynchronize(hc.s));   // the status decides whether anything comes back
    if (sum[RS_STATUS] & REGUPD_STATUS_NO_CHURN) return BLS381_EARG;   // nothing was written
    TRY(hc.download(indices, d_idx, 4 * n));
    TRY(hc.download(values, d_val, 32 * n));
    TRY(hc.finish());
    for (uint32_t x = 0; x < RS_WORDS; ++x) summary[x] = sum[x];
    return 0;
  });
}

// ---- fork choice: latest messages and the LMD-GHOST head (bls381_forkchoice.hpp)
// The tree, `seq` and `dirty` are the host's; the messages, the tree's numbering and the head's
// scratch live in one device block carved at creation.
struct FcDev {
  unsigned long long *key, *sums;   // sums: direct weights (2 B words), then best_count (B), B = the blocks now
  uint64_t *prefix, *count;
  uint32_t *target, *numbering, *best_rank, *jump_a, *jump_b;   // numbering: parent, pre, sub, rank, node_at (B each)
};
static FcDev carve_fc(Bump& b, size_t vcap, size_t bcap) {
  FcDev d;
  d.key = b.take<unsigned long long>(vcap);
  d.sums = b.take<unsigned long long>(3 * bcap);
  d.prefix = b.take<uint64_t>(2 * (bcap + 1));
  d.count = b.take<uint64_t>(bcap);
  d.target = b.take<uint32_t>(vcap);
  d.numbering = b.take<uint32_t>(5 * bcap);
  d.best_rank = b.take<uint32_t>(bcap);
  d.jump_a = b.take<uint32_t>(bcap);
  d.jump_b = b.take<uint32_t>(bcap);
  return d;
}
struct bls381_fork_choice {
  int device = -1;
  size_t vcap = 0, bcap = 0;
  uint64_t seq = 0;
  fc_tree tree;
  bool dirty = true;   // the tree has changed since its numbering went to the device
  void* block = nullptr;
  FcDev d{};
};

int bls381_fork_choice_create(size_t validator_capacity, size_t block_capacity, bls381_fork_choice** out) {
  if (!out) return BLS381_EARG;
  *out = nullptr;
  if (validator_capacity == 0 || (uint64_t)validator_capacity > 0xFFFFFFFFull || block_capacity == 0 ||
      block_capacity > FC_BLOCK_LIMIT)
    return BLS381_EARG;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  std::unique_ptr<bls381_fork_choice> fc(new bls381_fork_choice());
  fc->device = c->device;
  fc->vcap = validator_capacity;
  fc->bcap = block_capacity;
  const size_t bytes = carved_bytes([&](Bump& b) { carve_fc(b, validator_capacity, block_capacity); });
  bool ok = hipMalloc(&fc->block, bytes) == hipSuccess;
  if (ok) {
    Bump b(fc->block, bytes);
    fc->d = carve_fc(b, validator_capacity, block_capacity);
    ok = hipMemset(fc->d.key, 0, 8 * validator_capacity) == hipSuccess &&
         hipMemset(fc->d.target, 0xFF, 4 * validator_capacity) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
  }
  if (!ok) {
    (void)hipGetLastError();
    (void)hipFree(fc->block);
    t_err = "fork choice allocation failed";
    return BLS381_EHIP;
  }
  *out = fc.release();
  return 0;
}

void bls381_fork_choice_destroy(bls381_fork_choice* fc) {
  if (!fc) return;
  (void)hipSetDevice(fc->device);
  (void)hipDeviceSynchronize();   // calls queued on the caller's streams may still use the block
  (void)hipFree(fc->block);
  delete fc;
}

static Ctx* fc_ctx(const bls381_fork_choice* fc, int* rc) {
  Ctx* c = get_ctx(rc);
  if (c && c->device != fc->device) { t_err = "fork choice store belongs to another device"; *rc = BLS381_EARG; return nullptr; }
  return c;
}

size_t bls381_fork_choice_block_count(const bls381_fork_choice* fc) { return fc ? fc->tree.size() : 0; }
uint32_t bls381_fork_choice_node(const bls381_fork_choice* fc, const uint8_t root32[32]) {
  return fc && root32 ? fc->tree.find(root32) : FC_NONE;
}
int bls381_fork_choice_root(const bls381_fork_choice* fc, uint32_t node, uint8_t root32[32]) {
  if (!fc || !root32 || node >= fc->tree.size()) return BLS381_EARG;
  std::memcpy(root32, fc->tree.root[node].data(), 32);
  return 0;
}

int bls381_fork_choice_add_blocks(bls381_fork_choice* fc, size_t n, const uint8_t* roots32, const uint8_t* parent_roots32,
                                  const uint64_t* slots, uint32_t* node_out) {
  return guarded([&]() -> int {
    if (!fc || (n && (!roots32 || !parent_roots32 || !slots))) return BLS381_EARG;
    std::vector<uint32_t> ids(n);
    const size_t before = fc->tree.size();
    if (!fc->tree.add(n, roots32, parent_roots32, slots, fc->bcap, ids.data())) return BLS381_EARG;
    if (fc->tree.size() != before) fc->dirty = true;
    if (node_out) std::copy(ids.begin(), ids.end(), node_out);
    return 0;
  });
}

size_t bls381_fork_choice_on_attestations_workspace_size(size_t n_att) {
  if ((uint64_t)n_att > FC_SEQ_LIMIT) return 0;
  return carved_bytes([&](Bump& b) { b.take<fc_att>(n_att); });
}

int bls381_fork_choice_on_attestations_device(bls381_fork_choice* fc, size_t n_att, const uint32_t* h_att_off,
                                              const uint32_t* d_entries, const uint64_t* h_slots,
                                              const uint32_t* h_target_nodes, const uint8_t* d_ok, uint64_t* d_skipped,
                                              void* d_workspace, void* stream) {
  return guarded([&]() -> int {
    if (!fc || !d_skipped || !aligned8(d_skipped) || !aligned4(d_entries) ||
        (n_att && (!h_att_off || !h_slots || !h_target_nodes)))
      return BLS381_EARG;
    std::vector<fc_att> att;
    if (n_att && !fc_plan_batch(n_att, h_att_off, h_slots, h_target_nodes, fc->tree.size(), fc->seq, &att)) return BLS381_EARG;
    const size_t total = n_att ? (size_t)(h_att_off[n_att] - h_att_off[0]) : 0;
    if (total && (!d_entries || !d_workspace)) return BLS381_EARG;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPC(hipMemsetAsync(d_skipped, 0, 8, s));
    fc->seq += n_att;   // an attestation takes its number whether or not it leaves a message
    if (total == 0) return 0;
    Bump b(d_workspace, bls381_fork_choice_on_attestations_workspace_size(n_att));
    fc_att* d_att = b.take<fc_att>(n_att);
    Held<std::vector<fc_att>> hold(c->keep, s, std::move(att));
    HIPC(hipMemcpyAsync(d_att, hold->data(), n_att * sizeof(fc_att), hipMemcpyHostToDevice, s));
    const dim3 blk(EPOCH_BLOCK), grid(grid_for(total, EPOCH_BLOCK));
    for (int pass = 0; pass < 2; ++pass)
      LAUNCH("fc_attest", s, grid, blk, k_fc_attest, pass, (uint32_t)n_att, (const fc_att*)d_att, d_entries, d_ok,
             (uint64_t)fc->vcap, fc->d.key, fc->d.target, (unsigned long long*)d_skipped);
    return 0;
  });
}

int bls381_fork_choice_on_attestations(bls381_fork_choice* fc, size_t n_att, const uint32_t* att_off, const uint32_t* entries,
                                       const uint64_t* slots, const uint32_t* target_nodes, const uint8_t* ok,
                                       uint64_t* skipped_out) {
  return guarded([&]() -> int {
    if (!fc || !skipped_out || (n_att && (!att_off || !slots || !target_nodes))) return BLS381_EARG;
    const size_t end = n_att ? att_off[n_att] : 0;   // the device form checks the offsets before it queues anything
    if (n_att && att_off[n_att] != att_off[0] && !entries) return BLS381_EARG;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    HostCall hc(c);
    const size_t wsb = bls381_fork_choice_on_attestations_workspace_size(n_att);
    uint32_t* d_ent;
    uint8_t *d_ok, *d_ws;
    uint64_t* d_skipped;
    TRY(hc.carve([&](Bump& b) {
      d_ent = b.take<uint32_t>(end + 1);
      d_ok = b.take<uint8_t>(n_att + 1);
      d_skipped = b.take<uint64_t>(1);
      d_ws = b.take<uint8_t>(wsb + 1);
    }));
    if (entries) TRY(hc.upload(d_ent, entries, 4 * end));
    if (ok) TRY(hc.upload(d_ok, ok, n_att));
    TRY(bls381_fork_choice_on_attestations_device(fc, n_att, att_off, d_ent, slots, target_nodes, ok ? d_ok : nullptr,
                                                  d_skipped, d_ws, hc.s));
    uint64_t skipped = 0;
    TRY(hc.download(&skipped, d_skipped, 8));
    TRY(hc.finish());
    *skipped_out = skipped;
    return 0;
  });
}

int bls381_fork_choice_read_latest(bls381_fork_choice* fc, size_t first, size_t n, uint64_t* slots_out,
                                   uint32_t* targets_out) {
  return guarded([&]() -> int {
    if (!fc || first > fc->vcap || n > fc->vcap - first || (n && (!slots_out || !targets_out))) return BLS381_EARG;
    if (n == 0) return 0;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    HostCall hc(c);
    std::vector<uint64_t> keys(n);
    std::vector<uint32_t> targets(n);
    TRY(hc.download(keys.data(), fc->d.key + first, 8 * n));
    TRY(hc.download(targets.data(), fc->d.target + first, 4 * n));
    TRY(hc.finish());
    for (size_t k = 0; k < n; ++k) slots_out[k] = fc_key_slot(keys[k]);
    std::copy(targets.begin(), targets.end(), targets_out);
    return 0;
  });
}

int bls381_fork_choice_prune(bls381_fork_choice* fc, uint32_t new_anchor_node) {
  return guarded([&]() -> int {
    if (!fc || new_anchor_node >= fc->tree.size()) return BLS381_EARG;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    HIPC(hipDeviceSynchronize());   // calls queued on the caller's streams still use the old numbers
    HostCall hc(c);
    const size_t before = fc->tree.size();
    uint32_t* d_map;
    TRY(hc.carve([&](Bump& b) { d_map = b.take<uint32_t>(before); }));
    std::vector<uint32_t> map;
    fc->tree.prune(new_anchor_node, &map);
    fc->dirty = true;
    TRY(hc.upload(d_map, map.data(), 4 * before));
    LAUNCH("fc_remap", hc.s, dim3(grid_for(fc->vcap, EPOCH_BLOCK)), dim3(EPOCH_BLOCK), k_fc_remap, (uint64_t)fc->vcap,
           (const uint32_t*)d_map, fc->d.target);
    return hc.finish();   // `map` is read by the copy until here
  });
}

static bool fc_head_args_ok(const bls381_fork_choice* fc, uint32_t start_node, size_t n, const void* activation,
                            const void* exit_, const void* effective, size_t stride) {
  return fc && start_node < fc->tree.size() && n <= fc->vcap && field_ok(n, stride) &&
         (n == 0 || (activation && exit_ && effective));
}

int bls381_fork_choice_head_device(bls381_fork_choice* fc, uint32_t start_node, size_t n, const uint8_t* d_activation_epoch,
                                   const uint8_t* d_exit_epoch, const uint8_t* d_effective_balance, size_t stride,
                                   uint64_t epoch, uint32_t* d_head_out, uint64_t* d_weights_out, uint64_t* d_status_out,
                                   void* stream) {
  return guarded([&]() -> int {
    if (!fc_head_args_ok(fc, start_node, n, d_activation_epoch, d_exit_epoch, d_effective_balance, stride) || !d_head_out ||
        !aligned4(d_head_out) || !aligned8(d_weights_out) || !d_status_out || !aligned8(d_status_out))
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t B = fc->tree.size();
    const FcDev& d = fc->d;
    if (fc->dirty) {   // O(blocks) on the host and one copy, only after the tree has changed
      std::vector<uint32_t> pre, sub, node_at, rank, all(5 * B);
      fc->tree.number(&pre, &sub, &node_at, &rank);
      std::copy(fc->tree.parent.begin(), fc->tree.parent.end(), all.begin());
      std::copy(pre.begin(), pre.end(), all.begin() + B);
      std::copy(sub.begin(), sub.end(), all.begin() + 2 * B);
      std::copy(rank.begin(), rank.end(), all.begin() + 3 * B);
      std::copy(node_at.begin(), node_at.end(), all.begin() + 4 * B);
      Held<std::vector<uint32_t>> hold(c->keep, s, std::move(all));
      HIPC(hipMemcpyAsync(d.numbering, hold->data(), 4 * 5 * B, hipMemcpyHostToDevice, s));
      fc->dirty = false;
    }
    const uint32_t *parent = d.numbering, *pre = parent + B, *sub = pre + B, *rank = sub + B, *node_at = rank + B;
    unsigned long long *direct = d.sums, *best_count = d.sums + 2 * B;
    HIPC(hipMemsetAsync(d.sums, 0, 8 * 3 * B, s));
    HIPC(hipMemsetAsync(d.best_rank, 0, 4 * B, s));
    HIPC(hipMemsetAsync(d_status_out, 0, 8 * FCS_WORDS, s));
    const dim3 blk(EPOCH_BLOCK), nodes(grid_for(B, EPOCH_BLOCK));
    if (n)
      LAUNCH("fc_direct", s, dim3((unsigned)active_tiles(n), (unsigned)fc_node_tiles(B)), blk, k_fc_direct, (uint64_t)n,
             (const uint32_t*)d.target, make_u64_field(d_activation_epoch, stride), make_u64_field(d_exit_epoch, stride),
             make_u64_field(d_effective_balance, stride), epoch, (uint32_t)B, direct);
    LAUNCH("fc_scan", s, dim3(1), blk, k_fc_scan, (uint32_t)B, node_at, (const unsigned long long*)direct, d.prefix);
    LAUNCH("fc_count", s, nodes, blk, k_fc_count, (uint32_t)B, pre, sub, parent, (const uint64_t*)d.prefix, d.count,
           d_weights_out, d.jump_a, best_count, (unsigned long long*)d_status_out);
    for (int step = 0; step < 2; ++step)
      LAUNCH("fc_best", s, nodes, blk, k_fc_best, step, (uint32_t)B, parent, rank, (const uint64_t*)d.count,
             (const unsigned long long*)best_count, d.best_rank, d.jump_a);
    // the rounds depend on the capacity alone
    uint32_t *from = d.jump_a, *to = d.jump_b;
    for (uint32_t r = 0, rounds = fc_rounds((uint32_t)fc->bcap); r < rounds; ++r) {
      LAUNCH("fc_jump", s, nodes, blk, k_fc_jump, (uint32_t)B, (const uint32_t*)from, to, start_node,
             r + 1 == rounds ? d_head_out : (uint32_t*)nullptr);
      std::swap(from, to);
    }
    return 0;
  });
}

int bls381_fork_choice_head(bls381_fork_choice* fc, uint32_t start_node, size_t n, const uint8_t* activation_epoch,
                            const uint8_t* exit_epoch, const uint8_t* effective_balance, size_t stride, uint64_t epoch,
                            uint32_t* head_out, uint8_t head_root32[32], uint64_t* weights_out, uint64_t* status_out) {
  return guarded([&]() -> int {
    if (!fc_head_args_ok(fc, start_node, n, activation_epoch, exit_epoch, effective_balance, stride) || !head_out ||
        !status_out)
      return BLS381_EARG;
    int rc = 0;
    Ctx* c = fc_ctx(fc, &rc);
    if (!c) return rc;
    HostCall hc(c);
    HostFields hf;
    hf.add(activation_epoch, stride);
    hf.add(exit_epoch, stride);
    hf.add(effective_balance, stride);
    hf.plan(n);
    const size_t B = fc->tree.size();
    uint32_t* d_head;
    uint64_t *d_weights, *d_status;
    TRY(hc.carve([&](Bump& b) {
      hf.carve(b);
      d_weights = b.take<uint64_t>(B);
      d_status = b.take<uint64_t>(FCS_WORDS);
      d_head = b.take<uint32_t>(1);
    }));
    for (int g = 0; g < hf.ncopies; ++g) TRY(hc.upload(hf.dev_lo(g), hf.lo[g], hf.bytes[g]));
    TRY(bls381_fork_choice_head_device(fc, start_node, n, hf.dev(0), hf.dev(1), hf.dev(2), stride, epoch, d_head,
                                       weights_out ? d_weights : nullptr, d_status, hc.s));
    uint32_t head = FC_NONE;
    uint64_t status[FCS_WORDS];
    TRY(hc.download(&head, d_head, 4));
    TRY(hc.download(status, d_status, 8 * FCS_WORDS));
    if (weights_out) TRY(hc.download(weights_out, d_weights, 8 * B));
    TRY(hc.finish());
    if (head >= B) { t_err = "fork choice head: no head came back"; return BLS381_EHIP; }
    *head_out = head;
    if (head_root32) std::memcpy(head_root32, fc->tree.root[head].data(), 32);
    for (uint32_t x = 0; x < FCS_WORDS; ++x) status_out[x] = status[x];
    return 0;
  });
}

}  // extern "C"

// ---- multi-GPU over RCCL: one process per GPU, a communicator
// inside the library.  RCCL is opened with dlopen when a communicator is first
// made, so the library itself does not depend on it.
namespace {

struct RcclApi {
  void* h = nullptr;
  decltype(&ncclGetUniqueId) get_unique_id = nullptr;
  decltype(&ncclCommInitRank) comm_init_rank = nullptr;
  decltype(&ncclCommDestroy) comm_destroy = nullptr;
  decltype(&ncclAllGather) all_gather = nullptr;
  decltype(&ncclBroadcast) broadcast = nullptr;
  decltype(&ncclGetErrorString) error_string = nullptr;
};

RcclApi* rccl_api() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    // an RCCL the process has already loaded (e.g. PyTorch's torch/lib/librccl.so, soname
    // librccl.so.1) comes first, so the library and torch.distributed share one RCCL
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      api.h = dlopen(name, RTLD_NOW | RTLD_NOLOAD);
      if (api.h) break;
    }
    if (!api.h)
      for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) {
        api.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (api.h) break;
      }
    if (!api.h) return;
    api.get_unique_id = (decltype(api.get_unique_id))dlsym(api.h, "ncclGetUniqueId");
    api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(api.h, "ncclCommInitRank");
    api.comm_destroy = (decltype(api.comm_destroy))dlsym(api.h, "ncclCommDestroy");
    api.all_gather = (decltype(api.all_gather))dlsym(api.h, "ncclAllGather");
    api.broadcast = (decltype(api.broadcast))dlsym(api.h, "ncclBroadcast");
    api.error_string = (decltype(api.error_string))dlsym(api.h, "ncclGetErrorString");
  });
  if (!api.h || !api.get_unique_id || !api.comm_init_rank || !api.comm_destroy || !api.all_gather ||
      !api.broadcast || !api.error_string) {
    t_err = "RCCL (librccl.so) not loadable";
    return nullptr;
  }
  return &api;
}

// A communicator is RCCL's (one rank per process), or "virtual": one process
// plays all nranks ranks on its own GPU (the partition, per-rank partials and
// the rank-0 combination run unchanged; the all-gather is a device copy).
// RCCL refuses two ranks on one GPU, so the virtual form is how the sharded
// protocol is exercised with several ranks on a one-GPU box.
struct Comm {
  ncclComm_t comm = nullptr;
  bool virt = false;
  int nranks = 0, rank = -1, device = -1;
  uint8_t* rows = nullptr;   // gathered per-rank rows (device), grown on demand
  size_t rows_cap = 0;
  // the device-resident collectives leave their work queued on the caller's stream: the next
  // call that reuses `rows` waits for it (created with the communicator)
  hipEvent_t rows_ev = nullptr;
};
std::mutex g_comm_mu;
Comm g_comm;

int nccl_fail(RcclApi* api, const char* what, ncclResult_t r) {
  t_err = std::string(what) + ": " + api->error_string(r);
  return BLS381_EHIP;
}
#define NCCLC(api, x)                                            \
  do {                                                           \
    ncclResult_t r__ = (x);                                      \
    if (r__ != ncclSuccess) return nccl_fail(api, #x, r__);      \
  } while (0)

// Record-and-continue forms for the collective phases: a rank that fails still issues every
// collective its peers will (else they block in RCCL forever); the first error is kept in `err`.
#define HIPC_KEEP(err, x)                                            \
  do {                                                               \
    hipError_t e__ = (x);                                            \
    if (e__ != hipSuccess && !(err)) (err) = fail(#x, e__);          \
  } while (0)
#define NCCLC_KEEP(err, api, x)                                      \
  do {                                                               \
    ncclResult_t r__ = (x);                                          \
    if (r__ != ncclSuccess && !(err)) (err) = nccl_fail(api, #x, r__); \
  } while (0)

// Fp12 value (SoA, one item) -> 576 canonical bytes, or 576 zero bytes when its
// status is not OK (an honest partial product is never 0; a zero row makes the
// gathered product 0 and the verdict False on rank 0)
__global__ void __launch_bounds__(KBLOCK) k_fp12_row(const uint32_t* __restrict__ f, const uint8_t* __restrict__ st,
                                                     uint8_t* __restrict__ out576) {
  if (threadIdx.x >= 2) return;
  const int p = pr_odd() ? 1 : 0;
  const bool ok = st[0] == ST_OK;
  const fp12p_t a = soa_ld12(f, 1, 0);
  auto put = [&](int k, const fp2p_t& c) {
    uint8_t* o = out576 + 96 * k + 48 * p;
    if (ok) fp_plain_to_be48(o, fp_from_mont(c.v));
    else for (int b = 0; b < 48; ++b) o[b] = 0;
  };
  put(0, a.c0.c0); put(1, a.c0.c1); put(2, a.c0.c2); put(3, a.c1.c0); put(4, a.c1.c1); put(5, a.c1.c2);
}

// compressed partial aggregate, or 48 zero bytes (not a valid encoding) when its status is an error
__global__ void __launch_bounds__(KBLOCK) k_zero_if_error(const int32_t* __restrict__ st, uint8_t* __restrict__ buf,
                                                          uint32_t len) {
  const uint32_t t = threadIdx.x;
  if (t < len && st[0] != 0) buf[t] = 0;
}

Comm* comm_ctx(int* rc) {
  if (!g_comm.comm && !g_comm.virt) {
    t_err = "no communicator: call bls381_comm_init first";
    *rc = BLS381_EARG;
    return nullptr;
  }
  return &g_comm;
}

// Every collective exchanges rows through this buffer, allocated when the communicator is
// made: a rank whose local stage fails still has somewhere to put its zero / error row and
// takes part in every collective of the call (the other ranks would otherwise wait in RCCL
// forever).  Row blocks larger than the buffer go through it in pieces.
constexpr size_t COMM_ROWS_BYTES = 1 << 20;

int comm_rows(Comm* cm, size_t bytes, uint8_t** out) {
  if (cm->rows_cap < bytes) {
    t_err = "collective rows exceed the communicator buffer";
    *out = nullptr;
    return BLS381_EARG;
  }
  *out = cm->rows;
  return 0;
}

int comm_alloc_rows(Comm* cm) {
  HIPC(hipMalloc(&cm->rows, COMM_ROWS_BYTES));
  cm->rows_cap = COMM_ROWS_BYTES;
  if (!cm->rows_ev) HIPC(hipEventCreateWithFlags(&cm->rows_ev, hipEventDisableTiming));
  return 0;
}

// With g_comm_mu held: refuses a second communicator or more ranks than the row buffer serves,
// and gives `fresh` its ranks, device and rows.
int comm_prepare(Comm* fresh, int nranks, int rank, int device) {
  if (g_comm.comm || g_comm.virt) { t_err = "communicator already initialised"; return BLS381_EARG; }
  if (576 * ((size_t)nranks + 1) + 1024 > COMM_ROWS_BYTES) { t_err = "too many ranks"; return BLS381_EARG; }
  fresh->nranks = nranks;
  fresh->rank = rank;
  fresh->device = device;
  return comm_alloc_rows(fresh);
}

// The frame of a collective entry point: this thread's context, g_comm_mu held for the whole call,
// the communicator, and RCCL unless the communicator is virtual.  rc != 0: the call cannot start.
struct CommCall {
  int rc = 0;
  Ctx* c;
  std::unique_lock<std::mutex> lk;
  Comm* cm = nullptr;
  RcclApi* api = nullptr;
  CommCall() : c(get_ctx(&rc)) {
    if (!c) return;
    lk = std::unique_lock<std::mutex>(g_comm_mu);
    if (!(cm = comm_ctx(&rc))) return;
    if (!cm->virt && !(api = rccl_api())) rc = BLS381_ENODEV;
  }
};

// the ranks whose rows this process computes: its own, or all of them (virtual)
int first_rank(const Comm* cm) { return cm->virt ? 0 : cm->rank; }
int last_rank(const Comm* cm) { return cm->virt ? cm->nranks - 1 : cm->rank; }
bool is_root(const Comm* cm) { return cm->virt || cm->rank == 0; }

}  // namespace

extern "C" {

int bls381_comm_rccl_path(char* out, size_t cap) {
  if (!out || cap == 0) return BLS381_EARG;
  RcclApi* api = rccl_api();
  if (!api) return BLS381_ENODEV;
  Dl_info info;
  if (!dladdr((void*)api->get_unique_id, &info) || !info.dli_fname) { t_err = "dladdr failed"; return BLS381_EHIP; }
  std::snprintf(out, cap, "%s", info.dli_fname);
  return 0;
}

int bls381_comm_unique_id(uint8_t out[128]) {
  if (!out) return BLS381_EARG;
  RcclApi* api = rccl_api();
  if (!api) return BLS381_ENODEV;
  ncclUniqueId id;
  NCCLC(api, api->get_unique_id(&id));
  static_assert(sizeof(id) == 128, "ncclUniqueId size");
  std::memcpy(out, &id, sizeof(id));
  return 0;
}

int bls381_comm_init(int nranks, int rank, const uint8_t uid[128]) {
  if (nranks < 1 || rank < 0 || rank >= nranks || !uid) return BLS381_EARG;
  int rc = 0;
  Ctx* c = get_ctx(&rc);   // this thread's device (bls381_init) is the rank's GPU
  if (!c) return rc;
  RcclApi* api = rccl_api();
  if (!api) return BLS381_ENODEV;
  std::lock_guard<std::mutex> lk(g_comm_mu);
  Comm fresh;
  if ((rc = comm_prepare(&fresh, nranks, rank, c->device))) return rc;
  ncclUniqueId id;
  std::memcpy(&id, uid, sizeof(id));
  ncclComm_t comm;
  ncclResult_t nr = api->comm_init_rank(&comm, nranks, id, rank);
  if (nr != ncclSuccess) {
    (void)hipFree(fresh.rows);
    if (fresh.rows_ev) (void)hipEventDestroy(fresh.rows_ev);
    return nccl_fail(api, "ncclCommInitRank", nr);
  }
  fresh.comm = comm;
  g_comm = fresh;
  return 0;
}

int bls381_comm_init_virtual(int nranks) {
  if (nranks < 1) return BLS381_EARG;
  int rc = 0;
  Ctx* c = get_ctx(&rc);
  if (!c) return rc;
  std::lock_guard<std::mutex> lk(g_comm_mu);
  Comm fresh;
  if ((rc = comm_prepare(&fresh, nranks, 0, c->device))) return rc;
  fresh.virt = true;
  g_comm = fresh;
  return 0;
}

int bls381_comm_size(void) {
  std::lock_guard<std::mutex> lk(g_comm_mu);
  return (g_comm.comm || g_comm.virt) ? g_comm.nranks : 0;
}
int bls381_comm_rank(void) {
  std::lock_guard<std::mutex> lk(g_comm_mu);
  return (g_comm.comm || g_comm.virt) ? g_comm.rank : -1;
}

void bls381_comm_destroy(void) {
  std::lock_guard<std::mutex> lk(g_comm_mu);
  // the device-resident sharded calls return with their collectives still queued on the
  // caller's stream (rows_ev is recorded after the last one): the communicator must outlive them
  if (g_comm.rows_ev) (void)hipEventSynchronize(g_comm.rows_ev);
  if (g_comm.comm) {
    (void)hipDeviceSynchronize();
    RcclApi* api = rccl_api();
    if (api) (void)api->comm_destroy(g_comm.comm);
  }
  if (g_comm.rows) {
    (void)hipDeviceSynchronize();
    (void)hipFree(g_comm.rows);
  }
  if (g_comm.rows_ev) (void)hipEventDestroy(g_comm.rows_ev);
  g_comm = Comm();
}

// Collective calls: every rank issues the same collectives in the same order whatever happens
// locally.  A rank whose local stage fails (a plan, a workspace or a HIP error) contributes a
// zero row -- never an honest partial -- so the call's verdict is False / its aggregate is
// flagged, joins every collective, and returns its own error code afterwards.  g_comm_mu is
// held for the whole call (comm state, the row buffer and the collective sequence).

int bls381_verify_multiple_sharded(size_t n, const uint8_t* pks, const uint8_t* msgs, size_t msg_len,
                                   const uint8_t sig[96], const uint8_t dom8[8]) {
  if ((n && (!pks || (!msgs && msg_len))) || !sig || !dom8 || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  CommCall cc;
  if (cc.rc) return cc.rc;
  Ctx* c = cc.c;
  Comm* cm = cc.cm;
  RcclApi* api = cc.api;
  int rc = 0;
  HostCall hc(c);   // holds c->mu for the whole call
  const size_t R = (size_t)cm->nranks;
  hipStream_t s = c->q.main;
  uint8_t* d_rows;
  if ((rc = comm_rows(cm, 576 * R + 576 + 64, &d_rows))) return rc;   // fits by construction (init)
  if (cm->rows_ev) (void)hipEventSynchronize(cm->rows_ev);   // a device-form call may still use them
  uint8_t* d_v = d_rows + 576 * R + 576;
  // local stage: this rank's row(s); on failure the row is zero (verdict False on rank 0)
  int local = guarded([&]() -> int {
    // distinct message k (first-appearance order) -> rank k mod nranks: a message's
    // pubkey group never straddles two ranks (bls381_amd/sharding.py partition_messages)
    std::unordered_map<std::string, uint32_t> order;
    std::vector<uint32_t> owner(n);
    for (size_t i = 0; i < n; ++i) {
      std::string key((const char*)msgs + msg_len * i, msg_len);
      auto it = order.find(key);
      if (it == order.end()) it = order.emplace(key, (uint32_t)order.size()).first;
      owner[i] = it->second % (uint32_t)R;
    }
    int lrc = 0;
    for (int r = first_rank(cm); r <= last_rank(cm); ++r) {
      std::vector<uint8_t> my_pks, my_msgs;
      for (size_t i = 0; i < n; ++i) {
        if ((int)owner[i] != r) continue;
        my_pks.insert(my_pks.end(), pks + 48 * i, pks + 48 * (i + 1));
        my_msgs.insert(my_msgs.end(), msgs + msg_len * i, msgs + msg_len * (i + 1));
      }
      const uint32_t off[2] = {0, (uint32_t)(my_pks.size() / 48)};
      const int with_sig = r == 0 ? 1 : 0;
      Bump b(nullptr, 0);
      uint32_t* f;
      uint8_t* st;
      if ((lrc = vm_host(hc, 1, off, my_pks.data(), my_msgs.data(), msg_len, sig, dom8, &with_sig, b, &f, &st)))
        return lrc;
      // this rank's row (576 B, zero when a member is invalid): in place when virtual
      uint8_t* row = cm->virt ? d_rows + 576 * (size_t)r : d_rows + 576 * R;
      LAUNCH("fp12_row", s, dim3(1), dim3(KBLOCK), k_fp12_row, (const uint32_t*)f, (const uint8_t*)st, row);
      HIPC(hipStreamSynchronize(s));   // the next rank's plan reuses the workspace
    }
    return 0;
  });
  if (local) {
    (void)hipStreamSynchronize(s);
    if (cm->virt) return local;
    // a zero row (never an honest partial), ordered before the all-gather on the same stream
    if (hipMemsetAsync(d_rows + 576 * R, 0, 576, s) != hipSuccess) return local;   // row unusable: RCCL cannot help
  }
  if (!cm->virt) NCCLC(api, api->all_gather(d_rows + 576 * R, d_rows, 576, ncclUint8, cm->comm, s));
  if (is_root(cm)) {   // one final exponentiation, on rank 0 (verdict 0 if it cannot run)
    const int root = guarded([&]() -> int {
      int lrc;
      HIPC(hipMemsetAsync(d_v, 0, 1, s));
      if ((lrc = ensure_ws(c, 12 * FPW * R * 4 + 4 * R + 65536))) return lrc;
      Bump b(c->ws, c->ws_cap);
      uint32_t* g = b.take<uint32_t>(12 * FP_LIMBS * R);
      uint8_t* gst = b.take<uint8_t>(R);
      HIPC(hipMemsetAsync(gst, ST_OK, R, s));
      LAUNCH("fp12_from_bytes", s, dim3(grid_for(2 * R)), dim3(KBLOCK), k_fp12_from_bytes, R, (const uint8_t*)d_rows, g);
      Held<ProductPasses> passes(c->keep, s, plan_products({0u, (uint32_t)R}));
      TRY(run_product_passes(b, s, *passes, g, gst, R));
      LAUNCH_FE(s, (size_t)1, g, gst, d_v);
      return 0;
    });
    if (root) {
      (void)hipStreamSynchronize(s);
      (void)hipMemsetAsync(d_v, 0, 1, s);
      if (!local) local = root;
    }
  }
  if (!cm->virt) NCCLC(api, api->broadcast(d_v, d_v, 1, ncclUint8, 0, cm->comm, s));
  uint8_t v = 0;
  HIPC(hipMemcpyAsync(&v, d_v, 1, hipMemcpyDeviceToHost, s));
  TRY(hc.finish());
  if (local) return local;
  return v ? 1 : 0;
}

// The device form's per-rank row: the partial sum as a Jacobian point (x, y, z: 3 x 14 Montgomery
// words) and a bad flag (any member failed to decode), 44 words.  Rank 0 sums the rows without
// decompressing anything (the host form ships compressed partials and decodes them: one Fp square
// root per rank on rank 0's critical path).
constexpr size_t AGG_ROW_WORDS = 44;
__global__ void __launch_bounds__(64) k_agg_jac_row(const uint32_t* __restrict__ jac, const uint8_t* __restrict__ bad,
                                                   uint32_t* __restrict__ row) {
  const uint32_t t = threadIdx.x;
  if (t < 42) row[t] = jac[t];   // SoA of one group: the 42 words in (coordinate, limb) order
  if (t == 42) row[42] = bad[0] ? 1u : 0u;
  if (t == 43) row[43] = 0;
}
// one wave: lane j sums rows j, j + 64, ...; an LDS tree combines the 64 partial sums; lane 0
// compresses the total (or flags it, when any rank's row is bad)
__global__ void __launch_bounds__(64) k_agg_sum_rows(uint32_t R, const uint32_t* __restrict__ rows,
                                                    uint8_t* __restrict__ out48, int32_t* __restrict__ status) {
  __shared__ uint32_t part[64][42];
  __shared__ uint32_t anybad;
  const uint32_t t = threadIdx.x;
  if (t == 0) anybad = 0;
  __syncthreads();
  jac_t<fp_t> acc = jac_infinity<fp_t>();
  uint32_t bad = 0;
  for (uint32_t r = t; r < R; r += 64) {
    const uint32_t* row = rows + (size_t)r * AGG_ROW_WORDS;
    jac_t<fp_t> p;
#pragma unroll
    for (int k = 0; k < FP_LIMBS; ++k) { p.x.w[k] = row[k]; p.y.w[k] = row[14 + k]; p.z.w[k] = row[28 + k]; }
    bad |= row[42];
    acc = jac_add(acc, p);
  }
  if (bad) atomicOr(&anybad, 1u);
  auto put = [&](const jac_t<fp_t>& a) {
#pragma unroll
    for (int k = 0; k < FP_LIMBS; ++k) { part[t][k] = a.x.w[k]; part[t][14 + k] = a.y.w[k]; part[t][28 + k] = a.z.w[k]; }
  };
  auto get = [&](uint32_t j) {
    jac_t<fp_t> a;
#pragma unroll
    for (int k = 0; k < FP_LIMBS; ++k) { a.x.w[k] = part[j][k]; a.y.w[k] = part[j][14 + k]; a.z.w[k] = part[j][28 + k]; }
    return a;
  };
  put(acc);
  __syncthreads();
  for (uint32_t w = 32; w >= 1; w >>= 1) {
    if (t < w) put(jac_add(get(t), get(t + w)));
    __syncthreads();
  }
  if (t != 0) return;
  if (anybad) {
    for (int b = 0; b < 48; ++b) out48[b] = 0;
    *status = BLS381_EINVAL_POINT;
    return;
  }
  pt_compress(out48, get(0));
  *status = 0;
}

// Device-resident form of bls381_aggregate_pubkeys_sharded (include/bls381.h): this rank's keys
// are already in HBM and every rank receives the aggregate and the status in HBM, on the caller's
// stream; the call returns with its work queued (no host copy, no synchronisation).  This rank's
// partial sum travels as a Jacobian row (k_agg_jac_row), the rows are all-gathered and rank 0 sums
// them (k_agg_sum_rows) and compresses once; the aggregate and status are broadcast.
size_t bls381_aggregate_pubkeys_sharded_device_workspace_size(size_t n_local) {
  return bls381_aggregate_pubkeys_batch_workspace_size(1, n_local);
}

// the protocol with g_comm_mu held: this rank's n_local keys at d_pks (a virtual communicator: the
// whole call), aggregate and status into device memory, all on stream s
static int agg_sharded_impl(Ctx* c, Comm* cm, RcclApi* api, size_t n_local, const uint8_t* d_pks, uint8_t* d_out48,
                            int32_t* d_status, void* d_workspace, hipStream_t s, int force_err = 0) {
  int rc = 0;
  const size_t R = (size_t)cm->nranks;
  const size_t row_b = 4 * AGG_ROW_WORDS;
  uint8_t* d_rows;   // R rows, then this rank's own, then the sum (48 B) and the status
  if ((rc = comm_rows(cm, row_b * (R + 1) + 64 + 64, &d_rows))) return rc;   // fits by construction (init)
  uint8_t* d_sum = d_rows + row_b * (R + 1);
  int32_t* d_st = (int32_t*)(d_sum + 64);
  if (cm->rows_ev) (void)hipStreamWaitEvent(s, cm->rows_ev, 0);   // before any collective: no early return
  const size_t ws_local = bls381_aggregate_pubkeys_sharded_device_workspace_size(n_local);
  // virtual: one process plays every rank over the whole call, split as the host form splits it
  const size_t base = n_local / R, extra = n_local % R;
  int local = 0;
  for (int r = first_rank(cm); r <= last_rank(cm); ++r) {
    const size_t rr = (size_t)r;
    uint32_t* row = (uint32_t*)(cm->virt ? d_rows + row_b * rr : d_rows + row_b * R);
    const size_t lo = cm->virt ? rr * base + (rr < extra ? rr : extra) : 0;
    const size_t cnt = cm->virt ? base + (rr < extra ? 1 : 0) : n_local;
    // force_err: the caller could not stage its keys (d_workspace may be null): a flagged row only
    const int lrc = force_err ? force_err : guarded([&]() -> int {
      const uint32_t off1[2] = {0, (uint32_t)cnt};
      Held<AggPlan> hold(c->keep, s, plan_agg(1, off1, 1));
      const uint32_t* jac;
      const uint8_t* bad;
      size_t used = 0;
      int e;
      // the ranks of a virtual communicator reuse the workspace in stream order
      if ((e = run_agg<fp_t>(*hold, 1, d_pks + 48 * lo, d_workspace, s, &jac, &bad, &used, ws_local, nullptr,
                             policy_flags(0))))
        return e;
      LAUNCH("agg_jac_row", s, dim3(1), dim3(64), k_agg_jac_row, jac, bad, row);
      return 0;
    });
    if (lrc) {
      (void)hipMemsetAsync(row, 0, row_b, s);                   // z = 0 and the bad flag set:
      (void)hipMemsetAsync((uint8_t*)row + 4 * 42, 1, 1, s);   // the sum is flagged
      if (!local) local = lrc;
    }
  }
  if (local && cm->virt) return local;
  if (!cm->virt) NCCLC(api, api->all_gather(d_rows + row_b * R, d_rows, row_b, ncclUint8, cm->comm, s));
  if (is_root(cm)) {
    const int root = guarded([&]() -> int {
      LAUNCH("agg_sum_rows", s, dim3(1), dim3(64), k_agg_sum_rows, (uint32_t)R, (const uint32_t*)d_rows, d_sum, d_st);
      return 0;
    });
    if (root) {
      static const int32_t err = BLS381_EHIP;   // a copy source that outlives the queued copy
      (void)hipMemsetAsync(d_sum, 0, 48, s);
      (void)hipMemcpyAsync(d_st, &err, 4, hipMemcpyHostToDevice, s);
      if (!local) local = root;
    }
  }
  if (!cm->virt) {
    NCCLC(api, api->broadcast(d_sum, d_sum, 48, ncclUint8, 0, cm->comm, s));
    NCCLC(api, api->broadcast(d_st, d_st, 4, ncclUint8, 0, cm->comm, s));
  }
  HIPC(hipMemcpyAsync(d_out48, d_sum, 48, hipMemcpyDeviceToDevice, s));
  HIPC(hipMemcpyAsync(d_status, d_st, 4, hipMemcpyDeviceToDevice, s));
  if (cm->rows_ev) HIPC(hipEventRecord(cm->rows_ev, s));
  return local;
}

int bls381_aggregate_pubkeys_sharded_device(size_t n_local, const uint8_t* d_pks, uint8_t* d_out48,
                                            int32_t* d_status, void* d_workspace, void* stream) {
  if (!d_out48 || !d_status || !d_workspace || (n_local && !d_pks)) return BLS381_EARG;
  CommCall cc;
  if (cc.rc) return cc.rc;
  return agg_sharded_impl(cc.c, cc.cm, cc.api, n_local, d_pks, d_out48, d_status, d_workspace, (hipStream_t)stream);
}

int bls381_aggregate_pubkeys_sharded(size_t n, const uint8_t* pks, uint8_t out[48]) {
  // the device form's protocol over this rank's contiguous range (sizes differing by at most one,
  // sharding.shard_range; a virtual communicator takes the whole call), copied in from host memory
  if (!out || (n && !pks)) return BLS381_EARG;
  CommCall cc;
  if (cc.rc) return cc.rc;
  Ctx* c = cc.c;
  Comm* cm = cc.cm;
  RcclApi* api = cc.api;
  int rc = 0;
  if (cm->rows_ev) (void)hipEventSynchronize(cm->rows_ev);   // a device-form call may still use the rows
  const size_t R = (size_t)cm->nranks;
  HostCall hc(c);
  hipStream_t s = hc.s;
  const size_t base = n / R, extra = n % R, rr = (size_t)cm->rank;
  const size_t lo = cm->virt ? 0 : rr * base + (rr < extra ? rr : extra);
  const size_t cnt = cm->virt ? n : base + (rr < extra ? 1 : 0);
  const size_t wsl = bls381_aggregate_pubkeys_sharded_device_workspace_size(cnt);
  // result and status in the rows buffer's unused tail (the protocol uses its head)
  uint8_t* d_res = cm->rows + cm->rows_cap - 64;
  uint8_t* d_pks = nullptr;
  const uint8_t* d_in = nullptr;
  void* w = nullptr;
  int local = carve_ws(c, [&](Bump& b) {
    d_pks = b.take<uint8_t>(48 * cnt + 1);
    w = b.take<uint8_t>(wsl);
  });
  if (!local) {
    if (cnt && hipMemcpyAsync(d_pks, pks + 48 * lo, 48 * cnt, hipMemcpyHostToDevice, s) != hipSuccess)
      local = fail("hipMemcpyAsync", hipGetLastError());
    d_in = d_pks;
  }
  // a rank that cannot stage its keys still issues every collective of the call, with a flagged row
  // (with force_err set the impl runs no local stage, so it never touches the workspace)
  rc = agg_sharded_impl(c, cm, api, local ? 0 : cnt, local ? nullptr : d_in, d_res, (int32_t*)(d_res + 48),
                        local ? nullptr : w, s, local);
  int32_t st = 0;
  TRY(hc.download(out, d_res, 48));
  TRY(hc.download(&st, d_res + 48, 4));
  TRY(hc.finish());
  if (local) return local;
  return rc ? rc : st;
}

int bls381_verify_multiple_batch_sharded(size_t n_calls, const uint32_t* call_off, const uint8_t* pks,
                                         const uint8_t* msgs, size_t msg_len, const uint8_t* sigs,
                                         const uint8_t* dom8s, uint8_t* verdicts) {
  if (!call_off || !sigs || !dom8s || !verdicts || msg_len > BLS381_MSG_MAX) return BLS381_EARG;
  if (call_off[n_calls] && (!pks || (!msgs && msg_len))) return BLS381_EARG;
  CommCall cc;
  if (cc.rc) return cc.rc;
  Ctx* c = cc.c;
  Comm* cm = cc.cm;
  RcclApi* api = cc.api;
  int rc = 0;
  const size_t R = (size_t)cm->nranks;
  const size_t base = n_calls / R, extra = n_calls % R, width = base + (extra ? 1 : 0);
  if (width == 0) return 0;
  std::vector<uint8_t> rows(width * R, 0);
  int local = 0;
  for (int r = first_rank(cm); r <= last_rank(cm); ++r) {
    const size_t rr = (size_t)r;
    const size_t lo = rr * base + (rr < extra ? rr : extra), cnt = base + (rr < extra ? 1 : 0);
    if (!cnt) continue;
    const int lrc = guarded([&]() -> int {
      std::vector<uint32_t> off(cnt + 1);
      for (size_t k = 0; k <= cnt; ++k) off[k] = call_off[lo + k] - call_off[lo];
      const size_t k0 = call_off[lo];
      return bls381_verify_multiple_batch(cnt, off.data(), pks ? pks + 48 * k0 : nullptr,
                                          msgs ? msgs + msg_len * k0 : nullptr, msg_len, sigs + 96 * lo,
                                          dom8s + 8 * lo, rows.data() + width * rr);
    });
    if (lrc) {   // this rank's calls count as False for the others; it returns the error
      std::fill(rows.begin() + width * rr, rows.begin() + width * (rr + 1), (uint8_t)0);
      if (!local) local = lrc;
    }
  }
  if (!cm->virt) {   // all-gather the verdict rows (each rank filled its own), through the comm buffer
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t s = c->q.main;
    uint8_t* d_rows;
    const size_t piece = std::min(width, COMM_ROWS_BYTES / (R + 1));
    if ((rc = comm_rows(cm, piece * (R + 1), &d_rows))) return rc;   // fits by construction
    if (cm->rows_ev) (void)hipEventSynchronize(cm->rows_ev);   // a device-form call may still use them
    // every rank issues the same all-gathers (width and piece are the same everywhere) even after
    // an error of its own, so no peer waits on a collective this rank skipped
    int err = 0;
    for (size_t at = 0; at < width; at += piece) {
      const size_t w = std::min(piece, width - at);
      HIPC_KEEP(err, hipMemcpyAsync(d_rows + piece * R, rows.data() + width * (size_t)cm->rank + at, w,
                                    hipMemcpyHostToDevice, s));
      NCCLC_KEEP(err, api, api->all_gather(d_rows + piece * R, d_rows, w, ncclUint8, cm->comm, s));
      for (size_t q = 0; q < R; ++q)
        HIPC_KEEP(err, hipMemcpyAsync(rows.data() + width * q + at, d_rows + w * q, w, hipMemcpyDeviceToHost, s));
      HIPC_KEEP(err, hipStreamSynchronize(s));
    }
    if (err) return err;
  }
  for (size_t q = 0; q < R; ++q) {
    const size_t qlo = q * base + (q < extra ? q : extra), qcnt = base + (q < extra ? 1 : 0);
    std::memcpy(verdicts + qlo, rows.data() + width * q, qcnt);
  }
  return local;
}

}  // extern "C"

// ------------------------------------------ randomized batch verification --
// Opt-in small-exponent batch test over independent bls_verify items (kernels:
// bls381_kernels.hpp "randomized batch verification").  Per-item verdicts are
// kept: a sub-batch that fails, and every item whose signature is outside G2, is
// re-verified item by item with the default pipeline.
namespace {

// Randomized sub-batches of B items: the items pair up on the split Miller loop's quads
// (k_rb_ml_lines -> k_ml_accum), so a sub-batch has B/2 item-pair values plus its
// signature-sum value; the split loop runs in chunks of at most RB_ML_CHUNK item pairs.
constexpr size_t RB_ML_CHUNK = 32768;
// the MSM's point lists hold 16-bit point numbers (2 per item): at most 2^15 items per sub-batch
constexpr size_t RB_BATCH_MAX = 32768;
// sub-batches up to this size sum their signatures with the bucket MSM (k_rb_msm_*)
constexpr size_t RB_MSM_MAX_B = 256;
size_t rb_slots(size_t n, size_t B) { return ((n + B - 1) / B) * (B / 2 + 1); }
size_t rb_ml_chunk(size_t n, size_t B) { return std::min<size_t>(((n + B - 1) / B) * (B / 2), RB_ML_CHUNK); }
size_t rb_ws_size(size_t n, size_t B) {
  const size_t nb = (n + B - 1) / B, nslots = rb_slots(n, B), ch_ml = rb_ml_chunk(n, B);
  size_t s = verify_ws_size(n, false) + 4 * 65536;   // decodes + hash: no split-loop line buffer
  s += align256(2 * FPW * n) + 3 * align256(n) + align256(6 * FPW * n) + align256(n);   // R1, statuses, R2, zeros
  const size_t ch = nb + n / CHUNK_MIN + 1;                                              // R2 sums per sub-batch
  s += 3 * (align256(ch * sizeof(agg_chunk)) + align256(ch * 6 * FPW) + align256(ch));
  s += align256(4 * FPW * nb) + align256(nb);                                           // signature sums
  s += align256(4 * ML_L_WORDS_PER_ITEM * ch_ml) + align256(ch_ml);                     // line products
  s += 2 * (align256(12 * FPW * nslots) + align256(nslots) + align256(nslots * sizeof(agg_chunk)));
  s += 2 * align256(nb) + align256(64);
  // the signature sums as a bucket MSM (k_rb_msm_*): list starts, point lists, buckets, windows, sums
  s += align256(4 * nb * RB_MSM_W * (RB_MSM_D + 1)) + align256(2 * nb * RB_MSM_W * 2 * B) +
       align256(6 * FPW * nb * RB_MSM_W * RB_MSM_D) + align256(6 * FPW * nb * RB_MSM_W) + align256(6 * FPW * nb);
  // the per-item fallback over m <= n items (verify_nf(m) can exceed verify_nf(n) by the octet path's 2 per item)
  const size_t oct = std::min<size_t>(n, BLS_ML_OCT_MAX_N);
  s += align256(4 * n) + align256(n) + verify_ws_size(n) + align256(12 * FPW * 2 * oct) + align256(2 * oct);
  return s;
}

int run_verify_randomized(Ctx* c, size_t n, const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs,
                          const uint8_t* doms, const uint8_t* seed32, size_t B, uint8_t* d_verdicts, void* ws,
                          size_t ws_cap, hipStream_t s, uint64_t* stats) {
  const NoBalanceScope no_balance;
  const size_t nb = (n + B - 1) / B, hb = B / 2, nslots = rb_slots(n, B), ch_ml = rb_ml_chunk(n, B);
  Bump b(ws, ws_cap);
  VerifyWs w = carve_verify(b.take<uint8_t>(verify_ws_size(n, false)), n, false);
  uint32_t* r1 = b.take<uint32_t>(2 * FP_LIMBS * n);
  uint8_t* r1_st = b.take<uint8_t>(n);
  uint8_t* cls = b.take<uint8_t>(n);
  uint32_t* r2 = b.take<uint32_t>(6 * FP_LIMBS * n);
  uint8_t* zeros = b.take<uint8_t>(n);
  uint8_t* d_seed = b.take<uint8_t>(64);
  const dim3 g1(grid_for(n)), g2(grid_for(2 * n)), blk(KBLOCK);
  const int chk = check_subgroups();
  // async copy sources (the seed, the plan's chunk lists, the product passes below): held for
  // the error returns -- the last line is reached with the stream synchronised
  Held<std::vector<uint8_t>> seed(c->keep, s, std::vector<uint8_t>(seed32, seed32 + 32));
  HIPC(hipMemcpyAsync(d_seed, seed->data(), 32, hipMemcpyHostToDevice, s));
  HIPC(hipMemsetAsync(zeros, 0, n, s));
  // Miller values: B/2 item-pair slots per sub-batch + its signature-sum slot
  uint32_t* f = b.take<uint32_t>(12 * FP_LIMBS * nslots);
  uint8_t* fst = b.take<uint8_t>(nslots);
  uint32_t* mlL = b.take<uint32_t>(ML_L_WORDS_PER_ITEM * ch_ml);
  uint8_t* mlst = b.take<uint8_t>(ch_ml);
  // per sub-batch sum of [r_i] sig_i (planned here; runs on the priority stream)
  std::vector<uint32_t> off(nb + 1);
  for (size_t k = 0; k <= nb; ++k) off[k] = (uint32_t)std::min(n, k * B);
  Held<AggPlan> plan(c->keep, s, plan_agg(nb, off.data()));
  uint32_t* s_aff = b.take<uint32_t>(4 * FP_LIMBS * nb);
  uint8_t* s_st = b.take<uint8_t>(nb);
  {
    // Order: the one-lane prologue as one launch (k_prologue_1<1>: the hash's
    // search + root, decode + [r_i] pk_i, the codec-only signature decode), then the signatures' G2
    // test and the item classes (k_rb_g2_test, lane pairs); the signature branch (sums, their affine
    // form, their Miller loops) on the priority stream beside k_hash_bp and the item Miller loops.
    // Round 5's order (decode_g1, decode_g2 with the G2 test and the sums in sequence, then the pair
    // hash and k_rb_scale_g1) measured 2.36 against 2.43-2.53 M/s (r06b); removed.
    Fork fk(c->q, s);
    LAUNCH("rb_prologue", s, dim3(3 * grid_for(n)), blk, k_prologue_1<1>, n, pks, sigs, msgs, (uint32_t)32, doms, 8,
           (const uint8_t*)d_seed, w.pk_aff, w.pk_st, w.sig_aff, w.sig_st, w.h_aff, r1, r1_st, policy_flags(chk),
           policy_flags(0));
    LAUNCH("rb_g2_test", s, g2, blk, k_rb_g2_test, n, (const uint32_t*)w.sig_aff, w.sig_st, (const uint8_t*)w.pk_st,
           cls, chk);
    // the signature branch's window and combine chains and the sums' loops are latency-bound
    // launches of a few waves each: beside the full-chip ones on the main stream
    HIPC(fk.branch(c->q.prio));
    hipStream_t sb = c->q.prio.stream;
    // BLS381_RB_MSM (measurement knob): 1 (default) the sub-batch sums sum_i [r_i] sig_i as one bucket
    // MSM per sub-batch (k_rb_msm_*); 0 a joint 32-bit ladder per item (k_rb_scale_g2) and a tree sum
    // The MSM gives each (sub-batch, window, digit) bucket to one lane pair, which adds its ~B/16
    // points in sequence: past RB_MSM_MAX_B the buckets become long dependent chains on a few lane
    // pairs (r04e: B = 256 already equal to the ladder, 2.307 / 2.303 M/s), so larger sub-batches
    // take the per-item ladder and the tree sum, whose work spreads over every item.
    static const int rb_msm = env_knob("BLS381_RB_MSM", 1);
    const uint32_t* sjac;
    const uint8_t* sbad;
    if (rb_msm && B <= RB_MSM_MAX_B) {
      uint32_t* moff = b.take<uint32_t>(nb * RB_MSM_W * (RB_MSM_D + 1));
      uint16_t* midx = b.take<uint16_t>(nb * RB_MSM_W * 2 * B);
      uint32_t* mbucket = b.take<uint32_t>(6 * FP_LIMBS * nb * RB_MSM_W * RB_MSM_D);
      uint32_t* mwin = b.take<uint32_t>(6 * FP_LIMBS * nb * RB_MSM_W);
      uint32_t* mjac = b.take<uint32_t>(6 * FP_LIMBS * nb);
      LAUNCH("rb_msm_sort", sb, dim3((unsigned)nb), blk, k_rb_msm_sort, n, B, (const uint8_t*)d_seed,
             (const uint8_t*)w.sig_st, (const uint8_t*)w.pk_st, moff, midx);
      const size_t tasks = nb * RB_MSM_W * (RB_MSM_D - 1);
      LAUNCH("rb_msm_bucket", sb, dim3(grid_for(2 * tasks)), blk, k_rb_msm_bucket, n, B, nb, (const uint32_t*)w.sig_aff,
             (const uint32_t*)moff, (const uint16_t*)midx, mbucket);
      LAUNCH("rb_msm_window", sb, dim3(grid_for(2 * nb * RB_MSM_W)), blk, k_rb_msm_window, nb,
             (const uint32_t*)mbucket, mwin);
      LAUNCH("rb_msm_combine", sb, dim3(grid_for(2 * nb)), blk, k_rb_msm_combine, nb, (const uint32_t*)mwin, mjac);
      sjac = mjac;
      sbad = zeros;
    } else {
      LAUNCH("rb_scale_g2", sb, g2, blk, k_rb_scale_g2, n, (const uint8_t*)d_seed, (const uint32_t*)w.sig_aff,
             (const uint8_t*)w.sig_st, (const uint8_t*)w.pk_st, r2);
      size_t used = 0;
      uint8_t* sub = b.take<uint8_t>(0);
      if (int e = run_agg<fp2p_t>(*plan, nb, nullptr, sub, sb, &sjac, &sbad, &used, b.left(), nullptr, 0, r2, zeros, n))
        return e;
      b.off += used;
    }
    LAUNCH("agg_g2_affine", sb, dim3(grid_for(2 * nb)), blk, k_agg_g2_affine, nb, sjac, sbad, s_aff, s_st);
    // (r06: the sums' loop waves at raised issue priority, s_setprio 3, slowed k_hash_bp beside them
    // from 3.6 to 5.4 ms: 2.47 against 2.60 M/s at B = 64, same box; removed)
    LAUNCH("rb_miller_sig", sb, dim3(grid_for(4 * nb)), blk, k_rb_miller_sig, nb, hb, (const uint32_t*)s_aff,
           (const uint8_t*)s_st, nslots, f, fst);
    // the cofactor map beside the signature branch
    LAUNCH("hash_bp", s, g2, blk, k_hash_bp, n, w.h_aff, w.f_st);
    // the batched items two per Miller accumulator: lines of both pairs on a quad, then f^2 L
    // on quads (2^15 accumulators per 2^16 items: a pair launch would leave SIMDs half empty)
    const size_t nq = nb * hb;
    for (size_t q0 = 0; q0 < nq; q0 += ch_ml) {
      const size_t cnt = std::min(ch_ml, nq - q0);
      LAUNCH("rb_miller_lines", s, dim3(grid_for(4 * cnt)), blk, k_rb_ml_lines, n, q0, cnt, (const uint32_t*)w.h_aff,
             (const uint8_t*)w.f_st, (const uint32_t*)r1, (const uint8_t*)r1_st, (const uint8_t*)cls, mlL, mlst);
      LAUNCH("rb_miller_accum", s, dim3(grid_for(4 * cnt)), blk, k_ml_accum_q, nslots, q0, cnt, (const uint32_t*)mlL,
             (const uint8_t*)mlst, f, fst, hb);
    }
    HIPC(fk.join());
  }
  int rc = 0;
  std::vector<uint32_t> seg(nb + 1);
  for (size_t k = 0; k <= nb; ++k) seg[k] = (uint32_t)(k * (hb + 1));
  Held<ProductPasses> passes(c->keep, s, plan_products(seg));
  TRY(run_product_passes(b, s, *passes, f, fst, nslots));
  uint8_t* bv = b.take<uint8_t>(nb);
  LAUNCH_FE(s, nb, f, fst, bv);
  std::vector<uint8_t> h_bv(nb), h_cls(n);
  HIPC(hipMemcpyAsync(h_bv.data(), bv, nb, hipMemcpyDeviceToHost, s));
  HIPC(hipMemcpyAsync(h_cls.data(), cls, n, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));   // the plans and the seed copy are done with as well
  // verdicts: bad -> 0; batched in a passing sub-batch -> 1; the rest one by one
  std::vector<uint8_t> v(n, 0);
  std::vector<uint32_t> single;
  uint64_t n_batched = 0, n_failed = 0;
  for (size_t k = 0; k < nb; ++k) n_failed += h_bv[k] ? 0 : 1;
  for (size_t i = 0; i < n; ++i) {
    if (h_cls[i] == RB_BAD) continue;
    if (h_cls[i] == RB_BATCH && h_bv[i / B]) { v[i] = 1; ++n_batched; continue; }
    single.push_back((uint32_t)i);
  }
  if (stats) { stats[0] = n_batched; stats[1] = single.size(); stats[2] = n_failed; }
  const size_t m = single.size();
  if (m) {
    // the per-item pairings over the points this call already decoded and hashed: the
    // default pipeline minus its decodes and hash_to_G2 (the G2 test of the signatures is done)
    uint32_t* d_idx = b.take<uint32_t>(m);
    uint8_t* gv = b.take<uint8_t>(m);
    VerifyWs wm = carve_verify(b.take<uint8_t>(verify_ws_size(m)), m);
    HIPC(hipMemcpyAsync(d_idx, single.data(), 4 * m, hipMemcpyHostToDevice, s));
    const uint32_t rows = 2 * FP_LIMBS;
    LAUNCH("gather_points", s, dim3(grid_for(rows * m)), blk, k_gather_soa, m, (const uint32_t*)d_idx,
           (const uint32_t*)w.pk_aff, n, rows, 1u, wm.pk_aff);
    LAUNCH("gather_points", s, dim3(grid_for(2 * rows * m)), blk, k_gather_soa, m, (const uint32_t*)d_idx,
           (const uint32_t*)w.sig_aff, n, rows, 2u, wm.sig_aff);
    LAUNCH("gather_points", s, dim3(grid_for(2 * rows * m)), blk, k_gather_soa, m, (const uint32_t*)d_idx,
           (const uint32_t*)w.h_aff, n, rows, 2u, wm.h_aff);
    LAUNCH("gather_status", s, dim3(grid_for(m)), blk, k_gather_st, m, (const uint32_t*)d_idx,
           (const uint8_t*)w.pk_st, (const uint8_t*)w.sig_st, wm.pk_st, wm.sig_st);
    if ((rc = run_verify_pairings(m, wm, gv, s, false))) return rc;
    std::vector<uint8_t> h_gv(m);
    HIPC(hipMemcpyAsync(h_gv.data(), gv, m, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    for (size_t k = 0; k < m; ++k) v[single[k]] = h_gv[k];
  }
  HIPC(hipMemcpyAsync(d_verdicts, v.data(), n, hipMemcpyHostToDevice, s));
  HIPC(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

extern "C" {

size_t bls381_verify_batch_randomized_workspace_size(size_t n, size_t batch) {
  return (batch < 2 || batch % 2 || batch > RB_BATCH_MAX) ? 0 : rb_ws_size(n ? n : 1, batch);
}

int bls381_verify_batch_randomized_device(size_t n, const uint8_t* d_pks, const uint8_t* d_msgs32,
                                          const uint8_t* d_sigs, const uint8_t* d_dom8s, const uint8_t seed[32],
                                          size_t batch, uint8_t* d_verdicts, void* d_workspace, void* stream,
                                          uint64_t* stats) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n == 0) return 0;
    if (!d_pks || !d_msgs32 || !d_sigs || !d_dom8s || !seed || !d_verdicts || !d_workspace || batch < 2 || batch % 2 ||
        batch > RB_BATCH_MAX)
      return BLS381_EARG;
    return run_verify_randomized(c, n, d_pks, d_msgs32, d_sigs, d_dom8s, seed, batch, d_verdicts, d_workspace,
                                 rb_ws_size(n, batch), (hipStream_t)stream, stats);
  });
}

int bls381_verify_batch_randomized(size_t n, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs,
                                   const uint8_t* dom8s, const uint8_t seed[32], size_t batch,
                                   uint8_t* verdicts_out) {
  return guarded([&]() -> int {
    int rc = 0;
    Ctx* c = get_ctx(&rc);
    if (!c) return rc;
    if (n == 0) return 0;
    if (!pks || !msgs32 || !sigs || !dom8s || !seed || !verdicts_out || batch < 2 || batch % 2 || batch > RB_BATCH_MAX)
      return BLS381_EARG;
    HostCall hc(c);
    const size_t wsb = rb_ws_size(n, batch);
    VerifyIn d;
    TRY(hc.carve([&](Bump& b) { d.carve(b, n, wsb); }));
    TRY(d.upload(hc, n, pks, msgs32, sigs, dom8s));
    TRY(run_verify_randomized(c, n, d.pks, d.msgs, d.sigs, d.doms, seed, batch, d.v, d.ws, wsb, hc.s, nullptr));
    TRY(hc.download(verdicts_out, d.v, n));
    return hc.finish();
  });
}

}  // extern "C"
