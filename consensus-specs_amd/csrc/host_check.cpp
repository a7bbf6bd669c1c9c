// Host unit-test build of the device arithmetic headers -- TEST INFRASTRUCTURE.
//
// g++ compiles the exact headers the gfx950 kernels use so that, in a container
// with no GPU, every layer (Fp ... Fp12, codecs, subgroup checks, hash_to_G2,
// Miller loop, final exponentiation) can be checked against oracle/ by
// tests/test_host_arith.py.  This library is loaded only by tests; it is not a
// fallback and the product library (libbls381.so) never links it.
//
// Byte conventions (all big-endian, plain / non-Montgomery values):
//   Fp 48 B;  Fp2 96 B = re || im;  Fp12 576 B = a0,a1,a2,b0,b1,b2 (each Fp2)
//   G1 affine 96 B = x || y;  G2 affine 192 B = x || y (each Fp2)
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "bls381_hash.hpp"
#include "bls381_pairing.hpp"
#include "bls381_plan.hpp"
#include "bls381_shuffle.hpp"
#include "bls381_epoch.hpp"
#include "bls381_ssz.hpp"
#include "bls381_merkle.hpp"
#include "bls381_deptree.hpp"
#include "bls381_listtree.hpp"
#include "bls381_keytable.hpp"

// ---- stand-ins for the HIP types and runtime calls that bls381_scope.hpp is written against.
// Every call appends one line to a log (hc_scope_scenario, at the end of this file, returns it);
// the k-th call after a scenario's "begin" (destroys not counted) can be made to fail.  Internal linkage throughout: this
// library is loaded into processes that also hold the real runtime and exports no hip* name.
namespace {
struct StandIn {
  char kind;   // 'S' stream, 'E' event
  int id;
  bool complete = false;   // an event: what hipEventQuery reports (set by the scenario)
};
typedef StandIn* hipStream_t;
typedef StandIn* hipEvent_t;
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorNotReady = 600;
constexpr unsigned hipStreamNonBlocking = 1, hipEventDisableTiming = 2;

struct StandInState {
  std::string log;
  int next_id = 0, calls = 0, fail_at = 0;
  bool counting = false;
} g_si;

void si_log(const std::string& line) { g_si.log += line + "\n"; }
std::string si_name(const StandIn* h) { return h ? std::string(1, h->kind) + std::to_string(h->id) : "null"; }
// logs the call; the failing call is logged as "FAIL <call>" and returns its own code, 1000 + k
hipError_t si_call(const std::string& line) {
  if (g_si.counting && ++g_si.calls == g_si.fail_at) {
    si_log("FAIL " + line);
    return 1000 + g_si.calls;
  }
  si_log(line);
  return hipSuccess;
}
hipError_t si_create(char kind, const char* what, StandIn** out) {
  StandIn* h = new StandIn{kind, g_si.next_id};
  const hipError_t e = si_call(std::string(what) + " " + si_name(h));
  if (e != hipSuccess) { delete h; return e; }
  ++g_si.next_id;
  *out = h;
  return hipSuccess;
}
hipError_t si_destroy(const char* what, StandIn* h) {   // never the failing call: nothing could free h then
  si_log(std::string(what) + " " + si_name(h));
  delete h;
  return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return si_create('S', "stream_create", s); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return si_create('S', "stream_create", s); }
hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) {
  *lo = 0;
  *hi = -1;
  return si_call("priority_range");
}
hipError_t hipStreamSynchronize(hipStream_t s) { return si_call("sync " + si_name(s)); }
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { return si_call("wait " + si_name(s) + " " + si_name(e)); }
hipError_t hipStreamDestroy(hipStream_t s) { return si_destroy("stream_destroy", s); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return si_create('E', "event_create", e); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { return si_call("record " + si_name(e) + " " + si_name(s)); }
hipError_t hipEventQuery(hipEvent_t e) { return e->complete ? hipSuccess : hipErrorNotReady; }   // not logged
hipError_t hipEventDestroy(hipEvent_t e) { return si_destroy("event_destroy", e); }
}  // namespace

#include "bls381_scope.hpp"

using namespace bls381;

namespace {
fp_t ld(const uint8_t* p) { return fp_to_mont(fp_plain_from_be48(p)); }
void st(uint8_t* p, const fp_t& a) { fp_plain_to_be48(p, fp_from_mont(a)); }
fp2_t ld2(const uint8_t* p) { fp2_t r; r.c0 = ld(p); r.c1 = ld(p + 48); return r; }
void st2(uint8_t* p, const fp2_t& a) { st(p, a.c0); st(p + 48, a.c1); }
fp12_t ld12(const uint8_t* p) {
  fp12_t r;
  r.c0.c0 = ld2(p); r.c0.c1 = ld2(p + 96); r.c0.c2 = ld2(p + 192);
  r.c1.c0 = ld2(p + 288); r.c1.c1 = ld2(p + 384); r.c1.c2 = ld2(p + 480);
  return r;
}
void st12(uint8_t* p, const fp12_t& a) {
  st2(p, a.c0.c0); st2(p + 96, a.c0.c1); st2(p + 192, a.c0.c2);
  st2(p + 288, a.c1.c0); st2(p + 384, a.c1.c1); st2(p + 480, a.c1.c2);
}
aff_t<fp_t> ldg1(const uint8_t* p) { aff_t<fp_t> a; a.x = ld(p); a.y = ld(p + 48); return a; }
aff_t<fp2_t> ldg2(const uint8_t* p) { aff_t<fp2_t> a; a.x = ld2(p); a.y = ld2(p + 96); return a; }
}  // namespace

extern "C" {

// one-reduction combinations on raw normalized limbs (14 x u32, values < 2q, Montgomery
// or not -- the reduction is mod 2q only): op 0 a+b, 1 a-b, 2 -a, 3 2a, 4 a+b-c, 5 a+b+c,
// 6 a-b-c, 7 3a-2b, 8 3a+2b, 9..16 k*a for k = op-8 (k = 1..8)
void hc_fp_lc_raw(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* o) {
  fp_t x, y, z, r;
  for (int i = 0; i < 14; ++i) { x.w[i] = a[i]; y.w[i] = b[i]; z.w[i] = c[i]; }
  switch (op) {
    case 0: r = fp_add(x, y); break;
    case 1: r = fp_sub(x, y); break;
    case 2: r = fp_neg(x); break;
    case 3: r = fp_dbl(x); break;
    case 4: r = fp_add_sub(x, y, z); break;
    case 5: r = fp_add3(x, y, z); break;
    case 6: r = fp_sub2(x, y, z); break;
    case 7: r = fp_3m2(x, y); break;
    case 8: r = fp_3p2(x, y); break;
    default: r = fp_mul_small(x, op - 8); break;
  }
  for (int i = 0; i < 14; ++i) o[i] = r.w[i];
}

void hc_fp_mul(const uint8_t* a, const uint8_t* b, uint8_t* o) { st(o, fp_mul(ld(a), ld(b))); }
void hc_fp_add(const uint8_t* a, const uint8_t* b, uint8_t* o) { st(o, fp_add(ld(a), ld(b))); }
void hc_fp_sub(const uint8_t* a, const uint8_t* b, uint8_t* o) { st(o, fp_sub(ld(a), ld(b))); }
void hc_fp_half(const uint8_t* a, uint8_t* o) { st(o, fp_half(ld(a))); }
void hc_fp_inv(const uint8_t* a, uint8_t* o) { st(o, fp_inv(ld(a))); }
void hc_fp_inv_xgcd(const uint8_t* a, uint8_t* o) { st(o, fp_inv_xgcd(ld(a))); }
uint64_t hc_inv_fallbacks() { return g_inv_fallbacks; }
int hc_fp_sqrt(const uint8_t* a, uint8_t* o) {
  fp_t r;
  const bool ok = fp_sqrt(r, ld(a));
  st(o, r);
  return ok;
}
int hc_fp_legendre(const uint8_t* a) { return fp_legendre(ld(a)); }
// raw Montgomery multiply on plain limbs (checks fp_mul's bound handling directly)
void hc_fp_mont_mul_raw(const uint8_t* a, const uint8_t* b, uint8_t* o) {
  fp_plain_to_be48(o, fp_mul(fp_plain_from_be48(a), fp_plain_from_be48(b)));
}

void hc_fp2_mul(const uint8_t* a, const uint8_t* b, uint8_t* o) { st2(o, fp2_mul(ld2(a), ld2(b))); }
void hc_fp2_sqr(const uint8_t* a, uint8_t* o) { st2(o, fp2_sqr(ld2(a))); }
void hc_fp2_inv(const uint8_t* a, uint8_t* o) { st2(o, fp2_inv(ld2(a))); }
int hc_fp2_sqrt_select(const uint8_t* a, uint8_t* o) {
  fp2_t r;
  if (!fp2_sqrt(r, ld2(a))) return 0;
  st2(o, g2_select_root(r));
  return 1;
}

// lazy-operand stress: raw (Montgomery-domain) limbs in, operands are the lazy
// sums X+Y and Z+U (each summand < 2^384 as given); returns raw weakly-reduced limbs
static fp2_t ldraw2(const uint8_t* p) { fp2_t r; r.c0 = fp_plain_from_be48(p); r.c1 = fp_plain_from_be48(p + 48); return r; }
static void straw2(uint8_t* p, const fp2_t& a) { fp_plain_to_be48(p, a.c0); fp_plain_to_be48(p + 48, a.c1); }
void hc_fp2_mul_lazy_raw(const uint8_t* x, const uint8_t* y, const uint8_t* z, const uint8_t* u, uint8_t* o) {
  straw2(o, fp2_mul(fp2_add_lazy(ldraw2(x), ldraw2(y)), fp2_add_lazy(ldraw2(z), ldraw2(u))));
}

// Karabina compressed squaring (lazy reduction, bls381_lazy.hpp) on raw Montgomery-domain
// limbs: in/out = (g2, g3, g4, g5) as 4 x 96 bytes, inputs any values < 2q
void hc_cyc_csqr_raw(const uint8_t* in, uint8_t* out) {
  cyc_bc<fp2_t> g;
  g.g2 = ldraw2(in); g.g3 = ldraw2(in + 96); g.g4 = ldraw2(in + 192); g.g5 = ldraw2(in + 288);
  const cyc_bc<fp2_t> r = cyc_csqr(g);
  straw2(out, r.g2); straw2(out + 96, r.g3); straw2(out + 192, r.g4); straw2(out + 288, r.g5);
}

}  // extern "C"
namespace {
// raw limb words (14 x u32 per Fp, Montgomery domain, nothing converted), as hc_fp_lc_raw
fp_t rw(const uint32_t*& p) { fp_t r; for (int i = 0; i < 14; ++i) r.w[i] = *p++; return r; }
fp2_t rw2(const uint32_t*& p) { fp2_t r; r.c0 = rw(p); r.c1 = rw(p); return r; }
fp12_t rw12(const uint32_t*& p) {
  fp12_t r;
  r.c0.c0 = rw2(p); r.c0.c1 = rw2(p); r.c0.c2 = rw2(p); r.c1.c0 = rw2(p); r.c1.c1 = rw2(p); r.c1.c2 = rw2(p);
  return r;
}
void ww(uint32_t*& o, const fp_t& a) { for (int i = 0; i < 14; ++i) *o++ = a.w[i]; }
void ww2(uint32_t*& o, const fp2_t& a) { ww(o, a.c0); ww(o, a.c1); }
void ww12(uint32_t*& o, const fp12_t& a) {
  ww2(o, a.c0.c0); ww2(o, a.c0.c1); ww2(o, a.c0.c2); ww2(o, a.c1.c0); ww2(o, a.c1.c1); ww2(o, a.c1.c2);
}
jac_t<fp2_t> rwjac(const uint32_t*& p) { jac_t<fp2_t> r; r.x = rw2(p); r.y = rw2(p); r.z = rw2(p); return r; }
aff_t<fp2_t> rwaff(const uint32_t*& p) { aff_t<fp2_t> r; r.x = rw2(p); r.y = rw2(p); return r; }
int wwjac(uint32_t*& o, const jac_t<fp2_t>& a) { ww2(o, a.x); ww2(o, a.y); ww2(o, a.z); return jac_is_inf(a) ? 1 : 0; }
}  // namespace
extern "C" {

// the Montgomery products themselves on raw limbs (lazy operands as fp_mul_body / fp_sqr_body allow):
// op 0 fp_mul(a, b), 1 fp_sqr(a)
void hc_raw_fp(int op, const uint32_t* in, uint32_t* out) {
  const fp_t a = rw(in);
  ww(out, op == 0 ? fp_mul(a, rw(in)) : fp_sqr(a));
}

// The one-lane forms on raw limbs, for the operands and expectations of the device check library
// (dev_check.hip, tests/devcheck_vectors.py): `in` / `out` are sequences of raw Fp in the order of
// the operation's arguments (Fp2 = c0, c1; Fp12 = a0, a1, a2, b0, b1, b2; points x, y[, z]).
// Returns the predicate the device probe reports in its flag (infinity, degenerate), else 0.
int hc_raw_fp2(int op, const uint32_t* in, uint64_t aux, uint32_t* out) {
  switch (op) {
    case 0: { const fp2_t a = rw2(in), b = rw2(in); ww2(out, fp2_mul(a, b)); return 0; }   // lazy operands allowed
    case 1: ww2(out, fp2_sqr(rw2(in))); return 0;
    case 2: ww2(out, fp2_inv(rw2(in))); return 0;
    default: {   // cyc_csqr x aux on (g2, g3, g4, g5)
      cyc_bc<fp2_t> g;
      g.g2 = rw2(in); g.g3 = rw2(in); g.g4 = rw2(in); g.g5 = rw2(in);
      for (uint64_t j = 0; j < aux; ++j) g = cyc_csqr(g);
      ww2(out, g.g2); ww2(out, g.g3); ww2(out, g.g4); ww2(out, g.g5);
      return 0;
    }
  }
}
// The fused tower combinations on raw Fp2 operands in argument order: op 0 fp2_add_xi_sub2 (a, m, b, c),
// 1 fp2_sub2_add_xi (m, a, b, c), 2 fp2_sub2_add (m, a, b, c), 3 fp2_sub_sub_xi (t, a, b),
// 4 fp2_sub_sub_dbl (x, y, z), 5 fp2_dbl_sub2 (x, y, z), 6 fp2_3a_xi_b_m2c (a, b, c), 7 fp2_2a_b_m3c (a, b, c).
// Returns the number of operands read, -1 for an unknown op.
int hc_raw_fp2_lc(int op, const uint32_t* in, uint32_t* out) {
  if (op < 0 || op > 7) return -1;
  const int n = op <= 2 ? 4 : 3;
  fp2_t x[4];
  for (int j = 0; j < n; ++j) x[j] = rw2(in);
  switch (op) {
    case 0: ww2(out, fp2_add_xi_sub2(x[0], x[1], x[2], x[3])); break;
    case 1: ww2(out, fp2_sub2_add_xi(x[0], x[1], x[2], x[3])); break;
    case 2: ww2(out, fp2_sub2_add(x[0], x[1], x[2], x[3])); break;
    case 3: ww2(out, fp2_sub_sub_xi(x[0], x[1], x[2])); break;
    case 4: ww2(out, fp2_sub_sub_dbl(x[0], x[1], x[2])); break;
    case 5: ww2(out, fp2_dbl_sub2(x[0], x[1], x[2])); break;
    case 6: ww2(out, fp2_3a_xi_b_m2c(x[0], x[1], x[2])); break;
    default: ww2(out, fp2_2a_b_m3c(x[0], x[1], x[2])); break;
  }
  return n;
}
// op 0 fp6_mul (a, b: 3 Fp2 each -> 3 Fp2), 1 fp12_mul_by_line_pair_inl (f, then the lines c0, c1, c2 and
// d0, d1, d2 -> f (l l'), 6 Fp2), 2 line_pair_product alone (c0..d2 -> 6 Fp2)
int hc_raw_tower(int op, const uint32_t* in, uint32_t* out) {
  if (op == 0) {
    fp6_t a, b;
    a.c0 = rw2(in); a.c1 = rw2(in); a.c2 = rw2(in);
    b.c0 = rw2(in); b.c1 = rw2(in); b.c2 = rw2(in);
    const fp6_t r = fp6_mul(a, b);
    ww2(out, r.c0); ww2(out, r.c1); ww2(out, r.c2);
    return 0;
  }
  if (op != 1 && op != 2) return -1;
  fp12_t f = fp12_one<fp2_t>();
  if (op == 1) f = rw12(in);
  fp2_t l[6];
  for (int j = 0; j < 6; ++j) l[j] = rw2(in);
  const fp12_t L = line_pair_product(l[0], l[1], l[2], l[3], l[4], l[5]);
  ww12(out, op == 1 ? fp12_mul_by_line_pair_inl(f, L) : L);
  return 0;
}
// op 0 mul, 1 sqr, 2 cyclotomic sqr, 3 mul_by_line (f, c0, c1, c2), 4 frob (aux = p), 5 inv, 6 final_exp,
// 7 cyc_exp_x, 8 cyc_exp_x_gs, 9 cyc_decompress (g2..g5, 1 / (4 g2))
int hc_raw_fp12(int op, const uint32_t* in, uint64_t aux, uint32_t* out) {
  const fp12_t f = op == 9 ? fp12_one<fp2_t>() : rw12(in);
  switch (op) {
    case 0: ww12(out, fp12_mul(f, rw12(in))); return 0;
    case 1: ww12(out, fp12_sqr(f)); return 0;
    case 2: ww12(out, fp12_cyclotomic_sqr(f)); return 0;
    case 3: { const fp2_t c0 = rw2(in), c1 = rw2(in), c2 = rw2(in); ww12(out, fp12_mul_by_line(f, c0, c1, c2)); return 0; }
    case 4: ww12(out, fp12_frob(f, (int)aux)); return 0;
    case 5: ww12(out, fp12_inv(f)); return 0;
    case 6: ww12(out, final_exp(f)); return 0;
    case 7: ww12(out, cyc_exp_x<fp2_t, 1>(f)); return 0;
    case 8: ww12(out, cyc_exp_x_gs(f)); return 0;
    default: {
      cyc_bc<fp2_t> g;
      g.g2 = rw2(in); g.g3 = rw2(in); g.g4 = rw2(in); g.g5 = rw2(in);
      ww12(out, cyc_decompress(g, rw2(in)));
      return 0;
    }
  }
}
// op 0 jac_dbl, 1 jac_add_aff, 2 jac_add, 3 g2_psi_jac, 4 jac_mul_u64 (aux = k >= 1), 5 g2_mul_bp
int hc_raw_g2(int op, const uint32_t* in, uint64_t aux, uint32_t* out) {
  switch (op) {
    case 0: return wwjac(out, jac_dbl(rwjac(in)));
    case 1: { const jac_t<fp2_t> p = rwjac(in); return wwjac(out, jac_add_aff(p, rwaff(in))); }
    case 2: { const jac_t<fp2_t> p = rwjac(in); return wwjac(out, jac_add(p, rwjac(in))); }
    case 3: return wwjac(out, g2_psi_jac(rwjac(in)));
    case 4: return wwjac(out, jac_mul_u64(rwaff(in), aux));
    default: return wwjac(out, g2_mul_bp(rwaff(in)));
  }
}
// jac_mul_2x32 (the randomized batch's joint 32-bit ladder) on raw limbs: [k0] a + [k1] s, Jacobian out.
// group 0: E(Fp), in = a.x, a.y, s.x, s.y (4 Fp) -> X, Y, Z (3 Fp); group 1: E'(Fp2), in = 8 Fp -> 6 Fp.
// Returns whether the result is the point at infinity, -1 for an unknown group.
int hc_raw_mul_2x32(int group, const uint32_t* in, uint32_t k0, uint32_t k1, uint32_t* out) {
  if (group == 0) {
    aff_t<fp_t> a, s;
    a.x = rw(in); a.y = rw(in); s.x = rw(in); s.y = rw(in);
    const jac_t<fp_t> r = jac_mul_2x32(a, s, k0, k1);
    ww(out, r.x); ww(out, r.y); ww(out, r.z);
    return jac_is_inf(r) ? 1 : 0;
  }
  if (group != 1) return -1;
  const aff_t<fp2_t> a = rwaff(in), s = rwaff(in);
  return wwjac(out, jac_mul_2x32(a, s, k0, k1));
}
// Miller loop of n <= 2 pairs, each Q (x, y in Fp2) then P (x, y in Fp); returns degenerate
int hc_raw_miller(int n, const uint32_t* in, uint32_t* out) {
  aff_t<fp2_t> Q[2];
  g1_line_pre P[2];
  if (n < 1 || n > 2) return -1;
  for (int k = 0; k < n; ++k) {
    Q[k] = rwaff(in);
    aff_t<fp_t> p; p.x = rw(in); p.y = rw(in);
    P[k] = g1_prepare(p);
  }
  bool degen = false;
  ww12(out, n == 1 ? miller_loop_n<1>(Q, P, degen) : miller_loop_n<2>(Q, P, degen));
  return degen ? 1 : 0;
}

void hc_fp12_mul(const uint8_t* a, const uint8_t* b, uint8_t* o) { st12(o, fp12_mul(ld12(a), ld12(b))); }
void hc_fp12_sqr(const uint8_t* a, uint8_t* o) { st12(o, fp12_sqr(ld12(a))); }
void hc_fp12_inv(const uint8_t* a, uint8_t* o) { st12(o, fp12_inv(ld12(a))); }
void hc_fp12_frob(const uint8_t* a, int p, uint8_t* o) { st12(o, fp12_frob(ld12(a), p)); }
void hc_fp12_cyc_sqr(const uint8_t* a, uint8_t* o) { st12(o, fp12_cyclotomic_sqr(ld12(a))); }
void hc_fp12_mul_by_line(const uint8_t* f, const uint8_t* c0, const uint8_t* c1, const uint8_t* c2, uint8_t* o) {
  st12(o, fp12_mul_by_line(ld12(f), ld2(c0), ld2(c1), ld2(c2)));
}
void hc_final_exp(const uint8_t* a, uint8_t* o) { st12(o, final_exp(ld12(a))); }
// the verdict form (final_exp_check): 1 / 0, or 2 with fb = 0 when a snapshot had g2 = 0
int hc_final_exp_check(const uint8_t* a, int fb) {
  return fb ? final_exp_check<fp2_t, 1>(ld12(a)) : final_exp_check<fp2_t, 0>(ld12(a));
}

// lax != 0: py_ecc 1.7.0's codec, else the spec's strict one
int hc_g1_decompress(const uint8_t* b48, uint8_t* aff96, int lax) {
  aff_t<fp_t> a;
  const int s = g1_decompress(a, b48, lax != 0);
  if (s == PT_OK) { st(aff96, a.x); st(aff96 + 48, a.y); }
  return s;
}
int hc_g2_decompress(const uint8_t* b96, uint8_t* aff192, int lax) {
  aff_t<fp2_t> a;
  const int s = g2_decompress(a, b96, lax != 0);
  if (s == PT_OK) { st2(aff192, a.x); st2(aff192 + 96, a.y); }
  return s;
}
void hc_g1_compress_aff(const uint8_t* aff96, uint8_t* b48) { g1_compress(b48, jac_from_aff(ldg1(aff96))); }
void hc_g2_compress_aff(const uint8_t* aff192, uint8_t* b96) { g2_compress_aff(b96, ldg2(aff192)); }
int hc_g1_in_subgroup(const uint8_t* aff96) { return g1_in_subgroup(ldg1(aff96)); }
int hc_g2_in_subgroup(const uint8_t* aff192) { return g2_in_subgroup(ldg2(aff192)); }

int hc_hash_to_g2(const uint8_t* msg, uint32_t mlen, const uint8_t* dom8, uint8_t* aff192, uint8_t* comp96) {
  aff_t<fp2_t> c;
  const int trials = hash_to_g2_candidate(c, msg, mlen, dom8);
  aff_t<fp2_t> h;
  if (!jac_to_aff(h, g2_mul_cofactor(c))) return -2;
  st2(aff192, h.x); st2(aff192 + 96, h.y);
  g2_compress_aff(comp96, h);
  return trials;
}
void hc_sha256(const uint8_t* msg, uint32_t len, uint8_t* out32) {
  uint32_t d[8];
  sha256(d, msg, len);
  for (int i = 0; i < 8; ++i) {
    out32[4 * i] = (uint8_t)(d[i] >> 24); out32[4 * i + 1] = (uint8_t)(d[i] >> 16);
    out32[4 * i + 2] = (uint8_t)(d[i] >> 8); out32[4 * i + 3] = (uint8_t)d[i];
  }
}

// Miller loop of n <= 4 pairs (G2 affine 192 B each, G1 affine 96 B each)
int hc_miller_loop(int n, const uint8_t* q192, const uint8_t* p96, uint8_t* o576) {
  aff_t<fp2_t> Q[4];
  g1_line_pre P[4];
  if (n < 1 || n > 4) return -1;
  for (int k = 0; k < n; ++k) { Q[k] = ldg2(q192 + 192 * k); P[k] = g1_prepare(ldg1(p96 + 96 * k)); }
  fp12_t f;
  bool degen = false;
  switch (n) {
    case 1: f = miller_loop_n<1>(Q, P, degen); break;
    case 2: f = miller_loop_n<2>(Q, P, degen); break;
    case 3: f = miller_loop_n<3>(Q, P, degen); break;
    default: f = miller_loop_n<4>(Q, P, degen); break;
  }
  st12(o576, f);
  return degen ? 1 : 0;
}

// ---- whole-call semantics of the gfx950 pipelines, same headers, one thread
// (bls381_capi.hip run_verify_batch / run_vm_batch): decode, the subgroup
// policy (strict != 0: BLS381_POLICY_STRICT, the spec's codec and subgroup checks; else
// py_ecc 1.7.0's lax codec and no subgroup check), py_ecc's infinity short circuit
// (a pair with an infinite point is 1), a degenerate Miller loop -> False,
// one final exponentiation.  Returns 1 / 0.
static bool g1_in(const aff_t<fp_t>& a) { return g1_in_subgroup(a); }
static bool g2_in(const aff_t<fp2_t>& a) { return g2_in_subgroup(a); }

static int verify_pairs(int np, const aff_t<fp2_t>* Q, const aff_t<fp_t>* Pa) {
  // pairs one Miller loop each (products of f), as k_miller_pairs_batch
  fp12_t f = fp12_one<fp2_t>();
  for (int k = 0; k < np; ++k) {
    bool degen = false;
    g1_line_pre P = g1_prepare(Pa[k]);
    f = fp12_mul(f, miller_loop_n<1>(&Q[k], &P, degen));
    if (degen) return 0;
  }
  return fp12_is_one(final_exp(f)) ? 1 : 0;
}

int hc_verify(const uint8_t* pk48, const uint8_t* msg, uint32_t mlen, const uint8_t* sig96, const uint8_t* dom8,
              int strict) {
  aff_t<fp_t> P;
  aff_t<fp2_t> S;
  const int sp = g1_decompress(P, pk48, !strict);
  const int ss = g2_decompress(S, sig96, !strict);
  if (sp == PT_BAD || ss == PT_BAD) return 0;
  if (strict && ((sp == PT_OK && !g1_in(P)) || (ss == PT_OK && !g2_in(S)))) return 0;
  aff_t<fp2_t> Q[2];
  aff_t<fp_t> Pa[2];
  int np = 0;
  if (ss == PT_OK) {
    Q[np] = S;
    Pa[np].x = G1_VGEN_X_M;   // -[3(x^2-1)] g1, paired with the signature (k_hash_g2)
    Pa[np].y = G1_VGEN_NEGY_M;
    ++np;
  }
  if (sp == PT_OK) {
    aff_t<fp2_t> c;
    hash_to_g2_candidate(c, msg, mlen, dom8);
    if (jac_to_aff(Q[np], g2_mul_bp(c))) { Pa[np] = P; ++np; }
  }
  return verify_pairs(np, Q, Pa);
}

// n pubkeys / messages (mlen bytes each); pubkeys grouped by distinct message
int hc_verify_multiple(size_t n, const uint8_t* pks, const uint8_t* msgs, uint32_t mlen, const uint8_t* sig96,
                       const uint8_t* dom8, int strict) {
  std::map<std::string, jac_t<fp_t>> groups;
  for (size_t i = 0; i < n; ++i) {
    const std::string key((const char*)msgs + mlen * i, mlen);
    auto it = groups.find(key);
    if (it == groups.end()) it = groups.emplace(key, jac_infinity<fp_t>()).first;
    aff_t<fp_t> a;
    const int s = g1_decompress(a, pks + 48 * i, !strict);
    if (s == PT_BAD || (s == PT_OK && strict && !g1_in(a))) return 0;
    if (s == PT_OK) it->second = jac_add_aff(it->second, a);
  }
  aff_t<fp2_t> S;
  const int ss = g2_decompress(S, sig96, !strict);
  if (ss == PT_BAD || (ss == PT_OK && strict && !g2_in(S))) return 0;
  std::vector<aff_t<fp2_t>> Q;
  std::vector<aff_t<fp_t>> Pa;
  for (auto& g : groups) {
    aff_t<fp_t> a;
    if (!jac_to_aff(a, g.second)) continue;
    aff_t<fp2_t> c, h;
    hash_to_g2_candidate(c, (const uint8_t*)g.first.data(), mlen, dom8);
    if (!jac_to_aff(h, g2_mul_bp(c))) continue;
    Q.push_back(h);
    Pa.push_back(a);
  }
  if (ss == PT_OK) {
    aff_t<fp_t> ng;
    ng.x = G1_VGEN_X_M;
    ng.y = G1_VGEN_NEGY_M;
    Q.push_back(S);
    Pa.push_back(ng);
  }
  return verify_pairs((int)Q.size(), Q.data(), Pa.data());
}

// n independent bls_verify calls (32-byte messages) on `threads` host threads:
// the C++ CPU baseline line of bench.py (same arithmetic headers, g++ -O2)
int hc_verify_batch_mt(size_t n, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs, const uint8_t* dom8s,
                       int strict, int threads, uint8_t* verdicts) {
  if (threads < 1) threads = 1;
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([=] {
      for (size_t i = (size_t)t; i < n; i += (size_t)threads)
        verdicts[i] = (uint8_t)hc_verify(pks + 48 * i, msgs32 + 32 * i, 32, sigs + 96 * i, dom8s + 8 * i, strict);
    });
  for (auto& th : pool) th.join();
  return 0;
}

// G1 / G2 scalar multiplication with the same curve code (fixture helpers)
static scalar_t hc_scalar(const uint32_t* k_limbs, int nbits) {
  scalar_t k{};
  for (int i = 0; i < (nbits + 31) / 32 && i < 16; ++i) k.w[i] = k_limbs[i];
  return k;
}
void hc_g1_mul(const uint8_t* aff96, const uint32_t* k_limbs, int nbits, uint8_t* b48) {
  g1_compress(b48, jac_mul_limbs(ldg1(aff96), hc_scalar(k_limbs, nbits), nbits));
}
void hc_g2_mul(const uint8_t* aff192, const uint32_t* k_limbs, int nbits, uint8_t* b96) {
  g2_compress(b96, jac_mul_limbs(ldg2(aff192), hc_scalar(k_limbs, nbits), nbits));
}

// SSZ root program (bls381_ssz.hpp) over one serialized item: 1 ok, 0 malformed program
int hc_ssz_root(const uint8_t* item, const uint32_t* prog, uint32_t plen, uint8_t* out32) {
  static uint32_t stk[SSZ_STACK][8];
  uint32_t r[8];
  if (!ssz_run(r, item, prog, plen, stk)) return 0;
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) out32[4 * w + b] = (uint8_t)(r[w] >> (24 - 8 * b));
  return 1;
}

// verify_merkle_branch (bls381_ssz.hpp merkle_branch_root, the fold k_merkle_branch runs): 1 / 0
int hc_merkle_branch(const uint8_t* leaf32, const uint8_t* proof, uint32_t depth, uint64_t index,
                     const uint8_t* root32) {
  if (depth > 64) return 0;
  uint32_t v[8];
  for (int w = 0; w < 8; ++w)
    v[w] = ((uint32_t)leaf32[4 * w] << 24) | ((uint32_t)leaf32[4 * w + 1] << 16) | ((uint32_t)leaf32[4 * w + 2] << 8) |
           (uint32_t)leaf32[4 * w + 3];
  merkle_branch_root(v, proof, depth, index);
  uint32_t d = 0;
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) d |= (uint32_t)((uint8_t)(v[w] >> (24 - 8 * b)) ^ root32[4 * w + b]);
  return d == 0;
}

// ---- Merkle trees across items (bls381_merkle.hpp, the plan of bls381_plan.hpp): what the
// kernels k_merkle_reduce / k_merkle_finish / k_merkle_proofs run, the workgroups and lanes as
// plain loops, tiles dealt to `threads` host threads.
uint32_t hc_merkle_tile(void) { return MERKLE_TILE; }

namespace {
struct HcTree {
  MerklePlan p;
  std::vector<uint32_t> leaves, nodes, ztab;
  const uint32_t* row(uint32_t h) const { return h == 0 ? leaves.data() : nodes.data() + p.lv[h].off / 4; }
};

// one workgroup of the tile reduction (bls381_kernels.hpp merkle_reduce_tile): tile t of pass ps
// over the row `in`, writing into `nodes`; lv.in(h) is the level read, lv.out(h) the one written
extern "C++" {
struct HcTableLevels {
  const merkle_level* L;
  merkle_level in(uint32_t h) const { return L[h]; }
  merkle_level out(uint32_t h) const { return L[h]; }
};
template <class Lv>
void hc_merkle_tile_run(const uint32_t* in, uint32_t* nodes, const Lv& lv, const uint32_t* ztab, const merkle_pass& ps,
                        uint64_t t) {
  constexpr uint32_t T = MERKLE_TILE / 2;
  static thread_local uint32_t tile[2][8][MERKLE_LDS_ROW];
  uint32_t v[T][8];
  const merkle_level src = lv.in(ps.h0);
  for (uint32_t l = 0; l < T; ++l) {
    const uint64_t j = t * T + l;
    merkle_first_step(v[l], in, src.base, src.count, j, ztab + 8 * ps.h0);
  }
  uint32_t p = 0, live = T;
  for (uint32_t s = 1;; ++s) {
    const merkle_level o = lv.out(ps.h0 + s);
    for (uint32_t l = 0; l < live; ++l)
      merkle_keep(nodes, o.base, o.count, o.off, ((t * T) >> (s - 1)) + l, v[l]);
    if (s == ps.steps) break;
    for (uint32_t l = 0; l < live; ++l)
      for (int w = 0; w < 8; ++w) tile[p][w][merkle_lds_slot(l)] = v[l][w];
    live = T >> s;
    for (uint32_t l = 0; l < live; ++l) {
      uint32_t a[8], b[8];
      for (int w = 0; w < 8; ++w) {
        a[w] = tile[p][w][merkle_lds_slot(2 * l)];
        b[w] = tile[p][w][merkle_lds_slot(2 * l + 1)];
      }
      sha256_pair(v[l], a, b);
    }
    p ^= 1;
  }
}
// the tiles of a pass dealt to `threads` host threads
template <class Lv>
void hc_merkle_pass_run(const uint32_t* in, uint32_t* nodes, const Lv& lv, const uint32_t* ztab, const merkle_pass& ps,
                        int threads) {
  std::vector<std::thread> pool;
  for (int k = 0; k < threads; ++k)
    pool.emplace_back([&, k] {
      for (uint64_t b = (uint64_t)k; b < ps.tiles; b += (uint64_t)threads)
        hc_merkle_tile_run(in, nodes, lv, ztab, ps, ps.tile0 + b);
    });
  for (auto& th : pool) th.join();
}
}  // extern "C++"

// the whole tree: the passes, then k_merkle_finish's fold, mix and root
void hc_merkle_tree(HcTree& tr, const uint8_t* leaves32, int mix, uint64_t length, int threads, uint8_t* root32) {
  const MerklePlan& p = tr.p;
  // exact sizes, so that the sanitized build sees any access outside a row
  tr.leaves.assign(8 * (size_t)p.n, 0);
  if (p.n) std::memcpy(tr.leaves.data(), leaves32, 32 * (size_t)p.n);
  tr.nodes.assign(p.node_bytes / 4, 0xEEEEEEEEu);
  uint8_t z[MERKLE_ZERO_TABLE_BYTES];
  merkle_zero_table(z);
  tr.ztab.assign(MERKLE_ZERO_TABLE_BYTES / 4, 0);
  std::memcpy(tr.ztab.data(), z, sizeof(z));
  if (threads < 1) threads = 1;
  for (const merkle_pass& ps : p.passes)
    hc_merkle_pass_run(tr.row(ps.h0), tr.nodes.data(), HcTableLevels{p.lv}, tr.ztab.data(), ps, threads);
  uint32_t v[8];
  if (p.n) {
    merkle_load(v, tr.row(p.top));
    for (uint32_t g = p.top; g < p.depth; ++g) {
      merkle_fold_step(v, p.first, g, (const uint32_t*)tr.ztab.data());
      merkle_keep(tr.nodes.data(), p.lv[g + 1].base, p.lv[g + 1].count, p.lv[g + 1].off, p.lv[g + 1].base, v);
    }
  } else {
    merkle_load(v, (const uint32_t*)tr.ztab.data() + 8 * p.depth);
  }
  if (mix) merkle_mix_in_length(v, length);
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) root32[4 * w + b] = (uint8_t)(v[w] >> (24 - 8 * b));
}

// k_merkle_proofs: one (index, level) per iteration
void hc_merkle_siblings(const HcTree& tr, size_t n_idx, const uint64_t* indices, uint64_t index_base, uint8_t* proofs,
                        size_t stride) {
  const MerklePlan& p = tr.p;
  for (size_t k = 0; k < n_idx; ++k)
    for (uint32_t h = 0; h < p.depth; ++h) {
      const uint64_t i = indices ? indices[k] : index_base + k;
      const bool kept = h == 0 || p.lv[h].off != MERKLE_NONE;
      const uint32_t* row = kept ? tr.row(h) : tr.nodes.data();
      const uint32_t* src = merkle_node_src(row, p.lv[h].base, kept ? p.lv[h].count : 0, (i >> h) ^ 1,
                                            (const uint32_t*)tr.ztab.data() + 8 * h);
      std::memcpy(proofs + k * stride + 32 * (size_t)h, src, 32);
    }
}
}  // namespace

// bls381_merkle_root: 0, or -2 for arguments the engine rejects
int hc_merkle_root(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, int mix_length, uint64_t length,
                   int threads, uint8_t* root32) {
  if (!merkle_args_in_range(n, first, depth) || !root32 || (n && !leaves32)) return -2;
  HcTree tr;
  tr.p = plan_merkle(n, first, depth, false);
  hc_merkle_tree(tr, leaves32, mix_length, length, threads, root32);
  return 0;
}

// bls381_merkle_proofs: 0, or -2 for arguments the engine rejects
int hc_merkle_proofs(size_t n, const uint8_t* leaves32, uint64_t first, uint32_t depth, size_t n_idx,
                     const uint64_t* indices, uint8_t* proofs, size_t proof_stride, int threads, uint8_t* root32) {
  if (!merkle_args_in_range(n, first, depth) || n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * depth ||
      !root32 || (n && !leaves32) || (n_idx && (!indices || (!proofs && depth))))
    return -2;
  HcTree tr;
  tr.p = plan_merkle(n, first, depth, true);
  hc_merkle_tree(tr, leaves32, 0, 0, threads, root32);
  hc_merkle_siblings(tr, n_idx, indices, 0, proofs, proof_stride);
  return 0;
}

// bls381_deposits_build: the leaves through DEPOSIT_ROOT_PROG, the kept tree, proofs and data
int hc_deposits_build(size_t n, const uint8_t* deposit_data, uint64_t first_index, int threads, uint8_t* deposits,
                      uint8_t* root32) {
  if (!merkle_args_in_range(n, first_index, DEPOSIT_PROOF_DEPTH) || !root32 || (n && (!deposit_data || !deposits)))
    return -2;
  if (threads < 1) threads = 1;
  std::vector<uint8_t> leaves(32 * n + 32);
  std::vector<std::thread> pool;
  for (int k = 0; k < threads; ++k)
    pool.emplace_back([&, k] {
      uint32_t stk[SSZ_STACK][8], r[8];
      for (size_t i = (size_t)k; i < n; i += (size_t)threads) {
        ssz_run(r, deposit_data + DEPOSIT_DATA_BYTES * i, DEPOSIT_ROOT_PROG, DEPOSIT_ROOT_PROG_LEN, stk);
        for (int w = 0; w < 8; ++w)
          for (int b = 0; b < 4; ++b) leaves[32 * i + 4 * w + b] = (uint8_t)(r[w] >> (24 - 8 * b));
      }
    });
  for (auto& th : pool) th.join();
  HcTree tr;
  tr.p = plan_merkle(n, first_index, DEPOSIT_PROOF_DEPTH, true);
  hc_merkle_tree(tr, leaves.data(), 0, 0, threads, root32);
  hc_merkle_siblings(tr, n, nullptr, first_index, deposits, DEPOSIT_BYTES);
  for (size_t i = 0; i < n; ++i)
    std::memcpy(deposits + DEPOSIT_BYTES * i + DEPOSIT_PROOF_BYTES, deposit_data + DEPOSIT_DATA_BYTES * i,
                DEPOSIT_DATA_BYTES);
  return 0;
}

// plan_merkle and the workspace carves on the counting allocator.  levels: 65 x {base, count,
// off}; passes: up to 16 x {h0, steps, tile0, tiles}; out: {pass count, top, node bytes, the
// carve of the level table and the node slice, merkle_node_bound(n, depth)}.  0, or -2 for a
// shape plan_merkle rejects.
int hc_merkle_plan(uint64_t n, uint64_t first, uint32_t depth, int keep, uint64_t* levels, uint64_t* passes,
                   uint64_t* out) {
  if (!merkle_shape_ok(n, first, depth)) return -2;
  const MerklePlan p = plan_merkle(n, first, depth, keep != 0);
  for (uint32_t h = 0; h <= MERKLE_DEPTH_MAX; ++h) {
    levels[3 * h] = p.lv[h].base;
    levels[3 * h + 1] = p.lv[h].count;
    levels[3 * h + 2] = p.lv[h].off;
  }
  if (p.passes.size() > 16) return -2;
  for (size_t k = 0; k < p.passes.size(); ++k) {
    passes[4 * k] = p.passes[k].h0;
    passes[4 * k + 1] = p.passes[k].steps;
    passes[4 * k + 2] = p.passes[k].tile0;
    passes[4 * k + 3] = p.passes[k].tiles;
  }
  out[0] = p.passes.size();
  out[1] = p.top;
  out[2] = p.node_bytes;
  out[3] = merkle_ws_size(n, first, depth, keep != 0);
  out[4] = merkle_node_bound(n, depth);
  return 0;
}

// ---- the deposit tree kept in memory (bls381_deptree.hpp): what k_deptree_append / _roots /
// _chain / _gather run, workgroups and lanes as plain loops.  The store has its exact size, so
// the sanitized build sees any access outside it.
namespace {
struct HcDepTree {
  deptree_shape sh{};
  uint64_t count = 0;
  std::vector<uint32_t> store, ztab;
};
}  // namespace

void* hc_deptree_create(uint64_t capacity, uint32_t depth) {
  if (!deptree_args_ok(capacity, depth)) return nullptr;
  auto* t = new HcDepTree();
  uint64_t bytes = 0;
  t->sh = deptree_make_shape(capacity, depth, &bytes);
  t->store.assign(bytes / 4, 0xEEEEEEEEu);
  uint8_t z[MERKLE_ZERO_TABLE_BYTES];
  merkle_zero_table(z);
  t->ztab.assign(MERKLE_ZERO_TABLE_BYTES / 4, 0);
  std::memcpy(t->ztab.data(), z, sizeof(z));
  return t;
}
void hc_deptree_destroy(void* tree) { delete (HcDepTree*)tree; }
uint64_t hc_deptree_count(const void* tree) { return tree ? ((const HcDepTree*)tree)->count : 0; }

// bls381_deposit_tree_append: 0, or -2 for arguments the engine rejects
int hc_deptree_append(void* tree, size_t n, const uint8_t* leaves32, int threads) {
  HcDepTree* t = (HcDepTree*)tree;
  if (!t || n > t->sh.capacity - t->count || (n && !leaves32)) return -2;
  if (n == 0) return 0;
  if (threads < 1) threads = 1;
  std::memcpy(t->store.data() + 8 * t->count, leaves32, 32 * n);
  const deptree_levels lv{t->sh, t->count, t->count + n};
  for (const merkle_pass& ps : deptree_append_plan(t->sh, t->count, n))
    hc_merkle_pass_run(t->store.data() + t->sh.off[ps.h0] / 4, t->store.data(), lv, t->ztab.data(), ps, threads);
  t->count += n;
  return 0;
}

// bls381_deposit_tree_roots (k_deptree_roots, one count per iteration): 0 or -2
int hc_deptree_roots(void* tree, size_t m, const uint64_t* counts, uint8_t* roots32) {
  HcDepTree* t = (HcDepTree*)tree;
  if (!t || (m && (!counts || !roots32))) return -2;
  for (size_t q = 0; q < m; ++q)
    if (counts[q] > t->count) return -2;
  for (size_t q = 0; q < m; ++q) {
    uint32_t v[8];
    merkle_load(v, (const uint32_t*)t->ztab.data());
    for (uint32_t h = 0; h < t->sh.depth; ++h)
      deptree_chain_step(v, t->sh, (const uint32_t*)t->store.data(), counts[q], h, (const uint32_t*)t->ztab.data());
    uint32_t out[8];
    merkle_store(out, v);
    std::memcpy(roots32 + 32 * q, out, 32);
  }
  return 0;
}

// bls381_deposit_tree_proofs (k_deptree_chain, then k_deptree_gather): 0 or -2
int hc_deptree_proofs(void* tree, uint64_t k, size_t n_idx, const uint64_t* indices, uint8_t* proofs,
                      size_t proof_stride, uint8_t* root32) {
  HcDepTree* t = (HcDepTree*)tree;
  if (!t || k > t->count || n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * t->sh.depth || !root32 ||
      (n_idx && (!indices || !proofs)))
    return -2;
  const uint32_t* store = t->store.data();
  const uint32_t* ztab = t->ztab.data();
  std::vector<uint32_t> ptab(8 * (size_t)(t->sh.depth + 1));
  uint32_t v[8];
  merkle_load(v, ztab);
  for (uint32_t h = 0;; ++h) {
    merkle_store(ptab.data() + 8 * h, v);
    if (h == t->sh.depth) break;
    deptree_chain_step(v, t->sh, store, k, h, ztab);
  }
  std::memcpy(root32, ptab.data() + 8 * t->sh.depth, 32);
  for (size_t q = 0; q < n_idx; ++q)
    for (uint32_t h = 0; h < t->sh.depth; ++h)
      std::memcpy(proofs + q * proof_stride + 32 * (size_t)h,
                  deptree_sibling_src(t->sh, store, k, indices[q], h, (const uint32_t*)ptab.data(), ztab), 32);
  return 0;
}

// deptree_append_plan for a tree of `capacity` (depth 32) at `count`: out = {pass count, then
// {h0, steps, tile0, tiles} per pass, up to 8 passes}.  0, or -2 for a rejected shape or append.
int hc_deptree_plan(uint64_t capacity, uint64_t count, uint64_t n, uint64_t* out) {
  if (!deptree_args_ok(capacity, DEPTREE_DEPTH_MAX) || count > capacity || n > capacity - count) return -2;
  uint64_t bytes = 0;
  const deptree_shape sh = deptree_make_shape(capacity, DEPTREE_DEPTH_MAX, &bytes);
  const std::vector<merkle_pass> passes = deptree_append_plan(sh, count, n);
  if (passes.size() > 8) return -2;
  out[0] = passes.size();
  for (size_t k = 0; k < passes.size(); ++k) {
    out[1 + 4 * k] = passes[k].h0;
    out[2 + 4 * k] = passes[k].steps;
    out[3 + 4 * k] = passes[k].tile0;
    out[4 + 4 * k] = passes[k].tiles;
  }
  return 0;
}

// ---- SSZ list trees kept in memory (bls381_listtree.hpp): what k_listtree_scatter / _mark /
// _leaves / _compact / _reduce / _proofs run, workgroups and lanes as plain loops -- the flag
// rows, the compaction and the tile lists included.  The store and the update's workspace have
// their exact sizes, so the sanitized build sees any access outside them.
namespace {
struct HcListTree {
  listtree_shape sh{};
  uint64_t count = 0;
  std::vector<uint32_t> store, ztab, prog;
  uint8_t* bytes() { return (uint8_t*)store.data(); }
  uint64_t chunks() const { return listtree_chunks(sh, count); }
  uint32_t depth() const { return merkle_chunk_depth(chunks()); }
};

// k_listtree_reduce over a pass's workgroups: tile list[b] for b below the list's length (a
// workgroup at or above it returns), or tile0 + b without a list
void hc_listtree_pass(HcListTree* t, const listtree_levels& lv, const merkle_pass& ps, const uint32_t* list,
                      const uint32_t* list_len, int threads) {
  if (threads < 1) threads = 1;
  std::vector<std::thread> pool;
  for (int k = 0; k < threads; ++k)
    pool.emplace_back([&, k] {
      for (uint64_t b = (uint64_t)k; b < ps.tiles; b += (uint64_t)threads) {
        if (list && b >= *list_len) continue;
        hc_merkle_tile_run(t->store.data() + t->sh.off[ps.h0] / 4, t->store.data(), lv, t->ztab.data(), ps,
                           list ? list[b] : ps.tile0 + b);
      }
    });
  for (auto& th : pool) th.join();
}

// k_listtree_mark and k_listtree_compact of an update: the workspace's flag rows, tile lists and lengths
void hc_listtree_dirty(const HcListTree* t, size_t n_upd, const uint32_t* indices, const listtree_marks& m,
                       std::vector<uint32_t>& ws) {
  for (size_t u = 0; u < n_upd; ++u) listtree_mark(t->sh, t->count, m, indices, u, ws.data());
  for (uint32_t k = 0; k < m.passes; ++k) {
    uint32_t cnt[LISTTREE_COMPACT_LANES], lo, hi;
    const uint32_t* flags = ws.data() + m.flags[k];
    for (uint32_t l = 0; l < LISTTREE_COMPACT_LANES; ++l) {
      listtree_segment(m.tiles[k], l, &lo, &hi);
      cnt[l] = listtree_segment_count(flags, lo, hi);
    }
    uint32_t before = 0;
    for (uint32_t l = 0; l < LISTTREE_COMPACT_LANES; ++l) {
      listtree_segment(m.tiles[k], l, &lo, &hi);
      listtree_segment_write(flags, lo, hi, ws.data() + m.list[k] + before);
      before += cnt[l];
    }
    ws[m.lens + k] = before;
  }
}
}  // namespace

// bls381_list_tree_create: the tree, or null for arguments the engine rejects
void* hc_listtree_create(uint64_t capacity, uint64_t item_size, const uint32_t* prog, uint32_t plen) {
  const bool packed = !prog && plen == 0;
  if (!listtree_args_ok(capacity, item_size, packed) || (!packed && !ssz_prog_ok(prog, plen, item_size))) return nullptr;
  auto* t = new HcListTree();
  uint64_t bytes = 0;
  t->sh = listtree_make_shape(capacity, (uint32_t)item_size, packed, &bytes);
  t->store.assign(bytes / 4, 0);
  if (!packed) t->prog.assign(prog, prog + plen);
  uint8_t z[MERKLE_ZERO_TABLE_BYTES];
  merkle_zero_table(z);
  t->ztab.assign(MERKLE_ZERO_TABLE_BYTES / 4, 0);
  std::memcpy(t->ztab.data(), z, sizeof(z));
  return t;
}
void hc_listtree_destroy(void* tree) { delete (HcListTree*)tree; }
uint64_t hc_listtree_count(const void* tree) { return tree ? ((const HcListTree*)tree)->count : 0; }
uint32_t hc_listtree_depth(const void* tree) { return tree ? ((const HcListTree*)tree)->depth() : 0; }

// bls381_list_tree_append: 0, or -2 for arguments the engine rejects
int hc_listtree_append(void* tree, size_t n, const uint8_t* items, int threads) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || n > t->sh.capacity - t->count || (n && !items)) return -2;
  if (n == 0) return 0;
  const listtree_shape& sh = t->sh;
  std::memcpy(t->bytes() + t->count * sh.item_size, items, n * sh.item_size);
  const uint64_t c0 = listtree_chunk_of(sh, t->count), c1 = listtree_chunks(sh, t->count + n);
  if (!sh.packed) {
    static thread_local uint32_t stk[SSZ_STACK][8];
    for (uint64_t i = t->count; i < t->count + n; ++i) {
      uint32_t r[8];
      if (!ssz_run(r, t->bytes() + i * sh.item_size, t->prog.data(), (uint32_t)t->prog.size(), stk)) return -1;
      merkle_store(t->store.data() + sh.off[0] / 4 + 8 * i, r);
    }
  }
  const listtree_levels lv{sh, c1};
  for (const merkle_pass& ps : listtree_range_plan(sh, c0, c1)) hc_listtree_pass(t, lv, ps, nullptr, nullptr, threads);
  t->count += n;
  return 0;
}

// bls381_list_tree_update (device_form = 0: an index at or above the count is rejected, repeated
// indices dropped but for the last) or bls381_list_tree_update_device (1: such an index is
// skipped, repeated ones all run): 0, or -2 for arguments the engine rejects
int hc_listtree_update(void* tree, size_t n_upd, const uint32_t* indices, size_t off, size_t len, const uint8_t* values,
                       int device_form, int threads) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || n_upd > (size_t)INT32_MAX || off > t->sh.item_size || len > t->sh.item_size - off) return -2;
  if (n_upd == 0 || len == 0) return 0;
  if (!indices || !values) return -2;
  std::vector<uint32_t> idx(indices, indices + n_upd);
  std::vector<uint8_t> vals(values, values + n_upd * len);
  if (!device_form) {
    for (size_t u = 0; u < n_upd; ++u)
      if (indices[u] >= t->count) return -2;
    std::map<uint32_t, size_t> last;
    for (size_t u = 0; u < n_upd; ++u) last[indices[u]] = u;
    idx.clear();
    vals.clear();
    for (size_t u = 0; u < n_upd; ++u)
      if (last[indices[u]] == u) {
        idx.push_back(indices[u]);
        vals.insert(vals.end(), values + u * len, values + (u + 1) * len);
      }
    n_upd = idx.size();
  }
  if (t->count == 0) return 0;
  const listtree_shape& sh = t->sh;
  for (size_t g = 0; g < n_upd * len; ++g)
    listtree_scatter_byte(sh, t->count, idx.data(), vals.data(), (uint32_t)off, (uint32_t)len, g / len, (uint32_t)(g % len),
                          t->bytes());
  if (!sh.packed) {
    static thread_local uint32_t stk[SSZ_STACK][8];
    for (size_t u = 0; u < n_upd; ++u) {
      const uint64_t i = idx[u];
      if (i >= t->count) continue;
      uint32_t r[8];
      if (!ssz_run(r, t->bytes() + i * sh.item_size, t->prog.data(), (uint32_t)t->prog.size(), stk)) return -1;
      merkle_store(t->store.data() + sh.off[0] / 4 + 8 * i, r);
    }
  }
  const listtree_update_ws w = listtree_update_layout(sh, n_upd);
  if (w.passes == 0) return 0;
  const listtree_marks m = listtree_make_marks(w, t->chunks());
  std::vector<uint32_t> ws(w.words, 0xEEEEEEEEu);
  std::fill(ws.begin(), ws.begin() + w.flag_words, 0);
  hc_listtree_dirty(t, n_upd, idx.data(), m, ws);
  const listtree_levels lv{sh, t->chunks()};
  for (uint32_t k = 0; k < w.passes; ++k) {
    const uint32_t h0 = k * MERKLE_TILE_LOG;
    const merkle_pass ps{h0, std::min(MERKLE_TILE_LOG, sh.top - h0), 0, std::min<uint64_t>(n_upd, m.tiles[k])};
    hc_listtree_pass(t, lv, ps, ws.data() + m.list[k], ws.data() + m.lens + k, threads);
  }
  return 0;
}

// bls381_list_tree_root (k_merkle_finish with nothing left to fold): 0 or -2
int hc_listtree_root(void* tree, int mix_length, uint8_t* root32) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || !root32) return -2;
  uint32_t v[8];
  merkle_load(v, t->count ? (const uint32_t*)t->store.data() + t->sh.off[t->depth()] / 4 : (const uint32_t*)t->ztab.data());
  if (mix_length) merkle_mix_in_length(v, t->count);
  uint32_t out[8];
  merkle_store(out, v);
  std::memcpy(root32, out, 32);
  return 0;
}

// bls381_list_tree_proofs (the root, then k_listtree_proofs one (index, level) per iteration): 0 or -2
int hc_listtree_proofs(void* tree, size_t n_idx, const uint64_t* chunk_indices, uint8_t* proofs, size_t proof_stride,
                       uint8_t* root32) {
  HcListTree* t = (HcListTree*)tree;
  if (!t) return -2;
  const uint32_t d = t->depth();
  if (n_idx > (size_t)INT32_MAX || proof_stride < (size_t)32 * d || !root32 || (n_idx && (!chunk_indices || (!proofs && d))))
    return -2;
  hc_listtree_root(tree, 0, root32);
  for (size_t q = 0; q < n_idx; ++q)
    for (uint32_t h = 0; h < d; ++h)
      std::memcpy(proofs + q * proof_stride + 32 * (size_t)h,
                  listtree_sibling_src(t->sh, (const uint32_t*)t->store.data(), t->chunks(), chunk_indices[q], h,
                                       (const uint32_t*)t->ztab.data()),
                  32);
  return 0;
}

// bls381_list_tree_read: 0 or -2
int hc_listtree_read(void* tree, size_t first, size_t n, uint8_t* items_out) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || first > t->count || n > t->count - first || (n && !items_out)) return -2;
  std::memcpy(items_out, t->bytes() + first * t->sh.item_size, n * t->sh.item_size);
  return 0;
}
// the item bytes of the whole capacity, behind the count included (they must read as zero there)
int hc_listtree_read_capacity(void* tree, uint8_t* items_out) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || !items_out) return -2;
  std::memcpy(items_out, t->bytes(), t->sh.capacity * t->sh.item_size);
  return 0;
}

// The plan of an update of the given indices at the tree's current count, the tree unchanged:
// out = {launches, passes, then per pass {h0, steps, workgroups launched, list length, the
// list's tiles ...}}, at most out_cap words.  0, or -2 for a rejected call or a short `out`.
int hc_listtree_plan(void* tree, size_t n_upd, const uint32_t* indices, uint64_t* out, size_t out_cap) {
  HcListTree* t = (HcListTree*)tree;
  if (!t || n_upd == 0 || n_upd > (size_t)INT32_MAX || !indices || !out || out_cap < 2) return -2;
  const listtree_update_ws w = listtree_update_layout(t->sh, n_upd);
  const listtree_marks m = listtree_make_marks(w, t->chunks());
  std::vector<uint32_t> ws(w.words, 0xEEEEEEEEu);
  std::fill(ws.begin(), ws.begin() + w.flag_words, 0);
  if (w.passes) hc_listtree_dirty(t, n_upd, indices, m, ws);
  size_t at = 0;
  out[at++] = listtree_update_launches(t->sh);
  out[at++] = w.passes;
  for (uint32_t k = 0; k < w.passes; ++k) {
    const uint32_t h0 = k * MERKLE_TILE_LOG, len = ws[m.lens + k];
    if (at + 4 + len > out_cap) return -2;
    out[at++] = h0;
    out[at++] = std::min(MERKLE_TILE_LOG, t->sh.top - h0);
    out[at++] = std::min<uint64_t>(n_upd, m.tiles[k]);
    out[at++] = len;
    for (uint32_t q = 0; q < len; ++q) out[at++] = ws[m.list[k] + q];
  }
  return 0;
}

// the pubkey tables' hash (bls381_keytable.hpp) and slot counts (bls381_plan.hpp), as the engine computes them
uint32_t hc_reg_hash(const uint8_t* key48) { return reg_hash(key48); }
size_t hc_registry_table_slots(size_t capacity) { return registry_table_slots(capacity); }
size_t hc_deposit_table_slots(size_t n) { return deposit_table_slots(n); }

// get_shuffled_index (bls381_shuffle.hpp: the direct form, every position hashing its own source
// block): the shuffled index, or UINT64_MAX for arguments the engine rejects
uint64_t hc_shuffled_index(uint64_t index, uint64_t index_count, const uint8_t* seed32, uint32_t rounds) {
  if (index_count > 0xFFFFFFFFull || index >= index_count || rounds > SHUFFLE_ROUNDS_MAX) return UINT64_MAX;
  const shuffle_seed sd = shuffle_seed_from_bytes(seed32);
  const uint32_t n = (uint32_t)index_count;
  uint32_t pivots[SHUFFLE_ROUNDS_MAX + 1];
  for (uint32_t r = 0; r < rounds; ++r) pivots[r] = shuffle_pivot(sd, r, n);
  return shuffle_walk((uint32_t)index, n, rounds, pivots, shuffle_direct_bit{sd});
}

// Positions first .. first+count-1 of the shuffled list on `threads` host threads, through the
// table form (table 1: shuffle_source_words per (round, block), then one bit per round) or the
// direct form (table 0): the measurement base of tools/shuffle_bench.py and the table form's CPU
// check.  0, or -1 for arguments the engine rejects.
int hc_shuffle_list(uint64_t index_count, const uint8_t* seed32, uint32_t rounds, uint64_t first, uint64_t count,
                    int table, int threads, uint32_t* out) {
  if (index_count > 0xFFFFFFFFull || first > index_count || count > index_count - first ||
      rounds > SHUFFLE_ROUNDS_MAX || threads < 1)
    return -1;
  if (count == 0) return 0;
  const shuffle_seed sd = shuffle_seed_from_bytes(seed32);
  const uint32_t n = (uint32_t)index_count;
  const size_t blocks = shuffle_blocks(n);
  std::vector<uint32_t> pivots(SHUFFLE_ROUNDS_MAX + 1), tab(table ? (size_t)rounds * blocks * 8 : 0);
  for (uint32_t r = 0; r < rounds; ++r) pivots[r] = shuffle_pivot(sd, r, n);
  auto run = [&](auto body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([=] { body((size_t)t); });
    for (auto& th : pool) th.join();
  };
  if (table)
    run([&](size_t t) {
      for (size_t k = t; k < (size_t)rounds * blocks; k += (size_t)threads)
        shuffle_source_words(&tab[8 * k], sd, (uint32_t)(k / blocks), (uint32_t)(k % blocks));
    });
  run([&](size_t t) {
    for (uint64_t k = t; k < count; k += (uint64_t)threads) {
      const uint32_t i = (uint32_t)(first + k);
      out[k] = table ? shuffle_walk(i, n, rounds, pivots.data(), shuffle_table_bit<const uint32_t*>{tab.data(), 8 * blocks})
                     : shuffle_walk(i, n, rounds, pivots.data(), shuffle_direct_bit{sd});
    }
  });
  return 0;
}

// verify_bitfield (bls381_shuffle.hpp bitfield_ok): 1 / 0
int hc_verify_bitfield(const uint8_t* bits, size_t nbytes, uint32_t committee_size) {
  return bitfield_ok(bits, nbytes, committee_size);
}

// convert_to_indexed's two sets for one attestation (attesting_group, the code of
// k_attesting_entries, run by one thread): out0 / out1 receive the sorted custody-bit-0 /
// custody-bit-1 members (room for committee_len each), n_out their counts.  1, or 0 when a
// bitfield fails verify_bitfield (both sets are then empty) or the committee exceeds 4,096.
int hc_attesting_groups(const uint32_t* committee, uint32_t committee_len, const uint8_t* agg, const uint8_t* cust,
                        size_t nbytes, uint32_t* out0, uint32_t* out1, uint32_t* n_out) {
  n_out[0] = n_out[1] = 0;
  if (committee_len > ATT_MAX_COMMITTEE || !bitfield_ok(agg, nbytes, committee_len) ||
      !bitfield_ok(cust, nbytes, committee_len))
    return 0;
  attesting_counts(agg, cust, nbytes, &n_out[0], &n_out[1]);
  std::vector<uint32_t> buf(ATT_MAX_COMMITTEE), cnt(ATT_MASK_WORDS);
  const auto no_sync = [] {};
  if (n_out[0]) attesting_group(buf.data(), cnt.data(), 0u, 1u, no_sync, committee, committee_len, agg, cust, 0, n_out[0], out0);
  if (n_out[1]) attesting_group(buf.data(), cnt.data(), 0u, 1u, no_sync, committee, committee_len, agg, cust, 1, n_out[1], out1);
  return 1;
}

// ---- epoch context (bls381_epoch.hpp): the three phases of the active-index compaction in the
// kernels' own tile geometry, the packed index chunks and one slot's proposer search
// get_active_validator_indices over fields at base + i * stride, on `threads` host threads:
// indices_out (room for n), out2[0] = count, out2[1] = the active balance sum (0 without
// balances).  0, or -1 for arguments the engine rejects.
int hc_active_indices(uint64_t n, const uint8_t* activation, const uint8_t* exit_, size_t stride, uint64_t epoch,
                      const uint8_t* balance, size_t balance_stride, int threads, uint32_t* indices_out, uint64_t* out2) {
  if (n > 0xFFFFFFFFull || stride < 8 || (balance && balance_stride < 8) || threads < 1) return -1;
  out2[0] = out2[1] = 0;
  if (n == 0) return 0;
  const u64_field act = make_u64_field(activation, stride), ext = make_u64_field(exit_, stride);
  const u64_field bal = balance ? make_u64_field(balance, balance_stride) : act;
  const size_t tiles = active_tiles(n);
  std::vector<uint64_t> ballots(tiles * ACTIVE_TILE_BALLOTS), tile_balance(tiles);
  std::vector<uint32_t> tile_count(tiles), tile_offset(tiles);
  auto run = [&](auto body) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back([=] { body((size_t)t); });
    for (auto& th : pool) th.join();
  };
  run([&](size_t t) {   // k_active_count
    for (size_t tile = t; tile < tiles; tile += (size_t)threads) {
      uint32_t count = 0;
      uint64_t sum = 0;
      for (uint32_t k = 0; k < ACTIVE_ROUNDS; ++k)
        for (uint32_t wave = 0; wave < EPOCH_BLOCK / 64; ++wave) {
          uint64_t m = 0;
          for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t i = active_item(tile, k, 64 * wave + lane);
            if (i < n && validator_active(act, ext, epoch, (size_t)i)) {
              m |= (uint64_t)1 << lane;
              if (balance) sum += field_load(bal, (size_t)i);
            }
          }
          ballots[tile * ACTIVE_TILE_BALLOTS + 4 * k + wave] = m;
          count += (uint32_t)__builtin_popcountll(m);
        }
      tile_count[tile] = count;
      tile_balance[tile] = sum;
    }
  });
  uint64_t carry = 0, total = 0;   // k_active_scan
  for (size_t j = 0; j < tiles; ++j) {
    tile_offset[j] = (uint32_t)carry;
    carry += tile_count[j];
    total += tile_balance[j];
  }
  out2[0] = carry;
  out2[1] = total;
  run([&](size_t t) {   // k_active_scatter
    for (size_t tile = t; tile < tiles; tile += (size_t)threads) {
      uint32_t before = 0;
      for (uint32_t b = 0; b < ACTIVE_TILE_BALLOTS; ++b) {
        const uint64_t m = ballots[tile * ACTIVE_TILE_BALLOTS + b];
        for (uint32_t lane = 0; lane < 64; ++lane)
          if ((m >> lane) & 1u)
            indices_out[tile_offset[tile] + before + ballot_before(m, lane)] =
                (uint32_t)active_item(tile, b / 4, 64 * (b % 4) + lane);
        before += (uint32_t)__builtin_popcountll(m);
      }
    }
  });
  return 0;
}

// the packed chunks of List[uint64] over n uint32 indices: 4 * ceil(n / 4) words to chunks_out
void hc_index_chunks(uint64_t n, const uint32_t* indices, uint64_t* chunks_out) {
  for (size_t t = 0; t < 4 * index_chunk_count(n); ++t) chunks_out[t] = index_chunk_word(indices, (size_t)n, t);
}

// SHA-256(seed || u64le(q)) as 32 bytes (proposer_digest)
void hc_proposer_digest(const uint8_t* seed32, uint64_t q, uint8_t* out32) {
  uint32_t d[8];
  proposer_digest(d, shuffle_seed_from_bytes(seed32), q);
  for (uint32_t j = 0; j < 32; ++j) out32[j] = (uint8_t)proposer_digest_byte(d, j);
}

// get_beacon_proposer_index over one committee, try by try up to max_tries (the engine's cap is
// PROPOSER_MAX_TRIES): the proposer, or 0xFFFFFFFF at the cap, for an out-of-range candidate or
// for arguments the engine rejects; *tries_out = the try that ended the search (max_tries at the cap).
uint32_t hc_proposer_index(const uint32_t* committee, uint32_t committee_len, uint64_t epoch, const uint8_t* balance,
                           size_t balance_stride, uint64_t n_validators, const uint8_t* seed32,
                           uint64_t max_effective_balance, uint32_t max_tries, uint32_t* tries_out) {
  *tries_out = 0;
  if (committee_len == 0 || balance_stride < 8 || max_effective_balance == 0 ||
      max_effective_balance >= PROPOSER_BALANCE_LIMIT || max_tries > PROPOSER_MAX_TRIES)
    return PROPOSER_NONE;
  const shuffle_seed sd = shuffle_seed_from_bytes(seed32);
  const u64_field bal = make_u64_field(balance, balance_stride);
  const proposer_slot sl{0, committee_len, (uint32_t)(epoch % committee_len)};
  uint32_t d[8];
  for (uint32_t i = 0; i < max_tries; ++i) {
    if (i % 32 == 0) proposer_digest(d, sd, i / 32);
    uint32_t candidate;
    const int v = proposer_try(committee, sl, i, proposer_digest_byte(d, i % 32), bal, n_validators,
                               max_effective_balance, &candidate);
    *tries_out = i;
    if (v != PROPOSER_REJECT) return v == PROPOSER_ACCEPT ? candidate : PROPOSER_NONE;
  }
  *tries_out = max_tries;
  return PROPOSER_NONE;
}

#if defined(BLS_COUNT_OPS)
// Per-stage MAC counts (BLS_COUNT_MACS: partial products of the Fp products, 392 per
// fp_mul) of one bls_verify exactly as the gfx950
// kernels of bls381_capi.hip stage it (decode_g1 [+ subgroup check when strict],
// decode_g2 [+ subgroup check], hash_to_g2, miller_loop_2, final_exp).  out[5]
// receives the counts.
int hc_count_verify_stages(const uint8_t* pk48, const uint8_t* msg32, const uint8_t* sig96, const uint8_t* dom8,
                           int strict, uint64_t* out) {
  aff_t<fp_t> P;
  aff_t<fp2_t> S, H;
  g_fp_macs = 0;
  int sp = g1_decompress(P, pk48, !strict);
  if (strict && sp == PT_OK && !g1_in_subgroup(P)) sp = PT_BAD;
  out[0] = g_fp_macs;
  g_fp_macs = 0;
  int ss = g2_decompress(S, sig96, !strict);
  if (strict && ss == PT_OK && !g2_in_subgroup(S)) ss = PT_BAD;
  out[1] = g_fp_macs;
  g_fp_macs = 0;
  aff_t<fp2_t> c;
  hash_to_g2_candidate(c, msg32, 32, dom8);
  jac_to_aff(H, g2_mul_bp(c));
  out[2] = g_fp_macs;
  if (sp != PT_OK || ss != PT_OK) { out[3] = out[4] = 0; return -1; }
  g_fp_macs = 0;
  aff_t<fp2_t> Q[2] = {S, H};
  aff_t<fp_t> ng; ng.x = G1_VGEN_X_M; ng.y = G1_VGEN_NEGY_M;
  g1_line_pre Pp[2] = {g1_prepare(ng), g1_prepare(P)};
  bool degen = false;
  const fp12_t f = miller_loop_n<2>(Q, Pp, degen);
  out[3] = g_fp_macs;
  g_fp_macs = 0;
  const bool ok = final_exp_check<fp2_t, 1>(f) == 1;   // the kernel's verdict form (one product fewer)
  out[4] = g_fp_macs;
  // the split Miller loop of the throughput path, per kernel (bls381_kernels.hpp):
  // out[5] k_ml_lines (both running points, L = l l'), out[6] k_ml_accum (f^2 L)
  uint64_t lines = 0, accum = 0;
  g2_proj<fp2_t> T[2];
  for (int k = 0; k < 2; ++k) { T[k].x = Q[k].x; T[k].y = Q[k].y; T[k].z = fp2_one(); }
  fp12_t g;
  int step = 0;
  auto run_step = [&](bool add) {
    fp2_t c[3], d[3];
    g_fp_macs = 0;
    if (add) { line_add(T[0], Q[0], Pp[0], c[0], c[1], c[2]); line_add(T[1], Q[1], Pp[1], d[0], d[1], d[2]); }
    else { line_dbl(T[0], Pp[0], c[0], c[1], c[2]); line_dbl(T[1], Pp[1], d[0], d[1], d[2]); }
    const fp12_t L = line_pair_product(c[0], c[1], c[2], d[0], d[1], d[2]);
    lines += g_fp_macs;
    g_fp_macs = 0;
    if (step == 0) g = L;
    else if (add || step == 1) g = fp12_mul_by_line_pair_inl(g, L);
    else g = fp12_mul_by_line_pair_inl(fp12_sqr_inl(g), L);
    accum += g_fp_macs;
    ++step;
  };
  for (int b = 62; b >= 0; --b) {
    run_step(false);
    if ((BLS_X_ABS >> b) & 1) run_step(true);
  }
  out[5] = lines;
  out[6] = accum;
  return ok ? 1 : 0;
}

// MACs of the randomized path's per-item and per-sub-batch stages (bench.py rb roofline):
// out[0] [r] pk = sigma(pk) + the joint 32-bit ladder + affine (k_rb_decode_g1's scalar part),
// out[1] the signature's G2 test (k_rb_g2_test), out[2] one mixed G2 addition (the MSM's unit:
// ~15 per item at 4-bit windows), out[3] the joint 32-bit G2 ladder [r] sig (k_rb_scale_g2, the
// path above the MSM's sub-batch cap), out[4] one Miller pair (S, -[c] g1) (k_rb_miller_sig).
int hc_count_rb_item(const uint8_t* pk48, const uint8_t* sig96, uint32_t k0, uint32_t k1, uint64_t* out) {
  aff_t<fp_t> P;
  aff_t<fp2_t> S;
  if (g1_decompress(P, pk48, true) != PT_OK || g2_decompress(S, sig96, true) != PT_OK) return -1;
  g_fp_macs = 0;
  aff_t<fp_t> sp;
  sp.x = fp_mul(G1_BETA_M, P.x);
  sp.y = P.y;
  aff_t<fp_t> r1;
  jac_to_aff(r1, jac_mul_2x32(P, sp, k0, k1));
  out[0] = g_fp_macs;
  g_fp_macs = 0;
  (void)g2_in_subgroup(S);
  out[1] = g_fp_macs;
  g_fp_macs = 0;
  const jac_t<fp2_t> j = jac_mul_2x32(S, g2_psi(S), 3u, 5u);   // a generic Jacobian point
  g_fp_macs = 0;
  (void)jac_add_aff(j, S);
  out[2] = g_fp_macs;
  aff_t<fp2_t> sq = g2_psi(g2_psi(S));
  sq.y = fp2_neg(sq.y);
  g_fp_macs = 0;
  (void)jac_mul_2x32(S, sq, k0, k1);
  out[3] = g_fp_macs;
  aff_t<fp_t> ng; ng.x = G1_VGEN_X_M; ng.y = G1_VGEN_NEGY_M;
  const g1_line_pre pre = g1_prepare(ng);
  bool degen = false;
  g_fp_macs = 0;
  (void)miller_loop_n<1>(&S, &pre, degen);
  out[4] = g_fp_macs;
  return 0;
}

// MACs (BLS_COUNT_MACS) of one committee aggregation of n pubkeys (decode + adds)
int hc_count_aggregate(size_t n, const uint8_t* pks, uint64_t* out) {
  g_fp_macs = 0;
  jac_t<fp_t> acc = jac_infinity<fp_t>();
  for (size_t i = 0; i < n; ++i) {
    aff_t<fp_t> a;
    const int s = g1_decompress(a, pks + 48 * i, true);
    if (s == PT_BAD) return -1;
    if (s == PT_OK) acc = jac_add_aff(acc, a);
  }
  uint8_t b[48];
  g1_compress(b, acc);
  *out = g_fp_macs;
  return 0;
}
#endif

// ---- host planners (bls381_plan.hpp), as flat arrays.  A writer returns the u32 words it
// wrote, or -1 when `cap` words do not hold them.  A chunk-list sequence (product passes,
// aggregation levels) is written as: count, then per list its length and begin/end pairs.
}  // extern "C"
namespace {
struct Words {
  uint32_t* out;
  size_t cap, n = 0;
  bool ok = true;
  void put(uint64_t v) {
    if (n < cap) out[n++] = (uint32_t)v; else ok = false;
  }
  template <class T> void vec(const std::vector<T>& v) {
    put(v.size());
    for (const T& x : v) put((uint32_t)x);
  }
  void lists(const std::vector<std::vector<agg_chunk>>& ls) {
    put(ls.size());
    for (const auto& l : ls) {
      put(l.size());
      for (const agg_chunk& c : l) { put(c.begin); put(c.end); }
    }
  }
  long done() const { return ok ? (long)n : -1; }
};
// scalars (n_calls, n_keys, G, nquads, tasks, nslots, vm_ws_bound lo / hi), then every array of
// the plan in declaration order, then the aggregation levels
long dump_vm_plan(const VmPlan& pl, size_t mlen, uint32_t* out, size_t cap) {
  Words w{out, cap};
  const uint64_t bound = vm_ws_bound(pl, mlen);
  for (uint64_t v : {(uint64_t)pl.n_calls, (uint64_t)pl.n_keys, (uint64_t)pl.G, (uint64_t)pl.nquads, (uint64_t)pl.tasks,
                     (uint64_t)pl.nslots, bound & 0xffffffffu, bound >> 32})
    w.put(v);
  w.vec(pl.key_idx); w.vec(pl.group_off); w.vec(pl.group_msg); w.vec(pl.group_call); w.vec(pl.quad_pair);
  w.vec(pl.call_quad_off); w.lists(pl.passes); w.lists(pl.task_passes); w.vec(pl.quad_slot); w.vec(pl.sig_slot);
  w.vec(pl.sig_task); w.lists(pl.agg.levels);
  return w.done();
}
}  // namespace
extern "C" {

long hc_plan_products(size_t nseg, const uint32_t* off, uint32_t* out, size_t cap) {
  Words w{out, cap};
  w.lists(plan_products(std::vector<uint32_t>(off, off + nseg + 1)));
  return w.done();
}

// sizes[0] = agg_ws_size of the plan for points of ncomp Fp components, sizes[1] = the public G1
// bound (3 components) for the same counts
long hc_plan_agg(size_t ng, const uint32_t* offsets, int lanes_per_point, int ncomp, uint32_t* out, size_t cap,
                 size_t sizes[2]) {
  const AggPlan p = plan_agg(ng, offsets, lanes_per_point);
  sizes[0] = agg_ws_size(p, ncomp);
  sizes[1] = agg_ws_bound_sizes(ng, ng ? offsets[ng] - offsets[0] : 0);
  Words w{out, cap};
  w.lists(p.levels);
  return w.done();
}

long hc_plan_vm(size_t n_calls, const uint32_t* call_off, const uint8_t* msgs, size_t mlen, const uint8_t* h_pks,
                const uint8_t* h_sigs, const int* with_sig, uint32_t* out, size_t cap) {
  return dump_vm_plan(plan_vm(n_calls, call_off, msgs, mlen, h_pks, h_sigs, with_sig), mlen, out, cap);
}

long hc_plan_vm_grouped(size_t n_calls, const uint32_t* call_group_off, const uint32_t* group_key_off,
                        const uint8_t* msgs, size_t mlen, uint32_t* out, size_t cap) {
  return dump_vm_plan(plan_vm_grouped(n_calls, call_group_off, group_key_off, msgs, mlen), mlen, out, cap);
}

// out[0] = the verify_multiple bound from sizes alone; out[1] = verify_ws_size(n_verify), out[2] =
// the bytes carve_verify consumes for the same n
void hc_vm_ws_bounds(size_t n_calls, size_t n_keys, size_t mlen, size_t n_verify, size_t out[3]) {
  out[0] = vm_ws_bound_sizes(n_calls, n_keys, mlen);
  out[1] = verify_ws_size(n_verify);
  Bump count;
  carve_verify(count, n_verify);
  out[2] = count.off;
}

int hc_ssz_prog_ok(const uint32_t* prog, uint32_t plen, size_t item_size) { return ssz_prog_ok(prog, plen, item_size); }
// the deposit signing program (SSZ_PROG_MAX words at most); *item_size = the DepositData bytes
uint32_t hc_deposit_prog(uint32_t* out, size_t* item_size) {
  std::memcpy(out, DEPOSIT_SIGNING_PROG, sizeof(DEPOSIT_SIGNING_PROG));
  *item_size = DEPOSIT_DATA_BYTES;
  return DEPOSIT_SIGNING_PROG_LEN;
}

// the deposit leaf program, hash_tree_root(DepositData); *item_size = the serialized Deposit's bytes
uint32_t hc_deposit_root_prog(uint32_t* out, size_t* item_size) {
  std::memcpy(out, DEPOSIT_ROOT_PROG, sizeof(DEPOSIT_ROOT_PROG));
  *item_size = DEPOSIT_BYTES;
  return DEPOSIT_ROOT_PROG_LEN;
}

// ---- the scopes of the host layer (bls381_scope.hpp) over the stand-ins at the top of this file
}  // extern "C"
namespace {
void si_launch(hipStream_t s) { si_log("launch " + si_name(s)); }   // work queued by the scope's user
struct Tracked {   // held data: its release shows in the log
  const char* name;
  ~Tracked() { if (name) si_log(std::string("released ") + name); }
  Tracked(const char* n) : name(n) {}
  Tracked(Tracked&& o) : name(o.name) { o.name = nullptr; }
};

// a pipeline that forks onto both side streams and is left by `how`: 0 its join, 1 an error
// return before the join, 2 an exception before the join
int fork_pipeline(Streams& q, hipStream_t s, int how) {
  Fork fk(q, s);
  si_launch(s);
  if (fk.branch(q.side) != hipSuccess) return -1;
  si_launch(q.side.stream);
  if (fk.branch(q.side2) != hipSuccess) return -1;
  si_launch(q.side2.stream);
  si_launch(s);
  if (how == 1) return -2;
  if (how == 2) throw std::runtime_error("workspace bound exceeded");
  si_log("join rc " + std::to_string(fk.join()));
  si_launch(s);
  si_log("join rc " + std::to_string(fk.join()));
  return 0;
}
// an entry that holds data for a copy on `s` and is left by its last line (0) or an error return (1)
int hold_entry(KeepList& keep, hipStream_t s, int how) {
  Held<Tracked> data(keep, s, Tracked("data"));
  si_launch(s);   // the copy that reads *data
  if (how == 1) return -2;
  si_launch(s);
  return 0;
}
void si_complete_all(KeepList& keep) {
  for (Keep& k : keep.items) k.ev->complete = true;
  si_log("complete");
}

bool run_scenario(const std::string& name, int fail_at) {
  StandIn caller{'S', -1};   // the caller's stream: not one of the context's
  hipStream_t s = &caller;
  g_si = StandInState();
  g_si.fail_at = fail_at;
  if (name == "streams") {
    Streams q;
    si_log("begin");
    g_si.counting = true;
    const hipError_t e = streams_create(q);
    g_si.counting = false;
    si_log("create rc " + std::to_string(e));
    streams_destroy(q);   // after a failure: nothing left to destroy
    si_log("end");
    return true;
  }
  const bool is_fork = name == "fork" || name == "fork_return" || name == "fork_throw";
  const bool is_hold = name == "hold" || name == "hold_return";
  if (!is_fork && !is_hold) return false;
  Streams q;
  if (streams_create(q) != hipSuccess) return false;
  si_log("begin");
  g_si.counting = true;
  if (is_fork) {
    try {
      si_log("pipeline rc " + std::to_string(fork_pipeline(q, s, name == "fork" ? 0 : name == "fork_return" ? 1 : 2)));
    } catch (const std::exception& e) {
      si_log(std::string("caught ") + e.what());
    }
  } else {
    KeepList keep;
    si_log("entry rc " + std::to_string(hold_entry(keep, s, name == "hold" ? 0 : 1)));
    // later entries on the same context: each one first releases what has completed
    { Held<Tracked> next(keep, s, Tracked("next")); }
    si_complete_all(keep);
    { Held<Tracked> last(keep, s, Tracked("last")); }
    g_si.counting = false;
    si_log("shutdown");
    keep_clear(keep);
  }
  g_si.counting = false;
  si_log("end");
  streams_destroy(q);
  return true;
}
}  // namespace
extern "C" {

// Runs the named scenario ("streams", "fork", "fork_return", "fork_throw", "hold", "hold_return")
// with the fail_at-th stand-in call after "begin" failing (0: none) and writes the call log, one
// line per call, to out.  Returns its length, or -1 for an unknown scenario or a log over cap bytes.
long hc_scope_scenario(const char* name, int fail_at, char* out, size_t cap) {
  static std::mutex mu;
  std::lock_guard<std::mutex> lk(mu);
  if (!run_scenario(name, fail_at) || g_si.log.size() > cap) return -1;
  std::memcpy(out, g_si.log.data(), g_si.log.size());
  return (long)g_si.log.size();
}

}  // extern "C"

// ---- epoch rewards (bls381_rewards.hpp): hc_mul_div_u64, hc_isqrt_u64, hc_epoch_votes,
// hc_epoch_deltas, hc_epoch_slashings, hc_effective_balances
#include "host_check_rewards.hpp"

// ---- registry updates (bls381_regupd.hpp): hc_exit_queue, hc_registry_updates
#include "host_check_regupd.hpp"

// ---- fork choice (bls381_forkchoice.hpp): hc_fork_choice_create .. hc_fork_choice_head
#include "host_check_forkchoice.hpp"

// ---- roots of variable-size items (bls381_ssz.hpp ssz_run_ragged): hc_ssz_ragged_root, hc_ssz_ragged_prog_ok
#include "host_check_ssz_ragged.hpp"
