// Device unit-test build of the lane-pair / quad / octet arithmetic -- TEST INFRASTRUCTURE.
//
// The device counterpart of host_check.cpp: hipcc compiles bls381_quad.hpp (which pulls in the
// pair, pairing, hash, lazy and field headers) for gfx950 into lib/libbls381_devcheck.so, with
// one small probe kernel per function under test, so that tests/test_device_arith.py can compare
// the forms the host build never sees (DPP cross-lane moves, lane-parity selects, the split Fp12
// products, the octet squarings) with Python integers.  This library is loaded only by tests;
// the product library (libbls381.so) never links it and it exports no bls381_* symbol.
//
// Boundary: every Fp crosses raw, as 14 little-endian u32 limb words (28-bit limbs), in the
// Montgomery domain (R = 2^392); nothing is converted here, so a test controls limbs and not
// only values.  One entry point runs every probe:
//   dc_run(op, n_items, in, aux, out, flag)
//     in   [item][slot < nin][lane < gin][14]   one Fp per lane of the item per slot
//     aux  [item]                               a u64 per item (scalar, count, mask), or null
//     out  [item][slot < nout][lane < g][14]
//     flag [item][lane < g]                     a u32 per lane (predicates, degenerate, fallback)
// An item owns g adjacent lanes laid out as the form under test defines: pair (g = 2) lane p =
// coefficient p; quad (g = 4) lanes {0,1} the c0 half, {2,3} the c1 half of an Fp12, or the same
// Fp2 on both halves for curve points; octet (g = 8) two quads.  gin < g: the launcher gives both
// quads the same quad input, and the test asserts that both quads return the same result.
// Every launch is a whole number of 64-lane waves: padding lanes compute on zeros, or on a copy
// of item 0 where zero is outside the function's domain, and their stores are masked.
// dc_op_count / dc_op_name / dc_op_info describe the table to the test.
//
// Probes (slots in -> slots out; an Fp12 is 6 slots on a pair, 3 on a quad):
//   pair Fp2    P_MUL (a, b -> fp2_mul, the fp2p_mul_call path, lazy operands allowed), P_SQR,
//               P_CONJ, P_MUL_XI, P_ADD_MUL_XI, P_SUB2, P_3PM2 (aux: minus), P_MUL_SMALL (aux: k),
//               P_INV, P_PRED (flag: fp2_is_zero(a) | fp2_eq(a, b) << 1 | pr_both(a0 == b0) << 2),
//               the fused combinations P_ADD_XI_SUB2, P_SUB2_ADD_XI, P_SUB2_ADD (4 operands each),
//               P_SUB_SUB_XI, P_SUB_SUB_DBL, P_DBL_SUB2, P_3A_XI_B_M2C, P_2A_B_M3C (3 each),
//               P_ADD, P_SUB, P_DBL (fp_reduce_lc's conditional-subtraction path alone)
//   pair Fp12   P12_MUL, P12_SQR, P12_CYC_SQR, P12_MUL_BY_LINE, P12_FROB (p = 1, 2, 3), P12_INV,
//               P_CSQR (cyc_csqr on (g2..g5), aux: count), P12_FINAL_EXP (final_exp, the chain with
//               the exact fallback), P12_FINAL_EXP_NOFB (final_exp_ct<.., 0>, k_final_exp_verdict's:
//               c * t3, flag = the verdict 0 / 1 / 2)
//   quad        Q_MUL, Q_SQR, Q_TWO_LINES, Q_MUL_BY_LINE (fq12_mul_by_line_q1), Q_FROB, Q_INV,
//               Q_CONJ (flag: fq12_is_one), Q_CSQR (cq_compress, cq_sqr x aux, flag: a g2 = 0 seen),
//               Q_DECOMPRESS (cq_decompress with a given inverse), Q_CYC_EXP_X (cyc_exp_x_lg and
//               cyc_exp_x_gs_lg on the quad, flag: a snapshot had g2 = 0, the fallback's condition),
//               Q_FINAL_EXP (final_exp_lg<on_quad, csqr_on_quad>)
//   octet       O_MUL, O_SQR, O_MUL_BY_LINE, O_CSQR (cq_compress, co_enter, co_sqr x aux, co_exit),
//               O_CYC_EXP_X (cyc_exp_x_lg<on_octet, ..> with csqr_on_quad, then csqr_on_octet, and
//               cyc_exp_x_gs_lg<on_octet>), O_FINAL_EXP_OQ / _OO (final_exp_lg<on_octet, ..> likewise)
//   G2          G_DBL_Q, G_ADD_AFF_Q, G_ADD_Q, G_PSI_Q, G_MUL_U64_Q (jac_mul_u64_lg<on_quad>, aux: k),
//               G_MUL_BP_Q (g2_mul_bp_lg<on_quad>), G_DBL_O, G_MUL_U64_O, G_MUL_BP_O (the same on
//               on_octet; flag: the result is the point at infinity)
//   Miller      M_QUAD (aux: bit 0 lo active, bit 1 hi active), M_Q1, M_O1 (miller_loop_lg on the
//               quad, on the octet; flag: degenerate)
#include <cstring>
#include <vector>

#include "bls381_quad.hpp"

using namespace bls381;

namespace {

// name, lanes per item, lanes per item in the input, slots in, slots out, padding = copy of item 0
#define DC_OPS(X)                      \
  X(P_MUL, 2, 2, 2, 1, 0)              \
  X(P_SQR, 2, 2, 1, 1, 0)              \
  X(P_CONJ, 2, 2, 1, 1, 0)             \
  X(P_MUL_XI, 2, 2, 1, 1, 0)           \
  X(P_ADD_MUL_XI, 2, 2, 2, 1, 0)       \
  X(P_SUB2, 2, 2, 3, 1, 0)             \
  X(P_3PM2, 2, 2, 2, 1, 0)             \
  X(P_MUL_SMALL, 2, 2, 1, 1, 0)        \
  X(P_INV, 2, 2, 1, 1, 0)              \
  X(P_PRED, 2, 2, 2, 1, 0)             \
  X(P12_MUL, 2, 2, 12, 6, 0)           \
  X(P12_SQR, 2, 2, 6, 6, 0)            \
  X(P12_CYC_SQR, 2, 2, 6, 6, 0)        \
  X(P12_MUL_BY_LINE, 2, 2, 9, 6, 0)    \
  X(P12_FROB, 2, 2, 6, 18, 0)          \
  X(P12_INV, 2, 2, 6, 6, 0)            \
  X(P_CSQR, 2, 2, 4, 4, 0)             \
  X(P12_FINAL_EXP, 2, 2, 6, 6, 1)      \
  X(P12_FINAL_EXP_NOFB, 2, 2, 6, 6, 1) \
  X(Q_MUL, 4, 4, 6, 3, 0)              \
  X(Q_SQR, 4, 4, 3, 3, 0)              \
  X(Q_TWO_LINES, 4, 4, 3, 3, 0)        \
  X(Q_MUL_BY_LINE, 4, 4, 6, 3, 0)      \
  X(Q_FROB, 4, 4, 3, 9, 0)             \
  X(Q_INV, 4, 4, 3, 3, 0)              \
  X(Q_CONJ, 4, 4, 3, 3, 0)             \
  X(Q_CSQR, 4, 4, 3, 2, 1)             \
  X(Q_DECOMPRESS, 4, 4, 3, 3, 0)       \
  X(Q_CYC_EXP_X, 4, 4, 3, 6, 1)        \
  X(Q_FINAL_EXP, 4, 4, 3, 3, 1)        \
  X(O_MUL, 8, 4, 6, 3, 0)              \
  X(O_SQR, 8, 4, 3, 3, 0)              \
  X(O_MUL_BY_LINE, 8, 4, 6, 3, 0)      \
  X(O_CSQR, 8, 4, 3, 2, 1)             \
  X(O_CYC_EXP_X, 8, 4, 3, 9, 1)        \
  X(O_FINAL_EXP_OQ, 8, 4, 3, 3, 1)     \
  X(O_FINAL_EXP_OO, 8, 4, 3, 3, 1)     \
  X(G_DBL_Q, 4, 4, 3, 3, 1)            \
  X(G_ADD_AFF_Q, 4, 4, 5, 3, 1)        \
  X(G_ADD_Q, 4, 4, 6, 3, 1)            \
  X(G_PSI_Q, 4, 4, 3, 3, 1)            \
  X(G_MUL_U64_Q, 4, 4, 2, 3, 1)        \
  X(G_MUL_BP_Q, 4, 4, 2, 3, 1)         \
  X(G_DBL_O, 8, 4, 3, 3, 1)            \
  X(G_MUL_U64_O, 8, 4, 2, 3, 1)        \
  X(G_MUL_BP_O, 8, 4, 2, 3, 1)         \
  X(M_QUAD, 4, 4, 4, 3, 1)             \
  X(M_Q1, 4, 4, 4, 3, 1)               \
  X(M_O1, 8, 4, 4, 3, 1)               \
  X(P_ADD_XI_SUB2, 2, 2, 4, 1, 0)      \
  X(P_SUB2_ADD_XI, 2, 2, 4, 1, 0)      \
  X(P_SUB2_ADD, 2, 2, 4, 1, 0)         \
  X(P_SUB_SUB_XI, 2, 2, 3, 1, 0)       \
  X(P_SUB_SUB_DBL, 2, 2, 3, 1, 0)      \
  X(P_DBL_SUB2, 2, 2, 3, 1, 0)         \
  X(P_3A_XI_B_M2C, 2, 2, 3, 1, 0)      \
  X(P_2A_B_M3C, 2, 2, 3, 1, 0)        \
  X(P_ADD, 2, 2, 2, 1, 0)              \
  X(P_SUB, 2, 2, 2, 1, 0)              \
  X(P_DBL, 2, 2, 1, 1, 0)

enum dc_op : int {
#define X(name, g, gin, nin, nout, pad) name,
  DC_OPS(X)
#undef X
      DC_NOPS
};
struct op_info { const char* name; int g, gin, nin, nout, pad; };
constexpr op_info OPS[DC_NOPS] = {
#define X(name, g, gin, nin, nout, pad) {#name, g, gin, nin, nout, pad},
    DC_OPS(X)
#undef X
};

// ---- device side: lane-major SoA buffers (word (slot * 14 + k) of lane l at [(slot * 14 + k) * L + l]),
// read and written through global-address-space pointers as the product's soa_ld / soa_st are
typedef __attribute__((address_space(1))) const uint32_t g_cu32;
typedef __attribute__((address_space(1))) uint32_t g_u32;
typedef __attribute__((address_space(1))) const uint64_t g_cu64;

__device__ __forceinline__ fp_t lane_ld(const uint32_t* __restrict__ p, size_t L, size_t lane, int slot) {
  g_cu32* g = (g_cu32*)p;
  fp_t r;
#pragma unroll
  for (int k = 0; k < FP_LIMBS; ++k) r.w[k] = g[(size_t)(slot * FP_LIMBS + k) * L + lane];
  return r;
}
__device__ __forceinline__ void lane_st(uint32_t* __restrict__ p, size_t L, size_t lane, int slot, const fp_t& a) {
  g_u32* g = (g_u32*)p;
#pragma unroll
  for (int k = 0; k < FP_LIMBS; ++k) g[(size_t)(slot * FP_LIMBS + k) * L + lane] = a.w[k];
}

using fp12p_t = fp12_g<fp2p_t>;
__device__ __forceinline__ fp12p_t mk12(const fp_t* I) {
  fp12p_t f;
  f.c0.c0 = pr_make(I[0]); f.c0.c1 = pr_make(I[1]); f.c0.c2 = pr_make(I[2]);
  f.c1.c0 = pr_make(I[3]); f.c1.c1 = pr_make(I[4]); f.c1.c2 = pr_make(I[5]);
  return f;
}
__device__ __forceinline__ void put12(fp_t* O, const fp12p_t& f) {
  O[0] = f.c0.c0.v; O[1] = f.c0.c1.v; O[2] = f.c0.c2.v; O[3] = f.c1.c0.v; O[4] = f.c1.c1.v; O[5] = f.c1.c2.v;
}
__device__ __forceinline__ fq12_t mkq(const fp_t* I) {
  fq12_t f;
  f.h.c0 = pr_make(I[0]); f.h.c1 = pr_make(I[1]); f.h.c2 = pr_make(I[2]);
  return f;
}
__device__ __forceinline__ void putq(fp_t* O, const fq12_t& f) { O[0] = f.h.c0.v; O[1] = f.h.c1.v; O[2] = f.h.c2.v; }
__device__ __forceinline__ jac_t<fp2p_t> mkjac(const fp_t* I) {
  jac_t<fp2p_t> p; p.x = pr_make(I[0]); p.y = pr_make(I[1]); p.z = pr_make(I[2]); return p;
}
__device__ __forceinline__ aff_t<fp2p_t> mkaff(const fp_t* I) {
  aff_t<fp2p_t> p; p.x = pr_make(I[0]); p.y = pr_make(I[1]); return p;
}
__device__ __forceinline__ void putjac(fp_t* O, uint32_t& fl, const jac_t<fp2p_t>& p) {
  O[0] = p.x.v; O[1] = p.y.v; O[2] = p.z.v;
  fl = jac_is_inf(p) ? 1u : 0u;
}
__device__ __forceinline__ g1_line_pre mkg1(const fp_t* I) {
  aff_t<fp_t> P; P.x = I[0]; P.y = I[1];
  return g1_prepare(P);
}
// the snapshots' g2 = 0 test of cyc_exp_x_lg (the condition of its exact fallback)
__device__ __forceinline__ bool snapshot_g2_zero(const fq12_t& f) {
  cq_t g = cq_compress(f);
  bool zero = false;
  for (int s = 0; s < 6; ++s) {
    for (int j = CYC_X_RUNS_RTL[s]; j > 0; --j) g = cq_sqr(g);
    zero = zero | fp2_is_zero(cq_g2(g));
  }
  return zero;
}

// force-inlined into its kernel: the operand arrays never cross a call
template <int OP>
__device__ __forceinline__ void probe(const fp_t* I, uint64_t aux, fp_t* O, uint32_t& fl) {
  if constexpr (OP == P_MUL) O[0] = fp2_mul(pr_make(I[0]), pr_make(I[1])).v;
  else if constexpr (OP == P_SQR) O[0] = fp2_sqr(pr_make(I[0])).v;
  else if constexpr (OP == P_CONJ) O[0] = fp2_conj(pr_make(I[0])).v;
  else if constexpr (OP == P_MUL_XI) O[0] = fp2_mul_xi(pr_make(I[0])).v;
  else if constexpr (OP == P_ADD_MUL_XI) O[0] = fp2_add_mul_xi(pr_make(I[0]), pr_make(I[1])).v;
  else if constexpr (OP == P_SUB2) O[0] = fp2_sub2(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_3PM2) O[0] = fp2_3pm2(pr_make(I[0]), pr_make(I[1]), aux != 0).v;
  else if constexpr (OP == P_MUL_SMALL) O[0] = fp2_mul_small(pr_make(I[0]), (int)aux).v;
  else if constexpr (OP == P_INV) O[0] = fp2_inv(pr_make(I[0])).v;
  else if constexpr (OP == P_PRED) {
    const fp2p_t a = pr_make(I[0]), b = pr_make(I[1]);
    const fp_t a0 = pr_dpp<DPP_EVEN>(a.v), b0 = pr_dpp<DPP_EVEN>(b.v);
    fl = (fp2_is_zero(a) ? 1u : 0u) | (fp2_eq(a, b) ? 2u : 0u) | (pr_both(fp_eq(a0, b0)) ? 4u : 0u);
    O[0] = fp_zero();
  } else if constexpr (OP == P12_MUL) put12(O, fp12_mul(mk12(I), mk12(I + 6)));
  else if constexpr (OP == P12_SQR) put12(O, fp12_sqr(mk12(I)));
  else if constexpr (OP == P12_CYC_SQR) put12(O, fp12_cyclotomic_sqr(mk12(I)));
  else if constexpr (OP == P12_MUL_BY_LINE)
    put12(O, fp12_mul_by_line(mk12(I), pr_make(I[6]), pr_make(I[7]), pr_make(I[8])));
  else if constexpr (OP == P12_FROB) {
    for (int p = 1; p <= 3; ++p) put12(O + 6 * (p - 1), fp12_frob(mk12(I), p));
  } else if constexpr (OP == P12_INV) put12(O, fp12_inv(mk12(I)));
  else if constexpr (OP == P_CSQR) {
    cyc_bc<fp2p_t> g;
    g.g2 = pr_make(I[0]); g.g3 = pr_make(I[1]); g.g4 = pr_make(I[2]); g.g5 = pr_make(I[3]);
    for (uint64_t j = 0; j < aux; ++j) g = cyc_csqr(g);
    O[0] = g.g2.v; O[1] = g.g3.v; O[2] = g.g4.v; O[3] = g.g5.v;
  } else if constexpr (OP == P12_FINAL_EXP) put12(O, final_exp(mk12(I)));
  else if constexpr (OP == P12_FINAL_EXP_NOFB) {
    const fe_ct<fp2p_t> r = final_exp_ct<fp2p_t, 0>(mk12(I));
    const bool z0 = fp2_is_zero(r.c.c0.c0), z1 = fp2_is_zero(r.c.c1.c0);
    const bool one = fp12_eq(r.c, fp12_conj(r.t3));
    fl = (z0 && z1) ? 2u : (one ? 1u : 0u);   // final_exp_check<fp2p_t, 0>'s verdict
    put12(O, fp12_mul_inl(r.c, r.t3));
  } else if constexpr (OP == Q_MUL) putq(O, fq12_mul(mkq(I), mkq(I + 3)));
  else if constexpr (OP == Q_SQR) putq(O, fq12_sqr(mkq(I)));
  else if constexpr (OP == Q_TWO_LINES) putq(O, fq12_two_lines(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])));
  else if constexpr (OP == Q_MUL_BY_LINE)
    putq(O, fq12_mul_by_line_q1(mkq(I), pr_make(I[3]), pr_make(I[4]), pr_make(I[5])));
  else if constexpr (OP == Q_FROB) {
    for (int p = 1; p <= 3; ++p) putq(O + 3 * (p - 1), fq12_frob(mkq(I), p));
  } else if constexpr (OP == Q_INV) putq(O, fq12_inv(mkq(I)));
  else if constexpr (OP == Q_CONJ) {
    putq(O, fq12_conj(mkq(I)));
    fl = fq12_is_one(mkq(I)) ? 1u : 0u;
  } else if constexpr (OP == Q_CSQR) {
    cq_t g = cq_compress(mkq(I));
    bool zero = false;
    for (uint64_t j = 0; j < aux; ++j) {
      g = cq_sqr(g);
      zero = zero | fp2_is_zero(cq_g2(g));
    }
    O[0] = g.x.v; O[1] = g.y.v;
    fl = zero ? 1u : 0u;
  } else if constexpr (OP == Q_DECOMPRESS) {
    cq_t g;
    g.x = pr_make(I[0]); g.y = pr_make(I[1]);
    putq(O, cq_decompress(g, pr_make(I[2])));
  } else if constexpr (OP == Q_CYC_EXP_X) {
    putq(O, cyc_exp_x_lg<on_quad, csqr_on_quad>(mkq(I)));
    putq(O + 3, cyc_exp_x_gs_lg<on_quad>(mkq(I)));
    fl = snapshot_g2_zero(mkq(I)) ? 1u : 0u;
  } else if constexpr (OP == Q_FINAL_EXP) putq(O, final_exp_lg<on_quad, csqr_on_quad>(mkq(I)));
  else if constexpr (OP == O_MUL) putq(O, fq12_mul_oct(mkq(I), mkq(I + 3)));
  else if constexpr (OP == O_SQR) putq(O, fq12_sqr_oct(mkq(I)));
  else if constexpr (OP == O_MUL_BY_LINE)
    putq(O, fq12_mul_by_line_oct(mkq(I), pr_make(I[3]), pr_make(I[4]), pr_make(I[5])));
  else if constexpr (OP == O_CSQR) {
    fp2p_t g = co_enter(cq_compress(mkq(I)));
    for (uint64_t j = 0; j < aux; ++j) g = co_sqr(g);
    const cq_t r = co_exit(g);
    O[0] = r.x.v; O[1] = r.y.v;
    fl = fp2_is_zero(cq_g2(r)) ? 1u : 0u;
  } else if constexpr (OP == O_CYC_EXP_X) {
    putq(O, cyc_exp_x_lg<on_octet, csqr_on_quad>(mkq(I)));
    putq(O + 3, cyc_exp_x_lg<on_octet, csqr_on_octet>(mkq(I)));
    putq(O + 6, cyc_exp_x_gs_lg<on_octet>(mkq(I)));
    fl = snapshot_g2_zero(mkq(I)) ? 1u : 0u;
  } else if constexpr (OP == O_FINAL_EXP_OQ) putq(O, final_exp_lg<on_octet, csqr_on_quad>(mkq(I)));
  else if constexpr (OP == O_FINAL_EXP_OO) putq(O, final_exp_lg<on_octet, csqr_on_octet>(mkq(I)));
  else if constexpr (OP == G_DBL_Q) putjac(O, fl, jac_dbl_q(mkjac(I)));
  else if constexpr (OP == G_ADD_AFF_Q) putjac(O, fl, jac_add_aff_q(mkjac(I), mkaff(I + 3)));
  else if constexpr (OP == G_ADD_Q) putjac(O, fl, jac_add_q(mkjac(I), mkjac(I + 3)));
  else if constexpr (OP == G_PSI_Q) putjac(O, fl, g2_psi_jac_q(mkjac(I)));
  else if constexpr (OP == G_MUL_U64_Q) putjac(O, fl, jac_mul_u64_lg<on_quad>(mkaff(I), aux));
  else if constexpr (OP == G_MUL_BP_Q) putjac(O, fl, g2_mul_bp_lg<on_quad>(mkaff(I)));
  else if constexpr (OP == G_DBL_O) putjac(O, fl, jac_dbl_o(mkjac(I)));
  else if constexpr (OP == G_MUL_U64_O) putjac(O, fl, jac_mul_u64_lg<on_octet>(mkaff(I), aux));
  else if constexpr (OP == G_MUL_BP_O) putjac(O, fl, g2_mul_bp_lg<on_octet>(mkaff(I)));
  else if constexpr (OP == M_QUAD) {
    const bool active = ((aux >> (qd_hi() ? 1 : 0)) & 1u) != 0;
    bool degen = false;
    putq(O, miller_loop_quad(mkaff(I), mkg1(I + 2), active, degen));
    fl = degen ? 1u : 0u;
  } else if constexpr (OP == M_Q1) {
    bool degen = false;
    putq(O, miller_loop_lg<on_quad>(mkaff(I), mkg1(I + 2), degen));
    fl = degen ? 1u : 0u;
  } else if constexpr (OP == M_O1) {
    const fq12_ml r = miller_loop_lg_run<on_octet>(mkaff(I), mkg1(I + 2));
    putq(O, r.f);
    fl = r.degenerate ? 1u : 0u;
  } else if constexpr (OP == P_ADD_XI_SUB2)
    O[0] = fp2_add_xi_sub2(pr_make(I[0]), pr_make(I[1]), pr_make(I[2]), pr_make(I[3])).v;
  else if constexpr (OP == P_SUB2_ADD_XI)
    O[0] = fp2_sub2_add_xi(pr_make(I[0]), pr_make(I[1]), pr_make(I[2]), pr_make(I[3])).v;
  else if constexpr (OP == P_SUB2_ADD)
    O[0] = fp2_sub2_add(pr_make(I[0]), pr_make(I[1]), pr_make(I[2]), pr_make(I[3])).v;
  else if constexpr (OP == P_SUB_SUB_XI) O[0] = fp2_sub_sub_xi(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_SUB_SUB_DBL) O[0] = fp2_sub_sub_dbl(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_DBL_SUB2) O[0] = fp2_dbl_sub2(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_3A_XI_B_M2C) O[0] = fp2_3a_xi_b_m2c(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_2A_B_M3C) O[0] = fp2_2a_b_m3c(pr_make(I[0]), pr_make(I[1]), pr_make(I[2])).v;
  else if constexpr (OP == P_ADD) O[0] = fp2_add(pr_make(I[0]), pr_make(I[1])).v;
  else if constexpr (OP == P_SUB) O[0] = fp2_sub(pr_make(I[0]), pr_make(I[1])).v;
  else if constexpr (OP == P_DBL) O[0] = fp2_dbl(pr_make(I[0])).v;
}

// BLOCK lanes per block -- one wave, or for dc_run_wg the product kernels' workgroup of two (KBLOCK);
// L lanes in all (a multiple of BLOCK), the first `live` of them store
template <int OP, int BLOCK>
__global__ void __launch_bounds__(BLOCK) k_probe(const uint32_t* __restrict__ in, const uint64_t* __restrict__ aux,
                                              uint32_t* __restrict__ out, uint32_t* __restrict__ flag, size_t L,
                                              size_t live) {
  constexpr int NIN = OPS[OP].nin, NOUT = OPS[OP].nout;
  const size_t lane = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  fp_t I[NIN], O[NOUT];
#pragma unroll
  for (int j = 0; j < NIN; ++j) I[j] = lane_ld(in, L, lane, j);
  const uint64_t ax = ((g_cu64*)aux)[lane];
  uint32_t fl = 0;
  probe<OP>(I, ax, O, fl);
  if (lane >= live) return;
#pragma unroll
  for (int j = 0; j < NOUT; ++j) lane_st(out, L, lane, j, O[j]);
  ((g_u32*)flag)[lane] = fl;
}

// the lane-pair probes of at most four operands also exist as one workgroup of KBLOCK lanes
constexpr bool wg_probe(int op) { return OPS[op].g == 2 && OPS[op].nin <= 4 && OPS[op].nout <= 4; }

template <int OP>
hipError_t launch(int op, size_t L, size_t live, const uint32_t* in, const uint64_t* aux, uint32_t* out,
                  uint32_t* flag, int block) {
  if constexpr (OP < DC_NOPS) {
    if (op != OP) return launch<OP + 1>(op, L, live, in, aux, out, flag, block);
    if (block == 64) {
      hipLaunchKernelGGL((k_probe<OP, 64>), dim3((unsigned)(L / 64)), dim3(64), 0, 0, in, aux, out, flag, L, live);
    } else {
      if constexpr (wg_probe(OP)) {
        if (block != KBLOCK || L % KBLOCK) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_probe<OP, KBLOCK>), dim3((unsigned)(L / KBLOCK)), dim3(KBLOCK), 0, 0, in, aux, out, flag,
                           L, live);
      } else {
        return hipErrorInvalidValue;
      }
    }
    return hipGetLastError();
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace

extern "C" {

int dc_op_count() { return DC_NOPS; }
const char* dc_op_name(int op) { return (op >= 0 && op < DC_NOPS) ? OPS[op].name : nullptr; }
// info = {lanes per item, lanes per item in the input, slots in, slots out}
int dc_op_info(int op, int info[4]) {
  if (op < 0 || op >= DC_NOPS) return -1;
  info[0] = OPS[op].g; info[1] = OPS[op].gin; info[2] = OPS[op].nin; info[3] = OPS[op].nout;
  return 0;
}

}  // extern "C"
namespace {
// 0 or the HIP error code; host pointers in and out, null stream, nothing left allocated
int run(int op, size_t n, const uint32_t* in, const uint64_t* aux, uint32_t* out, uint32_t* flag, int block) {
  if (op < 0 || op >= DC_NOPS || n == 0 || n > 4096) return (int)hipErrorInvalidValue;
  const op_info& o = OPS[op];
  const size_t per_wave = (size_t)block / (size_t)o.g;
  const size_t n_pad = (n + per_wave - 1) / per_wave * per_wave;
  const size_t L = n_pad * o.g, live = n * o.g;
  std::vector<uint32_t> hin((size_t)o.nin * FP_LIMBS * L, 0u), hout((size_t)o.nout * FP_LIMBS * L);
  std::vector<uint64_t> haux(L, 0u);
  std::vector<uint32_t> hflag(L);
  for (size_t i = 0; i < n_pad; ++i) {
    if (i >= n && !o.pad) continue;      // zeros
    const size_t src = i < n ? i : 0;    // or a copy of item 0
    for (int l = 0; l < o.g; ++l) {
      const size_t lane = i * o.g + l;
      haux[lane] = aux ? aux[src] : 0;
      for (int j = 0; j < o.nin; ++j)
        for (int k = 0; k < FP_LIMBS; ++k)
          hin[(size_t)(j * FP_LIMBS + k) * L + lane] = in[((src * o.nin + j) * o.gin + (size_t)(l % o.gin)) * FP_LIMBS + k];
    }
  }
  uint32_t *din = nullptr, *dout = nullptr, *dflag = nullptr;
  uint64_t* daux = nullptr;
  hipError_t e = hipMalloc(&din, hin.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, hout.size() * 4);
  if (e == hipSuccess) e = hipMalloc(&dflag, L * 4);
  if (e == hipSuccess) e = hipMalloc(&daux, L * 8);
  if (e == hipSuccess) e = hipMemcpy(din, hin.data(), hin.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(daux, haux.data(), L * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch<0>(op, L, live, din, daux, dout, dflag, block);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(hout.data(), dout, hout.size() * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(hflag.data(), dflag, L * 4, hipMemcpyDeviceToHost);
  (void)hipFree(din); (void)hipFree(dout); (void)hipFree(dflag); (void)hipFree(daux);
  if (e != hipSuccess) return (int)e;
  for (size_t i = 0; i < n; ++i)
    for (int l = 0; l < o.g; ++l) {
      const size_t lane = i * o.g + l;
      flag[lane] = hflag[lane];
      for (int j = 0; j < o.nout; ++j)
        for (int k = 0; k < FP_LIMBS; ++k)
          out[((i * o.nout + j) * o.g + l) * FP_LIMBS + k] = hout[(size_t)(j * FP_LIMBS + k) * L + lane];
    }
  return 0;
}
}  // namespace
extern "C" {

int dc_run(int op, size_t n, const uint32_t* in, const uint64_t* aux, uint32_t* out, uint32_t* flag) {
  return run(op, n, in, aux, out, flag, 64);
}
// the same on workgroups of KBLOCK lanes (two waves, the product kernels' shape): the lane-pair probes
// of at most four operands only, any other op is hipErrorInvalidValue
int dc_run_wg(int op, size_t n, const uint32_t* in, const uint64_t* aux, uint32_t* out, uint32_t* flag) {
  return run(op, n, in, aux, out, flag, KBLOCK);
}

}  // extern "C"
