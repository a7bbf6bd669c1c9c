// Lazy reduction: sums of Fp products accumulated in one signed double-width value
// and reduced once (DESIGN.md §5 "Lazy reduction").
//
// A wide value is 28 signed 64-bit columns, T = sum_k T[k] 2^(28k).  Products of
// signed 28/29-bit limbs accumulate in place (one v_mad_i64_i32 each), so a
// linear combination of products -- e.g. Re(a b) = a0 b0 - a1 b1, or a whole Fp2
// coefficient of an Fp6 product -- costs its products plus ONE Montgomery
// reduction, instead of one reduction per product plus a reduction per addition.
//
// wredc(T) requires -q 2^386 <= T < 2^390 q (checked by the callers' bounds):
// the columns 13..26 start at 2^22 q_j (an offset of q 2^386, a multiple of q, so
// the result is unchanged mod q) which makes the reduced value non-negative, and
// the result is normalized with value < q + (T + q 2^386) / 2^392.  Column
// bound: every column stays below 2^63 in magnitude (each caller states its sum).
//
// The per-lane functions below take the lane parity p and both coefficients of
// each Fp2 operand (e = c0, o = c1): the gfx950 kernels call them with p = the
// lane's parity in its pair and (e, o) read across the pair by DPP, the host build
// (fp2_t) calls them once per coefficient -- one source for both.
#pragma once
#include "bls381_field.hpp"

namespace bls381 {

struct wide_t { int64_t c[28]; };
typedef int32_t lv_t[14];   // a signed limb vector (|limb| < 2^30)

constexpr int WIDE_OFF_SHIFT = 22;   // offset q 2^(364 + 22) in columns 13..26

BLS_INLINE void wz_init(wide_t& T) {
#pragma unroll
  for (int k = 0; k < 28; ++k) T.c[k] = 0;
#pragma unroll
  for (int j = 0; j < 14; ++j) T.c[13 + j] = (int64_t)Q_LIMBS[j] << WIDE_OFF_SHIFT;
}

// T += x y  (signed limbs)
BLS_INLINE void wmac(wide_t& T, const lv_t& x, const lv_t& y) {
  BLS_COUNT_MACS(196);
#pragma unroll
  for (int i = 0; i < 14; ++i)
#pragma unroll
    for (int j = 0; j < 14; ++j) T.c[i + j] += (int64_t)x[i] * (int64_t)y[j];
}

// T += k x^2 for a small signed k (105 products: cross terms doubled in the multiplier)
BLS_INLINE void wsqr_k(wide_t& T, const lv_t& x, int32_t k) {
  BLS_COUNT_MACS(105);
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const int32_t d = k * x[i], c = 2 * k * x[i];
    T.c[2 * i] += (int64_t)d * (int64_t)x[i];
#pragma unroll
    for (int j = i + 1; j < 14; ++j) T.c[i + j] += (int64_t)c * (int64_t)x[j];
  }
}

// signed Montgomery reduction T 2^-392 mod q (see the header for the bounds)
BLS_INLINE fp_t wredc(wide_t& T) {
  BLS_COUNT_MACS(196);
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const uint32_t m = ((uint32_t)T.c[i] * Q_INV28) & FP_MASK;
#pragma unroll
    for (int j = 0; j < 14; ++j) T.c[i + j] = (int64_t)((uint64_t)T.c[i + j] + (uint64_t)m * Q_LIMBS[j]);
    T.c[i + 1] += T.c[i] >> 28;
  }
  fp_t r;
  int64_t c = 0;
#pragma unroll
  for (int j = 0; j < 14; ++j) {
    const int64_t v = T.c[14 + j] + c;
    r.w[j] = (uint32_t)v & FP_MASK;
    c = v >> 28;
  }
  return r;
}

// The same reduction in column order, fused with the products that feed it (fp_mont_columns'
// scheme on signed columns): col(k, acc) returns acc plus the product terms of column k
// (k = 0..26).  Column k's accumulator starts as the carry out of column k - 1 -- the addend of the
// column's first multiply-add (BLS_KEEP_ORDER) -- takes the column's products and the reduction
// products m_i q_(k-i) of the rows i < k, and for k < 14 yields its own m_k.  No wide value is
// stored (56 VGPRs in row order), and no column pays a 64-bit add for its carry: row order paid one
// per row and one per output limb.
// wz_init's offset 2^22 q_j in the columns 13 + j is row 13's digit made 2^22 larger: m_13 comes
// from the column with its offset (2^22 q_0 added to the low word), and m_13 + 2^22 < 2^29
// multiplies q_0..q_13 in m_13's place, so every column holds the sum it holds in row order.
// Each column is the same integer as T.c[k] of wredc when row k reads it, so m_k, the carries and
// the result's limbs are wredc's.  Column bound: the caller's product terms (each states its sum),
// 14 reduction products < 2^57 and a carry below 2^36 in magnitude: below 2^63 in magnitude
// (tests/test_caller_instructions.py walks the worst column on Python integers).
BLS_INLINE int64_t wz_mac(int64_t acc, int32_t x, int32_t y) { return BLS_KEEP_ORDER(acc + (int64_t)x * (int64_t)y); }

template <class F>
BLS_INLINE fp_t wredc_columns(const F& col) {
  int32_t m[14];
  fp_t r;
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 27; ++k) {
    int64_t acc = col(k, c);
#pragma unroll
    for (int i = (k > 13 ? k - 13 : 0); i < k && i < 14; ++i) acc = wz_mac(acc, m[i], (int32_t)Q_LIMBS[k - i]);
    if (k < 14) {
      const uint32_t lo = (uint32_t)acc + (k == 13 ? Q_LIMBS[0] << WIDE_OFF_SHIFT : 0u);
      m[k] = (int32_t)(((lo * Q_INV28) & FP_MASK) + (k == 13 ? 1u << WIDE_OFF_SHIFT : 0u));
      acc = wz_mac(acc, m[k], (int32_t)Q_LIMBS[0]);
    } else {
      r.w[k - 14] = (uint32_t)acc & FP_MASK;
    }
    c = acc >> 28;
  }
  r.w[13] = (uint32_t)c & FP_MASK;
  return r;
}

// column k of x y
BLS_INLINE int64_t wcol_mul(int k, int64_t acc, const lv_t& x, const lv_t& y) {
#pragma unroll
  for (int i = (k > 13 ? k - 13 : 0); i <= k && i < 14; ++i) acc = wz_mac(acc, x[i], y[k - i]);
  return acc;
}
// column k of x^2 scaled: d = the scale times x, c = twice that (wsqr_k's multipliers)
BLS_INLINE int64_t wcol_sqr(int k, int64_t acc, const lv_t& x, const lv_t& d, const lv_t& c) {
#pragma unroll
  for (int i = (k > 13 ? k - 13 : 0); 2 * i < k; ++i) acc = wz_mac(acc, c[i], x[k - i]);
  if ((k & 1) == 0) acc = wz_mac(acc, d[k / 2], x[k / 2]);
  return acc;
}

BLS_INLINE void lv_from(lv_t& r, const fp_t& a) {
#pragma unroll
  for (int k = 0; k < 14; ++k) r[k] = (int32_t)a.w[k];
}

// 6X + 2x (X < 1.03q and x < 2q normalized: < 10.2q, limbs <= 8 (2^28 - 1))
BLS_INLINE fp_t fp_6p2(const fp_t& X, const fp_t& x) {
  uint32_t s[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) s[i] = 6u * X.w[i] + (x.w[i] << 1);
  return fp_reduce_lc<6>(s);
}

// six: 6 P + 2 x, else 3 S - 2 x (+ 4q), chosen per lane in one reduction (same bounds)
BLS_INLINE fp_t fp_6p2_3m2(bool six, const fp_t& P, const fp_t& S, const fp_t& x) {
  uint32_t s[14];
#pragma unroll
  for (int i = 0; i < 14; ++i) {
    const uint32_t x2 = x.w[i] << 1;
    s[i] = six ? 6u * P.w[i] + x2 : 3u * S.w[i] + Q4B_LIMBS[i] - x2;
  }
  return fp_reduce_lc<6>(s);
}

// ---- Karabina compressed squaring, one output coefficient per call ----------
// (g2..g5) -> (g2'..g5') of cyc_csqr (bls381_pairing.hpp):
//   g2' = 6 xi g4 g5 + 2 g2          g3' = 3 (g4^2 + xi g5^2) - 2 g3
//   g4' = 3 (g2^2 + xi g3^2) - 2 g4  g5' = 6 g2 g3 + 2 g5
// with the products of each output summed in one pass over the columns (wredc_columns; lane p =
// coefficient p):
//   Re(xi a b) = a0 (b0 - b1) - a1 (b0 + b1)      Im(xi a b) = a0 (b0 + b1) + a1 (b0 - b1)
//   Re(a b) = a0 b0 - a1 b1                        Im(a b) = a0 b1 + a1 b0
//   a^2 + xi b^2: lz_sqr_xisqr below
// Inputs normalized (limbs < 2^28, values < 2q).  Column sums: xi a b and a b hold 28
// products < 2^57 (2^61.8); the reduction adds < 2^59.8.  Values: |X| < 16 q^2.

// Re/Im of xi a b
BLS_INLINE fp_t lz_xi_mul(bool p, const fp_t& a0, const fp_t& a1, const fp_t& b0, const fp_t& b1) {
  lv_t x1, y1, x2, y2;
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    const int32_t s = (int32_t)b0.w[k] + (int32_t)b1.w[k];
    const int32_t d = (int32_t)b0.w[k] - (int32_t)b1.w[k];
    x1[k] = (int32_t)a0.w[k];
    x2[k] = (int32_t)a1.w[k];
    y1[k] = p ? s : d;
    y2[k] = p ? d : -s;
  }
  BLS_COUNT_MACS(588);   // two products and the reduction
  return wredc_columns([&](int k, int64_t acc) { return wcol_mul(k, wcol_mul(k, acc, x1, y1), x2, y2); });
}

// Re/Im of a b
BLS_INLINE fp_t lz_mul(bool p, const fp_t& a0, const fp_t& a1, const fp_t& b0, const fp_t& b1) {
  lv_t x1, y1, x2, y2;
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    x1[k] = (int32_t)a0.w[k];
    x2[k] = (int32_t)a1.w[k];
    y1[k] = (int32_t)(p ? b1.w[k] : b0.w[k]);
    y2[k] = p ? (int32_t)b0.w[k] : -(int32_t)b1.w[k];
  }
  BLS_COUNT_MACS(588);   // two products and the reduction
  return wredc_columns([&](int k, int64_t acc) { return wcol_mul(k, wcol_mul(k, acc, x1, y1), x2, y2); });
}

// Re/Im of a^2 + xi b^2, with the xi b^2 part as squares:
//   Re(xi b^2) = (b0 - b1)^2 - 2 b1^2,  Im(xi b^2) = (b0 + b1)^2 - 2 b1^2
// 196 + 105 + 105 products per lane instead of 3 x 196.  u = b0 -+ b1 is squared as signed
// limbs, unreduced (round 5; it was reduced mod 2q first): |u_k| < 2^28 (lane 0) or
// u_k < 2^29 (lane 1).  Columns, lane 1 (all terms but 2 b1^2 non-negative): a-term
// 14 x 2^57 + u^2 15 x 2^58 + reduction 14 x 2^56 < 2^62.7, and -2 b1^2 > -2^60.9; lane 0 is
// smaller; in column order the reduction's row 13 carries the offset (< 2^57 a product) and the
// carry rides along (< 2^36): < 2^62.9.  Values: lane 0 in (-16 q^2, 12 q^2), lane 1 in
// (-8 q^2, 24 q^2) (u < 4q), inside wredc's (-q 2^386, 2^390 q) ~ (-42 q^2, 675 q^2).
BLS_INLINE fp_t lz_sqr_xisqr(bool p, const fp_t& a0, const fp_t& a1, const fp_t& b0, const fp_t& b1) {
  lv_t x1, y1, u, u2, v, vm2, vm4;
#pragma unroll
  for (int k = 0; k < 14; ++k) {
    const int32_t e = (int32_t)a0.w[k], o = (int32_t)a1.w[k];
    x1[k] = e + (p ? e : o);
    y1[k] = p ? o : e - o;
    const int32_t c = (int32_t)b0.w[k], d = (int32_t)b1.w[k];
    u[k] = p ? c + d : c - d;
    u2[k] = 2 * u[k];
    v[k] = d;
    vm2[k] = -2 * d;
    vm4[k] = -4 * d;
  }
  BLS_COUNT_MACS(602);   // a product, two squarings and the reduction
  return wredc_columns([&](int k, int64_t acc) {
    return wcol_sqr(k, wcol_sqr(k, wcol_mul(k, acc, x1, y1), u, u, u2), v, vm2, vm4);
  });
}

}  // namespace bls381
