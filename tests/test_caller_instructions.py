"""The rewritten forms around the lane-pair Fp2 products: same limbs as the forms they replace.

Two rewrites (bls381_field.hpp, bls381_lazy.hpp), each checked limb for limb against Python integers,
against the replaced formula kept here as Python, and against the host build:

* fp_reduce_lc.  The conditional -2q of the KMAX <= 2 path is the addend `NQ2 & m` with m a lane mask
  (it was `s - (Q2 & m)`), the same sum mod 2^32 limb by limb; the k <= 7 path computes k in
  straight-line code (`reduce_new` against `reduce_parent`).  Every KMAX in use (2..8) is reached: 2 by
  fp_add / fp_sub / fp_neg / fp_dbl, 3 by fp_add_sub / fp_add3 / fp_sub2, 5 by fp_3m2 / fp_3p2, 8 by
  fp_mul_small, 4..8 by the fused tower combinations; the lane-pair probes add both lane parities of
  fp2_mul_xi, fp2_add_mul_xi, fp2_conj and the fused forms.
* lz_mul, lz_xi_mul, lz_sqr_xisqr in column order (wredc_columns) against the row order of wredc over a
  stored wide value (`lz_columns` against `lz_rows`), both lane parities.  The column accumulation is
  walked in the source's order with the carry as the first addend and every partial sum held below 2^63
  in magnitude; the worst column is stated in test_lazy_columns_equal_rows_and_stay_in_range.

Operands: limbs 0..12 all 2^28 - 1 (the largest such value below 2q), the top limb at its bound
(Q2_13) over zero low limbs, 2q - 1, zero, q, and 32 seeded random values per form.  The device
tests run the same operands on one workgroup of 128 lanes (64 lane pairs: the first and the last pair
of a wave, and the boundary between the workgroup's two waves) and compare with the host build.
"""
import ctypes
import os
import random

import numpy as np
import pytest

import bls_oracle as O
import devcheck_vectors as V
from test_leaf_columns import _const
from test_tower_combinations import AO, FORMS, OFFSET, Chain, cases, host_form, model

q = O.q
Q2, MASK = V.Q2, V.MASK
M32 = (1 << 32) - 1
Q_LIMBS = _const("Q_LIMBS")
Q2_LIMBS = _const("Q2_LIMBS")
NQ2_LIMBS = _const("NQ2_LIMBS")
Q2B, Q4B = _const("Q2B_LIMBS"), _const("Q4B_LIMBS")
LC_DIV_MAGIC = _const("LC_DIV_MAGIC")[0]
Q_INV28 = _const("Q_INV28")[0]
TOPB = Q2_LIMBS[13] << 364            # the top limb at its bound, low limbs zero (< 2q)
EXT = [AO, TOPB, Q2 - 1, 0, q]


def i32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def test_constants():
    assert [(-x) & M32 for x in Q2_LIMBS] == list(NQ2_LIMBS)
    assert V.is_normalised(V.limbs(TOPB)) and TOPB < Q2 and V.limbs(TOPB)[13] == Q2_LIMBS[13]
    assert V.limbs(AO)[:13] == (MASK,) * 13 and V.limbs(Q2 - 1)[13] == Q2_LIMBS[13]


# ------------------------------------------------------------- fp_reduce_lc --
def _finish(t):
    """fp_carry and the exact conditional subtraction, shared by both forms (unchanged code)."""
    t = list(t)
    for i in range(13):
        t[i + 1] = i32(t[i + 1] + (t[i] >> 28))
        t[i] &= MASK
    if t[13] >= Q2_LIMBS[13]:
        e = [t[i] - Q2_LIMBS[i] for i in range(14)]
        for i in range(13):
            e[i + 1] += e[i] >> 28
            e[i] &= MASK
        if e[13] >= 0:
            t = e
    return tuple(x & M32 for x in t)


def reduce_parent(s, kmax):
    """The replaced fp_reduce_lc on u32 limb sums (two's complement as the C++)."""
    s = [x & M32 for x in s]
    if kmax <= 2:
        m = M32 if i32(s[13]) > Q2_LIMBS[13] else 0
        t = [i32(s[i] - (Q2_LIMBS[i] & m)) for i in range(14)]
    else:
        top = max(i32(s[13]), 0)
        k = (top * LC_DIV_MAGIC) >> 40
        t = [i32(s[i] + k * NQ2_LIMBS[i]) for i in range(14)]
    return _finish(t)


def reduce_new(s, kmax):
    """fp_reduce_lc as it is now: -2q enters as the addend NQ2 & m, mod 2^32."""
    s = [x & M32 for x in s]
    if kmax <= 2:
        m = M32 if i32(s[13]) > Q2_LIMBS[13] else 0
        t = [i32(s[i] + (NQ2_LIMBS[i] & m)) for i in range(14)]
    else:
        top = max(i32(s[13]), 0)
        k = (top * LC_DIV_MAGIC) >> 40
        assert k <= 7
        t = [i32(s[i] + k * NQ2_LIMBS[i]) for i in range(14)]
    return _finish(t)


# hc_fp_lc_raw's ops: (op, KMAX, operands, limb sum, value)
def _lc_ops():
    ops = [
        (0, 2, 2, lambda a, b, c, i: a[i] + b[i], lambda a, b, c: a + b),
        (1, 2, 2, lambda a, b, c, i: a[i] + Q2B[i] - b[i], lambda a, b, c: a - b),
        (2, 2, 1, lambda a, b, c, i: Q2B[i] - a[i], lambda a, b, c: -a),
        (3, 2, 1, lambda a, b, c, i: a[i] << 1, lambda a, b, c: 2 * a),
        (4, 3, 3, lambda a, b, c, i: a[i] + b[i] + Q2B[i] - c[i], lambda a, b, c: a + b - c),
        (5, 3, 3, lambda a, b, c, i: a[i] + b[i] + c[i], lambda a, b, c: a + b + c),
        (6, 3, 3, lambda a, b, c, i: a[i] + Q4B[i] - b[i] - c[i], lambda a, b, c: a - b - c),
        (7, 5, 2, lambda a, b, c, i: 3 * a[i] + Q4B[i] - (b[i] << 1), lambda a, b, c: 3 * a - 2 * b),
        (8, 5, 2, lambda a, b, c, i: 3 * a[i] + (b[i] << 1), lambda a, b, c: 3 * a + 2 * b),
    ]
    for k in range(1, 9):
        ops.append((8 + k, 8, 1, (lambda k: lambda a, b, c, i: k * a[i])(k), (lambda k: lambda a, b, c: k * a)(k)))
    return ops


LC_OPS = _lc_ops()


def lc_operands(seed):
    """Triples of values: every combination of the extremes in the first two operands, then 32 random."""
    rng = random.Random(seed)
    out = [(x, y, z) for x in EXT for y in EXT for z in (EXT[0], EXT[3])]
    for _ in range(32):
        out.append(tuple(rng.choice(EXT) if rng.random() < 0.25 else rng.randrange(Q2) for _ in range(3)))
    return out


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_raw_fp2_lc.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_raw_fp2.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_fp_lc_raw.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    return lib


def test_reduce_lc_two_operand_forms(L):
    """KMAX 2, 3, 5, 8: the new reduction, the replaced one, the integers and the host build agree."""
    ch = Chain(L)
    seen = set()
    for op, kmax, nops, limb, val in LC_OPS:
        for x, y, z in lc_operands(9000 + op):
            a, b, c = V.limbs(x), V.limbs(y), V.limbs(z)
            s = [limb(a, b, c, i) for i in range(14)]
            assert all(0 <= v <= (1 << 31) - 8 for v in s[:13]) and s[13] >= -2
            want = V.limbs(val(x, y, z) % Q2)
            got = reduce_new(s, kmax)
            assert got == reduce_parent(s, kmax) == want, (op, x, y, z)
            assert ch.fp(op, a, b, c) == want, (op, x, y, z)
            seen.add(kmax)
    assert seen == {2, 3, 5, 8}


def _form_sum(form_coeff, it):
    add, sub = form_coeff
    off = OFFSET[len(sub)][0]
    return [off[i] + sum(it[2 * j + p][i] for j, p in add) - sum(it[2 * j + p][i] for j, p in sub) for i in range(14)]


def test_reduce_lc_fused_forms(L):
    """KMAX 4..8 through the fused tower combinations' limb sums."""
    seen = set()
    for form in FORMS:
        for n, it in enumerate(cases(form)):
            want = model(form, it)
            for p, coeff in enumerate(form[2]):
                kmax = len(coeff[0]) + OFFSET[len(coeff[1])][1]
                s = _form_sum(coeff, it)
                assert reduce_new(s, kmax) == reduce_parent(s, kmax) == want[p], (form[0], n, p)
                seen.add(kmax)
            assert host_form(L, form, it) == want
    assert seen == {4, 5, 6, 7, 8}


# ------------------------------------------------------ lazy reductions (Fp2) --
def _lz_terms(name, p, a0, a1, b0, b1):
    """The signed limb vectors of one lz_* call: products [(x, y)] and squares [(x, scale)]."""
    if name == "xi_mul":
        s = [x + y for x, y in zip(b0, b1)]
        d = [x - y for x, y in zip(b0, b1)]
        return [(a0, s if p else d), (a1, d if p else [-x for x in s])], []
    if name == "mul":
        return [(a0, b1 if p else b0), (a1, b0 if p else [-x for x in b1])], []
    x1 = [e + (e if p else o) for e, o in zip(a0, a1)]
    y1 = [o if p else e - o for e, o in zip(a0, a1)]
    u = [c + d if p else c - d for c, d in zip(b0, b1)]
    return [(x1, y1)], [(u, 1), (list(b1), -2)]


def lz_rows(name, p, a0, a1, b0, b1):
    """The replaced form: the stored wide value with wz_init's offset, reduced row by row (wredc)."""
    prods, sqrs = _lz_terms(name, p, a0, a1, b0, b1)
    T = [0] * 28
    for j in range(14):
        T[13 + j] = Q_LIMBS[j] << 22
    for x, y in prods:
        for i in range(14):
            for j in range(14):
                T[i + j] += x[i] * y[j]
    for x, k in sqrs:
        for i in range(14):
            T[2 * i] += k * x[i] * x[i]
            for j in range(i + 1, 14):
                T[i + j] += 2 * k * x[i] * x[j]
    total = sum(t << (28 * k) for k, t in enumerate(T))
    for i in range(14):
        m = ((T[i] & M32) * Q_INV28) & MASK
        for j in range(14):
            T[i + j] += m * Q_LIMBS[j]
        assert all(abs(t) < 1 << 63 for t in T)
        T[i + 1] += T[i] >> 28
    r, c = [], 0
    for j in range(14):
        v = T[14 + j] + c
        r.append(v & MASK)
        c = v >> 28
    return tuple(r), total


def lz_columns(name, p, a0, a1, b0, b1, worst=None):
    """wredc_columns with the source's accumulation order; every partial sum is range-checked."""
    prods, sqrs = _lz_terms(name, p, a0, a1, b0, b1)
    sq = [(x, [k * v for v in x], [2 * k * v for v in x]) for x, k in sqrs]    # x, d, c of wcol_sqr
    assert all(abs(v) < 1 << 31 for x, d, c2 in sq for v in x + d + c2)
    assert all(abs(v) < 1 << 31 for x, y in prods for v in list(x) + list(y))
    peak = [0]

    def mac(acc, x, y):
        acc += x * y
        peak[0] = max(peak[0], abs(acc))
        assert abs(acc) < 1 << 63
        return acc

    m, r, c = [0] * 14, [0] * 14, 0
    for k in range(27):
        acc = c                                          # the carry: the first multiply-add's addend
        lo = max(0, k - 13)
        for x, y in prods:
            for i in range(lo, min(k, 13) + 1):
                acc = mac(acc, x[i], y[k - i])
        for x, d, c2 in sq:
            for i in range(lo, (k + 1) // 2):
                acc = mac(acc, c2[i], x[k - i])
            if k % 2 == 0:
                acc = mac(acc, d[k // 2], x[k // 2])
        for i in range(lo, min(k, 14)):
            acc = mac(acc, m[i], Q_LIMBS[k - i])
        if k < 14:
            low = (acc + ((Q_LIMBS[0] << 22) if k == 13 else 0)) & M32
            m[k] = ((low * Q_INV28) & MASK) + ((1 << 22) if k == 13 else 0)
            assert m[k] < 1 << 29
            acc = mac(acc, m[k], Q_LIMBS[0])
            assert acc & MASK == 0     # the column's low limb is cleared
        else:
            r[k - 14] = acc & MASK
        c = acc >> 28
        assert abs(c) < 1 << 36
    r[13] = c & MASK
    assert 0 <= c <= MASK
    if worst is not None:
        worst.append(peak[0])
    return tuple(r)


def lz_items(seed):
    """(g a, g b) coefficient quadruples: the extremes in every slot, one slot at an extreme, then random."""
    rng = random.Random(seed)
    vals = [(x,) * 4 for x in EXT]
    for big in EXT[:3]:
        for j in range(4):
            vals.append(tuple(big if i == j else 0 for i in range(4)))
            vals.append(tuple(0 if i == j else big for i in range(4)))
    for _ in range(32):
        vals.append(tuple(rng.choice(EXT) if rng.random() < 0.25 else rng.randrange(Q2) for _ in range(4)))
    return [tuple(V.limbs(v) for v in it) for it in vals]


def test_lazy_columns_equal_rows_and_stay_in_range():
    """Column order returns row order's limbs; the result is T / 2^392 mod q below the stated bound.
    Worst column (lz_sqr_xisqr on the odd lane, where u = b0 + b1 < 2^29 and every term but -2 b1^2 is
    positive; columns 12 to 14): 14 products x1 y1 < 2^57, u^2 as at most 7 doubled cross terms < 2^59
    and one square < 2^58, 14 reduction products < 2^57 (m_13 + 2^22 < 2^29) and a carry below 2^36:
    58 x 2^57 + 2^36 < 2^62.9.  The walk holds every partial sum of every column under 2^63 in the
    source's order, and the measured peak under that bound."""
    worst = []
    for name in ("mul", "xi_mul", "sqr_xisqr"):
        for it in lz_items(9100):
            for p in (0, 1):
                rows, total = lz_rows(name, p, *it)
                cols = lz_columns(name, p, *it, worst=worst)
                assert cols == rows, (name, p)
                val = V.value(cols)
                assert V.is_normalised(cols) and (val << 392) % q == total % q
                assert val < q + ((total + (q << 386)) >> 392) + 1
    assert max(worst) < 14 * 2 ** 57 + 7 * 2 ** 59 + 2 ** 58 + 14 * 2 ** 57 + 2 ** 36 < 2 ** 63


def csqr_model(g, lz):
    """cyc_csqr on raw limbs (g2, g3, g4, g5 as c0, c1 each) with the given lz_* implementation."""
    g2, g3, g4, g5 = ((g[2 * j], g[2 * j + 1]) for j in range(4))
    out = []

    def p6(X, x):
        return reduce_new([6 * X[i] + (x[i] << 1) for i in range(14)], 6)

    def m3(X, x):
        return reduce_new([3 * X[i] + Q4B[i] - (x[i] << 1) for i in range(14)], 5)

    for p in (0, 1):
        out.append((p6(lz("xi_mul", p, *g4, *g5), g2[p]), m3(lz("sqr_xisqr", p, *g4, *g5), g3[p]),
                    m3(lz("sqr_xisqr", p, *g2, *g3), g4[p]), p6(lz("mul", p, *g2, *g3), g5[p])))
    return [out[p][j] for j in range(4) for p in (0, 1)]


def host_csqr(L, g):
    flat = [w for l in g for w in l]
    buf, out = (ctypes.c_uint32 * len(flat))(*flat), (ctypes.c_uint32 * (14 * 8))()
    assert L.hc_raw_fp2(3, buf, 1, out) == 0
    return [tuple(out[14 * j:14 * j + 14]) for j in range(8)]


def csqr_items(seed=9200):
    rng = random.Random(seed)
    vals = [(x,) * 8 for x in EXT]
    vals += [tuple(EXT[(i + j) % 3] for i in range(8)) for j in range(3)]
    for _ in range(32):
        vals.append(tuple(rng.choice(EXT) if rng.random() < 0.25 else rng.randrange(Q2) for _ in range(8)))
    return [[V.limbs(v) for v in it] for it in vals]


def test_host_compressed_squaring_equals_both_orders(L):
    """The host build's cyc_csqr (both lane parities of every lz_* form, then fp_6p2 / fp_3m2) returns the
    limbs of the column-order model and of the replaced row-order one."""
    for n, g in enumerate(csqr_items()):
        got = host_csqr(L, g)
        assert got == csqr_model(g, lz_columns), n
        assert got == csqr_model(g, lambda *a: lz_rows(*a)[0]), n


# -------------------------------------------------------------------- device --
class DevWG:
    """dc_run_wg of the device check library: one workgroup of 128 lanes per 64 lane pairs."""

    def __init__(self, dev):
        self.dev = dev
        dev.L.dc_run_wg.argtypes = [ctypes.c_int, ctypes.c_size_t] + [ctypes.c_void_p] * 4

    def run(self, name, lanes, aux=None):
        op, g, gin, nin, nout = self.dev.ops[name]
        a = np.ascontiguousarray(np.asarray(lanes, dtype=np.uint32))
        n = a.shape[0]
        assert g == 2 and n == 64 and a.shape == (n, nin, gin, 14), (name, a.shape)
        x = np.asarray(aux if aux is not None else [0] * n, dtype=np.uint64)
        out = np.zeros((n, nout, g, 14), dtype=np.uint32)
        flag = np.zeros((n, g), dtype=np.uint32)
        rc = self.dev.L.dc_run_wg(op, n, a.ctypes.data, x.ctypes.data, out.ctypes.data, flag.ctypes.data)
        assert rc == 0, "%s: HIP error %d" % (name, rc)
        return out


@pytest.fixture(scope="module")
def wg(native):
    import build_native
    from test_device_arith import Dev
    return DevWG(Dev(os.environ.get("BLS381_DEVCHECK_LIB") or build_native.build_devcheck()))


def _fill64(items):
    """Exactly one workgroup: the extremes first, 32 random ones last, the extremes again in between."""
    ext, rnd = items[:-32], items[-32:]
    assert len(ext) >= 1
    body = (ext * (32 // len(ext) + 1))[:32] if len(ext) < 32 else ext[:32]
    out = body + rnd
    assert len(out) == 64
    return out


def _fp2_items(nops, seed):
    rng = random.Random(seed)
    vals = [(x,) * (2 * nops) for x in EXT]
    for big in EXT[:3]:
        for j in range(2 * nops):
            vals.append(tuple(big if i == j else 0 for i in range(2 * nops)))
            vals.append(tuple(0 if i == j else big for i in range(2 * nops)))
    vals = vals[:32]
    for _ in range(32):
        vals.append(tuple(rng.choice(EXT) if rng.random() < 0.25 else rng.randrange(Q2) for _ in range(2 * nops)))
    return [[V.limbs(v) for v in it] for it in vals]


# probe, operands, aux per item, the host build's result for one item (ops = [[c0, c1], ...])
def _linear_probes(ch):
    neg = lambda a: [a[0], ch.fp(2, a[1])]
    return [
        ("P_ADD", 2, None, lambda x, aux: ch.add(x[0], x[1])),
        ("P_SUB", 2, None, lambda x, aux: ch.sub(x[0], x[1])),
        ("P_DBL", 1, None, lambda x, aux: ch.dbl(x[0])),
        ("P_CONJ", 1, None, lambda x, aux: neg(x[0])),
        ("P_MUL_XI", 1, None, lambda x, aux: ch.mul_xi(x[0])),
        ("P_ADD_MUL_XI", 2, None, lambda x, aux: ch.add_mul_xi(x[0], x[1])),
        ("P_SUB2", 3, None, lambda x, aux: ch.sub2(x[0], x[1], x[2])),
        ("P_3PM2", 2, lambda i: i & 1, lambda x, aux: [ch.fp(7 if aux else 8, x[0][p], x[1][p]) for p in (0, 1)]),
        ("P_MUL_SMALL", 1, lambda i: 1 + i % 8, lambda x, aux: [ch.fp(8 + aux, x[0][p]) for p in (0, 1)]),
    ]


@pytest.mark.gpu
def test_device_reduce_lc_forms_equal_the_host_build(wg, L):
    """fp_reduce_lc's two paths through the lane-pair probes (KMAX 2, 3, 5, 8 and the per-lane choice of
    fp2_mul_xi, fp2_add_mul_xi, fp2_conj): the host build's limbs on every lane of one workgroup."""
    from test_device_arith import pair_in, pair_out
    ch = Chain(L)
    for k, (name, nops, auxf, host) in enumerate(_linear_probes(ch)):
        items = _fill64(_fp2_items(nops, 9300 + k))
        aux = [auxf(i) for i in range(64)] if auxf else None
        out = wg.run(name, [pair_in(it) for it in items], aux)
        for i, it in enumerate(items):
            ops = [[it[2 * j], it[2 * j + 1]] for j in range(nops)]
            assert pair_out(out[i]) == [tuple(l) for l in host(ops, aux[i] if aux else 0)], (name, i)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_device_fused_forms_on_one_workgroup(wg, L, form):
    """The fused combinations (fp_reduce_lc's k <= 7 path under both lane parities) on 64 lane pairs."""
    from test_device_arith import pair_in, pair_out
    items = _fill64(cases(form))
    out = wg.run("P_" + form[0], [pair_in(it) for it in items])
    for i, it in enumerate(items):
        assert pair_out(out[i]) == host_form(L, form, it) == model(form, it), (form[0], i)


@pytest.mark.gpu
def test_device_compressed_squaring_on_one_workgroup(wg, L):
    """cyc_csqr_lazy (lz_mul, lz_xi_mul, lz_sqr_xisqr in column order, both lane parities) on 64 lane pairs."""
    from test_device_arith import pair_in, pair_out
    items = _fill64(csqr_items())
    out = wg.run("P_CSQR", [pair_in(it) for it in items], [1] * 64)
    for i, g in enumerate(items):
        assert pair_out(out[i]) == host_csqr(L, g), i
