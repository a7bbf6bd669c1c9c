"""The fused tower combinations (fp_lc and the fp2_* forms built on it, bls381_field.hpp / bls381_pair.hpp).

Each form adds and subtracts normalized values in one limb sum and reduces once (fp_reduce_lc).  What
can go wrong is the sum leaving fp_reduce_lc's contract: a limb past 2^31 - 8, a top limb below -2, a
value past KMAX 2q with KMAX <= 8, or an offset that is no multiple of 2q or does not dominate the
subtracted limbs.  `model` below is the limb sum on Python integers, asserting that contract at every
call and walking fp_reduce_lc's own steps; its result is the unique representative in [0, 2q), so the
host build, the chain of two-operand forms it replaces and the lane-pair probes must all return the
same 14 limbs.  Operands: every limb 2^28 - 1, values 2q - 1, zero, q, each coefficient's subtracted
terms at their maximum with its added terms at zero and the reverse, and 32 seeded random values.
"""
import ctypes
import os
import random

import pytest

import bls_oracle as O
import devcheck_vectors as V
import tower_model as M
from test_leaf_columns import _const

q = O.q
Q2, MASK = V.Q2, V.MASK
AO = (((Q2 >> 364) - 1) << 364) + (1 << 364) - 1    # limbs 0..12 all 2^28 - 1, the largest such value < 2q
Q2_LIMBS = _const("Q2_LIMBS")
LC_DIV_MAGIC = _const("LC_DIV_MAGIC")[0]
# offset and its value in units of 2q, by the number of subtracted values
OFFSET = {2: (_const("Q4B_LIMBS"), 2), 3: (_const("Q8T_LIMBS"), 4), 4: (_const("Q10F_LIMBS"), 5)}

# name, host op = order, operands, then per output coefficient (added, subtracted) slots; a slot is
# (operand, coefficient), repeated for a multiple
A0, A1, B0, B1, C0, C1, D0, D1 = [(j, p) for j in range(4) for p in range(2)]
FORMS = [
    # a + xi (m - b - c): operands a, m, b, c
    ("ADD_XI_SUB2", 4, [([A0, B0, C1, D1], [C0, D0, B1]), ([A1, B0, B1], [C0, C1, D0, D1])]),
    # (m - a - b) + xi c: operands m, a, b, c
    ("SUB2_ADD_XI", 4, [([A0, D0], [B0, C0, D1]), ([A1, D0, D1], [B1, C1])]),
    # m - a - b + c
    ("SUB2_ADD", 4, [([A0, D0], [B0, C0]), ([A1, D1], [B1, C1])]),
    # t - a - xi b: operands t, a, b
    ("SUB_SUB_XI", 3, [([A0, C1], [B0, C0]), ([A1], [B1, C0, C1])]),
    # x - y - 2z
    ("SUB_SUB_DBL", 3, [([A0], [B0, C0, C0]), ([A1], [B1, C1, C1])]),
    # 2 (x - y - z)
    ("DBL_SUB2", 3, [([A0, A0], [B0, B0, C0, C0]), ([A1, A1], [B1, B1, C1, C1])]),
    # 3a + xi b - 2c
    ("3A_XI_B_M2C", 3, [([A0, A0, A0, B0], [B1, C0, C0]), ([A1, A1, A1, B0, B1], [C1, C1])]),
    # 2a + b - 3c
    ("2A_B_M3C", 3, [([A0, A0, B0], [C0, C0, C0]), ([A1, A1, B1], [C1, C1, C1])]),
]


def test_constants():
    assert V.value(Q2_LIMBS) == Q2 and LC_DIV_MAGIC == -(-(1 << 40) // (Q2_LIMBS[13] + 1))
    for ns, (off, units) in OFFSET.items():
        assert V.value(off) == units * Q2                          # a multiple of 2q
        assert all(ns * MASK <= x <= (ns + 1) * MASK for x in off[:13])   # dominates ns normalized limbs
        assert off[13] >= ns * Q2_LIMBS[13] - 2                    # the top limb stays >= -2


def reduce_lc(s, kmax):
    """fp_reduce_lc<kmax> step by step, with its contract and the ranges its int32 arithmetic needs."""
    assert 1 <= kmax <= 8
    assert all(0 <= x <= (1 << 31) - 8 for x in s[:13]) and -2 <= s[13] < 1 << 31, s
    val = V.value(s)
    assert 0 <= val < kmax * Q2, (val // Q2, kmax)
    if kmax <= 2:
        k = 1 if s[13] > Q2_LIMBS[13] else 0
    else:
        top = max(s[13], 0)
        assert top < 1 << 22
        k = (top * LC_DIV_MAGIC) >> 40
    assert k <= 7 and val // Q2 - 1 <= k <= val // Q2
    t = [x - k * y for x, y in zip(s, Q2_LIMBS)]
    assert all(-(1 << 31) <= x < 1 << 31 for x in t)
    for i in range(13):
        t[i + 1] += t[i] >> 28
        t[i] &= MASK
    assert 0 <= t[13] and V.value(t) == val - k * Q2 < 2 * Q2
    if V.value(t) >= Q2:
        assert t[13] >= Q2_LIMBS[13]      # the branch that subtracts is taken
        t = list(V.limbs(V.value(t) - Q2))
    assert tuple(t) == V.limbs(val % Q2)
    return tuple(t)


def model(form, item):
    """Both coefficients of a fused form: item = raw Fp (operand 0 c0, operand 0 c1, operand 1 c0, ...)."""
    out = []
    for add, sub in form[2]:
        off, units = OFFSET[len(sub)]
        assert len(add) + len(sub) <= 7
        s = [off[i] + sum(item[2 * j + p][i] for j, p in add) - sum(item[2 * j + p][i] for j, p in sub) for i in range(14)]
        out.append(reduce_lc(s, len(add) + units))
        assert V.value(out[-1]) == (sum(V.value(item[2 * j + p]) for j, p in add)
                                    - sum(V.value(item[2 * j + p]) for j, p in sub)) % Q2
    return out


def cases(form):
    """The operand extremes of one form, then 32 seeded random items."""
    _, nops, coeffs = form
    n = 2 * nops
    ext = [V.limbs(AO), V.limbs(Q2 - 1), V.limbs(0), V.limbs(q)]
    assert all(x == MASK for x in ext[0][:13])
    items = [[x] * n for x in ext]
    for add, sub in coeffs:
        for big in ext[:2]:
            for at_max in (set(sub) - set(add), set(add) - set(sub)):
                items.append([big if (j, p) in at_max else ext[2] for j in range(nops) for p in range(2)])
    rng = random.Random(8100 + FORMS.index(form))
    edge = [Q2 - 1, AO, q, 0, 1]
    for _ in range(32):
        items.append([V.limbs(rng.choice(edge) if rng.random() < 0.25 else rng.randrange(Q2)) for _ in range(n)])
    assert all(V.is_normalised(l) for it in items for l in it)
    return items


def test_models_hold_the_reduction_contract():
    for form in FORMS:
        tops, lows = [], []
        for it in cases(form):
            got = model(form, it)
            assert all(V.is_normalised(l) for l in got)
            for add, sub in form[2]:
                off = OFFSET[len(sub)][0]
                s = [off[i] + sum(it[2 * j + p][i] for j, p in add) - sum(it[2 * j + p][i] for j, p in sub) for i in range(14)]
                tops.append(max(s[:13]))
                lows.append(s[13])
        assert max(tops) <= (1 << 31) - 8 and min(lows) >= -2
        if form[0] == "ADD_XI_SUB2":    # seven terms and the offset's own limb: the bound is approached
            assert max(tops) > 7 * MASK


# ---------------------------------------------------------------- host build --
@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_raw_fp2_lc.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_raw_tower.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_raw_fp12.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_fp_lc_raw.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4
    return lib


def _host(fn, op, item, nout, *aux):
    flat = [w for l in item for w in l]
    buf, out = (ctypes.c_uint32 * len(flat))(*flat), (ctypes.c_uint32 * (14 * nout))()
    rc = fn(op, buf, *aux, out)
    assert rc >= 0
    return [tuple(out[14 * j:14 * j + 14]) for j in range(nout)]


def host_form(L, form, item):
    return _host(L.hc_raw_fp2_lc, FORMS.index(form), item, 2)


def test_host_forms_equal_the_model(L):
    for form in FORMS:
        for i, it in enumerate(cases(form)):
            assert host_form(L, form, it) == model(form, it), (form[0], i)


class Chain:
    """The two-operand and three-operand forms the fused ones replace, through hc_fp_lc_raw."""

    def __init__(self, L):
        self.L = L

    def fp(self, op, x, y=None, z=None):
        a = [(ctypes.c_uint32 * 14)(*(v if v is not None else [0] * 14)) for v in (x, y, z)]
        o = (ctypes.c_uint32 * 14)()
        self.L.hc_fp_lc_raw(op, a[0], a[1], a[2], o)
        return tuple(o)

    def add(self, a, b): return [self.fp(0, a[0], b[0]), self.fp(0, a[1], b[1])]
    def sub(self, a, b): return [self.fp(1, a[0], b[0]), self.fp(1, a[1], b[1])]
    def dbl(self, a): return [self.fp(3, a[0]), self.fp(3, a[1])]
    def sub2(self, a, b, c): return [self.fp(6, a[0], b[0], c[0]), self.fp(6, a[1], b[1], c[1])]
    def mul3(self, a): return [self.fp(11, a[0]), self.fp(11, a[1])]
    def mul_xi(self, a): return [self.fp(1, a[0], a[1]), self.fp(0, a[0], a[1])]
    def add_mul_xi(self, a, b): return [self.fp(4, a[0], b[0], b[1]), self.fp(5, a[1], b[0], b[1])]

    def run(self, name, x):
        if name == "ADD_XI_SUB2": return self.add_mul_xi(x[0], self.sub2(x[1], x[2], x[3]))
        if name == "SUB2_ADD_XI": return self.add_mul_xi(self.sub2(x[0], x[1], x[2]), x[3])
        if name == "SUB2_ADD": return self.add(self.sub2(x[0], x[1], x[2]), x[3])
        if name == "SUB_SUB_XI": return self.sub2(x[0], x[1], self.mul_xi(x[2]))
        if name == "SUB_SUB_DBL": return self.sub2(x[0], x[1], self.dbl(x[2]))
        if name == "DBL_SUB2": return self.dbl(self.sub2(x[0], x[1], x[2]))
        if name == "3A_XI_B_M2C": return self.sub2(self.add_mul_xi(self.mul3(x[0]), x[1]), x[2], x[2])
        assert name == "2A_B_M3C"
        return self.sub(self.add(self.dbl(x[0]), x[1]), self.mul3(x[2]))


def test_host_forms_equal_the_chains_they_replace(L):
    ch = Chain(L)
    for form in FORMS:
        for i, it in enumerate(cases(form)):
            ops = [[it[2 * j], it[2 * j + 1]] for j in range(form[1])]
            assert host_form(L, form, it) == ch.run(form[0], ops), (form[0], i)


def test_host_tower_against_the_model(L):
    """fp6_mul, fp12_sqr, f (l l') and cyc_decompress of the host build against oracle/tower_model.py,
    on edge-value and random coefficients."""
    rng = random.Random(8200)
    d6 = lambda fps: tuple(V.dec2(fps))
    items, _ = V._fp12_items(rng, 24, 1, 12)
    for it in items:       # an Fp12's 12 raw Fp = two Fp6 operands
        got = _host(L.hc_raw_tower, 0, it, 6)
        V.check_fps(got, V._flat(M.mul6(d6(it[:6]), d6(it[6:]))), Q2, "fp6_mul")
        got = _host(L.hc_raw_fp12, 1, it, 12, 0)
        V.check_fps(got, V._flat(M.sqr12(d6(it))), Q2, "fp12_sqr")
    vals, _ = V.edge_values(rng, 24, 24, 12)
    for v in vals:         # f, then the lines (c0, c1, c2) and (d0, d1, d2)
        it = [V.limbs(x) for x in v]
        c, d = V.dec2(it[12:18]), V.dec2(it[18:])
        line = lambda e: (e[0], e[1], M.ZERO2, M.ZERO2, e[2], M.ZERO2)
        LL = M.mul12(line(c), line(d))
        V.check_fps(_host(L.hc_raw_tower, 2, it[12:], 12), V._flat(LL), Q2, "line_pair_product")
        V.check_fps(_host(L.hc_raw_tower, 1, it, 12), V._flat(M.mul12(d6(it[:12]), LL)), Q2, "fp12_mul_by_line_pair")
    c = V.decompress()
    for it in c.items:
        V.check_fps(_host(L.hc_raw_fp12, 9, it, 12, 0), c.expect(it, 0), Q2, "cyc_decompress")


# -------------------------------------------------------------------- device --
@pytest.fixture(scope="module")
def dev(native):
    import build_native
    from test_device_arith import Dev
    return Dev(os.environ.get("BLS381_DEVCHECK_LIB") or build_native.build_devcheck())


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_device_pair_forms_equal_the_host_build(dev, L, form):
    """The lane-pair form, one wave (32 lane pairs) per launch: the host build's limbs, and the model's."""
    from test_device_arith import pair_in, pair_out
    items = cases(form)
    for i0 in range(0, len(items), 32):
        chunk = items[i0:i0 + 32]
        out, _ = dev.run("P_" + form[0], [pair_in(it) for it in chunk])
        for i, it in enumerate(chunk):
            assert pair_out(out[i]) == host_form(L, form, it) == model(form, it), (form[0], i0 + i)
