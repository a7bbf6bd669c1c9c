"""The column-order Montgomery products (fp_mont_columns: fp_mul_body, fp_sqr_body, fp2p_mul_body) at
the extremes of their operand bounds.

A column's accumulator starts as the carry of the column before it and takes every product of the
column, so what can go wrong is a column sum passing 2^64.  `mont_columns` below is that accumulation
order on Python integers, asserting the bound at every step; the product it returns is exact
((T + sum m_i q 2^(28 i)) / R does not depend on the order), so the host build and the device probes
must return the same limbs.  Operands: every limb 2^29 - 2, values 4q - 2, zero, q, the terms of one
lane at their maximum with the other lane's at zero, and 32 seeded random lazy sums; for the one-lane
fp_mul the sums of two lazy sums Karatsuba feeds it (limbs to 2^30 - 4).
"""
import ctypes
import os
import random
import re

import pytest

import bls_oracle as O
import devcheck_vectors as V
import tower_model as M

q = O.q
MASK = V.MASK
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(name):
    src = open(os.path.join(ROOT, "consensus-specs_amd", "csrc", "bls381_consts.hpp")).read()
    body = re.search(r"\b%s(?:\[\d+\])? = \{?([^;]*?)\}?;" % name, src).group(1)
    return [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-f]+u?", body)]


Q_LIMBS = _const("Q_LIMBS")
Q8S_LIMBS = _const("Q8S_LIMBS")
Q_INV28 = _const("Q_INV28")[0]


def test_constants():
    assert tuple(Q_LIMBS) == V.limbs(q) and (q * Q_INV28 + 1) % (1 << 28) == 0
    assert V.value(Q8S_LIMBS) == 8 * q and min(Q8S_LIMBS[:13]) >= (1 << 29) - 2


def mont_columns(terms, bound):
    """fp_mont_columns: terms[k] = the (x, y) factor pairs of column k.  Returns the 14 result limbs
    and the largest accumulator seen, which stays below 2^bound."""
    m, r, c, top = [], [], 0, 0
    for k in range(27):
        acc = c
        for x, y in terms[k]:
            assert 0 <= x < 1 << 32 and 0 <= y < 1 << 32
            acc += x * y
            top = max(top, acc)
        for i in range(max(0, k - 13), min(k, 14)):
            acc += m[i] * Q_LIMBS[k - i]
            top = max(top, acc)
        if k < 14:
            m.append(((acc & 0xFFFFFFFF) * Q_INV28) & MASK)
            acc += m[k] * Q_LIMBS[0]
            top = max(top, acc)
            assert acc & MASK == 0
        else:
            r.append(acc & MASK)
        c = acc >> 28
    assert top < 2 ** bound, (top.bit_length(), bound)
    assert c < 1 << 28     # the top limb is the last carry
    return tuple(r + [c]), top


def _cols(*pairs):
    """Column terms of sum_p a_p b_p for operand limb vectors (a_p, b_p)."""
    return [[(a[i], b[k - i]) for a, b in pairs for i in range(max(0, k - 13), min(k, 13) + 1)] for k in range(27)]


def model_fp_mul(a, b):
    return mont_columns(_cols((a, b)), 64)


def model_fp_sqr(a):
    a2 = [2 * x for x in a]
    terms = []
    for k in range(27):
        t = [(a2[i], a[k - i]) for i in range(max(0, k - 13), 14) if 2 * i < k]
        if k % 2 == 0:
            t.append((a[k // 2], a[k // 2]))
        terms.append(t)
    return mont_columns(terms, 64)


def model_fp2p_mul(a0, a1, b0, b1):
    """Both lanes of fp2p_mul_body: lane 0 a0 b0 + a1 (8q - b1), lane 1 a1 b0 + a0 b1."""
    w = [s - x for s, x in zip(Q8S_LIMBS, b1)]
    assert min(w) >= 0
    # in the loop's order: own a with b0, then the partner's a with w
    lane = lambda own, other, ww: [[t for i in range(max(0, k - 13), min(k, 13) + 1)
                                    for t in ((own[i], b0[k - i]), (other[i], ww[k - i]))] for k in range(27)]
    (r0, t0), (r1, t1) = mont_columns(lane(a0, a1, w), 63.5), mont_columns(lane(a1, a0, b1), 63.5)
    return [r0, r1], max(t0, t1)


def model_fp2p_sqr(a0, a1):
    """fp2p_sqr_body: lane 0 (a1 + a0)(a0 + 8q - a1), lane 1 (a0 + a0) a1, through fp_mul_body."""
    x0 = [u + v for u, v in zip(a1, a0)]
    y0 = [u + s - v for u, s, v in zip(a0, Q8S_LIMBS, a1)]
    (r0, t0), (r1, t1) = model_fp_mul(x0, y0), model_fp_mul([2 * u for u in a0], a1)
    return [r0, r1], max(t0, t1)


# ------------------------------------------------------------------ operands --
AO = (((V.Q2 >> 364) - 1) << 364) + (1 << 364) - 1    # limbs 0..12 all 2^28 - 1, the largest such value < 2q
A = V.lazy(AO, AO)                      # every limb 2^29 - 2 (the top one as far as 4q allows)
B = V.lazy(V.Q2 - 1, V.Q2 - 1)          # value 4q - 2
Z = V.limbs(0)
QL = V.limbs(q)


def mul_cases():
    rng = random.Random(7001)
    items = [[A] * 4, [B] * 4, [Z] * 4, [QL] * 4,
             [A, A, A, Z], [B, B, B, Z],     # lane 0 at its maximum: w = 8q - 0
             [A, Z, Z, A], [Z, A, A, Z], [A, Z, A, Z], [Z, A, Z, A],   # one lane's terms only
             [A, B, B, A], [B, A, A, B], [A, A, B, B], [QL, Z, A, B], [A, B, QL, QL], [Z, Z, A, A]]
    edge = [V.Q2 - 1, AO, q, 0, 1]
    for _ in range(32):
        v = [rng.choice(edge) if rng.random() < 0.25 else rng.randrange(V.Q2) for _ in range(8)]
        items.append([V.lazy(v[2 * j], v[2 * j + 1]) for j in range(4)])
    exp = lambda it, aux: V._flat([M.mul2(*V.dec2(it))])
    return V.Cases("leaf_mul_extremes", items, [0] * len(items), exp, 16, pre=V.is_lazy)


def sqr_cases():
    rng = random.Random(7002)
    ext = [V.limbs(AO), V.limbs(V.Q2 - 1), Z, QL]
    items = [[x, y] for x in ext for y in ext]
    items += [[V.limbs(rng.randrange(V.Q2)), V.limbs(rng.randrange(V.Q2))] for _ in range(32)]
    exp = lambda it, aux: V._flat([M.mul2(V.dec2(it)[0], V.dec2(it)[0])])
    return V.Cases("leaf_sqr_extremes", items, [0] * len(items), exp, 16)


def test_the_extremes_are_there_and_the_columns_hold():
    c = mul_cases()
    V.assert_operands(c)
    assert len(c) <= 64 and len(sqr_cases()) <= 64
    assert max(max(l) for it in c.items for l in it) == (1 << 29) - 2
    assert all(x == (1 << 29) - 2 for x in A[:13]) and V.value(B) == 4 * q - 2
    tops = []
    for it in c.items:
        got, top = model_fp2p_mul(*it)
        tops.append(top)
        V.check_fps(got, c.expect(it, 0), c.bound, (c.name, "model"))
    # the worst case is lane 0's with w = 8q - 0: column 12 alone holds 13 full products of each kind
    full = (1 << 29) - 2
    assert 13 * (full * full + full * min(Q8S_LIMBS[:13])) < max(tops) < 2 ** 63.5 and tops.index(max(tops)) == 4
    for it in sqr_cases().items:
        got, _ = model_fp2p_sqr(*it)
        V.check_fps(got, V._flat([M.mul2(V.dec2(it)[0], V.dec2(it)[0])]), V.Q2, "sqr model")


# ---------------------------------------------------------------- host build --
@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_raw_fp2.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_raw_fp.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _host_fp(L, op, *ops):
    flat = [w for l in ops for w in l]
    buf, out = (ctypes.c_uint32 * len(flat))(*flat), (ctypes.c_uint32 * 14)()
    L.hc_raw_fp(op, buf, out)
    return tuple(out)


def test_host_fp_products_equal_the_column_model(L):
    """fp_mul_body / fp_sqr_body limb for limb, at Karatsuba's operands (a0 + a1)(b0 + b1) of lazy
    sums: limbs to 2^30 - 4, values to 8q - 4 (the products of fp2_mul in the host build)."""
    dbl = lambda x, y: tuple(u + v for u, v in zip(x, y))
    big = [dbl(A, A), dbl(B, B), dbl(A, B), A, B, Z, QL, V.limbs(V.Q2 - 1), V.limbs(AO)]
    assert max(dbl(A, A)) == (1 << 30) - 4 and V.value(dbl(B, B)) == 8 * q - 4
    rng = random.Random(7003)
    pairs = [(x, y) for x in big for y in big]
    pairs += [(V.lazy(rng.randrange(V.Q2), rng.randrange(V.Q2)), V.lazy(rng.randrange(V.Q2), rng.randrange(V.Q2)))
              for _ in range(32)]
    for x, y in pairs:
        want, _ = model_fp_mul(x, y)
        assert V.is_normalised(want) and V.dec(want) == V.dec(x) * V.dec(y) % q
        assert _host_fp(L, 0, x, y) == want
    for x in [A, B, Z, QL, V.limbs(V.Q2 - 1), V.limbs(AO)] + [p[0] for p in pairs[-32:]]:
        want, _ = model_fp_sqr(x)     # fp_sqr's operand: limbs < 2^29 (doubled in the multiplier)
        assert V.is_normalised(want) and V.dec(want) == V.dec(x) ** 2 % q
        assert _host_fp(L, 1, x) == want == model_fp_mul(x, x)[0]


def test_host_fp2_products_at_the_extremes(L):
    from test_devcheck_vectors import host_check
    host_check(L.hc_raw_fp2, 0, mul_cases(), 2)
    host_check(L.hc_raw_fp2, 1, sqr_cases(), 2)


# -------------------------------------------------------------------- device --
@pytest.fixture(scope="module")
def dev(native):
    import build_native
    from test_device_arith import Dev
    return Dev(os.environ.get("BLS381_DEVCHECK_LIB") or build_native.build_devcheck())


@pytest.mark.gpu
def test_device_fp2_products_equal_the_column_model(dev):
    """P_MUL (fp2p_mul_call) and P_SQR (fp2p_sqr_call -> fp_mul_body): the model's value, and the
    model's limbs."""
    from test_device_arith import pair_in, pair_out, run_cases
    for name, c, model in (("P_MUL", mul_cases(), model_fp2p_mul), ("P_SQR", sqr_cases(), model_fp2p_sqr)):
        out, _ = run_cases(dev, name, c, pair_in, pair_out)
        for i, it in enumerate(c.items):
            assert pair_out(out[i]) == model(*it)[0], (name, i)
