"""Host (g++) build of the device arithmetic headers vs the oracle / model.

The same headers are compiled for gfx950 by hipcc; this suite checks every
layer of them in a container with no GPU.  libbls381_hostcheck.so is test
infrastructure (consensus-specs_amd/csrc/host_check.cpp), never the product.
"""
import ctypes
import hashlib
import os
import random

import pytest

import bls_oracle as O
import tower_model as M
from devcheck_vectors import csqr_expect_raw as _csqr_expect

q = O.q


@pytest.fixture(scope="module")
def L():
    import build_native
    return ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())


def b48(x): return x.to_bytes(48, "big")
def i48(b): return int.from_bytes(b, "big")
def b96(a): return b48(a[0]) + b48(a[1])
def i96(b): return (i48(b[:48]), i48(b[48:96]))
def b576(f): return b"".join(b96(c) for c in f)
def i576(b): return tuple(i96(b[96 * i:96 * i + 96]) for i in range(6))


def test_fp_ops(L):
    rng = random.Random(5)
    buf = ctypes.create_string_buffer(48)
    edge = [(q - 1, q - 1), (0, q - 1), (1, 1), (q - 1, 1), (0, 0), (2 ** 256, q - 2)]
    for i in range(400):
        a, b = edge[i] if i < len(edge) else (rng.randrange(q), rng.randrange(q))
        L.hc_fp_mul(b48(a), b48(b), buf); assert i48(buf.raw) == a * b % q
        L.hc_fp_add(b48(a), b48(b), buf); assert i48(buf.raw) == (a + b) % q
        L.hc_fp_sub(b48(a), b48(b), buf); assert i48(buf.raw) == (a - b) % q
        L.hc_fp_half(b48(a), buf); assert i48(buf.raw) * 2 % q == a
    # raw Montgomery product (R = 2^392): weakly reduced output < 2q, congruent
    R = 1 << 392
    Rinv = pow(R, -1, q)
    for i in range(200):
        a, b = (rng.randrange(q), rng.randrange(q)) if i > 1 else (q - 1, q - 1)
        L.hc_fp_mont_mul_raw(b48(a), b48(b), buf)
        v = i48(buf.raw)
        assert v < 2 * q and v % q == a * b * Rinv % q


def test_fp_one_reduction_combinations_raw(L):
    """fp_reduce_lc (one reduction per linear combination) on raw limbs: the result is the
    unique normalized value in [0, 2q) congruent to the combination mod 2q -- what the
    two-operand add/sub chains it replaces return -- including inputs whose top limb
    equals 2q's (the borrowed constants' top limb goes negative), and the rare lanes that
    need the second subtraction."""
    q2 = 2 * q
    top2 = q2 >> 364
    rng = random.Random(0x1C)
    edge = [0, 1, q - 1, q, q + 1, q2 - 1, q2 - 2, top2 << 364, (top2 << 364) - 1, (1 << 364) - 1,
            ((top2 - 1) << 364) + (1 << 363), q2 - (1 << 200)]
    vals = edge + [rng.randrange(q2) for _ in range(300)]
    # values just below multiples of 2q after combination: X near the 2q boundary
    vals += [q2 - rng.randrange(1, 1 << 40) for _ in range(60)] + [rng.randrange(1 << 40) for _ in range(20)]
    lim = lambda v: (ctypes.c_uint32 * 14)(*[(v >> (28 * i)) & ((1 << 28) - 1) for i in range(14)])
    out = (ctypes.c_uint32 * 14)()
    ops = {0: lambda a, b, c: a + b, 1: lambda a, b, c: a - b, 2: lambda a, b, c: -a, 3: lambda a, b, c: 2 * a,
           4: lambda a, b, c: a + b - c, 5: lambda a, b, c: a + b + c, 6: lambda a, b, c: a - b - c,
           7: lambda a, b, c: 3 * a - 2 * b, 8: lambda a, b, c: 3 * a + 2 * b}
    for k in range(1, 9):
        ops[8 + k] = (lambda kk: (lambda a, b, c: kk * a))(k)
    n = 0
    for i in range(900):
        if i < len(edge) ** 2:
            a, b = edge[i // len(edge)], edge[i % len(edge)]
            c = edge[(i * 7) % len(edge)]
        else:
            a, b, c = rng.choice(vals), rng.choice(vals), rng.choice(vals)
        for op, f in ops.items():
            L.hc_fp_lc_raw(op, lim(a), lim(b), lim(c), out)
            got = sum(int(out[j]) << (28 * j) for j in range(14))
            assert all(int(out[j]) < (1 << 28) for j in range(14)), (op, a, b, c)
            assert got == f(a, b, c) % q2, (op, hex(a), hex(b), hex(c))
            n += 1
    assert n == 900 * len(ops)


def test_fp_legendre(L):
    """Binary-Jacobi Legendre symbol == Euler's criterion (squares, non-squares, 0, edges)."""
    rng = random.Random(21)
    L.hc_fp_legendre.restype = ctypes.c_int
    vals = [0, 1, 2, 3, 4, q - 1, q - 2, (q - 1) // 2, 2 ** 255, 2 ** 380 + 5]
    vals += [rng.randrange(q) for _ in range(300)] + [rng.randrange(q) ** 2 % q for _ in range(50)]
    for a in vals:
        e = pow(a, (q - 1) // 2, q)
        want = 0 if a % q == 0 else (1 if e == 1 else -1)
        assert L.hc_fp_legendre(b48(a)) == want, hex(a)


def test_fp_mul_extreme_operands(L):
    """fp_mul accepts any operands with limbs < 2^28 and value < 2^384 (< 9.6q):
    output must stay < 2q and congruent (column sums stay < 2^64)."""
    rng = random.Random(15)
    buf = ctypes.create_string_buffer(48)
    Rinv = pow(1 << 392, -1, q)
    top = (1 << 384) - 1
    cases = [(top, top), (top, 0), (2 * q - 1, 2 * q - 1), (q, q), (top, 1)]
    cases += [(rng.randrange(1 << 384), rng.randrange(1 << 384)) for _ in range(300)]
    for a, b in cases:
        L.hc_fp_mont_mul_raw(b48(a), b48(b), buf)
        v = i48(buf.raw)
        assert v < 2 * q and v % q == a * b * Rinv % q


def test_fp_inv_sqrt(L):
    rng = random.Random(6)
    buf = ctypes.create_string_buffer(48)
    for _ in range(10):
        a = rng.randrange(1, q)
        L.hc_fp_inv(b48(a), buf); assert i48(buf.raw) * a % q == 1
        s = L.hc_fp_sqrt(b48(a), buf)
        r = i48(buf.raw)
        assert bool(s) == (pow(a, (q - 1) // 2, q) == 1)
        if s:
            assert r * r % q == a


def test_fp2(L):
    rng = random.Random(7)
    buf = ctypes.create_string_buffer(96)
    for i in range(60):
        a, b = (rng.randrange(q), rng.randrange(q)), (rng.randrange(q), rng.randrange(q))
        L.hc_fp2_mul(b96(a), b96(b), buf); assert i96(buf.raw) == M.mul2(a, b)
        L.hc_fp2_sqr(b96(a), buf); assert i96(buf.raw) == M.mul2(a, a)
        L.hc_fp2_inv(b96(a), buf); assert i96(buf.raw) == M.inv2(a)
    for i in range(60):
        v = (rng.randrange(q), rng.randrange(q)) if i % 4 else (rng.randrange(q), 0)
        if i == 1:
            v = (0, rng.randrange(q))
        s = L.hc_fp2_sqrt_select(b96(v), buf)
        e = O.modular_squareroot(v)
        assert (e is None) == (s == 0)
        if e is not None:
            assert i96(buf.raw) == e


def test_fp2_lazy_operands_at_bounds(L):
    """Fp2 mul with lazy operands: limbs < 2^29, values < 4q (sums of two
    weakly reduced < 2q values).  Output must be < 2q and congruent."""
    rng = random.Random(17)
    Rinv = pow(1 << 392, -1, q)
    out = ctypes.create_string_buffer(96)
    edge = [2 * q - 1, 2 * q - 2, q, q - 1, 0, (1 << 380)]
    pick = lambda i: edge[i % len(edge)] if i < 24 else rng.randrange(2 * q)
    for i in range(400):
        X = (pick(i), pick(i + 1)); Y = (pick(i + 2), pick(i + 3))
        Z = (pick(i + 4), pick(i + 5)); U = (pick(i + 6), pick(i + 7))
        L.hc_fp2_mul_lazy_raw(b96(X), b96(Y), b96(Z), b96(U), out)
        r0, r1 = i96(out.raw)
        a = ((X[0] + Y[0]) % q, (X[1] + Y[1]) % q)
        b = ((Z[0] + U[0]) % q, (Z[1] + U[1]) % q)
        e = M.mul2(a, b)
        assert r0 < 2 * q and r1 < 2 * q
        assert (r0 % q, r1 % q) == (e[0] * Rinv % q, e[1] * Rinv % q)


def test_cyc_csqr_lazy_at_bounds(L):
    """Lazily reduced Karabina squaring (one signed wide sum per output coefficient) with
    inputs at the representation's extremes: values up to 2q - 1, normalized limbs all
    2^28 - 1 where possible.  Outputs < 2q and congruent to the formulas."""
    rng = random.Random(23)
    Rinv = pow(1 << 392, -1, q)
    out = ctypes.create_string_buffer(384)
    allones = sum((2**28 - 1) << (28 * k) for k in range(13)) + (((2 * q - 1) >> 364) << 364)
    allones = min(allones, 2 * q - 1)
    edge = [2 * q - 1, 2 * q - 2, q, q - 1, 0, 1, allones, (1 << 380) - 1]
    for i in range(600):
        if i < 256:
            vals = [edge[(i >> (k % 8)) % len(edge)] if (i + k) % 3 else edge[(i * 7 + k) % len(edge)] for k in range(8)]
        else:
            vals = [rng.choice(edge) if rng.random() < 0.3 else rng.randrange(2 * q) for _ in range(8)]
        g = tuple((vals[2 * j], vals[2 * j + 1]) for j in range(4))
        L.hc_cyc_csqr_raw(b"".join(b96(x) for x in g), out)
        got = [i96(out.raw[96 * j:96 * j + 96]) for j in range(4)]
        for j, e in enumerate(_csqr_expect(g, Rinv)):
            assert got[j][0] < 2 * q and got[j][1] < 2 * q, (i, j)
            assert (got[j][0] % q, got[j][1] % q) == e, (i, j)


def test_fp12(L):
    rng = random.Random(8)
    buf = ctypes.create_string_buffer(576)
    r2 = lambda: (rng.randrange(q), rng.randrange(q))
    f = tuple(r2() for _ in range(6))
    g = tuple(r2() for _ in range(6))
    L.hc_fp12_mul(b576(f), b576(g), buf); assert i576(buf.raw) == M.mul12(f, g)
    L.hc_fp12_sqr(b576(f), buf); assert i576(buf.raw) == M.mul12(f, f)
    L.hc_fp12_inv(b576(f), buf); assert i576(buf.raw) == M.inv12(f)
    for p in (1, 2, 3):
        L.hc_fp12_frob(b576(f), p, buf); assert i576(buf.raw) == M.frob12(f, p)
    t = M.mul12(M.conj12(f), M.inv12(f))
    t = M.mul12(M.frob12(t, 2), t)
    L.hc_fp12_cyc_sqr(b576(t), buf); assert i576(buf.raw) == M.mul12(t, t)
    c = [r2() for _ in range(3)]
    L.hc_fp12_mul_by_line(b576(f), b96(c[0]), b96(c[1]), b96(c[2]), buf)
    assert i576(buf.raw) == M.mul12(f, (c[0], c[1], M.ZERO2, M.ZERO2, c[2], M.ZERO2))
    L.hc_final_exp(b576(f), buf); assert i576(buf.raw) == M.final_exp(f)
    # f = 1 (the infinity/infinity verify): every compressed snapshot has g2 = 0, so the
    # exponentiations by x take the exact Granger-Scott fallback
    L.hc_final_exp(b576(M.ONE12), buf); assert i576(buf.raw) == M.ONE12
    # an element of Fp6 (b = 0): the easy part maps it to 1 as well
    g6 = f[:3] + (M.ZERO2,) * 3
    L.hc_final_exp(b576(g6), buf); assert i576(buf.raw) == M.final_exp(g6) == M.ONE12
    # the verdict form: c == conj(t^3) instead of the last product; without the fallback
    # (fb = 0, the throughput kernel) a g2 = 0 snapshot reports 2 (k_final_exp_redo's items)
    fr = M.ONE12
    for bit in bin(O.r)[2:]:                 # f^r: its final exponentiation is 1
        fr = M.mul12(fr, fr)
        if bit == "1":
            fr = M.mul12(fr, f)
    for x, want in ((f, 0), (fr, 1)):
        assert L.hc_final_exp_check(b576(x), 1) == L.hc_final_exp_check(b576(x), 0) == want
    for x in (M.ONE12, g6):
        assert L.hc_final_exp_check(b576(x), 1) == 1 and L.hc_final_exp_check(b576(x), 0) == 2


def test_codecs_and_subgroups(L, golden):
    vec, gb = golden
    buf = ctypes.create_string_buffer(192)
    for c in vec["priv_to_pub"]:
        pk = bytes.fromhex(c["output"][2:])
        assert L.hc_g1_decompress(pk, buf, 1) == 0
        assert O.pubkey_to_G1(pk) == (i48(buf.raw[:48]), i48(buf.raw[48:96]), 1)
        out = ctypes.create_string_buffer(48)
        L.hc_g1_compress_aff(buf.raw[:96], out)
        assert out.raw == pk
        assert L.hc_g1_in_subgroup(buf.raw[:96]) == 1
    for c in vec["sign_msg"][::5]:
        sig = bytes.fromhex(c["output"][2:])
        assert L.hc_g2_decompress(sig, buf, 1) == 0
        a = O.signature_to_G2(sig)
        assert (i96(buf.raw[:96]), i96(buf.raw[96:192])) == (a[0], a[1])
        out = ctypes.create_string_buffer(96)
        L.hc_g2_compress_aff(buf.raw, out)
        assert out.raw == sig
        assert L.hc_g2_in_subgroup(buf.raw) == 1
    for lax in (0, 1):
        for h in gb["invalid_g1"]:
            assert L.hc_g1_decompress(bytes.fromhex(h), buf, lax) == 2
        for h in gb["invalid_g2"]:
            assert L.hc_g2_decompress(bytes.fromhex(h), buf, lax) == 2
        assert L.hc_g1_decompress(bytes([0xC0]) + b"\x00" * 47, buf, lax) == 1
        assert L.hc_g2_decompress(bytes([0xC0]) + b"\x00" * 95, buf, lax) == 1
    # b_flag with x = q: the strict codec's infinity needs x == 0 exactly (not x == 0 mod q)
    xq = bytearray(O.q.to_bytes(48, "big")); xq[0] |= 0xC0
    assert L.hc_g1_decompress(bytes(xq), buf, 0) == 2 and L.hc_g1_decompress(bytes(xq), buf, 1) == 1
    s = M.sqrt_fp((5 ** 3 + 4) % q)
    assert L.hc_g1_in_subgroup(b48(5) + b48(s)) == 0
    x, y = M.map_candidate(b"\x11" * 32, b"\x00" * 8)
    assert L.hc_g2_in_subgroup(b96(x) + b96(y)) == 0


def test_sha256_any_length(L):
    rng = random.Random(9)
    out = ctypes.create_string_buffer(32)
    for n in (0, 1, 41, 55, 56, 63, 64, 65, 119, 200, 256):
        m = bytes(rng.getrandbits(8) for _ in range(n))
        L.hc_sha256(m, n, out)
        assert out.raw == hashlib.sha256(m).digest()


def test_hash_to_g2_vectors(L, golden):
    vec, gb = golden
    aff = ctypes.create_string_buffer(192)
    comp = ctypes.create_string_buffer(96)
    for c in vec["msg_hash_g2_compressed"]:
        m = bytes.fromhex(c["input"]["message"][2:])
        d = int(c["input"]["domain"], 16).to_bytes(8, "big")
        assert L.hc_hash_to_g2(m, 32, d, aff, comp) > 0
        assert comp.raw.hex() == c["output"][0][2:] + c["output"][1][2:]
    for c in gb["hash_to_g2"]:
        m, d = bytes.fromhex(c["message"]), int(c["domain"]).to_bytes(8, "big")
        assert L.hc_hash_to_g2(m, 32, d, aff, comp) == c["trials"]
        assert comp.raw.hex() == c["compressed"]
    m = b"variable length message"
    assert L.hc_hash_to_g2(m, len(m), b"\x00" * 8, aff, comp) > 0
    assert comp.raw == O.G2_to_signature(O.hash_to_G2(m, 0))


def test_miller_loop_and_verify_equation(L):
    rng = random.Random(10)
    buf = ctypes.create_string_buffer(576)
    fo = ctypes.create_string_buffer(576)
    sk = rng.randrange(1, O.r)
    msg, dom = bytes(range(32)), 9
    pk = O.pubkey_to_G1(O.privtopub(sk))
    sa = O.g2_affine(O.signature_to_G2(O.sign(msg, sk, dom)))
    H = O.g2_affine(O.hash_to_G2(msg, dom))
    ng = (O.g_x, (-O.g_y) % q)
    Q = b96(sa[0]) + b96(sa[1]) + b96(H[0]) + b96(H[1])
    P = b48(ng[0]) + b48(ng[1]) + b48(pk[0]) + b48(pk[1])
    L.hc_miller_loop(2, Q, P, buf)
    assert i576(buf.raw) == M.miller_loop_multi([(sa, ng), (H, (pk[0], pk[1]))])
    L.hc_final_exp(buf.raw, fo)
    assert i576(fo.raw) == M.ONE12
    # wrong public key -> not one
    pk2 = O.pubkey_to_G1(O.privtopub(sk + 1))
    P2 = b48(ng[0]) + b48(ng[1]) + b48(pk2[0]) + b48(pk2[1])
    L.hc_miller_loop(2, Q, P2, buf)
    L.hc_final_exp(buf.raw, fo)
    assert i576(fo.raw) != M.ONE12
    # single-pair loop matches the model too
    L.hc_miller_loop(1, Q[:192], P[:96], buf)
    assert i576(buf.raw) == M.miller_loop_multi([(sa, ng)])


def test_scalar_mul_fixture_helpers(L):
    out = ctypes.create_string_buffer(48)
    k = 0x263dbd792f5b1be47ed85f8938c0f29586af0d3ac7b977f21c278fe1462040e3
    limbs = (ctypes.c_uint32 * 8)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(8)])
    L.hc_g1_mul(b48(O.g_x) + b48(O.g_y), limbs, 256, out)
    assert out.raw == O.privtopub(k)


def test_fp_inv_binary_gcd_edges(L):
    """fp_inv (Pornin's optimized binary GCD on the Montgomery integer) and its fallback
    fp_inv_xgcd: random values, Montgomery integers with long runs of factors of two, small,
    near q, near powers of two, all-ones patterns; 0 -> 0.  The fast path must finish every
    one of them (no fallback taken)."""
    R = 1 << 392
    rinv = pow(R, -1, q)
    rng = random.Random(61)
    buf = ctypes.create_string_buffer(48)
    L.hc_inv_fallbacks.restype = ctypes.c_uint64
    before = L.hc_inv_fallbacks()
    vals = [1, 2, q - 1, q - 2, (q + 1) // 2, 3]
    mont = [1 << k for k in range(381)] + [q - (1 << k) for k in range(381)]
    mont += [(1 << k) - 1 for k in range(2, 382)] + [(1 << k) + 1 for k in range(2, 381)]
    mont += list(range(1, 300)) + [q - k for k in range(1, 300)] + [q // 3, q // 5, (q - 1) // 2]
    mont += [rng.randrange(1, 1 << rng.randrange(2, 381)) for _ in range(3000)]
    # common length <= 62 from the start (the exact-approximation branch, t == 2)
    mont += [rng.randrange(1 << 59, 1 << 62) for _ in range(2000)] + [(1 << 61) | rng.getrandbits(60) for _ in range(500)]
    vals += [(m % q) * rinv % q for m in mont if m % q]
    vals += [rng.randrange(1, q) for _ in range(6000)]
    for a in vals:
        L.hc_fp_inv(b48(a), buf)
        assert i48(buf.raw) * a % q == 1, a
    for a in vals[:300]:
        L.hc_fp_inv_xgcd(b48(a), buf)
        assert i48(buf.raw) * a % q == 1, a
    assert L.hc_inv_fallbacks() == before
    L.hc_fp_inv(b48(0), buf)
    assert i48(buf.raw) == 0
