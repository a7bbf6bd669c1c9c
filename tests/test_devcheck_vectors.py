"""The device check vectors (tests/devcheck_vectors.py) proven on the CPU.

Every generator's operands satisfy the precondition it claims, and wherever the host build of the
same headers has an equivalent one-lane form (libbls381_hostcheck.so, hc_raw_*), that form meets
the same expectation on the same operands -- so a mismatch in tests/test_device_arith.py is the
device form's.  Also the static checks of lib/libbls381_devcheck.so.  No GPU.
"""
import ctypes
import os

import pytest

import bls_oracle as O
import devcheck_vectors as V
import tower_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    for f in (lib.hc_raw_fp2, lib.hc_raw_fp12, lib.hc_raw_g2):
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_raw_miller.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def host_run(fn, op, item, aux, nout):
    """One item through a hc_raw_* export: raw Fp in, (nout raw Fp, return value) out."""
    flat = [w for l in item for w in l]
    buf = (ctypes.c_uint32 * len(flat))(*flat)
    out = (ctypes.c_uint32 * (14 * nout))()
    rc = fn(op, buf, aux, out) if aux is not None else fn(op, buf, out)
    return [tuple(out[14 * j:14 * j + 14]) for j in range(nout)], rc


def host_check(fn, op, cases, nout, stride=1):
    V.assert_operands(cases)
    for i in range(0, len(cases), stride):
        got, _ = host_run(fn, op, cases.items[i], cases.aux[i], nout)
        V.check_fps(got, cases.expect(cases.items[i], cases.aux[i]), cases.bound, (cases.name, i))


def test_operand_preconditions():
    """Generators with no host equivalent by that name: the operands are in range and the
    expectation functions run."""
    for c in (V.fp2_conj(), V.fp2_mul_xi(), V.fp2_add_mul_xi(), V.fp2_sub2(), V.fp2_3pm2(), V.fp2_mul_small(),
              V.fp2_pred(), V.fp12_conj(), V.two_lines()):
        V.assert_operands(c)
        assert len(c) <= 4096 and len(c.aux) == len(c)
        c.expect(c.items[0], c.aux[0])
    c = V.fp2_mul_lazy()
    assert max(max(l) for it in c.items for l in it) == (1 << 29) - 2     # the limb bound is reached
    assert max(V.value(l) for it in c.items for l in it) >= 2 * V.Q2 - 4  # and the value bound 4q - 2


def test_fp2_vectors_on_host(L):
    host_check(L.hc_raw_fp2, 0, V.fp2_mul_lazy(), 2)
    host_check(L.hc_raw_fp2, 1, V.fp2_sqr(), 2)
    host_check(L.hc_raw_fp2, 2, V.fp2_inv(), 2)


def test_csqr_vectors_on_host(L):
    host_check(L.hc_raw_fp2, 3, V.csqr_x1(), 8)
    host_check(L.hc_raw_fp2, 3, V.csqr_x63(), 8)
    host_check(L.hc_raw_fp2, 3, V.csqr_one(), 8)
    host_check(L.hc_raw_fp12, 9, V.decompress(), 12)


def test_fp12_vectors_on_host(L):
    host_check(L.hc_raw_fp12, 0, V.fp12_mul(), 12, stride=3)
    host_check(L.hc_raw_fp12, 1, V.fp12_sqr(), 12, stride=3)
    host_check(L.hc_raw_fp12, 3, V.fp12_mul_by_line(), 12, stride=3)
    host_check(L.hc_raw_fp12, 5, V.fp12_inv(), 12)
    host_check(L.hc_raw_fp12, 2, V.fp12_cyc_sqr(), 12)
    c = V.fp12_frob()
    V.assert_operands(c)
    for i in range(0, len(c), 4):
        got = [l for p in (1, 2, 3) for l in host_run(L.hc_raw_fp12, 4, c.items[i], p, 12)[0]]
        V.check_fps(got, c.expect(c.items[i], 0), c.bound, (c.name, i))


def test_cyc_exp_and_final_exp_vectors_on_host(L):
    for op in (7, 8):   # compressed, and the exact Granger-Scott chain
        host_check(L.hc_raw_fp12, op, V.cyc_exp_x(), 12)
        host_check(L.hc_raw_fp12, op, V.cyc_exp_x_one(), 12)
    host_check(L.hc_raw_fp12, 6, V.final_exp(), 12)
    host_check(L.hc_raw_fp12, 6, V.final_exp_degenerate(), 12)
    host_check(L.hc_raw_fp12, 6, V.final_exp_unit(), 12)


def test_g2_vectors_on_host(L):
    for op, c in ((0, V.jac_dbl()), (1, V.jac_add_aff()), (2, V.jac_add()), (3, V.jac_psi()), (4, V.jac_mul_u64()),
                  (5, V.g2_mul_bp())):
        V.assert_operands(c)
        for i, it in enumerate(c.items):
            got, inf = host_run(L.hc_raw_g2, op, it, c.aux[i], 6)
            V.check_point(got, inf, c.expect(it, c.aux[i]), (c.name, i))
    # the edge cases are there: a doubling through jac_add, P + (-P), infinity operands
    c = V.jac_add()
    kinds = set()
    for it in c.items:
        p, o = V._djac(it[:6]), V._djac(it[6:])
        if p[2] == M.ZERO2 or o[2] == M.ZERO2:
            kinds.add("inf")
        elif M.jac_to_affine(V.F2, p) == M.jac_to_affine(V.F2, o):
            kinds.add("dbl")
        elif c.expect(it, 0) is None:
            kinds.add("neg")
    assert kinds == {"inf", "dbl", "neg"}


def test_miller_vectors_on_host(L, golden, torsion):
    recs = V.miller_pairs(golden, torsion)
    assert [r["degenerate"] for r in recs] == [False] * 4 + [True]
    for k, r in enumerate(recs):
        degs = [V.model_degenerate(Qa) for Qa, _ in r["pairs"]]
        assert degs == [r["degenerate"], False]
        for pairs in ([r["pairs"][0]], [r["pairs"][1]], r["pairs"]):
            item = [l for Qa, P in pairs for l in V.mont_pair(Qa, P)]
            for l in item:
                assert V.is_normalised(l)
            got, deg = host_run(L.hc_raw_miller, len(pairs), item, None, 12)
            assert deg == int(any(V.model_degenerate(Qa) for Qa, _ in pairs))
            if not deg:
                V.check_fps(got, V._flat(M.miller_loop_multi(pairs)), V.Q2, ("miller", k, len(pairs)))
        if not r["degenerate"]:
            fe = M.final_exp(M.miller_loop_multi(r["pairs"]))
            assert (fe == M.ONE12) == r["valid"]
    # the model's pairing is the oracle's to the power -3 (final_exp's factor 3, the conjugated loop): one pair
    Qa, P = recs[0]["pairs"][1]
    e = O.pairing((Qa[0], Qa[1], O.FQ2_ONE), (P[0], P[1], 1))
    assert M.to_pyecc12(M.pairing(Qa, P)) == O.f12_pow(e, (-3) % O.r)


# ---------------------------------------------------------- static checks --
def test_devcheck_is_one_gfx950_code_object():
    import build_native
    blob = open(build_native.build_devcheck(), "rb").read()
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in blob
    assert b"amdhsa--gfx942" not in blob and b"amdhsa--gfx90a" not in blob
    assert b"bls381_verify" not in blob      # test infrastructure: no product symbol
