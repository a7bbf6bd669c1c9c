"""The randomized batch's reference model (tests/rb_model.py) and joint ladder on the CPU.

jac_mul_2x32 from the host build of the device headers (libbls381_hostcheck.so, hc_raw_mul_2x32)
against the model on G1, on the order-3 point (0, 2) and on G2; the model's bucket MSM against the
direct sum of [r_i] Q_i; the endomorphism constants of bls381_consts.hpp as [mu]; and the static
checks of lib/libbls381_rbcheck.so.  Every comparison is exact.  No GPU.
"""
import ctypes
import hashlib
import os
import random
import re

import pytest

import bls_oracle as O
import devcheck_vectors as V
import rb_model as RB
import tower_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
q, r = O.q, O.r
F1, F2 = M.Fq, M.Fq2

TOP = 0x80000000
FIXED_WEIGHTS = [(1, 0), (0, 1), (0xFFFFFFFF, 0xFFFFFFFF), (0x9E3779B9, 0x9E3779B9), (3, 3), (TOP, 0), (0, TOP),
                 (TOP, TOP), (0xC0FFEE, 0), (0, 0xC0FFEE), (2, 1), (1, 2)]


def weights(seed, n_random=6):
    rng = random.Random(seed)
    return FIXED_WEIGHTS + [(rng.randrange(1 << 32), rng.randrange(1 << 32)) for _ in range(n_random)]


def g1_members():
    g = (O.g_x, O.g_y, 1)
    return [M.jac_to_affine(F1, M.jac_mul(F1, g, k)) for k in (1, 0xDEADBEEF, r - 2)]


def g2_members():
    return V.g2_points()[:6:2]


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_raw_mul_2x32.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.hc_sha256.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def host_mul(L, group, fps, k0, k1):
    """raw Fp operands -> (Jacobian raw Fp, infinity flag)."""
    flat = [w for l in fps for w in l]
    nout = 3 if group == 0 else 6
    buf = (ctypes.c_uint32 * len(flat))(*flat)
    out = (ctypes.c_uint32 * (14 * nout))()
    inf = L.hc_raw_mul_2x32(group, buf, k0, k1, out)
    assert inf in (0, 1)
    return [tuple(out[14 * j:14 * j + 14]) for j in range(nout)], inf


def check_g1(got, inf, want_aff, ctx):
    for l in got:
        assert V.is_normalised(l), ctx
    p = tuple(V.dec(l) for l in got)
    assert bool(inf) == (want_aff is None) == (p[2] == 0), ctx
    if want_aff is not None:
        assert M.jac_to_affine(F1, p) == want_aff, ctx


def test_weight_follows_the_digest_words(L):
    """The device reads the digest as eight big-endian words d[0..7] (sha256 of bls381_hash.hpp, here
    through the host build) and takes k1 = d[0], k0 = d[1]; the index is 8 little-endian bytes."""
    seed = bytes(range(32))
    for i in (0, 1, 255, 256, (1 << 32) + 5):
        msg = seed + i.to_bytes(8, "little")
        out = ctypes.create_string_buffer(32)
        L.hc_sha256(msg, 40, out)
        assert out.raw == hashlib.sha256(msg).digest()
        d = [int.from_bytes(out.raw[4 * j:4 * j + 4], "big") for j in range(8)]
        assert RB.weight(seed, i) == (d[1], d[0])
    assert RB.weight(seed, 0) != RB.weight(seed, 1) != RB.weight(bytes(32), 1)
    k0, k1 = RB.weight(seed, 7)
    assert RB.scalar(k0, k1) == (k0 - M.X_ABS ** 2 * k1) % r


def test_host_ladder_on_g1_members(L):
    """[k0] P + [k1] sigma(P) on G1: the model's sum, which is [(k0 + mu k1) mod r] P."""
    for j, P in enumerate(g1_members()):
        S = RB.sigma(P)
        assert S == M.jac_to_affine(F1, M.jac_mul(F1, RB.jac(F1, P), RB.MU))
        ops = [V.mont(P[0]), V.mont(P[1]), V.mont(S[0]), V.mont(S[1])]
        for k0, k1 in weights(11 + j):
            want = RB.r1(P, k0, k1)
            assert want == M.jac_to_affine(F1, M.jac_mul(F1, RB.jac(F1, P), RB.scalar(k0, k1)))
            got, inf = host_mul(L, 0, ops, k0, k1)
            check_g1(got, inf, want, ("g1", j, k0, k1))


def test_host_ladder_on_the_order_3_point(L):
    """sigma fixes (0, 2): the ladder adds one point twice per bit (jac_add_aff's doubling branch on
    one lane) and the result is [k0 + k1] (0, 2): infinity exactly when k0 + k1 = 0 mod 3."""
    P = (0, 2)
    assert RB.sigma(P) == P and M.jac_to_affine(F1, M.jac_mul(F1, RB.jac(F1, P), 3)) is None
    ops = [V.mont(0), V.mont(2), V.mont(0), V.mont(2)]
    seen = set()
    for k0, k1 in weights(5, n_random=12):
        want = RB.r1(P, k0, k1)
        assert (want is None) == ((k0 + k1) % 3 == 0)
        seen.add(want)
        got, inf = host_mul(L, 0, ops, k0, k1)
        check_g1(got, inf, want, ("order3", k0, k1))
    assert seen == {None, (0, 2), (0, q - 2)}


def test_host_ladder_on_g2_members(L):
    """[k0] Q + [k1] phi(Q) on G2 with phi = -psi^2: [(k0 + mu k1) mod r] Q."""
    for j, Q in enumerate(g2_members()):
        S = RB.phi(Q)
        assert S == M.jac_to_affine(F2, M.jac_mul(F2, RB.jac(F2, Q), RB.MU))
        ops = V.montjac((Q[0], Q[1])) + V.montjac((S[0], S[1]))
        for k0, k1 in weights(23 + j, n_random=3):
            want = RB.r2(Q, k0, k1)
            if (k0, k1) in FIXED_WEIGHTS[:4]:
                assert want == M.jac_to_affine(F2, M.jac_mul(F2, RB.jac(F2, Q), RB.scalar(k0, k1)))
            got, inf = host_mul(L, 1, ops, k0, k1)
            V.check_point(got, inf, want, ("g2", j, k0, k1))
    # Q and phi(Q) = Q cannot happen on G2, but s = a can be asked of the ladder: [k0 + k1] Q
    Q = g2_members()[0]
    got, inf = host_mul(L, 1, V.montjac(Q) + V.montjac(Q), 5, 6)
    V.check_point(got, inf, M.jac_to_affine(F2, M.jac_mul(F2, RB.jac(F2, Q), 11)), "g2 s = a")


def _const(name):
    src = open(os.path.join(ROOT, "consensus-specs_amd", "csrc", "bls381_consts.hpp")).read()
    m = re.search(r"BLS_CONST fp_t %s = \{\{([^}]*)\}\}" % name, src)
    limbs = tuple(int(w.strip().rstrip("u"), 16) for w in m.group(1).split(","))
    assert len(limbs) == 14 and V.is_normalised(limbs)
    return V.dec(limbs)


def test_endomorphism_constants_act_as_mu():
    """G1_BETA_M and G2_ZETA_M of bls381_consts.hpp: (beta x, y) = [mu] P on G1 and (zeta x, y) =
    [mu] Q = -psi^2(Q) on G2, mu = -x^2 mod r."""
    beta, zeta = _const("G1_BETA_M"), _const("G2_ZETA_M")
    assert RB.MU == (-(M.X_ABS ** 2)) % r and (RB.MU * RB.MU + RB.MU + 1) % r == 0
    assert beta == M.BETA and pow(beta, 3, q) == 1 != beta and pow(zeta, 3, q) == 1 != zeta
    for P in g1_members():
        assert (beta * P[0] % q, P[1]) == M.jac_to_affine(F1, M.jac_mul(F1, RB.jac(F1, P), RB.MU))
    for Q in g2_members():
        zq = ((zeta * Q[0][0] % q, zeta * Q[0][1] % q), Q[1])
        assert zq == RB.phi(Q) == M.jac_to_affine(F2, M.jac_mul(F2, RB.jac(F2, Q), RB.MU))


def msm_points(n, seed):
    """n distinct G2 members (multiples of the generator)."""
    rng = random.Random(seed)
    gen = (O.G2_gen_x, O.G2_gen_y, M.ONE2)
    return [M.jac_to_affine(F2, M.jac_mul(F2, gen, rng.randrange(1, 1 << 64))) for _ in range(n)]


@pytest.mark.parametrize("B", [2, 4, 8])
def test_model_msm_equals_the_direct_sum(B):
    """Buckets, window sums and the Horner combine give sum_i [r_i] Q_i, by the ladder's route
    (k0 Q + k1 phi(Q)) and by one multiplication with (k0 + mu k1) mod r; items outside the batch
    keep their lists empty; Q / -Q pairs and a repeated point are among the inputs."""
    pts = msm_points(8, 31 + B)
    Q = pts[0]
    pts = pts[:3] + [(Q[0], M.neg2(Q[1])), None, pts[3], pts[3]] + pts[4:]      # 11 items: a ragged tail
    assert len(pts) == 11
    seed = hashlib.sha256(b"rb_model %d" % B).digest()
    m = RB.Msm(pts, B, seed)
    assert m.nb == (11 + B - 1) // B
    for b in range(m.nb):
        direct = RB.INF2
        for i in range(b * B, min(11, b * B + B)):
            if pts[i] is not None:
                direct = M.jac_add(F2, direct, M.jac_mul(F2, RB.jac(F2, pts[i]), RB.scalar(*m.weights[i])))
        assert m.s[b] == m.ladder_sum(b) == M.jac_to_affine(F2, direct), b
        for w in range(RB.MSM_W):
            assert m.off[b][w][0] == m.off[b][w][1] == 0
            assert [m.off[b][w][d + 1] - m.off[b][w][d] for d in range(1, RB.MSM_D)] == \
                [len(m.lists[b][w][d]) for d in range(1, RB.MSM_D)]
    none_at = 4
    b, t = divmod(none_at, B)
    assert not any(p // 2 == t for w in range(RB.MSM_W) for d in range(RB.MSM_D) for p in m.lists[b][w][d])


def test_rbcheck_is_one_gfx950_code_object():
    import build_native
    blob = open(build_native.build_rbcheck(), "rb").read()
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in blob
    assert b"amdhsa--gfx942" not in blob and b"amdhsa--gfx90a" not in blob
    assert b"bls381_verify" not in blob      # test infrastructure: no product symbol
    assert b"rbc_run" in blob
