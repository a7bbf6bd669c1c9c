"""The randomized batch's scalar side against Python integers (MI355X).

A sub-batch that fails bls381_verify_batch_randomized is re-verified item by item, so a wrong
weight, [r_i] pk_i or sum_i [r_i] sig_i never changes a verdict.  lib/libbls381_rbcheck.so
(consensus-specs_amd/csrc/rb_check.hip, test infrastructure) launches the product's own kernels --
k_prologue_1<1>, k_rb_g2_test, k_rb_msm_sort / _bucket / _window / _combine and k_rb_scale_g2 --
and returns every intermediate; tests/rb_model.py (proven on the CPU by tests/test_rb_model.py)
says what each must be.  Every comparison is exact: each output limb < 2^28, each value < 2q,
points compared as points (Jacobian against the model's affine one), infinity by Z = 0 mod q, the
sort's list starts exactly and each list as a multiset (the device fills them with atomics).
Each test is one probe call with n <= 96 items.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import bls_oracle as O
import devcheck_vectors as V
import rb_model as RB
import tower_model as M

pytestmark = pytest.mark.gpu

q = O.q
F1, F2 = M.Fq, M.Fq2
W, D = RB.MSM_W, RB.MSM_D


class Probe:
    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        self.L.rbc_run.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.c_int] + [ctypes.c_void_p] * 8
        dims = (ctypes.c_int * 3)()
        self.L.rbc_dims(dims)
        assert tuple(dims) == (RB.MSM_C, W, D)

    def run(self, pks, sigs, B, seed, strict):
        n = len(pks) // 48
        assert len(pks) == 48 * n and len(sigs) == 96 * n and 0 < n <= 96 and len(seed) == 32
        nb = (n + B - 1) // B
        o = {"st": np.zeros((4, n), np.uint8), "r1": np.zeros((n, 2, 14), np.uint32),
             "r2": np.zeros((n, 6, 14), np.uint32), "off": np.zeros((nb, W, D + 1), np.uint32),
             "idx": np.zeros((nb, W, 2 * B), np.uint16), "bucket": np.zeros((nb, W, D, 6, 14), np.uint32),
             "win": np.zeros((nb, W, 6, 14), np.uint32), "sb": np.zeros((nb, 6, 14), np.uint32)}
        rc = self.L.rbc_run(n, B, bytes(seed), bytes(pks), bytes(sigs), int(strict),
                            *[o[k].ctypes.data for k in ("st", "r1", "r2", "off", "idx", "bucket", "win", "sb")])
        assert rc == 0, "rbc_run: HIP error %d" % rc
        for k in ("r1", "r2", "bucket", "win", "sb"):
            assert (o[k] < (1 << 28)).all(), (k, "limb")
        return o


@pytest.fixture(scope="module")
def rbc(native):
    # `native` first: torch's HIP runtime is loaded before this library's
    import build_native
    return Probe(os.environ.get("BLS381_RBCHECK_LIB") or build_native.build_rbcheck())


# ------------------------------------------------------------------ decoding --
def fp(l):
    v = V.value(l)
    assert v < V.Q2, "value >= 2q"
    return v * V.RINV % q


def g2jac(a):
    """[6][14] raw -> Jacobian (X, Y, Z) over Fp2."""
    c = [fp(l) for l in a]
    return ((c[0], c[1]), (c[2], c[3]), (c[4], c[5]))


def same_point(F, got, want_aff):
    """The Jacobian `got` is the affine `want_aff` (None: infinity, Z = 0)."""
    X, Y, Z = got
    if want_aff is None or Z == F.zero:
        return want_aff is None and Z == F.zero
    zz = F.mul(Z, Z)
    return X == F.mul(want_aff[0], zz) and Y == F.mul(want_aff[1], F.mul(zz, Z))


# -------------------------------------------------------------------- inputs --
_POOL = {}
_STATUS = {}


def pool():
    """96 G2 members and 16 G1 members (multiples of the generators), computed once."""
    if not _POOL:
        g2 = (O.G2_gen_x, O.G2_gen_y, M.ONE2)
        g1 = (O.g_x, O.g_y, 1)
        ks = [int.from_bytes(hashlib.sha256(b"rb pool %d" % i).digest()[:12], "big") | 1 for i in range(112)]
        _POOL["sig"] = [M.jac_to_affine(F2, M.jac_mul(F2, g2, k)) for k in ks[:96]]
        _POOL["key"] = [M.jac_to_affine(F1, M.jac_mul(F1, g1, k)) for k in ks[96:]]
    return _POOL


def sig_bytes(Q):
    return O.G2_to_signature((Q[0], Q[1], M.ONE2))


def key_bytes(P):
    return O.G1_to_pubkey((P[0], P[1], 1))


def neg2pt(Q):
    return (Q[0], M.neg2(Q[1]))


INF_KEY = b"\xc0" + bytes(47)
INF_SIG = b"\xc0" + bytes(95)


def off_curve_key():
    """A canonical encoding whose x has no y: undecodable under both codecs."""
    x = 1
    while pow((x ** 3 + 4) % q, (q - 1) // 2, q) == 1:
        x += 1
    return (x + (1 << 383)).to_bytes(48, "big")


def off_curve_sig():
    x = 1
    while O.modular_squareroot(O.f2_add(O.f2_mul(O.f2_sqr((x, 0)), (x, 0)), O.B2)) is not None:
        x += 1
    return (1 << 383).to_bytes(48, "big") + x.to_bytes(48, "big")


def statuses(pk, sig, strict):
    k = (bytes(pk), bytes(sig), strict)
    if k not in _STATUS:
        for kind, b, f in (("k", pk, RB.key_status), ("s", sig, RB.sig_status)):
            if (kind, bytes(b), strict) not in _STATUS:
                _STATUS[(kind, bytes(b), strict)] = f(bytes(b), strict)
        _STATUS[k] = (_STATUS[("k", bytes(pk), strict)], _STATUS[("s", bytes(sig), strict)])
    return _STATUS[k]


# ---------------------------------------------------------- the whole comparison --
def model_of(items, B, seed, strict):
    """items: [(pk48, sig96)].  (per-item statuses and points, the Msm over the batched items)."""
    per = [statuses(pk, sig, strict) for pk, sig in items]
    pts = [Q if RB.batched(ps, ss) else None for (ps, _), (ss, Q) in per]
    return per, RB.Msm(pts, B, seed)


def check_call(rbc, items, B, seed, strict, per=None, msm=None):
    """One probe call compared with the model, output by output.  Returns (outputs, per, msm)."""
    if msm is None:
        per, msm = model_of(items, B, seed, strict)
    n = len(items)
    o = rbc.run(b"".join(pk for pk, _ in items), b"".join(s for _, s in items), B, seed, strict)
    pk_st, sig_st, cls, r1_st = (list(map(int, o["st"][j])) for j in range(4))
    for i, ((ps, P), (ss, Q)) in enumerate(per):
        k0, k1 = msm.weights[i]
        assert (pk_st[i], sig_st[i], cls[i]) == (ps, ss, RB.item_class(ps, ss)), ("status", i)
        # R1: affine, ST_OK; an infinite R1 (or no finite key) is ST_INF
        want = RB.r1(P, k0, k1) if ps == RB.ST_OK else None
        assert r1_st[i] == (RB.ST_INF if want is None else RB.ST_OK), ("r1_st", i)
        if want is not None:
            assert (fp(o["r1"][i][0]), fp(o["r1"][i][1])) == want, ("R1", i)
        # R2: the ladder; infinity for an item outside the batch
        want = RB.r2(Q, k0, k1) if msm.points[i] is not None else None
        assert same_point(F2, g2jac(o["r2"][i]), want), ("R2", i)
    for b in range(msm.nb):
        for w in range(W):
            off = list(map(int, o["off"][b][w]))
            assert off == msm.off[b][w], ("off", b, w)
            for d in range(1, D):
                got = sorted(int(x) for x in o["idx"][b][w][off[d]:off[d + 1]])
                assert got == sorted(msm.lists[b][w][d]), ("list", b, w, d)
                assert same_point(F2, g2jac(o["bucket"][b][w][d]), msm.bucket[b][w][d]), ("bucket", b, w, d)
            assert same_point(F2, g2jac(o["win"][b][w]), msm.win[b][w]), ("window", b, w)
        assert same_point(F2, g2jac(o["sb"][b]), msm.s[b]), ("S_b", b)
        # the two routes of the product agree on the device too: the MSM's S_b is the sum of the ladder's R2
        acc = RB.INF2
        for i in range(b * B, min(n, b * B + B)):
            acc = M.jac_add(F2, acc, g2jac(o["r2"][i]))
        assert same_point(F2, g2jac(o["sb"][b]), M.jac_to_affine(F2, acc)), ("S_b = sum R2", b)
    return o, per, msm


def seed_of(tag):
    return hashlib.sha256(b"test_randomized_scalars " + tag.encode()).digest()


# ------------------------------------------------------------------- statuses --
def fixture_items(torsion):
    items = [(bytes.fromhex(c["pubkey"]), bytes.fromhex(c["signature"])) for c in torsion["verify"]]
    p = pool()
    good = [(key_bytes(p["key"][j]), sig_bytes(p["sig"][j])) for j in range(5)]
    (good_k, good_s) = good[0]
    # hand-made ones, the items outside the batch each between two batched items (under both policies)
    items += [good[0], (off_curve_key(), good_s), good[1], (good_k, INF_SIG), good[2], (good_k, off_curve_sig()),
              good[3], (INF_KEY, good_s), good[4]]
    return [it for it in items if len(it[0]) == 48 and len(it[1]) == 96]


@pytest.mark.parametrize("policy", ["pyecc", "strict"])
def test_statuses_classes_and_points_on_the_fixtures(rbc, torsion, policy):
    """The torsion and non-canonical fixtures' verify items plus hand-made ones, under each policy:
    pk_st, sig_st, cls and r1_st as the oracle's decoders and subgroup tests give them; R1 for every
    finite key (keys with a torsion component under py_ecc's policy included: k0 P + k1 sigma(P));
    items outside the batch keep empty digit lists and an infinite R2."""
    strict = policy == "strict"
    items = fixture_items(torsion)
    assert len(items) <= 96
    B, seed = 8, seed_of("statuses")
    per, msm = model_of(items, B, seed, strict)
    seen = {(ps, ss) for (ps, _), (ss, _) in per}
    keys, sigs = {ps for ps, _ in seen}, {ss for _, ss in seen}
    # undecodable / infinite keys and signatures, a signature on the curve outside G2
    assert keys == {RB.ST_OK, RB.ST_INF, RB.ST_BAD} and {RB.ST_OK, RB.ST_INF, RB.ST_BAD} <= sigs
    assert (RB.ST_NOSUB in sigs) == (not strict)
    classes = {RB.item_class(ps, ss) for ps, ss in seen}
    assert classes == ({RB.RB_BAD, RB.RB_BATCH} if strict else {RB.RB_BAD, RB.RB_BATCH, RB.RB_SINGLE})
    # a torsion key: decodes, is not in G1 (py_ecc keeps it, the strict policy rejects it)
    tors = [i for i, (pk, _) in enumerate(items) if RB.key_status(pk, False)[0] == RB.ST_OK
            and not M.g1_in_subgroup(RB.jac(F1, RB.key_status(pk, False)[1]))]
    assert len(tors) >= 4
    for i in tors:
        assert per[i][0][0] == (RB.ST_BAD if strict else RB.ST_OK)
    # a signature outside G2 under py_ecc: RB_SINGLE, the same bytes RB_BAD under strict
    nosub = [i for i, (_, s) in enumerate(items) if RB.sig_status(s, False)[0] == RB.ST_NOSUB]
    assert nosub and all(RB.item_class(*[x[0] for x in per[i]]) == (RB.RB_BAD if strict else RB.RB_SINGLE)
                         for i in nosub if per[i][0][0] != RB.ST_BAD)
    # non-batched items sit between batched ones and keep their lists empty
    out = [i for i in range(len(items)) if msm.points[i] is None]
    assert out and any(msm.points[i - 1] is not None and msm.points[i + 1] is not None for i in out[1:-1])
    for i in out:
        b, t = divmod(i, B)
        assert not any(p // 2 == t for w in range(W) for d in range(D) for p in msm.lists[b][w][d])
    check_call(rbc, items, B, seed, strict, per, msm)


def test_r1_on_the_order_3_point(rbc):
    """The key (0, 2) of order 3 (py_ecc's policy keeps it): sigma fixes it, so jac_mul_2x32 adds one
    point twice per bit and R1 = [k0 + k1] (0, 2) is infinite exactly when k0 + k1 = 0 mod 3."""
    pk = b"\x80" + bytes(47)
    assert RB.key_status(pk, False) == (RB.ST_OK, (0, 2))
    n, seed = 24, seed_of("order 3")
    inf = [sum(RB.weight(seed, i)) % 3 == 0 for i in range(n)]
    assert 3 <= sum(inf) <= n - 3          # both outcomes are there
    p = pool()
    items = [(pk, sig_bytes(p["sig"][i])) for i in range(n)]
    o, _, _ = check_call(rbc, items, 8, seed, False)
    assert [int(s) for s in o["st"][3]] == [RB.ST_INF if f else RB.ST_OK for f in inf]
    assert {(fp(o["r1"][i][0]), fp(o["r1"][i][1])) for i in range(n) if not inf[i]} == {(0, 2), (0, q - 2)}


def test_two_seeds_give_different_weights(rbc):
    """The seed reaches the weights: the same items under two seeds have different R1, R2 and S_b
    (each compared with the model), and a member key's R1 is [(k0 + mu k1) mod r] pk."""
    p = pool()
    items = [(key_bytes(p["key"][i % 16]), sig_bytes(p["sig"][i])) for i in range(10)]
    outs = []
    for tag in ("seed a", "seed b"):
        seed = seed_of(tag)
        o, per, msm = check_call(rbc, items, 4, seed, True)
        for i in (0, 3, 9):
            P = per[i][0][1]
            want = M.jac_to_affine(F1, M.jac_mul(F1, RB.jac(F1, P), RB.scalar(*msm.weights[i])))
            assert (fp(o["r1"][i][0]), fp(o["r1"][i][1])) == want
            Q = per[i][1][1]
            assert same_point(F2, g2jac(o["r2"][i]), M.jac_to_affine(F2, M.jac_mul(F2, RB.jac(F2, Q), RB.scalar(*msm.weights[i]))))
        outs.append(o)
    for i in range(10):
        assert [fp(l) for l in outs[0]["r1"][i]] != [fp(l) for l in outs[1]["r1"][i]], i
    assert not np.array_equal(outs[0]["off"], outs[1]["off"])


# ------------------------------------------------------ the ladder and the MSM --
SIZES = {2: 25, 8: 35, 64: 75}     # n: whole sub-batches and a ragged last one


def msm_inputs(kind, B):
    """[(pk48, sig96)] of SIZES[B] items."""
    p = pool()
    n = SIZES[B]
    key = lambda i: key_bytes(p["key"][i % 16])
    sigs = [p["sig"][i] for i in range(n)]
    if kind == "repeat":        # every whole sub-batch: one signature B times (P + P in a bucket)
        sigs = [p["sig"][i // B] if i < n // B * B else p["sig"][i] for i in range(n)]
    elif kind == "negpairs":    # adjacent Q / -Q pairs (a bucket sums to infinity in the middle of its list)
        sigs = [p["sig"][i // 2] if i % 2 == 0 else neg2pt(p["sig"][i // 2]) for i in range(n)]
    items = [(key(i), sig_bytes(Q)) for i, Q in enumerate(sigs)]
    if kind == "outsiders":     # a bad key and an infinite signature in the middle of sub-batches
        for i in range(1, n, 5):
            items[i] = (off_curve_key(), items[i][1]) if i % 2 else (items[i][0], INF_SIG)
    elif kind == "empty":       # the first sub-batch holds no batched item: S_0 is infinity
        for i in range(B):
            items[i] = (off_curve_key(), items[i][1]) if i % 2 else (items[i][0], INF_SIG)
    return items


@pytest.mark.parametrize("B", [2, 8, 64])
@pytest.mark.parametrize("kind", ["distinct", "repeat", "negpairs", "outsiders", "empty"])
def test_ladder_and_msm(rbc, kind, B):
    """R2 = [r_i] sig_i (k_rb_scale_g2), the sort's lists, every bucket and window sum and S_b
    (k_rb_msm_*), with a ragged last sub-batch.  The cases the point formulas branch on are asserted
    from the model before the launch: a bucket holding Q and -Q, a bucket holding one point twice
    (jac_add_aff's doubling), a window whose top occupied digit sits directly above an empty one
    (k_rb_msm_window's run == sum: jac_add's doubling), zero digits, an all-infinite sub-batch."""
    items = msm_inputs(kind, B)
    seed = seed_of("%s %d" % (kind, B))
    per, msm = model_of(items, B, seed, False)
    assert msm.nb >= 2 and len(items) % B != 0
    assert msm.zero_digits() >= 1
    if kind == "negpairs":
        assert msm.buckets_with_cancellation()
    if kind == "repeat":
        assert msm.buckets_with_repeat()
    if kind == "outsiders":
        assert sum(pt is None for pt in msm.points) >= 4
    if kind == "empty":
        assert msm.s[0] is None and all(x is None for x in msm.win[0]) and msm.s[1] is not None
    if B == 2:
        assert len(msm.windows_with_run_eq_sum()) >= 3
    check_call(rbc, items, B, seed, False, per, msm)
