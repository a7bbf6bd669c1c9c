"""hash_to_G2's device searches at crafted trial counts, and privtopub / sign at edge scalars (MI355X).

The try-and-increment search exists in four device forms -- pair-sequential (hash_to_g2_candidate),
16 lanes per item (k_hash_search<16>), known offset (k_hash_g2_lg<on_octet / on_quad>, k_hash_g2) and
pooled over the wave (dev_hash_cand_1 in k_hash_cand_1 and both k_prologue_1) -- and random messages
never take the wide one into a second round or choose the pooled one's lane splits.
tests/golden/hash_search.json holds messages by trial count (up to 19) with oracle points;
tests/hash_search_cases.py composes the waves (tests/test_hash_search_host.py proves from the model
what they reach); lib/libbls381_hashcheck.so (consensus-specs_amd/csrc/hash_check.hip, test
infrastructure) launches the product's kernels and returns what each route wrote.  Every comparison
is exact: each limb < 2^28, each value < 2q and compared mod q; candidates against hashlib and Python
integers for every item, points against the fixture where it stores one, and against each other.
Then the product's own paths: the public hash entries' bytes, verdicts of items that are valid by
construction (pk = g1, sig = the hash itself), the randomized batch's stats, and wrong signatures
built from the next square offset and the negated hash.
"""
import ctypes
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import bls_oracle as O
import devcheck_vectors as V
import hash_search_cases as C

pytestmark = pytest.mark.gpu

q, r = O.q, O.r
ST_OK = 0
ROUTES = ("k_hash_cand_1 + k_hash_bp", "k_prologue_1<0> + k_hash_bp", "k_prologue_1<1> + k_hash_bp",
          "k_hash_g2_lg<on_octet>", "k_hash_g2_lg<on_quad>", "k_hash_g2 (koff)", "k_hash_g2 (sequential)")


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


class Probe:
    def __init__(self, path):
        self.L = ctypes.CDLL(path)
        self.L.hsc_run.argtypes = [ctypes.c_size_t, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int,
                                   ctypes.c_char_p, ctypes.c_char_p] + [ctypes.c_void_p] * 5
        self.cache = {}

    def run(self, key, msgs, mlen, doms, dom_stride, sig96):
        if key not in self.cache:
            n = len(msgs) // mlen
            assert 0 < n <= 4096 and len(msgs) == n * mlen and len(doms) == (8 * n if dom_stride else 8)
            o = {"cand": np.zeros((3, n, 4, 14), np.uint32), "koff": np.zeros(n, np.uint32),
                 "bp": np.zeros((7, n, 4, 14), np.uint32), "st": np.zeros((7, n), np.uint8),
                 "touched": np.zeros(1, np.uint32)}
            rc = self.L.hsc_run(n, msgs, mlen, doms, dom_stride, C.G1_KEY, sig96,
                                *[o[k].ctypes.data for k in ("cand", "koff", "bp", "st", "touched")])
            assert rc == 0, "hsc_run: error %#x" % rc
            self.cache[key] = o
        return self.cache[key]


@pytest.fixture(scope="module")
def hsc(native):
    # `native` first: torch's HIP runtime is loaded before this library's
    import build_native
    return Probe(os.environ.get("BLS381_HASHCHECK_LIB") or build_native.build_hashcheck())


def fp(l):
    assert all(int(w) < 1 << 28 for w in l), "limb"
    v = V.value(l)
    assert v < V.Q2, "value >= 2q"
    return v * V.RINV % q


def point(a):
    """[4][14] raw -> ((x.c0, x.c1), (y.c0, y.c1))"""
    c = [fp(l) for l in a]
    return (c[0], c[1]), (c[2], c[3])


def fixture_bp(p):
    c = [int(h, 16) for h in p["bp_affine"]]
    return (c[0], c[1]), (c[2], c[3])


def compositions(fx):
    return ([("pooled " + n, it) for n, it in C.pooled_compositions(fx.pool())]
            + [("wide " + n, it) for n, it in C.wide_compositions(fx.pool())])


NAMES = ["pooled lone_high"] + ["pooled all_%d" % t for t in range(1, 7)] + \
    ["pooled high_at_%d" % l for l in (0, 31, 63)] + ["pooled three_left", "pooled forty_left"] + \
    ["pooled n_%d" % n for n in (65, 127, 129, 200)] + ["pooled mix_%d" % s for s in range(4)] + \
    ["wide positions", "wide all_second_round"] + ["wide n_%d" % n for n in (1, 3, 5, 9)]


def probe_of(hsc, fx, name):
    comps = dict(compositions(fx))
    assert list(comps) == NAMES
    items = comps[name]
    # per-item domains (dom_stride 8), as every product path passes them; the shared form
    # (dom_stride 0) on the wide position batch
    stride = 0 if name == "wide positions" else 8
    o = hsc.run(name, b"".join(m.msg for m in items), 32, fx.dom8 * (len(items) if stride else 1), stride,
                bytes.fromhex(fx.raw["points"][0]["compressed"]))
    return items, o


# ------------------------------------------------------------------ the probe --
@pytest.mark.parametrize("name", NAMES)
def test_pooled_search_candidates(hsc, fx, name):
    """k_hash_cand_1 and role 0 of k_prologue_1<0> / <1>: every item's candidate is x0 + trials - 1
    with the spec's root of x^3 + 4(1 + i), and nothing is written past item n."""
    items, o = probe_of(hsc, fx, name)
    assert int(o["touched"][0]) == 0
    for j in range(3):
        for i, m in enumerate(items):
            x, y = point(o["cand"][j][i])
            x0 = C.x0_of(m.msg, fx.dom8)
            assert x == ((x0[0] + m.trials - 1) % q, x0[1]), (ROUTES[j], i, m.i, m.trials, (x[0] - x0[0]) % q)
            assert C.on_twist_with_selected_root(x, y), (ROUTES[j], i, m.i)
            if m.point is not None:
                assert [x[0], x[1], y[0], y[1]] == [int(h, 16) for h in m.point["candidate"]], (ROUTES[j], i)


@pytest.mark.parametrize("name", NAMES)
def test_wide_search_offsets_and_every_route_to_the_point(hsc, fx, name):
    """k_hash_search<16>'s offset is trials - 1 for every item; the three known-offset kernels, the
    sequential k_hash_g2 and the pooled k_hash_bp give one verification hash, the fixture's where it
    stores one."""
    items, o = probe_of(hsc, fx, name)
    assert [int(k) for k in o["koff"]] == [m.trials - 1 for m in items]
    assert (o["st"] == ST_OK).all()
    for i, m in enumerate(items):
        pts = [point(o["bp"][j][i]) for j in range(7)]
        assert all(p == pts[6] for p in pts), (i, m.i, [ROUTES[j] for j in range(7) if pts[j] != pts[6]])
        if m.point is not None:
            assert pts[0] == fixture_bp(m.point), (i, m.i)


# ------------------------------------------------------------- public entries --
def test_public_hash_entries_against_the_fixture(native, fx):
    """bls381_hash_to_g2 (k_hash_g2_out: the pair-sequential search) compressed and affine, and
    bls381_hash_to_g2_pyecc_projective, for every message with an oracle record."""
    pts = fx.raw["points"]
    for p in pts:
        comp, aff = native.hash_to_g2(fx.by_i[p["i"]].msg, fx.dom8)
        assert comp.hex() == p["compressed"], (p["i"], p["trials"])
        assert aff.hex() == "".join(p["affine"]), (p["i"], p["trials"])
    out = native.hash_to_g2_pyecc_projective(b"".join(fx.by_i[p["i"]].msg for p in pts), fx.dom8 * len(pts))
    for k, p in enumerate(pts):
        assert out[288 * k:288 * k + 288].hex() == "".join(p["projective"]), (p["i"], p["trials"])


def test_public_hash_at_the_padding_edges(native, fx):
    """msg || dom8 || tag at the SHA-256 padding edges (55 / 56, 63 / 64, 119 / 120 bytes and around)."""
    for c in fx.raw["lengths"]:
        comp, _ = native.hash_to_g2(fx.length_message(c["length"]), fx.dom8)
        assert comp.hex() == c["compressed"], c["length"]


# -------------------------------------------------------------------- verdicts --
def verify_batch(native, items, dom8):
    return list(native.verify_batch(b"".join(it[0] for it in items), b"".join(it[1] for it in items),
                                    b"".join(it[2] for it in items), dom8 * len(items)))


def wide_messages(fx):
    return [m for _, items in C.wide_compositions(fx.pool(points_only=True)) for m in items]


@pytest.mark.parametrize("policy", ["pyecc", "strict"])
def test_verify_batch_over_the_wide_compositions(native, fx, policy):
    """verify_batch (n <= 8192: k_hash_search<16> and the known-offset cofactor map): all True; then
    with wrong signatures at a second-round item of each wave position, exactly those False."""
    msgs = wide_messages(fx)
    items = C.valid_items(msgs)
    with native.subgroup_policy_scope(policy):
        assert verify_batch(native, items, fx.dom8) == [True] * len(items)
        # the positions batch: 16 items per trial count, the item of `t` trials at 16 k + 5 p
        k17 = C.WIDE_TRIALS.index(17)
        where = [16 * k17 + 5 * p for p in range(4)] + [16 * len(C.WIDE_TRIALS) + 5 * p for p in range(4)] + [len(items) - 1]
        assert all(msgs[i].trials >= 17 for i in where)
        want = C.spoil(items, msgs, where)
        assert verify_batch(native, items, fx.dom8) == want


def test_verify_multiple_batch_over_the_wide_compositions(native, fx):
    """verify_multiple_batch over the same messages, calls of one to three items signed by their
    aggregated hashes; the last call's signature negated.  Then one call at a 47-byte message."""
    msgs = wide_messages(fx)
    off, sigs = [0], []
    while off[-1] < len(msgs):
        k = min(1 + len(off) % 3, len(msgs) - off[-1])
        part = msgs[off[-1]:off[-1] + k]
        sigs.append(O.aggregate_signatures([bytes.fromhex(m.point["compressed"]) for m in part]))
        off.append(off[-1] + k)
    nc = len(sigs)
    assert nc >= 40
    sigs[-1] = O.G2_to_signature(O.pt_neg(O.Fq2Ops, O.signature_to_G2(sigs[-1])))
    got = native.verify_multiple_batch(np.array(off, np.uint32), C.G1_KEY * len(msgs), b"".join(m.msg for m in msgs), 32,
                                       b"".join(sigs), fx.dom8 * nc)
    assert list(got) == [True] * (nc - 1) + [False]
    c = next(c for c in fx.raw["lengths"] if c["length"] == 47)
    got = native.verify_multiple_batch(np.array([0, 1], np.uint32), C.G1_KEY, fx.length_message(47), 47,
                                       bytes.fromhex(c["compressed"]), fx.dom8)
    assert list(got) == [True]


def run_randomized(native, items, dom8, B, seed):
    import torch
    L = native.lib()
    n = len(items)
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d = [t(b"".join(it[0] for it in items)), t(b"".join(it[1] for it in items)), t(b"".join(it[2] for it in items)),
         t(dom8 * n)]
    v = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.bls381_verify_batch_randomized_workspace_size(n, B), dtype=torch.uint8, device=dev)
    st = (ctypes.c_uint64 * 3)()
    stream = torch.cuda.current_stream(dev)
    native.check(L.bls381_verify_batch_randomized_device(n, *[x.data_ptr() for x in d], bytes(seed), B, v.data_ptr(),
                                                         ws.data_ptr(), ctypes.c_void_p(stream.cuda_stream), st))
    return list(v.cpu().numpy().astype(bool)), list(st)


@pytest.mark.parametrize("B", [8, 64])
def test_randomized_batch_over_the_pooled_compositions(native, fx, B):
    """bls381_verify_batch_randomized_device (k_prologue_1<1>'s pooled search): every clean batch
    passes as batches -- stats == [n, 0, 0], no item re-verified alone -- and with wrong signatures
    exactly those items are False."""
    seed = bytes(range(32))
    comps = C.pooled_compositions(fx.pool(points_only=True))
    for name, msgs in comps:
        got, stats = run_randomized(native, C.valid_items(msgs), fx.dom8, B, seed)
        assert got == [True] * len(msgs), name
        assert stats == [len(msgs), 0, 0], (name, stats)
    for name in ("high_at_31", "three_left", "n_129"):
        msgs = dict(comps)[name]
        items = C.valid_items(msgs)
        where = [i for i, m in enumerate(msgs) if m.trials >= 16][:4] + [0]
        want = C.spoil(items, msgs, where)
        got, stats = run_randomized(native, items, fx.dom8, B, seed)
        assert got == want, name
        assert stats[2] == len({i // B for i in where}), (name, stats)


@pytest.mark.parametrize("policy", ["pyecc", "strict"])
def test_verify_batch_above_the_wide_threshold(native, fx, policy):
    """8192 + 65 items, the smallest batch past the wide search: k_prologue_1<0> (py_ecc) and
    k_hash_cand_1 (strict), the high-trial items in the last, partial wave."""
    pool = fx.pool(points_only=True)
    low = [m for t in range(1, 16) for m in pool[t]]
    high = [m for t in sorted(pool) if t >= 16 for m in pool[t]]
    n = 8192 + 65
    msgs = [low[i % len(low)] for i in range(n - len(high))] + high
    # one lane per item: the last wave holds item n - 1 alone, the wave before it the other high ones
    assert len(msgs) == n and msgs[-1].trials == fx.max_trials and n % 64 == 1
    items = C.valid_items(msgs)
    where = [n - 1, n - len(high), 4097]
    with native.subgroup_policy_scope(policy):
        assert verify_batch(native, items, fx.dom8) == [True] * n
        want = C.spoil(items, msgs, where)
        assert verify_batch(native, items, fx.dom8) == want


_QUAD_SCRIPT = r"""
import os, sys
root = sys.argv[1]
sys.path[:0] = [root, os.path.join(root, "consensus-specs_amd"), os.path.join(root, "oracle"), os.path.join(root, "tests")]
import bls_oracle as O
import hash_search_cases as C
from bls381_amd import _native as native
native.init(0)
fx = C.fixture()
msgs = [m for _, items in C.wide_compositions(fx.pool(points_only=True)) for m in items]
pk = O.privtopub(1)
sigs = [bytes.fromhex(m.point["compressed"]) for m in msgs]
bad = [i for i, m in enumerate(msgs) if m.trials >= 17][::3]
for k, i in enumerate(bad):
    sigs[i] = bytes.fromhex(msgs[i].point["negated_sig" if k % 2 else "next_square_sig"])
got = native.verify_batch(pk * len(msgs), b"".join(m.msg for m in msgs), b"".join(sigs), fx.dom8 * len(msgs))
assert list(got) == [i not in bad for i in range(len(msgs))], list(got)
print("quad hash ok", len(msgs), len(bad))
"""


def test_quad_cofactor_map_knob(fx):
    """BLS381_HASH_OCT=0 (read once per process, so in a child process): k_hash_g2_lg<on_quad> behind the
    wide search in the product's own path, over the wide compositions."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _QUAD_SCRIPT, root], env=dict(os.environ, BLS381_HASH_OCT="0"),
                         capture_output=True, text=True, timeout=110)
    assert res.returncode == 0 and "quad hash ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# --------------------------------------------------------------------- scalars --
def sk32(k):
    return k.to_bytes(32, "big")


def test_privtopub_and_sign_at_the_edge_scalars(native, fx):
    """k_privtopub and k_sign (jac_mul_limbs over 256 bits) at 0, around r and 2r (the ladder's last
    addition cancels at r and doubles at r + 2), powers of two, 2^256 - 1 and random scalars >= r:
    alone and through the shim, bytes against the oracle's."""
    from bls381_amd import bls
    ms = [fx.by_i[i].msg for i in fx.raw["scalar_messages"]]
    for s in fx.raw["scalars"]:
        k = int(s["k"], 16)
        assert native.privtopub(sk32(k)).hex() == s["pubkey"], hex(k)
        assert bls.privtopub(k).hex() == s["pubkey"], hex(k)
        for m, want in zip(ms, s["signatures"]):
            assert native.sign(m, sk32(k), fx.dom8).hex() == want, hex(k)
            assert bls.bls_sign(m, k, fx.domain).hex() == want, hex(k)
    k = (1 << 256) + 5
    assert bls.privtopub(k) == O.privtopub(k)


def test_batches_with_the_edge_scalars_among_random_ones(native, fx):
    """privtopub_batch and sign_batch of 130 items: every edge scalar among random ones, and at the first
    and last lane of a wave (privtopub: one lane per item; sign: a lane pair per item), so lanes that
    take the cancelling and the doubling branch share a wave with ordinary ones.  Per-item bytes equal
    the single calls' (compared with the oracle above)."""
    rng = random.Random(0xED6E)
    edge = [int(s["k"], 16) for s in fx.raw["scalars"]]
    n = 130
    ks = [rng.randrange(1, r) for _ in range(n)]
    # the first and last lane of the waves (one lane per item: items 0, 63, 64, ..; a lane pair per
    # item: items 0, 31, 32, ..), then every edge scalar once among the random ones
    ends = [0, 63, 64, 127, 128, 129, 31, 32, 95, 96]
    for at, k in zip(ends, [r, r + 2, 0, 2 * r + 4, r + 2, r, r - 1, r + 1, 2 * r, r + 2]):
        ks[at] = k
    for at, k in zip([s for s in range(1, 130, 4) if s not in ends], edge):
        ks[at] = k
    assert set(edge) <= set(ks)
    pool = [m for t in (1, 2, 3, 4, 5, 16, 17) for m in fx.pool()[t][:3]]
    msgs = [pool[i % len(pool)].msg for i in range(n)]
    pubs = native.privtopub_batch(b"".join(sk32(k) for k in ks))
    sigs = native.sign_batch(b"".join(msgs), b"".join(sk32(k) for k in ks), fx.dom8 * n)
    known = {int(s["k"], 16): s["pubkey"] for s in fx.raw["scalars"]}
    for i, k in enumerate(ks):
        assert pubs[48 * i:48 * i + 48] == native.privtopub(sk32(k)), (i, hex(k))
        if k in known:
            assert pubs[48 * i:48 * i + 48].hex() == known[k], (i, hex(k))
        assert sigs[96 * i:96 * i + 96] == native.sign(msgs[i], sk32(k), fx.dom8), (i, hex(k))
