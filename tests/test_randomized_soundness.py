"""Soundness of bls381_verify_batch_randomized: what the weights r_i exist for (MI355X).

Every tampered batch here leaves prod_i e(H(m_i), pk_i) * e(sum_i sig_i, -g1) unchanged -- two
signatures exchanged under one message, sig_a + D and sig_b - D, pk_a + E and pk_b - E under one
message, three signatures rotated -- so a build whose weights were all equal, or depended on the
quad (items 2q and 2q + 1 share one Miller accumulator) and not on the item, or ignored the seed or
k1, would accept them, while every touched item is invalid on its own.  With independent weights a
sub-batch holding such a group fails except with probability <= 2^-63 per case (two items of a
group share their weight with probability 2^-64; the groups here have at most three items), is
re-verified item by item, and the statistics say so: the verdicts alone could not.

The tampers are derived on the CPU with the oracle's point arithmetic; the expected verdicts are
native.verify_batch's, which must be False exactly on the touched items.
"""
import ctypes
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest

import bls_oracle as O
import rb_model as RB

pytestmark = pytest.mark.gpu

NKEYS = 11           # item i signs with key i % NKEYS: the positions below never pair one key with itself
NMAX = 260
DOM = (3).to_bytes(8, "big")
SEEDS = [bytes(range(32)), hashlib.sha256(b"test_randomized_soundness").digest()]
# sub-batch size -> batch size (a ragged last sub-batch; 258 is the smallest size past the bucket
# MSM's limit of 256 items: the per-item ladder and the tree sum, with a 2-item tail)
SIZES = {2: 9, 8: 29, 64: 135, 258: 260}


def _h(tag, i):
    return hashlib.sha256(b"soundness %s %d" % (tag, i)).digest()


@pytest.fixture(scope="module")
def base(native):
    """Keys, messages and one signing call: item i's own (key i % NKEYS, message i), and every key
    on each shared message."""
    sks = [int.from_bytes(_h(b"key", k), "big") % O.r for k in range(NKEYS)]
    pks = [O.privtopub(sk) for sk in sks]
    msgs = [_h(b"msg", i) for i in range(NMAX)]
    shared = [_h(b"shared", j) for j in range(2)]
    jobs = [(i % NKEYS, msgs[i]) for i in range(NMAX)] + [(k, s) for s in shared for k in range(NKEYS)]
    out = bytes(native.sign_batch(b"".join(m for _, m in jobs), b"".join(sks[k].to_bytes(32, "big") for k, _ in jobs),
                                  DOM * len(jobs)))
    sig = {(k, m): out[96 * j:96 * j + 96] for j, (k, m) in enumerate(jobs)}
    assert sig[(0, msgs[0])] == O.sign(msgs[0], sks[0], 3)
    assert len(set(pks)) == NKEYS >= 8
    return SimpleNamespace(pks=pks, msgs=msgs, shared=shared, sig=sig)


def clean_items(base, n, same=()):
    """n valid items [pk, msg, sig]: distinct messages, except that every 13th item (from 3) signs
    shared[1] and the positions in `same` sign shared[0]."""
    items = []
    for i in range(n):
        k = i % NKEYS
        m = base.shared[0] if i in same else (base.shared[1] if i % 13 == 3 else base.msgs[i])
        items.append([base.pks[k], m, base.sig[(k, m)]])
    return items


# ---- tampers: each returns the touched positions; the product over the group is unchanged ----
def _g2(s): return O.signature_to_G2(s)
def _g1(p): return O.pubkey_to_G1(p)
def _add2(a, b): return O.pt_add(O.Fq2Ops, a, b)
def _add1(a, b): return O.pt_add(O.FqOps, a, b)


def tamper_swap(base, n, pos):
    a, b = pos[:2]
    items = clean_items(base, n, same=(a, b))
    items[a][2], items[b][2] = items[b][2], items[a][2]
    return items, (a, b)


def tamper_comp_sigs(base, n, pos):
    a, b = pos[:2]
    items = clean_items(base, n)
    assert items[a][0] != items[b][0] and items[a][1] != items[b][1]
    Dp = _g2(base.sig[(5, base.shared[0])])         # a third signature
    items[a][2] = O.G2_to_signature(_add2(_g2(items[a][2]), Dp))
    items[b][2] = O.G2_to_signature(_add2(_g2(items[b][2]), O.pt_neg(O.Fq2Ops, Dp)))
    return items, (a, b)


def tamper_comp_keys(base, n, pos):
    a, b = pos[:2]
    items = clean_items(base, n, same=(a, b))
    E = _g1(base.pks[(a + 5) % NKEYS])
    items[a][0] = O.G1_to_pubkey(_add1(_g1(items[a][0]), E))
    items[b][0] = O.G1_to_pubkey(_add1(_g1(items[b][0]), O.pt_neg(O.FqOps, E)))
    return items, (a, b)


def tamper_cycle3(base, n, pos):
    a, b, c = pos
    items = clean_items(base, n, same=pos)
    items[a][2], items[b][2], items[c][2] = items[b][2], items[c][2], items[a][2]
    return items, pos


TAMPERS = {"swap": (tamper_swap, 2), "comp_sigs": (tamper_comp_sigs, 2), "comp_keys": (tamper_comp_keys, 2),
           "cycle3": (tamper_cycle3, 3)}


def positions(B, n, k):
    """Named position groups of k items inside one sub-batch of B (those that fit)."""
    s = B if n >= 2 * B + 2 else 0          # the second sub-batch where there is one before the tail
    tail = (n + B - 1) // B * B - B
    out = {"one_quad": [s + 2, s + 3, s + 4][:k],             # (2q, 2q + 1): the two halves of one quad
           "next_quad": [s + 2, s + 4, s + 6][:k],            # (2q, 2q + 2)
           "ends": ([s, s + B - 1] if k == 2 else [s, s + B // 2, s + B - 1]),
           "ragged": list(range(tail, tail + k))}
    if B == 2:
        out["one_quad"] = [s, s + 1][:k]
    return {name: tuple(p) for name, p in out.items()
            if len(set(p)) == k and max(p) < n and len({i // B for i in p}) == 1}


def run_randomized(native, items, B, seed):
    import torch
    L = native.lib()
    n = len(items)
    dev = torch.device("cuda", 0)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d = [t(b"".join(it[0] for it in items)), t(b"".join(it[1] for it in items)), t(b"".join(it[2] for it in items)),
         t(DOM * n)]
    v = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(L.bls381_verify_batch_randomized_workspace_size(n, B), dtype=torch.uint8, device=dev)
    st = (ctypes.c_uint64 * 3)()
    stream = torch.cuda.current_stream(dev)
    native.check(L.bls381_verify_batch_randomized_device(n, *[x.data_ptr() for x in d], bytes(seed), B, v.data_ptr(),
                                                         ws.data_ptr(), ctypes.c_void_p(stream.cuda_stream), st))
    return v.cpu().numpy().astype(bool), list(st)


def per_item(native, items):
    n = len(items)
    return np.asarray(native.verify_batch(b"".join(it[0] for it in items), b"".join(it[1] for it in items),
                                          b"".join(it[2] for it in items), DOM * n)).astype(bool)


def test_positions_cover_the_issue():
    """CPU part of the case table: every sub-batch size has the quad pair, and every size above 2 the
    (2q, 2q + 2), first / last and ragged-tail groups, each inside one sub-batch, keys all different."""
    for B, n in SIZES.items():
        assert n <= NMAX and n % B != 0
        p2, p3 = positions(B, n, 2), positions(B, n, 3)
        assert "one_quad" in p2 and p2["one_quad"][0] % 2 == 0 and p2["one_quad"][1] == p2["one_quad"][0] + 1
        assert set(p2) == ({"one_quad", "ends"} if B == 2 else {"one_quad", "next_quad", "ends", "ragged"})
        assert set(p3) == (set() if B == 2 else {"one_quad", "next_quad", "ends"} | ({"ragged"} if B < 258 else set()))
        for grp in list(p2.values()) + list(p3.values()):
            assert len({i % NKEYS for i in grp}) == len(grp)
        if B > 2:
            a, b = p2["ends"]
            assert a % B == 0 and b % B == B - 1
            assert all(i >= n // B * B for i in p2["ragged"])


@pytest.mark.parametrize("policy", ["pyecc", "strict"])
@pytest.mark.parametrize("B", [2, 8, 64, 258])
def test_cancelling_tampers_are_rejected(native, base, B, policy):
    """Each tamper at each position group, under two seeds: the per-item pipeline's verdicts (False on
    exactly the touched items), and the statistics of exactly one failing sub-batch re-verified.  A
    false accept has probability <= 2^-63 per case."""
    n = SIZES[B]
    native.set_subgroup_policy(policy)
    try:
        clean = clean_items(base, n)
        assert len({it[0] for it in clean}) >= 8 and per_item(native, clean).all()
        assert n < 29 or len({it[1] for it in clean}) < n       # a group shares a message
        for seed in SEEDS:
            v, st = run_randomized(native, clean, B, seed)
            assert v.all() and st == [n, 0, 0], ("clean", st)
        ran = 0
        for name, (fn, k) in TAMPERS.items():
            for where, pos in positions(B, n, k).items():
                items, touched = fn(base, n, pos)
                want = per_item(native, items)
                assert list(want) == [i not in touched for i in range(n)], (name, where)
                failing = {i // B for i in touched}
                assert len(failing) == 1
                resent = sum(min(B, n - b * B) for b in failing)
                for seed in SEEDS:
                    v, st = run_randomized(native, items, B, seed)
                    ctx = (name, where, pos, st)
                    assert np.array_equal(v, want), ctx
                    assert st[2] == len(failing) and st[1] == resent and st[0] + st[1] == n, ctx
                    ran += 1
        assert ran == (2 * 3 * 2 if B == 2 else (2 * (3 * 4 + 3) if B == 258 else 2 * 4 * 4))
    finally:
        native.set_subgroup_policy("pyecc")


def test_cancelling_buckets_on_a_valid_batch(native, base):
    """(pk, m, sig) and (-pk, m, -sig) are both valid; side by side in a sub-batch of 8 their
    signatures meet in one bucket wherever their weights share a digit, and the bucket passes through
    infinity.  The model's digits (tests/rb_model.py) show such buckets for this seed before the GPU
    is asked; every sub-batch then passes."""
    B, n, seed = 8, 20, SEEDS[0]
    items = []
    for i in range(0, n, 2):
        pk, m, s = clean_items(base, n)[i]
        items.append([pk, m, s])
        items.append([O.G1_to_pubkey(O.pt_neg(O.FqOps, _g1(pk))), m, O.G2_to_signature(O.pt_neg(O.Fq2Ops, _g2(s)))])
    msm = RB.Msm([O.g2_affine(_g2(it[2])) for it in items], B, seed)
    assert len(msm.buckets_with_cancellation()) >= 1
    assert per_item(native, items).all()
    v, st = run_randomized(native, items, B, seed)
    assert v.all() and st == [n, 0, 0], st
