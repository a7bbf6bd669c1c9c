"""The pubkey tables on the CPU: the compiled hash and slot counts (csrc/bls381_keytable.hpp,
bls381_plan.hpp, host build) against their restatement in key_table_model.py, the hash's
inversion, and -- with the hash just checked -- the chain condition of every input that
test_key_tables_gpu.py runs, so that no GPU case can silently stop colliding."""
import ctypes
import os
import random

import pytest

import bls_oracle as O
import key_table_model as K

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_reg_hash.argtypes = [ctypes.c_char_p]
    lib.hc_reg_hash.restype = ctypes.c_uint32
    for f in (lib.hc_registry_table_slots, lib.hc_deposit_table_slots):
        f.argtypes = [ctypes.c_size_t]
        f.restype = ctypes.c_size_t
    return lib


@pytest.fixture(scope="module")
def honest():
    return [O.privtopub(sk) for sk in K.HONEST_SKS]


@pytest.fixture(scope="module")
def checked_hash(L, honest):
    """K.reg_hash, after every key of every GPU case hashed alike in the compiled function."""
    keys = K.all_case_keys(honest)
    assert len(keys) > 3000
    for k in keys:
        assert K.reg_hash(k) == L.hc_reg_hash(k), k.hex()
    return K.reg_hash


def stats(checked_hash, keys, slots, probe_hash=None):
    return K.chain_stats(keys, slots, probe_hash, hash_fn=checked_hash)


# ------------------------------------------------------------ hash and slots
def test_reg_hash_matches_compiled(L):
    rng = random.Random(0xB15_2001)
    keys = [rng.randbytes(48) for _ in range(1000)] + [b"\x00" * 48, b"\xff" * 48]
    for k in keys:
        assert K.reg_hash(k) == L.hc_reg_hash(k), k.hex()
    assert len({K.reg_hash(k) for k in keys}) > 990          # it is a hash, not a constant


def test_craft_key_hits_its_target(L):
    rng = random.Random(0xB15_2002)
    out = set()
    for _ in range(1000):
        prefix, target = rng.randbytes(44), rng.getrandbits(32)
        k = K.craft_key(prefix, target)
        assert k[:44] == prefix and len(k) == 48
        assert K.reg_hash(k) == target == L.hc_reg_hash(k)
        out.add(k)
    assert len(out) == 1000
    for target in (0, 1, 0xFFFFFFFF, 0x80000000, 0x7FFF):     # the xorshift's edge patterns
        assert L.hc_reg_hash(K.craft_key(b"\x40" + b"\x00" * 43, target)) == target
    keys = K.crafted_keys(rng, 64, 0xDEADBEEF)
    assert len(set(keys)) == 64 and {L.hc_reg_hash(k) for k in keys} == {0xDEADBEEF}


def test_infinity_prefix_flags():
    rng = random.Random(0xB15_2003)
    ps = [K.infinity_prefix(rng) for _ in range(64)]
    assert all(len(p) == 44 and p[0] & 0x40 for p in ps)
    assert {p[0] >> 7 for p in ps} == {0, 1} and {(p[0] >> 5) & 1 for p in ps} == {0, 1}
    keys = K.crafted_keys(rng, 16, 7)
    assert {k[0] >> 7 for k in keys} == {0, 1}                # c_flag clear and set
    assert all(K.decodes(k) and O.pt_is_inf(O._FqOps, O.pubkey_to_G1(k)) for k in keys)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 9, 1024, 1025, INT32_MAX // 2])
def test_slot_counts(L, n):
    r, d = L.hc_registry_table_slots(n), L.hc_deposit_table_slots(n)
    assert r == K.registry_table_slots(n) and d == K.deposit_table_slots(n)
    for t, floor in ((r, 1), (d, 16)):                        # a power of two >= 2 n: never a full table
        assert t & (t - 1) == 0 and t >= 2 * n and t >= floor and (t == floor or t // 2 < 2 * n)


# ------------------------------------------------------------------ the model
def test_occupied_slots_and_chain_stats():
    h = lambda k: k[0]                                        # the key's first byte is its hash
    key = lambda s, i=0: bytes([s, i]) + b"\x00" * 46
    keys = [key(6), key(6, 1), key(7), key(2), key(6)]        # slots 6, 7, 0 (wrapped), 2; one repeat
    assert K.occupied_slots(keys, 8, h) == {6, 7, 0, 2}
    assert K.occupied_slots(reversed(keys), 8, h) == {6, 7, 0, 2}
    st = K.chain_stats(keys, 8, 7, h)
    assert st == K.ChainStats(3, True, 2)
    assert K.chain_stats(keys, 8, 1, h).absent_walk == 0 and K.chain_stats(keys, 8, 2, h).absent_walk == 1
    assert K.chain_stats([], 8, 0, h) == K.ChainStats(0, False, 0)
    assert K.chain_stats([key(3), key(4)], 8, None, h) == K.ChainStats(2, False, None)


def test_registry_model():
    a, b, c, bad = b"a" * 48, b"b" * 48, b"c" * 48, b"x" * 48
    dec = lambda k: k != bad
    assert K.registry_model([[a, b, a, bad, c, bad], [c, a, bad, b"d" * 48]], dec) == \
        [[0, 1, 0, -1, 4, -1], [4, 0, -1, 9]]
    assert K.registry_model([], dec) == [] and K.registry_model([[]], dec) == [[]]


# ------------------------------------- chain conditions of the GPU inputs
def test_chain_pile(checked_hash):
    c = K.case_pile()
    slots = K.registry_table_slots(c["capacity"])
    assert slots == 4096 and len(set(c["keys"])) == 1024 and len(set(c["absent"]) - set(c["keys"])) == 256
    st = stats(checked_hash, c["keys"], slots, c["absent_hash"])
    assert st.longest_run >= 1024 and st.absent_walk == 1024  # an absent key compares the whole chain
    assert {checked_hash(k) for k in c["keys"] + c["absent"]} == {K.PILE_HASH}


def test_chain_wrap(checked_hash):
    c = K.case_wrap()
    slots = K.registry_table_slots(c["capacity"])
    mask = slots - 1
    starts = sorted(checked_hash(k) & mask for k in c["keys"])
    assert starts == sorted(list(range(mask - 7, mask + 1)) * 8) and len(set(c["keys"])) == 64
    st = stats(checked_hash, c["keys"], slots, c["absent_hash"])
    assert st.wraps and st.longest_run == 64
    assert c["absent_hash"] & mask == mask and st.absent_walk == 57   # mask, then 0 .. 55
    assert not set(c["absent"]) & set(c["keys"]) and {checked_hash(k) for k in c["absent"]} == {c["absent_hash"]}


def test_chain_equal_keys(checked_hash):
    c = K.case_equal_keys()
    slots = K.registry_table_slots(c["capacity"])
    first, second = c["calls"]
    assert len(first) == 4096 and len(set(first)) == 32 and all(first.count(k) == 128 for k in set(first))
    assert len(second) == 64 and len(set(second)) == 64 and len(set(second) - set(first)) == 32
    assert first[:128] != sorted(first)[:128]                 # shuffled
    assert len({checked_hash(k) for k in first + second}) == 1
    assert stats(checked_hash, first, slots).longest_run == 32
    assert stats(checked_hash, first + second, slots).longest_run == 64


def test_chain_undecodable(checked_hash):
    c = K.case_undecodable()
    slots = K.registry_table_slots(c["capacity"])
    good = [k for k in c["keys"] if k not in c["bad"]]
    assert len(c["bad"]) == 3 and not any(K.decodes(b) for b in c["bad"]) and all(K.decodes(k) for k in good)
    assert all(c["keys"].count(b) == 3 for b in c["bad"])
    assert stats(checked_hash, good, slots).longest_run >= 24
    for b in c["bad"]:                                        # a bad key's lookup walks its hash's chain
        assert stats(checked_hash, good, slots, checked_hash(b)).absent_walk >= 8


def test_chain_decoded(checked_hash, honest):
    c = K.case_decoded(honest)
    slots = K.registry_table_slots(c["capacity"])
    assert len(set(honest)) == 40 and len(c["keys"]) == len(set(c["keys"])) == 360
    before = [p - 9 * k for k, p in enumerate(c["honest_pos"])]
    assert min(before) == 0 and max(before) == 8              # crafted keys before and after
    for k, hk in enumerate(honest):
        assert c["keys"][c["honest_pos"][k]] == hk
        assert sum(checked_hash(x) == checked_hash(hk) for x in c["keys"]) >= 9
        assert stats(checked_hash, c["keys"], slots, checked_hash(hk)).absent_walk >= 9


def test_chain_sizes_and_growth(checked_hash):
    for cap in (1, 3, 128):
        keys = K.case_exact_fill(cap)
        assert len(keys) == len(set(keys)) == cap
        assert stats(checked_hash, keys, K.registry_table_slots(cap)).longest_run >= (cap + 1) // 2
    c = K.case_growth()
    sizes = [len(call) for call in c["calls"]]
    assert sizes[:4] == [1, 127, 128, 129] and set(sizes[4:]) == {1} and len(sizes) == 40
    assert sum(sizes) == c["capacity"]
    keys = [k for call in c["calls"] for k in call]
    piled = {k for k in keys if checked_hash(k) == K.GROWTH_HASH}
    assert len(piled) >= 150 and len(set(keys)) < len(keys) and len(set(keys) - piled) >= 100
    st = stats(checked_hash, keys, K.registry_table_slots(c["capacity"]), K.GROWTH_HASH)
    assert st.longest_run >= len(piled) and st.absent_walk >= len(piled)
    assert c["extra"] not in keys and checked_hash(c["extra"]) == K.GROWTH_HASH


def test_chain_shared_hash(checked_hash):
    c = K.case_shared_hash()
    n = len(c["datas"])
    assert n == 1000 and K.deposit_table_slots(n) == 2048
    assert len(set(c["keys"])) == 200 and {checked_hash(k) for k in c["keys"]} == {K.DEP_HASH}
    assert stats(checked_hash, c["registered"], K.registry_table_slots(1024), K.DEP_HASH).absent_walk == 50
    inserted = set(c["table_keys"])
    assert len(inserted) >= 100
    st = stats(checked_hash, c["table_keys"], 2048, K.DEP_HASH)
    assert st.longest_run == st.absent_walk == len(inserted)
    assert all(d[:48] in c["keys"] for d in c["datas"])
    assert all((d[88] & 0x40 != 0) == ok for d, ok in zip(c["datas"], c["sig_ok"]))
    assert any(ok and any(d[89:]) for d, ok in zip(c["datas"], c["sig_ok"]))      # junk in some


@pytest.mark.parametrize("n", K.DENSE_SIZES)
def test_chain_dense_new(checked_hash, n):
    c = K.case_dense_new(n)
    slots = K.deposit_table_slots(n)
    assert len(c["keys"]) == len(set(c["keys"])) == n and all(c["sig_ok"])
    st = stats(checked_hash, c["keys"], slots)
    assert st.wraps and st.longest_run >= n // 2
    starts = {checked_hash(k) & (slots - 1) for k in c["keys"]}
    assert len(starts) == 5 and {slots - 4, slots - 3, slots - 2, slots - 1} <= starts


def test_chain_all_skipped(checked_hash):
    c = K.case_all_skipped()
    assert len(c["datas"]) == 300 and not any(c["sig_ok"]) and not set(c["keys"]) & set(c["registered"])
    assert stats(checked_hash, c["registered"], K.registry_table_slots(1024), K.DEP_HASH).absent_walk == 10
