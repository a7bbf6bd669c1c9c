"""Plain-Python model of the two pubkey tables (csrc/bls381_keytable.hpp; k_reg_insert /
k_reg_lookup and k_deposit_insert / k_deposit_resolve), used by test_key_tables_host.py and
test_key_tables_gpu.py: the hash restated, its inversion in the last word (keys with a chosen
hash), the shape of a linear-probing table, the registry's entry rule, and the seeded inputs of
every GPU case (built here so that the CPU suite checks their chains with the compiled hash).

Why crafted keys are registrable: under the "pyecc" policy a pubkey with b_flag set decodes to
infinity whatever its other bytes (g1_decompress, lax), and an infinite pubkey with an infinite
signature verifies True (py_ecc's pairing with an infinite point)."""
import collections
import json
import os
import random

import bls_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
MUL = 0x85EBCA6B
MUL_INV = pow(MUL, -1, 1 << 32)
SEED = 0x9E3779B9


# ------------------------------------------------------------------ the hash
def _round(h: int, v: int) -> int:
    h = ((h ^ v) * MUL) & M32
    return h ^ (h >> 15)


def _hash_words(key: bytes, words: int) -> int:
    h = SEED
    for w in range(words):
        h = _round(h, int.from_bytes(key[4 * w:4 * w + 4], "little"))
    return h


def reg_hash(key48: bytes) -> int:
    """reg_hash of bls381_keytable.hpp: twelve little-endian words, h = (h ^ v) * MUL; h ^= h >> 15."""
    assert len(key48) == 48
    return _hash_words(key48, 12)


def craft_key(prefix44: bytes, target_hash: int) -> bytes:
    """The 48-byte key with this prefix whose reg_hash is target_hash: the last round inverted
    (x ^ x >> 15 is undone by x ^ x >> 15 ^ x >> 30; the multiplier is odd)."""
    assert len(prefix44) == 44 and 0 <= target_hash <= M32
    x = target_hash ^ (target_hash >> 15) ^ (target_hash >> 30)
    v = ((x * MUL_INV) & M32) ^ _hash_words(prefix44, 11)
    return bytes(prefix44) + v.to_bytes(4, "little")


def infinity_prefix(rng) -> bytes:
    """44 random bytes with b_flag (bit 6 of byte 0) set: c_flag, a_flag and the low bits random."""
    p = bytearray(rng.randbytes(44))
    p[0] |= 0x40
    return bytes(p)


def crafted_keys(rng, count: int, target_hash: int) -> list:
    """`count` distinct infinity keys with one hash; both c_flag values occur from 8 keys on."""
    keys = []
    while len(keys) < count:
        p = bytearray(infinity_prefix(rng))
        p[0] = (p[0] & 0x7F) | (0x80 if len(keys) % 2 else 0)
        k = craft_key(bytes(p), target_hash)
        if k not in keys:
            keys.append(k)
    return keys


# ------------------------------------------------------------- table shapes
def registry_table_slots(capacity: int) -> int:
    t = 1
    while t < 2 * capacity:
        t <<= 1
    return t


def deposit_table_slots(n: int) -> int:
    t = 16
    while t < 2 * n:
        t <<= 1
    return t


def occupied_slots(keys, slots: int, hash_fn=reg_hash) -> set:
    """The slots linear probing fills with the distinct keys of `keys` (equal keys share a slot).
    The set does not depend on the insertion order."""
    assert slots & (slots - 1) == 0
    occ = set()
    for k in dict.fromkeys(bytes(k) for k in keys):
        s = hash_fn(k) & (slots - 1)
        assert len(occ) < slots
        while s in occ:
            s = (s + 1) & (slots - 1)
        occ.add(s)
    return occ


ChainStats = collections.namedtuple("ChainStats", "longest_run wraps absent_walk")


def chain_stats(keys, slots: int, probe_hash=None, hash_fn=reg_hash) -> ChainStats:
    """longest_run: the longest cyclic run of occupied slots; wraps: a run covers slots - 1 and 0;
    absent_walk: occupied slots a lookup of an absent key with hash probe_hash compares before
    it meets an empty slot (None without probe_hash)."""
    occ = occupied_slots(keys, slots, hash_fn)
    assert len(occ) < slots

    def walk(s):
        n = 0
        while s in occ:
            s, n = (s + 1) & (slots - 1), n + 1
        return n
    starts = [s for s in occ if ((s - 1) & (slots - 1)) not in occ]
    longest = max((walk(s) for s in starts), default=0)
    wraps = (slots - 1) in occ and 0 in occ
    return ChainStats(longest, wraps, None if probe_hash is None else walk(probe_hash & (slots - 1)))


# ------------------------------------------------------------- the registry
def decodes(key48: bytes) -> bool:
    """The lax codec (py_ecc's decompress_G1) reads the key."""
    try:
        O.pubkey_to_G1(key48)
        return True
    except ValueError:
        return False


def registry_model(calls, decodes_fn=decodes) -> list:
    """Per `add` call the entries it returns.  Entry e is the e-th key ever added, decodable or
    not; a key's entry is that of the first key with its bytes among the keys that decode, -1
    for a key that does not."""
    first, size, out = {}, 0, []
    for keys in calls:
        res = []
        for k in keys:
            k = bytes(k)
            if k not in first and decodes_fn(k):
                first[k] = size
            res.append(first.get(k, -1))
            size += 1
        out.append(res)
    return out


# ------------------------------------------------- inputs of the GPU cases
# Every builder is seeded and engine-free; test_key_tables_host.py checks each one's chain
# condition, test_key_tables_gpu.py runs it.
PILE_HASH = 0xDEADBEEF
CAP = 2048                       # 4,096 slots


def golden_batches() -> dict:
    with open(os.path.join(ROOT, "tests", "golden", "bls_golden_batches.json")) as f:
        return json.load(f)


def case_pile():
    """1,024 keys of one hash and 256 absent keys of the same hash."""
    ks = crafted_keys(random.Random(0xB15_1001), 1024 + 256, PILE_HASH)
    return {"capacity": CAP, "keys": ks[:1024], "absent": ks[1024:], "absent_hash": PILE_HASH}


def case_wrap():
    """Eight keys on each of the slots mask - 7 .. mask, and 64 absent keys that start at mask."""
    rng = random.Random(0xB15_1002)
    mask = registry_table_slots(CAP) - 1
    keys = []
    for s in range(mask - 7, mask + 1):
        for _ in range(8):
            keys += crafted_keys(rng, 1, (rng.getrandbits(32) & ~mask & M32) | s)
    rng.shuffle(keys)
    absent_hash = (0x5A5A5A5A & ~mask) | mask
    absent = crafted_keys(rng, 64, absent_hash)
    return {"capacity": CAP, "keys": keys, "absent": absent, "absent_hash": absent_hash}


def case_equal_keys():
    """32 keys of one hash, 128 copies each, shuffled; then those 32 and 32 more of that hash."""
    rng = random.Random(0xB15_1003)
    ks = crafted_keys(rng, 64, 0x0BADC0DE)
    first = ks[:32] * 128
    rng.shuffle(first)
    second = ks[:32] + ks[32:]
    rng.shuffle(second)
    return {"capacity": 8192, "calls": [first, second], "distinct": ks}


def case_undecodable():
    """Keys no codec decodes (invalid_g1), each three times, among 24 one-hash keys and, per bad
    key, 8 crafted keys of the bad key's hash before and after it."""
    rng = random.Random(0xB15_1004)
    bad = [bytes.fromhex(h) for h in golden_batches()["invalid_g1"]]
    pile = crafted_keys(rng, 24, PILE_HASH)
    keys = []
    for i, b in enumerate(bad):
        same = crafted_keys(rng, 8, reg_hash(b))
        keys += same[:3] + [b] + pile[8 * i:8 * i + 4] + [b] + same[3:] + pile[8 * i + 4:8 * i + 8] + [b]
    return {"capacity": CAP, "keys": keys, "bad": bad}


_sk_rng = random.Random(0xB15_1005)
HONEST_SKS = [_sk_rng.randrange(1, 1 << 250) for _ in range(40)]


def case_decoded(honest_keys):
    """Per honest key (privtopub of HONEST_SKS) eight crafted infinity keys of its exact hash,
    k % 9 of them before it and the rest after it."""
    assert len(honest_keys) == 40
    rng = random.Random(0xB15_1006)
    keys, honest_pos = [], []
    for k, hk in enumerate(honest_keys):
        same = crafted_keys(rng, 8, reg_hash(hk))
        keys += same[:k % 9]
        honest_pos.append(len(keys))
        keys += [hk] + same[k % 9:]
    return {"capacity": CAP, "keys": keys, "honest_pos": honest_pos}


def case_exact_fill(capacity: int):
    """`capacity` keys: one-hash and random keys alternating."""
    rng = random.Random(0xB15_1007 + capacity)
    pile = crafted_keys(rng, capacity, 0x13572468)
    return [pile[i] if i % 2 == 0 else infinity_prefix(rng) + rng.randbytes(4) for i in range(capacity)]


GROWTH_HASH = 0x600DF00D


def case_growth():
    """Adds of 1, 127, 128 and 129 keys, then 36 single-key adds: one-hash and random keys mixed,
    with repeats of earlier keys.  Fills its registry exactly."""
    rng = random.Random(0xB15_1008)
    sizes = [1, 127, 128, 129] + [1] * 36
    pile = crafted_keys(rng, sum(sizes), GROWTH_HASH)
    calls, seen = [], []
    for n in sizes:
        call = []
        for _ in range(n):
            r = rng.random()
            if r < 0.5:
                k = pile.pop()
            else:
                k = rng.choice(seen) if seen and r < 0.6 else infinity_prefix(rng) + rng.randbytes(4)
            call.append(k)
            seen.append(k)
        calls.append(call)
    extra = crafted_keys(rng, 1, GROWTH_HASH)[0]
    return {"capacity": sum(sizes), "calls": calls, "extra": extra}


# -------------------------------------------------------------- deposits
DOMAIN = 3
FIRST = 2 ** 31 - 5              # the batches' tree indices carry across bit 31
DEP_HASH = 0xC0FFEE11
N_SHARED, KEYS_SHARED, REG_SHARED = 1000, 200, 50


_POINT_SIGS = None


def good_signature(rng, junk: bool) -> bytes:
    """An infinity encoding: 0xC0, then 95 bytes, zero or with junk in some of them."""
    s = bytearray(96)
    s[0] = 0xC0
    if junk:
        for _ in range(rng.randrange(1, 12)):
            s[rng.randrange(1, 96)] = rng.randrange(1, 256)
    return bytes(s)


def bad_signature(rng) -> bytes:
    """A golden valid signature of something else (a point, so never an infinity encoding)."""
    global _POINT_SIGS
    if _POINT_SIGS is None:
        sigs = [bytes.fromhex(c["signature"]) for c in golden_batches()["verify"] if c["expected"]]
        _POINT_SIGS = [s for s in sigs if not s[0] & 0x40]
        assert len(_POINT_SIGS) >= 10
    return rng.choice(_POINT_SIGS)


def deposit_data(rng, pubkey: bytes, amount: int, signature: bytes) -> bytes:
    return pubkey + rng.randbytes(32) + amount.to_bytes(8, "little") + signature


def _datas(rng, keys_of, good_of, n):
    sig_ok = [bool(good_of[t]) for t in range(n)]
    datas = [deposit_data(rng, keys_of[t], 32 * 10 ** 9 + t,
                          good_signature(rng, t % 3 == 1) if sig_ok[t] else bad_signature(rng)) for t in range(n)]
    return datas, sig_ok


def case_shared_hash():
    """1,000 deposits of 200 keys with one hash, 50 of them registered beforehand.  Keys 50-54
    carry the fixed patterns (positions below); every other position takes a random key and a
    signature that is good with probability 1/2."""
    rng = random.Random(0xB15_1009)
    keys = crafted_keys(rng, KEYS_SHARED, DEP_HASH)
    n = N_SHARED
    fixed = {
        # bad, good, good: SKIPPED, NEW, TOPUP
        3: (50, False), 40: (50, True), 77: (50, True),
        # good only / bad only
        130: (51, True), 131: (52, False), 600: (52, False),
        # a good deposit more than 128 positions after the first good one
        5: (53, True), 300: (53, True),
        # a good deposit in tile 4 (128-lane tiles of the scan) whose winner is in tile 1
        200: (54, True), 520: (54, True), 100: (54, False),
    }
    key_at, good_at = [None] * n, [None] * n
    for pos, (k, good) in fixed.items():
        key_at[pos], good_at[pos] = keys[k], good
    for pos in range(n):
        if key_at[pos] is None:
            k = rng.randrange(REG_SHARED) if rng.random() < 0.25 else rng.randrange(55, KEYS_SHARED)
            key_at[pos], good_at[pos] = keys[k], rng.random() < 0.5
    datas, sig_ok = _datas(rng, key_at, good_at, n)
    return {"keys": keys, "registered": keys[:REG_SHARED], "datas": datas, "sig_ok": sig_ok, "fixed": fixed,
            "table_keys": [key_at[t] for t in range(n) if sig_ok[t] and key_at[t] not in keys[:REG_SHARED]]}


DENSE_SIZES = (127, 128, 129, 513)


def case_dense_new(n: int):
    """n distinct keys, all signatures good: half on one hash, half on the last four slots of the
    batch table, so their chain runs across its end."""
    rng = random.Random(0xB15_100A + n)
    mask = deposit_table_slots(n) - 1
    pile = crafted_keys(rng, n // 2, 0x7E57AB1E)
    wrap = []
    for i in range(n - n // 2):
        wrap += crafted_keys(rng, 1, (rng.getrandbits(32) & ~mask & M32) | (mask - i % 4))
    keys = pile + wrap
    rng.shuffle(keys)
    assert len(set(keys)) == n
    datas, sig_ok = _datas(rng, keys, [True] * n, n)
    return {"keys": keys, "datas": datas, "sig_ok": sig_ok}


def case_all_skipped():
    """300 deposits of 60 one-hash keys, every signature bad; 10 more keys of that hash are
    registered, so every lookup walks their chain to an empty slot."""
    rng = random.Random(0xB15_100B)
    keys = crafted_keys(rng, 70, DEP_HASH)
    key_at = [keys[rng.randrange(60)] for _ in range(300)]
    datas, sig_ok = _datas(rng, key_at, [False] * 300, 300)
    return {"keys": keys[:60], "registered": keys[60:], "datas": datas, "sig_ok": sig_ok}


def all_case_keys(honest_keys) -> list:
    """Every key a GPU case adds, looks up or deposits (the CPU suite hashes each with the compiled
    reg_hash)."""
    keys = []
    for c in (case_pile(), case_wrap()):
        keys += c["keys"] + c["absent"]
    for c in (case_equal_keys(), case_growth()):
        keys += [k for call in c["calls"] for k in call]
    keys += [case_growth()["extra"]] + case_undecodable()["keys"] + case_decoded(honest_keys)["keys"]
    for cap in (1, 3, 128):
        keys += case_exact_fill(cap)
    keys += case_shared_hash()["keys"]
    for n in DENSE_SIZES:
        keys += case_dense_new(n)["keys"]
    c = case_all_skipped()
    keys += c["keys"] + c["registered"]
    return list(dict.fromkeys(keys))
