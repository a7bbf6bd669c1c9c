"""Batches for hash_to_G2's device searches, composed from tests/golden/hash_search.json by trial
count (tests/test_hash_search_host.py proves what they reach, tests/test_hash_search_gpu.py runs them).

The pooled search (dev_hash_cand_1) works per 64-lane wave, two waves per workgroup: what it does is
decided by which lanes hold unresolved items after each round.  The wide search (k_hash_search<16>)
gives each item 16 lanes, four items per wave: a second round needs an item of 17 trials or more.
`wave_trace` runs the model (tests/pooled_search_model.py) over the fixture's square masks.
"""
import hashlib
import json
import os
import random

from pooled_search_model import pooled_search

HERE = os.path.dirname(os.path.abspath(__file__))


class Msg:
    def __init__(self, fx, rec):
        self.i, self.trials, self.squares = rec["i"], rec["trials"], int(rec["squares"], 16)
        self.msg = hashlib.sha256(fx["tag"].encode() + self.i.to_bytes(4, "big")).digest()
        self.point = None      # the fixture's oracle record, where it stores one


class Fixture:
    def __init__(self):
        with open(os.path.join(HERE, "golden", "hash_search.json")) as f:
            self.raw = json.load(f)
        self.domain = self.raw["domain"]
        self.dom8 = self.domain.to_bytes(8, "big")
        self.messages = [Msg(self.raw, r) for r in self.raw["messages"]]
        self.by_i = {m.i: m for m in self.messages}
        for p in self.raw["points"]:
            self.by_i[p["i"]].point = p
        self.max_trials = max(m.trials for m in self.messages)

    def pool(self, points_only=False):
        """trial count -> messages, lowest i first (points_only: those with an oracle record)."""
        by = {}
        for m in self.messages:
            if m.point is not None or not points_only:
                by.setdefault(m.trials, []).append(m)
        return by

    def length_message(self, n):
        return (hashlib.sha256(self.raw["tag"].encode() + b"/len" + bytes([n])).digest() * 4)[:n]


_FX = []


def fixture():
    if not _FX:
        _FX.append(Fixture())
    return _FX[0]


class Picker:
    """Messages by trial count from a pool, cycling through those of one count (so a composition
    holds distinct messages where the pool has enough, and keeps its trial counts where it has not)."""

    def __init__(self, by):
        self.by, self.at = by, {}

    def __call__(self, t, pred=None):
        c = [m for m in self.by[t] if pred is None or pred(m)] or self.by[t]
        j = self.at.get((t, pred), 0)
        self.at[(t, pred)] = j + 1
        return c[j % len(c)]

    def at_least(self, t):
        """Every message of t trials or more, the trial counts ascending."""
        return [m for u in sorted(self.by) if u >= t for m in self.by[u]]


def _bit2(m):
    return (m.squares >> 2) & 1 == 1


def _no_bit2(m):
    return not _bit2(m)


M40_ONE_TRIAL_LANES = (2, 5, 7)      # lane % 8: the 24 one-trial lanes of the m = 40 wave


def pooled_compositions(by):
    """[(name, [Msg])]: the waves of section "Pooled" -- what each is for is asserted from the
    model in tests/test_hash_search_host.py."""
    fx = fixture()
    out = []
    high = Picker(by).at_least(fx.max_trials)[0]
    out.append(("lone_high", [high]))
    for t in range(1, 7):
        p = Picker(by)
        out.append(("all_%d" % t, [p(t) for _ in range(64)]))
    for lane in (0, 31, 63):
        p = Picker(by)
        w = [p(1) for _ in range(64)]
        w[lane] = high
        out.append(("high_at_%d" % lane, w))
    # round 2 at m = 3: 22 / 21 / 21 lanes
    p = Picker(by)
    w = [p(1) for _ in range(64)]
    w[5], w[20], w[41] = p(2), p.at_least(17)[0], p.at_least(18)[0]
    out.append(("three_left", w))
    # round 2 at m = 40: ranks 0..23 own two lanes (offsets 1, 2), ranks 24..39 one (offset 1)
    p = Picker(by)
    ranks = ([p(3) for _ in range(8)]                 # two lanes: the first square on the second
             + [p(2, _bit2) for _ in range(8)]        # squares on both lanes: the first is the item's
             + [p(2, _no_bit2) for _ in range(8)]
             + [p(2) for _ in range(8)]               # one lane: resolved
             + [p(t) for t in (3, 4, 5, 6, 7, 9, 12, 15)])   # one lane: fail again
    w, it = [], iter(ranks)
    for lane in range(64):
        w.append(p(1) if lane % 8 in M40_ONE_TRIAL_LANES else next(it))
    out.append(("forty_left", w))
    # partial last waves and a second workgroup: the high-trial items in the last wave
    every = [m for t in sorted(by) for m in by[t]]
    for n in (65, 127, 129, 200):
        rng = random.Random(n)
        w = [rng.choice(every) for _ in range(n)]
        tail = Picker(by).at_least(16)
        last = n - 1 - (n - 1) % 64          # first item of the last wave
        for j, m in enumerate(tail[-(n - last):]):
            w[n - 1 - j] = m
        out.append(("n_%d" % n, w))
    for seed in range(4):
        rng = random.Random(0x5EA2C4 + seed)
        out.append(("mix_%d" % seed, [rng.choice(every) for _ in range(256)]))
    return out


WIDE_TRIALS = (1, 2, 15, 16, 17, 18)


def wide_compositions(by):
    """[(name, [Msg])]: four items per wave of k_hash_search<16>."""
    fx = fixture()
    out = []
    p = Picker(by)
    w = []
    for t in WIDE_TRIALS + (fx.max_trials,):
        for pos in range(4):
            wave = [p(1) for _ in range(4)]
            wave[pos] = p(t)
            w += wave
    out.append(("positions", w))
    out.append(("all_second_round", p.at_least(17)[-4:]))
    for n in (1, 3, 5, 9):
        p = Picker(by)
        w = [p(1) for _ in range(n)]
        w[n - 1] = p.at_least(17)[-1 - n % 3]     # the partial last wave goes into a second round
        out.append(("n_%d" % n, w))
    return out


Q = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def x0_of(msg, dom8):
    """The first candidate x of msg || dom8 (bls_signature.md:74-80), from hashlib."""
    return (int.from_bytes(hashlib.sha256(msg + dom8 + b"\x01").digest(), "big") % Q,
            int.from_bytes(hashlib.sha256(msg + dom8 + b"\x02").digest(), "big") % Q)


def on_twist_with_selected_root(x, y):
    """y^2 == x^3 + 4(1 + i) in Fp2, and y is the root the spec selects of (y, -y): the greater
    imaginary part, then the greater real part (bls_signature.md:99-108)."""
    (a, b), (c, d) = x, y
    x2 = ((a * a - b * b) % Q, 2 * a * b % Q)
    x3 = ((x2[0] * a - x2[1] * b + 4) % Q, (x2[0] * b + x2[1] * a + 4) % Q)
    if ((c * c - d * d) % Q, 2 * c * d % Q) != x3:
        return False
    nc, nd = -c % Q, -d % Q
    return d > nd or (d == nd and c > nc)


G1_KEY = bytes.fromhex("97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb")


def valid_items(msgs):
    """[[pk, msg, sig]] with pk = the G1 generator (privtopub(1)) and sig = hash_to_G2(msg) from the
    fixture: e(H, g1) = e(H, g1), valid with no signing involved."""
    return [[G1_KEY, m.msg, bytes.fromhex(m.point["compressed"])] for m in msgs]


def spoil(items, msgs, where):
    """The signatures at `where` replaced by the hash built from the next square offset (even
    positions of `where`) or the negated hash (odd ones); returns the expected verdicts."""
    for k, i in enumerate(where):
        items[i][2] = bytes.fromhex(msgs[i].point["negated_sig" if k % 2 else "next_square_sig"])
    return [i not in where for i in range(len(items))]


def wave_trace(wave):
    """The model over one wave of at most 64 messages: (found offsets of its items, [m of each round])."""
    valid = [lane < len(wave) for lane in range(64)]
    trace = []
    # offsets of 64 or more are past the masks; no decision reads them: a round tests an item's
    # offsets in ascending order from one at or below its first square, which is below 64
    found, rounds = pooled_search(lambda i, o: o < 64 and (wave[i].squares >> o) & 1 == 1, valid, trace)
    assert rounds == len(trace)
    return found[:len(wave)], trace


def waves_of(items):
    return [items[k:k + 64] for k in range(0, len(items), 64)]
