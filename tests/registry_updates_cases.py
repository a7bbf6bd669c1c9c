"""Crafted registries for the registry updates (tests/test_registry_updates_host.py and
tests/test_registry_updates_gpu.py): each case is a dict of the five field arrays (numpy uint64),
`cur`, `fin` and the constants `c` (the spec's names), built at the smallest size at which the thing
it is named for can go wrong.  The expected results come from tests/registry_updates_model.py.
"""
import importlib.util
import os
import random

import numpy as np

import registry_updates_model as M

FAR = M.FAR
ETH = 10 ** 9
CUR, FIN = 100, 90           # delayed(CUR) = 105, delayed(FIN) = 95 with the presets' delay of 4
DELAYED_CUR, DELAYED_FIN = 105, 95
TILE = 2048
FIELDS = ("elig", "act", "ext", "wd", "eff")


def golden_maker():
    """tests/golden/make_registry_updates_vectors.py as a module (its registry() rebuilds the inputs
    of the states stored as digests)."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_registry_updates_vectors.py")
    spec = importlib.util.spec_from_file_location("make_registry_updates_vectors", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Case(dict):
    """n active validators with nothing to do; the methods make some of them something else."""

    def __init__(self, name, n, cur=CUR, fin=FIN, **overrides):
        super().__init__(name=name, n=n, cur=cur, fin=fin, c=dict(M.MAINNET, **overrides),
                         elig=np.zeros(n, np.uint64), act=np.zeros(n, np.uint64), ext=np.full(n, FAR, np.uint64),
                         wd=np.full(n, FAR, np.uint64), eff=np.full(n, 32 * ETH, np.uint64))

    def low(self, *idx):            # at the ejection balance
        for i in idx:
            self["eff"][i] = 16 * ETH
        return self

    def exited(self, epoch, *idx):
        for i in idx:
            self["ext"][i] = epoch
            self["wd"][i] = min(FAR, epoch + 256)
        return self

    def queued(self, key, *idx, act=FAR):   # in the activation queue with eligibility epoch `key`
        for i in idx:
            self["elig"][i], self["act"][i] = key, act
        return self

    def deposit(self, *idx, eff=32 * ETH):  # no eligibility epoch yet
        for i in idx:
            self["elig"][i], self["act"][i], self["eff"][i] = FAR, FAR, eff
        return self

    def lists(self):
        return [[int(x) for x in self[f]] for f in FIELDS]

    def expected(self):
        """The model's (indices, values, summary), or None for arguments the call rejects."""
        if "_want" not in self:
            self["_want"] = M.registry_updates(*self.lists(), self["cur"], self["fin"], self["c"])
        return self["_want"]


def size_cases():
    """Every size at which the tiles end differently, each with ejections and a queue longer than the limit."""
    out = [Case("n=0", 0)]
    for n in (1, 2047, 2048, 2049, 4097):
        c = Case("n=%d" % n, n)
        rng = random.Random(n)
        picks = sorted(set([0, n - 1, n // 2] + [rng.randrange(n) for _ in range(min(n, 24))]))
        for t, i in enumerate(picks):
            if t % 3 == 0:
                c.low(i)
            elif t % 3 == 1:
                c.queued(rng.choice([50, 60, 60, 70]), i)
            else:
                c.exited(rng.choice([104, 105, 107, 107]), i)
        out.append(c)
    return out


def second_scan_round_case():
    """257 tiles: the second round of the tile scan.  Ejections and candidates on both sides of tile 256."""
    n = 256 * TILE + 1
    c = Case("n=%d" % n, n)
    c.low(5, 255 * TILE + 7, 256 * TILE - 1, 256 * TILE)
    c.exited(107, 9, 256 * TILE - 2)
    c.queued(60, 3, 4000, 255 * TILE + 1, 256 * TILE - 3).queued(60, 256 * TILE - 4).queued(55, 256 * TILE - 5)
    c.queued(61, 100, 200, 300, 400, 500).deposit(256 * TILE - 6)
    # tile 256 is validator 256 * TILE alone: ejected above, and here a candidate that is activated
    # already.  With L = 7 its pair (60, 256 * TILE) is the seventh smallest, the threshold itself: it
    # takes the place that validator 100 would get if the second round's candidate offset were wrong.
    c.queued(60, 256 * TILE, act=DELAYED_FIN)
    return c


def exit_queue_cases(L=4):
    """The exit queue before the call (no exited validator; its peak below, at and above delayed(cur);
    0, L - 1, L, L + 3 validators on it) times the number of ejections."""
    out = []
    n = 128
    for peak in (None, DELAYED_CUR - 1, DELAYED_CUR, DELAYED_CUR + 2):
        for c0 in ((0,) if peak is None else (L - 1, L, L + 3)):
            for ejections in sorted({0, 1, max(0, L - c0), max(0, L - c0) + 1, 3 * L + 1}):
                c = Case("peak=%s c0=%d ejections=%d" % (peak, c0, ejections), n)
                if peak is not None:
                    c.exited(peak, *range(100, 100 + c0)).exited(peak - 1, 120, 121).exited(3, 122)
                c.low(*[2 + 5 * k for k in range(ejections)])
                out.append(c)
    return out


def ejection_edge_cases():
    a = Case("ejected across tile edges", 4097).low(2046, 2047, 2048, 2049, 4095, 4096).exited(105, 7, 8, 9)
    b = Case("at the ejection balance: exiting, not active", 64).low(3, 4, 5, 6).exited(120, 4)
    b["act"][5] = CUR + 1                     # not active yet
    b["ext"][6], b["wd"][6] = CUR, CUR + 256  # no longer active
    return [a, b]


def activation_queue_cases(L=4):
    out = []
    for K in (0, L - 1, L, L + 1):
        out.append(Case("K=%d" % K, 64).queued(50, *range(10, 10 + K)))
    out.append(Case("equal keys across the threshold, two tiles", 4097).queued(50, *range(2045, 2051)).queued(51, 5, 4090))
    out.append(Case("dequeued entries that are activated already", 64)
               .queued(10, 5, 6, act=DELAYED_FIN).queued(11, 7, act=CUR + 2).queued(12, 20, 21, 22))
    out.append(Case("activation_epoch at and below delayed(finalized)", 64)
               .queued(10, 5, act=DELAYED_FIN).queued(10, 6, act=DELAYED_FIN - 1).queued(12, 20, 21, 22, 23))
    out.append(Case("eligible in this call and dequeued", 64).deposit(9, 11).deposit(13, eff=31 * ETH).queued(50, 30))
    out.append(Case("eligible in this call, beyond the limit", 64).deposit(9, 11).queued(50, 30, 31, 32))
    b7 = Case("keys that differ in byte 7", 64)
    for t, i in enumerate((40, 12, 33, 7, 21, 50)):
        b7.queued(((t * 37 % 11) + 1) << 56, i)
    b4 = Case("keys that differ in byte 4", 64)
    for t, i in enumerate((40, 12, 33, 7, 21, 50)):
        b4.queued((9 << 56) | (((t * 5 % 7) + 1) << 32), i)
    b0 = Case("keys that differ in byte 0", 64)
    for t, i in enumerate((40, 12, 33, 7, 21, 50)):
        b0.queued((9 << 56) | (3 << 32) | ((t * 3 % 7) + 1), i)
    mixed = Case("keys that differ in bytes 7, 4 and 0", 64)
    for i, key in zip((8, 9, 10, 11, 12, 13, 14), ((5 << 56) | 7, (5 << 56) | (1 << 32), 5 << 56, (5 << 56) | 1, 6 << 56,
                                                   (5 << 56) | (1 << 32) | 1, 4 << 56)):
        mixed.queued(key, i)
    out += [b7, b4, b0, mixed]
    out.append(Case("key 2^64 - 2", 64).queued(FAR - 1, 3, 4, 5).queued(FAR - 2, 30, 31, 32))
    out.append(Case("indices that differ above bit 8", 4097).queued(50, 3, 3 + 256, 3 + 512, 3 + 1024, 3 + 2048, 3 + 4096 - 256))
    return out


def churn_limit_cases():
    twelve = Case("L=12 with quotient 16", 322, CHURN_LIMIT_QUOTIENT=16)
    twelve.exited(50, *range(222, 322))       # 222 in front, 22 of them queued: 200 active, 200 // 16 = 12
    twelve.exited(107, 200, 201).low(*range(0, 60, 2)).queued(40, *range(61, 100, 2)).queued(39, 150, 151)
    big = Case("L above 256", 2049, CHURN_LIMIT_QUOTIENT=4)
    rng = random.Random(11)
    big.queued(0, *range(1, 2049, 3))         # 683 queued, 1,366 active: L = 341
    for i in range(1, 2049, 3):
        big["elig"][i] = rng.choice([20, 21, 22, 23, 24])
    big.low(*range(0, 2049, 6))               # 342 ejections: L + 1
    every = Case("L >= K with quotient 1", 300, CHURN_LIMIT_QUOTIENT=1).queued(30, *range(0, 300, 7)).low(1, 2, 3)
    return [twelve, big, every]


def overflow_cases():
    a = Case("one wrapping exit_epoch", 64).exited(FAR - 1, 10, 11, 12, 13).low(3)
    b = Case("exit epochs at and past 2^64 - 1", 64).exited(FAR - 1, 10, 11, 12).low(3, 4, 5, 6, 7, 8)
    c = Case("a withdrawable_epoch that wraps alone", 64).exited(FAR - 200, 10).low(3)
    return [a, b, c]


def rejected_cases():
    """BLS381_EARG: the model returns None."""
    return [Case("delayed(cur) wraps", 8, cur=FAR - 4), Case("delayed(cur) wraps by one", 8, cur=FAR),
            Case("delayed(finalized) wraps", 8, fin=FAR - 4), Case("quotient 0", 8, CHURN_LIMIT_QUOTIENT=0),
            Case("no churn limit", 8, MIN_PER_EPOCH_CHURN_LIMIT=0, CHURN_LIMIT_QUOTIENT=16),
            Case("no churn limit that the data shows", 64, MIN_PER_EPOCH_CHURN_LIMIT=0, CHURN_LIMIT_QUOTIENT=16)
            .exited(5, *range(10, 64))]


def random_cases(count, seed=1):
    """Small random registries around CUR: churn limits between 1 and the active count, queue churn
    below, at and above the limit."""
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n = rng.randrange(1, 40)
        c = Case("random %d" % k, n, fin=rng.choice([80, 90, 94, 99]), MIN_PER_EPOCH_CHURN_LIMIT=rng.choice([1, 1, 2, 4]),
                 CHURN_LIMIT_QUOTIENT=rng.choice([1, 2, 3, 8, 65536]))
        for i in range(n):
            kind = rng.randrange(8)
            if kind == 0:
                c.low(i)
            elif kind == 1:
                c.exited(rng.choice([3, 104, 105, 106, 106, 107]), i)
            elif kind == 2:
                c.queued(rng.choice([40, 41, 41, 42, CUR]), i, act=rng.choice([FAR, FAR, FAR, 95, 94, 101]))
            elif kind == 3:
                c.deposit(i, eff=rng.choice([32, 32, 31]) * ETH)
            elif kind == 4:
                c.low(i).exited(rng.choice([106, 107, 200]), i)
        out.append(c)
    return out


def all_accepted_cases():
    return (size_cases() + exit_queue_cases() + ejection_edge_cases() + activation_queue_cases() + churn_limit_cases() +
            overflow_cases())
