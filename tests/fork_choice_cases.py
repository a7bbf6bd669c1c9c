"""Crafted cases of the fork choice, shared by test_fork_choice_host.py and test_fork_choice_gpu.py.

A case is a script: a list of calls on a store, run on the model (fork_choice_model.py) for the
expected results and on a backend (the host build, the sanitizer program's text form, the engine's
host and device forms) for the results to compare.  Calls:
  ("S", validator_capacity, block_capacity)             a new store
  ("B", roots, parent_roots, slots)                     -> node ids, or None when rejected
  ("A", att_off, entries, slots, targets, ok or None)   -> members skipped, or None
  ("L", first, n)                                       -> (slots, targets), or None
  ("P", node)                                           -> True, or None
  ("H", start, activation, exit, effective, epoch)      -> (head, head root, counts, status), or None
"""
import hashlib
import importlib.util
import os
import random

import fork_choice_model as M

NONE = M.NONE
FAR = 2 ** 64 - 1
ETH = 10 ** 9
EPOCH = 20
# the bounds the kernels have (csrc/bls381_forkchoice.hpp, csrc/bls381_epoch.hpp)
VALIDATOR_TILE = 2048   # ACTIVE_TILE: validators a workgroup of k_fc_direct takes
NODE_BINS = 2048        # FC_BINS: nodes a workgroup sums in LDS
SCAN_TILE = 256         # FC_SCAN_TILE: nodes a round of k_fc_scan takes


def golden_maker():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_fork_choice_vectors.py")
    spec = importlib.util.spec_from_file_location("make_fork_choice_vectors", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- running a script --------------------------------------------------------------------------------
class ModelBackend:
    def create(self, vcap, bcap):
        self.s = M.Store(vcap, bcap)

    def add_blocks(self, roots, parents, slots):
        return self.s.add_blocks(roots, parents, slots)

    def on_attestations(self, att_off, entries, slots, targets, ok):
        return self.s.on_attestations(att_off, entries, slots, targets, ok)

    def latest(self, first, n):
        return self.s.latest(first, n)

    def prune(self, node):
        return self.s.prune(node)

    def head(self, start, act, ext, eff, epoch):
        got = self.s.head(start, act, ext, eff, epoch)
        return None if got is None else (got[0], self.s.root[got[0]], got[1], got[2])


def run_script(script, backend):
    out = []
    for call in script:
        tag, args = call[0], call[1:]
        if tag == "S":
            backend.create(*args)
            out.append(None)
        else:
            out.append({"B": backend.add_blocks, "A": backend.on_attestations, "L": backend.latest, "P": backend.prune,
                        "H": backend.head}[tag](*args))
    return out


def expected(script):
    return run_script(script, ModelBackend())


# ---- trees: lists of (root, parent index, slot) -------------------------------------------------------
def root(seed, i):
    return hashlib.sha256(b"block %d %d" % (seed, i)).digest()


def chain_tree(count, seed=1):
    return [(root(seed, i), i - 1 if i else NONE, 100 + i) for i in range(count)]


def comb_tree(count, seed=2):
    """A chain with a leaf at every node: even ids the spine, odd ids the leaves."""
    blocks = []
    for i in range(count):
        spine = i - 2 if i % 2 == 0 else i - 1
        blocks.append((root(seed, i), spine if i else NONE, 100 + i))
    return blocks


def random_tree(count, seed=3):
    rng = random.Random(seed)
    blocks = [(root(seed, 0), NONE, 100)]
    for i in range(1, count):
        p = rng.randrange(i) if rng.random() < 0.2 else rng.randrange(max(0, i - 6), i)
        blocks.append((root(seed, i), p, blocks[p][2] + rng.choice([1, 1, 2, 5])))
    return blocks


def star_tree(count, seed=4):
    return [(root(seed, i), 0 if i else NONE, 100 + (i > 0)) for i in range(count)]


def add_call(blocks, first=0):
    part = blocks[first:]
    return ("B", [b[0] for b in part], [blocks[b[1]][0] if b[1] != NONE else bytes(32) for b in part], [b[2] for b in part])


def registry(n, seed=5, plain=False):
    """(activation, exit, effective): mostly active at EPOCH, with pending, exited and empty ones."""
    rng = random.Random(seed)
    act, ext, eff = [], [], []
    for i in range(n):
        kind = "active" if plain else rng.choice(["active"] * 7 + ["pending", "exited", "zero"])
        act.append(rng.choice([EPOCH + 1, FAR]) if kind == "pending" else rng.choice([0, 5, EPOCH]))
        ext.append(rng.choice([EPOCH, 3]) if kind == "exited" else rng.choice([FAR, EPOCH + 1]))
        eff.append(0 if kind == "zero" else rng.choice([32, 32, 31, 17]) * ETH)
    return act, ext, eff


def batch(groups):
    """("A", ...) from (slot, target, members) triples."""
    off, entries = [0], []
    for _, _, members in groups:
        entries += list(members)
        off.append(len(entries))
    return ("A", off, entries, [g[0] for g in groups], [g[1] for g in groups], None)


def spread_votes(n, n_blocks, seed=6, per_att=97, targets=None):
    """Every validator below n once, in attestations of per_att members on random (or given) targets."""
    rng = random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)
    groups = []
    for k in range(0, n, per_att):
        t = targets[(k // per_att) % len(targets)] if targets else rng.randrange(n_blocks)
        groups.append((300, t, order[k:k + per_att]))
    return batch(groups)


def head_script(n, blocks, votes, start=0, seed=5, vcap=None, plain=False):
    return [("S", vcap or max(1, n), max(1, len(blocks))), add_call(blocks), votes,
            ("H", start) + registry(n, seed, plain) + (EPOCH,)]


# ---- the golden scenarios as scripts --------------------------------------------------------------------
def golden_script(sc):
    n = len(sc["validators"])
    v = sc["validators"]
    return [("S", n, len(sc["blocks"])), add_call(sc["blocks"]), batch(sc["log"]), ("L", 0, n),
            ("H", sc["start"], [x.activation_epoch for x in v], [x.exit_epoch for x in v], [x.effective_balance for x in v],
             EPOCH)]


# ---- latest messages ----------------------------------------------------------------------------------------
def latest_cases():
    blocks = random_tree(12, seed=11)
    n = 40
    reg = registry(n, 12, plain=True)
    tail = [("L", 0, n), ("H", 0) + reg + (EPOCH,)]
    out = {}
    # one validator in many attestations of one batch, at equal and at different slots
    out["one validator, equal slots in one batch"] = [("S", n, 12), add_call(blocks), batch(
        [(200, t, [7, 1 + t]) for t in (3, 9, 5, 11, 2)])] + tail
    out["one validator, different slots in one batch"] = [("S", n, 12), add_call(blocks), batch(
        [(s, t, [7, 20 + t]) for s, t in ((200, 3), (205, 9), (203, 5), (205, 11), (199, 2))])] + tail
    # across two batches: the later batch loses at the same slot and wins at a higher one
    out["two batches"] = [("S", n, 12), add_call(blocks), batch([(200, 4, [1, 2, 3]), (201, 5, [4])]),
                          batch([(200, 6, [1, 2]), (201, 7, [3, 4]), (150, 8, [5, 1])])] + tail
    out["every member on one validator"] = [("S", n, 12), add_call(blocks), batch(
        [(200, 4, [9] * 70), (200, 5, [9] * 3), (210, 6, [9] * 130), (210, 7, [9])])] + tail
    out["entries out of range"] = [("S", n, 12), add_call(blocks), batch(
        [(200, 4, [1, n, 2, n + 5, NONE]), (201, 5, [n - 1, 2 ** 31])])] + tail
    a = batch([(200, 4, [1, 2, 3]), (205, 5, [1, 2, n + 1]), (203, 6, [2, 3]), (207, 7, [])])
    out["verdicts with failures"] = [("S", n, 12), add_call(blocks), a[:5] + ([1, 0, 1, 0],),
                                     batch([(203, 8, [3, 1])])] + tail   # the failed ones took their seq
    out["the largest slot"] = [("S", n, 12), add_call(blocks), batch([(2 ** 32 - 1, 4, [1, 2]), (5, 5, [2, 3])]),
                               batch([(2 ** 32 - 1, 6, [1, 3])])] + tail
    out["empty attestations and an empty batch"] = [("S", n, 12), add_call(blocks), batch([]), batch(
        [(200, 4, []), (200, 5, [1]), (200, 6, []), (200, 7, []), (201, 8, [1, 2])])] + tail
    return out


def rejected_cases():
    """Every script ends with the state read back: the rejected call changed nothing."""
    blocks = random_tree(8, seed=21)
    n = 10
    reg = registry(n, 22, plain=True)
    base = [("S", n, 8), add_call(blocks[:6]), batch([(200, 3, [1, 2]), (201, 5, [2])])]
    tail = [("L", 0, n), ("H", 0) + reg + (EPOCH,)]
    out = {}
    out["a slot of 2^32"] = base + [batch([(200, 1, [4]), (2 ** 32, 2, [5])])] + tail
    out["an unknown target"] = base + [batch([(200, 1, [4]), (200, 6, [5])])] + tail
    out["descending offsets"] = base + [("A", [0, 2, 1], [4, 5], [200, 200], [1, 2], None)] + tail
    out["an unknown parent"] = base + [("B", [blocks[6][0], root(9, 9)], [blocks[blocks[6][1]][0], root(9, 8)],
                                        [blocks[6][2], 500])] + tail
    out["a slot not above the parent's"] = base + [("B", [root(9, 1)], [blocks[2][0]], [blocks[2][2]])] + tail
    out["more blocks than the capacity"] = base + [("B", [root(9, i) for i in range(3)], [blocks[0][0]] * 3, [400] * 3)] + tail
    out["start outside the tree"] = base + [("H", 6) + reg + (EPOCH,)] + tail
    out["more validators than the capacity"] = base + [("H", 0) + registry(n + 1, 22, plain=True) + (EPOCH,)] + tail
    out["latest past the capacity"] = base + [("L", 5, n - 4)] + tail
    out["prune outside the tree"] = base + [("P", 6)] + tail
    return out


# ---- votes ----------------------------------------------------------------------------------------------------
def tie_roots(which):
    """Three children of one anchor whose roots differ in one byte only: the last, or the first."""
    base = bytearray(root(31, 0))
    roots = []
    for x in (0x10, 0xF0, 0x7F):
        r = bytearray(base)
        r[31 if which == "last" else 0] = x
        roots.append(bytes(r))
    return [(root(31, 1), NONE, 100)] + [(r, 0, 101) for r in roots]


def vote_cases():
    out = {}
    for which in ("last", "first"):
        blocks = tie_roots(which)
        n = 9
        out["equal counts, roots differ in the %s byte" % which] = [
            ("S", n, 4), add_call(blocks), batch([(200, 1 + k % 3, [k]) for k in range(n)]),
            ("H", 0, [0] * n, [FAR] * n, [32 * ETH] * n, EPOCH)]
    blocks = random_tree(20, seed=32)
    n = 300
    out["all on one node"] = head_script(n, blocks, batch([(200, 19, list(range(n)))]))
    out["spread over every node"] = head_script(n, blocks, batch([(200, b, list(range(b, n, 20))) for b in range(20)]))
    # two votes of 2^63 on one tip: its count, the fork's and the anchor's pass 2^64 - 1
    blocks = chain_tree(3, seed=33) + [(root(33, 9), 1, 110)]
    out["a sum that wraps"] = [("S", 4, 4), add_call(blocks), batch([(200, 2, [0, 1]), (200, 3, [2]), (200, 0, [3])]),
                              ("H", 0, [0] * 4, [FAR] * 4, [2 ** 63, 2 ** 63, 2 ** 63, 5], EPOCH)]
    out["sums at the edge"] = [("S", 4, 4), add_call(blocks), batch([(200, 2, [0, 1]), (200, 3, [2]), (200, 1, [3])]),
                               ("H", 0, [0] * 4, [FAR] * 4, [2 ** 63, 2 ** 63 - 1, 2 ** 32 - 1, 2 ** 32 + 1], EPOCH)]
    blocks = random_tree(40, seed=34)
    out["start in the middle"] = head_script(200, blocks, spread_votes(200, 40, per_att=7), start=17)
    out["no validators"] = head_script(0, blocks, batch([]), vcap=3)
    out["one block"] = head_script(5, chain_tree(1), batch([(200, 0, [0, 1, 2, 3, 4])]))
    return out


def prune_cases():
    """The pruned store against a fresh store fed the surviving blocks and the same log: both in
    one script (the second S starts the fresh one), compared by test_prune_matches_fresh_store."""
    blocks = random_tree(30, seed=41)
    n = 120
    reg = registry(n, 42)
    votes = spread_votes(n, 30, seed=43, per_att=5)
    anchor = 4
    return [("S", n, 30), add_call(blocks), votes, ("H", 0) + reg + (EPOCH,), ("P", anchor), ("L", 0, n),
            ("H", 0) + reg + (EPOCH,), add_call_after_prune(blocks, anchor), batch([(400, 1, [0, 1, 2])]),
            ("H", 0) + reg + (EPOCH,)], blocks, votes, reg, anchor


def add_call_after_prune(blocks, anchor):
    """One more block below the new anchor, by roots (ids have moved)."""
    return ("B", [root(41, 999)], [blocks[anchor][0]], [blocks[anchor][2] + 50])


def surviving(blocks, anchor):
    """(kept blocks renumbered, old -> new)"""
    new = {}
    for i in range(anchor, len(blocks)):
        if i == anchor or blocks[i][1] in new:
            new[i] = len(new)
    kept = [(blocks[i][0], NONE if i == anchor else new[blocks[i][1]], blocks[i][2]) for i in sorted(new)]
    return kept, new


# ---- sizes: every bound the kernels have ------------------------------------------------------------------------
def validator_size_cases():
    blocks = random_tree(33, seed=51)
    T = VALIDATOR_TILE
    return {"%d validators" % n: head_script(n, blocks, spread_votes(n, 33, seed=52 + n % 7), vcap=max(n, 1))
            for n in (0, 1, T - 1, T, T + 1, 2 * T + 1)}


def block_size_cases():
    out = {}
    n = 600
    for count in (1, 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, NODE_BINS - 1, NODE_BINS, NODE_BINS + 1):
        blocks = random_tree(count, seed=60 + count % 5)
        out["%d blocks" % count] = head_script(n, blocks, spread_votes(n, count, seed=61, per_att=3))
    chain = chain_tree(1025)
    out["a chain of 1025"] = head_script(n, chain, spread_votes(n, 1025, seed=62, per_att=3))
    out["a chain of 1025, no votes"] = head_script(n, chain, batch([]))
    comb = comb_tree(601)
    out["a comb"] = head_script(n, comb, spread_votes(n, 601, seed=63, per_att=3))
    out["a comb, start in the middle"] = head_script(n, comb, spread_votes(n, 601, seed=63, per_att=3), start=300)
    out["a star"] = head_script(n, star_tree(300), spread_votes(n, 300, seed=64, per_att=2))
    out["votes on the last bins of two node tiles"] = head_script(
        n, random_tree(NODE_BINS + 9, seed=65), spread_votes(n, 0, seed=66, per_att=11,
                                                              targets=[NODE_BINS - 1, NODE_BINS, NODE_BINS + 8, 0, 2047, 2049]))
    return out


def large_registry_case():
    n = 70001
    blocks = random_tree(96, seed=71)
    return head_script(n, blocks, spread_votes(n, 96, seed=72, per_att=1024, targets=list(range(80, 96)) + [3, 40]), vcap=n)


def small_cases():
    """The latest-message, rejected, vote and prune scripts: what the host tests and the sanitizer
    program run beside the sized and the random ones."""
    out = {}
    out.update(latest_cases())
    out.update(rejected_cases())
    out.update(vote_cases())
    out["prune"] = prune_cases()[0]
    return out


def random_scripts(count, seed=81):
    rng = random.Random(seed)
    out = []
    for k in range(count):
        n, nb = rng.randrange(1, 90), rng.randrange(1, 50)
        blocks = random_tree(nb, seed=seed * 1000 + k)
        script = [("S", n, nb + 2), add_call(blocks)]
        for _ in range(rng.randrange(1, 4)):
            groups = [(rng.choice([200, 200, 201, 250]), rng.randrange(nb), [rng.randrange(n + 2) for _ in range(rng.randrange(0, 9))])
                      for _ in range(rng.randrange(0, 12))]
            a = batch(groups)
            script.append(a[:5] + ([rng.randrange(4) > 0 for _ in groups],) if rng.random() < 0.3 else a)
        script += [("L", 0, n), ("H", rng.randrange(nb)) + registry(n, seed + k) + (EPOCH,)]
        if rng.random() < 0.4:
            script += [("P", rng.randrange(nb)), ("L", 0, n), ("H", 0) + registry(n, seed + k) + (EPOCH,)]
        out.append(script)
    return out
