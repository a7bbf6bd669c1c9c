"""Pin the fork choice to the reference's own spec text: tests/golden/fork_choice.json.

As make_registry_updates_vectors.py does for the registry updates, this script takes the functions
mechanically from the spec's text: get_ancestor and lmd_ghost from the ```python blocks of
specs/core/0_fork-choice.md, slot_to_epoch and is_active_validator from those of
specs/core/0_beacon-chain.md, pulled by the fence rule of the reference's extractor
(scripts/function_puller.py:40-44) and run unmodified.  What the text leaves open is supplied here
and named in the output ("supplied"):
  * Store: an object whose get_parent(block) is the block's parent in the scenario's tree
  * get_children(store, block): the blocks whose parent is `block`, in the order they were added
  * hash_tree_root(block): the block's given root
  * get_latest_attestation_target(store, index): from the scenario's ordered attestation log by the
    prose rule of 0_fork-choice.md:71-72 (the highest slot; among equal slots the one observed
    first); a validator without an attestation gets a block of slot -1 that is in no tree, which
    get_ancestor turns into None at every slot
  * get_active_validator_indices(validators, epoch): over the text's own is_active_validator
    (lmd_ghost calls it with the registry list; the beacon-chain text's version takes the state)
  * the annotation names, and SLOTS_PER_EPOCH / FAR_FUTURE_EPOCH of the minimal preset

Scenarios: KINDS x 1, 7, 64 and 301 validators, at most 64 blocks each:
  * tie: two chains from the anchor whose tips get pairs of equal votes, so every count ties and
    the root decides
  * heavy_second: the first child holds the largest direct vote, the second child's subtree more
  * outside: the start block in the middle of the tree; votes for its ancestors and for forks
    outside its subtree
  * mixed: a random tree; validators not yet active, exited, without a message and with balance 0;
    several attestations per validator at equal and at different slots

Stored per scenario: the head (node and root), the vote count of every block -- the expression of
the text's get_vote_count, over the text's get_ancestor, evaluated per block -- and the latest
(slot, target) per validator.  The inputs are rebuilt from `seed` by scenario() below, which
tests/fork_choice_cases.py repeats; the blocks and, from 301 validators on, the validators, the log
and the latest messages are stored as SHA-256 digests.  None of the spec's text is stored.

Run (where the reference checkout exists: beside the repository, or at $BLS381_REFERENCE):
    python tests/golden/make_fork_choice_vectors.py
"""
import hashlib
import json
import os
import random
import re
import struct
import sys
import types
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BLS381_REFERENCE") or os.path.join(HERE, "..", "..", "..", "reference")   # beside the repository
FORK_CHOICE = ("specs/core/0_fork-choice.md", ("get_ancestor", "lmd_ghost"))
BEACON_CHAIN = ("specs/core/0_beacon-chain.md", ("slot_to_epoch", "is_active_validator"))
CONSTANTS = ("SLOTS_PER_EPOCH", "FAR_FUTURE_EPOCH")
SUPPLIED = ("Store.get_parent", "get_children", "hash_tree_root", "get_latest_attestation_target",
            "get_active_validator_indices")
EPOCH = 20
SIZES = (1, 7, 64, 301)
KINDS = ("tie", "heavy_second", "outside", "mixed")
DIGEST_FROM = 301
NONE = 0xFFFFFFFF
ETH = 10 ** 9
FAR = 2 ** 64 - 1


def pull_blocks(path, wanted):
    blocks, cur = [], None
    for line in open(os.path.join(REF, path)).readlines():
        line = line.rstrip()
        if line[:9] == "```python":
            cur = []
        elif line[:3] == "```":
            if cur is not None:
                blocks.append("\n".join(cur))
            cur = None
        elif cur is not None:
            cur.append(line)
    picked = {}
    for b in blocks:
        m = re.match(r"def (\w+)\(", b)
        if m and m.group(1) in wanted:
            assert m.group(1) not in picked, m.group(1)
            picked[m.group(1)] = b
    assert sorted(picked) == sorted(wanted), sorted(set(wanted) - set(picked))
    return "\n\n".join(picked[name] for name in wanted)


def constants():
    text = open(os.path.join(REF, "configs", "constant_presets", "minimal.yaml")).read()
    return {name: int(re.search(r"^%s:\s*(\d+)" % name, text, re.M).group(1)) for name in CONSTANTS}


# ---- scenarios (repeated by tests/fork_choice_cases.py) ------------------------------------------
def root_of(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


def chain(rng, blocks, parent, length):
    """Appends `length` blocks below block `parent`; returns the tip's index."""
    for _ in range(length):
        blocks.append((root_of(rng), parent, blocks[parent][2] + rng.choice([1, 1, 2, 3])))
        parent = len(blocks) - 1
    return parent


def random_tree(rng, count):
    blocks = [(root_of(rng), NONE, 8 * EPOCH - 30)]
    while len(blocks) < count:
        parent = rng.randrange(len(blocks)) if rng.random() < 0.3 else rng.randrange(max(0, len(blocks) - 4), len(blocks))
        chain(rng, blocks, parent, 1)
    return blocks


def validator(rng, kind="active"):
    v = types.SimpleNamespace(activation_epoch=rng.choice([0, 3, EPOCH]), exit_epoch=rng.choice([FAR, FAR, EPOCH + 1, EPOCH + 9]),
                              effective_balance=rng.choice([32, 32, 31, 24, 17]) * ETH)
    if kind == "pending":
        v.activation_epoch = rng.choice([EPOCH + 1, EPOCH + 5, FAR])
    elif kind == "exited":
        v.exit_epoch = rng.choice([EPOCH, EPOCH - 1, 4])
    elif kind == "zero":
        v.effective_balance = 0
    return v


def scenario(seed, n, kind):
    """blocks: (root, parent index or NONE, slot) in insertion order; validators; log: (slot, target
    block index, member validator indices) in the order observed; start: the start block's index."""
    rng = random.Random(seed)
    log = []
    start = 0
    if kind == "tie":
        blocks = [(root_of(rng), NONE, 100)]
        tips = [chain(rng, blocks, 0, rng.randrange(1, 6)), chain(rng, blocks, 0, rng.randrange(1, 6))]
        # a second tie further down the winning side is decided by the roots again
        for side in (0, 1):
            tips.append(chain(rng, blocks, tips[side], 2))
            tips.append(chain(rng, blocks, tips[side], 1))
        validators = [validator(rng) for _ in range(n)]
        for v in validators:
            v.activation_epoch, v.exit_epoch = 0, FAR
        for k in range(0, n - 1, 2):   # pairs of equal votes, one a side, at the same depth
            validators[k + 1].effective_balance = validators[k].effective_balance
            which = rng.choice([(2, 4), (3, 5), (0, 1)])
            log.append((blocks[tips[which[0]]][2], tips[which[0]], [k]))
            log.append((blocks[tips[which[1]]][2], tips[which[1]], [k + 1]))
        if n % 2:
            validators[n - 1].effective_balance = 0   # a vote that weighs nothing keeps the tie
            log.append((blocks[tips[0]][2], tips[0], [n - 1]))
    elif kind == "heavy_second":
        blocks = [(root_of(rng), NONE, 50)]
        first = chain(rng, blocks, 0, 1)
        second = chain(rng, blocks, 0, 1)
        leaves = [chain(rng, blocks, second, rng.randrange(1, 4)) for _ in range(min(6, max(2, n // 2)))]
        validators = [validator(rng) for _ in range(n)]
        for i in range(n):
            validators[i].activation_epoch, validators[i].exit_epoch, validators[i].effective_balance = 0, FAR, 32 * ETH
            target = first if i % 3 == 0 else leaves[i % len(leaves)]   # every third vote on the first child itself
            log.append((blocks[target][2], target, [i]))
    else:
        blocks = random_tree(rng, rng.randrange(24, 65))
        kinds = ["active"] * 6 + ["pending", "exited", "zero", "silent"]
        drawn = [kinds[i % len(kinds)] if n >= 64 else rng.choice(kinds) for i in range(n)]
        validators = [validator(rng, k) for k in drawn]
        if kind == "outside":
            start = len(blocks) // 2
        voters = [i for i in range(n) if drawn[i] != "silent"]
        for _ in range(3):   # three rounds: equal and different slots per validator, in observed order
            rng.shuffle(voters)
            at = 0
            while at < len(voters):
                members = voters[at:at + rng.randrange(1, 9)]
                at += len(members)
                target = rng.randrange(len(blocks))
                slot = blocks[target][2] + rng.choice([0, 0, 1, 4])
                log.append((slot, target, sorted(members)))
    return {"blocks": blocks, "validators": validators, "log": log, "start": start}


def digest(words):
    return hashlib.sha256(struct.pack("<%dQ" % len(words), *words)).hexdigest()


def blocks_digest(blocks):
    return hashlib.sha256(b"".join(r + struct.pack("<QQ", p, s) for r, p, s in blocks)).hexdigest()


def validator_words(validators):
    return [x for v in validators for x in (v.activation_epoch, v.exit_epoch, v.effective_balance)]


def log_words(log):
    return [x for slot, target, members in log for x in [slot, target, len(members)] + list(members)]


# ---- the text, run ---------------------------------------------------------------------------------
def run_spec(code, consts, extra):
    ns = {"List": typing.List}
    ns.update({name: object for name in ("Store", "BeaconState", "BeaconBlock", "Validator")})
    ns.update({name: int for name in ("Epoch", "Slot", "ValidatorIndex")})
    ns.update(consts)
    ns.update(extra)
    exec(compile(code, "spec text", "exec"), ns)   # noqa: S102 -- the reference's own spec text
    return ns


def run_scenario(code, consts, sc):
    blocks = [types.SimpleNamespace(root=r, parent=p, slot=s, index=i) for i, (r, p, s) in enumerate(sc["blocks"])]
    silent = types.SimpleNamespace(root=None, parent=NONE, slot=-1, index=NONE)
    latest = {}
    for slot, target, members in sc["log"]:   # 0_fork-choice.md:71: the highest slot, the first one observed
        for i in members:
            if i not in latest or slot > latest[i][0]:
                latest[i] = (slot, target)

    class Store:
        def get_parent(self, block):
            return blocks[block.parent]

    def get_active_validator_indices(validators, epoch):
        return [i for i, v in enumerate(validators) if spec["is_active_validator"](v, epoch)]

    spec = run_spec(code, consts, {
        "get_children": lambda store, block: [b for b in blocks if b.parent == block.index],
        "hash_tree_root": lambda block: block.root,
        "get_latest_attestation_target": lambda store, i: blocks[latest[i][1]] if i in latest else silent,
        "get_active_validator_indices": get_active_validator_indices})
    store = Store()
    state = types.SimpleNamespace(validator_registry=sc["validators"], slot=EPOCH * consts["SLOTS_PER_EPOCH"] + 3)
    assert spec["slot_to_epoch"](state.slot) == EPOCH
    head = spec["lmd_ghost"](store, state, blocks[sc["start"]])
    # get_vote_count's expression per block, over the text's get_ancestor and is_active_validator
    targets = [(i, spec["get_latest_attestation_target"](store, i))
               for i in get_active_validator_indices(sc["validators"], EPOCH)]
    counts = [sum(sc["validators"][i].effective_balance for i, t in targets if spec["get_ancestor"](store, t, b.slot) == b)
              for b in blocks]
    n = len(sc["validators"])
    return head, counts, [latest.get(i, (0, NONE))[0] for i in range(n)], [latest.get(i, (0, NONE))[1] for i in range(n)]


def main():
    sys.setrecursionlimit(10000)   # get_ancestor recurses once per block of a chain
    code = pull_blocks(*BEACON_CHAIN) + "\n\n" + pull_blocks(*FORK_CHOICE)
    consts = constants()
    out = {"source": "%s: %s; %s: %s" % (FORK_CHOICE[0], ", ".join(FORK_CHOICE[1]), BEACON_CHAIN[0], ", ".join(BEACON_CHAIN[1])),
           "supplied": list(SUPPLIED), "constants": consts, "epoch": EPOCH, "digest_from": DIGEST_FROM, "scenarios": []}
    for k, (kind, n) in enumerate((kind, n) for kind in KINDS for n in SIZES):
        seed = 9100 + k
        sc = scenario(seed, n, kind)
        assert len(sc["blocks"]) <= 64
        head, counts, latest_slot, latest_target = run_scenario(code, consts, sc)
        full = n < DIGEST_FROM
        out["scenarios"].append({
            "kind": kind, "n": n, "seed": seed, "n_blocks": len(sc["blocks"]), "start": sc["start"],
            "blocks": blocks_digest(sc["blocks"]),
            "validators": validator_words(sc["validators"]) if full else digest(validator_words(sc["validators"])),
            "log": log_words(sc["log"]) if full else digest(log_words(sc["log"])),
            "head": head.index, "head_root": head.root.hex(), "vote_counts": counts,
            "latest_slot": latest_slot if full else digest(latest_slot),
            "latest_target": latest_target if full else digest(latest_target)})
    path = os.path.join(HERE, "fork_choice.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
