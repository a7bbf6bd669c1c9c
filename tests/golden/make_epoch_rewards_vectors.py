"""Pin the epoch rewards to the reference's own spec text: tests/golden/epoch_rewards.json.

As make_epoch_context_vectors.py does for the epoch context, this script takes the functions
mechanically from the spec's text: the ```python blocks of specs/core/0_beacon-chain.md that define
the names in WANTED, pulled by the fence rule of the reference's extractor
(scripts/function_puller.py:40-44) and run unmodified over states built from namespaces.  What
the text leaves to its surroundings is supplied here and named in the output:
  * hash = SHA-256 (0_beacon-chain.md:591-595)
  * the constants of configs/constant_presets/{minimal,mainnet}.yaml named in CONSTANTS, and
    GENESIS_EPOCH = GENESIS_SLOT // SLOTS_PER_EPOCH
  * the annotation names (BeaconState, Validator, AttestationData, PendingAttestation = object;
    Epoch, Slot, Shard, Gwei, ValidatorIndex = int; Bytes32 = bytes; List, Tuple = typing's)
  * Crosslink: a class of the five fields of :304-316 (shard, start_epoch, end_epoch, parent_root,
    data_root), all zero by default, equal when the five fields are equal
  * hash_tree_root: a stand-in, SHA-256 over a tag and the fields of a Crosslink (only equality
    matters: :1312-1315 compares roots), over the packed indices for the active index list and
    over a tag for the HistoricalBatch stub
  * HistoricalBatch: a stub holding its two arguments; the state lists process_final_updates
    touches besides the effective balances (eth1_data_votes, latest_active_index_roots,
    latest_slashed_balances, latest_randao_mixes, latest_state_roots, historical_roots) are filled
    with tagged hashes and zeros

States: minimal-preset states of 1, 7, 64 and 301 validators and one mainnet-preset state of 301,
at the last slot of epoch 9, so that the previous epoch is 8; finalized_epoch is 3 or 4, on both
sides of MIN_EPOCHS_TO_INACTIVITY_PENALTY.  The registries mix active, not yet active, exited and
slashed validators (active slashed ones attest; exited slashed ones are eligible while
previous_epoch + 1 < withdrawable_epoch; some meet process_slashings' condition), balances of 0 and
a few Gwei that a penalty takes to 0, and balances around the hysteresis thresholds.  The
previous epoch's attestations follow a pattern per committee (PATTERNS): none; one; three with
overlapping bitfields, equal inclusion delays and different proposers; two candidates with equal
balances and different data_roots; two with equal balances and the same data_root; only
attestations that fail the parent_root / hash_tree_root filter (on shard 0 one of them equals
Crosslink()); mismatched target and head roots.  Proposers include slashed and not eligible
validators.  A separate block per state ("hysteresis") runs process_final_updates alone over
balances on both sides of each threshold.

Stored: the inputs, and as outputs the rewards and penalties of get_attestation_deltas and
get_crosslink_deltas, the balances after process_rewards_and_penalties, process_slashings and
process_final_updates, the effective balances, the per-shard winners with both balances, and the
three attesting balances; the per-validator outputs of the 301-validator states as SHA-256
digests of the lists packed as little-endian uint64.  None of the spec's text is stored.

Run (where the reference checkout exists: beside the repository, or at $BLS381_REFERENCE):
    python tests/golden/make_epoch_rewards_vectors.py
"""
import copy
import hashlib
import json
import os
import random
import re
import struct
import types
import typing

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("BLS381_REFERENCE") or os.path.join(HERE, "..", "..", "..", "reference")   # beside the repository
SPEC = os.path.join(REF, "specs", "core", "0_beacon-chain.md")
WANTED = ("int_to_bytes", "bytes_to_int", "integer_squareroot", "slot_to_epoch", "get_previous_epoch",
          "get_current_epoch", "get_epoch_start_slot", "is_active_validator", "get_active_validator_indices",
          "increase_balance", "decrease_balance", "get_epoch_committee_count", "get_shard_delta",
          "get_epoch_start_shard", "get_attestation_data_slot", "get_block_root_at_slot", "get_block_root",
          "get_randao_mix", "get_active_index_root", "generate_seed", "get_shuffled_index", "compute_committee",
          "get_crosslink_committee", "get_bitfield_bit", "verify_bitfield", "get_attesting_indices", "get_total_balance",
          "get_total_active_balance", "get_matching_source_attestations", "get_matching_target_attestations",
          "get_matching_head_attestations", "get_unslashed_attesting_indices", "get_attesting_balance",
          "get_winning_crosslink_and_attesting_indices", "get_base_reward", "get_attestation_deltas",
          "get_crosslink_deltas", "process_rewards_and_penalties", "process_slashings", "process_final_updates")
CONSTANTS = ("SHARD_COUNT", "TARGET_COMMITTEE_SIZE", "SHUFFLE_ROUND_COUNT", "MAX_EFFECTIVE_BALANCE",
             "EFFECTIVE_BALANCE_INCREMENT", "FAR_FUTURE_EPOCH", "GENESIS_SLOT", "SLOTS_PER_EPOCH", "MIN_SEED_LOOKAHEAD",
             "ACTIVATION_EXIT_DELAY", "SLOTS_PER_ETH1_VOTING_PERIOD", "SLOTS_PER_HISTORICAL_ROOT",
             "MIN_ATTESTATION_INCLUSION_DELAY", "MIN_EPOCHS_TO_INACTIVITY_PENALTY", "LATEST_RANDAO_MIXES_LENGTH",
             "LATEST_ACTIVE_INDEX_ROOTS_LENGTH", "LATEST_SLASHED_EXIT_LENGTH", "BASE_REWARD_FACTOR",
             "BASE_REWARDS_PER_EPOCH", "PROPOSER_REWARD_QUOTIENT", "INACTIVITY_PENALTY_QUOTIENT",
             "MIN_SLASHING_PENALTY_QUOTIENT")
EPOCH = 9
STATES = [("minimal", 1, 3), ("minimal", 7, 4), ("minimal", 64, 3), ("minimal", 301, 4), ("mainnet", 301, 3)]
PATTERNS = ("none", "one", "overlap", "tie_roots", "tie_same_root", "fail_filter", "mismatch")
ETH = 10 ** 9
DIGEST_FROM = 301   # per-validator outputs of states this large are stored as digests


def pull_blocks():
    blocks, cur = [], None
    for line in open(SPEC).readlines():
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
        if m and m.group(1) in WANTED:
            assert m.group(1) not in picked, m.group(1)
            picked[m.group(1)] = b
    assert sorted(picked) == sorted(WANTED), sorted(set(WANTED) - set(picked))
    return "\n\n".join(picked[name] for name in WANTED)


def constants(preset):
    text = open(os.path.join(REF, "configs", "constant_presets", preset + ".yaml")).read()
    return {name: int(re.search(r"^%s:\s*(\d+)" % name, text, re.M).group(1)) for name in CONSTANTS}


class Crosslink:
    FIELDS = ("shard", "start_epoch", "end_epoch", "parent_root", "data_root")

    def __init__(self, shard=0, start_epoch=0, end_epoch=0, parent_root=bytes(32), data_root=bytes(32)):
        self.shard, self.start_epoch, self.end_epoch = shard, start_epoch, end_epoch
        self.parent_root, self.data_root = parent_root, data_root

    def key(self):
        return tuple(getattr(self, f) for f in self.FIELDS)

    def __eq__(self, other):
        return isinstance(other, Crosslink) and self.key() == other.key()

    def __hash__(self):
        return hash(self.key())

    def stored(self):
        return [self.shard, self.start_epoch, self.end_epoch, self.parent_root.hex(), self.data_root.hex()]


class HistoricalBatch:
    def __init__(self, block_roots, state_roots):
        self.block_roots, self.state_roots = block_roots, state_roots


def hash_tree_root(value):
    if isinstance(value, Crosslink):
        return hashlib.sha256(b"crosslink" + struct.pack("<QQQ", value.shard, value.start_epoch, value.end_epoch) +
                              value.parent_root + value.data_root).digest()
    if isinstance(value, HistoricalBatch):
        return hashlib.sha256(b"historical batch").digest()
    return hashlib.sha256(b"indices" + b"".join(struct.pack("<Q", i) for i in value)).digest()


def run_spec(code, consts):
    ns = {"hash": lambda b: hashlib.sha256(b).digest(), "List": typing.List, "Tuple": typing.Tuple, "Bytes32": bytes,
          "Crosslink": Crosslink, "HistoricalBatch": HistoricalBatch, "hash_tree_root": hash_tree_root}
    ns.update({name: object for name in ("BeaconState", "Validator", "AttestationData", "PendingAttestation")})
    ns.update({name: int for name in ("Epoch", "Slot", "Shard", "Gwei", "ValidatorIndex")})
    ns.update(consts)
    ns["GENESIS_EPOCH"] = consts["GENESIS_SLOT"] // consts["SLOTS_PER_EPOCH"]
    exec(compile(code, SPEC, "exec"), ns)   # noqa: S102 -- the reference's own spec text
    return ns


def tagged(tag, *numbers):
    return hashlib.sha256(tag + struct.pack("<%dQ" % len(numbers), *numbers)).digest()


def registry(rng, n, c):
    """Validators around EPOCH: most are active in the previous and the current epoch; the rest are of the
    kinds in `special`."""
    far, half = c["FAR_FUTURE_EPOCH"], c["LATEST_SLASHED_EXIT_LENGTH"] // 2
    out = []
    special = ["pending", "joining", "exited", "leaving", "slashed_active", "slashed_active", "slashed_exited",
               "slashed_exited", "slashed_done", "slashed_due"]
    for i in range(n):
        kind = rng.choice(["active"] * 12 + special)
        if n >= 32:                             # every kind is there: one validator in five takes the next one
            kind = special[i // 5 % len(special)] if i % 5 == 3 else "active"
        if n == 1:
            kind = "active"
        v = types.SimpleNamespace(activation_epoch=0, exit_epoch=far, withdrawable_epoch=far, slashed=False)
        if kind == "pending":
            v.activation_epoch = far
        elif kind == "joining":                 # active from the current epoch on
            v.activation_epoch = EPOCH
        elif kind == "exited":
            v.exit_epoch, v.withdrawable_epoch = EPOCH - 3, EPOCH + 200
        elif kind == "leaving":                 # active in the previous epoch only
            v.exit_epoch, v.withdrawable_epoch = EPOCH, EPOCH + 256
        elif kind == "slashed_active":
            v.slashed, v.exit_epoch = True, EPOCH + 2
            v.withdrawable_epoch = EPOCH + rng.choice([half, half, 2 * half])
        elif kind == "slashed_exited":          # eligible: previous_epoch + 1 < withdrawable_epoch
            v.slashed, v.exit_epoch = True, EPOCH - 2
            v.withdrawable_epoch = rng.choice([EPOCH + 1, EPOCH + half, EPOCH + half, EPOCH + half + 1])
        elif kind == "slashed_done":            # not eligible: withdrawable at previous_epoch + 1 or before
            v.slashed, v.exit_epoch = True, EPOCH - 4
            v.withdrawable_epoch = rng.choice([EPOCH, EPOCH - 1])
        elif kind == "slashed_due":
            v.slashed, v.exit_epoch, v.withdrawable_epoch = True, EPOCH - 1, EPOCH + half
        v.kind = kind
        v.effective_balance = rng.choice([32, 32, 32, 32, 31, 24, 17, 16, 1, 0]) * ETH
        out.append(v)
    return out


def start_balances(rng, validators):
    out = []
    for v in validators:
        e = v.effective_balance
        out.append(rng.choice([e, e, e + 1, e + ETH // 3, e + 3 * ETH // 2 - 40000, e + 3 * ETH // 2 + 40000, e + 2 * ETH,
                               max(e, 20000) - 20000, max(e, ETH) - ETH, 0, 1, 1000, 99999]))
    return out


def hysteresis_balances(validators, c):
    inc = c["EFFECTIVE_BALANCE_INCREMENT"]
    edges = [0, 1, -1, inc // 2, 3 * (inc // 2) - 1, 3 * (inc // 2), 3 * (inc // 2) + 1, 2 * inc, -inc, -inc - 1, 5 * inc]
    return [max(0, v.effective_balance + edges[i % len(edges)]) for i, v in enumerate(validators)]


def bitfield(bits):
    out = bytearray((len(bits) + 7) // 8)
    for i, b in enumerate(bits):
        if b:
            out[i // 8] |= 1 << (i % 8)
    return bytes(out)


def attestations(rng, ns, c, state, prev, shards, committees):
    """The previous epoch's pending attestations, one pattern per committee."""
    n = len(state.validator_registry)
    target_root = ns["get_block_root"](state, prev)
    wrong = tagged(b"wrong root", 0)
    special = [i for i, v in enumerate(state.validator_registry) if v.kind in ("slashed_active", "slashed_done", "pending")]
    atts, patterns = [], []
    for k, (shard, members) in enumerate(zip(shards, committees)):
        pattern = PATTERNS[k % len(PATTERNS)] if n > 1 else "one"
        if n == 7 and not members and k % 2:
            pattern = "one"          # an attestation over an empty committee: an empty bitfield
        patterns.append(pattern)
        current = state.current_crosslinks[shard]
        good = Crosslink(shard, current.end_epoch, prev, hash_tree_root(current), tagged(b"data", shard, 1))

        def add(bits, crosslink, delay, target=True, head=True, proposer=None):
            data = types.SimpleNamespace(target_epoch=prev, target_root=target_root if target else wrong,
                                         crosslink=crosslink, beacon_block_root=None)
            slot = ns["get_attestation_data_slot"](state, data)
            head_root = ns["get_block_root_at_slot"](state, slot)
            data.beacon_block_root = head_root if head else wrong
            if proposer is None:   # every second one is slashed or not eligible
                proposer = special[len(atts) // 2 % len(special)] if special and len(atts) % 2 else rng.randrange(n)
            atts.append(types.SimpleNamespace(aggregation_bitfield=bitfield(bits), data=data, inclusion_delay=delay,
                                              proposer_index=proposer))

        m = len(members)
        some = [rng.random() < 0.6 for _ in range(m)]
        if pattern == "one":
            add([True] * m, good, c["MIN_ATTESTATION_INCLUSION_DELAY"] + k % 3)
        elif pattern == "overlap":
            add([i % 2 == 0 for i in range(m)], good, 5, head=False)
            add([i % 3 != 0 for i in range(m)], good, 3, proposer=(7 * k + 1) % n)
            add(some, good, 3, target=False, proposer=(7 * k + 2) % n)     # equal delays, different proposers
            add([i % 4 == 1 for i in range(m)], good, 3, proposer=(7 * k + 3) % n)
        elif pattern == "tie_roots":
            other = Crosslink(shard, current.end_epoch, prev, hash_tree_root(current), tagged(b"data", shard, 2))
            first, second = (good, other) if k % 2 else (other, good)
            add(some, first, 4)
            add(some, second, 6)
        elif pattern == "tie_same_root":
            # both pass the filter with one data_root: the current crosslink itself and a child of it
            child = Crosslink(shard, current.end_epoch, prev, hash_tree_root(current), current.data_root)
            same = Crosslink(*current.key())
            first, second = (child, same) if k % 2 else (same, child)
            add(some, first, 2)
            add(some, second, 2)
            add([not b for b in some], second if rng.random() < 0.5 else first, 9, head=False)
        elif pattern == "fail_filter":
            orphan = Crosslink(shard, current.end_epoch, prev, tagged(b"no parent", shard), tagged(b"data", shard, 3))
            add(some, orphan, 2)
            if shard == 0:
                add([not b for b in some], Crosslink(), 3)
        elif pattern == "mismatch":
            add(some, good, 2, target=False, head=False)
            add([i % 5 == 0 for i in range(m)], good, 7, target=True, head=False)
    return atts, patterns


def pack(values):
    return struct.pack("<%dQ" % len(values), *values)


def stored_list(values, n):
    return {"sha256": hashlib.sha256(pack(values)).hexdigest()} if n >= DIGEST_FROM else list(values)


def main():
    code = pull_blocks()
    out = {"source": "specs/core/0_beacon-chain.md python blocks defining %s (fence rule of "
                     "scripts/function_puller.py:40-44)" % ", ".join(WANTED),
           "supplied": {"hash": "sha256", "constants": {}, "GENESIS_EPOCH": "GENESIS_SLOT // SLOTS_PER_EPOCH",
                        "annotations": "BeaconState=Validator=AttestationData=PendingAttestation=object, "
                                       "Epoch=Slot=Shard=Gwei=ValidatorIndex=int, Bytes32=bytes, List/Tuple=typing's",
                        "Crosslink": "class of shard, start_epoch, end_epoch, parent_root, data_root; zero defaults; "
                                     "equal when all five are equal",
                        "hash_tree_root": "stand-in: sha256(b'crosslink' + u64le(shard, start_epoch, end_epoch) + "
                                          "parent_root + data_root); sha256(b'indices' + u64le(each)) for the index "
                                          "list; sha256(b'historical batch') for the HistoricalBatch stub",
                        "process_final_updates stubs": "HistoricalBatch(block_roots, state_roots); eth1_data_votes, "
                                                       "latest_active_index_roots, latest_slashed_balances, "
                                                       "latest_randao_mixes, latest_state_roots, historical_roots"},
           "digest": "sha256 of the list packed as little-endian u64 (lists of states of %d validators or more)" % DIGEST_FROM,
           "crosslink": "[shard, start_epoch, end_epoch, parent_root, data_root]",
           "epoch": EPOCH, "patterns": list(PATTERNS), "cases": []}
    rng = random.Random(0x4E3A)
    for preset, n, finalized in STATES:
        c = constants(preset)
        out["supplied"]["constants"][preset] = c
        ns = run_spec(code, c)
        state = types.SimpleNamespace()
        state.slot = (EPOCH + 1) * c["SLOTS_PER_EPOCH"] - 1
        state.finalized_epoch = finalized
        state.validator_registry = registry(rng, n, c)
        state.balances = start_balances(rng, state.validator_registry)
        state.latest_randao_mixes = [tagged(b"mix", n, k) for k in range(c["LATEST_RANDAO_MIXES_LENGTH"])]
        state.latest_active_index_roots = [tagged(b"index root", n, k) for k in range(c["LATEST_ACTIVE_INDEX_ROOTS_LENGTH"])]
        state.latest_block_roots = [tagged(b"block", n, k) for k in range(c["SLOTS_PER_HISTORICAL_ROOT"])]
        state.latest_state_roots = [tagged(b"state", n, k) for k in range(c["SLOTS_PER_HISTORICAL_ROOT"])]
        state.historical_roots = []
        state.eth1_data_votes = ["vote"]
        state.latest_slashed_balances = [0] * c["LATEST_SLASHED_EXIT_LENGTH"]
        total = ns["get_total_active_balance"](state)
        # total_penalties on either side of total_balance / 3
        penalties = total // 2 if n in (64,) else total // 40 + 12345
        state.latest_slashed_balances[(EPOCH + 1) % c["LATEST_SLASHED_EXIT_LENGTH"]] = 7 * ETH
        state.latest_slashed_balances[EPOCH % c["LATEST_SLASHED_EXIT_LENGTH"]] = 7 * ETH + penalties
        prev = ns["get_previous_epoch"](state)
        # shard 0 is the previous epoch's committee PATTERNS.index("fail_filter"): an attestation that equals
        # Crosslink() names shard 0
        state.latest_start_shard = 0
        count = ns["get_epoch_committee_count"](state, prev)
        while (c["SHARD_COUNT"] - ns["get_epoch_start_shard"](state, prev)) % c["SHARD_COUNT"] != PATTERNS.index("fail_filter"):
            state.latest_start_shard += 1
        start = ns["get_epoch_start_shard"](state, prev)
        shards = [(start + j) % c["SHARD_COUNT"] for j in range(count)]
        assert shards[PATTERNS.index("fail_filter")] == 0
        committees = [ns["get_crosslink_committee"](state, prev, s) for s in shards]
        state.current_crosslinks = [Crosslink(s, 2, 5, tagged(b"parent", n, s), tagged(b"data", s, 0))
                                    for s in range(c["SHARD_COUNT"])]
        state.previous_crosslinks = list(state.current_crosslinks)
        state.current_epoch_attestations = []
        state.previous_epoch_attestations, patterns = attestations(rng, ns, c, state, prev, shards, committees)
        atts = state.previous_epoch_attestations
        target_ids = {id(a) for a in ns["get_matching_target_attestations"](state, prev)}
        head_ids = {id(a) for a in ns["get_matching_head_attestations"](state, prev)}
        case = {"preset": preset, "n": n, "slot": state.slot, "current_epoch": EPOCH, "previous_epoch": prev,
                "finalized_epoch": finalized, "latest_start_shard": state.latest_start_shard,
                "kinds": [v.kind for v in state.validator_registry] if n < DIGEST_FROM else None,
                "activation_epochs": [v.activation_epoch for v in state.validator_registry],
                "exit_epochs": [v.exit_epoch for v in state.validator_registry],
                "withdrawable_epochs": [v.withdrawable_epoch for v in state.validator_registry],
                "slashed": [int(v.slashed) for v in state.validator_registry],
                "effective_balances": [v.effective_balance for v in state.validator_registry],
                "balances": list(state.balances),
                "total_active_balance": total, "total_penalties": penalties,
                "shards": shards, "committees": committees, "patterns": patterns,
                "attestations": [{
                    "shard": a.data.crosslink.shard, "bits": a.aggregation_bitfield.hex(),
                    "inclusion_delay": a.inclusion_delay, "proposer_index": a.proposer_index,
                    "target": id(a) in target_ids, "head": id(a) in head_ids, "crosslink": a.data.crosslink.stored(),
                    "passes_filter": hash_tree_root(state.current_crosslinks[a.data.crosslink.shard]) in
                                     (a.data.crosslink.parent_root, hash_tree_root(a.data.crosslink)),
                } for a in atts]}
        if case["kinds"] is None:
            del case["kinds"]
        # a pattern whose committee is on shard 0 and fails the filter carries the Crosslink() attestation; the
        # attestations name shards, so the committee of each is shards.index(shard)
        case["attesting_balances"] = [
            ns["get_attesting_balance"](state, ns["get_matching_source_attestations"](state, prev)),
            ns["get_attesting_balance"](state, ns["get_matching_target_attestations"](state, prev)),
            ns["get_attesting_balance"](state, ns["get_matching_head_attestations"](state, prev))]
        winners = []
        for s, members in zip(shards, committees):
            w, indices = ns["get_winning_crosslink_and_attesting_indices"](state, prev, s)
            winners.append({"shard": s, "crosslink": w.stored(), "attesters": len(indices),
                            "attesting_balance": ns["get_total_balance"](state, indices),
                            "committee_balance": ns["get_total_balance"](state, members)})
        case["winners"] = winners
        r1, p1 = ns["get_attestation_deltas"](state)
        r2, p2 = ns["get_crosslink_deltas"](state)
        case["attestation_deltas"] = {"rewards": stored_list(r1, n), "penalties": stored_list(p1, n)}
        case["crosslink_deltas"] = {"rewards": stored_list(r2, n), "penalties": stored_list(p2, n)}
        # process_final_updates alone over balances on both sides of each threshold
        edge = copy.deepcopy(state)
        edge.balances = hysteresis_balances(edge.validator_registry, c)
        edge_balances = list(edge.balances)
        ns["process_final_updates"](edge)
        case["hysteresis"] = {"balances": edge_balances,
                              "effective_balances_after": [v.effective_balance for v in edge.validator_registry]}
        ns["process_rewards_and_penalties"](state)
        case["balances_after_rewards"] = stored_list(state.balances, n)
        ns["process_slashings"](state)
        case["balances_after_slashings"] = stored_list(state.balances, n)
        ns["process_final_updates"](state)
        case["balances_after_final"] = stored_list(state.balances, n)
        case["effective_balances_after"] = stored_list([v.effective_balance for v in state.validator_registry], n)
        out["cases"].append(case)
        print(preset, n, "validators:", count, "committees,", len(atts), "attestations", flush=True)
    with open(os.path.join(HERE, "epoch_rewards.json"), "w") as f:
        f.write("{\n")
        for key in [k for k in out if k != "cases"]:
            f.write(' "%s": %s,\n' % (key, json.dumps(out[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(cs, separators=(",", ":")) for cs in out["cases"]) + "\n ]\n}\n")
    print("epoch_rewards.json:", len(out["cases"]), "cases,", os.path.getsize(os.path.join(HERE, "epoch_rewards.json")), "bytes")


if __name__ == "__main__":
    main()
