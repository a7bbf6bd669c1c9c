"""Pin the epoch context to the reference's own spec text: tests/golden/epoch_context.json.

As make_shuffling_vectors.py does for the shuffle, this script takes the functions mechanically
from the spec's text: the ```python blocks of specs/core/0_beacon-chain.md that define the names
in WANTED, pulled by the fence rule of the reference's extractor (scripts/function_puller.py:40-44)
and run unmodified over small states built from namespaces.  What the text leaves to its
surroundings is supplied here and named in the output:
  * hash = SHA-256 (0_beacon-chain.md:591-595)
  * the constants of configs/constant_presets/{minimal,mainnet}.yaml named in CONSTANTS
  * the annotation names (BeaconState, Validator = object; Epoch, Slot, Shard, Gwei,
    ValidatorIndex = int; Bytes32 = bytes; List = typing.List)
  * state.latest_active_index_roots[epoch % LATEST_ACTIVE_INDEX_ROOTS_LENGTH] =
    hash_tree_root(List[uint64](get_active_validator_indices(state, epoch))), what
    process_final_updates (:1545) stores: mix_in_length over the reference's own
    utils/merkle_minimal.merkleize_chunks of the packed chunks, as make_ssz_vectors.py pins roots

States: 0, 1, 7, 64 and 301 validators with mixed activation and exit epochs (the epoch itself,
its neighbours, FAR_FUTURE_EPOCH) and effective balances of 0 to 32 ETH, at epoch 5 of each
preset.  Per state: the active indices of epochs 4, 5 and 6 with their committee counts, shard
deltas, start shards, index roots and total balances; the seed of epoch 5; every crosslink
committee of epoch 5 (lengths and a digest; the lists themselves for the small states) and the
proposer of every slot of epoch 5 (null where the slot's first committee is empty: the spec
divides by its length).  Only inputs and outputs are stored, none of the spec's text.

Run (where the reference checkout exists):
    python tests/golden/make_epoch_context_vectors.py
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
REF = os.environ.get("BLS381_REFERENCE", "/root/reference")
SPEC = os.path.join(REF, "specs", "core", "0_beacon-chain.md")
WANTED = ("int_to_bytes", "bytes_to_int", "slot_to_epoch", "get_current_epoch", "get_epoch_start_slot",
          "is_active_validator", "get_active_validator_indices", "get_epoch_committee_count", "get_shard_delta",
          "get_epoch_start_shard", "get_randao_mix", "get_active_index_root", "generate_seed",
          "get_beacon_proposer_index", "get_shuffled_index", "compute_committee", "get_crosslink_committee",
          "get_total_balance")
CONSTANTS = ("SHARD_COUNT", "TARGET_COMMITTEE_SIZE", "SHUFFLE_ROUND_COUNT", "MAX_EFFECTIVE_BALANCE",
             "FAR_FUTURE_EPOCH", "SLOTS_PER_EPOCH", "MIN_SEED_LOOKAHEAD", "ACTIVATION_EXIT_DELAY",
             "LATEST_RANDAO_MIXES_LENGTH", "LATEST_ACTIVE_INDEX_ROOTS_LENGTH")
EPOCH = 5
SIZES = [0, 1, 7, 64, 301]
ETH = 10 ** 9


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


def run_spec(code, consts):
    ns = {"hash": lambda b: hashlib.sha256(b).digest(), "List": typing.List, "Bytes32": bytes}
    ns.update({name: object for name in ("BeaconState", "Validator")})
    ns.update({name: int for name in ("Epoch", "Slot", "Shard", "Gwei", "ValidatorIndex")})
    ns.update(consts)
    exec(compile(code, SPEC, "exec"), ns)   # noqa: S102 -- the reference's own spec text
    return ns


def ref_merkleize():
    sys.path.insert(0, os.path.join(REF, "test_libs", "pyspec"))
    from eth2spec.utils import merkle_minimal   # pure: hashlib via eth2spec.utils.hash_function
    return merkle_minimal.merkleize_chunks


def index_root(merkleize_chunks, indices):
    data = b"".join(struct.pack("<Q", i) for i in indices)
    data += bytes(-len(data) % 32)
    chunks = [data[k:k + 32] for k in range(0, len(data), 32)]
    return hashlib.sha256(bytes(merkleize_chunks(chunks)) + len(indices).to_bytes(32, "little")).digest()


def validators(rng, n, far):
    """Mixed epochs around EPOCH; about two in three are active at EPOCH."""
    act, ext, bal = [], [], []
    for i in range(n):
        a = rng.choice([0, 0, 0, 1, EPOCH - 1, EPOCH, EPOCH, EPOCH + 1, EPOCH + 3, far])
        e = rng.choice([far, far, far, far, far, EPOCH + 1, EPOCH + 9, EPOCH, EPOCH - 1, 2 ** 63 + i])
        if n == 1:
            a, e = 0, far
        act.append(a)
        ext.append(e)
        bal.append(rng.choice([0, 1, 16, 17, 31, 32, 32, 32]) * ETH)
    return act, ext, bal


def digest(values):
    return hashlib.sha256(struct.pack("<%dI" % len(values), *values)).hexdigest()


def main():
    code = pull_blocks()
    merkleize_chunks = ref_merkleize()
    out = {"source": "specs/core/0_beacon-chain.md python blocks defining %s (fence rule of "
                     "scripts/function_puller.py:40-44)" % ", ".join(WANTED),
           "supplied": {"hash": "sha256", "constants": {},
                        "annotations": "BeaconState=Validator=object, Epoch=Slot=Shard=Gwei=ValidatorIndex=int, "
                                       "Bytes32=bytes, List=typing.List",
                        "index_roots": "mix_in_length(utils/merkle_minimal.merkleize_chunks(packed chunks), len)"},
           "digest": "sha256 of the list packed as little-endian u32", "epoch": EPOCH, "cases": []}
    rng = random.Random(0xE90C)
    for preset in ("minimal", "mainnet"):
        c = constants(preset)
        out["supplied"]["constants"][preset] = c
        ns = run_spec(code, c)
        for n in SIZES:
            act, ext, bal = validators(rng, n, c["FAR_FUTURE_EPOCH"])
            state = types.SimpleNamespace()
            state.validator_registry = [types.SimpleNamespace(activation_epoch=a, exit_epoch=e, effective_balance=b)
                                        for a, e, b in zip(act, ext, bal)]
            state.slot = ns["get_epoch_start_slot"](EPOCH)
            state.latest_start_shard = rng.randrange(c["SHARD_COUNT"])
            state.latest_randao_mixes = [hashlib.sha256(b"mix" + struct.pack("<HI", n, k)).digest()
                                         for k in range(c["LATEST_RANDAO_MIXES_LENGTH"])]
            state.latest_active_index_roots = [bytes(32)] * c["LATEST_ACTIVE_INDEX_ROOTS_LENGTH"]
            case = {"preset": preset, "n": n, "slot": state.slot, "latest_start_shard": state.latest_start_shard,
                    "activation_epochs": act, "exit_epochs": ext, "effective_balances": bal, "epochs": []}
            for e in (EPOCH - 1, EPOCH, EPOCH + 1):
                active = ns["get_active_validator_indices"](state, e)
                root = index_root(merkleize_chunks, active)
                state.latest_active_index_roots[e % c["LATEST_ACTIVE_INDEX_ROOTS_LENGTH"]] = root
                case["epochs"].append({"epoch": e, "active": active, "index_root": root.hex(),
                                       "total_balance": ns["get_total_balance"](state, active),
                                       "committee_count": ns["get_epoch_committee_count"](state, e),
                                       "shard_delta": ns["get_shard_delta"](state, e),
                                       "start_shard": ns["get_epoch_start_shard"](state, e)})
            case["randao_mix"] = ns["get_randao_mix"](
                state, EPOCH + c["LATEST_RANDAO_MIXES_LENGTH"] - c["MIN_SEED_LOOKAHEAD"]).hex()
            case["seed"] = ns["generate_seed"](state, EPOCH).hex()
            count = case["epochs"][1]["committee_count"]
            start = case["epochs"][1]["start_shard"]
            shards = [(start + j) % c["SHARD_COUNT"] for j in range(count)]
            committees = [ns["get_crosslink_committee"](state, EPOCH, s) for s in shards]
            case["shards"] = shards
            case["committee_lengths"] = [len(m) for m in committees]
            case["committees_sha256"] = digest([v for m in committees for v in m])
            if n <= 64:
                case["committees"] = committees
            proposers = []
            per_slot = count // c["SLOTS_PER_EPOCH"]
            for s in range(c["SLOTS_PER_EPOCH"]):
                state.slot = ns["get_epoch_start_slot"](EPOCH) + s
                proposers.append(ns["get_beacon_proposer_index"](state) if committees[per_slot * s] else None)
            case["proposers"] = proposers
            out["cases"].append(case)
            print(preset, n, "validators:", len(case["epochs"][1]["active"]), "active,", count, "committees", flush=True)
    with open(os.path.join(HERE, "epoch_context.json"), "w") as f:
        f.write("{\n")
        for key in [k for k in out if k != "cases"]:
            f.write(' "%s": %s,\n' % (key, json.dumps(out[key])))
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(cs, separators=(",", ":")) for cs in out["cases"]) + "\n ]\n}\n")
    print("epoch_context.json:", len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
