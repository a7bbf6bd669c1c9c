"""Pin the registry updates to the reference's own spec text: tests/golden/registry_updates.json.

As make_epoch_rewards_vectors.py does for the rewards, this script takes the functions mechanically
from the spec's text: the ```python blocks of specs/core/0_beacon-chain.md that define the names in
WANTED, pulled by the fence rule of the reference's extractor (scripts/function_puller.py:40-44) and
run unmodified over states built from namespaces.  What the text leaves to its surroundings is
supplied here and named in the output:
  * the constants of configs/constant_presets/{minimal,mainnet}.yaml named in CONSTANTS
  * the annotation names (BeaconState, Validator = object; Epoch, Slot, ValidatorIndex = int;
    List = typing's)
  * OVERRIDES: per state, constants replaced by name (CHURN_LIMIT_QUOTIENT = 8 makes the text itself
    run with a churn limit above MIN_PER_EPOCH_CHURN_LIMIT on a few hundred validators)

States: 1, 7, 64 and 301 validators under both presets at the last slot of epoch 20 with
finalized_epoch 12 (delayed(finalized) = 17 <= 20: validators activated since still stand in the
activation queue), and the same sizes under the minimal preset with CHURN_LIMIT_QUOTIENT = 8.  The
registries mix: active validators at and above EJECTION_BALANCE; validators at it that already have
an exit epoch; validators not yet active at it; exited validators whose exit epochs lie below, at
and above delayed(current) with several on the largest; deposits with and without
MAX_EFFECTIVE_BALANCE and no eligibility epoch; eligible validators with equal and different
eligibility epochs, some already activated at or after delayed(finalized) and one a single epoch
before it.

Stored per state: the inputs (five lists), and as outputs the four epoch lists after
process_registry_updates; from 301 validators on every list is a SHA-256 digest of its entries
packed as little-endian uint64 (the inputs are rebuilt from `seed` by registry() below, which
tests/registry_updates_cases.py repeats).  Also stored: "exits", the (exit_epoch,
withdrawable_epoch) pairs that initiate_validator_exit gives when called on EXITS active validators
of the state before the call, in ascending index order.  None of the spec's text is stored.

Run (where the reference checkout exists: beside the repository, or at $BLS381_REFERENCE):
    python tests/golden/make_registry_updates_vectors.py
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
WANTED = ("slot_to_epoch", "get_current_epoch", "is_active_validator", "get_active_validator_indices",
          "get_delayed_activation_exit_epoch", "get_churn_limit", "initiate_validator_exit", "process_registry_updates")
CONSTANTS = ("SLOTS_PER_EPOCH", "FAR_FUTURE_EPOCH", "ACTIVATION_EXIT_DELAY", "MIN_VALIDATOR_WITHDRAWABILITY_DELAY",
             "MIN_PER_EPOCH_CHURN_LIMIT", "CHURN_LIMIT_QUOTIENT", "MAX_EFFECTIVE_BALANCE", "EJECTION_BALANCE")
EPOCH, FINALIZED = 20, 12
SIZES = (1, 7, 64, 301)
STATES = [(preset, n, {}) for preset in ("minimal", "mainnet") for n in SIZES] + \
         [("minimal", n, {"CHURN_LIMIT_QUOTIENT": 8}) for n in SIZES]
ETH = 10 ** 9
DIGEST_FROM = 301
EXITS = 14
FIELDS = ("activation_eligibility_epoch", "activation_epoch", "exit_epoch", "withdrawable_epoch", "effective_balance")
KINDS = ("active", "active", "active", "low", "low", "low_exiting", "low_pending", "exited_old", "exited_at", "exited_at",
         "exited_peak", "exited_peak", "deposit_full", "deposit_short", "eligible_a", "eligible_a", "eligible_b",
         "eligible_new", "activated_in_queue", "activated_before")


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


def constants(preset, overrides):
    text = open(os.path.join(REF, "configs", "constant_presets", preset + ".yaml")).read()
    c = {name: int(re.search(r"^%s:\s*(\d+)" % name, text, re.M).group(1)) for name in CONSTANTS}
    c.update(overrides)
    return c


def run_spec(code, consts):
    ns = {"List": typing.List}
    ns.update({name: object for name in ("BeaconState", "Validator")})
    ns.update({name: int for name in ("Epoch", "Slot", "ValidatorIndex")})
    ns.update(consts)
    exec(compile(code, SPEC, "exec"), ns)   # noqa: S102 -- the reference's own spec text
    return ns


def registry(seed, n, c):
    """n validators around EPOCH; validator i's kind is drawn from KINDS (every kind is there from
    64 validators on).  Repeated by tests/registry_updates_cases.py."""
    rng = random.Random(seed)
    far, delayed = c["FAR_FUTURE_EPOCH"], EPOCH + 1 + c["ACTIVATION_EXIT_DELAY"]
    delayed_fin = FINALIZED + 1 + c["ACTIVATION_EXIT_DELAY"]
    peak = delayed + rng.choice([-2, 0, 3])   # the largest exit epoch: below, at or above delayed(current)
    out = []
    for i in range(n):
        kind = KINDS[i % len(KINDS)] if n >= 64 and i % 3 else rng.choice(KINDS)
        v = types.SimpleNamespace(activation_eligibility_epoch=0, activation_epoch=0, exit_epoch=far, withdrawable_epoch=far,
                                  effective_balance=rng.choice([32, 32, 31, 24, 17]) * ETH)
        if kind == "low":
            v.effective_balance = rng.choice([16, 16, 15, 0]) * ETH
        elif kind == "low_exiting":
            v.effective_balance, v.exit_epoch, v.withdrawable_epoch = 16 * ETH, peak - 1, peak + 255
        elif kind == "low_pending":
            v.effective_balance, v.activation_epoch = 16 * ETH, EPOCH + 1
        elif kind == "exited_old":
            v.exit_epoch, v.withdrawable_epoch = EPOCH - 5, EPOCH + 251
        elif kind == "exited_at":
            v.exit_epoch, v.withdrawable_epoch = peak - 1, peak + 255
        elif kind == "exited_peak":
            v.exit_epoch, v.withdrawable_epoch = peak, peak + 256
        elif kind == "deposit_full":
            v.activation_eligibility_epoch, v.activation_epoch, v.effective_balance = far, far, 32 * ETH
        elif kind == "deposit_short":
            v.activation_eligibility_epoch, v.activation_epoch = far, far
            v.effective_balance = rng.choice([31, 17, 0]) * ETH
        elif kind in ("eligible_a", "eligible_b", "eligible_new"):
            v.activation_eligibility_epoch = {"eligible_a": EPOCH - 3, "eligible_b": EPOCH - 6, "eligible_new": EPOCH}[kind]
            v.activation_epoch = far
        elif kind == "activated_in_queue":      # takes a place in the queue and keeps its epoch
            v.activation_eligibility_epoch = rng.choice([EPOCH - 9, EPOCH - 3])
            v.activation_epoch = rng.choice([delayed_fin, delayed_fin + 1, EPOCH + 2])
        elif kind == "activated_before":
            v.activation_eligibility_epoch, v.activation_epoch = EPOCH - 10, delayed_fin - 1
        out.append(v)
    return out


def lists(validators):
    return {f: [getattr(v, f) for v in validators] for f in FIELDS}


def stored(values, n):
    if n < DIGEST_FROM:
        return list(values)
    return hashlib.sha256(struct.pack("<%dQ" % len(values), *values)).hexdigest()


def main():
    code = pull_blocks()
    out = {"source": "specs/core/0_beacon-chain.md: " + ", ".join(WANTED), "epoch": EPOCH, "finalized_epoch": FINALIZED,
           "digest_from": DIGEST_FROM, "states": []}
    for k, (preset, n, overrides) in enumerate(STATES):
        c = constants(preset, overrides)
        spec = run_spec(code, c)
        seed = 7000 + k
        validators = registry(seed, n, c)
        state = types.SimpleNamespace(slot=EPOCH * c["SLOTS_PER_EPOCH"] + c["SLOTS_PER_EPOCH"] - 1, finalized_epoch=FINALIZED,
                                      validator_registry=copy.deepcopy(validators))
        assert spec["get_current_epoch"](state) == EPOCH
        churn_limit = spec["get_churn_limit"](state)
        spec["process_registry_updates"](state)
        after = lists(state.validator_registry)
        # initiate_validator_exit alone, on the state before the call
        state2 = types.SimpleNamespace(slot=state.slot, finalized_epoch=FINALIZED, validator_registry=copy.deepcopy(validators))
        exits = []
        for i, v in enumerate(state2.validator_registry):
            if len(exits) < EXITS and spec["is_active_validator"](v, EPOCH) and v.exit_epoch == c["FAR_FUTURE_EPOCH"]:
                spec["initiate_validator_exit"](state2, i)
                exits.append([i, v.exit_epoch, v.withdrawable_epoch])
        before = lists(validators)
        out["states"].append({
            "preset": preset, "overrides": overrides, "n": n, "seed": seed,
            "constants": {name: c[name] for name in CONSTANTS}, "churn_limit": churn_limit,
            "inputs": {f: stored(before[f], n) for f in FIELDS},
            "outputs": {f: stored(after[f], n) for f in FIELDS[:4]},
            "exits": exits})
    path = os.path.join(HERE, "registry_updates.json")
    with open(path, "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
