"""Model of the epoch context (test infrastructure): the spec's functions restated over plain arrays.

Reference: specs/core/0_beacon-chain.md of the reference -- is_active_validator (:660-665),
get_active_validator_indices (:680-684), get_epoch_committee_count / get_shard_delta /
get_epoch_start_shard (:710-744), generate_seed (:807-816), get_beacon_proposer_index (:822-840),
get_crosslink_committee (:896-903), get_total_balance (:936-940), and hash_tree_root of a
List[uint64] (ssz_impl.py: pack, merkleize, mix_in_length).  A state is a ``State`` of lists;
the constants are a dict with the preset's names.  tests/golden/epoch_context.json
(make_epoch_context_vectors.py) pins these to the reference's own text.
"""
import hashlib
import json
import os

import shuffle_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
FAR_FUTURE_EPOCH = 2 ** 64 - 1
VALIDATOR_BYTES = 121                    # serialized Validator (:284-298)
OFF_ACTIVATION, OFF_EXIT, OFF_BALANCE = 88, 96, 113


def hash(data: bytes) -> bytes:   # noqa: A001 -- the spec's name
    return hashlib.sha256(data).digest()


def int_to_bytes(integer: int, length: int) -> bytes:
    return integer.to_bytes(length, "little")


class State:
    """The fields of BeaconState that the epoch context reads."""

    def __init__(self, activation_epochs, exit_epochs, effective_balances, slot, latest_start_shard, randao_mix,
                 consts):
        self.activation_epochs = list(activation_epochs)
        self.exit_epochs = list(exit_epochs)
        self.effective_balances = list(effective_balances)
        self.slot = slot
        self.latest_start_shard = latest_start_shard
        self.randao_mix = randao_mix   # get_randao_mix(state, epoch + LATEST_RANDAO_MIXES_LENGTH - MIN_SEED_LOOKAHEAD)
        self.c = consts

    def current_epoch(self):
        return self.slot // self.c["SLOTS_PER_EPOCH"]


def is_active(activation_epoch: int, exit_epoch: int, epoch: int) -> bool:
    return activation_epoch <= epoch < exit_epoch


def get_active_validator_indices(activation_epochs, exit_epochs, epoch: int):
    return [i for i, (a, e) in enumerate(zip(activation_epochs, exit_epochs)) if is_active(a, e, epoch)]


def get_total_balance(effective_balances, indices) -> int:
    return max(sum(effective_balances[i] for i in indices), 1)


def epoch_committee_count(active_count: int, c) -> int:
    return max(1, min(c["SHARD_COUNT"] // c["SLOTS_PER_EPOCH"],
                      active_count // c["SLOTS_PER_EPOCH"] // c["TARGET_COMMITTEE_SIZE"])) * c["SLOTS_PER_EPOCH"]


def shard_delta(active_count: int, c) -> int:
    return min(epoch_committee_count(active_count, c), c["SHARD_COUNT"] - c["SHARD_COUNT"] // c["SLOTS_PER_EPOCH"])


def active_count(state: State, epoch: int) -> int:
    return len(get_active_validator_indices(state.activation_epochs, state.exit_epochs, epoch))


def epoch_start_shard(state: State, epoch: int) -> int:
    c, current = state.c, state.current_epoch()
    assert epoch <= current + 1
    check_epoch = current + 1
    shard = (state.latest_start_shard + shard_delta(active_count(state, current), c)) % c["SHARD_COUNT"]
    while check_epoch > epoch:
        check_epoch -= 1
        shard = (shard + c["SHARD_COUNT"] - shard_delta(active_count(state, check_epoch), c)) % c["SHARD_COUNT"]
    return shard


def index_chunks(indices):
    """pack() of a List[uint64]: 8 little-endian bytes per index, zero-padded to whole 32-byte chunks."""
    data = b"".join(int_to_bytes(i, 8) for i in indices)
    data += bytes(-len(data) % 32)
    return [data[k:k + 32] for k in range(0, len(data), 32)]


def merkleize(chunks):
    layer = list(chunks) or [bytes(32)]
    zero = bytes(32)
    while len(layer) > 1:
        if len(layer) % 2:
            layer.append(zero)
        layer = [hash(layer[k] + layer[k + 1]) for k in range(0, len(layer), 2)]
        zero = hash(zero + zero)
    return layer[0]


def active_index_root(indices) -> bytes:
    """hash_tree_root(List[uint64](indices)): mix_in_length(merkleize(pack(indices)), len)."""
    return hash(merkleize(index_chunks(indices)) + int_to_bytes(len(indices), 32))


def generate_seed(randao_mix: bytes, index_root: bytes, epoch: int) -> bytes:
    return hash(randao_mix + index_root + int_to_bytes(epoch, 32))


def state_seed(state: State, epoch: int) -> bytes:
    """generate_seed with the index root the state would hold for ``epoch``."""
    root = active_index_root(get_active_validator_indices(state.activation_epochs, state.exit_epochs, epoch))
    return generate_seed(state.randao_mix, root, epoch)


def get_crosslink_committee(state: State, epoch: int, shard: int):
    c = state.c
    indices = get_active_validator_indices(state.activation_epochs, state.exit_epochs, epoch)
    return SM.compute_committee(indices, state_seed(state, epoch),
                                (shard + c["SHARD_COUNT"] - epoch_start_shard(state, epoch)) % c["SHARD_COUNT"],
                                epoch_committee_count(len(indices), c), c["SHUFFLE_ROUND_COUNT"])


def proposer_search(first_committee, epoch: int, effective_balances, seed: bytes, max_effective_balance: int,
                    max_tries=None):
    """The loop of get_beacon_proposer_index: (candidate_index, the try that accepted), or
    (None, max_tries) when no try below max_tries accepts (the engine's cap; the spec has none)."""
    i = 0
    while max_tries is None or i < max_tries:
        candidate_index = first_committee[(epoch + i) % len(first_committee)]
        random_byte = hash(seed + int_to_bytes(i // 32, 8))[i % 32]
        if effective_balances[candidate_index] * 255 >= max_effective_balance * random_byte:
            return candidate_index, i
        i += 1
    return None, max_tries


def get_beacon_proposer_index(state: State) -> int:
    c, epoch = state.c, state.current_epoch()
    committees_per_slot = epoch_committee_count(active_count(state, epoch), c) // c["SLOTS_PER_EPOCH"]
    offset = committees_per_slot * (state.slot % c["SLOTS_PER_EPOCH"])
    shard = (epoch_start_shard(state, epoch) + offset) % c["SHARD_COUNT"]
    first_committee = get_crosslink_committee(state, epoch, shard)
    return proposer_search(first_committee, epoch, state.effective_balances, state_seed(state, epoch),
                           c["MAX_EFFECTIVE_BALANCE"])[0]


def validator_records(activation_epochs, exit_epochs, effective_balances, rng=None) -> bytes:
    """Serialized Validator records (121 bytes each) carrying these three fields; every other
    byte is random (rng: random.Random) or zero."""
    out = bytearray()
    for a, e, b in zip(activation_epochs, exit_epochs, effective_balances):
        rec = bytearray(rng.getrandbits(8) for _ in range(VALIDATOR_BYTES)) if rng else bytearray(VALIDATOR_BYTES)
        rec[OFF_ACTIVATION:OFF_ACTIVATION + 8] = int_to_bytes(a, 8)
        rec[OFF_EXIT:OFF_EXIT + 8] = int_to_bytes(e, 8)
        rec[OFF_BALANCE:OFF_BALANCE + 8] = int_to_bytes(b, 8)
        out += rec
    return bytes(out)


def fixture():
    with open(os.path.join(HERE, "golden", "epoch_context.json")) as f:
        return json.load(f)


def fixture_state(case, consts) -> State:
    return State(case["activation_epochs"], case["exit_epochs"], case["effective_balances"], case["slot"],
                 case["latest_start_shard"], bytes.fromhex(case["randao_mix"]), consts)
