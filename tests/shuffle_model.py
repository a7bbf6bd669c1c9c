"""Model of committee selection (test infrastructure): the spec's shuffle and index sets restated.

* get_shuffled_index / compute_committee: specs/core/0_beacon-chain.md:860-890 of the reference,
  the loop restated literally (``rounds`` is the spec's SHUFFLE_ROUND_COUNT constant made an
  argument).  tests/golden/shuffling.json (make_shuffling_vectors.py) pins it to the reference's
  own text.
* shuffled_list: the same permutation for every position at once, one vectorised pass per round
  over the per-round table of source digests (the layout of the engine's table path).
* verify_bitfield / get_attesting_indices / convert_to_indexed_sets: :905-917, :960-1001.
"""
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def hash(data: bytes) -> bytes:   # noqa: A001 -- the spec's name
    return hashlib.sha256(data).digest()


def int_to_bytes(integer: int, length: int) -> bytes:
    return integer.to_bytes(length, "little")


def bytes_to_int(data: bytes) -> int:
    return int.from_bytes(data, "little")


def get_shuffled_index(index: int, index_count: int, seed: bytes, rounds: int = 90) -> int:
    assert index < index_count
    assert index_count <= 2 ** 40
    for round in range(rounds):   # noqa: A001
        pivot = bytes_to_int(hash(seed + int_to_bytes(round, length=1))[0:8]) % index_count
        flip = (pivot + index_count - index) % index_count
        position = max(index, flip)
        source = hash(seed + int_to_bytes(round, length=1) + int_to_bytes(position // 256, length=4))
        byte = source[(position % 256) // 8]
        bit = (byte >> (position % 8)) % 2
        index = flip if bit else index
    return index


def compute_committee(indices, seed: bytes, index: int, count: int, rounds: int = 90):
    start = (len(indices) * index) // count
    end = (len(indices) * (index + 1)) // count
    return [indices[get_shuffled_index(i, len(indices), seed, rounds)] for i in range(start, end)]


def shuffled_list(index_count: int, seed: bytes, rounds: int = 90) -> np.ndarray:
    """[get_shuffled_index(i, index_count, seed) for i in range(index_count)], one pass per round."""
    n = index_count
    idx = np.arange(n, dtype=np.int64)
    blocks = (n + 255) // 256
    for r in range(rounds):
        rb = int_to_bytes(r, 1)
        pivot = bytes_to_int(hash(seed + rb)[0:8]) % n if n else 0
        row = np.frombuffer(b"".join(hash(seed + rb + int_to_bytes(b, 4)) for b in range(blocks)), dtype=np.uint8)
        flip = (pivot + n - idx) % n
        position = np.maximum(idx, flip)
        bit = (row[position // 8] >> (position % 8).astype(np.uint8)) & 1
        idx = np.where(bit == 1, flip, idx)
    return idx.astype(np.uint32)


def get_bitfield_bit(bitfield: bytes, i: int) -> int:
    return (bitfield[i // 8] >> (i % 8)) % 2


def verify_bitfield(bitfield: bytes, committee_size: int) -> bool:
    if len(bitfield) != (committee_size + 7) // 8:
        return False
    for i in range(committee_size, len(bitfield) * 8):
        if get_bitfield_bit(bitfield, i) == 0b1:
            return False
    return True


def get_attesting_indices(committee, bitfield: bytes):
    assert verify_bitfield(bitfield, len(committee))
    return sorted([index for i, index in enumerate(committee) if get_bitfield_bit(bitfield, i) == 0b1])


def convert_to_indexed_sets(committee, aggregation_bitfield: bytes, custody_bitfield: bytes):
    """(custody_bit_0_indices, custody_bit_1_indices) of convert_to_indexed."""
    attesting_indices = get_attesting_indices(committee, aggregation_bitfield)
    custody_bit_1_indices = get_attesting_indices(committee, custody_bitfield)
    custody_bit_0_indices = [index for index in attesting_indices if index not in custody_bit_1_indices]
    return custody_bit_0_indices, custody_bit_1_indices


def attesting_entries(committees, aggregation_bitfields, custody_bitfields):
    """What the engine's batch call returns for these attestations: (group_key_off, ok, entries);
    an attestation with a bad bitfield has ok 0 and two empty groups."""
    off, ok, entries = [0], [], []
    for committee, agg, cust in zip(committees, aggregation_bitfields, custody_bitfields):
        good = verify_bitfield(agg, len(committee)) and verify_bitfield(cust, len(committee))
        g0, g1 = convert_to_indexed_sets(committee, agg, cust) if good else ([], [])
        ok.append(int(good))
        for g in (g0, g1):
            entries.extend(g)
            off.append(len(entries))
    return off, ok, entries


def random_bitfield(rng, committee_size: int, density: float = 0.5) -> bytes:
    """A valid bitfield for a committee of this size (rng: random.Random)."""
    bits = bytearray((committee_size + 7) // 8)
    for i in range(committee_size):
        if rng.random() < density:
            bits[i // 8] |= 1 << (i % 8)
    return bytes(bits)


def list_digest(values) -> str:
    """SHA-256 of a list packed as little-endian u32 (the fixture's digest column)."""
    return hashlib.sha256(np.asarray(values, dtype="<u4").tobytes()).hexdigest()


def generator_seeds():
    """The reference generator's seeds (test_generators/shuffling/main.py:18)."""
    return [hash(int_to_bytes(k, 4)) for k in range(30)]


GENERATOR_COUNTS = [0, 1, 2, 3, 5, 10, 33, 100, 1000]   # main.py:19


def fixture():
    with open(os.path.join(HERE, "golden", "shuffling.json")) as f:
        return json.load(f)
