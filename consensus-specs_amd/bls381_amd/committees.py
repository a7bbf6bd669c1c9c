"""Committee selection on the device: the producer of the grouped verify's member entries.

Mirrors of the reference's functions (specs/core/0_beacon-chain.md), run by the engine
(include/bls381.h ``bls381_shuffle`` / ``bls381_attesting_entries``; csrc/bls381_shuffle.hpp):

* ``shuffled_indices``   -- ``get_shuffled_index`` (:860-882) for a window of positions
* ``compute_committee``  -- :887-890, with ``committee_bounds`` giving every committee's slice
* ``get_attesting_indices`` -- :905-917 over a committee already computed
* ``attesting_entries``  -- ``convert_to_indexed``'s two index sets (:988-1001) for a batch of
  attestations, in the layout ``bls381_registry_verify_multiple_grouped_device`` takes

``rounds`` is the spec's SHUFFLE_ROUND_COUNT (90 mainnet, 10 minimal).  Lists hold at most
2^32 - 1 indices (the spec allows 2^40; registry entries are 32-bit).  Callers that keep the
shuffled list in HBM use the ``_device`` entry points directly.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

MAX_INDICES_PER_ATTESTATION = 4096


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _seed(seed) -> bytes:
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed must be 32 bytes")
    return seed


def _shuffle(index_count: int, seed, rounds: int, first: int, count: int, indices) -> np.ndarray:
    if not (0 <= index_count < 1 << 32 and 0 <= rounds <= 255 and 0 <= first and 0 <= count
            and first + count <= index_count):
        raise ValueError("shuffle: index_count < 2^32, rounds <= 255 and first + count <= index_count")
    out = np.zeros(count, dtype=np.uint32)
    if count:
        _native.check(_native.lib().bls381_shuffle(index_count, _seed(seed), rounds, first, count,
                                                   None if indices is None else _p(indices), _p(out)))
    return out


def shuffled_indices(index_count: int, seed, rounds: int = 90, first: int = 0, count=None) -> np.ndarray:
    """``[get_shuffled_index(i, index_count, seed) for i in range(first, first + count)]`` as uint32
    (``count`` defaults to the rest of the list)."""
    index_count, first = int(index_count), int(first)
    return _shuffle(index_count, seed, int(rounds), first, index_count - first if count is None else int(count), None)


def committee_bounds(n: int, committee_count: int) -> np.ndarray:
    """Boundaries of compute_committee's slices: committee j of ``committee_count`` over a list of
    ``n`` is positions [bounds[j], bounds[j + 1])."""
    if committee_count <= 0:
        raise ValueError("committee_count must be positive")
    return np.array([(n * j) // committee_count for j in range(committee_count + 1)], dtype=np.uint64)


def compute_committee(indices, seed, index: int, count: int, rounds: int = 90) -> np.ndarray:
    """compute_committee(indices, seed, index, count): committee ``index`` of ``count`` over the
    active ``indices``, as uint32."""
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    if not 0 <= index < count:
        raise ValueError("committee index out of range")
    n = len(indices)
    start, end = (n * index) // count, (n * (index + 1)) // count
    return _shuffle(n, seed, int(rounds), start, end - start, indices)


def attesting_entries(shuffled, committee_off, committee_len, aggregation_bitfields, custody_bitfields):
    """convert_to_indexed's index sets for a batch: attestation a's committee is
    ``shuffled[committee_off[a] : committee_off[a] + committee_len[a]]`` and its bitfields are
    ``aggregation_bitfields[a]`` / ``custody_bitfields[a]`` (bytes).  Returns
    ``(group_key_off, ok, entries)``: group 2a = custody bit 0, group 2a+1 = custody bit 1, each
    sorted, ``entries[group_key_off[g]:group_key_off[g + 1]]``; ``ok[a]`` is False (and both groups
    empty) when a bitfield fails verify_bitfield."""
    shuffled = np.ascontiguousarray(shuffled, dtype=np.uint32)
    coff = np.ascontiguousarray(committee_off, dtype=np.uint32)
    clen = np.ascontiguousarray(committee_len, dtype=np.uint32)
    n_att = len(coff)
    agg = [bytes(b) for b in aggregation_bitfields]
    cust = [bytes(b) for b in custody_bitfields]
    if not (len(clen) == len(agg) == len(cust) == n_att):
        raise ValueError("attesting_entries: one committee and two bitfields per attestation")
    # the engine takes one byte range per attestation for both bitfields; two bitfields of
    # different lengths cannot both pass verify_bitfield, so such a pair goes in as a pair of one
    # wrong length
    boff = np.zeros(n_att + 1, dtype=np.uint32)
    for a in range(n_att):
        if len(agg[a]) != len(cust[a]):
            agg[a] = cust[a] = bytes((int(clen[a]) + 7) // 8 + 1)
        boff[a + 1] = boff[a] + len(agg[a])
    agg_blob, cust_blob = b"".join(agg), b"".join(cust)
    gko = np.zeros(2 * n_att + 1, dtype=np.uint32)
    ok = np.zeros(n_att, dtype=np.uint8)
    cap = int(clen.sum())
    entries = np.zeros(cap, dtype=np.uint32)
    if n_att:
        _native.check(_native.lib().bls381_attesting_entries(
            n_att, _p(coff), _p(clen), _p(boff), agg_blob or None, cust_blob or None, _p(shuffled), len(shuffled),
            _p(gko), _p(ok), _p(entries), cap))
    return gko, ok.astype(bool), entries[:int(gko[-1])]


def get_attesting_indices(committee, bitfield) -> list:
    """The sorted attesting indices of ``bitfield`` over ``committee`` (a compute_committee
    result).  A bitfield that fails verify_bitfield raises AssertionError, as the spec's assert
    does."""
    committee = np.ascontiguousarray(committee, dtype=np.uint32)
    bitfield = bytes(bitfield)
    if len(committee) > MAX_INDICES_PER_ATTESTATION:
        raise ValueError("a committee holds at most %d members" % MAX_INDICES_PER_ATTESTATION)
    _, ok, entries = attesting_entries(committee, [0], [len(committee)], [bitfield], [bytes(len(bitfield))])
    if not ok[0]:
        raise AssertionError("verify_bitfield(bitfield, len(committee)) failed")
    return [int(v) for v in entries]
