"""The epoch context on the device: what the shuffle consumes, made from the validator fields.

Mirrors of the reference's functions (specs/core/0_beacon-chain.md), run by the engine
(include/bls381.h "epoch context"; csrc/bls381_epoch.hpp):

* ``active_validator_indices`` -- ``get_active_validator_indices`` (:680-684) with the active
  set's balance sum
* ``active_index_root``       -- ``hash_tree_root`` of that list as ``List[uint64]`` (:1545)
* ``beacon_proposer_indices`` -- the search of ``get_beacon_proposer_index`` (:822-840) for many
  slots at once

and the host arithmetic around them: ``generate_seed`` (:807-816, one 96-byte hash),
``epoch_committee_count`` / ``shard_delta`` / ``epoch_start_shard`` (:710-744).
``EpochCommittees`` composes them with the ``committees`` module into the committees and
proposers of one epoch.  Callers that keep the validator records in HBM use the ``_device`` entry
points directly.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from . import _native, committees

FAR_FUTURE_EPOCH = 2 ** 64 - 1
PROPOSER_NONE = 0xFFFFFFFF


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u64(values, what):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    if a.ndim != 1:
        raise ValueError("%s: one uint64 per validator" % what)
    return a


def active_validator_indices(activation_epochs, exit_epochs, epoch: int, effective_balances=None):
    """``(indices, total_balance)``: the ascending uint32 indices i with
    ``activation_epochs[i] <= epoch < exit_epochs[i]`` and the sum of their effective balances
    (0 without ``effective_balances``)."""
    act, ext = _u64(activation_epochs, "activation_epochs"), _u64(exit_epochs, "exit_epochs")
    bal = None if effective_balances is None else _u64(effective_balances, "effective_balances")
    n = len(act)
    if len(ext) != n or (bal is not None and len(bal) != n):
        raise ValueError("active_validator_indices: one entry per validator in every array")
    if not 0 <= int(epoch) < 1 << 64:
        raise ValueError("epoch is a uint64")
    out = np.zeros(n, dtype=np.uint32)
    count, total = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _native.check(_native.lib().bls381_active_indices(
        n, _p(act), _p(ext), 8, int(epoch), None if bal is None else _p(bal), 8, _p(out), ctypes.byref(count),
        ctypes.byref(total)))
    return out[:count.value], int(total.value)


def active_index_root(indices) -> bytes:
    """``hash_tree_root(List[uint64](indices))`` for indices below 2^32."""
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    root = np.zeros(32, dtype=np.uint8)
    _native.check(_native.lib().bls381_active_index_root(len(idx), _p(idx), _p(root)))
    return root.tobytes()


def generate_seed(randao_mix, active_index_root, epoch: int) -> bytes:
    """``hash(randao_mix + active_index_root + int_to_bytes(epoch, 32))``; the caller picks the mix
    of ``epoch + LATEST_RANDAO_MIXES_LENGTH - MIN_SEED_LOOKAHEAD``."""
    randao_mix, root = bytes(randao_mix), bytes(active_index_root)
    if len(randao_mix) != 32 or len(root) != 32:
        raise ValueError("generate_seed: a 32-byte mix and a 32-byte root")
    return hashlib.sha256(randao_mix + root + int(epoch).to_bytes(32, "little")).digest()


def epoch_committee_count(active_count: int, shard_count: int, slots_per_epoch: int, target_committee_size: int) -> int:
    return max(1, min(shard_count // slots_per_epoch,
                      active_count // slots_per_epoch // target_committee_size)) * slots_per_epoch


def shard_delta(active_count: int, shard_count: int, slots_per_epoch: int, target_committee_size: int) -> int:
    return min(epoch_committee_count(active_count, shard_count, slots_per_epoch, target_committee_size),
               shard_count - shard_count // slots_per_epoch)


def epoch_start_shard(latest_start_shard: int, current_epoch: int, epoch: int, active_count_at, shard_count: int,
                      slots_per_epoch: int, target_committee_size: int) -> int:
    """``get_epoch_start_shard``; ``active_count_at(e)`` is the active count of epoch e."""
    if epoch > current_epoch + 1:
        raise AssertionError("epoch <= get_current_epoch(state) + 1")
    delta = lambda e: shard_delta(active_count_at(e), shard_count, slots_per_epoch, target_committee_size)  # noqa: E731
    check_epoch = current_epoch + 1
    shard = (latest_start_shard + delta(current_epoch)) % shard_count
    while check_epoch > epoch:
        check_epoch -= 1
        shard = (shard + shard_count - delta(check_epoch)) % shard_count
    return shard


def beacon_proposer_indices(shuffled, committee_off, committee_len, effective_balances, seed, epoch: int,
                            max_effective_balance: int) -> np.ndarray:
    """One proposer per slot: slot k's first committee is
    ``shuffled[committee_off[k] : committee_off[k] + committee_len[k]]``.  ``PROPOSER_NONE``
    (0xFFFFFFFF) marks a slot whose search met a member outside ``effective_balances`` or found no
    proposer in 2^20 tries."""
    shuffled = np.ascontiguousarray(shuffled, dtype=np.uint32)
    coff = np.ascontiguousarray(committee_off, dtype=np.uint32)
    clen = np.ascontiguousarray(committee_len, dtype=np.uint32)
    bal = _u64(effective_balances, "effective_balances")
    if len(coff) != len(clen):
        raise ValueError("beacon_proposer_indices: one offset and one length per slot")
    out = np.zeros(len(coff), dtype=np.uint32)
    _native.check(_native.lib().bls381_proposer_indices(
        len(coff), _p(coff), _p(clen), _p(shuffled), len(shuffled), _p(bal), 8, len(bal), committees._seed(seed),
        int(epoch), int(max_effective_balance), _p(out)))
    return out


class EpochCommittees:
    """The committees and proposers of one epoch, from the validator arrays.

    ``start_shard`` is ``get_epoch_start_shard(state, epoch)`` (``epoch_start_shard`` above) and
    ``randao_mix`` the mix ``generate_seed`` reads for this epoch."""

    def __init__(self, activation_epochs, exit_epochs, effective_balances, epoch: int, randao_mix, start_shard: int, *,
                 shard_count: int = 1024, slots_per_epoch: int = 64, target_committee_size: int = 128,
                 shuffle_round_count: int = 90, max_effective_balance: int = 32 * 10 ** 9):
        self.epoch = int(epoch)
        self.shard_count, self.slots_per_epoch = shard_count, slots_per_epoch
        self.max_effective_balance = max_effective_balance
        self.effective_balances = _u64(effective_balances, "effective_balances")
        self.active, self.total_balance = active_validator_indices(activation_epochs, exit_epochs, epoch,
                                                                   self.effective_balances)
        self.index_root = active_index_root(self.active)
        self.seed = generate_seed(randao_mix, self.index_root, epoch)
        self.committee_count = epoch_committee_count(len(self.active), shard_count, slots_per_epoch,
                                                     target_committee_size)
        self.start_shard = int(start_shard)
        n = len(self.active)
        # every committee of the epoch is a slice of one shuffled list, gathered through the active set
        self.shuffled = committees._shuffle(n, self.seed, shuffle_round_count, 0, n, self.active)
        self.bounds = committees.committee_bounds(n, self.committee_count)
        self._proposers = None

    def crosslink_committee(self, shard: int) -> np.ndarray:
        j = (shard + self.shard_count - self.start_shard) % self.shard_count
        if j >= self.committee_count:
            raise ValueError("shard has no committee in this epoch")
        return self.shuffled[int(self.bounds[j]):int(self.bounds[j + 1])]

    def proposers(self) -> np.ndarray:
        """The proposer of every slot of the epoch (``PROPOSER_NONE`` for a slot whose first
        committee is empty, where the spec divides by zero)."""
        if self._proposers is None:
            per_slot = self.committee_count // self.slots_per_epoch
            first = [per_slot * s for s in range(self.slots_per_epoch)]
            off = np.array([self.bounds[j] for j in first], dtype=np.uint32)
            length = np.array([self.bounds[j + 1] - self.bounds[j] for j in first], dtype=np.uint32)
            out = np.full(self.slots_per_epoch, PROPOSER_NONE, dtype=np.uint32)
            full = np.flatnonzero(length)
            if len(full):
                out[full] = beacon_proposer_indices(self.shuffled, off[full], length[full], self.effective_balances,
                                                    self.seed, self.epoch, self.max_effective_balance)
            self._proposers = out
        return self._proposers

    def proposer(self, slot: int) -> int:
        return int(self.proposers()[slot % self.slots_per_epoch])
