"""Epoch rewards on the device: the whole-registry work of ``process_epoch``.

Mirrors of the reference's functions (specs/core/0_beacon-chain.md), run by the engine
(include/bls381.h "epoch rewards"; csrc/bls381_rewards.hpp):

* ``epoch_votes``               -- the ``PendingAttestation``s of one epoch as per-validator facts
  (``get_unslashed_attesting_indices``, :1294-1300, of the matching source / target / head
  attestations; the attestation ``min(..., key=inclusion_delay)`` picks, :1424-1427) and
  per-committee crosslink results (``get_winning_crosslink_and_attesting_indices``, :1308-1321)
* ``epoch_deltas``              -- ``get_attestation_deltas`` / ``get_crosslink_deltas`` and their
  application (``process_rewards_and_penalties``, :1389-1475)
* ``epoch_slashings``           -- ``process_slashings`` (:1505-1524)
* ``effective_balance_updates`` -- the hysteresis of ``process_final_updates`` (:1535-1540)

numpy in, numpy out.  ``EpochVotes.from_pending_attestations`` does the host work the device rules
assume (sorting by committee, candidate ids).  ``process_rewards_and_penalties``,
``process_slashings`` and ``update_effective_balances`` act on a ``state_tree.balances_tree`` and a
``state_tree.validator_registry_tree`` through the ``_device`` entry points: they read the records
and balances where the trees keep them, hand the results to the trees' device updates and copy no
per-validator array to the host (their scratch buffers are torch tensors on the current device).
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

NONE = 0xFFFFFFFF
VOTE_SOURCE, VOTE_TARGET, VOTE_HEAD, VOTE_WINNER, VOTE_MEMBER = 1, 2, 4, 8, 16
DEFAULT_CROSSLINK = (0, 0, 0, bytes(32), bytes(32))
RECORD = 121    # serialized Validator (:284-298) and its fields' offsets
OFF_ACTIVATION, OFF_EXIT, OFF_WITHDRAWABLE, OFF_SLASHED, OFF_EFFECTIVE = 88, 96, 104, 112, 113


class RewardConstants(ctypes.Structure):
    """``bls381_reward_constants``."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "base_reward_factor", "base_rewards_per_epoch", "proposer_reward_quotient", "min_attestation_inclusion_delay",
        "min_epochs_to_inactivity_penalty", "inactivity_penalty_quotient")]

    @classmethod
    def from_preset(cls, constants) -> "RewardConstants":
        """From a mapping with the spec's names (BASE_REWARD_FACTOR, ...)."""
        return cls(*[int(constants[name.upper()]) for name, _ in cls._fields_])


MAINNET = RewardConstants(32, 5, 8, 4, 4, 1 << 25)    # configs/constant_presets/mainnet.yaml


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arr(values, dtype, what):
    a = np.ascontiguousarray(values, dtype=dtype)
    if a.ndim != 1:
        raise ValueError("%s: a flat array" % what)
    return a


def _same_length(n, what, *arrays):
    if any(len(a) != n for a in arrays):
        raise ValueError("%s: one entry per validator in every array" % what)


def _raise_on(overflows: int, what: str) -> None:
    if overflows:
        raise OverflowError("%s: %d overflows (a quotient of 2^64 or more, a wrapped sum or balance, a proposer "
                            "micro-reward of 2^32 or more, or an index or delay out of range)" % (what, overflows))


# ---- call 1 ------------------------------------------------------------------------------------
def epoch_votes(committee_off, committee_len, shuffled, slashed, effective_balances, att_off, bits_off, aggregation_bits,
                att_flags, att_inclusion_delay, att_proposer, att_candidate, cand_count) -> dict:
    """``bls381_epoch_votes``: a dict of ``votes``, ``incl_delay``, ``incl_proposer``, ``committee_of``
    (one per validator), ``winner``, ``winner_balance``, ``committee_balance`` (one per committee) and
    ``totals`` (the three unfloored attesting balances)."""
    coff, clen = _arr(committee_off, np.uint32, "committee_off"), _arr(committee_len, np.uint32, "committee_len")
    sh = _arr(shuffled, np.uint32, "shuffled")
    sl, eff = _arr(slashed, np.uint8, "slashed"), _arr(effective_balances, np.uint64, "effective_balances")
    aoff, boff = _arr(att_off, np.uint32, "att_off"), _arr(bits_off, np.uint32, "bits_off")
    bits = np.frombuffer(bytes(aggregation_bits), dtype=np.uint8)
    flags, delay = _arr(att_flags, np.uint8, "att_flags"), _arr(att_inclusion_delay, np.uint64, "att_inclusion_delay")
    prop, cand = _arr(att_proposer, np.uint32, "att_proposer"), _arr(att_candidate, np.uint32, "att_candidate")
    kc = _arr(cand_count, np.uint32, "cand_count")
    n, nc = len(eff), len(coff)
    if len(sl) != n or len(clen) != nc or len(kc) != nc or len(aoff) != nc + 1:
        raise ValueError("epoch_votes: one entry per validator / committee, and n_committees + 1 offsets")
    n_att = int(aoff[-1])
    if len(boff) != n_att + 1 or any(len(a) != n_att for a in (flags, delay, prop, cand)) or len(bits) != int(boff[-1]):
        raise ValueError("epoch_votes: one entry per attestation, and n_att + 1 bit offsets")
    out = {"votes": np.zeros(n, np.uint32), "incl_delay": np.zeros(n, np.uint64), "incl_proposer": np.zeros(n, np.uint32),
           "committee_of": np.zeros(n, np.uint32), "winner": np.zeros(nc, np.uint32),
           "winner_balance": np.zeros(nc, np.uint64), "committee_balance": np.zeros(nc, np.uint64),
           "totals": np.zeros(3, np.uint64)}
    _native.check(_native.lib().bls381_epoch_votes(
        nc, _p(coff), _p(clen), _p(sh), len(sh), n, _p(sl), 1, _p(eff), 8, _p(aoff), _p(boff), _p(bits), _p(flags), _p(delay),
        _p(prop), _p(cand), _p(kc), _p(out["votes"]), _p(out["incl_delay"]), _p(out["incl_proposer"]), _p(out["committee_of"]),
        _p(out["winner"]), _p(out["winner_balance"]), _p(out["committee_balance"]), _p(out["totals"])))
    return out


def assign_candidates(attestations):
    """One committee's attestations in list order, each with ``crosslink`` (shard, start_epoch,
    end_epoch, parent_root, data_root) and ``passes_filter`` (the caller's verdict of the
    parent_root / hash_tree_root filter, :1312-1315).  Returns (candidate id per attestation, the
    crosslink of each id): ids ascend by data_root and, among equal data_roots, by descending
    first appearance, so the device's "largest balance, then largest id" is the spec's
    ``max(key=(balance, data_root))`` with the first in list order winning among equal keys.
    Attestations the filter rejects get no candidate; where no crosslink passes, those equal to
    ``Crosslink()`` form candidate 0 (``default=Crosslink()``, :1319-1320)."""
    passing = []
    for a in attestations:
        if a["passes_filter"] and a["crosslink"] not in passing:
            passing.append(a["crosslink"])
    if passing:
        order = sorted(range(len(passing)), key=lambda k: (passing[k][4], -k))
        rank = {passing[k]: r for r, k in enumerate(order)}
        return [rank.get(a["crosslink"], NONE) for a in attestations], [passing[k] for k in order]
    cand = [0 if a["crosslink"] == DEFAULT_CROSSLINK else NONE for a in attestations]
    return cand, ([DEFAULT_CROSSLINK] if 0 in cand else [])


class EpochVotes:
    """The inputs of ``bls381_epoch_votes`` for one epoch, and its outputs once ``run``."""

    def __init__(self, shuffled, committee_off, committee_len, slashed, effective_balances, per_committee):
        """per_committee[c]: the committee's attestations in list order, dicts with ``bits`` (bytes),
        ``target``, ``head``, ``inclusion_delay``, ``proposer_index``, ``crosslink``, ``passes_filter``."""
        self.shuffled = _arr(shuffled, np.uint32, "shuffled")
        self.committee_off = _arr(committee_off, np.uint32, "committee_off")
        self.committee_len = _arr(committee_len, np.uint32, "committee_len")
        self.slashed = _arr(slashed, np.uint8, "slashed")
        self.effective_balances = _arr(effective_balances, np.uint64, "effective_balances")
        att_off, bits_off, bits, flags, delay, proposer, cand, kc, self.crosslinks = [0], [0], [], [], [], [], [], [], []
        for atts in per_committee:
            ids, links = assign_candidates(atts)
            for a, k in zip(atts, ids):
                bits.append(bytes(a["bits"]))
                bits_off.append(bits_off[-1] + len(bits[-1]))
                flags.append(int(bool(a["target"])) | int(bool(a["head"])) << 1)
                delay.append(int(a["inclusion_delay"]))
                proposer.append(int(a["proposer_index"]))
                cand.append(k)
            att_off.append(len(flags))
            kc.append(len(links))
            self.crosslinks.append(links)
        self.att_off, self.bits_off = np.array(att_off, np.uint32), np.array(bits_off, np.uint32)
        self.bits = b"".join(bits)
        self.flags, self.delay = np.array(flags, np.uint8), np.array(delay, np.uint64)
        self.proposer, self.cand = np.array(proposer, np.uint32), np.array(cand, np.uint32)
        self.cand_count = np.array(kc, np.uint32)
        self.out = None

    @classmethod
    def from_pending_attestations(cls, committees, attestations, slashed, effective_balances) -> "EpochVotes":
        """``committees``: the epoch's ``epoch.EpochCommittees`` (its ``shuffled``, ``bounds``,
        ``start_shard``, ``shard_count`` and ``committee_count`` are read).  ``attestations``: the
        state's list for that epoch, in order, each a mapping with ``shard``,
        ``aggregation_bitfield``, ``inclusion_delay``, ``proposer_index``, ``target`` and ``head`` (the
        caller's root comparisons), ``crosslink`` (shard, start_epoch, end_epoch, parent_root,
        data_root) and ``passes_filter``.  Sorts them by committee, stably."""
        count = int(committees.committee_count)
        per = [[] for _ in range(count)]
        for a in attestations:
            j = (int(a["shard"]) + committees.shard_count - committees.start_shard) % committees.shard_count
            if j >= count:
                raise ValueError("an attestation names a shard without a committee in this epoch")
            per[j].append({"bits": a["aggregation_bitfield"], "target": a["target"], "head": a["head"],
                           "inclusion_delay": a["inclusion_delay"], "proposer_index": a["proposer_index"],
                           "crosslink": tuple(a["crosslink"]), "passes_filter": a["passes_filter"]})
        bounds = [int(b) for b in committees.bounds]
        return cls(committees.shuffled, bounds[:-1], [bounds[j + 1] - bounds[j] for j in range(count)], slashed,
                   effective_balances, per)

    def arguments(self):
        """The host-array arguments of both forms, in the header's order, after the fields."""
        return (self.att_off, self.bits_off, self.bits, self.flags, self.delay, self.proposer, self.cand, self.cand_count)

    def run(self) -> dict:
        """The host-pointer form; the outputs stay in ``self.out``."""
        self.out = epoch_votes(self.committee_off, self.committee_len, self.shuffled, self.slashed, self.effective_balances,
                               *self.arguments())
        return self.out

    def winning_crosslink(self, committee: int):
        """The winning crosslink of a committee after ``run`` (``Crosslink()``'s fields without one)."""
        w = int(self.out["winner"][committee])
        return DEFAULT_CROSSLINK if w == NONE else self.crosslinks[committee][w]

    def run_device(self, registry_tree, d_shuffled: int, n_shuffled: int) -> "DeviceVotes":
        """The device form over the records of a ``validator_registry_tree`` and a shuffled list in
        device memory (what ``bls381_shuffle_device`` wrote), queued on torch's current stream."""
        import torch
        L = _native.lib()
        n, nc = registry_tree.count, len(self.committee_off)
        dv = DeviceVotes(n, nc)
        n_att = int(self.att_off[-1])
        ws = torch.empty(max(1, L.bls381_epoch_votes_workspace_size(nc, n_att, int(self.bits_off[-1]))), dtype=torch.uint8,
                         device="cuda")
        rec = registry_tree.items_ptr
        bits = np.frombuffer(self.bits, dtype=np.uint8)
        _native.check(L.bls381_epoch_votes_device(
            nc, _p(self.committee_off), _p(self.committee_len), d_shuffled, n_shuffled, n, rec + OFF_SLASHED, RECORD,
            rec + OFF_EFFECTIVE, RECORD, _p(self.att_off), _p(self.bits_off), _p(bits), _p(self.flags), _p(self.delay),
            _p(self.proposer), _p(self.cand), _p(self.cand_count), dv.votes.data_ptr(), dv.incl_delay.data_ptr(),
            dv.incl_proposer.data_ptr(), dv.committee_of.data_ptr(), dv.winner.data_ptr(), dv.winner_balance.data_ptr(),
            dv.committee_balance.data_ptr(), dv.totals.data_ptr(), ws.data_ptr(), _stream()))
        dv.keep = ws
        return dv


class DeviceVotes:
    """The outputs of ``bls381_epoch_votes_device`` as torch tensors (uint64 values in int64 tensors)."""

    def __init__(self, n: int, n_committees: int):
        import torch
        self.n, self.n_committees = n, n_committees
        i32 = lambda k: torch.zeros(max(1, k), dtype=torch.int32, device="cuda")   # noqa: E731
        i64 = lambda k: torch.zeros(max(1, k), dtype=torch.int64, device="cuda")   # noqa: E731
        self.votes, self.incl_proposer, self.committee_of, self.winner = i32(n), i32(n), i32(n), i32(n_committees)
        self.incl_delay, self.winner_balance, self.committee_balance, self.totals = i64(n), i64(n_committees), i64(
            n_committees), i64(3)
        self.keep = None


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- call 2 ------------------------------------------------------------------------------------
def epoch_deltas(activation_epochs, exit_epochs, withdrawable_epochs, effective_balances, slashed, votes: dict, balances,
                 previous_epoch: int, finalized_epoch: int, total_balance: int, constants: RewardConstants = MAINNET,
                 which: int = 3):
    """``bls381_epoch_deltas`` over the dict ``epoch_votes`` returned for the previous epoch:
    ``(rewards, penalties, new_balances)``.  ``OverflowError`` when the status word is not 0."""
    act, ext = _arr(activation_epochs, np.uint64, "activation_epochs"), _arr(exit_epochs, np.uint64, "exit_epochs")
    wd, eff = _arr(withdrawable_epochs, np.uint64, "withdrawable_epochs"), _arr(effective_balances, np.uint64,
                                                                              "effective_balances")
    sl, bal = _arr(slashed, np.uint8, "slashed"), _arr(balances, np.uint64, "balances")
    n = len(eff)
    v = {k: np.ascontiguousarray(votes[k]) for k in ("votes", "incl_delay", "incl_proposer", "committee_of", "winner_balance",
                                                      "committee_balance", "totals")}
    _same_length(n, "epoch_deltas", act, ext, wd, sl, bal, v["votes"], v["incl_delay"], v["incl_proposer"], v["committee_of"])
    nc = len(v["winner_balance"])
    rewards, penalties, new = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    overflows = ctypes.c_uint64(0)
    _native.check(_native.lib().bls381_epoch_deltas(
        n, _p(act), _p(ext), _p(wd), _p(eff), 8, _p(sl), 1, _p(v["votes"].astype(np.uint32)), _p(v["incl_delay"].astype(np.uint64)),
        _p(v["incl_proposer"].astype(np.uint32)), _p(v["committee_of"].astype(np.uint32)), nc,
        _p(v["winner_balance"].astype(np.uint64)), _p(v["committee_balance"].astype(np.uint64)),
        _p(v["totals"].astype(np.uint64)), _p(bal), int(previous_epoch), int(finalized_epoch), int(total_balance),
        ctypes.byref(constants), int(which), _p(rewards), _p(penalties), _p(new), ctypes.byref(overflows)))
    _raise_on(overflows.value, "epoch_deltas")
    return rewards, penalties, new


# ---- call 3 ------------------------------------------------------------------------------------
def epoch_slashings(slashed, withdrawable_epochs, effective_balances, balances, current_epoch: int, total_penalties: int,
                    total_balance: int, latest_slashed_exit_length: int = 8192,
                    min_slashing_penalty_quotient: int = 32) -> np.ndarray:
    """``bls381_epoch_slashings``: the balances after ``process_slashings``."""
    sl, wd = _arr(slashed, np.uint8, "slashed"), _arr(withdrawable_epochs, np.uint64, "withdrawable_epochs")
    eff = _arr(effective_balances, np.uint64, "effective_balances")
    bal = np.array(balances, dtype=np.uint64)
    _same_length(len(eff), "epoch_slashings", sl, wd, bal)
    _native.check(_native.lib().bls381_epoch_slashings(len(eff), _p(sl), 1, _p(wd), _p(eff), 8, int(current_epoch),
                                                       int(total_penalties), int(total_balance),
                                                       int(latest_slashed_exit_length), int(min_slashing_penalty_quotient),
                                                       _p(bal)))
    return bal


# ---- call 4 ------------------------------------------------------------------------------------
def effective_balance_updates(balances, effective_balances, increment: int = 10 ** 9,
                              max_effective_balance: int = 32 * 10 ** 9):
    """``bls381_effective_balances``: ``(indices, values, changed)`` -- ``indices[i]`` is i where
    validator i's effective balance changes and 0xFFFFFFFF where it does not."""
    bal, eff = _arr(balances, np.uint64, "balances"), _arr(effective_balances, np.uint64, "effective_balances")
    n = len(eff)
    _same_length(n, "effective_balance_updates", bal)
    indices, values, changed = np.zeros(n, np.uint32), np.zeros(n, np.uint64), ctypes.c_uint64(0)
    _native.check(_native.lib().bls381_effective_balances(n, _p(bal), _p(eff), 8, int(increment), int(max_effective_balance),
                                                          _p(indices), _p(values), ctypes.byref(changed)))
    return indices, values, int(changed.value)


# ---- the trees ---------------------------------------------------------------------------------
def _trees(balances_tree, registry_tree):
    n = registry_tree.count
    if balances_tree.count != n or registry_tree.item_size != RECORD or balances_tree.item_size != 8:
        raise ValueError("a balances tree and a validator registry tree of one length")
    return n, balances_tree.items_ptr, registry_tree.items_ptr


def _update(tree, n, d_indices, off, length, d_values) -> None:
    import torch
    L = _native.lib()
    ws = torch.empty(max(1, L.bls381_list_tree_update_workspace_size(tree._handle(), n)), dtype=torch.uint8, device="cuda")
    _native.check(L.bls381_list_tree_update_device(tree._handle(), n, d_indices.data_ptr(), off, length, d_values.data_ptr(),
                                                   ws.data_ptr(), _stream()))
    torch.cuda.current_stream().synchronize()   # the scratch tensors go back to torch's allocator below


def _every_index(n):
    import torch
    return torch.arange(max(1, n), dtype=torch.int32, device="cuda")


def process_rewards_and_penalties(balances_tree, registry_tree, votes: DeviceVotes, current_epoch: int,
                                  finalized_epoch: int, d_total_balance: int, constants: RewardConstants = MAINNET,
                                  genesis_epoch: int = 0, which: int = 3) -> int:
    """``process_rewards_and_penalties`` over the trees: the deltas of the previous epoch's
    ``votes`` (``EpochVotes.run_device``) applied to every balance of ``balances_tree``.
    ``d_total_balance``: the device address of ``get_total_active_balance`` (``d_count_and_total + 1``
    of ``bls381_active_indices_device``).  Returns the status word (0 in the genesis epoch, where
    nothing runs); ``OverflowError`` when it is not 0 -- the tree is updated all the same."""
    import torch
    if int(current_epoch) == int(genesis_epoch):
        return 0
    n, d_bal, rec = _trees(balances_tree, registry_tree)
    if votes.n != n:
        raise ValueError("the votes are of another registry")
    L = _native.lib()
    i64 = lambda k: torch.empty(max(1, k), dtype=torch.int64, device="cuda")   # noqa: E731
    rewards, penalties, new, status = i64(n), i64(n), i64(n), i64(1)
    ws = torch.empty(max(1, L.bls381_epoch_deltas_workspace_size(n)), dtype=torch.uint8, device="cuda")
    _native.check(L.bls381_epoch_deltas_device(
        n, rec + OFF_ACTIVATION, rec + OFF_EXIT, rec + OFF_WITHDRAWABLE, rec + OFF_EFFECTIVE, RECORD, rec + OFF_SLASHED, RECORD,
        votes.votes.data_ptr(), votes.incl_delay.data_ptr(), votes.incl_proposer.data_ptr(), votes.committee_of.data_ptr(),
        votes.n_committees, votes.winner_balance.data_ptr(), votes.committee_balance.data_ptr(), votes.totals.data_ptr(), d_bal,
        int(current_epoch) - 1, int(finalized_epoch), d_total_balance, ctypes.byref(constants), int(which),
        rewards.data_ptr(), penalties.data_ptr(), new.data_ptr(), status.data_ptr(), ws.data_ptr(), _stream()))
    _update(balances_tree, n, _every_index(n), 0, 8, new)
    overflows = int(status.cpu()[0]) & (2 ** 64 - 1)
    _raise_on(overflows, "process_rewards_and_penalties")
    return overflows


def process_slashings(balances_tree, registry_tree, current_epoch: int, total_penalties: int, d_total_balance: int,
                      latest_slashed_exit_length: int = 8192, min_slashing_penalty_quotient: int = 32) -> int:
    """``process_slashings`` over the trees; ``total_penalties`` is the caller's difference of
    ``latest_slashed_balances``.  Returns 0 (the call has no overflow)."""
    n, d_bal, rec = _trees(balances_tree, registry_tree)
    if n == 0:
        return 0
    new = _device_copy(d_bal, n)
    _native.check(_native.lib().bls381_epoch_slashings_device(
        n, rec + OFF_SLASHED, RECORD, rec + OFF_WITHDRAWABLE, rec + OFF_EFFECTIVE, RECORD, int(current_epoch),
        int(total_penalties), d_total_balance, int(latest_slashed_exit_length), int(min_slashing_penalty_quotient),
        new.data_ptr(), _stream()))
    _update(balances_tree, n, _every_index(n), 0, 8, new)
    return 0


def update_effective_balances(balances_tree, registry_tree, increment: int = 10 ** 9,
                              max_effective_balance: int = 32 * 10 ** 9) -> int:
    """The hysteresis of ``process_final_updates`` over the trees: the registry tree's
    ``effective_balance`` fields move where the balances say so.  Returns how many changed."""
    import torch
    n, d_bal, rec = _trees(balances_tree, registry_tree)
    if n == 0:
        return 0
    indices = torch.empty(n, dtype=torch.int32, device="cuda")
    values, changed = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
    _native.check(_native.lib().bls381_effective_balances_device(n, d_bal, rec + OFF_EFFECTIVE, RECORD, int(increment),
                                                                 int(max_effective_balance), indices.data_ptr(),
                                                                 values.data_ptr(), changed.data_ptr(), _stream()))
    _update(registry_tree, n, indices, OFF_EFFECTIVE, 8, values)
    return int(changed.cpu()[0])


class _DeviceWords:
    """n 64-bit words at a device address, for ``torch.as_tensor``."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2, "strides": None}


def _device_copy(ptr: int, n: int):
    """A torch tensor holding a copy of n uint64 at a device address (the trees' stores are
    read-only for callers)."""
    import torch
    return torch.as_tensor(_DeviceWords(ptr, n), device="cuda").clone()
