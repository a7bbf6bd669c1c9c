"""Registry updates on the device: ejections, the exit queue and the activation queue.

Mirrors of the reference's functions (specs/core/0_beacon-chain.md), run by the engine
(include/bls381.h "registry updates"; csrc/bls381_regupd.hpp):

* ``registry_updates``          -- ``process_registry_updates`` (:1480-1502) over plain arrays:
  which validators change and the four epochs of every validator after the call
* ``exit_queue``                -- ``initiate_validator_exit``'s view of a registry (:1119-1124):
  the exit queue's epoch, how many validators hold it, the churn limit and the active count
* ``ExitQueue``                 -- that view as an object whose ``initiate()`` hands out the next
  ``(exit_epoch, withdrawable_epoch)``: a block's voluntary exits and slashings without a scan each
* ``process_registry_updates``  -- the call over a ``state_tree.validator_registry_tree`` through the
  ``_device`` entry point: it reads the records where the tree keeps them, hands indices and values
  to the tree's device update and copies only the eight-word summary to the host

numpy in, numpy out for the first two.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _native

NONE = 0xFFFFFFFF
FAR_FUTURE_EPOCH = 2 ** 64 - 1
RECORD = 121    # serialized Validator (:284-298) and its fields' offsets
OFF_ELIGIBILITY, OFF_ACTIVATION, OFF_EXIT, OFF_WITHDRAWABLE, OFF_EFFECTIVE = 80, 88, 96, 104, 113
STATUS_NO_CHURN = 1 << 63   # the device form's mark for a churn limit of 0


class RegistryConstants(ctypes.Structure):
    """``bls381_registry_constants``."""
    _fields_ = [(name, ctypes.c_uint64) for name in (
        "max_effective_balance", "ejection_balance", "activation_exit_delay", "min_validator_withdrawability_delay",
        "min_per_epoch_churn_limit", "churn_limit_quotient")]

    @classmethod
    def from_preset(cls, constants) -> "RegistryConstants":
        """From a mapping with the spec's names (MAX_EFFECTIVE_BALANCE, ...)."""
        return cls(*[int(constants[name.upper()]) for name, _ in cls._fields_])


MAINNET = RegistryConstants(32 * 10 ** 9, 16 * 10 ** 9, 4, 256, 4, 65536)   # configs/constant_presets/mainnet.yaml


class Summary(NamedTuple):
    """The eight words a call hands back."""
    eligible_set: int
    ejected: int
    activated: int
    changed: int
    active_count: int
    churn_limit: int
    exit_queue_epoch: int   # E0: before the call
    status: int


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arr(values, what):
    a = np.ascontiguousarray(values, dtype=np.uint64)
    if a.ndim != 1:
        raise ValueError("%s: a flat array" % what)
    return a


def _raise_on(status: int, what: str) -> None:
    if status & STATUS_NO_CHURN:
        raise ValueError("%s: a churn limit of 0 (no minimum and too few active validators)" % what)
    if status:
        raise OverflowError("%s: %d validators whose exit_epoch or withdrawable_epoch passed 2^64 - 1" % (what, status))


def registry_updates(activation_eligibility_epochs, activation_epochs, exit_epochs, withdrawable_epochs,
                     effective_balances, current_epoch: int, finalized_epoch: int,
                     constants: RegistryConstants = MAINNET):
    """``bls381_registry_updates``: ``(indices, values, summary)`` -- ``indices[i]`` is i where one of
    validator i's four epochs changes and 0xFFFFFFFF where none does, ``values[i]`` the four epochs
    (eligibility, activation, exit, withdrawable) after the call, ``summary`` a ``Summary`` whose
    status the caller looks at (no exception for wrapped epochs here: the values are part of the
    result)."""
    el, act = _arr(activation_eligibility_epochs, "activation_eligibility_epochs"), _arr(activation_epochs, "activation_epochs")
    ext, wd = _arr(exit_epochs, "exit_epochs"), _arr(withdrawable_epochs, "withdrawable_epochs")
    eff = _arr(effective_balances, "effective_balances")
    n = len(eff)
    if any(len(a) != n for a in (el, act, ext, wd)):
        raise ValueError("registry_updates: one entry per validator in every array")
    indices, values, summary = np.zeros(n, np.uint32), np.zeros((n, 4), np.uint64), np.zeros(8, np.uint64)
    _native.check(_native.lib().bls381_registry_updates(n, _p(el), _p(act), _p(ext), _p(wd), _p(eff), 8, int(current_epoch),
                                                        int(finalized_epoch), ctypes.byref(constants), _p(indices),
                                                        _p(values), _p(summary)))
    return indices, values, Summary(*[int(x) for x in summary])


def exit_queue(activation_epochs, exit_epochs, current_epoch: int, constants: RegistryConstants = MAINNET) -> "ExitQueue":
    """``bls381_exit_queue`` over plain arrays."""
    act, ext = _arr(activation_epochs, "activation_epochs"), _arr(exit_epochs, "exit_epochs")
    if len(act) != len(ext):
        raise ValueError("exit_queue: one entry per validator in both arrays")
    q = np.zeros(4, np.uint64)
    _native.check(_native.lib().bls381_exit_queue(len(act), _p(act), _p(ext), 8, int(current_epoch),
                                                  ctypes.byref(constants), _p(q)))
    return ExitQueue(int(q[0]), int(q[1]), int(q[2]), int(q[3]), int(constants.min_validator_withdrawability_delay))


class ExitQueue:
    """``initiate_validator_exit`` for a caller processing a block: ``epoch`` is the exit queue's
    epoch, ``churn`` how many validators hold it, ``churn_limit`` the limit (constant while the
    active set at the current epoch is, which exits never change)."""

    def __init__(self, epoch: int, churn: int, churn_limit: int, active_count: int,
                 min_validator_withdrawability_delay: int):
        if churn_limit <= 0:
            raise ValueError("ExitQueue: a churn limit of 0")
        self.epoch, self.churn, self.churn_limit, self.active_count = epoch, churn, churn_limit, active_count
        self.delay = min_validator_withdrawability_delay

    @classmethod
    def of_tree(cls, registry_tree, current_epoch: int, constants: RegistryConstants = MAINNET) -> "ExitQueue":
        """Over the records of a ``validator_registry_tree``, where the tree keeps them."""
        import torch
        n, rec = _records(registry_tree)
        L = _native.lib()
        q = torch.zeros(4, dtype=torch.int64, device="cuda")
        ws = torch.empty(max(1, L.bls381_registry_updates_workspace_size(n)), dtype=torch.uint8, device="cuda")
        _native.check(L.bls381_exit_queue_device(n, rec + OFF_ACTIVATION, rec + OFF_EXIT, RECORD, int(current_epoch),
                                                 ctypes.byref(constants), q.data_ptr(), ws.data_ptr(), _stream()))
        e0, c0, limit, active = [int(x) & (2 ** 64 - 1) for x in q.cpu()]
        return cls(e0, c0, limit, active, int(constants.min_validator_withdrawability_delay))

    def initiate(self):
        """The next ``(exit_epoch, withdrawable_epoch)``; the queue moves on.  The caller skips
        validators that already have an exit epoch (:1116-1117).  ``OverflowError`` leaves the queue
        as it was."""
        epoch, churn = (self.epoch + 1, 0) if self.churn >= self.churn_limit else (self.epoch, self.churn)
        if epoch + self.delay > FAR_FUTURE_EPOCH:
            raise OverflowError("ExitQueue: the withdrawable epoch passes 2^64 - 1")   # the queue stays where it is
        self.epoch, self.churn = epoch, churn + 1
        return epoch, epoch + self.delay


# ---- the tree ----------------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _records(registry_tree):
    if registry_tree.item_size != RECORD:
        raise ValueError("a validator registry tree")
    return registry_tree.count, registry_tree.items_ptr


def process_registry_updates(registry_tree, current_epoch: int, finalized_epoch: int,
                             constants: RegistryConstants = MAINNET) -> Summary:
    """``process_registry_updates`` over the tree: the four epochs of its records move where the
    spec moves them.  Returns the ``Summary``; ``OverflowError`` when its status is not 0 (the tree is
    updated all the same), ``ValueError`` for a churn limit of 0 (nothing changes then)."""
    import torch
    n, rec = _records(registry_tree)
    L = _native.lib()
    indices = torch.empty(max(1, n), dtype=torch.int32, device="cuda")
    values = torch.empty(max(1, 4 * n), dtype=torch.int64, device="cuda")
    summary = torch.empty(8, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(1, L.bls381_registry_updates_workspace_size(n)), dtype=torch.uint8, device="cuda")
    _native.check(L.bls381_registry_updates_device(
        n, rec + OFF_ELIGIBILITY, rec + OFF_ACTIVATION, rec + OFF_EXIT, rec + OFF_WITHDRAWABLE, rec + OFF_EFFECTIVE, RECORD,
        int(current_epoch), int(finalized_epoch), ctypes.byref(constants), indices.data_ptr(), values.data_ptr(),
        summary.data_ptr(), ws.data_ptr(), _stream()))
    if n:
        uws = torch.empty(max(1, L.bls381_list_tree_update_workspace_size(registry_tree._handle(), n)), dtype=torch.uint8,
                          device="cuda")
        _native.check(L.bls381_list_tree_update_device(registry_tree._handle(), n, indices.data_ptr(), OFF_ELIGIBILITY, 32,
                                                       values.data_ptr(), uws.data_ptr(), _stream()))
    out = Summary(*[int(x) & (2 ** 64 - 1) for x in summary.cpu()])   # synchronises: the scratch tensors may go
    torch.cuda.current_stream().synchronize()
    _raise_on(out.status, "process_registry_updates")
    return out
