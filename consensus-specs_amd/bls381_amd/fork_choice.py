"""Fork choice on the device: latest messages and the LMD-GHOST head.

``lmd_ghost`` of the reference (specs/core/0_fork-choice.md:78-103) run by the engine
(include/bls381.h "fork choice"; csrc/bls381_forkchoice.hpp):

* ``ForkChoice``  -- a store: the block tree on the host, one latest message per validator on the
  device.  ``add_block`` / ``add_blocks``, ``on_attestations`` (numpy arrays, or the device
  pointers the grouped verify works on), ``head`` (over a ``state_tree.validator_registry_tree``
  where the tree keeps its records, or over plain arrays), ``vote_counts``, ``latest``, ``prune``
* ``lmd_ghost``   -- one-shot, numpy in, numpy out

The registry handed to ``head`` is the start state's: for the spec's head, the justified state's.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native

NONE = 0xFFFFFFFF
RECORD = 121    # serialized Validator (0_beacon-chain.md:284-298) and its fields' offsets
OFF_ACTIVATION, OFF_EXIT, OFF_EFFECTIVE = 88, 96, 113


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _arr(values, dtype, what):
    a = np.ascontiguousarray(values, dtype=dtype)
    if a.ndim != 1:
        raise ValueError("%s: a flat array" % what)
    return a


def _root(root, what="root") -> bytes:
    root = bytes(root)
    if len(root) != 32:
        raise ValueError("%s must be 32 bytes" % what)
    return root


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bounds(slots, n_att_after: int) -> None:
    """The store keeps slots and attestation numbers below 2^32."""
    if len(slots) and int(np.max(slots)) >= 1 << 32:
        raise OverflowError("fork choice: a slot at or above 2^32")
    if n_att_after > 0xFFFFFFFF:
        raise OverflowError("fork choice: more than 2^32 - 1 attestations over the life of the store")


class ForkChoice:
    """``bls381_fork_choice``: at most ``block_capacity`` blocks, validators below ``validator_capacity``."""

    def __init__(self, validator_capacity: int, block_capacity: int):
        self.validator_capacity, self.block_capacity = int(validator_capacity), int(block_capacity)
        h = ctypes.c_void_p()
        _native.check(_native.lib().bls381_fork_choice_create(self.validator_capacity, self.block_capacity, ctypes.byref(h)))
        self._h = h
        self._attestations = 0
        self._counts = None

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().bls381_fork_choice_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ValueError("the fork choice store is closed")
        return self._h

    # ---- blocks ------------------------------------------------------------------------------------
    def __len__(self) -> int:
        return int(_native.lib().bls381_fork_choice_block_count(self._handle()))

    def add_blocks(self, roots, parent_roots, slots) -> np.ndarray:
        """Appends blocks (parents first); returns their node ids.  The first block ever added is the
        anchor, whose parent root is not looked at.  ``ValueError`` -- and no block of the call is
        added -- for an unknown parent, a slot not above the parent's, or more blocks than the capacity."""
        roots, parents = [_root(r) for r in roots], [_root(r, "parent root") for r in parent_roots]
        slots = _arr(slots, np.uint64, "slots")
        if not len(roots) == len(parents) == len(slots):
            raise ValueError("add_blocks: a root, a parent root and a slot per block")
        _bounds(slots, self._attestations)
        ids = np.zeros(len(roots), dtype=np.uint32)
        if len(roots):
            _native.check(_native.lib().bls381_fork_choice_add_blocks(self._handle(), len(roots), b"".join(roots),
                                                                      b"".join(parents), _p(slots), _p(ids)))
        return ids

    def add_block(self, root, parent_root, slot: int) -> int:
        return int(self.add_blocks([root], [parent_root], [int(slot)])[0])

    def node(self, root) -> int:
        """The node id of a root; ``KeyError`` for an unknown one."""
        node = int(_native.lib().bls381_fork_choice_node(self._handle(), _root(root)))
        if node == NONE:
            raise KeyError(bytes(root).hex())
        return node

    def root(self, node: int) -> bytes:
        out = ctypes.create_string_buffer(32)
        _native.check(_native.lib().bls381_fork_choice_root(self._handle(), int(node), out))
        return out.raw

    # ---- latest messages ---------------------------------------------------------------------------
    def _targets(self, targets) -> np.ndarray:
        """Target blocks as node ids: roots (32 bytes each) are looked up."""
        if len(targets) and isinstance(targets[0], (bytes, bytearray, memoryview)):
            return np.array([self.node(t) for t in targets], dtype=np.uint32)
        return _arr(targets, np.uint32, "targets")

    def on_attestations(self, att_off, entries, slots, targets, ok=None) -> int:
        """Attestation a's members are ``entries[att_off[a]:att_off[a + 1]]`` (validator indices); it
        votes at ``slots[a]`` for ``targets[a]`` (node ids or roots).  ``ok``: one verdict per
        attestation; a failed one leaves no message.  Returns how many members were skipped for being
        at or above the validator capacity."""
        att_off, entries = _arr(att_off, np.uint32, "att_off"), _arr(entries, np.uint32, "entries")
        slots, targets = _arr(slots, np.uint64, "slots"), self._targets(targets)
        n_att = len(slots)
        if len(att_off) != n_att + 1 or len(targets) != n_att or (n_att and int(att_off[-1]) > len(entries)):
            raise ValueError("on_attestations: n_att + 1 offsets into entries, a slot and a target per attestation")
        _bounds(slots, self._attestations + n_att)
        if ok is not None:
            ok = np.ascontiguousarray(ok, dtype=np.uint8)
            if len(ok) != n_att:
                raise ValueError("on_attestations: one verdict per attestation")
        skipped = np.zeros(1, dtype=np.uint64)
        _native.check(_native.lib().bls381_fork_choice_on_attestations(
            self._handle(), n_att, _p(att_off), _p(entries) if len(entries) else None, _p(slots), _p(targets),
            None if ok is None else _p(ok), _p(skipped)))
        self._attestations += n_att
        return int(skipped[0])

    def on_attestations_device(self, att_off, d_entries: int, slots, targets, d_ok: int = 0):
        """The same over device memory: ``d_entries`` the ``d_entries`` of
        ``bls381_attesting_entries_device`` (``att_off[a] = group_key_off[2 a]``), ``d_ok`` the
        grouped verify's verdicts (0: none).  Queued on the current stream, not synchronised.
        Returns the tensors the call uses (the skipped count, one int64, first): keep them until the
        stream has passed the call."""
        import torch
        att_off, slots, targets = _arr(att_off, np.uint32, "att_off"), _arr(slots, np.uint64, "slots"), self._targets(targets)
        n_att = len(slots)
        if len(att_off) != n_att + 1 or len(targets) != n_att:
            raise ValueError("on_attestations_device: n_att + 1 offsets, a slot and a target per attestation")
        _bounds(slots, self._attestations + n_att)
        L = _native.lib()
        skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(max(1, L.bls381_fork_choice_on_attestations_workspace_size(n_att)), dtype=torch.uint8, device="cuda")
        _native.check(L.bls381_fork_choice_on_attestations_device(
            self._handle(), n_att, _p(att_off), int(d_entries) or None, _p(slots), _p(targets), int(d_ok) or None,
            skipped.data_ptr(), ws.data_ptr(), _stream()))
        self._attestations += n_att
        return skipped, ws

    def latest(self, first: int, n: int):
        """``(slots, targets)`` of validators ``first .. first + n - 1``: the slot of the latest
        message (0 without one) and its target node (0xFFFFFFFF: none)."""
        slots, targets = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
        _native.check(_native.lib().bls381_fork_choice_read_latest(self._handle(), int(first), int(n), _p(slots) if n else None,
                                                                   _p(targets) if n else None))
        return slots, targets

    def prune(self, root) -> None:
        """On finalization: the subtree of ``root`` stays (renumbered, ``root`` becomes node 0)."""
        _native.check(_native.lib().bls381_fork_choice_prune(self._handle(), self.node(root)))
        self._counts = None

    # ---- the head ----------------------------------------------------------------------------------
    def head(self, start_root, registry, epoch: int) -> bytes:
        """The head's root from ``start_root`` with the votes weighed by ``registry`` at ``epoch``:
        a ``state_tree.validator_registry_tree`` (read where the tree keeps its records; only the head,
        the counts and the status word come back), or ``(activation_epochs, exit_epochs,
        effective_balances)``.  ``OverflowError`` when a vote count passed 2^64 - 1."""
        start = self.node(start_root)
        B = len(self)
        if hasattr(registry, "items_ptr"):
            import torch
            if registry.item_size != RECORD:
                raise ValueError("a validator registry tree")
            n, rec = registry.count, registry.items_ptr
            out = torch.zeros(2 + B, dtype=torch.int64, device="cuda")   # head, status, counts
            _native.check(_native.lib().bls381_fork_choice_head_device(
                self._handle(), start, n, rec + OFF_ACTIVATION, rec + OFF_EXIT, rec + OFF_EFFECTIVE, RECORD, int(epoch),
                out.data_ptr(), out.data_ptr() + 16, out.data_ptr() + 8, _stream()))
            host = out.cpu().numpy().view(np.uint64)   # synchronises
            head, status, counts = int(host[0]) & 0xFFFFFFFF, int(host[1]), host[2:].copy()
        else:
            act, ext, eff = (_arr(x, np.uint64, "registry") for x in registry)
            if not len(act) == len(ext) == len(eff):
                raise ValueError("head: one entry per validator in every array")
            h, status_w, counts = np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(B, np.uint64)
            _native.check(_native.lib().bls381_fork_choice_head(
                self._handle(), start, len(eff), _p(act), _p(ext), _p(eff), 8, int(epoch), _p(h), None, _p(counts), _p(status_w)))
            head, status = int(h[0]), int(status_w[0])
        self._counts = counts
        if status:
            raise OverflowError("fork choice: %d vote counts passed 2^64 - 1" % status)
        return self.root(head)

    def vote_counts(self) -> np.ndarray:
        """The vote count of every node, by node id, as the last ``head`` saw them."""
        if self._counts is None:
            raise ValueError("vote_counts: no head since the tree was made or pruned")
        return self._counts


def lmd_ghost(roots, parent_roots, block_slots, att_off, entries, att_slots, att_targets, start_root, activation_epochs,
              exit_epochs, effective_balances, epoch: int):
    """One-shot: ``(head root, vote counts by block, in the order given)``.  Blocks come parents first;
    ``att_targets`` are roots or indices into ``roots``."""
    n = len(effective_balances)
    with ForkChoice(max(1, n), max(1, len(roots))) as fc:
        ids = fc.add_blocks(roots, parent_roots, block_slots)
        if len(set(ids.tolist())) != len(ids):
            raise ValueError("lmd_ghost: a root given twice")
        fc.on_attestations(att_off, entries, att_slots, att_targets)
        head = fc.head(start_root, (activation_epochs, exit_epochs, effective_balances), epoch)
        return head, fc.vote_counts()
