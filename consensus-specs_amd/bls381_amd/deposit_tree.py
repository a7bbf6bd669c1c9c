"""The deposit tree kept on the device (include/bls381.h ``bls381_deposit_tree_*``).

Deposits arrive over time and ``Eth1Data.deposit_root`` is the deposit contract's root at some
count k; a block's deposits carry proofs against ``state.latest_eth1_data.deposit_root``
(specs/core/0_beacon-chain.md:1630, :1742), the root at the voted count.  ``DepositTree`` holds
the leaves and their inner nodes in device memory, appends to them, and answers for every count
up to the current one: ``root(k)`` is the reference's ``get_merkle_root(leaves[:k])`` and
``proofs(indices, k)`` its ``get_merkle_proof`` of that tree.  Later appends do not disturb a
query for an earlier count.  (``ssz.build_deposits`` is the tree of one batch alone, the
reference's test helper.)
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from .ssz import _leaf_blob

DEPOSIT_DATA_BYTES = 184
DEPOSIT_BYTES = 1208     # BLS381_DEPOSIT_BYTES


def _data_blob(datas) -> bytes:
    blob = bytes(datas) if isinstance(datas, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in datas)
    if len(blob) % DEPOSIT_DATA_BYTES:
        raise ValueError("DepositData serializations are %d bytes" % DEPOSIT_DATA_BYTES)
    return blob


class DepositTree:
    """A tree of ``2**depth`` leaves with room for ``capacity`` of them (fixed; at most
    ``2**depth - 1``, the contract's MAX_DEPOSIT_COUNT), on the current device."""

    def __init__(self, capacity: int, depth: int = 32):
        h = ctypes.c_void_p()
        _native.check(_native.lib().bls381_deposit_tree_create(int(capacity), int(depth), ctypes.byref(h)))
        self._h = h
        self.capacity = int(capacity)
        self.depth = int(depth)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().bls381_deposit_tree_destroy(self._h)
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
            raise ValueError("the deposit tree is closed")
        return self._h

    @property
    def count(self) -> int:
        return int(_native.lib().bls381_deposit_tree_count(self._handle()))

    def __len__(self) -> int:
        return self.count

    def append(self, leaves) -> None:
        """Leaves ``count .. count+n-1`` become the given 32-byte values (a sequence of them, or
        their concatenation).  ValueError when they do not fit; the tree is then unchanged."""
        blob = _leaf_blob(leaves)
        _native.check(_native.lib().bls381_deposit_tree_append(self._handle(), len(blob) // 32, blob or None))

    def append_deposit_data(self, datas) -> None:
        """Appends ``hash_tree_root(data)`` of serialized DepositData (184 bytes each)."""
        blob = _data_blob(datas)
        _native.check(_native.lib().bls381_deposit_tree_append_data(self._handle(), len(blob) // DEPOSIT_DATA_BYTES,
                                                                    blob or None))

    def roots(self, counts) -> list:
        """The root at each of ``counts`` (0 .. count): ``get_deposit_root()`` after that many deposits."""
        ks = np.ascontiguousarray([int(k) for k in counts], dtype=np.uint64)
        out = ctypes.create_string_buffer(max(32 * len(ks), 1))
        _native.check(_native.lib().bls381_deposit_tree_roots(self._handle(), len(ks),
                                                              ks.ctypes.data_as(ctypes.c_void_p) if len(ks) else None,
                                                              out))
        raw = out.raw
        return [raw[32 * q:32 * q + 32] for q in range(len(ks))]

    def root(self, count=None) -> bytes:
        return self.roots([self.count if count is None else count])[0]

    def proofs(self, indices, count=None):
        """(proofs, root) at ``count`` (default: the current one): proofs[t] is the concatenation of
        the ``depth`` siblings of indices[t], the form ``ssz.verify_merkle_branch_batch`` takes; an
        index at or above ``count`` gets the proof of a zero leaf."""
        k = self.count if count is None else int(count)
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        row = 32 * self.depth
        out = ctypes.create_string_buffer(max(row * len(idx), 1))
        root = ctypes.create_string_buffer(32)
        _native.check(_native.lib().bls381_deposit_tree_proofs(self._handle(), k, len(idx),
                                                               idx.ctypes.data_as(ctypes.c_void_p) if len(idx) else None,
                                                               out, row, root))
        raw = out.raw
        return [raw[row * t:row * t + row] for t in range(len(idx))], root.raw

    def deposits(self, datas, first_index: int, count=None) -> list:
        """Serialized Deposits (1,208 bytes: the proof, then the data) for leaves ``first_index ..
        first_index + len(datas) - 1`` with proofs under ``root(count)``: what
        ``PubkeyRegistry.process_deposits(deposits, first_index, tree.root(count), ...)`` consumes.
        ``datas`` must be the DepositData that were appended at those leaves; they are copied, not
        re-hashed against the tree.  Needs depth 32."""
        k = self.count if count is None else int(count)
        blob = _data_blob(datas)
        n = len(blob) // DEPOSIT_DATA_BYTES
        out = ctypes.create_string_buffer(max(DEPOSIT_BYTES * n, 1))
        _native.check(_native.lib().bls381_deposit_tree_deposits(self._handle(), k, int(first_index), n, blob or None,
                                                                 out))
        raw = out.raw
        return [raw[DEPOSIT_BYTES * i:DEPOSIT_BYTES * (i + 1)] for i in range(n)]
