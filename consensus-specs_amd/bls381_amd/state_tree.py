"""SSZ list trees kept on the device (include/bls381.h ``bls381_list_tree_*``).

The state transition asks for ``hash_tree_root(state)`` at every slot
(specs/core/0_beacon-chain.md:1216, :1235) while only a few registry records and balances change
between two slots.  ``ListTree`` holds a list's items and the Merkle tree over their chunks in
device memory, takes in-place updates as well as appends, re-hashes only the tiles on the paths
of what changed, and answers ``hash_tree_root`` of the list and proofs of its chunks.  The item
store is what the epoch context reads (``bls381_amd.epoch``): one buffer of records serves the
registry root and the active indices.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native, ssz

_PACKED_SIZES = (1, 2, 4, 8, 16, 32)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if len(a) else None


class ListTree:
    """``capacity`` items of ``typ`` on the current device.  ``typ`` is an ``ssz`` container
    (composite: a chunk per item, its ``hash_tree_root``) or ``ssz.uint(n)`` / ``ssz.Bytes(32)``
    (packed: the items' bytes are the chunks)."""

    def __init__(self, capacity: int, typ):
        kind = typ[0]
        self.typ = typ
        if kind == "container":
            if not ssz.is_fixed_size(typ):
                raise ValueError("a list tree holds fixed-size items")
            self.packed = False
            prog = np.ascontiguousarray(ssz.compile_root(typ), dtype=np.uint32)
        elif kind in ("uint", "bytes") and ssz.item_size(typ) in _PACKED_SIZES and (kind == "uint" or typ[1] == 32):
            self.packed = True
            prog = np.zeros(0, dtype=np.uint32)
        else:
            raise ValueError("a list tree holds containers, ssz.uint(n) or ssz.Bytes(32)")
        self.item_size = ssz.item_size(typ)
        self.capacity = int(capacity)
        h = ctypes.c_void_p()
        _native.check(_native.lib().bls381_list_tree_create(self.capacity, self.item_size, _ptr(prog), len(prog),
                                                            ctypes.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _native.lib().bls381_list_tree_destroy(self._h)
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
            raise ValueError("the list tree is closed")
        return self._h

    @property
    def count(self) -> int:
        return int(_native.lib().bls381_list_tree_count(self._handle()))

    def __len__(self) -> int:
        return self.count

    @property
    def depth(self) -> int:
        """ceil(log2(chunks)) at the current count: the length of a proof."""
        return int(_native.lib().bls381_list_tree_depth(self._handle()))

    @property
    def items_ptr(self) -> int:
        """The device address of item 0 (item i at ``+ i * item_size``); read-only, valid until close."""
        return int(_native.lib().bls381_list_tree_items_device(self._handle()) or 0)

    def _blob(self, items) -> bytes:
        blob = bytes(items) if isinstance(items, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in items)
        if len(blob) % self.item_size:
            raise ValueError("items are %d bytes" % self.item_size)
        return blob

    def append(self, items) -> None:
        """Items ``count .. count+n-1`` (serialized; a sequence of them or their concatenation).
        ValueError when they do not fit; the tree is then unchanged."""
        blob = self._blob(items)
        _native.check(_native.lib().bls381_list_tree_append(self._handle(), len(blob) // self.item_size, blob or None))

    def update_bytes(self, indices, off: int, length: int, values) -> None:
        """Bytes ``[off, off+length)`` of item ``indices[t]`` become ``values[t]``.  Repeated indices
        are applied in order.  ValueError for an index at or above the count; nothing changes then."""
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint32)
        blob = bytes(values) if isinstance(values, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in values)
        if len(blob) != len(idx) * length:
            raise ValueError("values are %d bytes each" % length)
        _native.check(_native.lib().bls381_list_tree_update(self._handle(), len(idx), _ptr(idx), int(off), int(length),
                                                            blob or None))

    def update(self, indices, items) -> None:
        """Replaces whole items."""
        self.update_bytes(indices, 0, self.item_size, self._blob(items))

    def field_layout(self, field: str):
        """(offset, length, type) of a field in the container's fixed layout."""
        if self.typ[0] != "container" or not ssz.is_fixed_size(self.typ):
            raise ValueError("field updates need a fixed-size container")
        off = 0
        for name, t in self.typ[1]:
            if name == field:
                return off, ssz.item_size(t), t
            off += ssz.item_size(t)
        raise KeyError(field)

    def update_field(self, indices, field: str, values) -> None:
        """Sets ``field`` of items ``indices[t]`` to ``values[t]`` (Python values of the field's type)."""
        off, length, t = self.field_layout(field)
        self.update_bytes(indices, off, length, b"".join(ssz.serialize(t, v) for v in values))

    def root(self, mix_length: bool = True) -> bytes:
        """``hash_tree_root`` of the list (``mix_length=False``: of the vector, no length mixed in)."""
        out = ctypes.create_string_buffer(32)
        _native.check(_native.lib().bls381_list_tree_root(self._handle(), int(bool(mix_length)), out))
        return out.raw

    def proofs(self, chunk_indices):
        """(proofs, root): proofs[t] is the concatenation of the ``depth`` siblings of chunk
        ``chunk_indices[t]``, the form ``ssz.verify_merkle_branch_batch`` takes, under the unmixed
        root; a chunk at or above the count's chunks gets the proof of a zero chunk."""
        idx = np.ascontiguousarray([int(i) for i in chunk_indices], dtype=np.uint64)
        row = 32 * self.depth
        out = ctypes.create_string_buffer(max(row * len(idx), 1))
        root = ctypes.create_string_buffer(32)
        _native.check(_native.lib().bls381_list_tree_proofs(self._handle(), len(idx), _ptr(idx), out, row, root))
        raw = out.raw
        return [raw[row * t:row * t + row] for t in range(len(idx))], root.raw

    def read(self, first: int, n: int) -> list:
        """Items ``first .. first+n-1`` as they stand, serialized."""
        n = int(n)
        out = ctypes.create_string_buffer(max(self.item_size * n, 1))
        _native.check(_native.lib().bls381_list_tree_read(self._handle(), int(first), n, out))
        raw = out.raw
        return [raw[self.item_size * i:self.item_size * (i + 1)] for i in range(n)]


def validator_registry_tree(capacity: int) -> ListTree:
    """``state.validator_registry``: 121-byte Validator records."""
    return ListTree(capacity, ssz.Validator)


def balances_tree(capacity: int) -> ListTree:
    """``state.balances``: List[uint64], four to a chunk."""
    return ListTree(capacity, ssz.uint(8))
