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


class RaggedListTree:
    """A list of variable-size containers kept on the device: ``state.previous_epoch_attestations``
    and ``state.current_epoch_attestations`` (List[PendingAttestation]).  It is a
    ``ListTree(capacity, ssz.Bytes(32))`` over the elements' roots: a list of composites and the
    list of their 32-byte roots have the same tree and the same length mix-in, so ``root()`` is the
    list's ``hash_tree_root``.  ``append`` roots the serialized items on the device
    (``bls381_ssz_ragged_roots_device``) and hands the roots, still in device memory, to
    ``bls381_list_tree_append_device``.  Scratch buffers are torch tensors on the current device."""

    def __init__(self, capacity: int, typ):
        prog = ssz.compile_root(typ)
        if ssz.is_fixed_size(typ) or not ssz.ragged_prog_ok(prog):
            raise ValueError("a ragged list tree holds variable-size containers with a ragged root program")
        self.typ = typ
        self.capacity = int(capacity)
        self._prog = np.ascontiguousarray(prog, dtype=np.uint32)
        self._tree = ListTree(self.capacity, ssz.Bytes(32))

    def close(self) -> None:
        self._tree.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def count(self) -> int:
        return self._tree.count

    def __len__(self) -> int:
        return self.count

    def append(self, serialized_items) -> None:
        """Appends the items' roots.  ValueError when an item breaks the offset rules (DESIGN.md
        §7b.3) or the items do not fit; the tree is then unchanged."""
        import torch
        items = [bytes(x) for x in serialized_items]
        n = len(items)
        if n > self.capacity - self.count:
            raise ValueError("the items do not fit the tree")
        if n == 0:
            return
        L = _native.lib()
        handle = self._tree._handle()
        blob = b"".join(items)
        starts = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in items], out=starts[1:])
        d_items = torch.frombuffer(bytearray(blob or b"\x00"), dtype=torch.uint8).cuda()
        d_starts = torch.from_numpy(starts).cuda()
        d_roots = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        d_status = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(1, L.bls381_ssz_ragged_roots_workspace_size(n)), dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _native.check(L.bls381_ssz_ragged_roots_device(
            n, d_items.data_ptr(), len(blob), d_starts.data_ptr(), _ptr(self._prog), len(self._prog),
            d_roots.data_ptr(), d_status.data_ptr(), d_bad.data_ptr(), ws.data_ptr(), stream))
        # the bad count is read before the append is queued: a malformed item leaves the tree as it was
        if int(d_bad.item()):
            raise ValueError("%d malformed item(s); first at %d" % (int(d_bad.item()), int(d_status.argmax().item())))
        ws2 = torch.empty(max(1, L.bls381_list_tree_append_workspace_size(handle, n)), dtype=torch.uint8, device="cuda")
        _native.check(L.bls381_list_tree_append_device(handle, n, d_roots.data_ptr(), ws2.data_ptr(), stream))
        torch.cuda.current_stream().synchronize()   # the scratch tensors go back to torch's allocator below

    def clear(self) -> None:
        """The empty list (the list-tree ABI has no reset: the tree is made anew)."""
        self._tree.close()
        self._tree = ListTree(self.capacity, ssz.Bytes(32))

    def replace(self, serialized_items) -> None:
        """The whole list becomes ``serialized_items`` (the epoch rotation's ``previous = current``
        from the serialized attestations).  ValueError as for ``append``; the tree is then unchanged."""
        new = RaggedListTree(self.capacity, self.typ)
        try:
            new.append(serialized_items)
        except Exception:
            new.close()
            raise
        self._tree.close()
        self._tree = new._tree

    def root(self) -> bytes:
        """``hash_tree_root`` of the list."""
        return self._tree.root(True)


def validator_registry_tree(capacity: int) -> ListTree:
    """``state.validator_registry``: 121-byte Validator records."""
    return ListTree(capacity, ssz.Validator)


def balances_tree(capacity: int) -> ListTree:
    """``state.balances``: List[uint64], four to a chunk."""
    return ListTree(capacity, ssz.uint(8))
