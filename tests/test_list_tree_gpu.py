"""The SSZ list tree kept on the device: bls381_list_tree_*, host-pointer forms
(through bls381_amd.state_tree.ListTree) and device forms on torch buffers, against
merkle_model.py, ssz_oracle.py and tests/golden/list_tree_history.json (the reference's
merkle_minimal.py), then against the engine's own from-scratch roots and the epoch context over
the tree's item store.  The cases are list_tree_cases.py's, shared with the CPU half
(test_list_tree_host.py).  Every device output is pre-filled with 0xEE with 64 bytes of slack
that must stay 0xEE."""
import ctypes
import random

import numpy as np
import pytest

import epoch_model as E
import list_tree_cases as C
import merkle_model as M

pytestmark = pytest.mark.gpu

W = 256                    # MERKLE_TILE (csrc/bls381_plan.hpp); test_list_tree_host.py reads it from the host build
SLACK = 64                 # bytes behind every device output that must stay 0xEE


class Dev:
    """torch buffers for the _device forms on the current stream."""

    def __init__(self, native):
        import torch
        self.torch, self.native, self.L, self.EARG = torch, native, native.lib(), native.EARG
        self.dev = torch.device("cuda:0")
        self.hip = ctypes.CDLL("libamdhip64.so")       # the runtime torch and the engine already share
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipMemcpy.restype = ctypes.c_int

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def sync(self):
        self.torch.cuda.synchronize()

    def up(self, data: bytes):
        if not data:
            return None
        return self.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.dev)

    def filled(self, nbytes):
        return self.torch.full((int(nbytes) + SLACK,), 0xEE, dtype=self.torch.uint8, device=self.dev)

    @staticmethod
    def ptr(t, off=0):
        return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None

    def down(self, t, nbytes):
        self.torch.cuda.current_stream().synchronize()
        raw = t.cpu().numpy().tobytes()
        assert raw[nbytes:] == b"\xEE" * SLACK, "bytes behind the output were written"
        return raw[:nbytes]

    def peek(self, address, nbytes):
        """nbytes of device memory at a raw address (the tree's item store)."""
        self.sync()
        out = ctypes.create_string_buffer(max(nbytes, 1))
        if nbytes:
            assert self.hip.hipMemcpy(out, ctypes.c_void_p(address), nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out.raw[:nbytes]

    def verify(self, leaves, proofs, depth, indices, root):
        from bls381_amd import ssz
        return list(ssz.verify_merkle_branch_batch(list(leaves), list(proofs), depth, list(indices), root))


def prog_of(typ):
    from bls381_amd import ssz
    return np.ascontiguousarray(ssz.compile_root(typ), dtype=np.uint32)


def raw_create(dev, capacity, item_size, prog):
    h = ctypes.c_void_p()
    rc = dev.L.bls381_list_tree_create(capacity, item_size, prog.ctypes.data_as(ctypes.c_void_p) if prog is not None else None,
                                       len(prog) if prog is not None else 0, ctypes.byref(h))
    if rc == dev.EARG:
        assert not h
        raise ValueError("rejected")
    assert rc == 0 and h
    return h


class RawHandle:
    def __init__(self, dev, h):
        self.dev, self.h = dev, h

    def close(self):
        if self.h:
            self.dev.L.bls381_list_tree_destroy(self.h)
            self.h = None


class HostPointerTree:
    """state_tree.ListTree behind the tree interface of list_tree_cases.py."""

    def __init__(self, dev, tree):
        self.d, self.t = dev, tree
        self.capacity, self.item_size = tree.capacity, tree.item_size

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.t.close()
        return False

    def close(self):
        self.t.close()

    count = property(lambda self: self.t.count)
    depth = property(lambda self: self.t.depth)

    def append(self, items):
        self.t.append(list(items))

    def update(self, indices, off, length, values):
        self.t.update_bytes(indices, off, length, list(values))

    def root(self, mix):
        return self.t.root(mix)

    def proofs(self, indices):
        return self.t.proofs(indices)

    def read(self, first, n):
        return self.t.read(first, n)

    def tail(self):
        c = self.count
        return self.d.peek(self.t.items_ptr + c * self.item_size, (self.capacity - c) * self.item_size)


class HostPointerEngine:
    device_form = False

    def __init__(self, dev, mod):
        self.dev, self.mod, self.verify = dev, mod, dev.verify

    def create(self, capacity, typ):
        return HostPointerTree(self.dev, self.mod.ListTree(capacity, typ))

    def create_raw(self, capacity, item_size, prog):
        return RawHandle(self.dev, raw_create(self.dev, capacity, item_size, prog))


class DeviceTree:
    """The _device forms: queued on the current stream with buffers of their own, read back after
    a synchronise."""

    def __init__(self, dev, capacity, item_size, prog):
        self.d, self.L, self.capacity, self.item_size = dev, dev.L, capacity, item_size
        self.h = raw_create(dev, capacity, item_size, prog)
        assert self.L.bls381_list_tree_capacity(self.h) == capacity
        self.keep = []

    def close(self):
        if self.h:
            self.L.bls381_list_tree_destroy(self.h)
            self.h = None
            self.keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    count = property(lambda self: self.L.bls381_list_tree_count(self.h))
    depth = property(lambda self: self.L.bls381_list_tree_depth(self.h))
    items_ptr = property(lambda self: self.L.bls381_list_tree_items_device(self.h))

    def ok(self, rc):
        if rc == self.d.EARG:
            raise ValueError("rejected")
        assert rc == 0

    def append(self, items):
        d_items = self.d.up(b"".join(items))
        ws = self.d.filled(self.L.bls381_list_tree_append_workspace_size(self.h, len(items)))
        self.keep += [d_items, ws]
        self.ok(self.L.bls381_list_tree_append_device(self.h, len(items), self.d.ptr(d_items), self.d.ptr(ws), self.d.stream()))

    def update(self, indices, off, length, values):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint32)
        d_idx, d_vals = self.d.up(idx.tobytes()), self.d.up(b"".join(values))
        ws = self.d.filled(self.L.bls381_list_tree_update_workspace_size(self.h, len(idx)))
        self.keep += [d_idx, d_vals, ws]
        self.ok(self.L.bls381_list_tree_update_device(self.h, len(idx), self.d.ptr(d_idx), off, length, self.d.ptr(d_vals),
                                                      self.d.ptr(ws), self.d.stream()))

    def queue_root(self, mix):
        out = self.d.filled(32)
        self.ok(self.L.bls381_list_tree_root_device(self.h, int(mix), self.d.ptr(out), self.d.stream()))
        return lambda: self.d.down(out, 32)

    def root(self, mix):
        return self.queue_root(mix)()

    def proofs(self, indices, stride=None):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * self.depth
        stride = row if stride is None else stride
        d_idx = self.d.up(idx.tobytes())
        out, root = self.d.filled(stride * len(idx)), self.d.filled(32)
        self.ok(self.L.bls381_list_tree_proofs_device(self.h, len(idx), self.d.ptr(d_idx), self.d.ptr(out), stride,
                                                      self.d.ptr(root), self.d.stream()))
        rows = self.d.down(out, stride * len(idx))
        self.last_rows = rows
        return [rows[stride * t:stride * t + row] for t in range(len(idx))], self.d.down(root, 32)

    def read(self, first, n):
        self.d.sync()                                   # the host-pointer read runs on the engine's own stream
        out = ctypes.create_string_buffer(max(self.item_size * n, 1))
        self.ok(self.L.bls381_list_tree_read(self.h, first, n, out))
        raw = out.raw
        return [raw[self.item_size * i:self.item_size * (i + 1)] for i in range(n)]

    def tail(self):
        c = self.count
        return self.d.peek(self.items_ptr + c * self.item_size, (self.capacity - c) * self.item_size)


class DeviceEngine:
    device_form = True

    def __init__(self, dev):
        self.dev, self.verify = dev, dev.verify

    def create(self, capacity, typ):
        return DeviceTree(self.dev, capacity, C.item_size(typ), prog_of(typ) if typ[0] == "container" else None)

    def create_raw(self, capacity, item_size, prog):
        return DeviceTree(self.dev, capacity, item_size, prog)


@pytest.fixture(scope="module")
def dev(native):
    return Dev(native)


@pytest.fixture(scope="module")
def mod(native):
    from bls381_amd import state_tree
    return state_tree


@pytest.fixture(scope="module", params=["host_pointer", "device"])
def eng(request, mod, dev):
    return HostPointerEngine(dev, mod) if request.param == "host_pointer" else DeviceEngine(dev)


# ------------------------------------------------------------ the shared cases
@pytest.mark.parametrize("name", ["validator", "uint64", "bytes32"])
def test_fixture(eng, name):
    C.check_fixture(eng, name)


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.BYTES32, 1), (C.UINT64, 4)], ids=["pair16", "bytes32", "uint64"])
def test_growth_through_depth_changes(eng, typ, per):
    C.check_growth(eng, W, typ, per)


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.BYTES32, 1), (C.UINT64, 4)], ids=["pair16", "bytes32", "uint64"])
def test_updates_inside_and_across_tiles(eng, typ, per):
    C.check_updates(eng, W, typ, per)


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.UINT64, 4)], ids=["pair16", "uint64"])
def test_three_passes(eng, typ, per):
    C.check_three_passes(eng, W, typ, per)


def test_packed_partial_chunks(eng):
    C.check_packed_partial(eng)


def test_field_updates_on_validator_records(eng):
    C.check_validator_fields(eng)


def test_update_field_finds_the_offsets(mod):
    from bls381_amd import ssz
    rng = random.Random("update_field")
    items = C.rand_items(rng, C.VALIDATOR, 20)
    with mod.validator_registry_tree(32) as tree, mod.balances_tree(32) as bal:
        assert [tree.field_layout(f)[:2] for f in ("effective_balance", "slashed", "exit_epoch")] == [(113, 8), (112, 1), (96, 8)]
        tree.append(items)
        tree.update_field([3, 19], "effective_balance", [31 * 10 ** 9, 17])
        tree.update_field([0], "slashed", [True])
        tree.update_field([19, 7], "exit_epoch", [5, 2 ** 64 - 1])
        C.apply_update(items, [3, 19], 113, 8, [(31 * 10 ** 9).to_bytes(8, "little"), (17).to_bytes(8, "little")])
        C.apply_update(items, [0], 112, 1, [b"\x01"])
        C.apply_update(items, [19, 7], 96, 8, [(5).to_bytes(8, "little"), b"\xff" * 8])
        assert tree.read(0, 20) == items and tree.root() == C.Model(C.VALIDATOR, items).root(True)
        assert len(tree) == 20 and tree.item_size == 121 and bal.item_size == 8 and bal.packed and not tree.packed
        with pytest.raises(KeyError):
            tree.update_field([0], "balance", [1])
        with pytest.raises(ValueError):
            bal.update_field([0], "effective_balance", [1])
        bal.append([(7).to_bytes(8, "little")] * 5)
        bal.update([4], [(9).to_bytes(8, "little")])
        assert bal.root() == C.Model(C.UINT64, [(7).to_bytes(8, "little")] * 4 + [(9).to_bytes(8, "little")]).root(True)
    with pytest.raises(ValueError):
        mod.ListTree(4, ssz.Container(("a", ssz.uint(8)), ("b", ssz.BYTES)))       # a variable-size container
    with pytest.raises(ValueError):
        mod.ListTree(4, ssz.Bytes(48))
    with pytest.raises(ValueError):
        tree.root()                                                                # closed


def test_repeated_indices(eng):
    C.check_repeated(eng, W)


# ----------------------------------------------------------- 7. device forms only
def test_queued_calls_keep_their_own_results(dev):
    """Append, update, root, update, append and root queued back to back on one stream with
    buffers of their own, read only at the end: each root is the model's at its point."""
    rng = random.Random("interleave")
    typ = C.VALIDATOR
    items = C.rand_items(rng, typ, W + 40)
    with DeviceEngine(dev).create(2 * W, typ) as tree:
        tree.append(items[:W - 3])
        now = items[:W - 3]
        vals = [rng.randbytes(8) for _ in range(3)]
        tree.update([0, W - 4, 9], 113, 8, vals)
        C.apply_update(now, [0, W - 4, 9], 113, 8, vals)
        r1, want1 = tree.queue_root(True), C.Model(typ, now).root(True)
        tree.update([W - 4], 112, 1, [b"\x01"])
        C.apply_update(now, [W - 4], 112, 1, [b"\x01"])
        tree.append(items[W - 3:])
        now = now + items[W - 3:]
        r2, r3 = tree.queue_root(True), tree.queue_root(False)
        m = C.Model(typ, now)
        assert (r1(), r2(), r3()) == (want1, m.root(True), m.root(False))
        assert tree.read(0, len(now)) == now


# ------------------------------------------- 9. against the existing code
def test_tree_roots_equal_the_from_scratch_roots(dev, mod):
    """After the field updates of case 6, bls381_ssz_list_root_device over items_ptr and the count
    equals the tree's mixed root; bls381_merkle_root_device over a uint64 tree's item store equals
    that tree's root."""
    L = dev.L
    with mod.validator_registry_tree(2 * C.VALIDATOR_COUNT) as vt:
        items = C.check_validator_fields(HostPointerEngine(dev, mod), HostPointerTree(dev, vt))
        n, prog = len(items), prog_of(C.VALIDATOR)
        ws, out = dev.filled(L.bls381_ssz_list_root_workspace_size(n)), dev.filled(32)
        assert L.bls381_ssz_list_root_device(n, ctypes.c_void_p(vt.items_ptr), 121, 121, prog.ctypes.data_as(ctypes.c_void_p),
                                             len(prog), 1, dev.ptr(out), dev.ptr(ws), dev.stream()) == 0
        assert dev.down(out, 32) == vt.root(True) == C.Model(C.VALIDATOR, items).root(True)
    rng = random.Random("balances")
    bals = C.rand_items(rng, C.UINT64, 4 * W + 3)
    with mod.balances_tree(8 * W) as bt:
        bt.append(bals)
        idx = [0, 5, 4 * W - 1, 4 * W, 4 * W + 2]
        vals = C.rand_items(rng, C.UINT64, len(idx))
        bt.update(idx, vals)
        chunks, d = W + 1, bt.depth
        assert d == 9
        ws, out = dev.filled(L.bls381_merkle_root_workspace_size(chunks, 0, d)), dev.filled(32)
        assert L.bls381_merkle_root_device(chunks, ctypes.c_void_p(bt.items_ptr), 0, d, 1, len(bals), dev.ptr(out), dev.ptr(ws),
                                           dev.stream()) == 0
        assert dev.down(out, 32) == bt.root(True)


def test_epoch_context_reads_the_tree_s_records(dev, mod):
    """bls381_active_indices_device with bases items_ptr + 88 / 96 / 113 and stride 121 returns
    epoch_model's indices and balance sum, again after an update_field that exits two validators."""
    L = dev.L
    rng = random.Random("epoch")
    n, epoch = W + 37, 10
    act = [rng.choice((0, 3, 10, 11, E.FAR_FUTURE_EPOCH)) for _ in range(n)]
    ext = [rng.choice((5, 10, 11, 40, E.FAR_FUTURE_EPOCH)) for _ in range(n)]
    bal = [rng.randrange(1, 32 * 10 ** 9) for _ in range(n)]
    records = E.validator_records(act, ext, bal, rng)
    with mod.validator_registry_tree(2 * W) as vt:
        vt.append(records)
        for round_ in range(2):
            want = E.get_active_validator_indices(act, ext, epoch)
            d_idx, d_ct = dev.filled(4 * n), dev.filled(16)
            ws = dev.filled(L.bls381_active_indices_workspace_size(n))
            p = vt.items_ptr
            assert L.bls381_active_indices_device(n, ctypes.c_void_p(p + E.OFF_ACTIVATION), ctypes.c_void_p(p + E.OFF_EXIT), 121,
                                                  epoch, ctypes.c_void_p(p + E.OFF_BALANCE), 121, dev.ptr(d_idx), dev.ptr(d_ct),
                                                  dev.ptr(ws), dev.stream()) == 0
            count, total = (int(v) for v in np.frombuffer(dev.down(d_ct, 16), dtype=np.uint64))
            assert count == len(want) and total == sum(bal[i] for i in want)
            assert np.frombuffer(dev.down(d_idx, 4 * n)[:4 * count], dtype=np.uint32).tolist() == want
            if round_ == 0:
                exits = want[1], want[-1]
                vt.update_field(exits, "exit_epoch", [epoch, epoch - 1])
                for i, e in zip(exits, (epoch, epoch - 1)):
                    ext[i] = e
                assert len(E.get_active_validator_indices(act, ext, epoch)) == len(want) - 2


# ------------------------------------------------------ 10. rejected calls
def test_rejected_calls(eng):
    C.check_rejected(eng, prog_of(C.PAIR16))
    bad = np.asarray([1, 0, 33], dtype=np.uint32)                 # a chunk of 33 bytes
    with pytest.raises(ValueError):
        eng.create_raw(4, 64, bad)


def test_call_under_another_device_is_rejected(native, dev):
    """A tree belongs to the device current at creation.  Runs only where two devices are
    visible; on a box with one the rule is not tested."""
    L, EARG = native.lib(), native.EARG
    if L.bls381_device_count() < 2:
        return
    h, root = raw_create(dev, 8, 8, None), ctypes.create_string_buffer(32)
    try:
        assert L.bls381_list_tree_append(h, 1, bytes(8)) == 0
        assert L.bls381_init(1) == 0
        assert L.bls381_list_tree_root(h, 1, root) == EARG
        assert L.bls381_list_tree_append(h, 1, bytes(8)) == EARG and L.bls381_list_tree_count(h) == 1
        assert L.bls381_list_tree_read(h, 0, 1, root) == EARG
    finally:
        assert L.bls381_init(0) == 0
        L.bls381_list_tree_destroy(h)


def test_bad_arguments(native, dev):
    """NULLs, alignment and the workspace-size functions of both forms, with the count and the
    root unchanged afterwards."""
    L, EARG = native.lib(), native.EARG
    h = ctypes.c_void_p()
    prog = prog_of(C.PAIR16)
    pp = prog.ctypes.data_as(ctypes.c_void_p)
    assert L.bls381_list_tree_create(16, 8, None, 0, None) == EARG
    assert L.bls381_list_tree_create(16, 8, None, 3, ctypes.byref(h)) == EARG and not h      # a length without a program
    assert L.bls381_list_tree_create(16, 16, pp, 0, ctypes.byref(h)) == EARG
    assert L.bls381_list_tree_count(None) == 0 == L.bls381_list_tree_capacity(None)
    assert L.bls381_list_tree_depth(None) == 0 and not L.bls381_list_tree_items_device(None)
    L.bls381_list_tree_destroy(None)
    assert L.bls381_list_tree_append_workspace_size(None, 1) == 0 == L.bls381_list_tree_update_workspace_size(None, 1)
    rng = random.Random("bad arguments")
    items = C.rand_items(rng, C.PAIR16, 5)
    blob = b"".join(items)
    want = C.Model(C.PAIR16, items)
    root, out = ctypes.create_string_buffer(32), ctypes.create_string_buffer(4096)
    i64, i32 = np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint32)
    p64, p32 = i64.ctypes.data_as(ctypes.c_void_p), i32.ctypes.data_as(ctypes.c_void_p)
    assert L.bls381_list_tree_create(8, 16, pp, len(prog), ctypes.byref(h)) == 0
    try:
        assert L.bls381_list_tree_append_workspace_size(h, 9) == 0                 # does not fit
        assert L.bls381_list_tree_append_workspace_size(h, 0) == 0
        assert L.bls381_list_tree_append_workspace_size(h, 8) > 0
        assert L.bls381_list_tree_update_workspace_size(h, 0) == 0 == L.bls381_list_tree_update_workspace_size(h, 2 ** 31)
        assert L.bls381_list_tree_update_workspace_size(h, 1) > 0
        # host-pointer forms
        assert L.bls381_list_tree_append(None, 1, blob) == EARG
        assert L.bls381_list_tree_append(h, 1, None) == EARG
        assert L.bls381_list_tree_append(h, 0, None) == 0
        assert L.bls381_list_tree_append(h, 5, blob) == 0 and L.bls381_list_tree_count(h) == 5
        assert L.bls381_list_tree_append(h, 4, bytes(64)) == EARG
        assert L.bls381_list_tree_update(None, 1, p32, 0, 16, blob) == EARG
        assert L.bls381_list_tree_update(h, 1, None, 0, 16, blob) == EARG
        assert L.bls381_list_tree_update(h, 1, p32, 0, 16, None) == EARG
        assert L.bls381_list_tree_update(h, 1, p32, 1, 16, blob) == EARG
        assert L.bls381_list_tree_update(h, 2 ** 31, p32, 0, 16, blob) == EARG
        assert L.bls381_list_tree_update(h, 0, None, 0, 16, None) == 0 == L.bls381_list_tree_update(h, 1, None, 0, 0, None)
        assert L.bls381_list_tree_root(None, 1, root) == EARG == L.bls381_list_tree_root(h, 1, None)
        assert L.bls381_list_tree_read(None, 0, 1, out) == EARG == L.bls381_list_tree_read(h, 0, 1, None)
        assert L.bls381_list_tree_read(h, 5, 1, out) == EARG and L.bls381_list_tree_read(h, 5, 0, None) == 0
        d = want.depth
        assert d == 3 == L.bls381_list_tree_depth(h)
        assert L.bls381_list_tree_proofs(None, 1, p64, out, 96, root) == EARG
        assert L.bls381_list_tree_proofs(h, 1, None, out, 96, root) == EARG
        assert L.bls381_list_tree_proofs(h, 1, p64, None, 96, root) == EARG
        assert L.bls381_list_tree_proofs(h, 1, p64, out, 96, None) == EARG
        assert L.bls381_list_tree_proofs(h, 1, p64, out, 95, root) == EARG
        assert L.bls381_list_tree_proofs(h, 2 ** 31, p64, out, 96, root) == EARG
        assert L.bls381_list_tree_proofs(h, 0, None, None, 96, root) == 0 and root.raw == want.root(False)
        # device forms: NULLs, misaligned proofs, stride, root and indices
        s, p = dev.stream(), dev.ptr
        d_items, d_idx, d_out = dev.up(blob), dev.up(bytes(32)), dev.filled(4096)
        ws = dev.filled(max(L.bls381_list_tree_update_workspace_size(h, 2), L.bls381_list_tree_append_workspace_size(h, 1)))
        assert L.bls381_list_tree_append_device(None, 1, p(d_items), p(ws), s) == EARG
        assert L.bls381_list_tree_append_device(h, 1, None, p(ws), s) == EARG
        assert L.bls381_list_tree_append_device(h, 1, p(d_items), None, s) == EARG
        assert L.bls381_list_tree_append_device(h, 4, p(d_items), p(ws), s) == EARG
        assert L.bls381_list_tree_append_device(h, 0, None, None, s) == 0
        good = (2, p(d_idx), 0, 16, p(d_items), p(ws))
        for at, bad in ((0, 2 ** 31), (1, None), (1, p(d_idx, 2)), (2, 1), (3, 17), (4, None), (5, None)):
            a = list(good)
            a[at] = bad
            assert L.bls381_list_tree_update_device(h, *a, s) == EARG, (at, bad)
        assert L.bls381_list_tree_update_device(None, *good, s) == EARG
        assert L.bls381_list_tree_update_device(h, 0, None, 0, 16, None, None, s) == 0
        assert L.bls381_list_tree_root_device(None, 1, p(d_out), s) == EARG == L.bls381_list_tree_root_device(h, 1, None, s)
        assert L.bls381_list_tree_root_device(h, 1, p(d_out, 2), s) == EARG
        good = (1, p(d_idx), p(d_out), 96, p(d_out, 2048))
        for at, bad in ((0, 2 ** 31), (1, None), (1, p(d_idx, 4)), (2, None), (2, p(d_out, 2)), (3, 98), (3, 92), (4, None),
                        (4, p(d_out, 2050))):
            a = list(good)
            a[at] = bad
            assert L.bls381_list_tree_proofs_device(h, *a, s) == EARG, (at, bad)
        assert L.bls381_list_tree_proofs_device(None, *good, s) == EARG
        assert L.bls381_list_tree_proofs_device(h, *good, s) == 0
        got = dev.down(d_out, 4096)
        assert got[2048:2080] == want.root(False) and C.split(got[:96]) == want.tree.proof(0)
        assert got[96:2048] == b"\xEE" * 1952 and got[2080:] == b"\xEE" * 2016
        assert L.bls381_list_tree_count(h) == 5
        assert L.bls381_list_tree_root(h, 1, root) == 0 and root.raw == want.root(True)
        assert L.bls381_list_tree_read(h, 0, 5, out) == 0 and out.raw[:80] == blob
    finally:
        L.bls381_list_tree_destroy(h)
    # a packed list needs no append workspace, and none for an update when it has one chunk
    assert L.bls381_list_tree_create(4, 8, None, 0, ctypes.byref(h)) == 0
    try:
        assert L.bls381_list_tree_append_workspace_size(h, 1) == 0 == L.bls381_list_tree_update_workspace_size(h, 1)
        d_items, d_idx = dev.up(bytes(range(16))), dev.up(bytes(8))
        assert L.bls381_list_tree_append_device(h, 2, dev.ptr(d_items), None, dev.stream()) == 0
        assert L.bls381_list_tree_update_device(h, 1, dev.ptr(d_idx), 0, 8, dev.ptr(d_items, 8), None, dev.stream()) == 0
        dev.sync()
        assert L.bls381_list_tree_root(h, 0, root) == 0 and root.raw == bytes(range(8, 16)) * 2 + bytes(16)
    finally:
        L.bls381_list_tree_destroy(h)
