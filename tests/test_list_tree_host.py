"""The SSZ list tree kept in memory on the CPU: the storage, the dirty-tile rule
and the update's mark, compaction and tile lists of csrc/bls381_listtree.hpp in the host build --
hc_listtree_* run the kernels' code with the workgroups and lanes as plain loops -- against
merkle_model.py, ssz_oracle.py and tests/golden/list_tree_history.json (the reference's
merkle_minimal.py); the model itself against that fixture.  The cases are list_tree_cases.py's;
GPU half: test_list_tree_gpu.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import deposit_model
import list_tree_cases as C
import merkle_model as M

U64 = ctypes.c_uint64


def compile_root(typ):
    from bls381_amd import ssz
    return np.ascontiguousarray(ssz.compile_root(typ), dtype=np.uint32)


class HostTree:
    def __init__(self, lib, capacity, item_size, prog, device_form, threads=2):
        self.lib, self.capacity, self.item_size, self.device_form, self.threads = lib, capacity, item_size, device_form, threads
        self.h = lib.hc_listtree_create(capacity, item_size, prog.ctypes.data_as(ctypes.c_void_p) if prog is not None else None,
                                        len(prog) if prog is not None else 0)
        if not self.h:
            raise ValueError("rejected")

    def close(self):
        if self.h:
            self.lib.hc_listtree_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @staticmethod
    def ok(rc):
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0

    @property
    def count(self):
        return self.lib.hc_listtree_count(self.h)

    @property
    def depth(self):
        return self.lib.hc_listtree_depth(self.h)

    def append(self, items):
        self.ok(self.lib.hc_listtree_append(self.h, len(items), b"".join(items) or None, self.threads))

    def update(self, indices, off, length, values):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint32)
        self.ok(self.lib.hc_listtree_update(self.h, len(idx), idx.ctypes.data_as(ctypes.c_void_p) if len(idx) else None,
                                            off, length, b"".join(values) or None, int(self.device_form), self.threads))

    def root(self, mix):
        size = 33
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        self.ok(self.lib.hc_listtree_root(self.h, int(mix), out))
        assert out.raw[32:] == b"\xEE"
        return out.raw[:32]

    def proofs(self, indices, stride=None):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * self.depth
        stride = row if stride is None else stride
        size = stride * len(idx) + 1
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        root = ctypes.create_string_buffer(32)
        self.ok(self.lib.hc_listtree_proofs(self.h, len(idx), idx.ctypes.data_as(ctypes.c_void_p) if len(idx) else None,
                                            out, stride, root))
        raw = out.raw
        assert raw[stride * len(idx):] == b"\xEE"
        self.last_rows = raw[:stride * len(idx)]
        return [raw[stride * t:stride * t + row] for t in range(len(idx))], root.raw

    def read(self, first, n):
        size = self.item_size * n + 1
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        self.ok(self.lib.hc_listtree_read(self.h, first, n, out))
        raw = out.raw
        assert raw[size - 1:] == b"\xEE"
        return [raw[self.item_size * i:self.item_size * (i + 1)] for i in range(n)]

    def tail(self):
        out = ctypes.create_string_buffer(self.item_size * self.capacity)
        self.ok(self.lib.hc_listtree_read_capacity(self.h, out))
        return out.raw[self.item_size * self.count:]


class HostEngine:
    """The host build behind the engine interface of list_tree_cases.py."""

    def __init__(self, lib, device_form):
        self.lib, self.device_form = lib, device_form

    def create(self, capacity, typ):
        return HostTree(self.lib, capacity, C.item_size(typ), compile_root(typ) if typ[0] == "container" else None,
                        self.device_form)

    def create_raw(self, capacity, item_size, prog):
        return HostTree(self.lib, capacity, item_size, prog, self.device_form)

    @staticmethod
    def verify(leaves, proofs, depth, indices, root):
        return [deposit_model.branch_root(leaf, C.split(p), depth, i) == root for leaf, p, i in zip(leaves, proofs, indices)]


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_merkle_tile.restype = ctypes.c_uint32
    lib.hc_listtree_create.restype = ctypes.c_void_p
    lib.hc_listtree_create.argtypes = [U64, U64, ctypes.c_void_p, ctypes.c_uint32]
    lib.hc_listtree_destroy.restype = None
    lib.hc_listtree_destroy.argtypes = [ctypes.c_void_p]
    lib.hc_listtree_count.restype = U64
    lib.hc_listtree_count.argtypes = [ctypes.c_void_p]
    lib.hc_listtree_depth.restype = ctypes.c_uint32
    lib.hc_listtree_depth.argtypes = [ctypes.c_void_p]
    lib.hc_listtree_append.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int]
    lib.hc_listtree_update.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                       ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
    lib.hc_listtree_root.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p]
    lib.hc_listtree_proofs.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t,
                                       ctypes.c_char_p]
    lib.hc_listtree_read.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_char_p]
    lib.hc_listtree_read_capacity.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    lib.hc_listtree_plan.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    for f in (lib.hc_listtree_append, lib.hc_listtree_update, lib.hc_listtree_root, lib.hc_listtree_proofs,
              lib.hc_listtree_read, lib.hc_listtree_read_capacity, lib.hc_listtree_plan):
        f.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module", params=["host_pointer", "device"])
def eng(request, L):
    """The two forms' update semantics (rejecting and keeping the last, or skipping and running all)."""
    return HostEngine(L, request.param == "device")


@pytest.fixture(scope="module")
def W(L):
    w = L.hc_merkle_tile()
    assert w == 256             # the cases' sizes follow W; the GPU half assumes this value
    return w


# ---------------------------------------------------------------- 1. the fixture
def test_fixture_is_the_one_the_generator_describes():
    fx = C.fixture()
    assert sorted(fx) == ["bytes32", "uint64", "validator"]
    for name, size in (("validator", 121), ("uint64", 8), ("bytes32", 32)):
        steps = fx[name]["steps"]
        assert fx[name]["item_size"] == size and len(steps) == 40
        assert {s["op"] for s in steps} == {"append", "update"}
        assert all(len(s["root"]) == 64 == len(s["root_unmixed"]) for s in steps)
    spans = {(s["off"], s["len"]) for s in fx["validator"]["steps"] if s["op"] == "update"}
    assert {(113, 8), (112, 1), (96, 8)} <= spans


@pytest.mark.parametrize("name", ["validator", "uint64", "bytes32"])
def test_model_equals_fixture(name):
    fx = C.fixture()[name]
    items = []
    for st, items in C.replay(fx):
        m = C.Model(C.FIXTURE_TYPES[name], items)
        assert m.root(True).hex() == st["root"] and m.root(False).hex() == st["root_unmixed"]
    assert [x.hex() for x in items] == fx["final"]


@pytest.mark.parametrize("name", ["validator", "uint64", "bytes32"])
def test_host_equals_fixture(eng, name):
    C.check_fixture(eng, name)


# ----------------------------------------------------------------- 2 .. 10
def test_growth_sizes_are_the_ones_the_cases_name(W):
    assert list(np.cumsum(C.growth_sizes(W))) == [1, 2, 3, 4, 5, W - 1, W, W + 1, W + 24, 2 * W + 1]


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.BYTES32, 1), (C.UINT64, 4)], ids=["pair16", "bytes32", "uint64"])
def test_growth_through_depth_changes(eng, W, typ, per):
    C.check_growth(eng, W, typ, per)


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.BYTES32, 1), (C.UINT64, 4)], ids=["pair16", "bytes32", "uint64"])
def test_updates_inside_and_across_tiles(eng, W, typ, per):
    C.check_updates(eng, W, typ, per)


@pytest.mark.parametrize("typ,per", [(C.PAIR16, 1), (C.UINT64, 4)], ids=["pair16", "uint64"])
def test_three_passes(eng, W, typ, per):
    C.check_three_passes(eng, W, typ, per)


def test_packed_partial_chunks(eng):
    C.check_packed_partial(eng)


def test_field_updates_on_validator_records(eng):
    C.check_validator_fields(eng)


def test_repeated_indices(eng, W):
    C.check_repeated(eng, W)


def test_rejected_calls(eng, L):
    C.check_rejected(eng, compile_root(C.PAIR16))
    bad = np.asarray([1, 0, 33], dtype=np.uint32)                 # a chunk of 33 bytes
    with pytest.raises(ValueError):
        eng.create_raw(4, 64, bad)
    assert L.hc_listtree_count(None) == 0 == L.hc_listtree_depth(None)
    L.hc_listtree_destroy(None)
    with eng.create(8, C.UINT64) as tree:
        tree.append([b"\x01" * 8] * 5)
        out, root = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(32)
        idx = np.zeros(1, dtype=np.uint64)
        i32 = np.zeros(1, dtype=np.uint32)
        ip, jp = idx.ctypes.data_as(ctypes.c_void_p), i32.ctypes.data_as(ctypes.c_void_p)
        assert tree.depth == 1
        assert L.hc_listtree_append(tree.h, 1, None, 1) == -2                        # needed NULLs
        assert L.hc_listtree_append(None, 1, b"\x00" * 8, 1) == -2
        assert L.hc_listtree_update(tree.h, 1, None, 0, 8, b"\x00" * 8, 0, 1) == -2
        assert L.hc_listtree_update(tree.h, 1, jp, 0, 8, None, 0, 1) == -2
        assert L.hc_listtree_update(None, 1, jp, 0, 8, b"\x00" * 8, 0, 1) == -2
        assert L.hc_listtree_root(tree.h, 1, None) == -2 == L.hc_listtree_root(None, 1, root)
        assert L.hc_listtree_proofs(tree.h, 1, None, out, 32, root) == -2
        assert L.hc_listtree_proofs(tree.h, 1, ip, None, 32, root) == -2
        assert L.hc_listtree_proofs(tree.h, 1, ip, out, 32, None) == -2
        assert L.hc_listtree_proofs(tree.h, 1, ip, out, 31, root) == -2              # stride below 32 * depth
        assert L.hc_listtree_read(tree.h, 0, 1, None) == -2
        assert L.hc_listtree_proofs(tree.h, 1, ip, out, 32, root) == 0
        assert root.raw == C.Model(C.UINT64, [b"\x01" * 8] * 5).root(False) and tree.count == 5


def test_threads_and_strides_do_not_change_the_bytes(L, W):
    rng = random.Random("threads")
    items = C.rand_items(rng, C.BYTES32, 3 * W + 7)
    idx = sorted(rng.sample(range(3 * W + 7), 40))
    vals = C.rand_items(rng, C.BYTES32, 40)
    trees = [HostTree(L, 4 * W, 32, None, True, threads) for threads in (1, 16)]
    try:
        for t in trees:
            t.append(items[:5])
            t.append(items[5:])
            t.update(idx, 0, 32, vals)
        C.apply_update(items, idx, 0, 32, vals)
        a, b = trees
        assert a.root(True) == b.root(True) == C.Model(C.BYTES32, items).root(True)
        d = a.depth
        packed, root = a.proofs(range(W + 2))
        wide, root2 = a.proofs(range(W + 2), stride=32 * d + 184)
        assert packed == wide and root == root2
        rows = a.last_rows
        assert all(rows[(32 * d + 184) * t + 32 * d:(32 * d + 184) * (t + 1)] == b"\xEE" * 184 for t in range(W + 2))
    finally:
        for t in trees:
            t.close()


# ------------------------------------------------------------- 11. the plan
def _plan(L, tree, indices):
    idx = np.ascontiguousarray(indices, dtype=np.uint32)
    cap = 2 + 4 * 4 + 4 * len(idx) + 8
    out = np.zeros(cap, dtype=np.uint64)
    assert L.hc_listtree_plan(tree.h, len(idx), idx.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), cap) == 0
    launches, passes = int(out[0]), int(out[1])
    at, plan = 2, []
    for _ in range(passes):
        h0, steps, grid, n = (int(x) for x in out[at:at + 4])
        plan.append((h0, steps, grid, [int(x) for x in out[at + 4:at + 4 + n]]))
        at += 4 + n
    return launches, plan


@pytest.mark.parametrize("capacity,passes", [(200, 1), (3 * 256 + 1, 2), (256 * 256 + 256, 3)])
def test_plan_launches_follow_the_height_not_the_update(L, W, capacity, passes):
    """An update's launch count is the same for n_upd = 1, W and the count, at heights of one,
    two and three passes -- the scatter, the mark, the compaction and a launch per pass (a
    composite list: one more, the leaves) -- and the dirty-tile lists are
    sorted(set(i >> (h0 + 8))), each pass launching min(n_upd, tiles of its row) workgroups."""
    logw = W.bit_length() - 1
    rng = random.Random(capacity)
    for typ, extra in ((C.BYTES32, 0), (C.PAIR16, 1)):
        count = capacity - 3
        size = C.item_size(typ)
        with HostTree(L, capacity, size, compile_root(typ) if extra else None, True) as tree:
            tree.append([bytes(size)] * count)
            seen = set()
            for n_upd in (1, min(W, count), count):
                idx = [rng.randrange(count) for _ in range(n_upd)] if n_upd < count else list(range(count))
                launches, plan = _plan(L, tree, idx + [count, 2 ** 32 - 1])          # indices at or above the count mark nothing
                seen.add(launches)
                assert launches == 3 + passes + extra
                assert [(h0, steps) for h0, steps, _, _ in plan] == [
                    (logw * k, min(logw, (capacity - 1).bit_length() - logw * k)) for k in range(passes)]
                for h0, _, grid, tiles in plan:
                    assert tiles == sorted({i >> (h0 + logw) for i in idx})
                    assert grid == min(n_upd + 2, ((count - 1) >> (h0 + logw)) + 1) >= len(tiles)
            assert len(seen) == 1


def test_plan_of_a_packed_list_marks_chunk_tiles(L, W):
    """uint64 items: four to a chunk, so item i dirties tile (i >> 2) >> 8 of pass 0."""
    with HostTree(L, 4 * 3 * W, 8, None, True) as tree:
        tree.append([bytes(8)] * (4 * 2 * W + 5))
        launches, plan = _plan(L, tree, [0, 4 * W - 1, 4 * W, 4 * 2 * W + 4])
        assert launches == 3 + 2 and [t for _, _, _, t in plan] == [[0, 1, 2], [0]]
