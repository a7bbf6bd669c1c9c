"""The deposit tree kept in memory on the CPU: the storage, the append's levels
and the query rule of csrc/bls381_deptree.hpp in the host build -- hc_deptree_* run the kernels'
code with the workgroups and lanes as plain loops -- against merkle_model.py and
tests/golden/deposit_tree_history.json (the reference's merkle_minimal.py); the model itself
against that fixture.  The cases are deposit_tree_cases.py's; GPU half: test_deposit_tree_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import deposit_tree_cases as C
import merkle_model as M

U64 = ctypes.c_uint64


class HostTree:
    def __init__(self, lib, capacity, depth):
        self.lib, self.depth, self.capacity = lib, depth, capacity
        self.h = lib.hc_deptree_create(capacity, depth)
        if not self.h:
            raise ValueError("rejected")

    def close(self):
        if self.h:
            self.lib.hc_deptree_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def count(self):
        return self.lib.hc_deptree_count(self.h)

    def append(self, leaves, threads=2):
        rc = self.lib.hc_deptree_append(self.h, len(leaves), b"".join(leaves) or None, threads)
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0

    def roots(self, counts):
        ks = np.ascontiguousarray(list(counts), dtype=np.uint64)
        size = 32 * len(ks) + 1
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        rc = self.lib.hc_deptree_roots(self.h, len(ks), ks.ctypes.data_as(ctypes.c_void_p), out)
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0 and out.raw[32 * len(ks):] == b"\xEE"
        return [out.raw[32 * q:32 * q + 32] for q in range(len(ks))]

    def proofs(self, indices, k, stride=None):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * self.depth
        stride = row if stride is None else stride
        size = stride * len(idx) + 1
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        root = ctypes.create_string_buffer(32)
        rc = self.lib.hc_deptree_proofs(self.h, k, len(idx), idx.ctypes.data_as(ctypes.c_void_p), out, stride, root)
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0 and out.raw[stride * len(idx):] == b"\xEE"
        self.last_rows = out.raw[:stride * len(idx)]
        return [out.raw[stride * t:stride * t + row] for t in range(len(idx))], root.raw


class HostEngine:
    """The host build behind the engine interface of deposit_tree_cases.py."""

    def __init__(self, lib):
        self.lib = lib

    def create(self, capacity, depth=32):
        return HostTree(self.lib, capacity, depth)


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_merkle_tile.restype = ctypes.c_uint32
    lib.hc_deptree_create.restype = ctypes.c_void_p
    lib.hc_deptree_create.argtypes = [U64, ctypes.c_uint32]
    lib.hc_deptree_destroy.restype = None
    lib.hc_deptree_destroy.argtypes = [ctypes.c_void_p]
    lib.hc_deptree_count.restype = U64
    lib.hc_deptree_count.argtypes = [ctypes.c_void_p]
    lib.hc_deptree_append.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_int]
    lib.hc_deptree_roots.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p]
    lib.hc_deptree_proofs.argtypes = [ctypes.c_void_p, U64, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p,
                                      ctypes.c_size_t, ctypes.c_char_p]
    lib.hc_deptree_plan.argtypes = [U64, U64, U64, ctypes.c_void_p]
    for f in (lib.hc_deptree_append, lib.hc_deptree_roots, lib.hc_deptree_proofs, lib.hc_deptree_plan):
        f.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def eng(L):
    return HostEngine(L)


@pytest.fixture(scope="module")
def W(L):
    w = L.hc_merkle_tile()
    assert w == 256             # the cases' sizes follow W; the GPU half assumes this value
    return w


# ---------------------------------------------------------------- the fixture
def test_fixture_is_the_one_the_generator_describes():
    fx = C.fixture()
    assert (fx["depth"], fx["id"], fx["n"], len(fx["roots"])) == (32, 300, 300, 300)
    pairs = {(p["k"], p["i"]) for p in fx["proofs"]}
    assert len(pairs) >= 12 and all(len(p["proof"]) == 32 for p in fx["proofs"])
    assert {(255, 254), (255, 0), (256, 255), (257, 256), (257, 0), (300, 299)} <= pairs      # i = k-1, i = 0, k around 256
    assert any(i >= k for k, i in pairs)                                                     # a zero leaf


def test_model_equals_fixture():
    fx = C.fixture()
    lv = C.leaves(fx["id"], fx["n"])
    for k in range(1, fx["n"] + 1):
        assert M.Tree(lv[:k], 0, 32).root.hex() == fx["roots"][k - 1], k
    for p in fx["proofs"]:
        assert [s.hex() for s in C.model(fx["id"], p["k"]).proof(p["i"])] == p["proof"]


def test_host_equals_fixture(eng):
    C.check_fixture(eng)


# --------------------------------------------------------------------- growth
def test_growth_sizes_are_the_ones_the_cases_name(W):
    sizes = C.growth_sizes(W)
    assert sizes == [1, 1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 23, 1, 255, 1]
    sums = np.cumsum(sizes)
    assert sums[12] == W and sums[14] == 2 * W and sums[15] == 2 * W + 1


def test_growth_by_uneven_appends(eng, W):
    C.check_growth(eng, W)


def test_append_that_straddles_tiles(eng, W):
    C.check_straddle_small(eng, W)


def test_append_across_a_tile_of_tiles(eng, W):
    C.check_straddle_large(eng, W)


def test_capacity_filled_exactly(eng):
    C.check_capacity(eng)


def test_small_depths(eng):
    C.check_small_depths(eng)


def test_rejected_calls(eng, L):
    C.check_rejected(eng)
    with eng.create(16) as tree:
        leaf = C.leaves(C.TREE_ID, 1)
        tree.append(leaf)
        out, root = ctypes.create_string_buffer(1024), ctypes.create_string_buffer(32)
        idx = np.zeros(1, dtype=np.uint64)
        ip = idx.ctypes.data_as(ctypes.c_void_p)
        assert L.hc_deptree_append(tree.h, 1, None, 1) == -2                      # needed NULLs
        assert L.hc_deptree_append(None, 1, leaf[0], 1) == -2
        assert L.hc_deptree_roots(tree.h, 1, None, out) == -2
        assert L.hc_deptree_roots(tree.h, 1, ip, None) == -2
        assert L.hc_deptree_proofs(tree.h, 1, 1, None, out, 1024, root) == -2
        assert L.hc_deptree_proofs(tree.h, 1, 1, ip, None, 1024, root) == -2
        assert L.hc_deptree_proofs(tree.h, 1, 1, ip, out, 1024, None) == -2
        assert L.hc_deptree_proofs(tree.h, 1, 1, ip, out, 1023, root) == -2       # stride below 32 * depth
        assert L.hc_deptree_proofs(tree.h, 1, 1, ip, out, 1024, root) == 0
        assert root.raw == C.model(C.TREE_ID, 1).root and tree.count == 1


def test_threads_and_strides_do_not_change_the_bytes(eng, W):
    lv = C.leaves(C.TREE_ID + 6, 3 * W + 7)
    with eng.create(4 * W) as a, eng.create(4 * W) as b:
        for t, threads in ((a, 1), (b, 16)):
            t.append(lv[:5], threads)
            t.append(lv[5:], threads)
        ks = [0, 5, W, 3 * W + 7]
        assert a.roots(ks) == b.roots(ks) == [C.model(C.TREE_ID + 6, k).root for k in ks]
        packed, root = a.proofs(range(W + 2), 2 * W)
        wide, root2 = a.proofs(range(W + 2), 2 * W, stride=1208)
        assert packed == wide and root == root2
        rows = a.last_rows
        assert all(rows[1208 * t + 1024:1208 * (t + 1)] == b"\xEE" * 184 for t in range(W + 2))


# ------------------------------------------------------------------- the plan
def _plan(L, capacity, count, n):
    out = np.zeros(1 + 4 * 8, dtype=np.uint64)
    if L.hc_deptree_plan(capacity, count, n, out.ctypes.data_as(ctypes.c_void_p)):
        return None
    return [tuple(int(x) for x in out[1 + 4 * k:5 + 4 * k]) for k in range(int(out[0]))]


def test_plan_work_follows_the_append_not_the_count(L, W):
    """Capacity 2^21, n = 16: the pass that starts at level h0 launches at most
    ceil((ceil(n / 2^h0) + 1) / W) + 1 tiles, and the plan is the same at count 2^20 and at
    2^20 + 2^19 -- an append's work does not depend on how full the tree is."""
    cap, n = 2 ** 21, 16
    logw = W.bit_length() - 1
    plan = _plan(L, cap, 2 ** 20, n)
    assert [(h0, steps) for h0, steps, _, _ in plan] == [(0, 8), (8, 8), (16, 5)]       # to H = 21
    for h0, steps, tile0, tiles in plan:
        assert h0 % logw == 0 and tile0 == (2 ** 20 >> h0) // W
        assert 1 <= tiles <= -(-(-(-n // 2 ** h0) + 1) // W) + 1
    shape = lambda p: [(h0, steps, tiles) for h0, steps, _, tiles in p]
    assert shape(_plan(L, cap, 2 ** 20 + 2 ** 19, n)) == shape(plan)
    # any count, any n: the bound holds, every tile holds a node of the window and the window's
    # ends are covered
    for count, m in ((0, 1), (W - 1, 2), (W * W - 1, 2), (12345, 4096), (2 ** 20 - 3, 70000), (cap - 1, 1), (0, cap)):
        for h0, steps, tile0, tiles in _plan(L, cap, count, m):
            assert tiles <= -(-(-(-m // 2 ** h0) + 1) // W) + 1
            assert tile0 == (count >> h0) // W and tile0 + tiles - 1 == ((count + m - 1) >> h0) // W
    assert _plan(L, cap, 5, 0) == []
    assert _plan(L, cap, cap, 1) is None and _plan(L, 2 ** 32, 0, 1) is None and _plan(L, 0, 0, 0) is None
