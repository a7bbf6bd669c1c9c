"""Merkle trees across items on the CPU: the node rules of csrc/bls381_merkle.hpp
and the plan of csrc/bls381_plan.hpp in the host build -- hc_merkle_root / hc_merkle_proofs run
the kernels' code with the workgroups and lanes as plain loops -- against
tests/golden/merkle_trees.json (the reference's merkle_minimal.py) and merkle_model.py; the
model itself against the fixture.  GPU half: test_merkle_tree_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import merkle_cases as C
import merkle_model as M

U64 = ctypes.c_uint64


class HostEngine:
    """The host build behind the engine interface of merkle_cases.py."""

    def __init__(self, lib):
        self.lib = lib

    def root(self, leaves, depth, first=0, length=None, threads=2):
        out = ctypes.create_string_buffer(32)
        blob = b"".join(leaves)
        rc = self.lib.hc_merkle_root(len(leaves), blob or None, first, depth, length is not None, length or 0,
                                     threads, out)
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0
        return out.raw

    def proofs(self, leaves, depth, indices, first=0, stride=None):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * depth if depth <= 64 else 0
        stride = row if stride is None else stride
        size = stride * len(idx) + 1
        out = ctypes.create_string_buffer(b"\xEE" * size, size)
        root = ctypes.create_string_buffer(32)
        rc = self.lib.hc_merkle_proofs(len(leaves), b"".join(leaves) or None, first, depth, len(idx),
                                       idx.ctypes.data_as(ctypes.c_void_p), out, stride, 2, root)
        if rc == -2:
            raise ValueError("rejected")
        assert rc == 0 and out.raw[stride * len(idx):] == b"\xEE"
        self.last_rows = out.raw[:stride * len(idx)]
        return [out.raw[stride * k:stride * k + row] for k in range(len(idx))], root.raw


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_merkle_tile.restype = ctypes.c_uint32
    lib.hc_merkle_root.argtypes = [ctypes.c_size_t, ctypes.c_char_p, U64, ctypes.c_uint32, ctypes.c_int, U64,
                                   ctypes.c_int, ctypes.c_char_p]
    lib.hc_merkle_proofs.argtypes = [ctypes.c_size_t, ctypes.c_char_p, U64, ctypes.c_uint32, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p]
    lib.hc_merkle_plan.argtypes = [U64, U64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p]
    for f in (lib.hc_merkle_root, lib.hc_merkle_proofs, lib.hc_merkle_plan):
        f.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def eng(L):
    return HostEngine(L)


@pytest.fixture(scope="module")
def W(L):
    w = L.hc_merkle_tile()
    assert w >= 4 and w & (w - 1) == 0          # a power of two
    return w


FX = M.fixture()


class ModelEngine:
    """merkle_model.py behind the same interface: the model against the fixture."""

    @staticmethod
    def root(leaves, depth, first=0, length=None):
        return M.merkle_root(leaves, depth, first, length)

    @staticmethod
    def proofs(leaves, depth, indices, first=0):
        t = M.Tree(leaves, first, depth)
        return [b"".join(t.proof(i)) for i in indices], t.root


# ---------------------------------------------------------------- the fixture
def test_fixture_is_the_one_the_generator_describes():
    assert [t["n"] for t in FX["trees"]] == [1, 2, 3, 5, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
    assert [t["n"] for t in FX["large"]] == [65537, 262145]
    assert [(t["first"], t["n"]) for t in FX["windows"]] == [(1, 1), (3, 2), (511, 2), (512, 1), (700, 600)]
    for t in FX["trees"]:
        assert sorted(t["proofs"]) == sorted(str(i) for i in (t["n"], t["n"] + 1, 2 ** 31))


@pytest.mark.parametrize("t", FX["trees"], ids=lambda t: "n%d" % t["n"])
def test_model_equals_fixture_trees(t):
    C.check_fixture_tree(ModelEngine, t)


def test_model_equals_fixture_large_windows_and_empty():
    for t in FX["large"]:
        C.check_fixture_large(ModelEngine, t)
    for t in FX["windows"]:
        C.check_fixture_window(ModelEngine, t)
    C.check_fixture_empty(ModelEngine, FX)
    assert M.Z[:32] == [bytes.fromhex(x) for x in M_deposit_zero_hashes()]


def M_deposit_zero_hashes():
    import json
    with open(os.path.join(M.ROOT, "tests", "golden", "deposit_tree.json")) as f:
        return json.load(f)["zerohashes"]


@pytest.mark.parametrize("t", FX["trees"], ids=lambda t: "n%d" % t["n"])
def test_host_equals_fixture_trees(eng, t):
    C.check_fixture_tree(eng, t)


@pytest.mark.parametrize("t", FX["large"], ids=lambda t: "n%d" % t["n"])
def test_host_equals_fixture_large(eng, t):
    C.check_fixture_large(eng, t)


def test_host_equals_fixture_windows_and_empty(eng):
    for t in FX["windows"]:
        C.check_fixture_window(eng, t)
    C.check_fixture_empty(eng, FX)


# ------------------------------------------------------------ tile boundaries
def test_tile_is_256_here_and_no_size_is_left_out(W):
    """The sizes run below follow W; with W = 256, W^2 + 1 = 65,537 <= 2^20 and none is skipped."""
    run, skipped = C.tile_sizes(W)
    assert (W, skipped) == (256, []) and run == [255, 256, 257, 65535, 65536, 65537]


@pytest.mark.parametrize("k", range(6))
def test_tile_boundary_sizes(eng, W, k):
    run, _ = C.tile_sizes(W)
    if k >= len(run):
        pytest.skip("W^2 sizes above 2^20 are left out")
    C.check_tile_size(eng, run[k])


@pytest.mark.parametrize("k", range(3))
def test_windows_that_straddle_a_tile(eng, W, k):
    C.check_tile_window(eng, *C.tile_windows(W)[k])


def test_threads_and_strides_do_not_change_the_bytes(eng, W):
    lv = C.leaves(C.TILE_ID, W * W + 1)
    assert eng.root(lv, 32, 0, None, threads=1) == eng.root(lv, 32, 0, None, threads=16)
    lv = lv[:W + 1]
    packed, root = eng.proofs(lv, 32, range(W + 1), 3)
    wide, root2 = eng.proofs(lv, 32, range(W + 1), 3, stride=1208)
    assert packed == wide and root == root2
    rows = eng.last_rows
    assert all(rows[1208 * k + 1024:1208 * (k + 1)] == b"\xEE" * 184 for k in range(W + 1))


# ------------------------------------------------- depth edges and length mix
def test_depth_edges(eng, W):
    C.check_depth_edges(eng, W)


def test_rejected_shapes(eng, L):
    C.check_rejected(eng)
    out = ctypes.create_string_buffer(32)
    assert L.hc_merkle_root(2 ** 31, None, 0, 32, 0, 0, 1, out) == -2           # n above 2^31 - 1
    assert L.hc_merkle_root(1, None, 0, 32, 0, 0, 1, out) == -2                 # a needed NULL
    assert L.hc_merkle_root(0, None, 0, 32, 0, 0, 1, None) == -2
    leaf = C.leaves(0, 1)[0]
    assert L.hc_merkle_proofs(1, leaf, 0, 32, 1, None, out, 1024, 1, out) == -2
    idx = np.zeros(1, dtype=np.uint64)
    assert L.hc_merkle_proofs(1, leaf, 0, 32, 1, idx.ctypes.data_as(ctypes.c_void_p), None, 1024, 1, out) == -2
    proofs = ctypes.create_string_buffer(1024)
    assert L.hc_merkle_proofs(1, leaf, 0, 32, 1, idx.ctypes.data_as(ctypes.c_void_p), proofs, 1023, 1, out) == -2
    assert L.hc_merkle_proofs(1, leaf, 0, 32, 1, idx.ctypes.data_as(ctypes.c_void_p), proofs, 1024, 1, out) == 0


def test_length_mix(eng):
    C.check_length_mix(eng)


# ------------------------------------------------------------------- the plan
def _plan(L, n, first, depth, keep):
    lv = np.zeros(65 * 3, dtype=np.uint64)
    ps = np.zeros(16 * 4, dtype=np.uint64)
    out = np.zeros(5, dtype=np.uint64)
    rc = L.hc_merkle_plan(n, first, depth, keep, lv.ctypes.data_as(ctypes.c_void_p),
                          ps.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    if rc:
        return None
    npass = int(out[0])
    return ([tuple(int(x) for x in lv[3 * h:3 * h + 3]) for h in range(65)],
            [tuple(int(x) for x in ps[4 * k:4 * k + 4]) for k in range(npass)],
            int(out[1]), int(out[2]), int(out[3]), int(out[4]))


NONE = 2 ** 64 - 1


def _align256(x):
    return (x + 255) & ~255


def test_plan_levels_passes_and_workspace(L, W):
    """Level bases and counts by the window rule, the pass list by the tile rule, the kept rows
    back to back without overlap, the workspace size as the carve of the level table and the node
    slice: n up to 2^40, depths 0 .. 64, windows at 0, inside a tile, across tiles and at the top
    of the tree."""
    logw = W.bit_length() - 1
    checked = 0
    for depth in list(range(0, 65, 3)) + [1, 2, 8, 16, 32, 40, 64]:
        cap = 2 ** depth
        for n in (0, 1, 2, 3, W - 1, W, W + 1, W * W, W * W + 1, 2 ** 31 - 1, 2 ** 40):
            for first in (0, 1, W - 1, W, 2 ** 31 + 7, cap - n, (cap - n) // 3):
                if first < 0 or first + n > cap or first + n >= 2 ** 64:
                    continue
                for keep in (0, 1):
                    plan = _plan(L, n, first, depth, keep)
                    assert plan is not None, (n, first, depth)
                    lv, passes, top, node_bytes, ws_bytes, bound = plan
                    for h in range(65):
                        base, count, off = lv[h]
                        assert base == (first >> h)
                        assert count == ((((first + n - 1) >> h) - base + 1) if n and h <= depth else 0)
                    # passes: W-aligned tiles over the real nodes, log2 W levels at a time, until one node
                    h = 0
                    for h0, steps, tile0, tiles in passes:
                        assert h0 == h and lv[h][1] > 1 and steps == min(logw, depth - h)
                        assert tile0 == lv[h][0] // W and tile0 + tiles - 1 == (lv[h][0] + lv[h][1] - 1) // W
                        h += steps
                    assert top == h and (n == 0 or h == depth or lv[h][1] == 1)
                    assert n == 0 or lv[top][1] == 1
                    assert len(passes) <= -(-depth // logw)
                    # kept rows
                    kept = [g for g in range(65) if lv[g][2] != NONE]
                    want = (list(range(1, depth + 1)) if n else []) if keep else [p[0] + p[1] for p in passes]
                    assert kept == want
                    end = 0
                    for g in kept:
                        assert lv[g][2] == end and lv[g][2] % 32 == 0      # back to back: no gap, no overlap
                        end += 32 * lv[g][1]
                    assert node_bytes == end
                    assert ws_bytes == _align256(_align256(65 * 24) + node_bytes)
                    if keep:
                        assert node_bytes <= bound
                    checked += 1
    assert checked > 1000
    assert _plan(L, 9, 0, 3, 0) is None and _plan(L, 1, 0, 65, 0) is None and _plan(L, 2, 2 ** 64 - 1, 64, 1) is None
