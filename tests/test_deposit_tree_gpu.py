"""The deposit tree kept on the device: bls381_deposit_tree_*, host-pointer forms
(through bls381_amd.deposit_tree.DepositTree) and device forms, against merkle_model.py and
tests/golden/deposit_tree_history.json (the reference's merkle_minimal.py); deposits built under
the root of an earlier count then go through process_deposits.  The cases are
deposit_tree_cases.py's, shared with the CPU half (test_deposit_tree_host.py)."""
import ctypes
import random

import numpy as np
import pytest

import deposit_model as D
import deposit_tree_cases as C
import merkle_model as M
import ssz_oracle as S

pytestmark = pytest.mark.gpu

W = 256                    # MERKLE_TILE (csrc/bls381_plan.hpp); test_deposit_tree_host.py reads it from the host build
SLACK = 64                 # bytes behind every device output that must stay 0xEE
DOMAIN = 3


class HostPointerTree:
    """DepositTree behind the tree interface of deposit_tree_cases.py."""

    def __init__(self, tree):
        self.t = tree
        self.capacity = tree.capacity

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.t.close()
        return False

    def close(self):
        self.t.close()

    @property
    def count(self):
        return self.t.count

    def append(self, leaves):
        self.t.append(list(leaves))

    def roots(self, counts):
        return self.t.roots(counts)

    def proofs(self, indices, k):
        return self.t.proofs(indices, k)


class HostPointerEngine:
    def __init__(self, mod):
        self.mod = mod

    def create(self, capacity, depth=32):
        return HostPointerTree(self.mod.DepositTree(capacity, depth))


class Dev:
    """torch buffers for the _device forms on the current stream; every output is pre-filled
    with 0xEE and the bytes behind it must stay so."""

    def __init__(self, native):
        import torch
        self.torch, self.L, self.EARG = torch, native.lib(), native.EARG
        self.dev = torch.device("cuda:0")

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def up(self, data: bytes):
        if not data:
            return None
        return self.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.dev)

    def filled(self, nbytes):
        return self.torch.full((int(nbytes) + SLACK,), 0xEE, dtype=self.torch.uint8, device=self.dev)

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def down(self, t, nbytes):
        self.torch.cuda.current_stream().synchronize()
        raw = t.cpu().numpy().tobytes()
        assert raw[nbytes:] == b"\xEE" * SLACK, "bytes behind the output were written"
        return raw[:nbytes]


class DeviceTree:
    """The _device forms: queued on the current stream, read back after a synchronise."""

    def __init__(self, dev, capacity, depth):
        self.d, self.L, self.depth, self.capacity = dev, dev.L, depth, capacity
        h = ctypes.c_void_p()
        rc = self.L.bls381_deposit_tree_create(capacity, depth, ctypes.byref(h))
        if rc == dev.EARG:
            raise ValueError("rejected")
        assert rc == 0 and h
        self.h = h
        assert self.L.bls381_deposit_tree_capacity(h) == capacity

    def close(self):
        if self.h:
            self.L.bls381_deposit_tree_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def count(self):
        return self.L.bls381_deposit_tree_count(self.h)

    def ok(self, rc):
        if rc == self.d.EARG:
            raise ValueError("rejected")
        assert rc == 0

    def append(self, leaves):
        d_leaves = self.d.up(b"".join(leaves))
        self.ok(self.L.bls381_deposit_tree_append_device(self.h, len(leaves), self.d.ptr(d_leaves), self.d.stream()))

    def roots(self, counts):
        ks = np.ascontiguousarray(list(counts), dtype=np.uint64)
        out = self.d.filled(32 * len(ks))
        self.ok(self.L.bls381_deposit_tree_roots_device(self.h, len(ks), ks.ctypes.data_as(ctypes.c_void_p),
                                                        self.d.ptr(out), self.d.stream()))
        raw = self.d.down(out, 32 * len(ks))
        return [raw[32 * q:32 * q + 32] for q in range(len(ks))]

    def queue_proofs(self, indices, k, stride=None):
        """Queues the query with buffers of its own; read() synchronises and returns its result."""
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * self.depth
        stride = row if stride is None else stride
        d_idx = self.d.up(idx.tobytes())
        ws = self.d.filled(self.L.bls381_deposit_tree_proofs_workspace_size(self.depth))
        out, root = self.d.filled(stride * len(idx)), self.d.filled(32)
        self.ok(self.L.bls381_deposit_tree_proofs_device(self.h, k, len(idx), self.d.ptr(d_idx), self.d.ptr(out), stride,
                                                         self.d.ptr(root), self.d.ptr(ws), self.d.stream()))

        def read():
            rows = self.d.down(out, stride * len(idx))
            self.last_rows = rows
            return [rows[stride * t:stride * t + row] for t in range(len(idx))], self.d.down(root, 32)
        read.keep = (d_idx, ws)
        return read

    def proofs(self, indices, k, stride=None):
        return self.queue_proofs(indices, k, stride)()


class DeviceEngine:
    def __init__(self, dev):
        self.dev = dev

    def create(self, capacity, depth=32):
        return DeviceTree(self.dev, capacity, depth)


@pytest.fixture(scope="module")
def dev(native):
    return Dev(native)


@pytest.fixture(scope="module")
def mod(native):
    from bls381_amd import deposit_tree
    return deposit_tree


@pytest.fixture(scope="module", params=["host_pointer", "device"])
def eng(request, mod, dev):
    return HostPointerEngine(mod) if request.param == "host_pointer" else DeviceEngine(dev)


# ------------------------------------------------------------ the shared cases
def test_fixture(eng):
    C.check_fixture(eng)


def test_growth_by_uneven_appends(eng):
    assert C.growth_sizes(W)[-4:] == [23, 1, 255, 1]
    C.check_growth(eng, W)


def test_append_that_straddles_tiles(eng):
    C.check_straddle_small(eng, W)


def test_append_across_a_tile_of_tiles(eng):
    C.check_straddle_large(eng, W)


def test_capacity_filled_exactly(eng):
    C.check_capacity(eng)


def test_small_depths(eng):
    C.check_small_depths(eng)


def test_rejected_calls(eng):
    C.check_rejected(eng)


# ----------------------------------------------------------- device forms only
def test_queued_queries_keep_their_own_results(dev):
    """Appends and queries queued back to back on one stream, read only at the end: a query
    holds what it was asked at its count, whatever was queued behind it; proof rows of 1,208
    bytes keep the 184 bytes behind each proof."""
    tid = C.TREE_ID + 7
    lv = C.leaves(tid, 2 * W + 9)
    with DeviceTree(dev, 4 * W, 32) as tree:
        tree.append(lv[:W - 1])
        q1 = tree.queue_proofs([0, W - 2, W - 1], W - 1, stride=1208)
        tree.append(lv[W - 1:W + 5])
        q2 = tree.queue_proofs([0, W - 2, W - 1, W + 4], W + 5)
        q3 = tree.queue_proofs([W - 2], W - 1)
        tree.append(lv[W + 5:])
        for q, k, idx in ((q1, W - 1, [0, W - 2, W - 1]), (q2, W + 5, [0, W - 2, W - 1, W + 4]), (q3, W - 1, [W - 2])):
            m = C.model(tid, k)
            proofs, root = q()
            assert root == m.root and [C.split(p) for p in proofs] == [m.proof(i) for i in idx], k
            if q is q1:
                assert all(tree.last_rows[1208 * t + 1024:1208 * (t + 1)] == b"\xEE" * 184 for t in range(3))
        assert tree.roots([2 * W + 9])[0] == C.model(tid, 2 * W + 9).root


def test_many_counts_in_one_call(eng):
    """More counts than one launch of the roots kernel carries."""
    tid = C.TREE_ID
    lv = C.leaves(tid, 2 * W + 1)
    with eng.create(4 * W) as tree:
        tree.append(lv)
        counts = [(37 * q) % (2 * W + 2) for q in range(1100)]
        assert tree.roots(counts) == [C.model(tid, k).root for k in counts]


# ------------------------------------------------------------------- deposits
N_DEP = 40


def test_bad_arguments(native, dev):
    L, EARG = native.lib(), native.EARG
    h = ctypes.c_void_p()
    assert L.bls381_deposit_tree_create(16, 32, None) == EARG
    assert L.bls381_deposit_tree_create(0, 32, ctypes.byref(h)) == EARG and not h
    assert L.bls381_deposit_tree_create(1, 0, ctypes.byref(h)) == EARG
    assert L.bls381_deposit_tree_create(1, 33, ctypes.byref(h)) == EARG
    assert L.bls381_deposit_tree_create(2 ** 32, 32, ctypes.byref(h)) == EARG
    assert L.bls381_deposit_tree_count(None) == 0 == L.bls381_deposit_tree_capacity(None)
    L.bls381_deposit_tree_destroy(None)
    assert L.bls381_deposit_tree_proofs_workspace_size(33) == 0 == L.bls381_deposit_tree_proofs_workspace_size(0)
    assert L.bls381_deposit_tree_deposits_workspace_size(2 ** 31) == 0
    assert L.bls381_deposit_tree_append_data_workspace_size(2 ** 31) == 0
    assert L.bls381_deposit_tree_proofs_workspace_size(32) >= 33 * 32
    lv = C.leaves(C.TREE_ID, 5)
    blob = b"".join(lv)
    out, root = ctypes.create_string_buffer(2048), ctypes.create_string_buffer(32)
    idx = np.zeros(2, dtype=np.uint64)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    assert L.bls381_deposit_tree_create(16, 32, ctypes.byref(h)) == 0
    try:
        # host-pointer forms: NULLs, k above the count, a short stride, deposits outside the count
        assert L.bls381_deposit_tree_append(None, 1, blob) == EARG
        assert L.bls381_deposit_tree_append(h, 1, None) == EARG
        assert L.bls381_deposit_tree_append(h, 0, None) == 0
        assert L.bls381_deposit_tree_append_data(h, 1, None) == EARG
        assert L.bls381_deposit_tree_append_data(h, 0, None) == 0
        assert L.bls381_deposit_tree_append(h, 5, blob) == 0 and L.bls381_deposit_tree_count(h) == 5
        assert L.bls381_deposit_tree_append(h, 12, bytes(32 * 12)) == EARG and L.bls381_deposit_tree_count(h) == 5
        assert L.bls381_deposit_tree_roots(h, 1, None, out) == EARG
        assert L.bls381_deposit_tree_roots(h, 1, ip, None) == EARG
        assert L.bls381_deposit_tree_roots(h, 0, None, None) == 0
        idx[0] = 6
        assert L.bls381_deposit_tree_roots(h, 1, ip, out) == EARG
        idx[0] = 0
        assert L.bls381_deposit_tree_proofs(h, 6, 1, ip, out, 1024, root) == EARG
        assert L.bls381_deposit_tree_proofs(h, 5, 1, None, out, 1024, root) == EARG
        assert L.bls381_deposit_tree_proofs(h, 5, 1, ip, None, 1024, root) == EARG
        assert L.bls381_deposit_tree_proofs(h, 5, 1, ip, out, 1024, None) == EARG
        assert L.bls381_deposit_tree_proofs(h, 5, 1, ip, out, 1023, root) == EARG
        assert L.bls381_deposit_tree_proofs(h, 5, 0, None, None, 1024, root) == 0 and root.raw == C.model(C.TREE_ID, 5).root
        data, dep = bytes(184 * 2), ctypes.create_string_buffer(1208 * 2)
        assert L.bls381_deposit_tree_deposits(h, 5, 4, 2, data, dep) == EARG          # first_index + n > k
        assert L.bls381_deposit_tree_deposits(h, 6, 4, 2, data, dep) == EARG          # k above the count
        assert L.bls381_deposit_tree_deposits(h, 5, 6, 0, data, dep) == EARG          # first_index > k
        assert L.bls381_deposit_tree_deposits(h, 5, 3, 2, None, dep) == EARG
        assert L.bls381_deposit_tree_deposits(h, 5, 3, 2, data, None) == EARG
        assert L.bls381_deposit_tree_deposits(h, 5, 5, 0, None, None) == 0
        assert L.bls381_deposit_tree_deposits(h, 5, 3, 2, data, dep) == 0
        # device forms: NULL workspace / root, misaligned proofs, stride, indices and leaves
        d_leaf, ws, d_out, d_idx = dev.up(blob), dev.filled(1 << 14), dev.filled(4096), dev.up(bytes(16))
        p, s = dev.ptr, dev.stream()
        off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
        args = lambda k, ix, pr, st, rt, w: (h, k, 1, ix, pr, st, rt, w, s)
        good = (5, p(d_idx), p(d_out), 1024, off(d_out, 2048), p(ws))
        for at, bad in ((0, 6), (1, None), (1, off(d_idx, 4)), (2, None), (2, off(d_out, 2)), (3, 1026), (3, 1020),
                        (4, None), (5, None)):
            a = list(good)
            a[at] = bad
            assert L.bls381_deposit_tree_proofs_device(*args(*a)) == EARG, (at, bad)
        assert L.bls381_deposit_tree_proofs_device(*args(*good)) == 0
        assert dev.down(d_out, 4096)[2048:2080] == C.model(C.TREE_ID, 5).root
        assert L.bls381_deposit_tree_append_device(h, 1, None, s) == EARG
        assert L.bls381_deposit_tree_append_device(h, 1, off(d_leaf, 1), s) == EARG
        assert L.bls381_deposit_tree_append_device(h, 0, None, s) == 0
        assert L.bls381_deposit_tree_append_data_device(h, 1, p(d_leaf), None, s) == EARG
        assert L.bls381_deposit_tree_roots_device(h, 1, ip, None, s) == EARG
        d_data = dev.up(data)
        assert L.bls381_deposit_tree_deposits_device(h, 5, 3, 2, p(d_data), p(d_out), None, s) == EARG
        assert L.bls381_deposit_tree_deposits_device(h, 5, 3, 2, p(d_data), off(d_out, 2), p(ws), s) == EARG
        assert L.bls381_deposit_tree_deposits_device(h, 5, 4, 2, p(d_data), p(d_out), p(ws), s) == EARG
        assert L.bls381_deposit_tree_count(h) == 5
        dev.torch.cuda.current_stream().synchronize()
    finally:
        L.bls381_deposit_tree_destroy(h)
    # deposits need the deposit contract's depth
    assert L.bls381_deposit_tree_create(7, 3, ctypes.byref(h)) == 0
    try:
        assert L.bls381_deposit_tree_append(h, 5, blob) == 0
        assert L.bls381_deposit_tree_deposits(h, 5, 3, 2, bytes(184 * 2), ctypes.create_string_buffer(1208 * 2)) == EARG
    finally:
        L.bls381_deposit_tree_destroy(h)


@pytest.fixture(scope="module")
def deposit_datas(native):
    """40 DepositData of 40 new keys, each signed over its signing root; built once."""
    rng = random.Random(0xB15_0020)
    sks = [rng.randrange(1, 1 << 250) for _ in range(N_DEP)]
    sk_blob = b"".join(k.to_bytes(32, "big") for k in sks)
    pks = native.privtopub_batch(sk_blob)
    values = [{"pubkey": pks[48 * i:48 * i + 48], "withdrawal_credentials": rng.randbytes(32),
               "amount": 32 * 10 ** 9 + i, "signature": b"\x00" * 96} for i in range(N_DEP)]
    roots = b"".join(S.signing_root(S.DepositData, v) for v in values)
    sigs = native.sign_batch(roots, sk_blob, DOMAIN.to_bytes(8, "big") * N_DEP)
    for i, v in enumerate(values):
        v["signature"] = sigs[96 * i:96 * i + 96]
    datas = [S.serialize(S.DepositData, v) for v in values]
    leaves = [S.hash_tree_root(S.DepositData, v) for v in values]
    return datas, leaves


def test_append_data_equals_append_of_the_roots(native, mod, dev, deposit_datas):
    datas, leaves = deposit_datas
    cuts = (0, 7, 27, N_DEP)
    ks = list(range(N_DEP + 1))
    want = [M.Tree(leaves[:k], 0, 32).root for k in ks]
    with mod.DepositTree(100) as a, mod.DepositTree(100) as b:
        for lo, hi in zip(cuts, cuts[1:]):
            a.append_deposit_data(datas[lo:hi])
            b.append(leaves[lo:hi])
        assert a.count == b.count == N_DEP
        assert a.roots(ks) == b.roots(ks) == want
        assert a.proofs([0, 26, 39], 33) == b.proofs([0, 26, 39], 33)
    # the device form, its leaves hashed straight into the tree
    L = native.lib()
    with DeviceTree(dev, 100, 32) as t:
        for lo, hi in zip(cuts, cuts[1:]):
            d_data = dev.up(b"".join(datas[lo:hi]))
            ws = dev.filled(L.bls381_deposit_tree_append_data_workspace_size(hi - lo))
            assert L.bls381_deposit_tree_append_data_device(t.h, hi - lo, dev.ptr(d_data), dev.ptr(ws), dev.stream()) == 0
        assert t.count == N_DEP and t.roots(ks) == want


def test_deposits_under_an_earlier_root_go_through_process_deposits(native, mod, dev, deposit_datas):
    """A tree of 40 signed DepositData in three uneven appends; Deposits for leaves 10 .. 24 under
    the root at count 30, below the final count: process_deposits accepts them under roots([30])
    and refuses them under the final root."""
    from bls381_amd.registry import PubkeyRegistry
    datas, leaves = deposit_datas
    k, first, n = 30, 10, 15
    with mod.DepositTree(2 ** 17) as tree:
        for lo, hi in ((0, 3), (3, 29), (29, N_DEP)):
            tree.append_deposit_data(datas[lo:hi])
        m = M.Tree(leaves[:k], 0, 32)
        deposits = tree.deposits(datas[first:first + n], first, k)
        assert len(deposits) == n and all(len(d) == 1208 for d in deposits)
        assert [d[1024:] for d in deposits] == datas[first:first + n]              # the data, as given
        assert [C.split(d[:1024]) for d in deposits] == [m.proof(first + i) for i in range(n)]
        root_k, root_final = tree.roots([k, N_DEP])
        assert root_k == m.root and root_final == M.Tree(leaves, 0, 32).root != root_k
        reg = PubkeyRegistry(256)
        res = reg.process_deposits(deposits, first, root_k, DOMAIN, commit=False)
        assert res.first_bad_proof == -1 and list(res.outcome) == [D.NEW] * n
        res = reg.process_deposits(deposits, first, root_final, DOMAIN, commit=False)
        assert res.first_bad_proof == 0
        with pytest.raises(ValueError):
            tree.deposits(datas[first:first + n], k - n + 1, k)                    # first_index + n > k
        assert tree.deposits(datas[:N_DEP], 0) == tree.deposits(datas[:N_DEP], 0, N_DEP)
        # the device form: the same bytes, nothing behind them
        L = native.lib()
        d_data = dev.up(b"".join(datas[first:first + n]))
        ws, d_dep = dev.filled(L.bls381_deposit_tree_deposits_workspace_size(n)), dev.filled(1208 * n)
        assert L.bls381_deposit_tree_deposits_device(tree._h, k, first, n, dev.ptr(d_data), dev.ptr(d_dep), dev.ptr(ws),
                                                     dev.stream()) == 0
        assert dev.down(d_dep, 1208 * n) == b"".join(deposits)
