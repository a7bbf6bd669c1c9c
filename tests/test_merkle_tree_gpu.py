"""Merkle trees across items on the device: bls381_merkle_root / _proofs,
bls381_ssz_list_root and bls381_deposits_build, host-pointer and device forms, and their Python
front (bls381_amd/ssz.py) against tests/golden/merkle_trees.json (the reference's
merkle_minimal.py), merkle_model.py and deposit_model.py; the built deposits then go through
process_deposits.  The cases are merkle_cases.py's, shared with the CPU half
(test_merkle_tree_host.py)."""
import ctypes
import random

import numpy as np
import pytest

import deposit_model as D
import merkle_cases as C
import merkle_model as M
import ssz_oracle as S

pytestmark = pytest.mark.gpu

W = 256                    # MERKLE_TILE (csrc/bls381_plan.hpp); test_merkle_tree_host.py reads it from the host build
FX = M.fixture()
SLACK = 64                 # bytes behind every device output that must stay 0xEE
DOMAIN = 3


@pytest.fixture(scope="module")
def ssz(native):
    from bls381_amd import ssz
    return ssz


class HostPointerEngine:
    """bls381_merkle_root / bls381_merkle_proofs through bls381_amd.ssz."""

    def __init__(self, ssz):
        self.ssz = ssz

    def root(self, leaves, depth, first=0, length=None):
        return self.ssz.merkle_root(leaves, depth, first, length)

    def proofs(self, leaves, depth, indices, first=0):
        return self.ssz.merkle_proofs(leaves, depth, list(indices), first)


class DeviceEngine:
    """The _device forms on torch buffers and the current stream; every output is pre-filled
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

    def root(self, leaves, depth, first=0, length=None):
        d_leaves = self.up(b"".join(leaves))
        ws = self.filled(self.L.bls381_merkle_root_workspace_size(len(leaves), first, depth))
        out = self.filled(32)
        rc = self.L.bls381_merkle_root_device(len(leaves), self.ptr(d_leaves), first, depth, length is not None,
                                              length or 0, self.ptr(out), self.ptr(ws), self.stream())
        if rc == self.EARG:
            raise ValueError("rejected")
        assert rc == 0
        return self.down(out, 32)

    def proofs(self, leaves, depth, indices, first=0, stride=None):
        idx = np.ascontiguousarray(list(indices), dtype=np.uint64)
        row = 32 * depth if depth <= 64 else 0
        stride = row if stride is None else stride
        d_leaves, d_idx = self.up(b"".join(leaves)), self.up(idx.tobytes())
        ws = self.filled(self.L.bls381_merkle_proofs_workspace_size(len(leaves), first, depth))
        out, root = self.filled(stride * len(idx)), self.filled(32)
        rc = self.L.bls381_merkle_proofs_device(len(leaves), self.ptr(d_leaves), first, depth, len(idx),
                                                self.ptr(d_idx), self.ptr(out), stride, self.ptr(root), self.ptr(ws),
                                                self.stream())
        if rc == self.EARG:
            raise ValueError("rejected")
        assert rc == 0
        self.last_rows = self.down(out, stride * len(idx))
        return [self.last_rows[stride * k:stride * k + row] for k in range(len(idx))], self.down(root, 32)


@pytest.fixture(scope="module", params=["host_pointer", "device"])
def eng(request, native, ssz):
    return HostPointerEngine(ssz) if request.param == "host_pointer" else DeviceEngine(native)


@pytest.fixture(scope="module")
def dev(native):
    return DeviceEngine(native)


# ---------------------------------------------------------------- the fixture
@pytest.mark.parametrize("t", FX["trees"], ids=lambda t: "n%d" % t["n"])
def test_fixture_trees(eng, t):
    C.check_fixture_tree(eng, t)


@pytest.mark.parametrize("t", FX["large"], ids=lambda t: "n%d" % t["n"])
def test_fixture_large(eng, t):
    C.check_fixture_large(eng, t)


def test_fixture_windows_and_empty(eng):
    for t in FX["windows"]:
        C.check_fixture_window(eng, t)
    C.check_fixture_empty(eng, FX)


# ------------------------------------------------------------ tile boundaries
@pytest.mark.parametrize("n", C.tile_sizes(W)[0])
def test_tile_boundary_sizes(eng, n):
    assert C.tile_sizes(W)[1] == []          # W^2 + 1 <= 2^20: no size is left out
    C.check_tile_size(eng, n)


@pytest.mark.parametrize("window", C.tile_windows(W), ids=lambda w: "first%d_n%d" % w)
def test_windows_that_straddle_a_tile(eng, window):
    C.check_tile_window(eng, *window)


def test_depth_edges(eng):
    C.check_depth_edges(eng, W)


def test_rejected_shapes(eng):
    C.check_rejected(eng)


def test_length_mix(eng):
    C.check_length_mix(eng)


def test_bad_arguments(native, dev):
    L, EARG = native.lib(), native.EARG
    leaf = C.leaves(0, 1)[0]
    out = ctypes.create_string_buffer(32)
    idx = np.zeros(1, dtype=np.uint64)
    ip = idx.ctypes.data_as(ctypes.c_void_p)
    proofs = ctypes.create_string_buffer(1024)
    assert L.bls381_merkle_root(1, None, 0, 32, 0, 0, out) == EARG
    assert L.bls381_merkle_root(1, leaf, 0, 32, 0, 0, None) == EARG
    assert L.bls381_merkle_root(2 ** 31, leaf, 0, 32, 0, 0, out) == EARG
    assert L.bls381_merkle_root(0, None, 0, 32, 0, 0, out) == 0 and out.raw == M.Z[32]
    assert L.bls381_merkle_proofs(1, leaf, 0, 32, 1, None, proofs, 1024, out) == EARG
    assert L.bls381_merkle_proofs(1, leaf, 0, 32, 1, ip, None, 1024, out) == EARG
    assert L.bls381_merkle_proofs(1, leaf, 0, 32, 1, ip, proofs, 1023, out) == EARG
    assert L.bls381_merkle_proofs(1, leaf, 0, 32, 1, ip, proofs, 1024, None) == EARG
    assert L.bls381_merkle_proofs(1, leaf, 0, 32, 1, ip, proofs, 1024, out) == 0
    assert out.raw == M.Tree([leaf], 0, 32).root
    assert L.bls381_merkle_proofs(1, leaf, 0, 0, 1, ip, None, 0, out) == 0 and out.raw == leaf      # depth 0: no proofs
    assert L.bls381_merkle_root_workspace_size(9, 0, 3) == 0 == L.bls381_merkle_proofs_workspace_size(1, 0, 65)
    # device forms: NULL workspace / root / leaves, misaligned leaves, proofs, stride and indices
    d_leaf, ws, d_out, d_idx = dev.up(leaf * 2), dev.filled(1 << 16), dev.filled(2048), dev.up(bytes(16))
    p, s = dev.ptr, dev.stream()
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    assert L.bls381_merkle_root_device(1, p(d_leaf), 0, 32, 0, 0, p(d_out), None, s) == EARG
    assert L.bls381_merkle_root_device(1, p(d_leaf), 0, 32, 0, 0, None, p(ws), s) == EARG
    assert L.bls381_merkle_root_device(1, None, 0, 32, 0, 0, p(d_out), p(ws), s) == EARG
    assert L.bls381_merkle_root_device(1, off(d_leaf, 1), 0, 32, 0, 0, p(d_out), p(ws), s) == EARG
    args = lambda lv, ix, pr, st: (1, lv, 0, 32, 1, ix, pr, st, off(d_out, 1024), p(ws), s)
    assert L.bls381_merkle_proofs_device(*args(p(d_leaf), p(d_idx), off(d_out, 2), 1024)) == EARG
    assert L.bls381_merkle_proofs_device(*args(p(d_leaf), p(d_idx), p(d_out), 1026)) == EARG
    assert L.bls381_merkle_proofs_device(*args(p(d_leaf), off(d_idx, 4), p(d_out), 1024)) == EARG
    assert L.bls381_merkle_proofs_device(*args(p(d_leaf), p(d_idx), p(d_out), 1024)) == 0
    assert dev.down(d_out, 2048)[1024:1056] == M.Tree([leaf], 0, 32).root
    assert L.bls381_ssz_list_root(1, leaf, 32, None, 0, 1, out) == EARG
    assert L.bls381_deposits_build(1, None, 0, proofs, out) == EARG
    assert L.bls381_deposits_build(1, bytes(184), 2 ** 32, ctypes.create_string_buffer(1208), out) == EARG
    assert L.bls381_deposits_build(0, None, 0, None, out) == 0 and out.raw == M.Z[32]
    assert L.bls381_deposits_build_workspace_size(2 ** 31) == 0 == L.bls381_ssz_list_root_workspace_size(2 ** 31)


# --------------------------------------------------------------------- proofs
def test_every_proof_of_a_tile_and_one_leaf(native, ssz, dev):
    """n = W + 1, all n indices: the output by digest, the 184 bytes behind each proof in a
    1,208-byte row untouched (host-pointer and device form), and every proof through
    verify_merkle_branch_batch -- accepted as it is, refused with one bit flipped."""
    n = W + 1
    lv = C.leaves(C.TILE_ID, n)
    m = C.model(C.TILE_ID, n, 0, 32)
    want = [b"".join(m.proof(i)) for i in range(n)]
    proofs, root = ssz.merkle_proofs(lv, 32, range(n))
    assert root == m.root and C.sha(proofs) == C.sha(want)
    wide, root = dev.proofs(lv, 32, range(n), stride=1208)
    assert root == m.root and C.sha(wide) == C.sha(want)
    assert all(dev.last_rows[1208 * k + 1024:1208 * (k + 1)] == b"\xEE" * 184 for k in range(n))
    rows = ctypes.create_string_buffer(b"\xEE" * (1208 * n), 1208 * n)
    idx = np.arange(n, dtype=np.uint64)
    out = ctypes.create_string_buffer(32)
    assert native.lib().bls381_merkle_proofs(n, b"".join(lv), 0, 32, n, idx.ctypes.data_as(ctypes.c_void_p), rows, 1208,
                                             out) == 0
    assert out.raw == m.root
    raw = rows.raw
    assert all(raw[1208 * k:1208 * k + 1024] == want[k] and raw[1208 * k + 1024:1208 * (k + 1)] == b"\xEE" * 184
               for k in range(n))
    assert ssz.verify_merkle_branch_batch(lv, proofs, 32, range(n), root).all()
    bad = [D.flip(p, (37 * k + 5) % (8 * 1024)) for k, p in enumerate(proofs)]
    assert not ssz.verify_merkle_branch_batch(lv, bad, 32, range(n), root).any()


# ------------------------------------------------------------- build_deposits
N_DEP = 257


def _unpack(d: bytes) -> dict:
    return {"pubkey": d[:48], "withdrawal_credentials": d[48:80], "amount": int.from_bytes(d[80:88], "little"),
            "signature": d[88:]}


@pytest.fixture(scope="module")
def deposit_datas(native):
    """257 DepositData of 257 new keys, each signed over its signing root; built once."""
    rng = random.Random(0xB15_0010)
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


@pytest.mark.parametrize("first_index", [0, 2 ** 31 + 7])
@pytest.mark.parametrize("n", [1, 5, N_DEP])
def test_build_deposits(native, ssz, dev, deposit_datas, n, first_index):
    from bls381_amd.registry import PubkeyRegistry
    datas, leaves = deposit_datas[0][:n], deposit_datas[1][:n]
    tree = D.SparseTree({first_index + i: leaf for i, leaf in enumerate(leaves)})
    want = [b"".join(tree.proof(first_index + i)) + d for i, d in enumerate(datas)]
    deposits, root = ssz.build_deposits(datas, first_index)
    assert root == tree.root and deposits == want
    # the device form: the same bytes, nothing behind them
    L = native.lib()
    d_data, ws = dev.up(b"".join(datas)), dev.filled(L.bls381_deposits_build_workspace_size(n))
    d_dep, d_root = dev.filled(1208 * n), dev.filled(32)
    assert L.bls381_deposits_build_device(n, dev.ptr(d_data), first_index, dev.ptr(d_dep), dev.ptr(d_root),
                                          dev.ptr(ws), dev.stream()) == 0
    assert dev.down(d_dep, 1208 * n) == b"".join(want) and dev.down(d_root, 32) == tree.root
    # what process_deposit makes of them
    reg = PubkeyRegistry(1024)
    res = reg.process_deposits(deposits, first_index, root, DOMAIN, commit=False)
    assert res.first_bad_proof == -1 and list(res.outcome) == [D.NEW] * n and res.n_new == n
    res = reg.process_deposits(deposits, first_index, D.flip(root, 77), DOMAIN, commit=False)
    assert res.first_bad_proof == 0


# ----------------------------------------------------------------- list roots
def _value(typ, rng):
    k = typ[0]
    if k == "uint":
        return rng.randrange(256 ** typ[1])
    if k == "bool":
        return rng.random() < 0.5
    if k == "bytes":
        return rng.randbytes(typ[1])
    if k == "vector":
        return [_value(typ[1], rng) for _ in range(typ[2])]
    if k == "list":
        raise AssertionError("lists are given sizes by the caller")
    return {name: _value(t, rng) for name, t in typ[1]}


@pytest.mark.parametrize("n", [0, 1, 2, 3, 257])
def test_list_of_validators(native, ssz, dev, n):
    rng = random.Random(0xB15_0011 + n)
    typ = ssz.List(ssz.Validator)
    vals = [_value(ssz.Validator, rng) for _ in range(n)]
    want = M.hash_tree_root(typ, vals)
    assert ssz.hash_tree_root(typ, vals) == want
    # the device form, items 128 bytes apart (121-byte Validators), as a Vector too
    L = native.lib()
    size, stride = ssz.item_size(ssz.Validator), 128
    assert size == 121
    blob = b"".join(ssz.serialize(ssz.Validator, v).ljust(stride, b"\xAA") for v in vals)
    prog = ssz.compile_root(ssz.Validator)
    d_items, ws = dev.up(blob), dev.filled(L.bls381_ssz_list_root_workspace_size(n))
    for mix in (1, 0):
        out = dev.filled(32)
        assert L.bls381_ssz_list_root_device(n, dev.ptr(d_items), stride, size, prog.ctypes.data_as(ctypes.c_void_p),
                                             len(prog), mix, dev.ptr(out), dev.ptr(ws), dev.stream()) == 0
        roots = [M.hash_tree_root(ssz.Validator, v) for v in vals]
        assert dev.down(out, 32) == (want if mix else M.merkleize_chunks(roots))


@pytest.mark.parametrize("n", [0, 1, 4, 5, 1025])
def test_list_of_uint64(ssz, n):
    rng = random.Random(0xB15_0012 + n)
    vals = [rng.randrange(2 ** 64) for _ in range(n)]
    assert ssz.hash_tree_root(ssz.List(ssz.uint(8)), vals) == M.hash_tree_root(M.List(("uint", 8)), vals)


@pytest.mark.parametrize("n", [0, 1, 32, 33])
def test_bytes(ssz, n):
    v = random.Random(0xB15_0013 + n).randbytes(n)
    assert ssz.hash_tree_root(ssz.BYTES, v) == M.hash_tree_root(M.BYTES, v)


def test_large_vectors(ssz):
    rng = random.Random(0xB15_0014)
    for typ in (ssz.Vector(ssz.Bytes(32), 8192), ssz.Vector(ssz.Crosslink, 1024)):
        v = _value(typ, rng)
        assert ssz.hash_tree_root(typ, v) == M.hash_tree_root(typ, v)


def test_mixed_container(ssz):
    """Fixed fields, a List(Validator), a List(uint64), a list of a container that holds `bytes`
    (the slow path) and a vector beyond the 64-chunk stack, through hash_tree_root and signing_root."""
    rng = random.Random(0xB15_0015)
    inner = ssz.Container(("bits", ssz.BYTES), ("data", ssz.Crosslink))
    typ = ssz.Container(("slot", ssz.uint(8)), ("fork", ssz.Fork), ("registry", ssz.List(ssz.Validator)),
                        ("balances", ssz.List(ssz.uint(8))), ("attestations", ssz.List(inner)),
                        ("roots", ssz.Vector(ssz.Bytes(32), 128)), ("eth1", ssz.Eth1Data),
                        ("signature", ssz.Bytes(96)))
    v = {"slot": 12345, "fork": _value(ssz.Fork, rng), "registry": [_value(ssz.Validator, rng) for _ in range(70)],
         "balances": [rng.randrange(2 ** 64) for _ in range(70)],
         "attestations": [{"bits": rng.randbytes(k), "data": _value(ssz.Crosslink, rng)} for k in (0, 5, 40)],
         "roots": [rng.randbytes(32) for _ in range(128)], "eth1": _value(ssz.Eth1Data, rng),
         "signature": rng.randbytes(96)}
    assert ssz.hash_tree_root(typ, v) == M.hash_tree_root(typ, v)
    assert ssz.signing_root(typ, v) == M.signing_root(typ, v)
    assert ssz.signing_root(typ, v) != ssz.hash_tree_root(typ, v)
    # the predefined containers, as values
    for t in (ssz.Validator, ssz.Eth1Data, ssz.Fork, ssz.VoluntaryExit, ssz.Transfer, ssz.ProposerSlashing):
        x = _value(t, rng)
        assert ssz.hash_tree_root(t, x) == M.hash_tree_root(t, x)
    for t in (ssz.VoluntaryExit, ssz.Transfer, ssz.BeaconBlockHeader):
        x = _value(t, rng)
        assert ssz.signing_root(t, x) == M.signing_root(t, x)


def test_fixed_size_batches_are_what_they_were(ssz):
    """hash_tree_root_batch / signing_root_batch on the types that existed before: the oracle's bytes."""
    rng = random.Random(0xB15_0016)
    for name in ("Crosslink", "AttestationData", "AttestationDataAndCustodyBit", "DepositData", "BeaconBlockHeader"):
        typ, otyp = getattr(ssz, name), getattr(S, name)
        vals = [_value(typ, rng) for _ in range(5)]
        blobs = [ssz.serialize(typ, v) for v in vals]
        assert blobs == [S.serialize(otyp, v) for v in vals]
        assert ssz.hash_tree_root_batch(typ, blobs) == [S.hash_tree_root(otyp, v) for v in vals]
        if name in ("DepositData", "BeaconBlockHeader"):
            assert ssz.signing_root_batch(typ, blobs) == [S.signing_root(otyp, v) for v in vals]
