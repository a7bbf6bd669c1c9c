"""verify_merkle_branch on the CPU: the fold the kernel runs (csrc/bls381_ssz.hpp
merkle_branch_root, host build) against tests/golden/deposit_tree.json (the reference's
merkle_minimal.py) and against the spec's loop restated in deposit_model.py; the deposit leaf
program and the Deposit container.  GPU half: test_process_deposits.py."""
import ctypes
import os

import numpy as np
import pytest

import deposit_model as M
from bls381_amd import ssz


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_merkle_branch.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64,
                                     ctypes.c_char_p]
    lib.hc_merkle_branch.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def trees():
    return M.fixture()


def hc(L, leaf, proof, depth, index, root):
    return L.hc_merkle_branch(leaf, b"".join(proof) + b"\x00", depth, index, root)


def test_fixture_proofs_verify(L, trees):
    assert [len(t["leaves"]) for t in trees] == [1, 2, 5, 8]
    for t in trees:
        for i, (leaf, proof) in enumerate(zip(t["leaves"], t["proofs"])):
            assert len(proof) == 32
            assert M.verify_merkle_branch(leaf, proof, 32, i, t["root"])      # the model reads the fixture alike
            assert hc(L, leaf, proof, 32, i, t["root"]) == 1


def test_fixture_proofs_one_bit_off(L, trees):
    for t in trees:
        for i, (leaf, proof) in enumerate(zip(t["leaves"], t["proofs"])):
            bit = (37 * i + 5) % 256
            assert hc(L, M.flip(leaf, bit), proof, 32, i, t["root"]) == 0
            assert hc(L, leaf, [M.flip(proof[0], bit)] + proof[1:], 32, i, t["root"]) == 0
            assert hc(L, leaf, proof[:31] + [M.flip(proof[31], bit)], 32, i, t["root"]) == 0
            assert hc(L, leaf, proof, 32, i, M.flip(t["root"], bit)) == 0


def test_fixture_proofs_wrong_index(L, trees):
    for t in trees:
        for i, (leaf, proof) in enumerate(zip(t["leaves"], t["proofs"])):
            assert hc(L, leaf, proof, 32, i ^ 1, t["root"]) == 0
            assert hc(L, leaf, proof, 32, i ^ (1 << 31), t["root"]) == 0
            assert hc(L, leaf, proof, 32, i ^ (1 << 32), t["root"]) == 1      # bits past the depth are not read


def test_synthetic_branches(L):
    cases = M.synthetic_cases()
    assert sorted({c[2] for c in cases}) == [0, 1, 5, 33, 64]
    for leaf, proof, depth, index, root in cases:
        assert hc(L, leaf, proof, depth, index, root) == 1, (depth, index)
        assert hc(L, leaf, proof, depth, index, M.flip(root, 200)) == 0
        if depth:
            assert hc(L, leaf, proof, depth, index ^ (1 << (depth - 1)), root) == 0, (depth, index)
    leaf = b"\x07" * 32
    assert hc(L, leaf, [], 0, 2 ** 64 - 1, leaf) == 1                          # depth 0: the leaf is the root


def test_sparse_tree_builder_matches_fixture(trees):
    for t in trees:
        tree = M.SparseTree(dict(enumerate(t["leaves"])))
        assert tree.root == t["root"]
        assert [tree.proof(i) for i in range(len(t["leaves"]))] == t["proofs"]


def test_deposit_root_program_is_the_engines(L):
    # csrc/bls381_plan.hpp DEPOSIT_ROOT_PROG == the compiler's hash_tree_root(DepositData)
    want = [1, 0, 32, 1, 32, 16, 2, 2, 1, 48, 32, 1, 80, 8, 1, 88, 32, 1, 120, 32, 1, 152, 32, 2, 3, 2, 4]
    assert list(ssz.compile_root(ssz.DepositData, False)) == want
    buf = (ctypes.c_uint32 * 512)()
    size = ctypes.c_size_t(0)
    L.hc_deposit_root_prog.restype = ctypes.c_uint32
    n = L.hc_deposit_root_prog(buf, ctypes.byref(size))
    assert list(buf[:n]) == want
    assert size.value == 1208 == ssz.item_size(ssz.Deposit)


def test_deposit_container(L):
    assert ssz.item_size(ssz.Deposit) == 1208
    data = {"pubkey": bytes(range(48)), "withdrawal_credentials": b"\x01" * 32, "amount": 32 * 10 ** 9,
            "signature": bytes(range(96))}
    proof = [bytes([k]) * 32 for k in range(32)]
    ser = ssz.serialize(ssz.Deposit, {"proof": proof, "data": data})
    assert ser == b"".join(proof) + ssz.serialize(ssz.DepositData, data) and len(ser) == 1208
    with pytest.raises(ValueError):
        ssz.serialize(ssz.Deposit, {"proof": proof[:31], "data": data})
    # hash_tree_root(Deposit) through the host interpreter == merkleize([merkleize(proof), root(data)])
    import ssz_oracle as S
    prog = ssz.compile_root(ssz.Deposit, False)
    buf = ctypes.create_string_buffer(32)
    assert L.hc_ssz_root(ser, prog.ctypes.data_as(ctypes.c_void_p), len(prog), buf) == 1
    want = S.merkleize_chunks([S.merkleize_chunks(proof), S.hash_tree_root(S.DepositData, data)])
    assert buf.raw == want
    packed = ssz.Vector(ssz.uint(8), 5)                                        # basic elements are packed
    assert list(ssz.compile_root(packed)) == [1, 0, 32, 1, 32, 8, 2, 2]
    assert ssz.serialize(packed, [1, 2, 3, 4, 5]) == b"".join(int(x).to_bytes(8, "little") for x in (1, 2, 3, 4, 5))
