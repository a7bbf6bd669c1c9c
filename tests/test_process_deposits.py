"""process_deposit on the device: verify_merkle_branch batches against the spec's
fold restated in deposit_model.py, and PubkeyRegistry.process_deposits against the spec's
process_deposit loop restated there (signature verdicts known by construction, three of them
spot-checked with the oracle).  CPU half: test_merkle_branch_host.py."""
import ctypes
import random

import numpy as np
import pytest

import bls_oracle as O
import deposit_model as M
import ssz_oracle as S

pytestmark = pytest.mark.gpu

DOMAIN = 3
FIRST = 2 ** 31 - 3          # the batch's indices carry across bit 31
N_REG = 10                   # keys in the registry before the batch
VALID, TAMPERED, ZERO = "valid", "tampered", "zero"


# ------------------------------------------------ verify_merkle_branch_batch
def _corrupt(rng, leaf, proof, depth, index, root, per_item_root):
    """One corruption of an item; what it does to the verdict is the model's to say."""
    kinds = ["leaf"] + (["sibling", "index"] if depth else []) + (["root"] if per_item_root else [])
    kind = rng.choice(kinds)
    bit = rng.randrange(256)
    if kind == "leaf":
        leaf = M.flip(leaf, bit)
    elif kind == "sibling":
        k = rng.randrange(depth)
        proof = proof[:k] + [M.flip(proof[k], bit)] + proof[k + 1:]
    elif kind == "index":
        index ^= 1 << rng.randrange(depth)
    else:
        root = M.flip(root, bit)
    return leaf, proof, index, root


def _run_branch_batch(items, depth, single_root=None):
    from bls381_amd import ssz
    want = [M.verify_merkle_branch(l, p, depth, i, single_root or r) for l, p, i, r in items]
    got = ssz.verify_merkle_branch_batch([x[0] for x in items], [x[1] for x in items], depth,
                                         [x[2] for x in items], single_root or [x[3] for x in items])
    assert got.dtype == bool and list(got) == want
    return want


def test_merkle_branch_batch_fixture_proofs(native):
    """Depth 32, 304 items (three workgroups of 128): per-item roots over all four fixture trees,
    then one root for all over the 8-leaf tree; a third of the items corrupted."""
    trees = M.fixture()
    rng = random.Random(0xB15_000B)
    base = [(t["leaves"][i], t["proofs"][i], i, t["root"]) for t in trees for i in range(len(t["leaves"]))]
    assert len(base) == 16
    for single in (False, True):
        src = [b for b in base if b[3] == trees[3]["root"]] if single else base
        items = []
        for k in range(304):
            leaf, proof, index, root = src[k % len(src)]
            if k % 3 == 1:
                leaf, proof, index, root = _corrupt(rng, leaf, proof, 32, index, root, not single)
            items.append((leaf, proof, index, root))
        want = _run_branch_batch(items, 32, trees[3]["root"] if single else None)
        assert want.count(True) == 304 - 101 and not any(want[1::3])
    assert _run_branch_batch(base[:1], 32) == [True]                           # n == 1
    assert _run_branch_batch([(M.flip(base[0][0], 0),) + base[0][1:]], 32, base[0][3]) == [False]


@pytest.mark.parametrize("depth", M.SYNTH_DEPTHS)
def test_merkle_branch_batch_synthetic(native, depth):
    """Depths 0, 1, 5, 33, 64 with indices up to 2^64 - 1: 300 items per call, a third corrupted."""
    rng = random.Random(0xB15_000C + depth)
    items = []
    for k in range(300):
        leaf = rng.randbytes(32)
        proof = [rng.randbytes(32) for _ in range(depth)]
        index = M.SYNTH_INDICES[k % 4] if k < 200 else rng.randrange(2 ** 64)
        root = M.branch_root(leaf, proof, depth, index)
        if k % 3 == 1:
            leaf, proof, index, root = _corrupt(rng, leaf, proof, depth, index, root, True)
        items.append((leaf, proof, index, root))
    want = _run_branch_batch(items, depth)
    assert want.count(True) == 200
    for case in M.synthetic_cases():                                           # the CPU suite's cases, one by one root
        if case[2] == depth:
            assert _run_branch_batch([(case[0], case[1], case[3], case[4])], depth, case[4]) == [True]


def test_merkle_branch_batch_bad_arguments(native):
    from bls381_amd import ssz
    L = native.lib()
    leaf, idx, ok = b"\x01" * 32, np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
    ip, op = idx.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p)
    proof = b"\x02" * (32 * 65)
    assert L.bls381_merkle_branch_batch(1, leaf, proof, 64, ip, leaf, 0, op) == 0
    assert L.bls381_merkle_branch_batch(1, leaf, proof, 65, ip, leaf, 0, op) == native.EARG
    assert L.bls381_merkle_branch_batch(1, leaf, proof, 1, ip, leaf, 16, op) == native.EARG
    assert L.bls381_merkle_branch_batch(1, leaf, proof, 1, ip, leaf, 64, op) == native.EARG
    for args in ((None, proof, 1, ip, leaf, 0, op), (leaf, None, 1, ip, leaf, 0, op), (leaf, proof, 1, None, leaf, 0, op),
                 (leaf, proof, 1, ip, None, 0, op), (leaf, proof, 1, ip, leaf, 0, None)):
        assert L.bls381_merkle_branch_batch(1, *args) == native.EARG
    assert L.bls381_merkle_branch_batch(0, None, None, 1, None, None, 0, None) == 0
    assert L.bls381_merkle_branch_batch_device(1, None, None, 1, None, None, 0, None, None) == native.EARG
    assert L.bls381_merkle_branch_batch_device(1, leaf, proof, 65, ip, leaf, 0, op, None) == native.EARG
    with pytest.raises(ValueError):
        ssz.verify_merkle_branch_batch([leaf], [[leaf] * 65], 65, [0], leaf)
    assert list(ssz.verify_merkle_branch_batch([], [], 32, [], leaf)) == []


# ------------------------------------------------------------ process_deposits
def _leaf(data184: bytes) -> bytes:
    return S.hash_tree_root(S.DepositData, _unpack(data184))


def _unpack(d: bytes) -> dict:
    return {"pubkey": d[:48], "withdrawal_credentials": d[48:80], "amount": int.from_bytes(d[80:88], "little"),
            "signature": d[88:]}


def _with_proofs(datas, first_index, extra_leaves=None):
    """Serialized Deposits for `datas` at tree indices first_index + i, and the tree's root."""
    leaves = dict(extra_leaves or {})
    leaves.update({first_index + i: _leaf(d) for i, d in enumerate(datas)})
    tree = M.SparseTree(leaves)
    return [b"".join(tree.proof(first_index + i)) + d for i, d in enumerate(datas)], tree.root, leaves


class Batch:
    pass


@pytest.fixture(scope="module")
def batch(native, golden):
    """300 deposits from 41 signers (10 of them registered) and one undecodable key, built once."""
    _, gb = golden
    rng = random.Random(0xB15_000D)
    sks = [rng.randrange(1, 1 << 250) for _ in range(41)]
    pks_blob = native.privtopub_batch(b"".join(k.to_bytes(32, "big") for k in sks))
    pks = [pks_blob[48 * i:48 * i + 48] for i in range(41)]
    bad_key = bytes.fromhex(gb["invalid_g1"][0])
    n = 300
    # (signer, mode) per position; signers 0-9 are registered, 10-14 carry the cases below, 15-40 fill
    plan = [None] * n
    special = {0: (0, VALID), 1: (1, ZERO),                    # registered keys: TOPUP whatever the signature
               2: (10, VALID),                                  # NEW
               3: (11, TAMPERED),                               # SKIPPED
               4: (12, VALID), 9: (12, VALID),                  # NEW, TOPUP
               5: (14, VALID), 250: (14, VALID),                # NEW, TOPUP more than a workgroup apart
               6: (13, TAMPERED), 7: (13, VALID), 8: (13, ZERO),   # SKIPPED, NEW, TOPUP
               10: ("bad", ZERO)}                               # undecodable pubkey: SKIPPED
    for pos, what in special.items():
        plan[pos] = what
    for pos in range(n):
        if plan[pos] is None:
            signer = rng.randrange(10) if rng.random() < 0.3 else rng.randrange(15, 41)
            plan[pos] = (signer, rng.choice([VALID, VALID, TAMPERED, ZERO]))
    values, roots = [], []
    for pos, (signer, mode) in enumerate(plan):
        v = {"pubkey": bad_key if signer == "bad" else pks[signer], "withdrawal_credentials": rng.randbytes(32),
             "amount": 32 * 10 ** 9 + pos, "signature": b"\x00" * 96}
        values.append(v)
        roots.append(S.signing_root(S.DepositData, v))
    sigs = native.sign_batch(b"".join(roots), b"".join((sks[s] if s != "bad" else 1).to_bytes(32, "big")
                                                       for s, _ in plan), DOMAIN.to_bytes(8, "big") * n)
    datas, sig_ok = [], []
    for pos, (signer, mode) in enumerate(plan):
        v = values[pos]
        if mode != ZERO:
            v["signature"] = sigs[96 * pos:96 * pos + 96]
        if mode == TAMPERED:
            v["amount"] += 1                                    # signed data changed
        datas.append(S.serialize(S.DepositData, v))
        sig_ok.append(mode == VALID and signer != "bad")
    for k in (2, 3, 8):                                         # the oracle's own verify on a valid, a tampered, a zero one
        v = _unpack(datas[k])
        assert O.verify(S.signing_root(S.DepositData, v), v["pubkey"], v["signature"], DOMAIN) == sig_ok[k]
    b = Batch()
    b.n, b.pks, b.datas, b.sig_ok, b.plan = n, pks, datas, sig_ok, plan
    b.deposits, b.root, b.leaves = _with_proofs(datas, FIRST)
    b.model = M.process_deposits_model(pks[:N_REG], b.deposits, sig_ok, FIRST, b.root, _leaf)
    return b


def _registry(batch, capacity=1024):
    from bls381_amd.registry import PubkeyRegistry
    reg = PubkeyRegistry(capacity)
    assert list(reg.add(batch.pks[:N_REG])) == list(range(N_REG))
    return reg


def _assert_result(res, model):
    outcome, vidx, bad, n_new = model
    assert list(res.outcome) == outcome
    assert list(res.validator_index) == vidx
    assert res.first_bad_proof == bad
    assert res.n_new == n_new


def test_model_covers_the_cases(batch):
    """The model itself, on the cases the batch was built around (no engine call)."""
    outcome, vidx, bad, n_new = batch.model
    assert bad == -1
    assert [outcome[k] for k in (0, 1)] == [M.TOPUP, M.TOPUP] and vidx[:2] == [0, 1]
    assert outcome[2] == M.NEW and vidx[2] == N_REG
    assert outcome[3] == M.SKIPPED and vidx[3] == -1
    assert (outcome[4], outcome[9]) == (M.NEW, M.TOPUP) and vidx[9] == vidx[4]
    assert (outcome[5], outcome[250]) == (M.NEW, M.TOPUP) and vidx[250] == vidx[5]
    assert outcome[6:9] == [M.SKIPPED, M.NEW, M.TOPUP] and vidx[8] == vidx[7]
    assert outcome[10] == M.SKIPPED
    assert n_new >= 10 and outcome.count(M.SKIPPED) >= 10 and outcome.count(M.TOPUP) >= 100


def test_process_deposits_commit_and_replay(native, batch):
    reg = _registry(batch)
    res = reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN)
    _assert_result(res, batch.model)
    outcome, vidx, _, n_new = batch.model
    assert len(reg) == N_REG + n_new
    new_pos = [i for i in range(batch.n) if outcome[i] == M.NEW]
    new_keys = [batch.datas[i][:48] for i in new_pos]
    new_entries = [vidx[i] for i in new_pos]
    assert new_entries == list(range(N_REG, N_REG + n_new))
    assert list(reg.lookup(new_keys)) == new_entries
    assert reg.aggregate_indices([new_entries])[0] == O.aggregate_pubkeys(new_keys)   # the appended points are decoded
    # the same data again at the next indices: every key that was NEW is now a validator
    deposits2, root2, _ = _with_proofs(batch.datas, FIRST + batch.n, batch.leaves)
    model2 = M.process_deposits_model(batch.pks[:N_REG] + new_keys, deposits2, batch.sig_ok, FIRST + batch.n, root2,
                                      _leaf)
    res2 = reg.process_deposits(deposits2, FIRST + batch.n, root2, DOMAIN)
    _assert_result(res2, model2)
    assert all(res2.outcome[i] == M.TOPUP and res2.validator_index[i] == vidx[i] for i in new_pos)
    assert res2.n_new == 0 and len(reg) == N_REG + n_new
    reg.close()


def test_process_deposits_without_commit(native, batch):
    reg = _registry(batch)
    res = reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN, commit=False)
    _assert_result(res, batch.model)
    assert len(reg) == N_REG
    new_keys = [batch.datas[i][:48] for i in range(batch.n) if batch.model[0][i] == M.NEW]
    assert list(reg.lookup(new_keys)) == [-1] * len(new_keys)
    assert list(reg.lookup(batch.pks[:N_REG])) == list(range(N_REG))
    reg.close()


def test_process_deposits_bad_proof(native, batch):
    """The spec's assert: the first failing branch is reported and nothing is appended."""
    k = 137
    deposits = list(batch.deposits)
    for pos, sibling in ((k, 3), (200, 31)):
        d = bytearray(deposits[pos])
        d[32 * sibling + 7] ^= 0x10
        deposits[pos] = bytes(d)
    model = M.process_deposits_model(batch.pks[:N_REG], deposits, batch.sig_ok, FIRST, batch.root, _leaf)
    assert model[2] == k and model[:2] == batch.model[:2]
    reg = _registry(batch)
    res = reg.process_deposits(deposits, FIRST, batch.root, DOMAIN, commit=True)
    _assert_result(res, model)
    assert res.first_bad_proof == k
    assert len(reg) == N_REG
    new_keys = [batch.datas[i][:48] for i in range(batch.n) if model[0][i] == M.NEW]
    assert list(reg.lookup(new_keys)) == [-1] * len(new_keys)
    # the right data under the wrong index fails at deposit 0
    res = reg.process_deposits(batch.deposits, FIRST + 1, batch.root, DOMAIN)
    assert res.first_bad_proof == 0 and list(res.outcome) == batch.model[0] and len(reg) == N_REG
    reg.close()


def test_process_deposits_capacity(native, batch):
    n_new = batch.model[3]
    reg = _registry(batch, capacity=N_REG + n_new - 1)
    with pytest.raises(ValueError):
        reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN)
    assert len(reg) == N_REG
    new_keys = [batch.datas[i][:48] for i in range(batch.n) if batch.model[0][i] == M.NEW]
    assert list(reg.lookup(new_keys)) == [-1] * len(new_keys)
    assert list(reg.lookup(batch.pks[:N_REG])) == list(range(N_REG))
    res = reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN, commit=False)   # still usable
    _assert_result(res, batch.model)
    reg.close()
    reg = _registry(batch, capacity=N_REG + n_new)                                         # an exact fit
    _assert_result(reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN), batch.model)
    assert len(reg) == N_REG + n_new
    reg.close()


def test_process_deposits_device_form(native, batch):
    """Device pointers (torch buffers) give what the host form gives on the same batch."""
    import torch
    L = native.lib()
    dev = torch.device("cuda:0")
    n = batch.n
    reg = _registry(batch)
    host = reg.process_deposits(batch.deposits, FIRST, batch.root, DOMAIN, commit=False)
    d_dep = torch.frombuffer(bytearray(b"".join(batch.deposits)), dtype=torch.uint8).to(dev)
    d_out = torch.full((n,), 0xEE, dtype=torch.uint8, device=dev)
    d_vi = torch.full((n,), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(L.bls381_registry_process_deposits_workspace_size(n), dtype=torch.uint8, device=dev)
    bad = ctypes.c_int64(99)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.bls381_registry_process_deposits_device(reg._h, n, d_dep.data_ptr(), FIRST, batch.root,
                                                   DOMAIN.to_bytes(8, "big"), 1, d_out.data_ptr(), d_vi.data_ptr(),
                                                   ctypes.byref(bad), ws.data_ptr(), stream)
    assert rc == host.n_new == batch.model[3] and bad.value == -1
    assert d_out.cpu().tolist() == list(host.outcome) == batch.model[0]
    assert d_vi.cpu().tolist() == list(host.validator_index) == batch.model[1]
    assert len(reg) == N_REG + host.n_new
    # bad arguments
    assert L.bls381_registry_process_deposits_device(reg._h, n, d_dep.data_ptr(), FIRST, batch.root,
                                                     DOMAIN.to_bytes(8, "big"), 1, d_out.data_ptr(), d_vi.data_ptr(),
                                                     ctypes.byref(bad), None, stream) == native.EARG
    assert L.bls381_registry_process_deposits(None, 0, None, 0, None, None, 0, None, None,
                                              ctypes.byref(bad)) == native.EARG
    assert L.bls381_registry_process_deposits(reg._h, 0, None, 0, None, None, 1, None, None, ctypes.byref(bad)) == 0
    assert bad.value == -1 and len(reg) == N_REG + host.n_new
    reg.close()


@pytest.mark.parametrize("policy", ["pyecc", "strict"])
def test_process_deposits_follows_subgroup_policy(native, batch, torsion, policy):
    """Deposits whose pubkey and signature are torsion cases of bls_torsion.json with an infinite
    signature: there the pairing check reads e(H(m), pk) alone, which is 1 for a pubkey of order
    prime to r whatever the message, so the fixture's verdict columns hold for the deposit's own
    signing root -- True under "pyecc" (NEW), False under "strict" (SKIPPED)."""
    cases = {c["kind"]: c for c in torsion["verify"]}
    picked = [cases["pk_T11_sig_inf"], cases["pk_order3_sig_inf"]]
    assert all(c["expected_pyecc"] and not c["expected_strict"] and int(c["domain"]) == DOMAIN for c in picked)
    datas = [S.serialize(S.DepositData, {"pubkey": bytes.fromhex(c["pubkey"]), "withdrawal_credentials": b"\x05" * 32,
                                         "amount": 10 ** 9, "signature": bytes.fromhex(c["signature"])})
             for c in picked] + [batch.datas[2]]
    sig_ok = [c["expected_" + policy] for c in picked] + [True]
    deposits, root, _ = _with_proofs(datas, 0)
    model = M.process_deposits_model(batch.pks[:N_REG], deposits, sig_ok, 0, root, _leaf)
    assert model[0] == ([M.NEW, M.NEW, M.NEW] if policy == "pyecc" else [M.SKIPPED, M.SKIPPED, M.NEW])
    reg = _registry(batch)
    with native.subgroup_policy_scope(policy):
        res = reg.process_deposits(deposits, 0, root, DOMAIN, commit=False)
    _assert_result(res, model)
    reg.close()
