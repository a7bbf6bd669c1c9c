"""The two pubkey tables under crafted hash collisions and duplicates: the registry's
(k_reg_insert / k_reg_lookup) and the batch-local one of process_deposits (k_deposit_insert /
k_deposit_resolve, then k_deposit_scan and k_deposit_compact).  The inputs are
key_table_model.py's seeded cases -- keys with chosen hashes, registrable because a pubkey with
b_flag set is infinity under the "pyecc" policy -- whose probe chains test_key_tables_host.py
checks with the compiled hash.  Expected values: registry_model, deposit_model's
process_deposit loop, and the oracle."""
import random

import pytest

import bls_oracle as O
import deposit_model as M
import key_table_model as K
import ssz_oracle as S

pytestmark = pytest.mark.gpu

DOMAIN, FIRST = K.DOMAIN, K.FIRST


@pytest.fixture(autouse=True)
def pyecc_policy(native):
    old = native.get_subgroup_policy()
    native.set_subgroup_policy("pyecc")
    try:
        yield
    finally:
        native.set_subgroup_policy(old)


def _registry(capacity):
    from bls381_amd.registry import PubkeyRegistry
    return PubkeyRegistry(capacity)


def _run_calls(reg, calls):
    """Every add against registry_model, then every key looked up again: its model entry."""
    want = K.registry_model(calls)
    size = 0
    for call, w in zip(calls, want):
        assert list(reg.add(call)) == w
        size += len(call)
        assert len(reg) == size
    flat = [k for call in calls for k in call]
    assert list(reg.lookup(flat)) == [e for w in want for e in w]
    return want


# ------------------------------------------------------------------ registry
def test_key_tables_registry_one_hash_pile(native):
    c = K.case_pile()
    reg = _registry(c["capacity"])
    assert list(reg.add(c["keys"])) == list(range(1024)) == K.registry_model([c["keys"]])[0]
    assert list(reg.lookup(c["keys"])) == list(range(1024))
    assert list(reg.lookup(c["absent"])) == [-1] * 256        # each walks the whole chain
    mixed = [k for pair in zip(c["absent"], c["keys"][::4]) for k in pair]
    assert list(reg.lookup(mixed)) == [e for i in range(256) for e in (-1, 4 * i)]
    assert len(reg) == 1024
    reg.close()


def test_key_tables_registry_wrap_around(native):
    c = K.case_wrap()
    reg = _registry(c["capacity"])
    assert list(reg.add(c["keys"])) == list(range(64)) == K.registry_model([c["keys"]])[0]
    assert list(reg.lookup(c["keys"])) == list(range(64))
    assert list(reg.lookup(c["absent"])) == [-1] * 64         # from slot mask across the table's end
    assert list(reg.lookup(K.case_pile()["absent"][:8])) == [-1] * 8   # an empty first slot
    reg.close()


def test_key_tables_registry_equal_keys_under_contention(native):
    c = K.case_equal_keys()
    first, second = c["calls"]
    reg = _registry(c["capacity"])
    want = K.registry_model(c["calls"])
    ent = list(reg.add(first))
    assert ent == want[0] == [first.index(k) for k in first]  # every copy: the key's first position
    assert len(reg) == 4096
    ent2 = list(reg.add(second))
    assert ent2 == want[1]
    assert all(e == (first.index(k) if k in first else 4096 + i) for i, (k, e) in enumerate(zip(second, ent2)))
    assert len(reg) == 4096 + 64                              # every appended key counts
    assert list(reg.lookup(first + second)) == want[0] + want[1]
    reg.close()


def test_key_tables_registry_undecodable_keys_in_the_chain(native):
    c = K.case_undecodable()
    reg = _registry(c["capacity"])
    want = K.registry_model([c["keys"]])[0]
    ent = list(reg.add(c["keys"]))
    assert ent == want
    for i, k in enumerate(c["keys"]):                         # the model, spelled out
        assert ent[i] == (-1 if k in c["bad"] else i)
    assert len(reg) == len(c["keys"])                         # bad keys consume entries
    assert list(reg.lookup(c["keys"])) == want
    assert list(reg.lookup(c["bad"])) == [-1] * 3
    ent2 = list(reg.add(c["bad"] + c["keys"][:5]))            # added again: still no entry, and no shadow
    assert ent2 == [-1] * 3 + want[:5] and len(reg) == len(c["keys"]) + 8
    reg.close()


def test_key_tables_registry_decoded_points_among_collisions(native):
    honest_blob = native.privtopub_batch(b"".join(sk.to_bytes(32, "big") for sk in K.HONEST_SKS))
    honest = [honest_blob[48 * i:48 * i + 48] for i in range(40)]
    assert [honest[i] for i in (0, 17, 39)] == [O.privtopub(K.HONEST_SKS[i]) for i in (0, 17, 39)]
    c = K.case_decoded(honest)
    reg = _registry(c["capacity"])
    want = _run_calls(reg, [c["keys"]])[0]
    assert want == list(range(360))
    pos = c["honest_pos"]
    rng = random.Random(0xB15_3001)
    crafted = [i for i in range(360) if i not in pos]
    groups, members = [], []
    for g in range(8):                                        # honest and crafted entries mixed
        hs = rng.sample(range(40), 5 + 4 * g)
        idx = [pos[h] for h in hs] + rng.sample(crafted, 20)
        rng.shuffle(idx)
        groups.append(idx)
        members.append(hs)
    groups += [list(range(360)), crafted[:40], [pos[3] - 1, pos[3], pos[3] + 1]]
    members += [list(range(40)), [], [3]]
    got = reg.aggregate_indices(groups)
    for hs, out in zip(members, got):                         # infinity contributes nothing
        assert out == O.aggregate_pubkeys([honest[h] for h in hs])
    reg.close()


@pytest.mark.parametrize("capacity", [1, 3, 128])
def test_key_tables_registry_filled_exactly(native, capacity):
    keys = K.case_exact_fill(capacity)
    reg = _registry(capacity)
    _run_calls(reg, [keys[:capacity // 2], keys[capacity // 2:]] if capacity > 1 else [keys])
    assert len(reg) == capacity
    with pytest.raises(ValueError):
        reg.add([K.craft_key(b"\x40" * 44, 5)])
    assert len(reg) == capacity and list(reg.lookup(keys)) == list(range(capacity))
    reg.close()


def test_key_tables_registry_growth(native):
    c = K.case_growth()
    reg = _registry(c["capacity"])
    want = _run_calls(reg, c["calls"])
    assert len(reg) == c["capacity"]
    with pytest.raises(ValueError):                           # one more key on a full registry
        reg.add([c["extra"]])
    assert len(reg) == c["capacity"]
    flat = [k for call in c["calls"] for k in call]
    assert list(reg.lookup(flat + [c["extra"]])) == [e for w in want for e in w] + [-1]
    reg.close()


# ------------------------------------------------------------------ deposits
def _unpack(d: bytes) -> dict:
    return {"pubkey": d[:48], "withdrawal_credentials": d[48:80], "amount": int.from_bytes(d[80:88], "little"),
            "signature": d[88:]}


def _leaf(data184: bytes) -> bytes:
    return S.hash_tree_root(S.DepositData, _unpack(data184))


def _with_proofs(datas, first_index, extra_leaves=None):
    leaves = dict(extra_leaves or {})
    leaves.update({first_index + i: _leaf(d) for i, d in enumerate(datas)})
    tree = M.SparseTree(leaves)
    return [b"".join(tree.proof(first_index + i)) + d for i, d in enumerate(datas)], tree.root, leaves


def _oracle_spot_check(datas, sig_ok):
    """The oracle's verify on a good signature without junk, a bad one and a good one with junk."""
    plain = next(i for i, d in enumerate(datas) if sig_ok[i] and not any(d[89:]))
    junk = next(i for i, d in enumerate(datas) if sig_ok[i] and any(d[89:]))
    picks = [plain, junk] + ([sig_ok.index(False)] if False in sig_ok else [])
    for i in picks:
        v = _unpack(datas[i])
        assert O.verify(S.signing_root(S.DepositData, v), v["pubkey"], v["signature"], DOMAIN) == sig_ok[i]


def _assert_result(res, model):
    outcome, vidx, bad, n_new = model
    assert list(res.outcome) == outcome
    assert list(res.validator_index) == vidx
    assert res.first_bad_proof == bad == -1
    assert res.n_new == n_new


class Shared:
    pass


@pytest.fixture(scope="module")
def shared():
    """The shared-hash batch with its proofs and model, built once and left unchanged."""
    c = K.case_shared_hash()
    b = Shared()
    b.case, b.datas, b.sig_ok, b.registered, b.n = c, c["datas"], c["sig_ok"], c["registered"], len(c["datas"])
    _oracle_spot_check(b.datas, b.sig_ok)
    b.deposits, b.root, b.leaves = _with_proofs(b.datas, FIRST)
    b.model = M.process_deposits_model(b.registered, b.deposits, b.sig_ok, FIRST, b.root, _leaf)
    return b


def _shared_registry(b):
    reg = _registry(1024)
    assert list(reg.add(b.registered)) == list(range(K.REG_SHARED))
    return reg


def test_key_tables_shared_hash_model_covers_the_patterns(shared):
    """The model on the fixed patterns (no engine call)."""
    outcome, vidx, bad, n_new = shared.model
    assert bad == -1 and FIRST < 2 ** 31 < FIRST + shared.n
    assert [outcome[t] for t in (3, 40, 77)] == [M.SKIPPED, M.NEW, M.TOPUP] and vidx[77] == vidx[40]
    assert outcome[130] == M.NEW and [outcome[131], outcome[600]] == [M.SKIPPED, M.SKIPPED]
    assert (outcome[5], outcome[300]) == (M.NEW, M.TOPUP) and vidx[300] == vidx[5]
    assert [outcome[t] for t in (100, 200, 520)] == [M.SKIPPED, M.NEW, M.TOPUP] and vidx[520] == vidx[200]
    assert 200 // 128 == 520 // 128 - 3                       # the winner three tiles of the scan back
    assert n_new >= 100 and outcome.count(M.SKIPPED) >= 100 and outcome.count(M.TOPUP) >= 300
    # top-ups of keys registered in this batch with the winner in another tile, and early returns
    # (a bad signature before the key's first good one)
    new_at = {shared.datas[t][:48]: t for t in range(shared.n) if outcome[t] == M.NEW}
    assert sum(outcome[t] == M.TOPUP and new_at.get(shared.datas[t][:48], t) // 128 != t // 128
               for t in range(shared.n)) >= 100
    assert sum(outcome[t] == M.SKIPPED and new_at.get(shared.datas[t][:48], -1) > t for t in range(shared.n)) >= 20


def test_key_tables_deposits_shared_hash_commit_and_replay(native, shared):
    reg = _shared_registry(shared)
    res = reg.process_deposits(shared.deposits, FIRST, shared.root, DOMAIN)
    _assert_result(res, shared.model)
    outcome, vidx, _, n_new = shared.model
    assert len(reg) == K.REG_SHARED + n_new
    new_pos = [t for t in range(shared.n) if outcome[t] == M.NEW]
    new_keys = [shared.datas[t][:48] for t in new_pos]
    assert [vidx[t] for t in new_pos] == list(range(K.REG_SHARED, K.REG_SHARED + n_new))
    assert list(reg.lookup(new_keys)) == [vidx[t] for t in new_pos]
    assert list(reg.lookup(shared.registered)) == list(range(K.REG_SHARED))
    never = [k for k in shared.case["keys"] if k not in new_keys and k not in shared.registered]
    assert never and list(reg.lookup(never)) == [-1] * len(never)
    # the same data at the next indices: every key that was NEW is now a validator
    deposits2, root2, _ = _with_proofs(shared.datas, FIRST + shared.n, shared.leaves)
    model2 = M.process_deposits_model(shared.registered + new_keys, deposits2, shared.sig_ok, FIRST + shared.n, root2,
                                      _leaf)
    res2 = reg.process_deposits(deposits2, FIRST + shared.n, root2, DOMAIN)
    _assert_result(res2, model2)
    assert all(res2.outcome[t] == M.TOPUP and res2.validator_index[t] == vidx[t] for t in new_pos)
    assert res2.n_new == 0 and len(reg) == K.REG_SHARED + n_new
    reg.close()


def test_key_tables_deposits_shared_hash_without_commit(native, shared):
    reg = _shared_registry(shared)
    res = reg.process_deposits(shared.deposits, FIRST, shared.root, DOMAIN, commit=False)
    _assert_result(res, shared.model)
    assert len(reg) == K.REG_SHARED
    keys = shared.case["keys"]
    assert list(reg.lookup(keys)) == list(range(K.REG_SHARED)) + [-1] * (len(keys) - K.REG_SHARED)
    reg.close()


def test_key_tables_deposits_shared_hash_strict_policy(native, shared):
    """The strict codec rejects the junk infinity keys: only deposits of registered keys count."""
    model = M.process_deposits_model(shared.registered, shared.deposits, [False] * shared.n, FIRST, shared.root, _leaf)
    assert set(model[0]) == {M.SKIPPED, M.TOPUP} and model[3] == 0
    reg = _shared_registry(shared)
    native.set_subgroup_policy("strict")
    try:
        res = reg.process_deposits(shared.deposits, FIRST, shared.root, DOMAIN)
    finally:
        native.set_subgroup_policy("pyecc")
    _assert_result(res, model)
    assert all((res.outcome[t] == M.TOPUP) == (shared.datas[t][:48] in shared.registered) for t in range(shared.n))
    assert len(reg) == K.REG_SHARED
    reg.close()


@pytest.mark.parametrize("n", K.DENSE_SIZES)
def test_key_tables_deposits_dense_new_across_tiles(native, n):
    c = K.case_dense_new(n)
    if n == K.DENSE_SIZES[0]:
        _oracle_spot_check(c["datas"], c["sig_ok"])
    before = K.crafted_keys(random.Random(0xB15_3002), 7, K.DEP_HASH)
    deposits, root, _ = _with_proofs(c["datas"], FIRST)
    model = M.process_deposits_model(before, deposits, c["sig_ok"], FIRST, root, _leaf)
    assert model[0] == [M.NEW] * n and model[1] == list(range(7, 7 + n))
    reg = _registry(7 + n)                                    # an exact fit
    assert list(reg.add(before)) == list(range(7))
    res = reg.process_deposits(deposits, FIRST, root, DOMAIN)
    _assert_result(res, model)
    assert list(res.validator_index) == list(range(7, 7 + n))  # the scan's carry between tiles
    assert len(reg) == 7 + n and list(reg.lookup(c["keys"])) == list(range(7, 7 + n))
    reg.close()


def test_key_tables_deposits_all_skipped(native):
    c = K.case_all_skipped()
    deposits, root, _ = _with_proofs(c["datas"], FIRST)
    model = M.process_deposits_model(c["registered"], deposits, c["sig_ok"], FIRST, root, _leaf)
    assert model[0] == [M.SKIPPED] * 300 and model[3] == 0
    reg = _registry(1024)
    assert list(reg.add(c["registered"])) == list(range(10))
    res = reg.process_deposits(deposits, FIRST, root, DOMAIN)
    _assert_result(res, model)
    assert res.n_new == 0 and len(reg) == 10                  # nothing appended
    assert list(reg.lookup(c["keys"])) == [-1] * 60
    reg.close()
