"""The epoch context on the CPU: the code the kernels share (csrc/bls381_epoch.hpp, host build)
against tests/golden/epoch_context.json (the reference's spec text,
make_epoch_context_vectors.py) and against the spec restated in epoch_model.py, which is itself
checked against the fixture here.  GPU half: test_epoch_gpu.py."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

import epoch_cases as C
import epoch_model as M
import shuffle_model as SM

GUARD32 = 0xEEEEEEEE


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_active_indices.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_active_indices.restype = ctypes.c_int
    lib.hc_index_chunks.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_index_chunks.restype = None
    lib.hc_proposer_digest.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.hc_proposer_digest.restype = None
    lib.hc_proposer_index.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_size_t,
                                      ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    lib.hc_proposer_index.restype = ctypes.c_uint32
    return lib


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def p(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def hc_active(L, n, act, ext, stride, epoch, bal=None, bal_stride=8, threads=3):
    """act / ext / bal: ctypes pointers.  (indices, total); nothing is written past the count."""
    out = np.full(n + 1, GUARD32, dtype=np.uint32)
    res = np.zeros(2, dtype=np.uint64)
    assert L.hc_active_indices(n, act, ext, stride, epoch, bal, bal_stride, threads, p(out), p(res)) == 0
    count = int(res[0])
    assert count <= n and np.all(out[count:] == GUARD32)
    return out[:count], int(res[1])


def hc_proposer(L, committee, epoch, bal, seed, n_validators=None, max_eb=C.MAX_EB, max_tries=1 << 20, stride=8):
    committee = np.ascontiguousarray(committee, dtype=np.uint32)
    tries = ctypes.c_uint32(0)
    got = L.hc_proposer_index(p(committee), len(committee), epoch, p(bal), stride,
                              len(bal) if n_validators is None else n_validators, seed, max_eb, max_tries,
                              ctypes.byref(tries))
    return got, tries.value


# ------------------------------------------------------------- the model against the fixture
def test_fixture_shape(fx):
    assert fx["epoch"] == 5
    assert [(c["preset"], c["n"]) for c in fx["cases"]] == [(pr, n) for pr in ("minimal", "mainnet")
                                                           for n in (0, 1, 7, 64, 301)]
    k = fx["supplied"]["constants"]
    assert (k["minimal"]["SLOTS_PER_EPOCH"], k["minimal"]["SHUFFLE_ROUND_COUNT"], k["minimal"]["SHARD_COUNT"]) == (8, 10, 8)
    assert (k["mainnet"]["SLOTS_PER_EPOCH"], k["mainnet"]["SHUFFLE_ROUND_COUNT"], k["mainnet"]["SHARD_COUNT"]) == (64, 90, 1024)
    for c in fx["cases"]:
        assert len(c["proposers"]) == k[c["preset"]]["SLOTS_PER_EPOCH"]
        assert any(v is not None for v in c["proposers"]) == (c["n"] > 0)


def test_model_matches_the_fixture(fx):
    for case in fx["cases"]:
        consts = fx["supplied"]["constants"][case["preset"]]
        st = M.fixture_state(case, consts)
        for e in case["epochs"]:
            active = M.get_active_validator_indices(st.activation_epochs, st.exit_epochs, e["epoch"])
            assert active == e["active"]
            assert M.active_index_root(active).hex() == e["index_root"]
            assert M.get_total_balance(st.effective_balances, active) == e["total_balance"]
            assert M.epoch_committee_count(len(active), consts) == e["committee_count"]
            assert M.shard_delta(len(active), consts) == e["shard_delta"]
            assert M.epoch_start_shard(st, e["epoch"]) == e["start_shard"]
        assert M.state_seed(st, 5).hex() == case["seed"]
        committees = [M.get_crosslink_committee(st, 5, s) for s in case["shards"]]
        assert [len(m) for m in committees] == case["committee_lengths"]
        assert SM.list_digest([v for m in committees for v in m]) == case["committees_sha256"]
        if "committees" in case:
            assert committees == case["committees"]
        per_slot = len(committees) // consts["SLOTS_PER_EPOCH"]
        for s, want in enumerate(case["proposers"]):
            st.slot = case["slot"] + s
            assert (want is None) == (len(committees[per_slot * s]) == 0)
            if want is not None:
                assert M.get_beacon_proposer_index(st) == want


# ------------------------------------------------------------------------- active indices
def test_active_indices_fixture(L, fx):
    for case in fx["cases"]:
        act, ext, bal = C.u64(case["activation_epochs"]), C.u64(case["exit_epochs"]), C.u64(case["effective_balances"])
        for e in case["epochs"]:
            got, total = hc_active(L, case["n"], p(act), p(ext), 8, e["epoch"], p(bal))
            assert got.tolist() == e["active"]
            assert max(total, 1) == e["total_balance"]


@pytest.mark.parametrize("n", C.ACTIVE_SIZES)
def test_active_indices_patterns(L, n):
    bal = C.balances(n)
    for name, (act, ext, epoch) in C.active_patterns(n).items():
        want = C.expected_active(act, ext, epoch)
        assert want.tolist() == M.get_active_validator_indices(act.tolist(), ext.tolist(), epoch), name
        got, total = hc_active(L, n, p(act), p(ext), 8, epoch, p(bal))
        assert np.array_equal(got, want), name
        assert total == C.expected_total(bal, want), name
        got, total = hc_active(L, n, p(act), p(ext), 8, epoch)   # no balances: no sum
        assert np.array_equal(got, want) and total == 0, name
    assert len(C.expected_active(*C.active_patterns(n)["all"])) == n
    assert len(C.expected_active(*C.active_patterns(n)["none"])) == 0
    assert C.expected_active(*C.active_patterns(n)["ends"]).tolist() == sorted({0, n - 1} & set(range(n)))


def test_active_edges_and_unsigned_compare(L):
    far = C.FAR
    act = C.u64([5, 6, 0, 0, far, 0, 2 ** 63, 2 ** 63 + 1, 0])
    ext = C.u64([far, far, 5, 6, far, far, far, far, 2 ** 63])
    assert hc_active(L, 9, p(act), p(ext), 8, 5)[0].tolist() == [0, 3, 5, 8]           # == activation in, == exit out
    assert hc_active(L, 9, p(act), p(ext), 8, 2 ** 63)[0].tolist() == [0, 1, 5, 6]
    assert hc_active(L, 9, p(act), p(ext), 8, far - 1)[0].tolist() == [0, 1, 5, 6, 7]
    assert hc_active(L, 9, p(act), p(ext), 8, far)[0].tolist() == []                    # nothing exits after FAR


@pytest.mark.parametrize("n", [1, 65, 257, 2049])
def test_active_indices_over_validator_records(L, n):
    """Stride 121 at an odd base: byte-wise loads, and the last record's fields end inside the
    buffer (the copy handed over ends 8 bytes after the last balance)."""
    act, ext, epoch = C.active_patterns(n)["mixed"]
    bal = C.balances(n)
    buf, base = C.records_at_odd_base(act, ext, bal)
    span = (n - 1) * M.VALIDATOR_BYTES + M.OFF_BALANCE + 8
    tight = buf[:base + span].copy()   # no byte after the last field
    got, total = hc_active(L, n, p(tight, base + M.OFF_ACTIVATION), p(tight, base + M.OFF_EXIT), M.VALIDATOR_BYTES, epoch,
                           p(tight, base + M.OFF_BALANCE), M.VALIDATOR_BYTES)
    want = C.expected_active(act, ext, epoch)
    assert np.array_equal(got, want) and total == C.expected_total(bal, want)


def test_active_balance_sum_wraps_at_64_bits(L):
    n = 5
    act, ext = C.u64([0] * n), C.u64([C.FAR] * n)
    bal = C.u64([2 ** 63, 2 ** 63, 7, 2 ** 64 - 1, 1])
    assert hc_active(L, n, p(act), p(ext), 8, 0, p(bal))[1] == sum(int(b) for b in bal) % 2 ** 64


def test_active_rejected_arguments(L):
    a = C.u64([0])
    out = np.zeros(2, dtype=np.uint32)
    res = np.zeros(2, dtype=np.uint64)
    assert L.hc_active_indices(1 << 32, p(a), p(a), 8, 0, None, 8, 1, p(out), p(res)) == -1
    assert L.hc_active_indices(1, p(a), p(a), 7, 0, None, 8, 1, p(out), p(res)) == -1
    assert L.hc_active_indices(1, p(a), p(a), 8, 0, p(a), 4, 1, p(out), p(res)) == -1


# -------------------------------------------------------------------------- index chunks
@pytest.mark.parametrize("n", C.ROOT_SIZES + [301])
def test_index_chunks_and_root(L, n):
    rng = random.Random(n)
    idx = np.array(sorted(rng.sample(range(1 << 32), n)), dtype=np.uint32)
    words = np.full(4 * ((n + 3) // 4) + 1, 0xEEEEEEEEEEEEEEEE, dtype=np.uint64)
    L.hc_index_chunks(n, p(idx), p(words))
    assert words[-1] == 0xEEEEEEEEEEEEEEEE
    data = words[:-1].astype("<u8").tobytes()
    assert [data[k:k + 32] for k in range(0, len(data), 32)] == M.index_chunks(idx.tolist())
    import ssz_oracle as S   # the oracle's merkleize over the same chunks, the length mixed in
    chunks = M.index_chunks(idx.tolist()) or [S.ZERO]
    assert M.active_index_root(idx.tolist()) == hashlib.sha256(S.merkleize_chunks(chunks) + n.to_bytes(32, "little")).digest()


def test_index_roots_of_the_fixture(L, fx):
    for case in fx["cases"]:
        for e in case["epochs"]:
            idx = np.array(e["active"], dtype=np.uint32)
            words = np.zeros(4 * ((len(idx) + 3) // 4), dtype=np.uint64)
            L.hc_index_chunks(len(idx), p(idx), p(words))
            data = words.astype("<u8").tobytes()
            root = M.merkleize([data[k:k + 32] for k in range(0, len(data), 32)])
            assert hashlib.sha256(root + len(idx).to_bytes(32, "little")).hexdigest() == e["index_root"]


# ----------------------------------------------------------------------------- proposers
def test_proposer_digest(L):
    out = np.zeros(32, dtype=np.uint8)
    for seed in (bytes(32), bytes(range(32)), hashlib.sha256(b"x").digest()):
        for q in (0, 1, 255, 256, 2 ** 15 - 1, 2 ** 32 + 5, 2 ** 64 - 1):
            L.hc_proposer_digest(seed, q, p(out))
            assert out.tobytes() == hashlib.sha256(seed + q.to_bytes(8, "little")).digest()


def test_proposers_of_the_fixture(L, fx):
    for case in fx["cases"]:
        consts = fx["supplied"]["constants"][case["preset"]]
        st = M.fixture_state(case, consts)
        bal = C.u64(case["effective_balances"])
        seed = bytes.fromhex(case["seed"])
        committees = case.get("committees") or [M.get_crosslink_committee(st, 5, s) for s in case["shards"]]
        per_slot = len(committees) // consts["SLOTS_PER_EPOCH"]
        for s, want in enumerate(case["proposers"]):
            if want is not None:
                got, _ = hc_proposer(L, committees[per_slot * s], 5, bal, seed, max_eb=consts["MAX_EFFECTIVE_BALANCE"])
                assert got == want, (case["preset"], case["n"], s)


def test_proposer_full_balances_win_at_try_zero(L):
    bal = C.u64([C.MAX_EB] * 50)
    for length in (1, 3, 50):
        committee = C.committee_of(length, 50)
        for epoch in (0, 1, 7, 2 ** 40 + 3):
            got, tries = hc_proposer(L, committee, epoch, bal, hashlib.sha256(bytes([length])).digest())
            assert (got, tries) == (int(committee[epoch % length]), 0)


@pytest.mark.parametrize("want", C.WINNING_TRIES + ["late"])
def test_proposer_winning_try_at_digest_and_window_edges(L, want):
    seed, t = C.seed_with_winning_try(want)
    assert t == want or (want == "late" and t > 512)
    bal = C.u64([0] * 100)
    for length, epoch in ((1, 9), (3, 7), (4096, 4099)):
        assert epoch % length != 0 or length == 1
        committee = C.committee_of(length, 100)
        assert M.proposer_search(committee.tolist(), epoch, bal.tolist(), seed, C.MAX_EB) == (int(committee[(epoch + t) % length]), t)
        assert hc_proposer(L, committee, epoch, bal, seed) == (int(committee[(epoch + t) % length]), t)
        # the cap: one try fewer finds nothing
        assert hc_proposer(L, committee, epoch, bal, seed, max_tries=t) == (0xFFFFFFFF, t)


def test_proposer_random_cases_match_the_model(L):
    rng = random.Random(0xE9)
    for _ in range(200):
        nv = rng.choice([1, 5, 300])
        bal = C.u64([rng.choice([0, 1, 8, 16, 31, 32, 40]) * C.ETH + rng.randrange(3) for _ in range(nv)])
        committee = C.committee_of(rng.choice([1, 2, 3, 17, 128]), nv, seed=rng.randrange(1000))
        epoch = rng.choice([0, 5, 2 ** 32 - 1, 2 ** 64 - 1, rng.randrange(2 ** 64)])
        seed = rng.getrandbits(256).to_bytes(32, "little")
        clamped = [min(int(b), C.MAX_EB) for b in bal]
        want = M.proposer_search(committee.tolist(), epoch, bal.tolist(), seed, C.MAX_EB)
        assert want == M.proposer_search(committee.tolist(), epoch, clamped, seed, C.MAX_EB)   # the clamp changes nothing
        assert hc_proposer(L, committee, epoch, bal, seed) == want


def test_proposer_balance_just_below_the_limit(L):
    """max_effective_balance = 2^56 - 1 and larger balances: the products stay within 64 bits."""
    max_eb = 2 ** 56 - 1
    bal = C.u64([2 ** 64 - 1, max_eb, max_eb // 2, 0])
    committee = np.array([3, 2, 1, 0], dtype=np.uint32)
    for k in range(20):
        seed = hashlib.sha256(bytes([k])).digest()
        assert hc_proposer(L, committee, k, bal, seed, max_eb=max_eb) == M.proposer_search(
            committee.tolist(), k, bal.tolist(), seed, max_eb)


def test_proposer_over_validator_records(L):
    n = 40
    bal = C.balances(n)
    buf, base = C.records_at_odd_base(C.u64([0] * n), C.u64([C.FAR] * n), bal)
    tight = buf[:base + (n - 1) * M.VALIDATOR_BYTES + M.OFF_BALANCE + 8].copy()
    committee = C.committee_of(17, n)
    for k in range(10):
        seed = hashlib.sha256(b"rec" + bytes([k])).digest()
        tries = ctypes.c_uint32(0)
        got = L.hc_proposer_index(p(committee), 17, k, p(tight, base + M.OFF_BALANCE), M.VALIDATOR_BYTES, n, seed, C.MAX_EB,
                                  1 << 20, ctypes.byref(tries))
        assert (got, tries.value) == M.proposer_search(committee.tolist(), k, bal.tolist(), seed, C.MAX_EB)


def test_proposer_out_of_range_entry_and_rejected_arguments(L):
    bal = C.u64([0] * 4)
    seed, t = C.seed_with_winning_try(31)
    # an entry >= n_validators met before the winning try ends the search; its balance is not read
    # (bal has 4 entries, the entry is 4 or 2^32 - 1)
    for bad in (4, 0xFFFFFFFF):
        committee = np.array([0, 1, bad, 3], dtype=np.uint32)
        assert hc_proposer(L, committee, 0, bal, seed) == (0xFFFFFFFF, 2)
    # met only after the winning try: not looked at
    committee = np.array([0] * 40 + [99], dtype=np.uint32)
    assert hc_proposer(L, committee, 0, bal, seed) == (0, 31)
    ok = np.array([0], dtype=np.uint32)
    assert hc_proposer(L, ok, 0, bal, seed, max_eb=0)[0] == 0xFFFFFFFF
    assert hc_proposer(L, ok, 0, bal, seed, max_eb=2 ** 56)[0] == 0xFFFFFFFF
    assert hc_proposer(L, ok, 0, bal, seed, stride=7)[0] == 0xFFFFFFFF
    assert hc_proposer(L, ok[:0], 0, bal, seed)[0] == 0xFFFFFFFF
