"""Committee selection on the CPU: the shuffle and the attesting-group code the kernels run
(csrc/bls381_shuffle.hpp, host build) against tests/golden/shuffling.json (the reference's spec
text, make_shuffling_vectors.py) and against the spec restated in shuffle_model.py.
GPU half: test_committees_gpu.py."""
import ctypes
import os
import random

import numpy as np
import pytest

import shuffle_model as M

ATT_LENGTHS = [0, 1, 7, 8, 9, 255, 256, 257, 4096]


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_shuffled_index.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32]
    lib.hc_shuffled_index.restype = ctypes.c_uint64
    lib.hc_shuffle_list.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.hc_shuffle_list.restype = ctypes.c_int
    lib.hc_verify_bitfield.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_uint32]
    lib.hc_verify_bitfield.restype = ctypes.c_int
    lib.hc_attesting_groups.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p,
                                        ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_attesting_groups.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def hc_list(L, n, seed, rounds, table, first=0, count=None, threads=3):
    count = n - first if count is None else count
    out = np.full(count + 1, 0xABCD1234, dtype=np.uint32)
    assert L.hc_shuffle_list(n, seed, rounds, first, count, table, threads, out.ctypes.data_as(ctypes.c_void_p)) == 0
    assert out[count] == 0xABCD1234
    return out[:count]


def hc_groups(L, committee, agg, cust):
    c = np.ascontiguousarray(committee, dtype=np.uint32)
    o0 = np.full(len(c) + 1, 0xEEEEEEEE, dtype=np.uint32)
    o1 = np.full(len(c) + 1, 0xEEEEEEEE, dtype=np.uint32)
    n = np.zeros(2, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ok = L.hc_attesting_groups(p(c), len(c), agg, cust, len(agg), p(o0), p(o1), p(n))
    assert np.all(o0[n[0]:] == 0xEEEEEEEE) and np.all(o1[n[1]:] == 0xEEEEEEEE)     # nothing past the counts
    return ok, o0[:n[0]].tolist(), o1[:n[1]].tolist()


# ------------------------------------------------------------------- the shuffle
def test_fixture_is_the_generators_cases(fx):
    assert fx["seeds"] == [s.hex() for s in M.generator_seeds()]
    assert fx["supplied"]["SHUFFLE_ROUND_COUNT"] == {"minimal": 10, "mainnet": 90}
    keys = {(c["rounds"], c["seed"], c["count"]) for c in fx["cases"]}
    assert keys == {(r, k, n) for r in (10, 90) for k in range(30) for n in M.GENERATOR_COUNTS} and len(fx["cases"]) == 540
    stored = [c for c in fx["cases"] if "shuffled" in c]
    assert len(stored) == 2 * (4 * 8 + 1)
    for c in stored:
        assert M.list_digest(c["shuffled"]) == c["sha256"]
    pick = {(c["rounds"], c["seed"], c["count"]): c for c in stored}
    assert pick[(10, 0, 10)]["shuffled"] == [8, 9, 6, 7, 4, 3, 5, 1, 0, 2]
    assert pick[(90, 0, 10)]["shuffled"] == [7, 4, 3, 2, 0, 5, 1, 8, 6, 9]


def test_hc_shuffled_index_matches_every_fixture_case(L, fx):
    """One hc_shuffled_index call per position of all 540 cases: the full list where the fixture
    stores it, its digest everywhere; every result is a permutation."""
    seeds = [bytes.fromhex(s) for s in fx["seeds"]]
    for c in fx["cases"]:
        n, seed = c["count"], seeds[c["seed"]]
        got = [L.hc_shuffled_index(i, n, seed, c["rounds"]) for i in range(n)]
        assert sorted(got) == list(range(n)), c
        assert M.list_digest(got) == c["sha256"], (c["rounds"], c["seed"], n)
        if "shuffled" in c:
            assert got == c["shuffled"]


def test_table_form_matches_every_fixture_case(L, fx):
    """The table form (the layout kernel A writes and kernel B reads) and the direct form through
    hc_shuffle_list, whole lists and ragged windows."""
    seeds = [bytes.fromhex(s) for s in fx["seeds"]]
    for c in fx["cases"]:
        n, seed, rounds = c["count"], seeds[c["seed"]], c["rounds"]
        full = hc_list(L, n, seed, rounds, table=1)
        assert M.list_digest(full) == c["sha256"]
        if c["seed"] < 2:
            assert np.array_equal(hc_list(L, n, seed, rounds, table=0), full)
            first = n // 3
            assert np.array_equal(hc_list(L, n, seed, rounds, 1, first, n - first - n // 5), full[first:n - n // 5])


def test_model_forms_agree_with_each_other_and_the_fixture(fx):
    seeds = [bytes.fromhex(s) for s in fx["seeds"]]
    for c in fx["cases"]:
        if c["seed"] >= 6 and c["count"] == 1000:
            continue                                             # the loop form is slow: six seeds at 1000
        n, seed, rounds = c["count"], seeds[c["seed"]], c["rounds"]
        whole = M.shuffled_list(n, seed, rounds)
        assert M.list_digest(whole) == c["sha256"]
        if c["seed"] < 2 or n <= 33:
            assert [M.get_shuffled_index(i, n, seed, rounds) for i in range(n)] == whole.tolist()


def test_model_committees_match_the_fixture(fx):
    seed = bytes.fromhex(fx["seeds"][0])
    indices = [(7 * i + 3) % 1000 + 5000 for i in range(1000)]
    assert len(fx["committees"]) == 4
    for c in fx["committees"][:2]:                               # the minimal preset's two splits (10 rounds)
        parts = [M.compute_committee(indices, seed, j, c["committee_count"], c["rounds"])
                 for j in range(c["committee_count"])]
        assert [len(p) for p in parts] == c["lengths"]
        assert M.list_digest([v for p in parts for v in p]) == c["sha256"]
    sh = M.shuffled_list(1000, seed, 90)
    for c in fx["committees"][2:]:
        assert M.list_digest([indices[i] for i in sh]) == c["sha256"] and sum(c["lengths"]) == 1000


@pytest.mark.parametrize("n", [257, 65793])
def test_larger_lists_against_the_model(L, n):
    """Past the generator's counts: a ragged last block, and n = 65,793 = 65,536 + 257 (the second
    byte of the block counter).  Spot positions against the spec's loop."""
    seed = M.hash(b"larger lists %d" % n)
    for rounds in (10, 90):
        want = M.shuffled_list(n, seed, rounds)
        assert sorted(want.tolist()) == list(range(n))
        assert np.array_equal(hc_list(L, n, seed, rounds, table=1, threads=8), want)
        for i in (0, 1, 255, 256, n - 257, n - 1):
            assert L.hc_shuffled_index(i, n, seed, rounds) == want[i] == M.get_shuffled_index(i, n, seed, rounds)


def test_index_count_near_2_to_32(L):
    """pivot + n - index needs 33 bits: positions at both ends of a list of 2^32 - 1."""
    n, seed = 2 ** 32 - 1, M.hash(b"huge")
    for i in (0, 1, 2 ** 31, n - 2, n - 1):
        for rounds in (10, 90):
            assert L.hc_shuffled_index(i, n, seed, rounds) == M.get_shuffled_index(i, n, seed, rounds)
    first = n - 5
    got = hc_list(L, n, seed, 90, table=0, first=first, count=5)
    assert got.tolist() == [M.get_shuffled_index(first + k, n, seed, 90) for k in range(5)]


def test_zero_rounds_is_the_identity(L):
    seed = M.hash(b"identity")
    for n in (1, 2, 257, 1000):
        assert [L.hc_shuffled_index(i, n, seed, 0) for i in range(n)] == list(range(n))
        assert hc_list(L, n, seed, 0, table=1).tolist() == list(range(n))
        assert M.shuffled_list(n, seed, 0).tolist() == list(range(n))


def test_rejected_arguments(L):
    seed = bytes(32)
    bad = 2 ** 64 - 1
    assert L.hc_shuffled_index(0, 0, seed, 90) == bad            # index < index_count
    assert L.hc_shuffled_index(5, 5, seed, 90) == bad
    assert L.hc_shuffled_index(0, 2 ** 32, seed, 90) == bad      # the 32-bit cap
    assert L.hc_shuffled_index(0, 5, seed, 256) == bad
    assert L.hc_shuffled_index(0, 5, seed, 255) < 5
    buf = np.zeros(8, dtype=np.uint32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.hc_shuffle_list(5, seed, 10, 3, 3, 1, 1, p) == -1
    assert L.hc_shuffle_list(2 ** 32, seed, 10, 0, 1, 0, 1, p) == -1
    assert L.hc_shuffle_list(0, seed, 10, 0, 0, 1, 1, p) == 0


# -------------------------------------------------------------- attesting groups
def _committee(rng, n):
    return rng.sample(range(1 << 20), n)                        # distinct, unsorted


@pytest.mark.parametrize("n", ATT_LENGTHS)
def test_attesting_groups_random_bitfields(L, n):
    rng = random.Random(0xB15_0100 + n)
    for trial in range(6 if n < 4096 else 2):
        committee = _committee(rng, n)
        agg = M.random_bitfield(rng, n, rng.choice([0.1, 0.5, 0.9]))
        cust = M.random_bitfield(rng, n, rng.choice([0.1, 0.5]))
        ok, g0, g1 = hc_groups(L, committee, agg, cust)
        assert ok == 1
        assert (g0, g1) == M.convert_to_indexed_sets(committee, agg, cust)
        assert g1 == M.get_attesting_indices(committee, cust)    # whatever the aggregation bits say


@pytest.mark.parametrize("n", ATT_LENGTHS)
def test_attesting_groups_all_zero_and_all_one(L, n):
    rng = random.Random(0xB15_0200 + n)
    committee = _committee(rng, n)
    zero, one = M.random_bitfield(rng, n, 0.0), M.random_bitfield(rng, n, 1.0)
    assert hc_groups(L, committee, zero, zero) == (1, [], [])
    assert hc_groups(L, committee, one, zero) == (1, sorted(committee), [])
    assert hc_groups(L, committee, one, one) == (1, [], sorted(committee))
    assert hc_groups(L, committee, zero, one) == (1, [], sorted(committee))      # custody set, aggregation clear


def test_custody_bit_where_the_aggregation_bit_is_clear(L):
    committee = [50, 40, 30, 20, 10, 60, 70, 80, 90]
    agg = bytes([0b00010011, 0])                                # members 0, 1, 4
    cust = bytes([0b00000110, 1])                               # members 1, 2, 8: 2 and 8 did not aggregate
    ok, g0, g1 = hc_groups(L, committee, agg, cust)
    assert (ok, g0, g1) == (1, [10, 50], [30, 40, 90])
    assert (g0, g1) == M.convert_to_indexed_sets(committee, agg, cust)


def test_entries_equal_to_the_sort_padding_value(L):
    """0xFFFFFFFF is what the sort pads with; as a committee member it still comes out."""
    committee = [0xFFFFFFFF, 5, 0xFFFFFFFE]
    assert hc_groups(L, committee, b"\x07", b"\x00") == (1, [5, 0xFFFFFFFE, 0xFFFFFFFF], [])


def test_verify_bitfield_rejections(L):
    for n in ATT_LENGTHS:
        nbytes = (n + 7) // 8
        good = bytes(nbytes)
        assert L.hc_verify_bitfield(good, nbytes, n) == 1 == int(M.verify_bitfield(good, n))
        for wrong in (bytes(nbytes + 1), bytes(max(nbytes - 1, 0))):                  # wrong length
            if len(wrong) != nbytes:
                assert L.hc_verify_bitfield(wrong, len(wrong), n) == 0 == int(M.verify_bitfield(wrong, n))
        for bit in range(n, 8 * nbytes):                                             # every padding bit
            b = bytearray(nbytes)
            b[bit // 8] |= 1 << (bit % 8)
            assert L.hc_verify_bitfield(bytes(b), nbytes, n) == 0 == int(M.verify_bitfield(bytes(b), n))
            if n:
                full = bytearray(M.random_bitfield(random.Random(1), n, 1.0))
                assert L.hc_verify_bitfield(bytes(full), nbytes, n) == 1
    committee = list(range(9))
    assert hc_groups(L, committee, b"\xff\x03", b"\x00\x00") == (0, [], [])          # padding bit in aggregation
    assert hc_groups(L, committee, b"\xff\x01", b"\x00\x02") == (0, [], [])          # padding bit in custody
    assert hc_groups(L, committee, b"\xff", b"\x00") == (0, [], [])                  # too short
    assert hc_groups(L, committee, b"\xff\x01", b"\x00\x00") == (1, committee, [])
    with pytest.raises(AssertionError):
        M.get_attesting_indices(committee, b"\xff\x03")
