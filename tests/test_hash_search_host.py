"""tests/golden/hash_search.json and the batches composed from it (tests/hash_search_cases.py), on
the CPU: the fixture holds what its generator promises, the host build of the product's
hash_to_g2_candidate agrees with it, and the pooled search's model says that the composed waves reach
the lane splits they were built for -- so tests/test_hash_search_gpu.py steers the device searches,
and a fixture regenerated differently fails here before it weakens that test.
"""
import ctypes

import pytest

import bls_oracle as O
import hash_search_cases as C

LENGTHS = [46, 47, 54, 55, 56, 63, 64, 110, 111, 119, 120]
r = O.r


@pytest.fixture(scope="module")
def fx():
    return C.fixture()


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(build_native.build_hostcheck())
    lib.hc_hash_to_g2.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return lib


def test_fixture_conditions(fx):
    raw = fx.raw
    assert raw["tag"] == "trial-search" and raw["domain"] == 7
    by = fx.pool()
    assert len({m.i for m in fx.messages}) == len(fx.messages)
    for t in range(1, 7):
        assert len(by[t]) == 64
    for t in range(7, 16):
        assert len(by[t]) == 8
    assert len(by[16]) >= 4
    high = [m for m in fx.messages if m.trials >= 17]
    assert len(high) >= 4 and any(m.trials >= 18 for m in high)
    assert fx.max_trials < 33            # a third wide round is out of scope
    for m in fx.messages:
        # the mask's first set bit is the trial count
        assert m.squares and (m.squares & -m.squares).bit_length() == m.trials and m.squares < 1 << 64
    # oracle points: two messages per distinct trial count and all with 16 or more
    pts = fx.pool(points_only=True)
    for t, ms in by.items():
        assert len(pts[t]) == (len(ms) if t >= 16 else 2)
    for p in raw["points"]:
        m = fx.by_i[p["i"]]
        assert p["trials"] == m.trials and p["next_offset"] >= m.trials and (m.squares >> p["next_offset"]) & 1
        assert not (m.squares >> m.trials) & ((1 << (p["next_offset"] - m.trials)) - 1)
        x0 = C.x0_of(m.msg, fx.dom8)
        assert [int(h, 16) for h in p["candidate"][:2]] == [(x0[0] + m.trials - 1) % O.q, x0[1]]
        assert len({p["compressed"], p["next_square_sig"], p["negated_sig"]}) == 3
    assert [c["length"] for c in raw["lengths"]] == LENGTHS
    K = [int(s["k"], 16) for s in raw["scalars"]]
    assert K[:22] == [0, 1, 2, 3, (r - 1) // 2, (r + 1) // 2, r - 2, r - 1, r, r + 1, r + 2, 2 * r - 1, 2 * r,
                      2 * r + 1, 2 * r + 3, 2 * r + 4, 1 << 31, 1 << 32, 1 << 224, 1 << 248, 1 << 255, (1 << 256) - 1]
    assert len(K) == 25 and all(r <= k < 1 << 256 for k in K[22:])
    even, odd = (fx.by_i[i].trials for i in raw["scalar_messages"])
    assert even % 2 == 0 and odd % 2 == 1
    assert all(len(s["signatures"]) == 2 for s in raw["scalars"])
    # the edge scalars' known answers
    pub = {int(s["k"], 16): s["pubkey"] for s in raw["scalars"]}
    inf1, inf2 = "c0" + "00" * 47, "c0" + "00" * 95
    assert pub[0] == pub[r] == pub[2 * r] == inf1
    assert pub[r + 1] == pub[1] == pub[2 * r + 1] and pub[r + 2] == pub[2] and pub[2 * r + 3] == pub[3]
    sig = {int(s["k"], 16): s["signatures"] for s in raw["scalars"]}
    assert sig[r] == sig[0] == [inf2, inf2] and sig[r + 2] == sig[2]


def test_fixture_candidates_and_one_oracle_run(fx):
    """Every stored candidate is on the twist with the spec's root; the oracle itself re-run on the
    message of the most trials (the generator confirmed every kept message with it)."""
    for p in fx.raw["points"]:
        x0, x1, y0, y1 = (int(h, 16) for h in p["candidate"])
        assert C.on_twist_with_selected_root((x0, x1), (y0, y1))
    m = max(fx.messages, key=lambda m: (m.trials, -m.i))
    x, y, trials = O.hash_to_G2_affine_candidate(m.msg, fx.domain)
    assert trials == m.trials == fx.max_trials
    assert [x[0], x[1], y[0], y[1]] == [int(h, 16) for h in m.point["candidate"]]


def test_host_build_agrees_with_the_fixture(fx, L):
    aff = ctypes.create_string_buffer(192)
    comp = ctypes.create_string_buffer(96)
    for p in fx.raw["points"]:
        assert L.hc_hash_to_g2(fx.by_i[p["i"]].msg, 32, fx.dom8, aff, comp) == p["trials"]
        assert comp.raw.hex() == p["compressed"]
        assert aff.raw.hex() == "".join(p["affine"])
    for c in fx.raw["lengths"]:
        m = fx.length_message(c["length"])
        assert len(m) == c["length"]
        assert L.hc_hash_to_g2(m, len(m), fx.dom8, aff, comp) == c["trials"]
        assert comp.raw.hex() == c["compressed"]


def traces(by):
    return {name: [C.wave_trace(w) for w in C.waves_of(items)] for name, items in C.pooled_compositions(by)}, \
        dict(C.pooled_compositions(by))


def test_model_over_the_composed_waves(fx):
    """The model returns trials - 1 for every item of every pooled composition (from the whole pool and
    from the messages with oracle records), and the compositions reach what they are built for."""
    for points_only in (False, True):
        tr, comps = traces(fx.pool(points_only))
        for name, items in comps.items():
            got = [f for found, _ in tr[name] for f in found]
            assert got == [m.trials - 1 for m in items], name
    tr, comps = traces(fx.pool())
    assert [len(items) for items in comps.values()] == [1] + [64] * 11 + [65, 127, 129, 200] + [256] * 4
    assert tr["lone_high"][0][1] == [1]                                # all 64 lanes: one round
    assert tr["all_1"][0][1] == [64]
    for t in range(2, 7):
        assert tr["all_%d" % t][0][1] == [64] * t
    for lane in (0, 31, 63):
        assert tr["high_at_%d" % lane][0][1] == [64, 1]
        assert comps["high_at_%d" % lane][lane].trials == fx.max_trials
    assert tr["three_left"][0][1] == [64, 3]
    assert sorted(m.trials for m in comps["three_left"] if m.trials > 1)[0] == 2
    assert sorted(m.trials for m in comps["three_left"] if m.trials > 1)[1:] >= [17, 18]
    # m = 40
    w = comps["forty_left"]
    m40 = tr["forty_left"][0][1]
    assert m40[:2] == [64, 40] and len(m40) >= 3
    left = [m for m in w if m.trials > 1]
    assert len(left) == 40
    two, one = left[:24], left[24:]
    assert sum(m.trials == 3 for m in two) >= 4                        # first square on the second lane
    assert any(m.trials == 2 and (m.squares >> 2) & 1 for m in two)    # squares on both lanes
    assert sum(m.trials > 2 for m in one) >= 4                         # one-lane ranks that fail again
    assert m40[2] == sum(m.trials > 3 for m in two) + sum(m.trials > 2 for m in one)
    # partial last waves: their high-trial items pool with invalid lanes lending themselves
    for n in (65, 127, 129, 200):
        assert comps["n_%d" % n][-1].trials >= 16 and len(tr["n_%d" % n]) == (n + 63) // 64
    # coverage across the compositions
    rounds = [len(t) for ws in tr.values() for _, t in ws]
    ms = {m for ws in tr.values() for _, t in ws for m in t}
    assert max(rounds) >= 5
    assert any(32 < m < 64 for m in ms)
    assert any(m < 32 and 64 % m for m in ms)
    print("pooled model: %d waves, rounds per wave %d..%d (mean %.2f), distinct m %d: %s" % (
        len(rounds), min(rounds), max(rounds), sum(rounds) / len(rounds), len(ms), sorted(ms)))


def test_wide_compositions(fx):
    by = fx.pool()
    comps = dict(C.wide_compositions(by))
    pos = comps["positions"]
    assert len(pos) == 4 * 4 * (len(C.WIDE_TRIALS) + 1)
    for k, t in enumerate(C.WIDE_TRIALS + (fx.max_trials,)):
        for p in range(4):
            wave = pos[16 * k + 4 * p:16 * k + 4 * p + 4]
            assert [m.trials for m in wave] == [t if j == p else 1 for j in range(4)]
    assert len(comps["all_second_round"]) == 4 and all(m.trials >= 17 for m in comps["all_second_round"])
    for n in (1, 3, 5, 9):
        assert len(comps["n_%d" % n]) == n and comps["n_%d" % n][-1].trials >= 17
    # the same shapes from the messages with oracle records (the verdict tests' items)
    for name, items in C.wide_compositions(fx.pool(points_only=True)):
        assert [m.trials for m in items] == [m.trials for m in comps[name]], name
        assert all(m.point is not None for m in items)


def test_probe_batches_hold_stored_points(fx):
    """The probe batches reach the fixture's stored points at every trial count."""
    comps = C.pooled_compositions(fx.pool()) + C.wide_compositions(fx.pool())
    seen = {m.trials for _, items in comps for m in items if m.point is not None}
    assert seen == set(range(1, fx.max_trials + 1))


def test_valid_items_are_valid_and_spoiled_ones_are_not(fx):
    """The verdict tests' items through the oracle's verify: (g1, msg, hash_to_G2(msg)) is valid, and
    neither the hash from the next square offset nor the negated hash is."""
    assert C.G1_KEY == O.privtopub(1)
    m = fx.pool(points_only=True)[17][0]
    items = C.valid_items([m, m, m])
    assert C.spoil(items, [m, m, m], [1, 2]) == [True, False, False]
    assert [O.verify(msg, pk, sig, fx.domain) for pk, msg, sig in items] == [True, False, False]


def test_hashcheck_is_one_gfx950_code_object():
    import build_native
    blob = open(build_native.build_hashcheck(), "rb").read()
    assert b"hipv4-amdgcn-amd-amdhsa--gfx950" in blob
    assert b"amdhsa--gfx942" not in blob and b"amdhsa--gfx90a" not in blob
    assert b"bls381_verify" not in blob      # test infrastructure: no product symbol
    assert b"hsc_run" in blob
