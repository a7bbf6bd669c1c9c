"""The epoch rewards on the CPU: rewards_model.py against tests/golden/epoch_rewards.json (the
reference's spec text, make_epoch_rewards_vectors.py), then the code the kernels share
(csrc/bls381_rewards.hpp, host build) against the model, and the same header in a stand-alone
ASan/UBSan program.  GPU half: test_rewards_gpu.py."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import rewards_cases as C
import rewards_model as M

U64 = 1 << 64
vp, u64, u32, sz = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_size_t


@pytest.fixture(scope="module")
def L():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_mul_div_u64.argtypes = [u64, u64, u64, vp]
    lib.hc_mul_div_u64.restype = u64
    lib.hc_isqrt_u64.argtypes = [u64]
    lib.hc_isqrt_u64.restype = u64
    lib.hc_epoch_votes.argtypes = [u64, vp, vp, vp, u64, vp, sz, vp, sz] + [vp] * 16
    lib.hc_epoch_votes.restype = ctypes.c_int
    lib.hc_epoch_deltas.argtypes = ([u64, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, u64, u64, vp,
                                     u32] + [vp] * 4)
    lib.hc_epoch_deltas.restype = ctypes.c_int
    lib.hc_epoch_slashings.argtypes = [u64, vp, sz, vp, vp, sz, u64, u64, u64, u64, u64, vp]
    lib.hc_epoch_slashings.restype = ctypes.c_int
    lib.hc_effective_balances.argtypes = [u64, vp, vp, sz, u64, u64, vp, vp, vp]
    lib.hc_effective_balances.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


def p(a, off=0):
    return ctypes.c_void_p(a.ctypes.data + off)


def a64(x):
    return np.array(list(x) + [0], dtype=np.uint64)   # never empty


def a32(x):
    return np.array(list(x) + [0], dtype=np.uint32)


# ------------------------------------------------------------- the model against the fixture
def test_fixture_shape(fx):
    assert [(c["preset"], c["n"]) for c in fx["cases"]] == [("minimal", 1), ("minimal", 7), ("minimal", 64),
                                                           ("minimal", 301), ("mainnet", 301)]
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(golden, "epoch_rewards.json")) <= os.path.getsize(
        os.path.join(golden, "merkle_trees.json"))
    k = fx["supplied"]["constants"]
    assert (k["minimal"]["MIN_ATTESTATION_INCLUSION_DELAY"], k["mainnet"]["MIN_ATTESTATION_INCLUSION_DELAY"]) == (2, 4)
    delays = {c["previous_epoch"] - c["finalized_epoch"] for c in fx["cases"]}
    assert delays == {4, 5} and k["minimal"]["MIN_EPOCHS_TO_INACTIVITY_PENALTY"] == 4   # both sides of the threshold
    seen = set()
    for c in fx["cases"]:
        seen.update(c["patterns"])
    assert seen == set(fx["patterns"])


def test_fixture_covers_the_cases(fx):
    """What the generator promises is in the states it made."""
    c = fx["cases"][2]
    kinds = set(c["kinds"])
    assert {"slashed_active", "slashed_exited", "slashed_done", "pending", "exited", "leaving", "joining"} <= kinds
    vo, per, cand_count, _ = M.case_votes(c)
    sl = c["slashed"]
    members = [v for m in c["committees"] for v in m]
    assert any(sl[v] and vo["votes"][v] == M.MEMBER for v in members)                      # slashed attesters: no bits
    assert any(len(a) == 0 for a in per) and any(len(a) >= 3 for a in per)                 # none / overlapping
    assert any(k == 2 for k in cand_count) and any(k == 0 for k in cand_count)             # ties / filter failures
    proposers = {a["proposer_index"] for a in c["attestations"]}
    assert any(sl[q] for q in proposers)
    assert any(c["kinds"][q] in ("pending", "slashed_done") for q in proposers)
    # equal delays, different proposers
    assert any(len({a["proposer"] for a in m if a["delay"] == 3}) >= 2 for m in per)
    # the attestation equal to Crosslink() forms candidate 0 of shard 0 in some state
    assert any(cs["winners"][cs["shards"].index(0)]["crosslink"][:3] == [0, 0, 0] and
               cs["winners"][cs["shards"].index(0)]["attesters"] > 0 for cs in fx["cases"])
    k, _ = M.case_constants(fx, c)
    half = k["LATEST_SLASHED_EXIT_LENGTH"] // 2
    assert any(s and w == c["current_epoch"] + half for s, w in zip(sl, c["withdrawable_epochs"]))
    for cs in fx["cases"][1:]:
        h = cs["hysteresis"]
        moved = [a != b for a, b in zip(cs["effective_balances"], h["effective_balances_after"])]
        assert any(moved) and not all(moved)


def test_model_matches_the_fixture(fx):
    for case in fx["cases"]:
        k, K = M.case_constants(fx, case)
        vo, per, cand_count, crosslinks = M.case_votes(case)
        assert [max(1, t) for t in vo["totals"]] == case["attesting_balances"]
        for c, w in enumerate(case["winners"]):
            assert max(1, vo["committee_balance"][c]) == w["committee_balance"]
            assert max(1, vo["winner_balance"][c]) == w["attesting_balance"]
            x = w["crosslink"]
            want = (x[0], x[1], x[2], bytes.fromhex(x[3]), bytes.fromhex(x[4]))
            if vo["winner"][c] == M.NONE:
                assert want == M.DEFAULT_CROSSLINK and w["attesters"] == 0
            else:
                assert crosslinks[c][vo["winner"][c]] == want
                assert sum(1 for v in case["committees"][c] if vo["votes"][v] & M.WINNER) == w["attesters"]
        r1, p1, _, o1 = M.case_deltas(fx, case, vo, 1)
        r2, p2, _, o2 = M.case_deltas(fx, case, vo, 2)
        r3, p3, b3, o3 = M.case_deltas(fx, case, vo, 3)
        assert (o1, o2, o3) == (0, 0, 0)
        assert M.matches(case["attestation_deltas"]["rewards"], r1) and M.matches(case["attestation_deltas"]["penalties"], p1)
        assert M.matches(case["crosslink_deltas"]["rewards"], r2) and M.matches(case["crosslink_deltas"]["penalties"], p2)
        assert r3 == [a + b for a, b in zip(r1, r2)] and p3 == [a + b for a, b in zip(p1, p2)]
        assert M.matches(case["balances_after_rewards"], b3)
        b4 = M.slashings(case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3, case["current_epoch"],
                         case["total_penalties"], case["total_active_balance"], k["LATEST_SLASHED_EXIT_LENGTH"],
                         k["MIN_SLASHING_PENALTY_QUOTIENT"])
        assert M.matches(case["balances_after_slashings"], b4) and M.matches(case["balances_after_final"], b4)
        idx, val, changed = M.hysteresis(b4, case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"],
                                         k["MAX_EFFECTIVE_BALANCE"])
        assert M.matches(case["effective_balances_after"], val)
        assert changed == sum(1 for a, b in zip(val, case["effective_balances"]) if a != b)
        h = case["hysteresis"]
        assert M.hysteresis(h["balances"], case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"],
                            k["MAX_EFFECTIVE_BALANCE"])[1] == h["effective_balances_after"]
    assert any(b == 0 and a > 0 for case in fx["cases"][:3]
               for a, b in zip(case["balances"], case["balances_after_rewards"]))   # a penalty takes a balance to 0


def test_model_square_root_is_the_specs():
    for n in [0, 1, 2, 3, 4, 15, 16, 17, (1 << 32) - 1, 1 << 32, U64 - 1]:
        r = M.isqrt(n)
        assert r * r <= n < (r + 1) * (r + 1)


# ------------------------------------------------------------- the host build: arithmetic
def muldiv_edges():
    ops = [0, 1, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, U64 - 1]
    out = [(a, b, d) for a in ops for b in ops for d in (1, U64 - 1)]
    out += [(U64 - 1, U64 - 1, U64 - 1), (U64 - 1, 3, 3), (1 << 63, 2, 1), (1 << 32, 1 << 32, 1),   # 2^64 - 1 and 2^64
            ((1 << 32) + 1, (1 << 32) - 1, 1), (U64 - 1, 2, 2), (1 << 63, 4, 2), (U64 - 1, U64 - 1, U64 - 2)]
    return out


def isqrt_edges():
    out = [0, 1, 2, 3, U64 - 1, U64 - 2]
    for k in list(range((1 << 16) - 2, (1 << 16) + 3)) + list(range((1 << 32) - 3, 1 << 32)):
        out += [k * k - 1, k * k, k * k + 1]
    return [n for n in out if 0 <= n < U64]


def random_triples(count, seed=0xD17):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        a, b = rng.getrandbits(rng.choice([8, 32, 33, 64])), rng.getrandbits(rng.choice([8, 32, 33, 64]))
        out.append((a, b, max(1, rng.getrandbits(rng.choice([1, 31, 33, 64])))))
    return out


def model_muldiv(a, b, d):
    o = M.Count()
    return M.mul_div(a, b, d, o), o.n


def test_mul_div_edges_and_random_triples(L):
    triples = muldiv_edges() + random_triples(4000)
    assert any(a * b // d == U64 - 1 for a, b, d in triples) and any(a * b // d == U64 for a, b, d in triples)
    for a, b, d in triples:
        ovf = ctypes.c_uint32(7)
        got = L.hc_mul_div_u64(a, b, d, ctypes.byref(ovf))
        assert (got, ovf.value) == model_muldiv(a, b, d), (a, b, d)
        assert (got, ovf.value) == ((a * b // d, 0) if a * b // d < U64 else (U64 - 1, 1))


def test_square_root_edges(L):
    import math
    rng = random.Random(5)
    for n in isqrt_edges() + [rng.getrandbits(rng.choice([16, 33, 64])) for _ in range(2000)]:
        assert L.hc_isqrt_u64(n) == math.isqrt(n) == M.isqrt(n), n


# ------------------------------------------------------------- the host build: the four calls
def hc_votes(L, v):
    a = C.pack_votes(v)
    n, nc = v["n"], len(v["committees"])
    votes, cof, iprop, win = a32([7] * n), a32([7] * n), a32([0] * n), a32([7] * nc)
    idelay, wbal, cbal, tot = a64([0] * n), a64([7] * nc), a64([7] * nc), a64([7] * 3)
    rc = L.hc_epoch_votes(nc, p(a["coff"]), p(a["clen"]), p(a["shuffled"]), n, p(a["slashed"]), 1, p(a["eff"]), 8,
                          p(a["att_off"]), p(a["bits_off"]), p(a["bits"]), p(a["flags"]), p(a["delay"]), p(a["proposer"]),
                          p(a["cand"]), p(a["cand_count"]), p(votes), p(idelay), p(iprop), p(cof), p(win), p(wbal), p(cbal),
                          p(tot))
    assert rc == 0
    return {"votes": votes[:n].tolist(), "incl_delay": idelay[:n].tolist(), "incl_proposer": iprop[:n].tolist(),
            "committee_of": cof[:n].tolist(), "winner": win[:nc].tolist(), "winner_balance": wbal[:nc].tolist(),
            "committee_balance": cbal[:nc].tolist(), "totals": tot[:3].tolist()}


def hc_deltas(L, K, which, previous_epoch, finalized_epoch, total_balance, act, ext, wd, slashed, eff, balances, vo,
              n_committees=None, use_records=False):
    n = len(eff)
    nc = len(vo["winner_balance"]) if n_committees is None else n_committees
    rew, pen, new, ovf = a64([0] * n), a64([0] * n), a64(balances), a64([9])
    k = a64(K)
    args_v = [a32(vo["votes"]), a64(vo["incl_delay"]), a32(vo["incl_proposer"]), a32(vo["committee_of"]),
              a64(vo["winner_balance"]), a64(vo["committee_balance"]), a64(vo["totals"])]
    if use_records:
        rec = C.records(act, ext, wd, slashed, eff)
        fields = [p(rec, C.OFF_ACTIVATION), p(rec, C.OFF_EXIT), p(rec, C.OFF_WITHDRAWABLE), p(rec, C.OFF_EFFECTIVE), C.RECORD,
                  p(rec, C.OFF_SLASHED), C.RECORD]
    else:
        keep = [a64(act), a64(ext), a64(wd), a64(eff), np.array(list(slashed) + [0], dtype=np.uint8)]
        fields = [p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), 8, p(keep[4]), 1]
    rc = L.hc_epoch_deltas(n, *fields, p(args_v[0]), p(args_v[1]), p(args_v[2]), p(args_v[3]), nc, p(args_v[4]),
                           p(args_v[5]), p(args_v[6]), p(new), previous_epoch, finalized_epoch, total_balance, p(k), which,
                           p(rew), p(pen), p(new), p(ovf))   # new_balances aliases balances
    assert rc == 0
    return rew[:n].tolist(), pen[:n].tolist(), new[:n].tolist(), int(ovf[0])


def same_votes(got, want):
    for key in ("votes", "committee_of", "winner", "winner_balance", "committee_balance", "totals"):
        assert got[key] == want[key], key
    for i, vt in enumerate(want["votes"]):
        if vt & M.SOURCE:
            assert (got["incl_delay"][i], got["incl_proposer"][i]) == (want["incl_delay"][i], want["incl_proposer"][i])


def fixture_votes_input(case, per, cand_count):
    return {"n": case["n"], "committees": case["committees"], "atts": per, "cand_count": cand_count,
            "slashed": case["slashed"], "eff": case["effective_balances"]}


def test_host_votes_walk_matches_the_model(L, fx):
    for case in fx["cases"]:
        vo, per, cand_count, _ = M.case_votes(case)
        same_votes(hc_votes(L, fixture_votes_input(case, per, cand_count)), vo)
    for seed, (lens, n, n_atts, n_cands) in enumerate([([1], 1, [1], [1]), ([7, 8, 9], 40, [0, 1, 17], [0, 1, 5]),
                                                       ([63, 64, 65, 0], 257, [3, 2, 5, 1], [2, 0, 3, 1]),
                                                       ([255, 256, 257], 2049, [4, 4, 4], [1, 5, 2])]):
        for patterns in (C.BIT_PATTERNS, ("random",)):
            v = C.synth_votes(seed, lens, n, n_atts, n_cands, patterns, big=seed & 1, gap=seed)
            same_votes(hc_votes(L, v), M.votes(v["n"], v["committees"], v["atts"], v["cand_count"], v["slashed"], v["eff"]))


def test_host_deltas_match_the_model(L, fx):
    for case in fx["cases"]:
        vo = M.case_votes(case)[0]
        _, K = M.case_constants(fx, case)
        for which in (1, 2, 3):
            for use_records in (False, True):
                got = hc_deltas(L, K, which, case["previous_epoch"], case["finalized_epoch"], case["total_active_balance"],
                                case["activation_epochs"], case["exit_epochs"], case["withdrawable_epochs"], case["slashed"],
                                case["effective_balances"], case["balances"], vo, use_records=use_records)
                assert got == M.case_deltas(fx, case, vo, which)


def test_host_deltas_products_past_64_bits(L):
    """Totals and committee balances above 2^57: base_reward * attesting_balance passes 2^64."""
    v = C.synth_votes(3, [300, 211], 600, [3, 2], [2, 1], big=True)
    vo = M.votes(v["n"], v["committees"], v["atts"], v["cand_count"], v["slashed"], v["eff"])
    assert min(vo["totals"]) > 1 << 57 and min(vo["committee_balance"]) > 1 << 57
    act, ext, wd, _, _, bal = C.synth_registry(3, 600, 8, eff=v["eff"], slashed=v["slashed"])
    total = sum(v["eff"]) % U64
    want = M.deltas(C.MAINNET_K, 3, 8, 2, total, act, ext, wd, v["slashed"], v["eff"], bal, vo)
    root = M.isqrt(total)
    assert any(e * 32 // root // 5 * vo["totals"][0] >= U64 for e in v["eff"]) and want[3] == 0
    assert hc_deltas(L, C.MAINNET_K, 3, 8, 2, total, act, ext, wd, v["slashed"], v["eff"], bal, vo) == want


@pytest.mark.parametrize("name", sorted(C.overflow_cases()))
def test_host_deltas_overflows(L, name):
    kw = C.overflow_cases()[name]
    want = M.deltas(**kw)
    assert want[3] > 0
    assert hc_deltas(L, **kw) == want


def test_host_slashings_match_the_model(L, fx):
    def run(slashed, wd, eff, bal, cur, tp, total, length, q):
        b = a64(bal)
        s8 = np.array(list(slashed) + [0], dtype=np.uint8)
        w, e = a64(wd), a64(eff)
        assert L.hc_epoch_slashings(len(bal), p(s8), 1, p(w), p(e), 8, cur, tp, total, length, q, p(b)) == 0
        assert b[:len(bal)].tolist() == M.slashings(slashed, wd, eff, bal, cur, tp, total, length, q)
    for case in fx["cases"]:
        k, _ = M.case_constants(fx, case)
        run(case["slashed"], case["withdrawable_epochs"], case["effective_balances"], case["balances"], case["current_epoch"],
            case["total_penalties"], case["total_active_balance"], k["LATEST_SLASHED_EXIT_LENGTH"],
            k["MIN_SLASHING_PENALTY_QUOTIENT"])
    cur, length, rows = C.slashing_edges()
    sl, wd, eff, bal = (list(col) for col in zip(*rows))
    for tp, total in ((0, 0), (1, 10), (3, 10), (4, 10), (U64 - 1, U64 - 1), ((U64 - 1) // 3 + 1, U64 - 1), (5, 0)):
        run(sl, wd, eff, bal, cur, tp, total, length, 32)


def test_host_hysteresis_matches_the_model(L, fx):
    def run(bal, eff, inc, top):
        n = len(bal)
        b, e, idx, val, ch = a64(bal), a64(eff), a32([7] * n), a64([7] * n), a64([7])
        assert L.hc_effective_balances(n, p(b), p(e), 8, inc, top, p(idx), p(val), p(ch)) == 0
        assert (idx[:n].tolist(), val[:n].tolist(), int(ch[0])) == M.hysteresis(bal, eff, inc, top)
    for case in fx["cases"]:
        k, _ = M.case_constants(fx, case)
        for bal in (case["balances"], case["hysteresis"]["balances"]):
            run(bal, case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"])
    inc, top, rows = C.hysteresis_edges()
    run([r[0] for r in rows], [r[1] for r in rows], inc, top)
    run([r[0] for r in rows], [r[1] for r in rows], U64 - 1, U64 - 1)   # 3 * (increment / 2) passes 2^64
    run([r[0] for r in rows], [r[1] for r in rows], 1, U64 - 1)


# ------------------------------------------------------------- the stand-alone sanitizer program
def text(*parts):
    out = []
    for x in parts:
        out += [str(int(v)) for v in x] if isinstance(x, (list, tuple, bytes, np.ndarray)) else [str(int(x))]
    return " ".join(out)


def votes_text(v, want):
    a = C.pack_votes(v)
    n, nc, n_att = v["n"], len(v["committees"]), int(a["att_off"][-1])
    nbits = int(a["bits_off"][-1])
    return "V " + text(nc, len(a["shuffled"]), n, a["coff"], a["clen"], a["shuffled"], a["slashed"][:n], a["eff"][:n],
                       a["att_off"], n_att, a["bits_off"], nbits, a["bits"][:nbits], a["flags"][:n_att], a["delay"][:n_att],
                       a["proposer"][:n_att], a["cand"][:n_att], a["cand_count"][:nc], want["votes"], want["committee_of"],
                       want["incl_delay"], want["incl_proposer"], want["winner"], want["winner_balance"],
                       want["committee_balance"], want["totals"])


def deltas_text(K, which, previous_epoch, finalized_epoch, total_balance, act, ext, wd, slashed, eff, balances, vo, want):
    return "D " + text(len(eff), len(vo["winner_balance"]), act, ext, wd, eff, slashed, vo["votes"], vo["incl_delay"],
                       vo["incl_proposer"], vo["committee_of"], vo["winner_balance"], vo["committee_balance"], vo["totals"],
                       balances, previous_epoch, finalized_epoch, total_balance, K, which, want[0], want[1], want[2], want[3])


def test_standalone_program_under_sanitizers(fx, tmp_path):
    """The same header behind its own main, built with -fsanitize=address,undefined: the fixture
    cases and the arithmetic edges.  Nothing loaded into Python runs under a sanitizer."""
    import build_native
    exe = build_native.build_rewards_check()
    lines = []
    for a, b, d in muldiv_edges() + random_triples(300):
        lines.append("M " + text(a, b, d, *model_muldiv(a, b, d)))
    for n in isqrt_edges():
        lines.append("S " + text(n, M.isqrt(n)))
    for case in fx["cases"]:
        k, K = M.case_constants(fx, case)
        vo, per, cand_count, _ = M.case_votes(case)
        lines.append(votes_text(fixture_votes_input(case, per, cand_count), vo))
        for which in (1, 2, 3):
            kw = dict(K=K, which=which, previous_epoch=case["previous_epoch"], finalized_epoch=case["finalized_epoch"],
                      total_balance=case["total_active_balance"], act=case["activation_epochs"], ext=case["exit_epochs"],
                      wd=case["withdrawable_epochs"], slashed=case["slashed"], eff=case["effective_balances"],
                      balances=case["balances"], vo=vo)
            lines.append(deltas_text(want=M.deltas(**kw), **kw))
        b3 = M.case_deltas(fx, case, vo, 3)[2]
        args = (case["current_epoch"], case["total_penalties"], case["total_active_balance"], k["LATEST_SLASHED_EXIT_LENGTH"],
                k["MIN_SLASHING_PENALTY_QUOTIENT"])
        b4 = M.slashings(case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3, *args)
        lines.append("L " + text(case["n"], case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3,
                                 *args, b4))
        inc, top = k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"]
        lines.append("H " + text(case["n"], b4, case["effective_balances"], inc, top,
                                 *M.hysteresis(b4, case["effective_balances"], inc, top)))
    for name, kw in sorted(C.overflow_cases().items()):
        lines.append(deltas_text(want=M.deltas(**kw), **kw))
    v = C.synth_votes(11, [63, 64, 65, 4096], 4400, [3, 2, 5, 2], [2, 0, 3, 1], C.BIT_PATTERNS + ("random",), big=True, gap=3)
    lines.append(votes_text(v, M.votes(v["n"], v["committees"], v["atts"], v["cand_count"], v["slashed"], v["eff"])))
    cur, length, rows = C.slashing_edges()
    sl, wd, eff, bal = (list(col) for col in zip(*rows))
    for tp, total in ((4, 10), ((U64 - 1) // 3 + 1, U64 - 1), (5, 0)):
        lines.append("L " + text(len(rows), sl, wd, eff, bal, cur, tp, total, length, 32,
                                 M.slashings(sl, wd, eff, bal, cur, tp, total, length, 32)))
    inc, top, rows = C.hysteresis_edges()
    for step, cap in ((inc, top), (U64 - 1, U64 - 1)):
        bal, eff = [r[0] for r in rows], [r[1] for r in rows]
        lines.append("H " + text(len(rows), bal, eff, step, cap, *M.hysteresis(bal, eff, step, cap)))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.split()[:2] == [str(len(lines)), "cases,"] and " 0 failed" in run.stdout
