"""Epoch rewards on the device: bls381_epoch_votes, bls381_epoch_deltas,
bls381_epoch_slashings, bls381_effective_balances in both forms and their Python front
(bls381_amd/rewards.py) against tests/golden/epoch_rewards.json and rewards_model.py, then records
-> trees -> active indices -> shuffle -> votes -> deltas -> slashings -> effective balances -> tree
updates on device buffers.  CPU half: test_rewards_host.py."""
import ctypes
import random
import types

import numpy as np
import pytest

import rewards_cases as C
import rewards_model as M

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of 0xEE behind every device output
U64 = 1 << 64


def cvp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def R(native):
    from bls381_amd import rewards
    return rewards


@pytest.fixture(scope="module")
def fx():
    return M.fixture()


@pytest.fixture(scope="module")
def dev(native):
    import torch

    class Dev:
        device = torch.device("cuda:0")
        L = native.lib()

        @staticmethod
        def stream():
            return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        @staticmethod
        def up(arr):
            return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).copy()).to(Dev.device)

        @staticmethod
        def out(nbytes):
            """nbytes of output with GUARD bytes behind them, all 0xEE."""
            return torch.full((int(nbytes) + GUARD,), 0xEE, dtype=torch.uint8, device=Dev.device)

        @staticmethod
        def down(t, nbytes, dtype):
            """The first nbytes as dtype; everything behind them is still 0xEE."""
            torch.cuda.synchronize()
            raw = t.cpu().numpy()
            assert np.all(raw[int(nbytes):] == 0xEE), "written past the output"
            return np.frombuffer(raw[:int(nbytes)].tobytes(), dtype=dtype).tolist()

    return Dev


@pytest.fixture(scope="module")
def fixture_votes(fx):
    """The model's votes of every fixture state, computed once."""
    return [M.case_votes(case) for case in fx["cases"]]


# ------------------------------------------------------------------ the calls on device buffers
def fields_on_device(dev, act, ext, wd, slashed, eff, use_records):
    """The five field pointers, the uint64 stride, the slashed stride, and the tensors to keep."""
    if use_records:
        rec = dev.up(C.records(act, ext, wd, slashed, eff))
        q = rec.data_ptr()
        return {"act": q + C.OFF_ACTIVATION, "ext": q + C.OFF_EXIT, "wd": q + C.OFF_WITHDRAWABLE, "eff": q + C.OFF_EFFECTIVE,
                "stride": C.RECORD, "slashed": q + C.OFF_SLASHED, "sstride": C.RECORD, "keep": [rec]}
    keep = [dev.up(np.array(list(x) + [0], dtype=np.uint64)) for x in (act, ext, wd, eff)]
    keep.append(dev.up(np.array(list(slashed) + [0], dtype=np.uint8)))
    return {"act": keep[0].data_ptr(), "ext": keep[1].data_ptr(), "wd": keep[2].data_ptr(), "eff": keep[3].data_ptr(),
            "stride": 8, "slashed": keep[4].data_ptr(), "sstride": 1, "keep": keep}


def dev_votes(dev, v, use_records=False):
    L = dev.L
    a = C.pack_votes(v)
    n, nc = v["n"], len(v["committees"])
    n_att = int(a["att_off"][-1])
    zeros = [0] * n
    f = fields_on_device(dev, zeros, zeros, zeros, v["slashed"], v["eff"], use_records)
    d_sh = dev.up(np.append(a["shuffled"], np.uint32(0)))
    o = {"votes": dev.out(4 * n), "incl_delay": dev.out(8 * n), "incl_proposer": dev.out(4 * n), "committee_of": dev.out(4 * n),
         "winner": dev.out(4 * nc), "winner_balance": dev.out(8 * nc), "committee_balance": dev.out(8 * nc),
         "totals": dev.out(24)}
    ws = dev.out(L.bls381_epoch_votes_workspace_size(nc, n_att, int(a["bits_off"][-1])))
    rc = L.bls381_epoch_votes_device(
        nc, cvp(a["coff"]), cvp(a["clen"]), d_sh.data_ptr(), len(a["shuffled"]), n, f["slashed"], f["sstride"], f["eff"],
        f["stride"], cvp(a["att_off"]), cvp(a["bits_off"]), cvp(a["bits"]), cvp(a["flags"]), cvp(a["delay"]),
        cvp(a["proposer"]), cvp(a["cand"]), cvp(a["cand_count"]), o["votes"].data_ptr(), o["incl_delay"].data_ptr(),
        o["incl_proposer"].data_ptr(), o["committee_of"].data_ptr(), o["winner"].data_ptr(), o["winner_balance"].data_ptr(),
        o["committee_balance"].data_ptr(), o["totals"].data_ptr(), ws.data_ptr(), dev.stream())
    assert rc == 0
    sizes = {"votes": (4 * n, np.uint32), "incl_delay": (8 * n, np.uint64), "incl_proposer": (4 * n, np.uint32),
             "committee_of": (4 * n, np.uint32), "winner": (4 * nc, np.uint32), "winner_balance": (8 * nc, np.uint64),
             "committee_balance": (8 * nc, np.uint64), "totals": (24, np.uint64)}
    return {k: dev.down(o[k], *sizes[k]) for k in o}


def host_votes(R, v):
    a = C.pack_votes(v)
    n, n_att = v["n"], int(a["att_off"][-1])
    out = R.epoch_votes(a["coff"], a["clen"], a["shuffled"], a["slashed"][:n], a["eff"][:n], a["att_off"], a["bits_off"],
                        a["bits"][:int(a["bits_off"][-1])].tobytes(), a["flags"][:n_att], a["delay"][:n_att],
                        a["proposer"][:n_att], a["cand"][:n_att], a["cand_count"][:len(v["committees"])])
    return {k: x.tolist() for k, x in out.items()}


def same_votes(got, want):
    for key in ("votes", "committee_of", "winner", "winner_balance", "committee_balance", "totals"):
        assert got[key] == want[key], key
    for i, vt in enumerate(want["votes"]):
        if vt & M.SOURCE:
            assert (got["incl_delay"][i], got["incl_proposer"][i]) == (want["incl_delay"][i], want["incl_proposer"][i])


def model_votes(v):
    return M.votes(v["n"], v["committees"], v["atts"], v["cand_count"], v["slashed"], v["eff"])


def dev_deltas(dev, K, which, previous_epoch, finalized_epoch, total_balance, act, ext, wd, slashed, eff, balances, vo,
               n_committees=None, use_records=False, alias=False):
    """(rewards, penalties, new_balances, status) of the device form."""
    L = dev.L
    n = len(eff)
    nc = len(vo["winner_balance"]) if n_committees is None else n_committees
    f = fields_on_device(dev, act, ext, wd, slashed, eff, use_records)
    u64a = lambda x: dev.up(np.array(list(x) + [0], dtype=np.uint64))   # noqa: E731
    u32a = lambda x: dev.up(np.array(list(x) + [0], dtype=np.uint32))   # noqa: E731
    d_votes, d_delay, d_prop, d_cof = u32a(vo["votes"]), u64a(vo["incl_delay"]), u32a(vo["incl_proposer"]), u32a(vo["committee_of"])
    d_wb, d_cb, d_tot, d_total = u64a(vo["winner_balance"]), u64a(vo["committee_balance"]), u64a(vo["totals"]), u64a([total_balance])
    d_bal = dev.out(8 * n)
    d_bal[:8 * n] = dev.up(np.array(balances, dtype=np.uint64))[:8 * n]
    d_rew, d_pen, d_status = dev.out(8 * n), dev.out(8 * n), dev.out(8)
    d_new = d_bal if alias else dev.out(8 * n)
    ws = dev.out(L.bls381_epoch_deltas_workspace_size(n))
    k = R_constants(K)
    rc = L.bls381_epoch_deltas_device(
        n, f["act"], f["ext"], f["wd"], f["eff"], f["stride"], f["slashed"], f["sstride"], d_votes.data_ptr(), d_delay.data_ptr(),
        d_prop.data_ptr(), d_cof.data_ptr(), nc, d_wb.data_ptr(), d_cb.data_ptr(), d_tot.data_ptr(), d_bal.data_ptr(),
        previous_epoch, finalized_epoch, d_total.data_ptr(), ctypes.byref(k), which, d_rew.data_ptr(), d_pen.data_ptr(),
        d_new.data_ptr(), d_status.data_ptr(), ws.data_ptr(), dev.stream())
    assert rc == 0
    if not alias:
        assert dev.down(d_bal, 8 * n, np.uint64) == list(balances)   # the input is left alone
    return (dev.down(d_rew, 8 * n, np.uint64), dev.down(d_pen, 8 * n, np.uint64), dev.down(d_new, 8 * n, np.uint64),
            dev.down(d_status, 8, np.uint64)[0])


def R_constants(K):
    from bls381_amd import rewards
    return rewards.RewardConstants(*[int(x) for x in K])


def host_deltas(native, K, which, previous_epoch, finalized_epoch, total_balance, act, ext, wd, slashed, eff, balances, vo,
                n_committees=None):
    """(rewards, penalties, new_balances, overflows) of the host-pointer form."""
    n = len(eff)
    nc = len(vo["winner_balance"]) if n_committees is None else n_committees
    a64 = lambda x: np.array(list(x) + [0], dtype=np.uint64)   # noqa: E731
    a32 = lambda x: np.array(list(x) + [0], dtype=np.uint32)   # noqa: E731
    keep = [a64(act), a64(ext), a64(wd), a64(eff), np.array(list(slashed) + [0], dtype=np.uint8), a32(vo["votes"]),
            a64(vo["incl_delay"]), a32(vo["incl_proposer"]), a32(vo["committee_of"]), a64(vo["winner_balance"]),
            a64(vo["committee_balance"]), a64(vo["totals"]), a64(balances)]
    rew, pen, new, ovf = a64([0] * n), a64([0] * n), a64([0] * n), ctypes.c_uint64(99)
    k = R_constants(K)
    native.check(native.lib().bls381_epoch_deltas(
        n, cvp(keep[0]), cvp(keep[1]), cvp(keep[2]), cvp(keep[3]), 8, cvp(keep[4]), 1, cvp(keep[5]), cvp(keep[6]), cvp(keep[7]),
        cvp(keep[8]), nc, cvp(keep[9]), cvp(keep[10]), cvp(keep[11]), cvp(keep[12]), previous_epoch, finalized_epoch,
        total_balance, ctypes.byref(k), which, cvp(rew), cvp(pen), cvp(new), ctypes.byref(ovf)))
    return rew[:n].tolist(), pen[:n].tolist(), new[:n].tolist(), ovf.value


def dev_slashings(dev, slashed, wd, eff, balances, cur, tp, total, length, q, use_records=False):
    n = len(eff)
    f = fields_on_device(dev, [0] * n, [0] * n, wd, slashed, eff, use_records)
    d_total = dev.up(np.array([total], dtype=np.uint64))
    d_bal = dev.out(8 * n)
    d_bal[:8 * n] = dev.up(np.array(balances, dtype=np.uint64))[:8 * n]
    assert dev.L.bls381_epoch_slashings_device(n, f["slashed"], f["sstride"], f["wd"], f["eff"], f["stride"], cur, tp,
                                               d_total.data_ptr(), length, q, d_bal.data_ptr(), dev.stream()) == 0
    return dev.down(d_bal, 8 * n, np.uint64)


def dev_hysteresis(dev, balances, eff, inc, top, use_records=False):
    n = len(eff)
    f = fields_on_device(dev, [0] * n, [0] * n, [0] * n, [0] * n, eff, use_records)
    d_bal = dev.up(np.array(list(balances) + [0], dtype=np.uint64))
    d_idx, d_val, d_ch = dev.out(4 * n), dev.out(8 * n), dev.out(8)
    assert dev.L.bls381_effective_balances_device(n, d_bal.data_ptr(), f["eff"], f["stride"], inc, top, d_idx.data_ptr(),
                                                  d_val.data_ptr(), d_ch.data_ptr(), dev.stream()) == 0
    return dev.down(d_idx, 4 * n, np.uint32), dev.down(d_val, 8 * n, np.uint64), dev.down(d_ch, 8, np.uint64)[0]


# ------------------------------------------------------------------------------- the fixture
def fixture_votes_input(case, per, cand_count):
    return {"n": case["n"], "committees": case["committees"], "atts": per, "cand_count": cand_count,
            "slashed": case["slashed"], "eff": case["effective_balances"]}


def test_fixture_votes_both_forms(dev, R, fx, fixture_votes):
    for case, (vo, per, cand_count, _) in zip(fx["cases"], fixture_votes):
        v = fixture_votes_input(case, per, cand_count)
        same_votes(dev_votes(dev, v, use_records=True), vo)
        same_votes(host_votes(R, v), vo)


def test_fixture_through_the_python_front(R, fx, fixture_votes):
    """EpochVotes.from_pending_attestations and the wrappers, from the state's lists to the final
    balances and effective balances the reference's text gives."""
    for case, (vo, _, _, _) in zip(fx["cases"], fixture_votes):
        k, K = M.case_constants(fx, case)
        lens = [len(m) for m in case["committees"]]
        bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        committees = types.SimpleNamespace(shuffled=np.array([v for m in case["committees"] for v in m], dtype=np.uint32),
                                           bounds=bounds, start_shard=case["shards"][0], shard_count=k["SHARD_COUNT"],
                                           committee_count=len(lens))
        atts = [{"shard": a["shard"], "aggregation_bitfield": bytes.fromhex(a["bits"]), "inclusion_delay": a["inclusion_delay"],
                 "proposer_index": a["proposer_index"], "target": a["target"], "head": a["head"],
                 "crosslink": (a["crosslink"][0], a["crosslink"][1], a["crosslink"][2], bytes.fromhex(a["crosslink"][3]),
                               bytes.fromhex(a["crosslink"][4])),
                 "passes_filter": a["passes_filter"]} for a in case["attestations"]]
        ev = R.EpochVotes.from_pending_attestations(committees, atts, case["slashed"], case["effective_balances"])
        out = ev.run()
        same_votes({key: x.tolist() for key, x in out.items()}, vo)
        assert [max(1, int(t)) for t in out["totals"]] == case["attesting_balances"]
        for c, w in enumerate(case["winners"]):
            x = w["crosslink"]
            assert ev.winning_crosslink(c) == (x[0], x[1], x[2], bytes.fromhex(x[3]), bytes.fromhex(x[4]))
        const = R.RewardConstants.from_preset(k)
        args = (case["activation_epochs"], case["exit_epochs"], case["withdrawable_epochs"], case["effective_balances"],
                case["slashed"], out, case["balances"], case["previous_epoch"], case["finalized_epoch"],
                case["total_active_balance"], const)
        r1, p1, _ = R.epoch_deltas(*args, which=1)
        r2, p2, _ = R.epoch_deltas(*args, which=2)
        _, _, b3 = R.epoch_deltas(*args, which=3)
        assert M.matches(case["attestation_deltas"]["rewards"], r1.tolist()) and M.matches(case["attestation_deltas"]["penalties"], p1.tolist())
        assert M.matches(case["crosslink_deltas"]["rewards"], r2.tolist()) and M.matches(case["crosslink_deltas"]["penalties"], p2.tolist())
        assert M.matches(case["balances_after_rewards"], b3.tolist())
        b4 = R.epoch_slashings(case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3, case["current_epoch"],
                               case["total_penalties"], case["total_active_balance"], k["LATEST_SLASHED_EXIT_LENGTH"],
                               k["MIN_SLASHING_PENALTY_QUOTIENT"])
        assert M.matches(case["balances_after_slashings"], b4.tolist())
        idx, val, changed = R.effective_balance_updates(b4, case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"],
                                                        k["MAX_EFFECTIVE_BALANCE"])
        assert M.matches(case["effective_balances_after"], val.tolist())
        assert (idx.tolist(), val.tolist(), changed) == M.hysteresis(b4.tolist(), case["effective_balances"],
                                                                    k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"])
        h = case["hysteresis"]
        assert R.effective_balance_updates(h["balances"], case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"],
                                           k["MAX_EFFECTIVE_BALANCE"])[1].tolist() == h["effective_balances_after"]


def test_fixture_deltas_slashings_hysteresis_device_forms(dev, native, fx, fixture_votes):
    for case, (vo, _, _, _) in zip(fx["cases"], fixture_votes):
        k, K = M.case_constants(fx, case)
        kw = dict(K=K, previous_epoch=case["previous_epoch"], finalized_epoch=case["finalized_epoch"],
                  total_balance=case["total_active_balance"], act=case["activation_epochs"], ext=case["exit_epochs"],
                  wd=case["withdrawable_epochs"], slashed=case["slashed"], eff=case["effective_balances"],
                  balances=case["balances"], vo=vo)
        for which in (1, 2, 3):
            want = M.deltas(which=which, **kw)
            assert dev_deltas(dev, which=which, use_records=which != 2, **kw) == want
            assert host_deltas(native, which=which, **kw) == want
        b3 = M.deltas(which=3, **kw)[2]
        args = (case["current_epoch"], case["total_penalties"], case["total_active_balance"], k["LATEST_SLASHED_EXIT_LENGTH"],
                k["MIN_SLASHING_PENALTY_QUOTIENT"])
        b4 = M.slashings(case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3, *args)
        assert M.matches(case["balances_after_slashings"], b4)
        for use_records in (False, True):
            assert dev_slashings(dev, case["slashed"], case["withdrawable_epochs"], case["effective_balances"], b3, *args,
                                 use_records=use_records) == b4
            assert dev_hysteresis(dev, b4, case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"],
                                  use_records) == M.hysteresis(b4, case["effective_balances"], k["EFFECTIVE_BALANCE_INCREMENT"],
                                                               k["MAX_EFFECTIVE_BALANCE"])


# ----------------------------------------------------------------------------- votes: the edges
def test_votes_committee_lengths_and_bit_patterns(dev, R):
    """Lengths 1 .. 4,096 (the byte, word, wave and workgroup edges), four attestations each with
    the patterns none / all / alternating / last bit only, and five candidates."""
    lens = C.COMMITTEE_LENGTHS
    for perm in range(4):   # every pattern meets every candidate slot
        patterns = C.BIT_PATTERNS[perm:] + C.BIT_PATTERNS[:perm]
        v = C.synth_votes(40 + perm, lens, sum(lens) + 300, [4] * len(lens), [5] * len(lens), patterns, gap=perm)
        want = model_votes(v)
        same_votes(dev_votes(dev, v, use_records=perm & 1), want)
        if perm == 0:
            same_votes(host_votes(R, v), want)


def test_votes_attestation_and_candidate_counts(dev, R):
    """0, 1 and 17 attestations and 0, 1 and 5 candidates in a committee, in every pairing."""
    n_atts = [0, 1, 17, 0, 1, 17, 0, 1, 17]
    n_cands = [0, 0, 0, 1, 1, 1, 5, 5, 5]
    v = C.synth_votes(7, [65, 9, 64, 7, 257, 63, 8, 1, 255], 900, n_atts, n_cands)
    want = model_votes(v)
    assert want["winner"][:3] == [M.NONE] * 3 and all(w != M.NONE for w in want["winner"][3:])
    same_votes(dev_votes(dev, v), want)
    same_votes(host_votes(R, v), want)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2049])
def test_votes_registry_sizes_with_most_validators_in_no_committee(dev, R, n):
    lens = [1] if n == 1 else [9, 0, 17, 33]
    v = C.synth_votes(n, lens, n, [2] * len(lens), [2] * len(lens))
    want = model_votes(v)
    assert n == 1 or want["votes"].count(0) > n // 2
    same_votes(dev_votes(dev, v, use_records=n & 1), want)
    same_votes(host_votes(R, v), want)


def test_votes_and_deltas_with_sums_above_2_57(dev, native, R):
    """Totals and committee balances above 2^57: base_reward * attesting_balance passes 2^64, so a
    64-bit product would give other rewards."""
    v = C.synth_votes(3, [300, 211], 600, [3, 2], [2, 1], big=True)
    vo = model_votes(v)
    assert min(vo["totals"]) > 1 << 57 and min(vo["committee_balance"]) > 1 << 57
    got = dev_votes(dev, v)
    same_votes(got, vo)
    act, ext, wd, _, _, bal = C.synth_registry(3, 600, 8, eff=v["eff"], slashed=v["slashed"])
    total = sum(v["eff"]) % U64
    kw = dict(K=C.MAINNET_K, which=3, previous_epoch=8, finalized_epoch=2, total_balance=total, act=act, ext=ext, wd=wd,
              slashed=v["slashed"], eff=v["eff"], balances=bal, vo=vo)
    want = M.deltas(**kw)
    root = M.isqrt(total)
    wrapped = [(e * 32 // root // 5 * vo["totals"][0] % U64) // total for e in v["eff"]]
    exact = [e * 32 // root // 5 * vo["totals"][0] // total for e in v["eff"]]
    assert wrapped != exact and want[3] == 0
    assert dev_deltas(dev, **kw) == want
    assert host_deltas(native, **kw) == want


# --------------------------------------------------------------------------- deltas: the edges
@pytest.mark.parametrize("name", sorted(C.overflow_cases()))
def test_deltas_overflow_kinds(dev, native, R, name):
    """A non-zero status, every other output as the model saturates it; the front raises."""
    kw = C.overflow_cases()[name]
    want = M.deltas(**kw)
    assert want[3] > 0
    assert dev_deltas(dev, **kw) == want
    assert host_deltas(native, **kw) == want
    vo = {key: np.array(x, dtype=np.uint64 if key in ("incl_delay", "winner_balance", "committee_balance", "totals") else np.uint32)
          for key, x in kw["vo"].items()}
    with pytest.raises(OverflowError):
        R.epoch_deltas(kw["act"], kw["ext"], kw["wd"], kw["eff"], kw["slashed"], vo, kw["balances"], kw["previous_epoch"],
                       kw["finalized_epoch"], kw["total_balance"], R_constants(kw["K"]), kw["which"])


@pytest.mark.parametrize("n", [1, 257, 2049])
def test_deltas_random_registries_and_aliasing(dev, native, n):
    """Random eligibility, votes and proposers over both presets' constants, several workgroups;
    d_new_balances aliasing d_balances gives the same balances."""
    rng = random.Random(n)
    lens = [1] if n == 1 else [n // 3, n // 4, 5]
    v = C.synth_votes(n + 1, lens, n, [3] * len(lens), [2] * len(lens))
    vo = model_votes(v)
    act, ext, wd, _, _, bal = C.synth_registry(n, n, 8, eff=v["eff"], slashed=v["slashed"])
    total = max(1, sum(e for e, a, x in zip(v["eff"], act, ext) if a <= 9 < x))
    for K, fin in ((C.MAINNET_K, 3), ([32, 5, 8, 2, 4, 1 << 25], 4)):
        kw = dict(K=K, which=rng.choice([1, 2, 3]), previous_epoch=8, finalized_epoch=fin, total_balance=total, act=act,
                  ext=ext, wd=wd, slashed=v["slashed"], eff=v["eff"], balances=bal, vo=vo)
        want = M.deltas(**kw)
        assert dev_deltas(dev, use_records=True, **kw) == want
        assert dev_deltas(dev, alias=True, **kw) == want
        assert host_deltas(native, **kw) == want


def test_slashings_and_hysteresis_edges(dev, R):
    cur, length, rows = C.slashing_edges()
    sl, wd, eff, bal = (list(col) for col in zip(*rows))
    for tp, total in ((0, 0), (3, 10), (4, 10), ((U64 - 1) // 3 + 1, U64 - 1), (U64 - 1, U64 - 1)):
        want = M.slashings(sl, wd, eff, bal, cur, tp, total, length, 32)
        assert dev_slashings(dev, sl, wd, eff, bal, cur, tp, total, length, 32, use_records=True) == want
        assert R.epoch_slashings(sl, wd, eff, bal, cur, tp, total, length, 32).tolist() == want
    inc, top, rows = C.hysteresis_edges()
    b, e = [r[0] for r in rows], [r[1] for r in rows]
    for step, cap in ((inc, top), (U64 - 1, U64 - 1), (1, U64 - 1)):
        want = M.hysteresis(b, e, step, cap)
        assert dev_hysteresis(dev, b, e, step, cap) == want
        idx, val, changed = R.effective_balance_updates(b, e, step, cap)
        assert (idx.tolist(), val.tolist(), changed) == want
    n = 2049   # several workgroups, the count summed across waves
    rng = random.Random(2049)
    e = [rng.choice([0, 1, 16, 31, 32]) * C.ETH for _ in range(n)]
    b = [max(0, x + rng.choice([0, -1, 1, C.ETH, 2 * C.ETH, -C.ETH])) for x in e]
    assert dev_hysteresis(dev, b, e, C.ETH, 32 * C.ETH, use_records=True) == M.hysteresis(b, e, C.ETH, 32 * C.ETH)


# ------------------------------------------------------------------------------ arguments
def test_rejected_arguments(native, dev, R):
    L = native.lib()
    EARG = native.EARG
    v = C.synth_votes(1, [9, 8], 40, [2, 1], [1, 1])
    a = C.pack_votes(v)
    n = 40

    def votes_rc(**change):
        b = dict(a)
        b.update(change)
        out32 = [np.zeros(n + 2, np.uint32) for _ in range(4)]
        out64 = [np.zeros(n + 2, np.uint64) for _ in range(3)]
        tot = np.zeros(3, np.uint64)
        return L.bls381_epoch_votes(2, cvp(b["coff"]), cvp(b["clen"]), cvp(b["shuffled"]), len(b["shuffled"]), n, cvp(b["slashed"]),
                                    b.get("sstride", 1), cvp(b["eff"]), b.get("stride", 8), cvp(b["att_off"]), cvp(b["bits_off"]),
                                    cvp(b["bits"]), cvp(b["flags"]), cvp(b["delay"]), cvp(b["proposer"]), cvp(b["cand"]),
                                    cvp(b["cand_count"]), cvp(out32[0]), cvp(out64[0]), cvp(out32[1]), cvp(out32[2]), cvp(out32[3]),
                                    cvp(out64[1]), cvp(out64[2]), cvp(tot))
    assert votes_rc() == 0
    u32 = lambda x: np.array(x, dtype=np.uint32)   # noqa: E731
    assert votes_rc(clen=u32([9, 9])) == EARG                          # outside n_shuffled (and a bitfield of the wrong length)
    assert votes_rc(coff=u32([0, 8])) == EARG                          # overlapping slices
    assert votes_rc(clen=u32([4097, 8])) == EARG                       # above 4,096 members
    bad = a["bits"].copy()
    bad[1] |= 0x80                                                     # a padding bit of a 9-member bitfield
    assert votes_rc(bits=bad) == EARG
    assert votes_rc(bits_off=u32([0, 2, 1, 5])) == EARG                # descending
    assert votes_rc(att_off=u32([0, 3, 2])) == EARG
    assert votes_rc(flags=np.array([4, 0, 0, 0], np.uint8)) == EARG
    assert votes_rc(cand=u32([1, 0, 0, 0])) == EARG                    # at its committee's cand_count
    assert votes_rc(stride=7) == EARG and votes_rc(sstride=0) == EARG
    assert L.bls381_epoch_votes_workspace_size(1 << 31, 0, 0) == 0
    tot = np.full(3, 7, np.uint64)
    assert L.bls381_epoch_votes(0, None, None, None, 0, 0, None, 1, None, 8, None, None, None, None, None, None, None, None,
                                None, None, None, None, None, None, None, cvp(tot)) == 0 and tot.tolist() == [0, 0, 0]
    assert L.bls381_epoch_votes(0, None, None, None, 0, 0, None, 1, None, 8, None, None, None, None, None, None, None, None,
                                None, None, None, None, None, None, None, None) == EARG

    kw = C.overflow_cases()["increase"]
    ok = dict(kw, balances=[1, 1])
    assert host_deltas(native, **ok)[3] == 0
    for change in (dict(which=0), dict(which=4), dict(previous_epoch=U64 - 1), dict(finalized_epoch=9),
                   dict(K=[32, 0, 8, 1, 4, 1 << 25]), dict(K=[32, 5, 0, 1, 4, 1 << 25]), dict(K=[32, 5, 8, 1, 4, 0])):
        with pytest.raises(ValueError):
            host_deltas(native, **dict(ok, **change))
    ovf = ctypes.c_uint64(5)
    k = R_constants(C.MAINNET_K)
    none26 = [None] * 4
    assert L.bls381_epoch_deltas(0, *none26, 8, None, 1, *none26, 0, None, None, cvp(tot), None, 8, 7, 1, ctypes.byref(k), 3,
                                 None, None, None, ctypes.byref(ovf)) == 0 and ovf.value == 0
    assert L.bls381_epoch_deltas(0, *none26, 8, None, 1, *none26, 0, None, None, cvp(tot), None, 8, 7, 1, None, 3,
                                 None, None, None, ctypes.byref(ovf)) == EARG
    assert L.bls381_epoch_deltas_workspace_size(1 << 32) == 0
    one = np.ones(2, np.uint64)
    sl8 = np.ones(2, np.uint8)
    assert L.bls381_epoch_slashings(1, cvp(sl8), 1, cvp(one), cvp(one), 8, 9, 1, 1, 64, 0, cvp(one)) == EARG   # quotient 0
    assert L.bls381_epoch_slashings(1, cvp(sl8), 0, cvp(one), cvp(one), 8, 9, 1, 1, 64, 32, cvp(one)) == EARG
    assert L.bls381_epoch_slashings(0, None, 1, None, None, 8, 9, 1, 1, 64, 32, None) == 0
    ch = ctypes.c_uint64(5)
    idx = np.zeros(2, np.uint32)
    assert L.bls381_effective_balances(1, cvp(one), cvp(one), 8, 0, 32, cvp(idx), cvp(one), ctypes.byref(ch)) == EARG   # increment 0
    assert L.bls381_effective_balances(1, cvp(one), cvp(one), 8, 1, 32, cvp(idx), cvp(one), None) == EARG
    assert L.bls381_effective_balances(0, None, None, 8, 1, 32, None, None, ctypes.byref(ch)) == 0 and ch.value == 0
    # device forms: alignment
    d = dev.out(64)
    q = d.data_ptr()
    assert L.bls381_effective_balances_device(1, q, q, 8, 1, 32, q + 2, q + 16, q + 32, dev.stream()) == EARG     # d_indices
    assert L.bls381_effective_balances_device(1, q, q, 8, 1, 32, q, q + 16, q + 36, dev.stream()) == EARG         # d_changed
    assert L.bls381_epoch_slashings_device(1, q, 1, q, q, 8, 9, 1, q + 4, 64, 32, q + 8, dev.stream()) == EARG    # d_total_balance
    assert L.bls381_epoch_slashings_device(1, q, 1, q, q, 8, 9, 1, None, 64, 32, q + 8, dev.stream()) == EARG
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ the chain
def test_epoch_boundary_on_device_buffers(native, dev, R, fx):
    """A minimal-preset epoch boundary with the records in a validator_registry_tree and the
    balances in a balances_tree: active indices -> shuffle -> votes -> deltas -> slashings ->
    effective balances -> the trees' device updates.  The host reads the active count (the shuffle
    takes it as a scalar) and, at the end, the status words; both roots equal the ssz roots of the
    model's new lists."""
    import torch

    import list_tree_cases as LT
    from bls381_amd import state_tree
    L = dev.L
    k = fx["supplied"]["constants"]["minimal"]
    const = R.RewardConstants.from_preset(k)
    rng = random.Random(0xB0DA)
    n, cur, fin = 300, 9, 3
    prev = cur - 1
    half = k["LATEST_SLASHED_EXIT_LENGTH"] // 2
    act, ext, wd, sl, eff, bal = C.synth_registry(0xB0DA, n, prev)
    wd = [cur + half if s and rng.random() < 0.5 else w for s, w in zip(sl, wd)]
    rec = C.records(act, ext, wd, sl, eff, seed=5)
    items = [rec[C.RECORD * i:C.RECORD * (i + 1)].tobytes() for i in range(n)]
    sp = dev.stream()
    with state_tree.validator_registry_tree(512) as vt, state_tree.balances_tree(512) as bt:
        vt.append(items)
        bt.append([b.to_bytes(8, "little") for b in bal])
        q = vt.items_ptr
        aws = dev.out(L.bls381_active_indices_workspace_size(n))
        d_idx, d_ct_prev, d_ct_cur, d_idx_cur = dev.out(4 * n), dev.out(16), dev.out(16), dev.out(4 * n)
        for epoch, idx, ct in ((prev, d_idx, d_ct_prev), (cur, d_idx_cur, d_ct_cur)):
            native.check(L.bls381_active_indices_device(n, q + C.OFF_ACTIVATION, q + C.OFF_EXIT, C.RECORD, epoch, q + C.OFF_EFFECTIVE,
                                                        C.RECORD, idx.data_ptr(), ct.data_ptr(), aws.data_ptr(), sp))
        count = dev.down(d_ct_prev, 16, np.uint64)[0]                     # the chain's one host read before the end
        assert count == sum(1 for a, x in zip(act, ext) if a <= prev < x)
        seed, rounds = bytes(range(32)), k["SHUFFLE_ROUND_COUNT"]
        d_sh = dev.out(4 * count)
        sws = dev.out(L.bls381_shuffle_workspace_size(count, count, rounds))
        native.check(L.bls381_shuffle_device(count, seed, rounds, 0, count, d_idx.data_ptr(), d_sh.data_ptr(), sws.data_ptr(), sp))
        from bls381_amd import epoch as E
        ncom = E.epoch_committee_count(count, k["SHARD_COUNT"], k["SLOTS_PER_EPOCH"], k["TARGET_COMMITTEE_SIZE"])
        bounds = [(count * j) // ncom for j in range(ncom + 1)]
        lens = [bounds[j + 1] - bounds[j] for j in range(ncom)]
        # attestations by committee length alone: the members are not known on the host
        per = []
        for c, m in enumerate(lens):
            links = [(c, 2, prev, bytes([c + 1]) * 32, bytes([r]) * 32) for r in (9, 3, 3)]
            links[2] = links[2][:3] + (bytes(32), links[2][4])
            mine = []
            for a in range(c % 4):
                bits = C.pattern_bits("random", m, rng)
                mine.append({"bits": C.bitfield(bits), "target": rng.random() < 0.7, "head": rng.random() < 0.5,
                             "inclusion_delay": rng.choice([2, 2, 3, 5]), "proposer_index": rng.randrange(n),
                             "crosslink": links[(a + c) % 3], "passes_filter": (a + c) % 3 != 1 or c % 2 == 0})
            per.append(mine)
        ev = R.EpochVotes(np.zeros(0, np.uint32), bounds[:-1], lens, sl, eff, per)
        dv = ev.run_device(vt, d_sh.data_ptr(), count)
        d_total = d_ct_cur.data_ptr() + 8
        total_penalties = 5 * C.ETH
        status = R.process_rewards_and_penalties(bt, vt, dv, cur, fin, d_total, const)
        R.process_slashings(bt, vt, cur, total_penalties, d_total, k["LATEST_SLASHED_EXIT_LENGTH"], k["MIN_SLASHING_PENALTY_QUOTIENT"])
        changed = R.update_effective_balances(bt, vt, k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"])
        torch.cuda.synchronize()
        # the model over the committees the device shuffled
        shuffled = dev.down(d_sh, 4 * count, np.uint32)
        assert sorted(shuffled) == [i for i, (a, x) in enumerate(zip(act, ext)) if a <= prev < x]
        committees = [shuffled[bounds[j]:bounds[j + 1]] for j in range(ncom)]
        atts = [[{"bits": a["bits"], "flags": int(a["target"]) | int(a["head"]) << 1, "delay": a["inclusion_delay"],
                  "proposer": a["proposer_index"], "cand": int(ev.cand[ev.att_off[c] + t])} for t, a in enumerate(mine)]
                for c, mine in enumerate(per)]
        for c, mine in enumerate(per):   # the front's candidate ids are the model's
            assert [x["cand"] for x in atts[c]] == M.assign_candidates(mine)[0]
        vo = M.votes(n, committees, atts, ev.cand_count.tolist(), sl, eff)
        total = sum(e for e, a, x in zip(eff, act, ext) if a <= cur < x)
        _, _, b3, ovf = M.deltas([k[name] for name in M.CONSTANT_NAMES], 3, prev, fin, total, act, ext, wd, sl, eff, bal, vo)
        assert status == ovf == 0 and b3 != bal
        b4 = M.slashings(sl, wd, eff, b3, cur, total_penalties, total, k["LATEST_SLASHED_EXIT_LENGTH"],
                         k["MIN_SLASHING_PENALTY_QUOTIENT"])
        assert b4 != b3
        idx, val, want_changed = M.hysteresis(b4, eff, k["EFFECTIVE_BALANCE_INCREMENT"], k["MAX_EFFECTIVE_BALANCE"])
        assert changed == want_changed > 0
        LT.apply_update(items, range(n), C.OFF_EFFECTIVE, 8, [v.to_bytes(8, "little") for v in val])
        assert bt.root() == LT.Model(LT.UINT64, [b.to_bytes(8, "little") for b in b4]).root(True)
        assert vt.root() == LT.Model(LT.VALIDATOR, items).root(True)
        assert vt.read(0, n) == items
        # GENESIS_EPOCH returns early, as in the spec
        assert R.process_rewards_and_penalties(bt, vt, dv, 0, 0, d_total, const) == 0
        assert bt.root() == LT.Model(LT.UINT64, [b.to_bytes(8, "little") for b in b4]).root(True)
