#!/usr/bin/env python3
"""Times the four epoch-rewards device calls at 2^20 validators in mainnet shape:
1,024 committees of 1,024 members, about 8 attestations per committee, the validator records
(121 bytes) and every other array in device memory.

Call times are device events on the launch stream around BATCH back-to-back calls of the _device
form (host planning and the descriptor copies of bls381_epoch_votes_device included), after a
warm-up; kernel times are the library's own HIP events (bls381_profile_enable, one pair per
launch, read per kernel name) in a pass of their own.  Beside each time: the bytes the call must
read and write, counted from the shapes (the fields it needs, not the whole records; the
formulas are in `needed_bytes`), divided by the time.  There is no GPU fallback: without a
device the tool fails.

    python tools/epoch_rewards_bench.py [--out profiles/epoch_rewards_bench.json] [--reps 10]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-specs_amd"))

import numpy as np  # noqa: E402

NC, CS, ATTS = 1024, 1024, 8
N = NC * CS
BATCH = 20
ETH = 10 ** 9
KERNELS = ("votes_clear", "votes_committees", "votes_totals", "epoch_deltas", "epoch_deltas_apply", "epoch_slashings",
           "effective_balances")
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, the denominator of the shares below


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def needed_bytes(n, n_att, bitfield_bytes, sources, slashed_count, due):
    """Bytes each call must move, from the shapes.  votes: the shuffled list (4), slashed (1) and
    effective_balance (8) per member, the bitfields once per pass over them (source/target/head
    and each candidate), the descriptors; writes votes and committee_of twice (the clear, then the
    walk) and 12 bytes per source attester.  deltas: four uint64 fields, slashed, votes, delay,
    proposer, committee_of, balances read; rewards, penalties written, the proposer buffer zeroed;
    then balances, rewards, penalties, proposer rewards read and rewards, new balances written;
    one 8-byte atomic per source attester.  slashings: the flag of everyone, 16 bytes of fields and
    16 of balance for the slashed.  effective balances: balance and field read, index and value
    written."""
    return {"epoch_votes": n * 13 + 3 * bitfield_bytes + 24 * n_att + 2 * n * 8 + 12 * sources,
            "epoch_deltas": n * (32 + 1 + 4 + 8 + 4 + 4 + 8) + n * 24 + n * 32 + n * 16 + 8 * sources,
            "epoch_slashings": n + 16 * slashed_count + 16 * due,
            "effective_balances": n * 28}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_rewards_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    from bls381_amd import _native, rewards as R
    _native.init(0)
    L = _native.lib()
    rng = np.random.default_rng(0xE90C4)
    cur, prev, fin = 9, 8, 3
    slashed = (rng.random(N) < 0.01).astype(np.uint8)
    eff = rng.choice(np.array([32, 32, 32, 31, 24, 16], dtype=np.uint64), N) * np.uint64(ETH)
    wd = np.where(slashed != 0, rng.choice(np.array([cur + 4096, cur + 5000], dtype=np.uint64), N), np.uint64(2 ** 64 - 1))
    rec = rng.integers(0, 256, size=(N, R.RECORD), dtype=np.uint8)
    for off, col in ((R.OFF_ACTIVATION, np.zeros(N, np.uint64)), (R.OFF_EXIT, np.full(N, 2 ** 64 - 1, np.uint64)),
                     (R.OFF_WITHDRAWABLE, wd), (R.OFF_EFFECTIVE, eff)):
        rec[:, off:off + 8] = col.astype("<u8").view(np.uint8).reshape(N, 8)
    rec[:, R.OFF_SLASHED] = slashed
    bal = eff + rng.integers(0, 3 * ETH, N).astype(np.uint64)
    shuffled = rng.permutation(N).astype(np.uint32)
    coff, clen = np.arange(0, N, CS, dtype=np.uint32), np.full(NC, CS, dtype=np.uint32)
    n_att = NC * ATTS
    att_off = np.arange(0, n_att + 1, ATTS, dtype=np.uint32)
    bits_off = np.arange(0, (n_att + 1) * (CS // 8), CS // 8, dtype=np.uint32)
    bits = (rng.integers(0, 256, n_att * CS // 8, dtype=np.uint8) & rng.integers(0, 256, n_att * CS // 8, dtype=np.uint8))
    flags = rng.integers(0, 4, n_att).astype(np.uint8)
    delay = rng.integers(1, 33, n_att).astype(np.uint64)
    proposer = rng.integers(0, N, n_att).astype(np.uint32)
    cand = rng.integers(0, 2, n_att).astype(np.uint32)
    cand_count = np.full(NC, 2, dtype=np.uint32)

    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda")   # noqa: E731
    zeros = lambda nbytes: torch.zeros(max(1, int(nbytes)), dtype=torch.uint8, device="cuda")       # noqa: E731
    d_rec, d_sh, d_bal0 = up(rec.reshape(-1)), up(shuffled), up(bal)
    q = d_rec.data_ptr()
    d_votes, d_delay, d_prop, d_cof = zeros(4 * N), zeros(8 * N), zeros(4 * N), zeros(4 * N)
    d_win, d_wbal, d_cbal, d_tot = zeros(4 * NC), zeros(8 * NC), zeros(8 * NC), zeros(24)
    d_total = up(np.array([int(eff.sum())], dtype=np.uint64))
    d_rew, d_pen, d_new, d_status = zeros(8 * N), zeros(8 * N), zeros(8 * N), zeros(8)
    d_idx, d_val, d_changed = zeros(4 * N), zeros(8 * N), zeros(8)
    vws = zeros(L.bls381_epoch_votes_workspace_size(NC, n_att, int(bits_off[-1])))
    dws = zeros(L.bls381_epoch_deltas_workspace_size(N))
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731

    def votes():
        _native.check(L.bls381_epoch_votes_device(
            NC, p(coff), p(clen), d_sh.data_ptr(), N, N, q + R.OFF_SLASHED, R.RECORD, q + R.OFF_EFFECTIVE, R.RECORD, p(att_off),
            p(bits_off), p(bits), p(flags), p(delay), p(proposer), p(cand), p(cand_count), d_votes.data_ptr(), d_delay.data_ptr(),
            d_prop.data_ptr(), d_cof.data_ptr(), d_win.data_ptr(), d_wbal.data_ptr(), d_cbal.data_ptr(), d_tot.data_ptr(),
            vws.data_ptr(), stream()))

    def deltas():
        _native.check(L.bls381_epoch_deltas_device(
            N, q + R.OFF_ACTIVATION, q + R.OFF_EXIT, q + R.OFF_WITHDRAWABLE, q + R.OFF_EFFECTIVE, R.RECORD, q + R.OFF_SLASHED,
            R.RECORD, d_votes.data_ptr(), d_delay.data_ptr(), d_prop.data_ptr(), d_cof.data_ptr(), NC, d_wbal.data_ptr(),
            d_cbal.data_ptr(), d_tot.data_ptr(), d_bal0.data_ptr(), prev, fin, d_total.data_ptr(), ctypes.byref(R.MAINNET), 3,
            d_rew.data_ptr(), d_pen.data_ptr(), d_new.data_ptr(), d_status.data_ptr(), dws.data_ptr(), stream()))

    def slashings():
        _native.check(L.bls381_epoch_slashings_device(N, q + R.OFF_SLASHED, R.RECORD, q + R.OFF_WITHDRAWABLE, q + R.OFF_EFFECTIVE,
                                                      R.RECORD, cur, 100000 * ETH, d_total.data_ptr(), 8192, 32,
                                                      d_new.data_ptr(), stream()))

    def effective():
        _native.check(L.bls381_effective_balances_device(N, d_new.data_ptr(), q + R.OFF_EFFECTIVE, R.RECORD, ETH, 32 * ETH,
                                                         d_idx.data_ptr(), d_val.data_ptr(), d_changed.data_ptr(), stream()))

    calls = (("epoch_votes", votes), ("epoch_deltas", deltas), ("epoch_slashings", slashings), ("effective_balances", effective))
    for _, fn in calls:     # warm-up, in the order of the chain: each call's inputs are the one before's outputs
        fn()
        fn()
    torch.cuda.synchronize()
    votes_host = np.frombuffer(d_votes.cpu().numpy().tobytes(), dtype=np.uint32)
    sources = int((votes_host & 1).sum())
    assert int((votes_host & 16).sum()) == 16 * N and int(np.frombuffer(d_status.cpu().numpy().tobytes(), np.uint64)[0]) == 0
    due = int(((slashed != 0) & (wd == cur + 4096)).sum())
    need = needed_bytes(N, n_att, int(bits_off[-1]), sources, int(slashed.sum()), due)
    result = {"validators": N, "committees": NC, "committee_size": CS, "attestations": n_att, "source_attesters": sources,
              "record_stride": R.RECORD, "batch": BATCH, "hbm_peak_GBs": HBM_PEAK_GBS,
              "timing": "call: device events around %d back-to-back _device calls; kernel: the library's HIP events per "
                        "launch, in a pass of their own" % BATCH, "calls": {}, "kernels": {}}
    for name, fn in calls:
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(BATCH):
                fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) / BATCH)
        row = {"ms": spread(times), "needed_bytes": need[name]}
        row["GBs"] = need[name] / (row["ms"]["median"] * 1e-3) / 1e9
        row["share_of_hbm_peak"] = row["GBs"] / HBM_PEAK_GBS
        result["calls"][name] = row
        print(name, json.dumps(row), flush=True)
    L.bls381_profile_enable(1)
    read = lambda: {k: (v["count"], v["total_ms"]) for k, v in _native.profile_read().items()}   # noqa: E731
    per = {}
    for _ in range(args.reps):
        for _, fn in calls:
            before = read()
            fn()
            torch.cuda.synchronize()
            after = read()
            for k in KERNELS:
                if k in after and after[k][0] > before.get(k, (0, 0.0))[0]:
                    per.setdefault(k, []).append(after[k][1] - before.get(k, (0, 0.0))[1])
    L.bls381_profile_enable(0)
    result["kernels"] = {k + "_ms": spread(v) for k, v in per.items()}
    print("kernels", json.dumps(result["kernels"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
