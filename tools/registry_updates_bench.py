#!/usr/bin/env python3
"""Times bls381_registry_updates_device at 2^20 and 2^22 validators whose 121-byte
records are resident, in two scenarios:

  quiet         an ordinary epoch: 20 ejections, 40 validators in the activation queue
  mass_deposit  n / 2 validators in the queue (eligibility epochs spread over 64 epochs), 20 ejections

Call times are device events on the launch stream around BATCH back-to-back calls of the _device
form after a warm-up, so they are warm figures: the same records are read again and again and, at
2^20 validators (127 MB), fit the last-level cache.  Kernel times are the library's own HIP events
(bls381_profile_enable, one pair per launch, summed per kernel name over a call: the thirteen
select launches are one figure) in a pass of their own.  Beside each call time: the bytes the
call must read and write, counted from the shapes (`needed_bytes`), divided by the time.
Comparison bases, both on the host over plain arrays and both including no copy: a numpy
restatement of the closed forms (`numpy_restatement`) and the g++ build of the shared header
(hc_registry_updates_threads of lib/libbls381_hostcheck.so on 16 threads, and on one, the best
of three calls each).  Every run's summary must equal the numpy restatement's.  There is no GPU fallback: without a device the tool fails.

    python tools/registry_updates_bench.py [--out profiles/registry_updates_bench.json] [--reps 10]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-specs_amd"))

import numpy as np  # noqa: E402

SIZES = (1 << 20, 1 << 22)
BATCH = 20
HOST_THREADS = 16
ETH = 10 ** 9
FAR = 2 ** 64 - 1
CUR, FIN = 1000, 998
KERNELS = ("regupd_count", "regupd_scan", "regupd_compact", "regupd_select", "regupd_apply")
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, the denominator of the shares below


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def registry(n, scenario, rng):
    elig, act = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    ext, wd = np.full(n, FAR, np.uint64), np.full(n, FAR, np.uint64)
    eff = np.full(n, 32 * ETH, np.uint64)
    exited = rng.choice(n, n // 100, replace=False)
    ext[exited] = rng.integers(CUR - 500, CUR + 8, len(exited)).astype(np.uint64)
    wd[exited] = ext[exited] + np.uint64(256)
    queue = 40 if scenario == "quiet" else n // 2
    rest = np.setdiff1d(np.arange(n), exited)
    picks = rng.choice(rest, queue + 20, replace=False)
    q, low = picks[:queue], picks[queue:]
    elig[q] = rng.integers(CUR - 64, CUR, queue).astype(np.uint64)
    act[q] = FAR
    eff[low] = 16 * ETH
    return elig, act, ext, wd, eff


def numpy_restatement(elig, act, ext, wd, eff, cur, fin, k):
    """The closed forms of DESIGN.md §7h in numpy: (indices, values, summary)."""
    n = len(eff)
    delayed_cur, delayed_fin = cur + 1 + k.activation_exit_delay, fin + 1 + k.activation_exit_delay
    far = np.uint64(FAR)
    new_elig = np.where((elig == far) & (eff >= np.uint64(k.max_effective_balance)), np.uint64(cur), elig)
    active = (act <= np.uint64(cur)) & (np.uint64(cur) < ext)
    ejected = active & (eff <= np.uint64(k.ejection_balance)) & (ext == far)
    cand = (new_elig != far) & (act >= np.uint64(delayed_fin))
    n_active = int(active.sum())
    L = max(k.min_per_epoch_churn_limit, n_active // k.churn_limit_quotient)
    has = ext != far
    M = int(ext[has].max()) if has.any() else -1
    e0, c0 = (M, int((ext == np.uint64(M)).sum())) if M >= delayed_cur else (delayed_cur, 0)
    rank = np.cumsum(ejected) - ejected
    new_ext = np.where(ejected, np.uint64(e0) + ((np.uint64(min(c0, L)) + rank.astype(np.uint64)) // np.uint64(L)), ext)
    new_wd = np.where(ejected, new_ext + np.uint64(k.min_validator_withdrawability_delay), wd)
    ci = np.flatnonzero(cand)
    if len(ci) > L:
        ci = ci[np.argsort(new_elig[ci], kind="stable")[:L]]
    new_act = act.copy()
    take = ci[act[ci] == far]
    new_act[take] = delayed_cur
    values = np.stack([new_elig, new_act, new_ext, new_wd], axis=1)
    changed = (new_elig != elig) | (new_act != act) | (new_ext != ext) | (new_wd != wd)
    indices = np.where(changed, np.arange(n, dtype=np.uint32), np.uint32(0xFFFFFFFF))
    summary = [int((new_elig != elig).sum()), int(ejected.sum()), int((new_act != act).sum()), int(changed.sum()), n_active, L,
               e0, 0]
    return indices, values, summary, int(cand.sum())


def needed_bytes(n, K):
    """count: five fields read, two ballots per 64 validators written; compact: the ballots, and per
    candidate two fields read, key and index written; select: twelve passes over the K (key, index)
    pairs; apply: five fields and the ballots read, an index and four epochs written."""
    return n * 40 + n // 4 + n // 8 + K * (16 + 12) + 12 * K * 12 + n * 40 + n // 8 + n * 36


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registry_updates_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import build_native
    from bls381_amd import _native, registry_updates as RU
    _native.init(0)
    L = _native.lib()
    H = ctypes.CDLL(build_native.build_hostcheck())
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    H.hc_registry_updates_threads.argtypes = [u64, vp, vp, vp, vp, vp, ctypes.c_size_t, u64, u64, vp, ctypes.c_uint32, vp, vp, vp]
    H.hc_registry_updates_threads.restype = ctypes.c_int
    k = RU.MAINNET
    k6 = np.array([getattr(k, name) for name, _ in k._fields_], dtype=np.uint64)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    result = {"record_stride": RU.RECORD, "batch": BATCH, "hbm_peak_GBs": HBM_PEAK_GBS, "current_epoch": CUR,
              "finalized_epoch": FIN, "host_threads": HOST_THREADS,
              "timing": "call: device events around %d back-to-back _device calls on resident records (warm); kernel: the "
                        "library's HIP events per launch, summed per kernel name over one call, in a pass of their own; "
                        "numpy: wall time of one call over plain host arrays; host build: the best of three calls" % BATCH, "runs": []}
    for n in SIZES:
        for scenario in ("quiet", "mass_deposit"):
            rng = np.random.default_rng(n + len(scenario))
            cols = registry(n, scenario, rng)
            t0 = time.perf_counter()
            want_idx, want_val, want_summary, K = numpy_restatement(*cols, CUR, FIN, k)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            h_idx, h_val, h_sum = np.zeros(n, np.uint32), np.zeros(4 * n, np.uint64), np.zeros(8, np.uint64)
            host_ms = {}
            for threads in (HOST_THREADS, 1):
                times = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    assert H.hc_registry_updates_threads(n, *[p(c) for c in cols], 8, CUR, FIN, p(k6), threads, p(h_idx), p(h_val),
                                                         p(h_sum)) == 0
                    times.append((time.perf_counter() - t0) * 1e3)
                host_ms[threads] = min(times)
                assert [int(x) for x in h_sum] == want_summary and np.array_equal(h_idx, want_idx)
            rec = rng.integers(0, 256, size=(n, RU.RECORD), dtype=np.uint8)
            for off, col in zip((RU.OFF_ELIGIBILITY, RU.OFF_ACTIVATION, RU.OFF_EXIT, RU.OFF_WITHDRAWABLE, RU.OFF_EFFECTIVE), cols):
                rec[:, off:off + 8] = col.astype("<u8").view(np.uint8).reshape(n, 8)
            d_rec = torch.from_numpy(rec.reshape(-1)).to("cuda")
            q = d_rec.data_ptr()
            zeros = lambda nbytes: torch.zeros(max(1, int(nbytes)), dtype=torch.uint8, device="cuda")   # noqa: E731
            d_idx, d_val, d_sum = zeros(4 * n), zeros(32 * n), zeros(64)
            ws = zeros(L.bls381_registry_updates_workspace_size(n))

            def call():
                _native.check(L.bls381_registry_updates_device(
                    n, q + RU.OFF_ELIGIBILITY, q + RU.OFF_ACTIVATION, q + RU.OFF_EXIT, q + RU.OFF_WITHDRAWABLE, q + RU.OFF_EFFECTIVE,
                    RU.RECORD, CUR, FIN, ctypes.byref(k), d_idx.data_ptr(), d_val.data_ptr(), d_sum.data_ptr(), ws.data_ptr(),
                    stream()))

            call()
            call()
            torch.cuda.synchronize()
            got = [int(x) for x in np.frombuffer(d_sum.cpu().numpy().tobytes(), np.uint64)]
            assert got == want_summary, (got, want_summary)
            assert np.array_equal(np.frombuffer(d_idx.cpu().numpy().tobytes(), np.uint32), want_idx)
            assert np.array_equal(np.frombuffer(d_val.cpu().numpy().tobytes(), np.uint64).reshape(n, 4), want_val)
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BATCH):
                    call()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) / BATCH)
            L.bls381_profile_enable(1)
            read = lambda: {name: (v["count"], v["total_ms"]) for name, v in _native.profile_read().items()}   # noqa: E731
            per = {}
            for _ in range(args.reps):
                before = read()
                call()
                torch.cuda.synchronize()
                after = read()
                for name in KERNELS:
                    if name in after:
                        per.setdefault(name, []).append(after[name][1] - before.get(name, (0, 0.0))[1])
            L.bls381_profile_enable(0)
            need = needed_bytes(n, K)
            row = {"validators": n, "scenario": scenario, "candidates": K, "summary": want_summary, "ms": spread(times),
                   "needed_bytes": need, "kernels_ms": {name: spread(v) for name, v in per.items()},
                   "numpy_ms": numpy_ms, "host_build_ms": host_ms[HOST_THREADS], "host_build_one_thread_ms": host_ms[1]}
            row["GBs"] = need / (row["ms"]["median"] * 1e-3) / 1e9
            row["share_of_hbm_peak"] = row["GBs"] / HBM_PEAK_GBS
            result["runs"].append(row)
            print(json.dumps(row), flush=True)
            del d_rec, d_idx, d_val, ws
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
