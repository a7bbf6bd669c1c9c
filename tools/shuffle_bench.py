#!/usr/bin/env python3
"""Times the committee stages on the GPU: the shuffle and the attesting entries.

Kernel times are the library's own HIP events on the launch stream (bls381_profile_enable, one
pair per launch, read per kernel name); call times are a host clock around the host-pointer entry
points, which end in a stream synchronise and include their copies.  Three parts:

  full      bls381_shuffle of the whole list, 90 rounds, n = 2^18, 2^20, 2^22: table build
            (shuffle_table), walk (shuffle_walk), pivots, and the call.
  epoch     1,024 committees x 128: the shuffle of the 131,072 active indices with the gather,
            then bls381_attesting_entries over 1,024 attestations with random bitfields.
  boundary  the window count = ceil(n / 256) at n = 2^20 through each path, then small and
            boundary windows of lists up to 2^26.  The path is fixed per process
            (BLS381_SHUFFLE_PATH), so each side runs in child processes, alternating.

The comparison base is the same header's host build (libbls381_hostcheck.so hc_shuffle_list) on 16
threads.  There is no GPU fallback: without a device the tool fails.

    python tools/shuffle_bench.py [--out profiles/shuffle_bench.json] [--reps 10] [--skip-host]
    rocprofv3 --pmc ... -- python tools/shuffle_bench.py --one 22     (tools/pmc_summary.py reads the passes)
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-specs_amd"))

import numpy as np  # noqa: E402

ROUNDS = 90
SEED = hashlib.sha256(b"shuffle_bench").digest()
EPOCH_MS = 7.6          # the grouped-registry verify of 1,024 attestations (README.md), the yardstick
KERNELS = ("shuffle_pivots", "shuffle_table", "shuffle_walk", "shuffle_direct", "attesting_entries")


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


class Engine:
    def __init__(self):
        from bls381_amd import _native
        _native.init(0)
        self.native = _native
        self.L = _native.lib()
        self.L.bls381_profile_enable(1)
        self.seen = self.read()

    def read(self):
        return {k: (v["count"], v["total_ms"]) for k, v in self.native.profile_read().items()}

    def timed(self, fn, reps, warmup=2):
        """fn() `reps` times after `warmup`: call times (ms) and per-kernel times (ms per launch)."""
        for _ in range(warmup):
            fn()
        calls, kernels = [], {}
        for _ in range(reps):
            before = self.read()
            t0 = time.perf_counter()
            fn()
            calls.append((time.perf_counter() - t0) * 1e3)
            after = self.read()
            for k in KERNELS:
                if k in after and after[k][0] > before.get(k, (0, 0.0))[0]:
                    kernels.setdefault(k, []).append(after[k][1] - before.get(k, (0, 0.0))[1])
        out = {"call_ms": spread(calls)}
        out.update({k + "_ms": spread(v) for k, v in kernels.items()})
        return out

    def shuffle(self, n, first, count, indices=None):
        out = np.zeros(count, dtype=np.uint32)

        def run():
            self.native.check(self.L.bls381_shuffle(n, SEED, ROUNDS, first, count,
                                                    None if indices is None else p(indices), p(out)))
        return run, out


def host_lib():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_shuffle_list.argtypes = [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.hc_shuffle_list.restype = ctypes.c_int
    return lib


def host_base(lib, n, first, count, table, reps=3):
    out = np.zeros(count, dtype=np.uint32)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert lib.hc_shuffle_list(n, SEED, ROUNDS, first, count, table, 16, p(out)) == 0
        times.append((time.perf_counter() - t0) * 1e3)
    return spread(times), out


# (n, count) pairs run through both paths: the rule's own boundary count = ceil(n / 256) at
# n = 2^20, then a small window and the boundary window of longer lists, where the table's
# rounds * ceil(n / 256) hashes grow and the direct path's rounds hashes in sequence do not
BOUNDARY_SHAPES = [(1 << 20, 4096), (1 << 20, 64), (1 << 22, 64), (1 << 22, 1 << 14), (1 << 24, 64), (1 << 24, 1 << 16),
                   (1 << 26, 64), (1 << 26, 1 << 18)]


def boundary_child(args):
    eng = Engine()
    rows = []
    for n, count in BOUNDARY_SHAPES:
        run, out = eng.shuffle(n, n // 2, count)
        res = eng.timed(run, args.reps)
        res.update({"n": n, "count": count, "digest": hashlib.sha256(out.tobytes()).hexdigest()})
        rows.append(res)
    print("BOUNDARY " + json.dumps({"path": os.environ.get("BLS381_SHUFFLE_PATH", "0"), "shapes": rows}), flush=True)


def boundary(args):
    runs = []
    for path in ("1", "2", "1", "2"):
        env = dict(os.environ, BLS381_SHUFFLE_PATH=path)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--boundary-child", "--reps", str(args.reps)],
                           env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise RuntimeError("boundary child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
        runs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("BOUNDARY ")][-1][9:]))
    for k in range(len(BOUNDARY_SHAPES)):
        assert len({r["shapes"][k]["digest"] for r in runs}) == 1, "the two paths disagree"
    kernel = lambda row: sum(v["median"] for name, v in row.items() if name.endswith("_ms") and name != "call_ms")
    summary = [{"n": n, "count": count,
                "direct_kernel_ms": [kernel(r["shapes"][k]) for r in runs if r["path"] == "1"],
                "table_kernel_ms": [kernel(r["shapes"][k]) for r in runs if r["path"] == "2"]}
               for k, (n, count) in enumerate(BOUNDARY_SHAPES)]
    for row in summary:
        print("boundary", json.dumps(row), flush=True)
    return {"first": "n / 2", "summary": summary, "runs": runs,
            "note": "path 1 = direct (shuffle_pivots + shuffle_direct), 2 = table (shuffle_pivots + shuffle_table + "
                    "shuffle_walk); two alternating child processes per path, kernel-time sums of the medians"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shuffle_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--boundary-child", action="store_true")
    ap.add_argument("--one", type=int, metavar="LOG2N", help="only two full-list shuffles of n = 2^LOG2N: the workload "
                    "of a profiler run (counter passes, kernel trace)")
    args = ap.parse_args()
    if args.boundary_child:
        return boundary_child(args)
    if args.one:
        run, out = Engine().shuffle(1 << args.one, 0, 1 << args.one)
        run()
        run()
        print("shuffled", 1 << args.one, hashlib.sha256(out.tobytes()).hexdigest())
        return None
    result = {"rounds": ROUNDS, "epoch_yardstick_ms": EPOCH_MS, "timing": "kernel: HIP events per launch; call: host clock "
              "around the synchronising host-pointer entry point (copies included)", "full": [], "host_16_threads": []}
    result["boundary"] = boundary(args)          # children first: this process has not opened the GPU yet
    eng = Engine()
    lib = None if args.skip_host else host_lib()
    for lg in (18, 20, 22):
        n = 1 << lg
        run, out = eng.shuffle(n, 0, n)
        row = {"n": n}
        row.update(eng.timed(run, args.reps))
        assert np.array_equal(np.sort(out), np.arange(n, dtype=np.uint32))
        row["digest"] = hashlib.sha256(out.tobytes()).hexdigest()
        result["full"].append(row)
        print("full", json.dumps(row), flush=True)
        if lib is not None:
            t, ref = host_base(lib, n, 0, n, 1)
            assert np.array_equal(ref, out), "GPU and host lists differ"
            hrow = {"n": n, "form": "table", "ms": t}
            if lg == 18:
                hrow["direct_form_ms"] = host_base(lib, n, 0, n, 0, reps=1)[0]
            result["host_16_threads"].append(hrow)
            print("host", json.dumps(hrow), flush=True)
    # the epoch shape
    rng = np.random.default_rng(0xB15_0400)
    nc, cs = 1024, 128
    n = nc * cs
    active = rng.permutation(1 << 18)[:n].astype(np.uint32)
    run, shuffled = eng.shuffle(n, 0, n, active)
    epoch = {"committees": nc, "committee_size": cs, "shuffle": eng.timed(run, args.reps)}
    coff = np.arange(0, n, cs, dtype=np.uint32)
    clen = np.full(nc, cs, dtype=np.uint32)
    boff = np.arange(0, (nc + 1) * (cs // 8), cs // 8, dtype=np.uint32)
    agg = rng.integers(0, 256, nc * cs // 8, dtype=np.uint8)
    cust = agg & rng.integers(0, 256, nc * cs // 8, dtype=np.uint8) & rng.integers(0, 256, nc * cs // 8, dtype=np.uint8)
    gko, ok, entries = np.zeros(2 * nc + 1, dtype=np.uint32), np.zeros(nc, dtype=np.uint8), np.zeros(n, dtype=np.uint32)

    def run_att():
        eng.native.check(eng.L.bls381_attesting_entries(nc, p(coff), p(clen), p(boff), p(agg), p(cust), p(shuffled), n,
                                                        p(gko), p(ok), p(entries), n))
    epoch["attesting_entries"] = eng.timed(run_att, args.reps)
    assert ok.all() and gko[-1] == int(np.unpackbits(agg | cust).sum())
    c0 = shuffled[:cs]
    bits0 = np.unpackbits(agg[:cs // 8], bitorder="little").astype(bool) & ~np.unpackbits(cust[:cs // 8], bitorder="little").astype(bool)
    assert entries[:gko[1]].tolist() == sorted(c0[bits0].tolist())
    k = lambda d, name: d.get(name + "_ms", {"median": 0.0})["median"]
    kernel_ms = sum(k(epoch["shuffle"], name) for name in KERNELS) + k(epoch["attesting_entries"], "attesting_entries")
    epoch["kernel_ms_total"] = kernel_ms
    epoch["share_of_epoch_verify"] = kernel_ms / EPOCH_MS
    result["epoch"] = epoch
    print("epoch", json.dumps(epoch), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
