#!/usr/bin/env python3
"""Times the epoch context on the GPU: active indices, their root, the proposers.

Kernel times are the library's own HIP events on the launch stream (bls381_profile_enable, one
pair per launch, read per kernel name), medians of --reps runs of the device entry points over
torch buffers, so no upload is in them.  At n = 2^18, 2^20 and 2^22 validators, two in three
active:

  active    the three launches of bls381_active_indices_device with the balance sum, over plain
            arrays (stride 8, 8-byte loads) and over serialized Validator records (stride 121,
            byte-wise loads)
  root      bls381_active_index_root_device over the active list: the chunk kernel and the Merkle
            passes
  proposers 64 slots over 128-member committees of the shuffled active list, mixed balances

The comparison bases are numpy (flatnonzero and a masked sum) and the same header's host build
(libbls381_hostcheck.so hc_active_indices) on 16 threads.  There is no GPU fallback: without a
device the tool fails.

    python tools/epoch_bench.py [--out profiles/epoch_bench.json] [--reps 10] [--skip-host]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-specs_amd"))

import numpy as np  # noqa: E402

SEED = hashlib.sha256(b"epoch_bench").digest()
EPOCH_MS = 7.6          # the grouped-registry verify of 1,024 attestations (README.md), the yardstick
EPOCH = 1000
MAX_EB = 32 * 10 ** 9
FAR = 2 ** 64 - 1
RECORD, OFF_ACT, OFF_EXIT, OFF_BAL = 121, 88, 96, 113
KERNELS = ("active_count", "active_scan", "active_scatter", "index_chunks", "merkle_reduce", "merkle_finish", "proposers")


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


class Engine:
    def __init__(self):
        import torch            # before the engine: one HIP runtime for both
        from bls381_amd import _native
        _native.init(0)
        self.torch, self.native, self.L = torch, _native, _native.lib()
        self.device = torch.device("cuda:0")
        self.L.bls381_profile_enable(1)

    def up(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8)).to(self.device)

    def empty(self, nbytes):
        return self.torch.zeros(max(int(nbytes), 1), dtype=self.torch.uint8, device=self.device)

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def read(self):
        return {k: (v["count"], v["total_ms"]) for k, v in self.native.profile_read().items()}

    def timed(self, fn, reps, warmup=2):
        """fn() `reps` times after `warmup`: per-kernel times (ms per call, a name's launches summed)
        and the host clock around the queued call and a synchronise."""
        for _ in range(warmup):
            fn()
        self.torch.cuda.synchronize()
        calls, kernels = [], {}
        for _ in range(reps):
            before = self.read()
            t0 = time.perf_counter()
            fn()
            self.torch.cuda.synchronize()
            calls.append((time.perf_counter() - t0) * 1e3)
            after = self.read()
            for k in KERNELS:
                if k in after and after[k][0] > before.get(k, (0, 0.0))[0]:
                    kernels.setdefault(k, []).append(after[k][1] - before.get(k, (0, 0.0))[1])
        out = {"call_ms": spread(calls)}
        out.update({k + "_ms": spread(v) for k, v in kernels.items()})
        out["kernel_ms_total"] = sum(statistics.median(v) for v in kernels.values())
        return out


def host_lib():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_active_indices.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hc_active_indices.restype = ctypes.c_int
    return lib


def clock(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return spread(times)


def validators(n, rng):
    act = rng.choice(np.array([0, 10, EPOCH, EPOCH + 1, FAR], dtype=np.uint64), n, p=[0.5, 0.2, 0.1, 0.1, 0.1])
    ext = rng.choice(np.array([FAR, EPOCH, EPOCH + 7], dtype=np.uint64), n, p=[0.8, 0.1, 0.1])
    bal = rng.integers(0, 33, n).astype(np.uint64) * np.uint64(10 ** 9)
    return act, ext, bal


def records(act, ext, bal, rng):
    n = len(act)
    rec = rng.integers(0, 256, (n, RECORD), dtype=np.uint8)
    for off, field in ((OFF_ACT, act), (OFF_EXIT, ext), (OFF_BAL, bal)):
        rec[:, off:off + 8] = field.astype("<u8").view(np.uint8).reshape(n, 8)
    return np.concatenate([rec.reshape(-1), np.zeros(8, dtype=np.uint8)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epoch_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    eng = Engine()
    L = eng.L
    lib = None if args.skip_host else host_lib()
    result = {"epoch_yardstick_ms": EPOCH_MS, "timing": "kernel: HIP events per launch, summed per kernel name and call; "
              "call: host clock around the queued device entry point and a synchronise (no copies)", "sizes": []}
    rng = np.random.default_rng(0xE90C)
    for lg in (18, 20, 22):
        n = 1 << lg
        act, ext, bal = validators(n, rng)
        want = np.flatnonzero((act <= np.uint64(EPOCH)) & (np.uint64(EPOCH) < ext)).astype(np.uint32)
        total = int(bal[want].sum(dtype=np.uint64))
        row = {"n": n, "active": int(len(want))}
        d_idx, d_ct = eng.empty(4 * n), eng.empty(16)
        ws = eng.empty(L.bls381_active_indices_workspace_size(n))
        d_act, d_ext, d_bal = eng.up(act), eng.up(ext), eng.up(bal)
        d_rec = eng.up(records(act, ext, bal, rng))
        forms = {"stride_8": (d_act.data_ptr(), d_ext.data_ptr(), 8, d_bal.data_ptr()),
                 "stride_121": (d_rec.data_ptr() + OFF_ACT, d_rec.data_ptr() + OFF_EXIT, RECORD, d_rec.data_ptr() + OFF_BAL)}
        for name, (pa, pe, stride, pb) in forms.items():
            def run():
                eng.native.check(L.bls381_active_indices_device(n, pa, pe, stride, EPOCH, pb, stride, d_idx.data_ptr(),
                                                                d_ct.data_ptr(), ws.data_ptr(), eng.stream()))
            row["active_" + name] = eng.timed(run, args.reps)
            ct = np.frombuffer(d_ct.cpu().numpy().tobytes(), dtype=np.uint64)
            got = np.frombuffer(d_idx.cpu().numpy().tobytes(), dtype=np.uint32)[:int(ct[0])]
            assert np.array_equal(got, want) and int(ct[1]) == total, name
        count = len(want)
        d_root = eng.empty(32)
        rws = eng.empty(L.bls381_active_index_root_workspace_size(count))

        def run_root():
            eng.native.check(L.bls381_active_index_root_device(count, d_idx.data_ptr(), d_root.data_ptr(), rws.data_ptr(),
                                                               eng.stream()))
        row["root"] = eng.timed(run_root, args.reps)
        row["root"]["root"] = d_root.cpu().numpy().tobytes().hex()
        # 64 proposers over 128-member committees of a shuffled active list
        shuffled = rng.permutation(want)[:64 * 128].astype(np.uint32)
        d_sh, d_prop = eng.up(shuffled), eng.empty(4 * 64)
        coff, clen = np.arange(0, 64 * 128, 128, dtype=np.uint32), np.full(64, 128, dtype=np.uint32)
        pws = eng.empty(L.bls381_proposer_indices_workspace_size(64))

        def run_prop():
            eng.native.check(L.bls381_proposer_indices_device(64, p(coff), p(clen), d_sh.data_ptr(), len(shuffled),
                                                              d_bal.data_ptr(), 8, n, SEED, EPOCH, MAX_EB, d_prop.data_ptr(),
                                                              pws.data_ptr(), eng.stream()))
        row["proposers"] = eng.timed(run_prop, args.reps)
        kernel_ms = row["active_stride_8"]["kernel_ms_total"] + row["root"]["kernel_ms_total"] + row["proposers"]["kernel_ms_total"]
        row["kernel_ms_total_stride_8"] = kernel_ms
        row["share_of_epoch_verify"] = kernel_ms / EPOCH_MS
        row["stride_121_over_stride_8"] = row["active_stride_121"]["kernel_ms_total"] / row["active_stride_8"]["kernel_ms_total"]
        row["numpy_ms"] = clock(lambda: (np.flatnonzero((act <= np.uint64(EPOCH)) & (np.uint64(EPOCH) < ext)),
                                         bal[(act <= np.uint64(EPOCH)) & (np.uint64(EPOCH) < ext)].sum(dtype=np.uint64)))
        if lib is not None:
            out, res = np.zeros(n, dtype=np.uint32), np.zeros(2, dtype=np.uint64)
            row["host_16_threads_ms"] = clock(lambda: lib.hc_active_indices(n, p(act), p(ext), 8, EPOCH, p(bal), 8, 16,
                                                                           p(out), p(res)))
            assert np.array_equal(out[:int(res[0])], want) and int(res[1]) == total
        result["sizes"].append(row)
        print("size", json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
