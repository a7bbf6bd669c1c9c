#!/usr/bin/env python3
"""Times the Merkle tree stages on the GPU: three device forms.

  root      bls381_merkle_root_device over 2^20 leaves, depth 32
  proofs    bls381_merkle_proofs_device: the root and all 2^16 proofs over 2^16 leaves, depth 32
  deposits  bls381_deposits_build_device of 2^16 DepositData

Kernel times are the library's own HIP events on the launch stream (bls381_profile_enable, one
pair per launch, summed per call); call times are a host clock around queueing the device form on
torch's current stream and synchronising it (no copies: inputs and outputs stay on the device).
Each figure stands beside the same call's host build (libbls381_hostcheck.so, the same headers
with the tile loop as plain loops) on 16 threads, and beside the bytes the call must move -- 32
bytes per node read and per node written, the deposits' data and records too -- at the HBM rate
below.  There is no GPU fallback: without a device the tool fails.

    python tools/merkle_bench.py [--out profiles/merkle_tree.txt] [--reps 10] [--skip-host]
"""
import argparse
import ctypes
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-specs_amd"))

import numpy as np  # noqa: E402

HBM_BYTES_PER_S = 6.3e12      # a streaming copy on the MI355X (8.0e12 is the data sheet's peak)
DEPTH = 32
KERNELS = ("merkle_reduce", "merkle_finish", "merkle_proofs", "ssz_root", "deposit_data_copy")
U64 = ctypes.c_uint64


def med(xs):
    return statistics.median(xs)


class Engine:
    def __init__(self):
        import torch          # first: the engine then shares torch's HIP runtime
        from bls381_amd import _native
        _native.init(0)
        self.torch, self.native, self.L = torch, _native, _native.lib()
        self.dev = torch.device("cuda:0")
        self.L.bls381_profile_enable(1)

    def read(self):
        return {k: (v["count"], v["total_ms"]) for k, v in self.native.profile_read().items()}

    def up(self, data: bytes):
        return self.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.dev)

    def empty(self, nbytes):
        return self.torch.zeros(max(int(nbytes), 1), dtype=self.torch.uint8, device=self.dev)

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def timed(self, fn, reps, warmup=3):
        """fn() queues one device call; returns (call ms, {kernel: ms per call}, launches per call)."""
        sync = self.torch.cuda.current_stream().synchronize
        for _ in range(warmup):
            fn()
        sync()
        calls, kernels, launches = [], {k: [] for k in KERNELS}, 0
        self.L.bls381_profile_enable(0)          # call times without the event pairs
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            sync()
            calls.append((time.perf_counter() - t0) * 1e3)
        self.L.bls381_profile_enable(1)
        for _ in range(reps):
            before = self.read()
            fn()
            sync()
            after = self.read()
            launches = 0
            for k in KERNELS:
                c0, t0k = before.get(k, (0, 0.0))
                c1, t1k = after.get(k, (0, 0.0))
                if c1 > c0:
                    kernels[k].append(t1k - t0k)
                    launches += c1 - c0
        return med(calls), {k: med(v) for k, v in kernels.items() if v}, launches


def host_lib():
    import build_native
    lib = ctypes.CDLL(os.environ.get("BLS381_HOSTCHECK_LIB") or build_native.build_hostcheck())
    lib.hc_merkle_root.argtypes = [ctypes.c_size_t, ctypes.c_char_p, U64, ctypes.c_uint32, ctypes.c_int, U64,
                                   ctypes.c_int, ctypes.c_char_p]
    lib.hc_merkle_proofs.argtypes = [ctypes.c_size_t, ctypes.c_char_p, U64, ctypes.c_uint32, ctypes.c_size_t,
                                     ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p]
    lib.hc_deposits_build.argtypes = [ctypes.c_size_t, ctypes.c_char_p, U64, ctypes.c_int, ctypes.c_char_p,
                                      ctypes.c_char_p]
    return lib


def host_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert fn() == 0
        times.append((time.perf_counter() - t0) * 1e3)
    return med(times)


def leaves_blob(n):
    return b"".join(hashlib.sha256(b"leaf" + (7).to_bytes(4, "little") + i.to_bytes(8, "little")).digest()
                    for i in range(n))


def commit_id():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_tree.txt"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--commit", default=None, help="the commit the tree stands on, where git cannot be asked")
    args = ap.parse_args()
    eng = Engine()
    L, p = eng.L, lambda t: ctypes.c_void_p(t.data_ptr())
    lib = None if args.skip_host else host_lib()
    rows = []

    def row(name, shape, fn, moved, host_fn, check):
        call, kernels, launches = eng.timed(fn, args.reps)
        host = host_ms(host_fn) if lib is not None else None
        check()                                   # the two builds wrote the same bytes
        kernel = sum(kernels.values())
        rows.append({"name": name, "shape": shape, "kernel_ms": kernel, "call_ms": call, "launches": launches,
                     "kernels": kernels, "host16_ms": host,
                     "moved_bytes": moved, "hbm_ms": moved / HBM_BYTES_PER_S * 1e3})
        print(name, rows[-1], flush=True)

    # ---- the root of 2^20 leaves
    n = 1 << 20
    blob = leaves_blob(n)
    d_leaves, d_root = eng.up(blob), eng.empty(32)
    ws = eng.empty(L.bls381_merkle_root_workspace_size(n, 0, DEPTH))
    h_root = ctypes.create_string_buffer(32)

    def check_root():
        assert lib is None or d_root.cpu().numpy().tobytes() == h_root.raw, "GPU and host roots differ"
    row("root", "2^20 leaves, depth 32",
        lambda: eng.native.check(L.bls381_merkle_root_device(n, p(d_leaves), 0, DEPTH, 0, 0, p(d_root), p(ws),
                                                             eng.stream())),
        32 * (n + n // 256 * 2 + 1),       # the leaves once, the pass levels written and read, the root
        lambda: lib.hc_merkle_root(n, blob, 0, DEPTH, 0, 0, 16, h_root), check_root)

    # ---- root and every proof over 2^16 leaves
    n = 1 << 16
    blob = blob[:32 * n]
    d_leaves = eng.up(blob)
    idx = np.arange(n, dtype=np.uint64)
    d_idx, d_proofs = eng.up(idx.tobytes()), eng.empty(32 * DEPTH * n)
    ws = eng.empty(L.bls381_merkle_proofs_workspace_size(n, 0, DEPTH))
    h_proofs = ctypes.create_string_buffer(32 * DEPTH * n)

    def check_proofs():
        if lib is not None:
            assert d_root.cpu().numpy().tobytes() == h_root.raw and d_proofs.cpu().numpy().tobytes() == h_proofs.raw, \
                "GPU and host proofs differ"
    row("proofs", "2^16 leaves, 2^16 proofs, depth 32",
        lambda: eng.native.check(L.bls381_merkle_proofs_device(n, p(d_leaves), 0, DEPTH, n, p(d_idx), p(d_proofs),
                                                               32 * DEPTH, p(d_root), p(ws), eng.stream())),
        32 * (n + n) + 2 * 32 * DEPTH * n + 8 * n,   # leaves read, kept levels written, siblings read and written
        lambda: lib.hc_merkle_proofs(n, blob, 0, DEPTH, n, idx.ctypes.data_as(ctypes.c_void_p), h_proofs, 32 * DEPTH,
                                     16, h_root), check_proofs)

    # ---- deposits_build of 2^16
    rng = np.random.default_rng(0xB15_0500)
    data = rng.integers(0, 256, 184 * n, dtype=np.uint8).tobytes()
    d_data, d_dep = eng.up(data), eng.empty(1208 * n)
    ws = eng.empty(L.bls381_deposits_build_workspace_size(n))
    h_dep = ctypes.create_string_buffer(1208 * n)
    first = (1 << 31) + 7

    def check_deposits():
        if lib is not None:
            assert d_root.cpu().numpy().tobytes() == h_root.raw and d_dep.cpu().numpy().tobytes() == h_dep.raw, \
                "GPU and host deposits differ"
    row("deposits_build", "2^16 DepositData at index 2^31 + 7",
        lambda: eng.native.check(L.bls381_deposits_build_device(n, p(d_data), first, p(d_dep), p(d_root), p(ws),
                                                                eng.stream())),
        # the data read twice, the leaves written and read, the kept levels, the siblings read, the records written
        2 * 184 * n + 32 * (2 * n + n) + 32 * DEPTH * n + 1208 * n,
        lambda: lib.hc_deposits_build(n, data, first, 16, h_dep, h_root), check_deposits)

    arch = eng.torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    name = "%s (%s)" % (eng.torch.cuda.get_device_name(0), arch)
    lines = ["Merkle tree stages, device forms (tools/merkle_bench.py, %d reps, medians)" % args.reps,
             "box: %s; commit: %s (the working tree's parent)" % (name, args.commit or commit_id()),
             "kernel ms: the library's HIP events summed per call; call ms: host clock, queue + synchronise;",
             "host ms: the same headers' host build on 16 threads; HBM ms: the bytes the call must move at %.1f TB/s"
             % (HBM_BYTES_PER_S / 1e12), "",
             "%-15s %-38s %9s %9s %8s %10s %10s %9s" % ("form", "shape", "kernel ms", "call ms", "launches",
                                                       "host16 ms", "moved MB", "HBM ms")]
    for r in rows:
        lines.append("%-15s %-38s %9.3f %9.3f %8d %10s %10.1f %9.4f" % (
            r["name"], r["shape"], r["kernel_ms"], r["call_ms"], r["launches"],
            "-" if r["host16_ms"] is None else "%.1f" % r["host16_ms"], r["moved_bytes"] / 1e6, r["hbm_ms"]))
    lines.append("")
    for r in rows:
        per_kernel = ", ".join("%s %.3f" % kv for kv in r["kernels"].items())
        lines.append("%-15s per kernel, ms per call: %s" % (r["name"], per_kernel))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
