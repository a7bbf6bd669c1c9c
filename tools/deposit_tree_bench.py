#!/usr/bin/env python3
"""Times the deposit tree kept on the device on the GPU, device forms, beside
what a caller without it must do for the same answers: rebuild the tree over all k leaves.

  append          bls381_deposit_tree_append_device of 16 and of 4,096 leaves at counts 2^16 and
                  2^20 (a fresh tree filled to the count before every repetition, untimed)
  roots           bls381_deposit_tree_roots_device for 1 and for 1,024 counts, count 2^20
  proofs          bls381_deposit_tree_proofs_device, 16 indices at k = 2^20
  deposits        bls381_deposit_tree_deposits_device, 16 records at k = 2^20
  rebuild_root    bls381_merkle_root_device over all 2^20 leaves: one root (per count asked)
  rebuild_proofs  bls381_merkle_proofs_device over all 2^20 leaves for the same 16 indices
  rebuild_deposits  bls381_deposits_build_device over all 2^20 DepositData (it makes every record)

Kernel times are the library's own HIP events on the launch stream (bls381_profile_enable, one
pair per launch, summed per call); call times are a host clock around queueing the device form on
torch's current stream and synchronising it (inputs and outputs stay on the device).  Medians of
--reps.  The tree's answers are compared with the rebuilds' bytes before anything is written.
There is no GPU fallback: without a device the tool fails.  Run it under a time limit.

    python tools/deposit_tree_bench.py [--out profiles/deposit_tree_bench.json] [--reps 10]
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

DEPTH = 32
CAPACITY = 1 << 21
KERNELS = ("deptree_append", "deptree_roots", "deptree_chain", "deptree_gather", "ssz_root", "deposit_data_copy",
           "merkle_reduce", "merkle_finish", "merkle_proofs")


class Engine:
    def __init__(self):
        import torch          # first: the engine then shares torch's HIP runtime
        from bls381_amd import _native
        _native.init(0)
        self.torch, self.native, self.L = torch, _native, _native.lib()
        self.dev = torch.device("cuda:0")

    def read(self):
        return {k: (v["count"], v["total_ms"]) for k, v in self.native.profile_read().items()}

    def up(self, data: bytes):
        return self.torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.dev)

    def empty(self, nbytes):
        return self.torch.zeros(max(int(nbytes), 1), dtype=self.torch.uint8, device=self.dev)

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def sync(self):
        self.torch.cuda.current_stream().synchronize()

    def timed(self, fn, reps, setup=None, warmup=2):
        """fn(state) queues one device call, setup() (untimed, synchronised) makes its state;
        returns (call us, {kernel: us per call}, launches per call)."""
        def one(profile):
            state = setup() if setup else None
            self.sync()
            self.L.bls381_profile_enable(1 if profile else 0)
            before = self.read() if profile else None
            t0 = time.perf_counter()
            fn(state)
            self.sync()
            dt = (time.perf_counter() - t0) * 1e6
            return dt, before, (self.read() if profile else None)
        for _ in range(warmup):
            one(False)
        calls = [one(False)[0] for _ in range(reps)]           # call times without the event pairs
        kernels, launches = {k: [] for k in KERNELS}, 0
        for _ in range(reps):
            _, before, after = one(True)
            launches = 0
            for k in KERNELS:
                c0, t0k = before.get(k, (0, 0.0))
                c1, t1k = after.get(k, (0, 0.0))
                if c1 > c0:
                    kernels[k].append((t1k - t0k) * 1e3)
                    launches += c1 - c0
        self.L.bls381_profile_enable(0)
        return statistics.median(calls), {k: statistics.median(v) for k, v in kernels.items() if v}, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deposit_tree_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    eng = Engine()
    L, check = eng.L, eng.native.check
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = []

    def row(name, shape, fn, setup=None):
        call, kernels, launches = eng.timed(fn, args.reps, setup)
        rows.append({"name": name, "shape": shape, "kernel_us": round(sum(kernels.values()), 2),
                     "call_us": round(call, 2), "launches": launches,
                     "kernels_us": {k: round(v, 2) for k, v in kernels.items()}})
        print(json.dumps(rows[-1]), flush=True)

    n_all = 1 << 20
    rng = np.random.default_rng(0xB15_0600)
    data = rng.integers(0, 256, 184 * n_all, dtype=np.uint8).tobytes()
    d_data = eng.up(data)
    del data
    # the leaves of the whole run: hash_tree_root of the data, by a tree of its own
    d_leaves = eng.empty(32 * (n_all + 4096))
    ws_ssz = eng.empty(L.bls381_ssz_root_workspace_size())
    from bls381_amd import ssz
    prog = ssz.compile_root(ssz.DepositData)
    check(L.bls381_ssz_root_batch_device(n_all, p(d_data), 184, 184, prog.ctypes.data_as(ctypes.c_void_p), len(prog),
                                         p(d_leaves), p(ws_ssz), eng.stream()))
    eng.sync()
    extra = ctypes.c_void_p(d_leaves.data_ptr() + 32 * 1000)      # the leaves an append adds: any 32-byte values

    trees = []

    def fresh(count):
        def setup():
            while trees:
                L.bls381_deposit_tree_destroy(trees.pop())
            h = ctypes.c_void_p()
            check(L.bls381_deposit_tree_create(CAPACITY, DEPTH, ctypes.byref(h)))
            trees.append(h)
            check(L.bls381_deposit_tree_append_device(h, count, p(d_leaves), eng.stream()))
            return h
        return setup

    # ---- appends
    for count, label in ((1 << 16, "2^16"), (1 << 20, "2^20")):
        for n in (16, 4096):
            row("append", "%d leaves at count %s" % (n, label),
                lambda h, n=n: check(L.bls381_deposit_tree_append_device(h, n, extra, eng.stream())), fresh(count))

    # ---- queries on a tree of 2^20 leaves, and the rebuilds beside them
    tree = fresh(n_all)()
    eng.sync()
    k = n_all
    d_roots = eng.empty(32 * 1024)
    one = np.array([k], dtype=np.uint64)
    many = rng.integers(0, k + 1, 1024, dtype=np.uint64)
    for ks, label in ((one, "1 count (2^20)"), (many, "1,024 counts up to 2^20")):
        row("roots", label, lambda _, ks=ks: check(L.bls381_deposit_tree_roots_device(
            tree, len(ks), ks.ctypes.data_as(ctypes.c_void_p), p(d_roots), eng.stream())))
    check(L.bls381_deposit_tree_roots_device(tree, 1, one.ctypes.data_as(ctypes.c_void_p), p(d_roots), eng.stream()))
    eng.sync()
    root_tree = d_roots.cpu().numpy().tobytes()[:32]

    idx = np.array([0, 1, 255, 256, 65535, 65536, k // 2, k - 1] + [int(x) for x in rng.integers(0, k, 8)],
                   dtype=np.uint64)
    d_idx, d_proofs, d_root = eng.up(idx.tobytes()), eng.empty(1024 * 16), eng.empty(32)
    ws = eng.empty(L.bls381_deposit_tree_proofs_workspace_size(DEPTH))
    row("proofs", "16 indices at k = 2^20", lambda _: check(L.bls381_deposit_tree_proofs_device(
        tree, k, 16, p(d_idx), p(d_proofs), 1024, p(d_root), p(ws), eng.stream())))
    proofs_tree = d_proofs.cpu().numpy().tobytes()
    assert d_root.cpu().numpy().tobytes() == root_tree

    first = k - 16
    d_dep = eng.empty(1208 * 16)
    ws_dep = eng.empty(L.bls381_deposit_tree_deposits_workspace_size(16))
    d_tail = ctypes.c_void_p(d_data.data_ptr() + 184 * first)
    row("deposits", "16 records at k = 2^20", lambda _: check(L.bls381_deposit_tree_deposits_device(
        tree, k, first, 16, d_tail, p(d_dep), p(ws_dep), eng.stream())))
    dep_tree = d_dep.cpu().numpy().tobytes()

    ws = eng.empty(L.bls381_merkle_root_workspace_size(k, 0, DEPTH))
    row("rebuild_root", "2^20 leaves, one root", lambda _: check(L.bls381_merkle_root_device(
        k, p(d_leaves), 0, DEPTH, 0, 0, p(d_root), p(ws), eng.stream())))
    assert d_root.cpu().numpy().tobytes() == root_tree, "the tree's root and the rebuild's differ"

    ws = eng.empty(L.bls381_merkle_proofs_workspace_size(k, 0, DEPTH))
    d_proofs2 = eng.empty(1024 * 16)
    row("rebuild_proofs", "2^20 leaves, 16 indices", lambda _: check(L.bls381_merkle_proofs_device(
        k, p(d_leaves), 0, DEPTH, 16, p(d_idx), p(d_proofs2), 1024, p(d_root), p(ws), eng.stream())))
    assert d_proofs2.cpu().numpy().tobytes() == proofs_tree, "the tree's proofs and the rebuild's differ"
    del ws, d_proofs2

    ws = eng.empty(L.bls381_deposits_build_workspace_size(k))
    d_all = eng.empty(1208 * k)
    row("rebuild_deposits", "2^20 DepositData, every record", lambda _: check(L.bls381_deposits_build_device(
        k, p(d_data), 0, p(d_all), p(d_root), p(ws), eng.stream())))
    assert d_all[1208 * first:].cpu().numpy().tobytes() == dep_tree, "the tree's deposits and the rebuild's differ"
    assert d_root.cpu().numpy().tobytes() == root_tree

    eng.sync()
    while trees:
        L.bls381_deposit_tree_destroy(trees.pop())
    arch = eng.torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    out = {"tool": "tools/deposit_tree_bench.py", "box": "%s (%s)" % (eng.torch.cuda.get_device_name(0), arch),
           "reps": args.reps, "capacity": CAPACITY, "depth": DEPTH,
           "units": "microseconds; kernel_us: the library's HIP events summed per call; call_us: host clock, "
                    "queue + synchronise; medians",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
