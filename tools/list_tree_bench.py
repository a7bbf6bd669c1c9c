#!/usr/bin/env python3
"""Times the SSZ list trees kept on the device on the GPU, device forms, beside
what a caller without them does for one root after the same change: hash the whole list again.

On a Validator tree (121-byte records) and a uint64 tree at count 2^20, capacity 2^21:
  update          bls381_list_tree_update_device of 1, 16 and 4,096 effective_balance fields
                  (uint64 tree: items) at random indices, and of every item
  append          bls381_list_tree_append_device of 16 items (the count grows by 16 a repetition)
  root            bls381_list_tree_root_device
  proofs          bls381_list_tree_proofs_device, 16 chunk indices
  rebuild         bls381_ssz_list_root_device over the records / bls381_merkle_root_device over
                  the balance chunks, read from the tree's own item store

Kernel times are the library's own HIP events on the launch stream (bls381_profile_enable, one
pair per launch, summed per call); call times are a host clock around queueing the device form on
torch's current stream and synchronising it (inputs and outputs stay on the device).  Medians of
--reps.  The tree's root is compared with the rebuild's bytes before anything is written.
There is no GPU fallback: without a device the tool fails.  Run it under a time limit.

    python tools/list_tree_bench.py [--out profiles/list_tree_bench.json] [--reps 10]
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

CAPACITY = 1 << 21
COUNT = 1 << 20
KERNELS = ("listtree_scatter", "listtree_leaves_idx", "listtree_leaves", "listtree_mark", "listtree_compact",
           "listtree_reduce", "listtree_root", "listtree_proofs", "ssz_root", "merkle_reduce", "merkle_finish")


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

    def timed(self, fn, reps, warmup=2):
        """fn() queues one device call; returns (call us, {kernel: us per call}, launches per call)."""
        def one(profile):
            self.sync()
            self.L.bls381_profile_enable(1 if profile else 0)
            before = self.read() if profile else None
            t0 = time.perf_counter()
            fn()
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_tree_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    eng = Engine()
    L, check = eng.L, eng.native.check
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    from bls381_amd import ssz
    rows = []

    def row(tree, name, shape, fn):
        call, kernels, launches = eng.timed(fn, args.reps)
        rows.append({"tree": tree, "name": name, "shape": shape, "kernel_us": round(sum(kernels.values()), 2),
                     "call_us": round(call, 2), "launches": launches,
                     "kernels_us": {k: round(v, 2) for k, v in kernels.items()}})
        print(json.dumps(rows[-1]), flush=True)

    rng = np.random.default_rng(0xB15_0720)
    prog = np.ascontiguousarray(ssz.compile_root(ssz.Validator), dtype=np.uint32)
    pp = prog.ctypes.data_as(ctypes.c_void_p)
    for label, size, off, length, tprog in (("validator", 121, 113, 8, prog), ("uint64", 8, 0, 8, None)):
        h = ctypes.c_void_p()
        check(L.bls381_list_tree_create(CAPACITY, size, pp if tprog is not None else None,
                                        len(prog) if tprog is not None else 0, ctypes.byref(h)))
        d_items = eng.up(rng.integers(0, 256, size * COUNT, dtype=np.uint8).tobytes())
        ws = eng.empty(L.bls381_list_tree_append_workspace_size(h, COUNT))
        check(L.bls381_list_tree_append_device(h, COUNT, p(d_items), p(ws), eng.stream()))
        eng.sync()
        count = lambda: L.bls381_list_tree_count(h)
        d_vals = eng.up(rng.integers(0, 256, length * COUNT, dtype=np.uint8).tobytes())
        for n_upd in (1, 16, 4096, COUNT):
            idx = (np.arange(COUNT) if n_upd == COUNT else rng.integers(0, COUNT, n_upd)).astype(np.uint32)
            d_idx = eng.up(idx.tobytes())
            ws = eng.empty(L.bls381_list_tree_update_workspace_size(h, n_upd))
            row(label, "update", "every item (2^20)" if n_upd == COUNT else "%d fields at random indices" % n_upd,
                lambda: check(L.bls381_list_tree_update_device(h, n_upd, p(d_idx), off, length, p(d_vals), p(ws), eng.stream())))
        ws = eng.empty(L.bls381_list_tree_append_workspace_size(h, 16))
        row(label, "append", "16 items at count 2^20 + 16 k",
            lambda: check(L.bls381_list_tree_append_device(h, 16, p(d_items), p(ws), eng.stream())))
        d_root = eng.empty(32)
        row(label, "root", "mixed with the count", lambda: check(L.bls381_list_tree_root_device(h, 1, p(d_root), eng.stream())))
        root_tree = d_root.cpu().numpy().tobytes()
        chunks = count() if tprog is not None else (count() * size + 31) // 32
        cidx = np.array([0, 1, 255, 256, 65535, 65536, chunks // 2, chunks - 1] + [int(x) for x in rng.integers(0, chunks, 8)],
                        dtype=np.uint64)
        d_cidx, d_proofs, d_root2 = eng.up(cidx.tobytes()), eng.empty(1024 * 16), eng.empty(32)
        row(label, "proofs", "16 chunk indices", lambda: check(L.bls381_list_tree_proofs_device(
            h, 16, p(d_cidx), p(d_proofs), 1024, p(d_root2), eng.stream())))
        store = ctypes.c_void_p(L.bls381_list_tree_items_device(h))
        n = count()
        if tprog is not None:
            ws = eng.empty(L.bls381_ssz_list_root_workspace_size(n))
            row(label, "rebuild", "bls381_ssz_list_root_device over %d records" % n, lambda: check(L.bls381_ssz_list_root_device(
                n, store, size, size, pp, len(prog), 1, p(d_root), p(ws), eng.stream())))
        else:
            depth = L.bls381_list_tree_depth(h)
            ws = eng.empty(L.bls381_merkle_root_workspace_size(chunks, 0, depth))
            row(label, "rebuild", "bls381_merkle_root_device over %d chunks" % chunks, lambda: check(L.bls381_merkle_root_device(
                chunks, store, 0, depth, 1, n, p(d_root), p(ws), eng.stream())))
        assert d_root.cpu().numpy().tobytes() == root_tree, "the tree's root and the rebuild's differ"
        eng.sync()
        L.bls381_list_tree_destroy(h)
        del d_items, d_vals

    arch = eng.torch.cuda.get_device_properties(0).gcnArchName.split(":")[0]
    out = {"tool": "tools/list_tree_bench.py", "box": "%s (%s)" % (eng.torch.cuda.get_device_name(0), arch),
           "reps": args.reps, "capacity": CAPACITY, "count": COUNT,
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
