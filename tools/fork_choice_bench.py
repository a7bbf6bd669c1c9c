#!/usr/bin/env python3
"""Times bls381_fork_choice_head_device at 2^20 and 2^22 validators whose 121-byte
records are resident, over a tree of 8,192 blocks, in two vote scenarios:

  tip      every validator's latest message names the tip (one bin: the contended extreme)
  spread   the messages are spread over the last 64 blocks, neighbouring validators on different ones

and bls381_fork_choice_on_attestations_device for 128 attestations of 1,024 members each.

Call times are device events on the launch stream around BATCH back-to-back calls of the _device
form after a warm-up, so they are warm figures: the same records are read again and again and, at
2^20 validators (127 MB), fit the last-level cache.  Kernel times are the library's own HIP events
(bls381_profile_enable, one pair per launch, summed per kernel name over a call: the rounds of
fc_jump are one figure, the two steps of fc_best another) in a pass of their own.  Beside each call
time: the bytes the call must read and write, counted from the shapes (`needed_bytes`), divided by
the time.  Comparison bases, both on the host over plain arrays and both including no copy: the
model's algorithm in numpy (`numpy_restatement`) and the g++ build of the shared header
(hc_fork_choice_head of lib/libbls381_hostcheck.so on one thread, the best of three calls).  Every
run's head and vote counts must equal the numpy restatement's.  There is no GPU fallback: without
a device the tool fails.

    python tools/fork_choice_bench.py [--out profiles/fork_choice_bench.json] [--reps 10]
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

SIZES = (1 << 20, 1 << 22)
BLOCKS = 8192
LAST = 64
BATCH = 20
ATTESTATIONS, MEMBERS = 128, 1024
ETH = 10 ** 9
FAR = 2 ** 64 - 1
EPOCH = 1000
NODE_BINS = 2048   # FC_BINS
KERNELS = ("fc_direct", "fc_scan", "fc_count", "fc_best", "fc_jump")
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E peak, the denominator of the shares below


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def tree(rng):
    """A chain whose last LAST blocks fork: (roots, parents as indices, slots)."""
    roots = [hashlib.sha256(b"bench block %d" % i).digest() for i in range(BLOCKS)]
    parent = np.arange(-1, BLOCKS - 1, dtype=np.int64)
    for i in range(BLOCKS - LAST + 1, BLOCKS):
        parent[i] = rng.integers(max(BLOCKS - LAST, i - 8), i)
    slots = np.zeros(BLOCKS, np.uint64)
    for i in range(1, BLOCKS):
        slots[i] = slots[parent[i]] + 1
    return roots, parent, slots


def registry(n, rng):
    act, ext = np.zeros(n, np.uint64), np.full(n, FAR, np.uint64)
    eff = rng.choice(np.array([32, 32, 32, 31, 24], np.uint64), n) * np.uint64(ETH)
    gone = rng.choice(n, n // 50, replace=False)
    ext[gone[:len(gone) // 2]] = EPOCH - 3
    act[gone[len(gone) // 2:]] = FAR
    return act, ext, eff


def messages(n, scenario, rng):
    """Every validator once, in attestations of MEMBERS members: (att_off, entries, slots, targets)."""
    entries = rng.permutation(n).astype(np.uint32)
    n_att = (n + MEMBERS - 1) // MEMBERS
    off = np.minimum(np.arange(n_att + 1, dtype=np.uint64) * MEMBERS, n).astype(np.uint32)
    targets = np.full(n_att, BLOCKS - 1, np.uint32) if scenario == "tip" else \
        (BLOCKS - LAST + np.arange(n_att) % LAST).astype(np.uint32)
    return off, entries, np.full(n_att, 9000, np.uint64), targets


def numpy_restatement(parent, roots, target, act, ext, eff, start):
    """The model's algorithm in numpy: (head, counts)."""
    B = len(parent)
    votes = (target != 0xFFFFFFFF) & (act <= np.uint64(EPOCH)) & (np.uint64(EPOCH) < ext)
    direct = np.zeros(B, np.uint64)
    np.add.at(direct, target[votes], eff[votes])
    size = np.ones(B, np.int64)
    for i in range(B - 1, 0, -1):
        size[parent[i]] += size[i]
    pre, nxt = np.zeros(B, np.int64), np.ones(B, np.int64)
    for i in range(1, B):
        q = parent[i]
        pre[i] = nxt[q]
        nxt[q] += size[i]
        nxt[i] = pre[i] + 1
    laid = np.zeros(B + 1, np.uint64)
    laid[pre + 1] = direct
    prefix = np.cumsum(laid, dtype=np.uint64)
    counts = prefix[pre + size] - prefix[pre]
    best = {}
    for i in range(1, B):
        q = int(parent[i])
        if q not in best or (int(counts[i]), roots[i]) > (int(counts[best[q]]), roots[best[q]]):
            best[q] = i
    head = start
    while head in best:
        head = best[head]
    return head, counts


def needed_bytes(n, voters):
    """fc_direct: every validator's target once per node tile, and the three fields of a validator
    with a message in the one tile that holds its target; the rest works on the tree: about 100
    bytes a block."""
    tiles = (BLOCKS + NODE_BINS - 1) // NODE_BINS
    return n * 4 * tiles + voters * 24 + BLOCKS * 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fork_choice_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import build_native
    from bls381_amd import _native, fork_choice as FC
    _native.init(0)
    L = _native.lib()
    H = ctypes.CDLL(build_native.build_hostcheck())
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, res, argtypes in (("create", vp, [u64, u64]), ("destroy", None, [vp]),
                                ("add_blocks", ctypes.c_int, [vp, u64, vp, vp, vp, vp]),
                                ("on_attestations", ctypes.c_int, [vp, u64, vp, vp, vp, vp, vp, vp]),
                                ("head", ctypes.c_int, [vp, u32, u64, vp, vp, vp, ctypes.c_size_t, u64, vp, vp, vp, vp])):
        fn = getattr(H, "hc_fork_choice_" + name)
        fn.restype, fn.argtypes = res, argtypes
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    result = {"record_stride": FC.RECORD, "batch": BATCH, "blocks": BLOCKS, "hbm_peak_GBs": HBM_PEAK_GBS, "epoch": EPOCH,
              "timing": "call: device events around %d back-to-back _device calls on resident records (warm); kernel: the "
                        "library's HIP events per launch, summed per kernel name over one call, in a pass of their own; "
                        "numpy: wall time of one call over plain host arrays; host build: the best of three calls, one "
                        "thread" % BATCH, "runs": []}
    rng = np.random.default_rng(7)
    roots, parent, block_slots = tree(rng)
    root_blob = b"".join(roots)
    parent_blob = b"".join(roots[q] if q >= 0 else bytes(32) for q in parent)
    for n in SIZES:
        act, ext, eff = registry(n, rng)
        rec = rng.integers(0, 256, size=(n, FC.RECORD), dtype=np.uint8)
        for off, col in zip((FC.OFF_ACTIVATION, FC.OFF_EXIT, FC.OFF_EFFECTIVE), (act, ext, eff)):
            rec[:, off:off + 8] = col.astype("<u8").view(np.uint8).reshape(n, 8)
        d_rec = torch.from_numpy(rec.reshape(-1)).to("cuda")
        q = d_rec.data_ptr()
        del rec
        for scenario in ("tip", "spread"):
            off, entries, slots, targets = messages(n, scenario, rng)
            target = np.zeros(n, np.uint32)
            target[entries] = np.repeat(targets, np.diff(off))
            t0 = time.perf_counter()
            want_head, want_counts = numpy_restatement(parent, roots, target, act, ext, eff, 0)
            numpy_ms = (time.perf_counter() - t0) * 1e3
            # the host build, one thread
            hs = H.hc_fork_choice_create(n, BLOCKS)
            skipped, h_head, h_status, h_counts = np.zeros(1, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint64), np.zeros(BLOCKS, np.uint64)
            assert H.hc_fork_choice_add_blocks(hs, BLOCKS, root_blob, parent_blob, p(block_slots), None) == 0
            assert H.hc_fork_choice_on_attestations(hs, len(slots), p(off), p(entries), p(slots), p(targets), None, p(skipped)) == 0
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                assert H.hc_fork_choice_head(hs, 0, n, p(act), p(ext), p(eff), 8, EPOCH, p(h_head), None, p(h_counts), p(h_status)) == 0
                times.append((time.perf_counter() - t0) * 1e3)
            H.hc_fork_choice_destroy(hs)
            assert int(h_head[0]) == want_head and np.array_equal(h_counts, want_counts)
            # the engine
            with FC.ForkChoice(n, BLOCKS) as fc:
                fc.add_blocks(roots, [roots[i] if i >= 0 else bytes(32) for i in parent], block_slots)
                assert fc.on_attestations(off, entries, slots, targets) == 0
                out = torch.zeros(2 + BLOCKS, dtype=torch.int64, device="cuda")

                def call():
                    _native.check(L.bls381_fork_choice_head_device(
                        fc._handle(), 0, n, q + FC.OFF_ACTIVATION, q + FC.OFF_EXIT, q + FC.OFF_EFFECTIVE, FC.RECORD, EPOCH,
                        out.data_ptr(), out.data_ptr() + 16, out.data_ptr() + 8, stream()))

                call()
                call()
                torch.cuda.synchronize()
                got = out.cpu().numpy().view(np.uint64)
                assert int(got[0]) == want_head and int(got[1]) == 0 and np.array_equal(got[2:], want_counts), (int(got[0]), want_head)
                times_call = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(BATCH):
                        call()
                    b.record()
                    b.synchronize()
                    times_call.append(a.elapsed_time(b) / BATCH)
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
                # on_attestations_device: 128 attestations of 1,024 members, a higher slot each batch
                a_off = (np.arange(ATTESTATIONS + 1, dtype=np.uint32) * MEMBERS)
                d_entries = torch.from_numpy(rng.integers(0, n, ATTESTATIONS * MEMBERS).astype(np.int64).astype(np.uint32).view(np.int32)).to("cuda")
                a_targets = (BLOCKS - LAST + np.arange(ATTESTATIONS) % LAST).astype(np.uint32)
                d_skipped = torch.zeros(1, dtype=torch.int64, device="cuda")
                ws = torch.empty(max(1, L.bls381_fork_choice_on_attestations_workspace_size(ATTESTATIONS)), dtype=torch.uint8, device="cuda")
                slot = [9001]

                def attest():
                    a_slots = np.full(ATTESTATIONS, slot[0], np.uint64)
                    slot[0] += 1
                    _native.check(L.bls381_fork_choice_on_attestations_device(
                        fc._handle(), ATTESTATIONS, p(a_off), d_entries.data_ptr(), p(a_slots), p(a_targets), None,
                        d_skipped.data_ptr(), ws.data_ptr(), stream()))

                attest()
                attest()
                torch.cuda.synchronize()
                times_att = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(BATCH):
                        attest()
                    b.record()
                    b.synchronize()
                    times_att.append(a.elapsed_time(b) / BATCH)
                assert int(d_skipped.cpu()[0]) == 0
            voters = int(((act <= EPOCH) & (EPOCH < ext)).sum())
            need = needed_bytes(n, n)   # every validator has a message; the fields of all of them are read
            row = {"validators": n, "scenario": scenario, "voting": voters, "head": want_head, "ms": spread(times_call),
                   "needed_bytes": need, "kernels_ms": {name: spread(v) for name, v in per.items()},
                   "on_attestations_ms": spread(times_att), "numpy_ms": numpy_ms, "host_build_one_thread_ms": min(times)}
            row["GBs"] = need / (row["ms"]["median"] * 1e-3) / 1e9
            row["share_of_hbm_peak"] = row["GBs"] / HBM_PEAK_GBS
            result["runs"].append(row)
            print(json.dumps(row), flush=True)
        del d_rec
    by = {(r["validators"], r["scenario"]): r["kernels_ms"]["fc_direct"]["median"] for r in result["runs"]}
    result["direct_tip_over_spread"] = {str(n): by[(n, "tip")] / by[(n, "spread")] for n in SIZES}
    print(json.dumps(result["direct_tip_over_spread"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
