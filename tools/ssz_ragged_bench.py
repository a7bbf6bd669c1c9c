#!/usr/bin/env python3
"""Times the roots of variable-size SSZ items on resident serializations:

  pending_8192     List[PendingAttestation] of 8,192 elements, bitfields of 16 to 512 bytes:
                   bls381_ssz_ragged_list_root_device, and the element roots alone
  attestations_128 List[Attestation] of 128 elements, both bitfields of 16 to 512 bytes
  slashing_4x4096  one AttesterSlashing, 4 x 4,096 indices: bls381_ssz_ragged_roots_device, n = 1
  indexed_4096     one IndexedAttestation, 4,096 + 0 indices: the cost of one long field in one lane

Call times are device events on the launch stream around BATCH back-to-back calls of the _device
form after a warm-up, medians over --reps batches, so they are warm figures: the same items are
read again and again and fit the last-level cache.  Bases: the per-element path of
``ssz.hash_tree_root(List(PendingAttestation), values)`` as it was before the one-call path (a
root per field of each element through ``hash_tree_root``, ``merkle_root`` to combine them and again
over the elements: five engine calls per element, each with its own host synchronisation), timed
once at the full 8,192 by wall clock; and the g++ build of the shared header
(hc_ssz_ragged_root of lib/libbls381_hostcheck.so) on one host thread, the best of three passes.
Every root is compared with the host build's.  There is no GPU fallback: without a device the tool fails.

    python tools/ssz_ragged_bench.py [--out profiles/ssz_ragged_bench.json] [--reps 10]
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

BATCH = 20
vp = ctypes.c_void_p


def p(a):
    return a.ctypes.data_as(vp)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def attestation_data(rng):
    b32 = lambda: rng.bytes(32)   # noqa: E731
    u = lambda: int(rng.integers(0, 1 << 40))   # noqa: E731
    return {"beacon_block_root": b32(), "source_epoch": u(), "source_root": b32(), "target_epoch": u(), "target_root": b32(),
            "crosslink": {"shard": u(), "start_epoch": u(), "end_epoch": u(), "parent_root": b32(), "data_root": b32()}}


def workloads(S, rng):
    bits = lambda: rng.bytes(int(rng.integers(16, 513)))   # noqa: E731
    idx = lambda k: [int(x) for x in rng.integers(0, 1 << 22, k)]   # noqa: E731
    indexed = lambda a, b: {"custody_bit_0_indices": idx(a), "custody_bit_1_indices": idx(b), "data": attestation_data(rng),   # noqa: E731
                            "signature": rng.bytes(96)}
    return [
        ("pending_8192", S.PendingAttestation, True,
         [{"aggregation_bitfield": bits(), "data": attestation_data(rng), "inclusion_delay": 1 + i % 64, "proposer_index": i}
          for i in range(8192)]),
        ("attestations_128", S.Attestation, True,
         [{"aggregation_bitfield": bits(), "data": attestation_data(rng), "custody_bitfield": bits(), "signature": rng.bytes(96)}
          for _ in range(128)]),
        ("slashing_4x4096", S.AttesterSlashing, False,
         [{"attestation_1": indexed(4096, 4096), "attestation_2": indexed(4096, 4096)}]),
        ("indexed_4096", S.IndexedAttestation, False, [indexed(4096, 0)]),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssz_ragged_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    import build_native
    from bls381_amd import _native, ssz as S
    _native.init(0)
    L = _native.lib()
    H = ctypes.CDLL(build_native.build_hostcheck())
    H.hc_ssz_ragged_root.argtypes = [vp, ctypes.c_uint32, vp, ctypes.c_uint32, vp]
    H.hc_ssz_ragged_root.restype = ctypes.c_int
    stream = lambda: vp(torch.cuda.current_stream().cuda_stream)   # noqa: E731
    result = {"batch": BATCH,
              "timing": "device: device events around %d back-to-back _device calls on resident items after a warm-up, "
                        "median of the batches (warm: the items fit the last-level cache); host build: one thread, wall "
                        "time of a pass over all items, the best of three; per-element path: wall time, once" % BATCH,
              "runs": []}
    rng = np.random.default_rng(0x55A)
    for name, typ, as_list, values in workloads(S, rng):
        items = [S.serialize(typ, v) for v in values]
        n, blob, prog = len(items), b"".join(items), S.compile_root(typ)
        starts = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in items], out=starts[1:])
        # the host build, one thread
        out = ctypes.create_string_buffer(32)
        host_roots, host_ms = [], []
        for _ in range(3):
            host_roots = []
            t0 = time.perf_counter()
            for x in items:
                assert H.hc_ssz_ragged_root(x, len(x), p(prog), len(prog), out) == 0
                host_roots.append(out.raw)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        d_items = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        d_starts = torch.from_numpy(starts).cuda()
        d_roots = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
        d_status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_root = torch.zeros(32, dtype=torch.uint8, device="cuda")
        d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = torch.empty(max(L.bls381_ssz_ragged_roots_workspace_size(n), L.bls381_ssz_ragged_list_root_workspace_size(n)),
                         dtype=torch.uint8, device="cuda")

        def roots_call():
            _native.check(L.bls381_ssz_ragged_roots_device(n, d_items.data_ptr(), len(blob), d_starts.data_ptr(), p(prog), len(prog),
                                                           d_roots.data_ptr(), d_status.data_ptr(), d_bad.data_ptr(), ws.data_ptr(),
                                                           stream()))

        def list_call():
            _native.check(L.bls381_ssz_ragged_list_root_device(n, d_items.data_ptr(), len(blob), d_starts.data_ptr(), p(prog),
                                                               len(prog), 1, d_root.data_ptr(), d_bad.data_ptr(), ws.data_ptr(),
                                                               stream()))

        def timed(call):
            call()
            call()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BATCH):
                    call()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) / BATCH)
            return spread(times)

        row = {"workload": name, "items": n, "bytes": len(blob), "item_bytes_max": max(len(x) for x in items),
               "roots_ms": timed(roots_call), "host_build_one_thread_ms": min(host_ms)}
        raw = bytes(d_roots.cpu().numpy())
        assert [raw[32 * i:32 * i + 32] for i in range(n)] == host_roots and int(d_bad.item()) == 0
        if as_list:
            row["list_root_ms"] = timed(list_call)
            want = S.merkle_root(host_roots, S.chunk_depth(n), 0, n)
            assert bytes(d_root.cpu().numpy()) == want
        if name == "pending_8192":
            t0 = time.perf_counter()
            per_elem = []
            for v in values:
                fr = [S.hash_tree_root(ft, v[fname]) for fname, ft in typ[1]]
                per_elem.append(S.merkle_root(fr, S.chunk_depth(len(fr))))
            slow = S.merkle_root(per_elem, S.chunk_depth(n), 0, n)
            row["per_element_path_ms"] = (time.perf_counter() - t0) * 1e3
            row["per_element_path_calls"] = n * (len(typ[1]) + 1) + 1
            assert slow == want
            t0 = time.perf_counter()
            assert S.hash_tree_root(S.List(typ), values) == want
            row["hash_tree_root_python_ms"] = (time.perf_counter() - t0) * 1e3   # serialization in Python included
        result["runs"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
