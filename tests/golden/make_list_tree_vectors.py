"""Generate tests/golden/list_tree_history.json: scripted histories of appends and in-place
updates of three SSZ lists, with the list's root after every step, from the reference's Merkle
code.

The reference's own test_libs/pyspec/eth2spec/utils/merkle_minimal.py (pure, hashlib only) is
imported, as make_merkle_tree_vectors.py does: every root is its merkleize_chunks over the
list's chunks as they stand, and mix_in_length (ssz_impl.py:122-124, restated with the
reference's hash because ssz_impl.py does not import on this Python) of that root and the count.
The chunk of a Validator record is merkleize_chunks over its eight field chunks (a Bytes48 field:
merkleize_chunks of its two chunks), ssz_impl.py:143-155.

Three lists: "validator" (121-byte Validator records, a chunk per record), "uint64" (8-byte
items, four to a chunk) and "bytes32" (32-byte items, the chunks themselves).  Each history is
about 40 steps:
  {"op": "append", "items": [hex ...]}
  {"op": "update", "indices": [...], "off": o, "len": l, "values": [hex ...]}
each with "root" (mixed with the count) and "root_unmixed"; "final" is the list after the last
step.  Updates of Validator records include the fields the state transition writes:
effective_balance (off 113, len 8), slashed (112, 1), exit_epoch (96, 8).

The tests read the JSON only.

Run: python tests/golden/make_list_tree_vectors.py <reference checkout>/test_libs/pyspec
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

STEPS = 40
VALIDATOR_FIELDS = ((0, 48), (48, 32), (80, 8), (88, 8), (96, 8), (104, 8), (112, 1), (113, 8))   # (offset, length)
LISTS = (("validator", 121, ((0, 121), (113, 8), (112, 1), (96, 8))),
         ("uint64", 8, ((0, 8),)),
         ("bytes32", 32, ((0, 32), (4, 3))))


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "eth2spec")):
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from eth2spec.utils import merkle_minimal as mm   # pure: hashlib via eth2spec.utils.hash_function

    def chunkify(b):
        b = b + b"\x00" * (-len(b) % 32)
        return [b[i:i + 32] for i in range(0, len(b), 32)]

    def chunks_of(name, items):
        if name != "validator":
            return chunkify(b"".join(items))
        return [bytes(mm.merkleize_chunks([bytes(mm.merkleize_chunks(chunkify(it[o:o + n]))) for o, n in VALIDATOR_FIELDS]))
                for it in items]

    out = {}
    for name, size, spans in LISTS:
        rng = random.Random("list tree " + name)
        items, steps = [], []
        for s in range(STEPS):
            if s < 3 or rng.random() < 0.45:
                new = [rng.randbytes(size) for _ in range(rng.choice((1, 1, 2, 3, 5, 9)))]
                if name == "validator":
                    new = [it[:112] + bytes([it[112] & 1]) + it[113:] for it in new]      # slashed is a bool
                items += new
                step = {"op": "append", "items": [it.hex() for it in new]}
            else:
                off, length = spans[rng.randrange(len(spans))]
                idx = sorted(rng.sample(range(len(items)), min(len(items), rng.choice((1, 1, 2, 4)))))
                vals = [rng.randbytes(length) for _ in idx]
                if name == "validator" and off <= 112 < off + length:
                    vals = [v[:112 - off] + bytes([v[112 - off] & 1]) + v[113 - off:] for v in vals]
                for i, v in zip(idx, vals):
                    items[i] = items[i][:off] + v + items[i][off + length:]
                step = {"op": "update", "indices": idx, "off": off, "len": length, "values": [v.hex() for v in vals]}
            root = bytes(mm.merkleize_chunks(chunks_of(name, items)))
            step["root_unmixed"] = root.hex()
            step["root"] = bytes(mm.hash(root + len(items).to_bytes(32, "little"))).hex()
            steps.append(step)
        out[name] = {"item_size": size, "steps": steps, "final": [it.hex() for it in items]}
    with open(os.path.join(HERE, "list_tree_history.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote list_tree_history.json:", {k: len(v["final"]) for k, v in out.items()})


if __name__ == "__main__":
    main()
