"""Generate tests/golden/deposit_tree_history.json: the deposit tree's root at every count and
proofs under roots of earlier counts, from the reference's Merkle code.

The reference's own test_libs/pyspec/eth2spec/utils/merkle_minimal.py (pure, hashlib only) is
imported, as make_merkle_tree_vectors.py does.  Leaf i of tree `id` is
sha256(b"leaf" + id (4 B LE) + i (8 B LE)), merkle_model.leaves_of(id, n); the file holds
digests, not leaves.

  "roots"   roots[k-1] = get_merkle_root(leaves[:k]) for every k = 1 .. n
  "proofs"  for (k, i) pairs -- i = k-1, i = 0, an inner leaf, a zero leaf, k on both sides of
            256 -- get_merkle_proof(calc_merkle_tree_from_leaves(leaves[:k]), i) in full

The tests read the JSON only.

Run: python tests/golden/make_deposit_tree_history_vectors.py <reference checkout>/test_libs/pyspec
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

TREE_ID = 300
N = 300
PAIRS = ((1, 0), (2, 1), (3, 0), (100, 99), (100, 37), (255, 254), (255, 0), (256, 255), (256, 128), (257, 256),
         (257, 0), (257, 255), (300, 299), (300, 0), (300, 300), (7, 2 ** 31))


def leaves_of(tree_id: int, n: int):
    return [hashlib.sha256(b"leaf" + tree_id.to_bytes(4, "little") + i.to_bytes(8, "little")).digest()
            for i in range(n)]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "eth2spec")):
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from eth2spec.utils import merkle_minimal as mm   # pure: hashlib via eth2spec.utils.hash_function

    leaves = leaves_of(TREE_ID, N)
    out = {"depth": 32, "id": TREE_ID, "n": N,
           "roots": [bytes(mm.get_merkle_root(leaves[:k])).hex() for k in range(1, N + 1)], "proofs": []}
    for k, i in PAIRS:
        tree = mm.calc_merkle_tree_from_leaves(leaves[:k])
        assert bytes(tree[-1][0]).hex() == out["roots"][k - 1]
        out["proofs"].append({"k": k, "i": i, "proof": [bytes(s).hex() for s in mm.get_merkle_proof(tree, i)]})
    with open(os.path.join(HERE, "deposit_tree_history.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote deposit_tree_history.json")


if __name__ == "__main__":
    main()
