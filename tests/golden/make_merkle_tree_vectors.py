"""Generate tests/golden/merkle_trees.json: roots and proofs of the reference's Merkle trees.

The reference's own test_libs/pyspec/eth2spec/utils/merkle_minimal.py (pure, hashlib only) is
imported, as make_deposit_tree_vectors.py does.  Leaf i of tree `id` is
sha256(b"leaf" + id (4 B LE) + i (8 B LE)); the file holds digests, not leaves.

  "trees"    n leaves from index 0: get_merkle_root, the SHA-256 of all n get_merkle_proofs
             concatenated, the proofs of indices n, n+1 and 2^31 in full, merkleize_chunks
  "chunks0"  merkleize_chunks([])
  "large"    n in {65537, 262145}: the two roots only
  "windows"  (first, n): the root over [ZERO] * first + leaves, and the proofs of first,
             first+n-1 and 0

The tests read the JSON only.

Run: python tests/golden/make_merkle_tree_vectors.py <reference checkout>/test_libs/pyspec
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

SIZES = (1, 2, 3, 5, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
LARGE = (65537, 262145)
WINDOWS = ((1, 1), (3, 2), (511, 2), (512, 1), (700, 600))
ZERO = b"\x00" * 32


def leaves_of(tree_id: int, n: int):
    return [hashlib.sha256(b"leaf" + tree_id.to_bytes(4, "little") + i.to_bytes(8, "little")).digest()
            for i in range(n)]


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "eth2spec")):
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from eth2spec.utils import merkle_minimal as mm   # pure: hashlib via eth2spec.utils.hash_function

    def proof(tree, i):
        return [bytes(s).hex() for s in mm.get_merkle_proof(tree, i)]

    out = {"depth": 32, "chunks0": bytes(mm.merkleize_chunks([])).hex(), "trees": [], "large": [], "windows": []}
    tree_id = 0
    for n in SIZES:
        leaves = leaves_of(tree_id, n)
        tree = mm.calc_merkle_tree_from_leaves(leaves)
        assert mm.get_merkle_root(leaves) == tree[-1][0]
        every = hashlib.sha256(b"".join(b"".join(mm.get_merkle_proof(tree, i)) for i in range(n))).hexdigest()
        out["trees"].append({"id": tree_id, "n": n, "root": bytes(tree[-1][0]).hex(), "proofs_sha256": every,
                             "proofs": {str(i): proof(tree, i) for i in (n, n + 1, 2 ** 31)},
                             "chunks_root": bytes(mm.merkleize_chunks(leaves)).hex()})
        tree_id += 1
    for n in LARGE:
        leaves = leaves_of(tree_id, n)
        out["large"].append({"id": tree_id, "n": n, "root": bytes(mm.get_merkle_root(leaves)).hex(),
                             "chunks_root": bytes(mm.merkleize_chunks(leaves)).hex()})
        tree_id += 1
    for first, n in WINDOWS:
        leaves = leaves_of(tree_id, n)
        tree = mm.calc_merkle_tree_from_leaves([ZERO] * first + leaves)
        out["windows"].append({"id": tree_id, "first": first, "n": n, "root": bytes(tree[-1][0]).hex(),
                               "proofs": {str(i): proof(tree, i) for i in (first, first + n - 1, 0)}})
        tree_id += 1
    with open(os.path.join(HERE, "merkle_trees.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote merkle_trees.json")


if __name__ == "__main__":
    main()
