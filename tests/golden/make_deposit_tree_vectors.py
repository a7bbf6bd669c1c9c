"""Generate tests/golden/deposit_tree.json: deposit-tree roots and Merkle proofs.

The reference's own test_libs/pyspec/eth2spec/utils/merkle_minimal.py (pure,
hashlib only) is imported, as make_ssz_vectors.py does, and for 1, 2, 5 and 8
random leaves the file records the leaves, get_merkle_root and every
get_merkle_proof (depth 32, the deposit contract's tree).  The tests read the
JSON only.

Run: python tests/golden/make_deposit_tree_vectors.py <reference checkout>/test_libs/pyspec
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "eth2spec")):
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    from eth2spec.utils import merkle_minimal as mm   # pure: hashlib via eth2spec.utils.hash_function
    rng = random.Random(0xB15_0009)
    out = {"depth": 32, "zerohashes": [bytes(h).hex() for h in mm.zerohashes], "trees": []}
    for n in (1, 2, 5, 8):
        leaves = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]
        tree = mm.calc_merkle_tree_from_leaves(leaves)
        assert mm.get_merkle_root(leaves) == tree[-1][0]
        out["trees"].append({"leaves": [x.hex() for x in leaves], "root": bytes(tree[-1][0]).hex(),
                             "proofs": [[bytes(s).hex() for s in mm.get_merkle_proof(tree, i)] for i in range(n)]})
    with open(os.path.join(HERE, "deposit_tree.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote deposit_tree.json")


if __name__ == "__main__":
    main()
