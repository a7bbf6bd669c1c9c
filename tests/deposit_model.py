"""Pure-Python restatements used by test_merkle_branch_host.py and test_process_deposits.py
(hashlib only): the fold of verify_merkle_branch, a sparse deposit tree with zero hashes, the
synthetic branch cases, and the loop of process_deposit with the signature verdicts as input.

Spec lines: specs/core/0_beacon-chain.md:846-857 (verify_merkle_branch), :1732-1775
(process_deposit)."""
import hashlib
import json
import os
import random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIPPED, NEW, TOPUP = 0, 1, 2
DEPTH = 32


def h(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def branch_root(leaf: bytes, proof, depth: int, index: int) -> bytes:
    """The spec's loop: bit i of index set -> hash(proof[i] + value), else hash(value + proof[i])."""
    value = leaf
    for i in range(depth):
        if index // (2 ** i) % 2:
            value = h(proof[i] + value)
        else:
            value = h(value + proof[i])
    return value


def verify_merkle_branch(leaf, proof, depth, index, root) -> bool:
    return branch_root(leaf, proof, depth, index) == root


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "deposit_tree.json")) as f:
        fx = json.load(f)
    return [{"leaves": [bytes.fromhex(x) for x in t["leaves"]], "root": bytes.fromhex(t["root"]),
             "proofs": [[bytes.fromhex(s) for s in p] for p in t["proofs"]]} for t in fx["trees"]]


def flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit // 8] ^= 1 << (bit % 8)
    return bytes(out)


SYNTH_DEPTHS = (0, 1, 5, 33, 64)
SYNTH_INDICES = (0, 0xAAAAAAAA, 2 ** 32 - 1, 2 ** 64 - 1)


def synthetic_cases(seed=0xB15_000A):
    """(leaf, proof, depth, index, root) with the root folded by branch_root: every depth x index."""
    rng = random.Random(seed)
    out = []
    for depth in SYNTH_DEPTHS:
        for index in SYNTH_INDICES:
            leaf = rng.randbytes(32)
            proof = [rng.randbytes(32) for _ in range(depth)]
            out.append((leaf, proof, depth, index, branch_root(leaf, proof, depth, index)))
    return out


ZERO_HASHES = [b"\x00" * 32]
for _ in range(DEPTH):
    ZERO_HASHES.append(h(ZERO_HASHES[-1] + ZERO_HASHES[-1]))


class SparseTree:
    """A depth-32 tree whose leaves sit at arbitrary indices, every other leaf zero (the deposit
    contract's tree with the batch's leaves far from index 0)."""

    def __init__(self, leaves: dict):
        self.levels = [dict(leaves)]
        for d in range(DEPTH):
            cur, nxt = self.levels[-1], {}
            for i in {k >> 1 for k in cur}:
                nxt[i] = h(cur.get(2 * i, ZERO_HASHES[d]) + cur.get(2 * i + 1, ZERO_HASHES[d]))
            self.levels.append(nxt)
        self.root = self.levels[DEPTH].get(0, ZERO_HASHES[DEPTH])

    def proof(self, index: int):
        return [self.levels[d].get((index >> d) ^ 1, ZERO_HASHES[d]) for d in range(DEPTH)]


def process_deposits_model(registry_keys, deposits, sig_ok, first_index, root, leaf_of):
    """process_deposit over `deposits` (1,208-byte serializations) in order.  registry_keys: the
    validator pubkeys before the batch (entry e = validator e); sig_ok[i]: the verdict of
    bls_verify for deposit i; leaf_of(data184) = hash_tree_root(deposit.data).  Returns
    (outcome, validator_index, first_bad_proof, n_new); like the engine, the outcomes do not
    depend on the proofs."""
    pubkeys = list(registry_keys)
    outcome, vidx, bad = [], [], -1
    for i, dep in enumerate(deposits):
        proof = [dep[32 * k:32 * k + 32] for k in range(DEPTH)]
        data = dep[32 * DEPTH:]
        if bad < 0 and not verify_merkle_branch(leaf_of(data), proof, DEPTH, first_index + i, root):
            bad = i
        pubkey = data[:48]
        if pubkey not in pubkeys:
            if not sig_ok[i]:
                outcome.append(SKIPPED)
                vidx.append(-1)
                continue
            pubkeys.append(pubkey)
            outcome.append(NEW)
        else:
            outcome.append(TOPUP)
        vidx.append(pubkeys.index(pubkey))
    return outcome, vidx, bad, outcome.count(NEW)
