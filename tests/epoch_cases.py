"""Cases shared by test_epoch_host.py and test_epoch_gpu.py (test infrastructure)."""
import hashlib
import random

import numpy as np

import epoch_model as M

FAR = M.FAR_FUTURE_EPOCH
ETH = 10 ** 9
MAX_EB = 32 * ETH
# wave (64), workgroup (256) and tile (2,048) edges of the compaction
ACTIVE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 5]
# 513 tiles: the scan's one workgroup loops three times
ACTIVE_LARGE = (1 << 20) + 3
ROOT_SIZES = [0, 1, 3, 4, 5, 1024, 1025]
# the digest edge (32 tries share a digest) and the window edge (256 tries a window)
WINNING_TRIES = [0, 31, 32, 255, 256, 257]


def u64(values):
    return np.array(values, dtype=np.uint64)


def active_patterns(n, seed=7):
    """name -> (activation_epochs, exit_epochs, epoch) as uint64 arrays and an int."""
    rng = random.Random(seed * 1000003 + n)
    out = {}
    out["all"] = (u64([0] * n), u64([FAR] * n), 5)
    out["none"] = (u64([FAR] * n), u64([FAR] * n), 5)
    out["alternating"] = (u64([0 if i % 2 else FAR for i in range(n)]), u64([FAR] * n), 5)
    out["ends"] = (u64([0 if i in (0, n - 1) else 9 for i in range(n)]), u64([FAR] * n), 5)
    # epoch == activation is active, epoch == exit is not
    out["edges"] = (u64([rng.choice([4, 5, 6]) for _ in range(n)]), u64([rng.choice([5, 6, 7]) for _ in range(n)]), 5)
    # epochs at and above 2^63 and FAR_FUTURE_EPOCH in both fields: a signed comparison fails these
    big = [0, 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, FAR - 1, FAR]
    out["unsigned"] = (u64([rng.choice(big) for _ in range(n)]), u64([rng.choice(big) for _ in range(n)]), 2 ** 63)
    out["unsigned_far"] = (u64([rng.choice(big) for _ in range(n)]), u64([rng.choice(big) for _ in range(n)]), FAR - 1)
    out["mixed"] = (u64([rng.choice([0, 3, 5, 6, FAR]) for _ in range(n)]),
                    u64([rng.choice([FAR, 5, 6, 4, 2 ** 63]) for _ in range(n)]), 5)
    return out


def balances(n, seed=11):
    rng = random.Random(seed + n)
    return u64([rng.choice([0, 1, 16, 31, 32, 32]) * ETH + rng.randrange(2) for _ in range(n)])


def expected_active(act, ext, epoch):
    return np.flatnonzero((act <= np.uint64(epoch)) & (np.uint64(epoch) < ext)).astype(np.uint32)


def expected_total(bal, active):
    return sum(int(bal[i]) for i in active) % (1 << 64)


def records_at_odd_base(act, ext, bal, seed=3):
    """(buffer, base): serialized Validator records with random other bytes, starting at an odd
    offset ``base`` of an 8-byte aligned buffer."""
    rec = M.validator_records([int(v) for v in act], [int(v) for v in ext], [int(v) for v in bal], random.Random(seed))
    base = 3
    buf = np.frombuffer(bytes(base) + rec + bytes(8), dtype=np.uint8).copy()
    return buf, base


def first_zero_byte_try(seed: bytes, limit: int):
    """With balances all 0 a try accepts exactly when its random byte is 0: the winning try of
    such a committee under ``seed``, or None when none below ``limit`` accepts."""
    for q in range((limit + 31) // 32):
        d = hashlib.sha256(seed + q.to_bytes(8, "little")).digest()
        k = d.find(0)
        if k >= 0:
            return 32 * q + k if 32 * q + k < limit else None
    return None


_SEEDS = {}


def seed_with_winning_try(want):
    """A seed under which a zero-balance committee's winning try is ``want`` (an int), or above
    512 for want == 'late'.  Found with the model's rule on the CPU."""
    if want not in _SEEDS:
        for k in range(1 << 20):
            seed = hashlib.sha256(b"proposer seed" + k.to_bytes(4, "little")).digest()
            t = first_zero_byte_try(seed, 4096)
            if t is not None and ((want == "late" and t > 512) or t == want):
                _SEEDS[want] = (seed, t)
                break
    return _SEEDS[want]


def committee_of(length, n_validators, seed=5):
    rng = random.Random(seed + length)
    return np.array([rng.randrange(n_validators) for _ in range(length)], dtype=np.uint32)
