"""Generate tests/golden/hash_search.json: hash_to_G2 inputs chosen by their try-and-increment
trial count, and edge scalars for privtopub / sign.

Random messages almost never need more than ten trials, so the device searches (the pair-sequential
one, the 16-lane wide one with its known-offset consumers, the wave-pooled one) never see the inputs
on which they differ: a second wide round needs 17 trials or more.  This generator searches for them.

* messages: msg_i = sha256(TAG || i as 4 big-endian bytes) under the one DOMAIN, for i < LIMIT.  The
  search tests x^3 + 4(1 + i) for squareness through the Legendre symbol of its norm (Python
  integers, WORKERS processes); every kept message's trial count is then confirmed with
  oracle.hash_to_G2_affine_candidate.  Kept, lowest i first: 64 messages for each trial count 1..6, 8
  for each of 7..15, 4 with exactly 16, and up to 8 with 17 or more (the highest counts first).  Per
  message: i, trials and the 64-bit mask of the square offsets 0..63 (the pooled search's later
  rounds test offsets past the first square).
  A trial count of 33 or more (a third round of the wide search) costs about 2^32 candidates: out of
  scope.
* points: for two messages of every trial count and every message of 16 or more -- the candidate
  after root selection, hash_to_G2 compressed / affine / py_ecc projective, the verification hash
  BP(H0) = [3(x^2 - 1) mod r] hash_to_G2 (x the curve parameter) affine, and two wrong signatures:
  the hash built from the NEXT square offset after the first, and the negated hash.
* lengths: messages at the SHA-256 padding edges of msg || dom8 || tag, with trials and compressed hash.
* scalars: K (0, 1, .., r - 1, r, r + 1, r + 2, .., 2r + 4, powers of two, 2^256 - 1, three random
  values >= r) with oracle.privtopub(k) and oracle.sign(m, k, DOMAIN) for two messages, one of an
  even and one of an odd trial count.

Deterministic: the output does not depend on the number of workers.
Run:  python tests/golden/make_hash_search_vectors.py [OUT]   (8 processes: about a minute and a half;
OUT: another file to write, to compare with the committed one)
"""
import hashlib
import json
import multiprocessing
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import bls_oracle as O  # noqa: E402

TAG = b"trial-search"
DOMAIN = 7
LIMIT = 1 << 20
CHUNK = 1 << 12
WORKERS = min(16, os.cpu_count() or 1)
LENGTHS = [46, 47, 54, 55, 56, 63, 64, 110, 111, 119, 120]
BP_SCALAR = 3 * (O.BLS_X ** 2 - 1) % O.r
q, r = O.q, O.r


def msg_of(i):
    return hashlib.sha256(TAG + i.to_bytes(4, "big")).digest()


def len_msg(n):
    return (hashlib.sha256(TAG + b"/len" + bytes([n])).digest() * 4)[:n]


def x0_of(msg, domain=DOMAIN):
    d = O.domain_to_bytes8(domain)
    return (int.from_bytes(hashlib.sha256(msg + d + b"\x01").digest(), "big") % q,
            int.from_bytes(hashlib.sha256(msg + d + b"\x02").digest(), "big") % q)


def is_square(x):
    """x^3 + 4(1 + i) is a square of Fp2: its norm is a square of Fp."""
    a, b = O.f2_add(O.f2_mul(O.f2_sqr(x), x), O.B2)
    n = (a * a + b * b) % q
    return n == 0 or pow(n, (q - 1) // 2, q) == 1


def trials_of(msg):
    re, im = x0_of(msg)
    t = 1
    while not is_square(((re + t - 1) % q, im)):
        t += 1
    return t


def square_mask(msg):
    re, im = x0_of(msg)
    return sum(1 << k for k in range(64) if is_square(((re + k) % q, im)))


def scan(c):
    """One chunk of i: every (i, trials) of 7 or more trials, the first 64 of each count below."""
    out, seen = [], {}
    for i in range(c * CHUNK, (c + 1) * CHUNK):
        t = trials_of(msg_of(i))
        if t <= 6:
            seen[t] = seen.get(t, 0) + 1
            if seen[t] > 64:
                continue
        out.append((i, t))
    return out


def quota(t):
    return 64 if t <= 6 else 8 if t <= 15 else 4


def choose(found):
    """found: (i, trials) in order of i."""
    by = {}
    for i, t in found:
        by.setdefault(t, []).append(i)
    keep = []
    for t in range(1, 17):
        assert len(by.get(t, [])) >= quota(t), ("too few messages of trial count", t)
        keep += [(i, t) for i in by[t][:quota(t)]]
    high = sorted(((i, t) for i, t in found if t >= 17), key=lambda e: (-e[1], e[0]))
    above = [e for e in high if e[1] >= 18][:5]
    high = above + [e for e in high if e[1] == 17][:8 - len(above)]
    assert len(high) >= 4 and above
    return keep + sorted(high, key=lambda e: (e[1], e[0]))


def fq2_hex(c):
    return [c[0].to_bytes(48, "big").hex(), c[1].to_bytes(48, "big").hex()]


def point_record(e):
    i, t, mask = e
    msg = msg_of(i)
    x, y, trials = O.hash_to_G2_affine_candidate(msg, DOMAIN)
    assert trials == t
    H = O.hash_to_G2(msg, DOMAIN)
    ax, ay = O.g2_affine(H)
    bx, by = O.g2_affine(O.pt_multiply(O.Fq2Ops, H, BP_SCALAR))
    # the next square offset after the first: the point a search that skipped the first would give
    k2 = next(k for k in range(t, 64) if (mask >> k) & 1)
    x2 = ((x[0] + k2 - (t - 1)) % q, x[1])
    y2 = O.modular_squareroot(O.f2_add(O.f2_mul(O.f2_sqr(x2), x2), O.B2))
    assert y2 is not None
    H2 = O.pt_multiply(O.Fq2Ops, (x2, y2, O.FQ2_ONE), O.G2_cofactor)
    return {"i": i, "trials": t, "candidate": fq2_hex(x) + fq2_hex(y),
            "compressed": O.G2_to_signature(H).hex(), "affine": fq2_hex(ax) + fq2_hex(ay),
            "bp_affine": fq2_hex(bx) + fq2_hex(by),
            "projective": [h[2:] for c in O.g2_projective_to_hex(H) for h in c],
            "next_offset": k2, "next_square_sig": O.G2_to_signature(H2).hex(),
            "negated_sig": O.G2_to_signature(O.pt_neg(O.Fq2Ops, H)).hex()}


def confirm(e):
    assert O.hash_to_G2_affine_candidate(msg_of(e[0]), DOMAIN)[2] == e[1], e
    return e[0], e[1], square_mask(msg_of(e[0]))


def length_record(n):
    m = len_msg(n)
    return {"length": n, "trials": O.hash_to_G2_affine_candidate(m, DOMAIN)[2],
            "compressed": O.G2_to_signature(O.hash_to_G2(m, DOMAIN)).hex()}


def scalars():
    rnd = [int.from_bytes(hashlib.sha256(TAG + b"/scalar" + bytes([j])).digest(), "big") | 1 << 255 for j in range(3)]
    K = [0, 1, 2, 3, (r - 1) // 2, (r + 1) // 2, r - 2, r - 1, r, r + 1, r + 2, 2 * r - 1, 2 * r, 2 * r + 1,
         2 * r + 3, 2 * r + 4, 1 << 31, 1 << 32, 1 << 224, 1 << 248, 1 << 255, (1 << 256) - 1] + rnd
    assert all(0 <= k < 1 << 256 for k in K) and all(k >= r for k in rnd)
    return K


def scalar_record(a):
    k, ids = a
    return {"k": hex(k), "pubkey": O.privtopub(k).hex(), "signatures": [O.sign(msg_of(i), k, DOMAIN).hex() for i in ids]}


def main():
    t0 = time.time()
    with multiprocessing.Pool(WORKERS) as pool:
        found = [e for part in pool.map(scan, range(LIMIT // CHUNK)) for e in part]
        t_search = time.time() - t0
        kept = pool.map(confirm, choose(found))
        with_points, per = [], {}
        for e in kept:
            per[e[1]] = per.get(e[1], 0) + 1
            if per[e[1]] <= 2 or e[1] >= 16:
                with_points.append(e)
        points = pool.map(point_record, with_points)
        lengths = pool.map(length_record, LENGTHS)
        even = next(e[0] for e in kept if e[1] == 16)
        odd = next(e[0] for e in kept if e[1] == 17)
        sc = pool.map(scalar_record, [(k, (even, odd)) for k in scalars()])
    out = {"tag": TAG.decode(), "domain": DOMAIN, "limit": LIMIT,
           "messages": [{"i": i, "trials": t, "squares": "%016x" % m} for i, t, m in kept],
           "points": points, "lengths": lengths, "scalar_messages": [even, odd], "scalars": sc}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "hash_search.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, separators=(",", ":"))
        f.write("\n")
    counts = {}
    for i, t in found:
        if t >= 16:
            counts[t] = counts.get(t, 0) + 1
    print("hash_search.json: %d bytes, %d messages, %d points; trial counts of 16 or more among i < 2^20: %s; "
          "search %.0f s, total %.0f s on %d processes" % (os.path.getsize(path), len(kept), len(points),
                                                          sorted(counts.items()), t_search, time.time() - t0, WORKERS))


if __name__ == "__main__":
    main()
