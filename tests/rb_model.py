"""Reference model of the randomized batch's scalar side (bls381_kernels.hpp "randomized batch
verification"): weights, statuses and classes, R1 = [r_i] pk_i, R2 = [r_i] sig_i, and the bucket
MSM of the sub-batch sums S_b -- digits, per-(sub-batch, window, digit) point lists, buckets,
window sums and the Horner combine.  Plain Python integers on oracle/bls_oracle.py and
oracle/tower_model.py; no test functions and no device calls (tests/test_rb_model.py proves it on
the CPU, tests/test_randomized_scalars.py and tests/test_randomized_soundness.py use it).

The weights follow rb_scalar's code: d = SHA-256(seed || i as 8 little-endian bytes) as eight
big-endian words, k1 = d[0] (digest bytes 0..3), k0 = d[1] (bytes 4..7), and k0 = 1 when both are 0.
"""
import hashlib

import bls_oracle as O
import tower_model as M

q, r = O.q, O.r
MU = (-(M.X_ABS ** 2)) % r          # sigma on G1 and phi = -psi^2 on G2 act as [MU]
MSM_C, MSM_W, MSM_D = 4, 8, 16      # RB_MSM_C / _W / _D
ST_OK, ST_INF, ST_BAD, ST_NOSUB = 0, 1, 2, 3
RB_BAD, RB_BATCH, RB_SINGLE = 0, 1, 2
F1, F2 = M.Fq, M.Fq2
INF1 = (1, 1, 0)
INF2 = (M.ONE2, M.ONE2, M.ZERO2)


def weight(seed, i):
    """(k0, k1) of item i: r_i = k0 + MU k1 (mod r)."""
    assert len(seed) == 32
    h = hashlib.sha256(bytes(seed) + int(i).to_bytes(8, "little")).digest()
    k1, k0 = int.from_bytes(h[0:4], "big"), int.from_bytes(h[4:8], "big")
    if (k0 | k1) == 0:
        k0 = 1
    return k0, k1


def scalar(k0, k1):
    return (k0 + MU * k1) % r


# ------------------------------------------------------------- endomorphisms --
def sigma(P):
    """(beta x, y) on an affine point of E(Fp)."""
    return (M.BETA * P[0] % q, P[1])


def phi(Q):
    """-psi^2 on an affine point of E'(Fp2)."""
    x, y = M.psi_affine(M.psi_affine(Q))
    return (x, M.neg2(y))


def jac(F, a):
    return (F.one, F.one, F.zero) if a is None else (a[0], a[1], F.one)


def mul_2x32(F, a, s, k0, k1):
    """[k0] a + [k1] s as an affine point, or None for infinity."""
    t = M.jac_add(F, M.jac_mul(F, jac(F, a), k0), M.jac_mul(F, jac(F, s), k1))
    return M.jac_to_affine(F, t)


def r1(P, k0, k1):
    """k0 P + k1 sigma(P): holds for a key outside G1 too."""
    return mul_2x32(F1, P, sigma(P), k0, k1)


def r2(Q, k0, k1):
    return mul_2x32(F2, Q, phi(Q), k0, k1)


# --------------------------------------------------------- statuses and classes --
def key_status(pk48, strict):
    """(status, affine point or None) as dev_rb_decode_g1 assigns them."""
    try:
        p = O.pubkey_to_G1(pk48, strict)
    except ValueError:
        return ST_BAD, None
    if O.pt_is_inf(O.FqOps, p):
        return ST_INF, None
    if strict and not O.in_G1(p):
        return ST_BAD, None
    return ST_OK, (p[0], p[1])


def sig_status(sig96, strict):
    """(status, affine point or None) after the codec-only decode and k_rb_g2_test."""
    try:
        p = O.signature_to_G2(sig96, strict)
    except ValueError:
        return ST_BAD, None
    if O.pt_is_inf(O.Fq2Ops, p):
        return ST_INF, None
    a = O.g2_affine(p)
    if not O.in_G2(p):
        return (ST_BAD, None) if strict else (ST_NOSUB, a)
    return ST_OK, a


def item_class(ps, ss):
    return RB_BAD if ST_BAD in (ps, ss) else (RB_SINGLE if ss == ST_NOSUB else RB_BATCH)


def batched(ps, ss):
    """The item's signature enters the sub-batch sum (rb_msm_scalars, k_rb_scale_g2)."""
    return ps != ST_BAD and ss == ST_OK


# ------------------------------------------------------------------ bucket MSM --
def digits(k):
    return [(k >> (MSM_C * w)) & (MSM_D - 1) for w in range(MSM_W)]


class Msm:
    """The bucket MSM of one call: items = [(Q affine or None when not batched)], B, seed.

    lists[b][w][d]   point numbers 2 t + h of sub-batch b with digit d in window w (d >= 1), sorted
    off[b][w]        MSM_D + 1 list starts (off[0] = off[1] = 0)
    bucket[b][w][d]  affine sum of the list's points, None for infinity
    win[b][w]        sum_d d bucket[d];  s[b]  sum_w 2^(C w) win[w]
    """

    def __init__(self, points, B, seed, first=0):
        n = len(points)
        self.n, self.B, self.nb = n, B, (n + B - 1) // B
        self.weights = [weight(seed, first + i) for i in range(n)]
        self.points = points
        self.lists, self.off, self.bucket, self.win, self.s = [], [], [], [], []
        for b in range(self.nb):
            m = min(B, n - b * B)
            L = [[[] for _ in range(MSM_D)] for _ in range(MSM_W)]
            for t in range(m):
                if points[b * B + t] is None:
                    continue
                for h in (0, 1):
                    for w, d in enumerate(digits(self.weights[b * B + t][h])):
                        if d:
                            L[w][d].append(2 * t + h)
            self.lists.append(L)
            offs = []
            for w in range(MSM_W):
                o, run = [0], 0
                for d in range(1, MSM_D):
                    o.append(run)
                    run += len(L[w][d])
                o.append(run)
                offs.append(o)
            self.off.append(offs)
            bk = [[self._sum(b, L[w][d]) for d in range(MSM_D)] for w in range(MSM_W)]
            self.bucket.append(bk)
            wn = []
            for w in range(MSM_W):
                acc = INF2
                for d in range(1, MSM_D):
                    acc = M.jac_add(F2, acc, M.jac_mul(F2, jac(F2, bk[w][d]), d))
                wn.append(M.jac_to_affine(F2, acc))
            self.win.append(wn)
            acc = INF2
            for w in range(MSM_W - 1, -1, -1):
                for _ in range(MSM_C):
                    acc = M.jac_dbl(F2, acc)
                acc = M.jac_add(F2, acc, jac(F2, wn[w]))
            self.s.append(M.jac_to_affine(F2, acc))

    def point(self, b, p):
        """Point number p of sub-batch b: item p // 2, phi applied when p is odd."""
        Q = self.points[b * self.B + p // 2]
        return phi(Q) if p & 1 else Q

    def _sum(self, b, lst):
        acc = INF2
        for p in lst:
            acc = M.jac_add(F2, acc, jac(F2, self.point(b, p)))
        return M.jac_to_affine(F2, acc)

    def ladder_sum(self, b):
        """sum_i (k0 Q_i + k1 phi(Q_i)) over the sub-batch: the per-item ladder's route."""
        acc = INF2
        for i in range(b * self.B, min(self.n, (b + 1) * self.B)):
            if self.points[i] is not None:
                acc = M.jac_add(F2, acc, jac(F2, r2(self.points[i], *self.weights[i])))
        return M.jac_to_affine(F2, acc)

    # coverage conditions of the tests (asserted from the model before a launch)
    def buckets_with_cancellation(self):
        """(b, w, d) whose list holds a point and its negative."""
        out = []
        for b in range(self.nb):
            for w in range(MSM_W):
                for d in range(1, MSM_D):
                    pts = [self.point(b, p) for p in self.lists[b][w][d]]
                    if any((x, M.neg2(y)) in pts for x, y in pts):
                        out.append((b, w, d))
        return out

    def buckets_with_repeat(self):
        """(b, w, d) whose list holds one point twice (jac_add_aff's doubling branch)."""
        out = []
        for b in range(self.nb):
            for w in range(MSM_W):
                for d in range(1, MSM_D):
                    pts = [self.point(b, p) for p in self.lists[b][w][d]]
                    if len(set(pts)) < len(pts):
                        out.append((b, w, d))
        return out

    def windows_with_run_eq_sum(self):
        """(b, w) whose top occupied digit d has bucket d - 1 at infinity: k_rb_msm_window's
        running sum and sum are then the same point and jac_add(sum, run) doubles."""
        out = []
        for b in range(self.nb):
            for w in range(MSM_W):
                occ = [d for d in range(1, MSM_D) if self.bucket[b][w][d] is not None]
                if occ and occ[-1] > 1 and self.bucket[b][w][occ[-1] - 1] is None:
                    out.append((b, w))
        return out

    def zero_digits(self):
        return sum(1 for i, (k0, k1) in enumerate(self.weights) if self.points[i] is not None
                   for k in (k0, k1) for d in digits(k) if d == 0)
