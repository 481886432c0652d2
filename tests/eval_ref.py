"""Exact reference of csp_minsnap_eval_batch and csp_minsnap_eval_batch_vjp (TEST INFRASTRUCTURE ONLY).

The contract (include/csp_minsnap.h) fixes cum, t_c, j and tau as fp64 operations, so segments() computes them in numpy
fp64 by rules 1-4: they are the kernel's own bits.  Everything after that is exact rational arithmetic on the fp64
inputs.  Every fp64 number is a dyadic rational, so the rationals that occur are n * 2**e with integer n: Dy holds an
array of them as Python integers over one shared exponent, which is the same arithmetic as fractions.Fraction on the same
inputs (Dy.fractions() converts, and tests/test_eval_math.py checks the two against each other) at a fraction of the cost.

For every output the reference returns the exact value and A, the sum of the absolute values of all products that enter
it; the tests' gate is the running-error bound gamma(n) * A (gamma(), below).  A is evaluated in fp64 (relative error
1e-15, nothing against the factor n in the gate).
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53


def gamma(n):
    """n u / (1 - n u), u = 2**-53, for a count or an array of counts."""
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def falling(p, d):
    """p (p-1) ... (p-d+1); zero for p < d."""
    r = 1
    for i in range(d):
        r *= max(p - i, 0)
    return r


class Dy:
    """An array of exact dyadic rationals n * 2**e: n an object array of Python ints, e one int."""

    def __init__(self, n, e):
        self.n, self.e = n, int(e)

    @staticmethod
    def of(x):
        x = np.asarray(x, dtype=np.float64)
        assert np.all(np.isfinite(x))
        m, ex = np.frexp(x)
        n = np.ldexp(m, 53).astype(np.int64).astype(object)          # exact: |m| < 1 has 53 bits
        ex = ex.astype(np.int64) - 53
        e = int(ex.min()) if x.size else 0
        return Dy(n * (2 ** (ex - e).astype(object)), e)

    @staticmethod
    def zeros(shape):
        z = np.empty(shape, dtype=object)
        z[...] = 0
        return Dy(z, 0)

    @property
    def shape(self):
        return self.n.shape

    def __getitem__(self, idx):
        return Dy(self.n[idx], self.e)

    def __mul__(self, o):
        if isinstance(o, Dy):
            return Dy(self.n * o.n, self.e + o.e)
        return Dy(self.n * int(o), self.e)

    def _aligned(self, o):
        e = min(self.e, o.e)
        return self.n * (1 << (self.e - e)), o.n * (1 << (o.e - e)), e

    def __add__(self, o):
        a, b, e = self._aligned(o)
        return Dy(a + b, e)

    def __sub__(self, o):
        a, b, e = self._aligned(o)
        return Dy(a - b, e)

    def __neg__(self):
        return Dy(-self.n, self.e)

    def where(self, mask):
        """The entries where mask holds, zero elsewhere."""
        return Dy(np.where(mask, self.n, 0), self.e)

    def sum(self, axis):
        return Dy(self.n.sum(axis=axis), self.e)

    def fractions(self):
        s = Fraction(2) ** self.e
        out = np.empty(self.n.shape, dtype=object)
        for i, v in np.ndenumerate(self.n):
            out[i] = Fraction(int(v)) * s
        return out

    def floats(self):
        """Rounded to fp64 (to within one ulp: for printing and for |exact| in the fp32 gate)."""
        out = np.empty(self.n.shape, dtype=np.float64)
        for i, v in np.ndenumerate(self.n):
            v, e = int(v), self.e
            b = v.bit_length()
            if b > 64:
                v >>= b - 64
                e += b - 64
            out[i] = math.ldexp(float(v), e)
        return out

    def abs_err(self, got):
        """|got - exact| for an fp64 or fp32 array of the same shape, formed exactly and then rounded."""
        got = np.asarray(got, dtype=np.float64)
        return np.abs((Dy.of(got) - self).floats())


def segments(times, query):
    """Rules 1-4 in numpy fp64 for one uniform batch: times [B,S], query [B,Q] ->
    cum [B,S+1], j [B,Q] (-1 for an inf / NaN query), tau [B,Q], low, high, valid [B,Q]."""
    times, query = np.asarray(times, np.float64), np.asarray(query, np.float64)
    B, S = times.shape
    cum = np.zeros((B, S + 1))
    for j in range(S):                       # left to right, one rounding per addition
        cum[:, j + 1] = cum[:, j] + times[:, j]
    valid = np.isfinite(query)
    t = np.where(valid, query, 0.0)
    low, high = valid & (t < 0.0), valid & (t > cum[:, -1:])
    tc = np.minimum(np.maximum(t, 0.0), cum[:, -1:])
    j = np.zeros(query.shape, dtype=np.int64)
    for b in range(B):
        j[b] = np.minimum(np.searchsorted(cum[b], tc[b], side="right") - 1, S - 1)
    tau = tc - np.take_along_axis(cum, j, axis=1)
    j = np.where(valid, j, -1)
    return cum, j, tau, low, high, valid


class Ref:
    """Exact forward and reverse mode of one UNIFORM batch with finite, non-negative times and finite coefficients.
    times [B,S], coeffs [B,S,3,M], query [B,Q] as fp64 arrays holding the stored values (fp32 inputs converted).  A
    query that is inf or NaN gets seg -1, zero exact values (the caller checks for NaN there) and no contribution."""

    def __init__(self, times, coeffs, query, max_deriv):
        self.times, self.coeffs, self.query = (np.asarray(x, np.float64) for x in (times, coeffs, query))
        self.B, self.S = self.times.shape
        self.M = self.coeffs.shape[-1]
        self.Q = self.query.shape[1]
        self.cum, self.seg, self.tau, self.low, self.high, self.valid = segments(self.times, self.query)
        jj = np.maximum(self.seg, 0)
        # the record of every query: [B,Q,3,M]
        self.rec = np.take_along_axis(self.coeffs, jj[:, :, None, None], axis=1)
        rec = Dy.of(self.rec)
        tau = Dy.of(self.tau)
        pw = [Dy.of(np.ones_like(self.tau))]
        for _ in range(1, self.M):
            pw.append(pw[-1] * tau)
        self.pw = pw
        fpw = [np.ones_like(self.tau)]
        for _ in range(1, self.M):
            fpw.append(fpw[-1] * self.tau)
        self.fpw = fpw
        # x[d] exact [B,Q,3] and its A, for d = 0 .. max_deriv
        self.x, self.xA = [], []
        for d in range(max_deriv + 1):
            acc, A = Dy.zeros((self.B, self.Q, 3)), np.zeros((self.B, self.Q, 3))
            for k in range(self.M):
                p = self.M - 1 - k
                if p < d:
                    continue
                f = falling(p, d)
                acc = acc + rec[:, :, :, k] * Dy(pw[p - d].n[:, :, None] * f, pw[p - d].e)
                A = A + np.abs(self.rec[:, :, :, k]) * (f * fpw[p - d])[:, :, None]
            self.x.append(acc.where(self.valid[:, :, None]))
            self.xA.append(np.where(self.valid[:, :, None], A, 0.0))

    def values(self, D):
        """(exact Dy [B,Q,D,3], A [B,Q,D,3])"""
        e = min(x.e for x in self.x[:D])
        n = np.stack([x.n * (1 << (x.e - e)) for x in self.x[:D]], axis=2)
        return Dy(n, e), np.stack(self.xA[:D], axis=2)

    def vjp(self, g):
        """g [B,Q,D,3] -> dict of (exact Dy, A) for 'coeffs' [B,S,3,M], 'times' [B,S], 'query' [B,Q], and 'count' [B,S],
        the number of queries in each segment."""
        g = np.asarray(g, np.float64)
        D = g.shape[2]
        gd = Dy.of(g)
        # g_tau and its A
        gt, gtA = Dy.zeros((self.B, self.Q)), np.zeros((self.B, self.Q))
        for d in range(D):
            gt = gt + (gd[:, :, d, :] * self.x[d + 1]).sum(axis=2)
            gtA = gtA + (np.abs(g[:, :, d, :]) * self.xA[d + 1]).sum(axis=2)
        inr = self.valid & ~self.low & ~self.high
        gq, gqA = gt.where(inr), np.where(inr, gtA, 0.0)
        # grad_times
        tn = np.empty((self.B, self.S), dtype=object)
        tA = np.zeros((self.B, self.S))
        hi = gt.where(self.high)
        for i in range(self.S):
            later = inr & (self.seg > i)
            col = -gt.where(later).n.sum(axis=1)
            a = np.where(later, gtA, 0.0).sum(axis=1)
            if i == self.S - 1:
                col = col + hi.n.sum(axis=1)
                a = a + np.where(self.high, gtA, 0.0).sum(axis=1)
            tn[:, i], tA[:, i] = col, a
        # grad_coeffs: per query column, every trajectory adds into the record of its own segment
        ok = self.valid
        rows = np.arange(self.B)
        terms, tA_terms = [], []
        e = None
        for k in range(self.M):
            p = self.M - 1 - k
            acc, A = Dy.zeros((self.B, self.Q, 3)), np.zeros((self.B, self.Q, 3))
            for d in range(min(D, p + 1)):
                f = falling(p, d)
                acc = acc + gd[:, :, d, :] * Dy(self.pw[p - d].n[:, :, None] * f, self.pw[p - d].e)
                A = A + np.abs(g[:, :, d, :]) * (f * self.fpw[p - d])[:, :, None]
            terms.append(acc.where(ok[:, :, None]))
            tA_terms.append(np.where(ok[:, :, None], A, 0.0))
        e = min(t.e for t in terms)
        cn = np.empty((self.B, self.S, 3, self.M), dtype=object)
        cn[...] = 0
        cA = np.zeros((self.B, self.S, 3, self.M))
        count = np.zeros((self.B, self.S), dtype=np.int64)
        jj = np.maximum(self.seg, 0)
        for k in range(self.M):
            n = terms[k].n * (1 << (terms[k].e - e))
            for q in range(self.Q):
                cn[rows, jj[:, q], :, k] += n[:, q, :]
                cA[rows, jj[:, q], :, k] += tA_terms[k][:, q, :]
        for q in range(self.Q):
            count[rows, jj[:, q]] += ok[:, q]
        return {"coeffs": (Dy(cn, e), cA), "times": (Dy(tn, gt.e), tA), "query": (gq, gqA), "count": count}
