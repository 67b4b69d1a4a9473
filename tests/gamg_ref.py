"""The model of PCGAMG in plain numpy / Python: the strength mask, the greedy distance-2 independent set in key order, the aggregate
rule, the tentative and the smoothed prolongator and the Galerkin operators with the library's own order of operations (so that the
prolongators come out bit for bit), and the dense hierarchy and cycle on top of mg_ref.py."""
import math

import numpy as np

import mg_ref as mr

M32 = 0xFFFFFFFF


def mix(i):
    h = i & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def key(state, i):
    return (state << 62) | ((mix(i) >> 2) << 32) | i


def diagonal(ai, aj, aa):
    m = len(ai) - 1
    d = np.zeros(m)
    for i in range(m):
        for t in range(ai[i], ai[i + 1]):
            if aj[t] == i:
                d[i] = aa[t]
                break
    return d


def strength(ai, aj, aa, theta, diag=None):
    """strong[t] = (j != i) and |a_t| > theta * sqrt(|d_i| * |d_j|), one byte per stored entry"""
    m = len(ai) - 1
    d = diagonal(ai, aj, aa) if diag is None else diag
    s = np.zeros(len(aj), dtype=np.uint8)
    for i in range(m):
        for t in range(ai[i], ai[i + 1]):
            j = int(aj[t])
            if j != i:
                bound = np.float64(theta) * np.sqrt(np.float64(abs(d[i])) * np.float64(abs(d[j])))
                s[t] = 1 if abs(np.float64(aa[t])) > bound else 0
    return s


def strength_np(ai, aj, aa, theta, diag):
    """the same mask with whole-array operations (the same IEEE operations in the same order per entry)"""
    ai, aj, aa, d = np.asarray(ai), np.asarray(aj), np.asarray(aa, dtype=np.float64), np.asarray(diag, dtype=np.float64)
    rows = np.repeat(np.arange(len(ai) - 1), np.diff(ai))
    with np.errstate(all="ignore"):
        return ((aj != rows) & (np.abs(aa) > np.float64(theta) * np.sqrt(np.abs(d[rows]) * np.abs(d[aj])))).astype(np.uint8)


def graph(ai, aj, strong):
    """the undirected graph: i ~ j when the stored entry (i, j) or (j, i) is strong"""
    m = len(ai) - 1
    nb = [set() for _ in range(m)]
    for i in range(m):
        for t in range(ai[i], ai[i + 1]):
            j = int(aj[t])
            if strong[t] and j != i:
                nb[i].add(j)
                nb[j].add(i)
    return nb


def greedy_mis2(ai, aj, strong):
    """-> (root flags, agg, nagg): nodes visited in decreasing key, a node is a root iff no root lies within distance 2"""
    m = len(ai) - 1
    nb = graph(ai, aj, strong)
    root = np.zeros(m, dtype=bool)
    for u in sorted(range(m), key=lambda i: -key(1, i)):
        near = set(nb[u])
        for v in nb[u]:
            near |= nb[v]
        if not any(root[v] for v in near if v != u):
            root[u] = True
    rank = np.cumsum(root) - 1
    first = [max([key(2, j) for j in nb[i] | {i} if root[j]], default=0) for i in range(m)]
    agg = np.zeros(m, dtype=np.int32)
    for i in range(m):
        c = first[i] or max([first[j] for j in nb[i]], default=0)
        assert c, "the set is not maximal at node %d" % i
        agg[i] = rank[c & M32]
    return root, agg, int(root.sum())


def aggregate(ai, aj, aa, theta):
    return greedy_mis2(ai, aj, strength(ai, aj, aa, theta))


# ---- sparse products in the library's order (spgemm.hip: entries of A's row in storage order, c = c + a * b from +0.0)
def spgemm(ai, aj, aa, bi, bj, ba):
    ci, cj, ca = [0], [], []
    for i in range(len(ai) - 1):
        acc = {}
        for t in range(ai[i], ai[i + 1]):
            r = int(aj[t])
            for q in range(bi[r], bi[r + 1]):
                c = int(bj[q])
                acc[c] = acc.get(c, 0.0) + float(aa[t]) * float(ba[q])
        for c in sorted(acc):
            cj.append(c)
            ca.append(acc[c])
        ci.append(len(cj))
    return np.array(ci, dtype=np.int32), np.array(cj, dtype=np.int32), np.array(ca, dtype=np.float64)


def transpose(ai, aj, aa, ncols):
    rows = [[] for _ in range(ncols)]
    for i in range(len(ai) - 1):
        for t in range(ai[i], ai[i + 1]):
            rows[int(aj[t])].append((i, float(aa[t])))
    ti, tj, ta = [0], [], []
    for r in rows:
        tj += [c for c, _ in r]
        ta += [v for _, v in r]
        ti.append(len(tj))
    return np.array(ti, dtype=np.int32), np.array(tj, dtype=np.int32), np.array(ta, dtype=np.float64)


def tentative(agg, nagg):
    cnt = np.bincount(agg, minlength=nagg)
    m = len(agg)
    return np.arange(m + 1, dtype=np.int32), np.array(agg, dtype=np.int32), np.array([1.0 / math.sqrt(float(cnt[a])) for a in agg])


def scaled_operator(ai, aj, aa):
    """S = D^-1 A as VecReciprocal and MatDiagonalScale give it, and rho = its largest row sum of |s| (entries in storage order)"""
    d = diagonal(ai, aj, aa)
    dinv = 1.0 / d
    sa = np.array([float(aa[t]) * float(dinv[i]) for i in range(len(ai) - 1) for t in range(ai[i], ai[i + 1])])
    rho = 0.0
    for i in range(len(ai) - 1):
        s = 0.0
        for t in range(ai[i], ai[i + 1]):
            s = s + abs(float(sa[t]))
        if i == 0 or s > rho:
            rho = s
    return sa, rho


def prolongator(ai, aj, aa, agg, nagg, nsmooths=1):
    """-> (P as CSR, rho): P = T - (4 / (3 rho)) S T through MatMatMult, MatScale, MatAXPY"""
    ti, tj, ta = tentative(agg, nagg)
    sa, rho = scaled_operator(ai, aj, aa)
    if not nsmooths:
        return (ti, tj, ta), rho
    pi, pj, pa = spgemm(ai, aj, sa, ti, tj, ta)
    alpha = -(4.0 / (3.0 * rho))
    pa = np.array([alpha * float(v) for v in pa])
    for i in range(len(ai) - 1):
        t = int(np.searchsorted(pj[pi[i]:pi[i + 1]], tj[i])) + pi[i]
        assert pj[t] == tj[i]
        pa[t] = float(pa[t]) + 1.0 * float(ta[i])
    return (pi, pj, pa), rho


def dense(csr, ncols):
    ai, aj, aa = csr
    M = np.zeros((len(ai) - 1, ncols))
    for i in range(len(ai) - 1):
        M[i, aj[ai[i]:ai[i + 1]]] = aa[ai[i]:ai[i + 1]]
    return M


class Hierarchy:
    """what PCGAMG's set-up builds from (ai, aj, aa): sizes, aggs, rhos fine level first; Ps / rho_mg / As_dense in PCMG's numbering
    (level 0 the coarsest, Ps[0] None)"""

    def __init__(self, ai, aj, aa, theta=0.0, coarse_eq_limit=50, nlevels=25, nsmooths=1):
        A = (np.asarray(ai, dtype=np.int32), np.asarray(aj, dtype=np.int32), np.asarray(aa, dtype=np.float64))
        self.sizes, self.aggs, self.coarsenings = [], [], 0
        Ps, rhos, As = [], [], [A]
        while True:
            n = len(A[0]) - 1
            self.sizes.append(n)
            d = diagonal(*A)
            assert np.all(d != 0.0)
            _, agg, nagg = aggregate(*A, theta)
            self.coarsenings += 1
            if n <= coarse_eq_limit or len(self.sizes) >= nlevels or nagg == n or nagg == 0:
                break
            self.aggs.append((agg, nagg))
            P, rho = prolongator(*A, agg, nagg, nsmooths)
            Pt = transpose(*P, nagg)
            A = spgemm(*Pt, *spgemm(*A, *P))
            Ps.append(P); rhos.append(rho); As.append(A)
        self.n = len(self.sizes)
        self.Ps = [None] + Ps[::-1]
        self.rho_mg = [None] + rhos[::-1]
        self.As_csr = As[::-1]
        self.As_dense = [dense(a, len(a[0]) - 1) for a in self.As_csr]
        self.Ps_dense = [None] + [dense(self.Ps[l], self.sizes[::-1][l - 1]) for l in range(1, self.n)]

    def cycle(self):
        """the dense V cycle: Chebyshev (2 steps, Jacobi, bounds (rho / 10, rho)) before and after, exact coarse solve"""
        return mr.MG(self.As_dense, self.Ps_dense, cheby_smoother(self.As_dense, self.rho_mg))


def cheby_smoother(As, rhos, steps=2):
    """KSPSolve_Chebychev with PCJACOBI from the guess x, `steps` iterations, no norm (cheby_ref.chebychev in dense form)"""
    def smooth(l, b, x):
        A, dinv = As[l], 1.0 / np.diag(As[l])
        emax, emin = rhos[l], rhos[l] / 10.0
        scale = 2.0 / (emax + emin)
        alpha = 1.0 - scale * emin
        mu, omegaprod = 1.0 / alpha, 2.0 / alpha
        c = [1.0, mu, 0.0]
        pkm1 = x
        pk = x + scale * (dinv * (b - A @ x))
        for _ in range(steps):
            c[2] = 2.0 * mu * c[1] - c[0]
            omega = omegaprod * c[1] / c[2]
            pkp1 = (omega * scale) * (dinv * (b - A @ pk)) + (1.0 - omega) * pkm1 + omega * pk
            pkm1, pk = pk, pkp1
            c[0], c[1] = c[1], c[2]
        return pk
    return smooth


# ---- the shapes the tests share
def path(n):
    return mr.to_csr(mr.laplace1d(n))


def poisson2d(n):
    ai, aj, aa = [0], [], []
    for i in range(n):
        for j in range(n):
            for di, dj, v in ((-1, 0, -1.0), (0, -1, -1.0), (0, 0, 4.0), (0, 1, -1.0), (1, 0, -1.0)):
                if 0 <= i + di < n and 0 <= j + dj < n:
                    aj.append((i + di) * n + j + dj); aa.append(v)
            ai.append(len(aj))
    return np.array(ai, dtype=np.int32), np.array(aj, dtype=np.int32), np.array(aa)


def poisson7(nx, ny, nz):
    ai, aj, aa = [0], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                for dk, dj, di, v in ((-1, 0, 0, -1.0), (0, -1, 0, -1.0), (0, 0, -1, -1.0), (0, 0, 0, 6.0), (0, 0, 1, -1.0), (0, 1, 0, -1.0), (1, 0, 0, -1.0)):
                    if 0 <= i + di < nx and 0 <= j + dj < ny and 0 <= k + dk < nz:
                        aj.append(((k + dk) * ny + j + dj) * nx + i + di); aa.append(v)
                ai.append(len(aj))
    return np.array(ai, dtype=np.int32), np.array(aj, dtype=np.int32), np.array(aa)


def with_empty_rows_and_isolated_nodes():
    """12 nodes: rows 2 and 7 store nothing, row 5 only its diagonal, row 9 a weak entry only (theta = 0.5), the rest a broken path"""
    rows = {0: {0: 2.0, 1: -1.0}, 1: {0: -1.0, 1: 2.0, 3: -1.0}, 3: {1: -1.0, 3: 2.0, 4: -1.0}, 4: {3: -1.0, 4: 2.0}, 5: {5: 1.0},
            6: {6: 2.0, 8: -1.0}, 8: {6: -1.0, 8: 2.0, 9: -0.01}, 9: {8: -0.01, 9: 2.0}, 10: {10: 2.0, 11: -1.5}, 11: {10: -1.5, 11: 2.0}}
    return from_rows(12, rows)


def from_rows(m, rows):
    ai, aj, aa = [0], [], []
    for i in range(m):
        for j in sorted(rows.get(i, {})):
            aj.append(j); aa.append(rows[i][j])
        ai.append(len(aj))
    return np.array(ai, dtype=np.int32), np.array(aj, dtype=np.int32), np.array(aa, dtype=np.float64)


def star(leaves=300):
    """a hub row with `leaves` off-diagonal entries; the leaves store only their diagonal, so the pattern is not symmetric"""
    rows = {0: dict([(0, float(leaves))] + [(j, -1.0) for j in range(1, leaves + 1)])}
    rows.update({j: {j: 1.0} for j in range(1, leaves + 1)})
    return from_rows(leaves + 1, rows)


def upwind(n):
    """2-D first-order upwind convection: row (i, j) couples to (i-1, j) and (i, j-1) only -- strong in one direction"""
    rows = {}
    for i in range(n):
        for j in range(n):
            r = {i * n + j: 2.0}
            if i:
                r[(i - 1) * n + j] = -1.0
            if j:
                r[i * n + j - 1] = -1.0
            rows[i * n + j] = r
    return from_rows(n * n, rows)


def anisotropic(n, eps=1e-3):
    """-u_xx - eps u_yy on an n x n grid, x the fast index: with theta = 0.1 only the x couplings are strong"""
    rows = {}
    for j in range(n):
        for i in range(n):
            r = {j * n + i: 2.0 + 2.0 * eps}
            if i:
                r[j * n + i - 1] = -1.0
            if i < n - 1:
                r[j * n + i + 1] = -1.0
            if j:
                r[(j - 1) * n + i] = -eps
            if j < n - 1:
                r[(j + 1) * n + i] = -eps
            rows[j * n + i] = r
    return from_rows(n * n, rows)


def random_graph(m, deg, seed, symmetric):
    rng = np.random.default_rng(seed)
    rows = {i: {i: 4.0} for i in range(m)}
    for i in range(m):
        for j in rng.integers(0, m, size=deg):
            j = int(j)
            if j != i:
                v = -float(rng.integers(1, 4))
                rows[i][j] = v
                if symmetric:
                    rows[j][i] = v
    return from_rows(m, rows)


def check_invariants(ai, aj, strong, root, agg, nagg):
    """independent of the model: a partition, roots pairwise further than 2 apart, every node within 2 of its root, numbers 0 .. nagg-1
    in root index order"""
    m = len(ai) - 1
    nb = graph(ai, aj, strong)
    roots = [i for i in range(m) if root[i]]
    assert len(roots) == nagg and len(agg) == m and (m == 0 or (agg.min() >= 0 and agg.max() < nagg))
    assert [int(agg[r]) for r in roots] == list(range(nagg))
    for r in roots:
        near = set(nb[r])
        for v in nb[r]:
            near |= nb[v]
        assert not any(root[v] for v in near if v != r), r
    for i in range(m):
        r = roots[agg[i]]
        assert i == r or r in nb[i] or any(r in nb[v] for v in nb[i]), i
