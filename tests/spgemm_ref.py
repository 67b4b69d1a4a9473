"""The arithmetic contract of the sparse matrix products, restated in numpy (what csrc/spgemm.hip and the host route of
MatMatMult / MatTranspose / MatPtAP are compared with, bit for bit).

C = A B, A m x k, B k x n, CSR with ascending columns in each row.
  symbolic: row i of C holds the union of the column lists of the rows B[aj[t], :], t over row i of A, ascending; structural --
            an entry is stored even where its value comes out zero.
  numeric:  every stored c_ij starts at +0.0; the stored entries t of A's row i are taken in storage order, and for each one every
            stored b = B[aj[t], j] gives c_ij = c_ij + (a_it * b): the product rounded, then the sum (multiply and add are separate
            ufuncs below: two roundings).  Nothing is skipped: a stored 0.0 in A times an Inf in B is a NaN.
A^T: explicit CSR whose rows list their entries in ascending original row (a stable counting sort).
P^T A P = matmult(transpose(P), matmult(A, P)), with exactly those bits."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def symbolic(ai, aj, bi, bj):
    m = ai.size - 1
    rows = []
    for i in range(m):
        cols = [bj[bi[r]:bi[r + 1]] for r in aj[ai[i]:ai[i + 1]]]
        rows.append(np.unique(np.concatenate(cols)) if cols else np.zeros(0, np.int32))
    ci = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int32)
    cj = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return ci, cj


def numeric(ai, aj, aa, bi, bj, ba, ci, cj, reverse=False):
    """reverse: the entries of A's row taken back to front -- NOT the contract; shows that a test can see the order"""
    ca = np.zeros(cj.size)
    with np.errstate(all="ignore"):
        for i in range(ai.size - 1):
            cols = cj[ci[i]:ci[i + 1]]
            acc = np.zeros(cols.size)
            steps = range(ai[i], ai[i + 1])
            for t in (reversed(steps) if reverse else steps):
                r = aj[t]
                pos = np.searchsorted(cols, bj[bi[r]:bi[r + 1]])
                acc[pos] = np.add(acc[pos], np.multiply(aa[t], ba[bi[r]:bi[r + 1]]))
            ca[ci[i]:ci[i + 1]] = acc
    return ca


def matmult(A, B, reverse=False):
    """A, B: (ai, aj, aa) triples; returns C's triple"""
    ci, cj = symbolic(A[0], A[1], B[0], B[1])
    return ci, cj, numeric(A[0], A[1], A[2], B[0], B[1], B[2], ci, cj, reverse)


def transpose(A, n):
    ai, aj, aa = A
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    o = np.argsort(aj, kind="stable")
    ti = np.concatenate(([0], np.cumsum(np.bincount(aj, minlength=n)))).astype(np.int32)
    return ti, rows[o].astype(np.int32), np.ascontiguousarray(aa[o])


def ptap(A, P, ncoarse):
    return matmult(transpose(P, ncoarse), matmult(A, P))


# ---------------------------------------------------------------------------------------------------- inputs
def random_csr(m, n, lens, seed, values=None):
    """m x n, row r with lens[r] distinct ascending columns; values N(0, 1) unless given as a function of (rng, nnz)"""
    rng = np.random.default_rng(seed)
    lens = np.minimum(np.asarray(lens, dtype=np.int64), n)
    ai = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    aj = np.concatenate([np.sort(rng.choice(n, size=int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    aa = rng.standard_normal(aj.size) if values is None else values(rng, aj.size)
    return ai, aj, np.ascontiguousarray(aa, dtype=np.float64)


def rect_pair(seed=5):
    """the random rectangular case: 37 x 53 times 53 x 41, 0 to 9 entries per row, with empty rows of A (3, 20), empty rows of B
    (7, 30, 52) and rows of A that name only empty B rows (11: columns 7 and 30; 25: column 52)"""
    rng = np.random.default_rng(seed)
    la = rng.integers(0, 10, 37); la[[3, 20]] = 0
    lb = rng.integers(0, 10, 53); lb[[7, 30, 52]] = 0
    A = list(random_csr(37, 53, la, seed + 1))
    B = random_csr(53, 41, lb, seed + 2)
    rows = [A[1][A[0][i]:A[0][i + 1]] for i in range(37)]
    vals = [A[2][A[0][i]:A[0][i + 1]] for i in range(37)]
    rows[11], vals[11] = np.array([7, 30], np.int32), np.array([1.5, -2.0])
    rows[25], vals[25] = np.array([52], np.int32), np.array([3.0])
    ai = np.concatenate(([0], np.cumsum([r.size for r in rows]))).astype(np.int32)
    return (ai, np.concatenate(rows).astype(np.int32), np.concatenate(vals)), B


def order_sensitive_pair():
    """one row of A with 1, 1e16, -1e16 against three B rows that share column 2 (values 1 there): forward (1 + 1e16) - 1e16 = 0,
    reversed (-1e16 + 1e16) + 1 = 1"""
    A = (np.array([0, 3, 5], np.int32), np.array([0, 1, 2, 0, 2], np.int32), np.array([1.0, 1e16, -1e16, 2.0, 0.5]))
    B = (np.array([0, 2, 4, 6], np.int32), np.array([0, 2, 1, 2, 2, 3], np.int32), np.array([2.0, 1.0, 5.0, 1.0, 1.0, -4.0]))
    return A, B


def aggregation_p(nx, ny, nz, weights=None):
    """piecewise-constant 2 x 2 x 2 aggregation of an nx x ny x nz grid (x fastest): P is (nx ny nz) x (nx ny nz / 8), one entry per row"""
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    idx = (x + nx * (y + ny * z)).ravel()
    agg = ((x // 2) + (nx // 2) * ((y // 2) + (ny // 2) * (z // 2))).ravel()
    o = np.argsort(idx)
    pj = agg[o].astype(np.int32)
    pa = np.ones(pj.size) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    return np.arange(pj.size + 1, dtype=np.int32), pj, pa
