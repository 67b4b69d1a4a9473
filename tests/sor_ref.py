"""MatSOR restated in plain Python (MatSOR_SeqAIJ and MatInvertDiagonal_SeqAIJ, aij.c; MatSOR_MPIAIJ, mpiaij.c), written from the
contract and never from the code under test: the reference of tests/test_sor_cpu.py, test_sor_gpu.py and tools/sor_ranks.py.  Python
floats are IEEE doubles and every product, difference and sum below is one operation, so the order and the roundings are the contract's.
Also here: the matrices of those tests and the brute-force form of the level rule."""
import numpy as np

import orc

FORWARD, BACKWARD, SYMMETRIC = 1, 2, 3
LOCAL_FORWARD, LOCAL_BACKWARD, LOCAL_SYMMETRIC = 4, 8, 12
ZERO_INITIAL_GUESS, EISENSTAT, APPLY_UPPER, APPLY_LOWER = 16, 32, 64, 128
SWEEPS = {"forward": FORWARD, "backward": BACKWARD, "symmetric": SYMMETRIC,
          "local_forward": LOCAL_FORWARD, "local_backward": LOCAL_BACKWARD, "local_symmetric": LOCAL_SYMMETRIC}
ITS = [(1, 1), (2, 1), (1, 2)]
OMEGA_SHIFT = [(1.0, 0.0), (1.3, 0.0), (1.0, 0.25)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def inverted_diagonal(ai, aj, aa, omega, fshift):
    """mdiag, idiag; ValueError("missing", row) / ("zero", row) for what MatInvertDiagonal_SeqAIJ refuses"""
    m = len(ai) - 1
    mdiag = np.empty(m)
    for i in range(m):
        hit = [k for k in range(ai[i], ai[i + 1]) if aj[k] == i]
        if not hit:
            raise ValueError("missing", i)
        mdiag[i] = aa[hit[0]]
    plain = (omega == 1 and fshift == 0)
    if plain and np.any(mdiag == 0):
        raise ValueError("zero", int(np.flatnonzero(mdiag == 0)[0]))
    with np.errstate(all="ignore"):
        idiag = (np.float64(1.0) / mdiag) if plain else (np.float64(omega) / (np.float64(fshift) + mdiag))
    return mdiag, idiag


def sor_ref(ai, aj, aa, b, x0, omega=1.0, flag=LOCAL_SYMMETRIC, fshift=0.0, its=1, lits=1):
    """x after MatSOR(A, b, omega, flag, fshift, its, lits, x0); x0's content is not read under ZERO_INITIAL_GUESS"""
    m = len(ai) - 1
    ai = [int(v) for v in ai]; aj = [int(v) for v in aj]; aa = [float(v) for v in aa]
    mdiag, idiag = inverted_diagonal(ai, aj, aa, omega, fshift)
    mdiag = [float(v) for v in mdiag]; idiag = [float(v) for v in idiag]
    b = [float(v) for v in b]; x = [float(v) for v in x0]
    omega = float(omega)
    fwd, bwd = bool(flag & (FORWARD | LOCAL_FORWARD)), bool(flag & (BACKWARD | LOCAL_BACKWARD))
    its = its * lits

    def general(i):
        s = b[i]
        for k in range(ai[i], ai[i + 1]):
            s = s - aa[k] * x[aj[k]]
        x[i] = (1. - omega) * x[i] + (s + mdiag[i] * x[i]) * idiag[i]

    if flag & ZERO_INITIAL_GUESS:
        xb, t = b, [0.0] * m
        if fwd:
            for i in range(m):
                s = b[i]
                for k in range(ai[i], ai[i + 1]):
                    if aj[k] < i:
                        s = s - aa[k] * x[aj[k]]
                t[i] = s
                x[i] = s * idiag[i]
            xb = t
        if bwd:
            for i in range(m - 1, -1, -1):
                s = xb[i]
                for k in range(ai[i], ai[i + 1]):
                    if aj[k] > i:
                        s = s - aa[k] * x[aj[k]]
                x[i] = s * idiag[i] if xb is b else (1. - omega) * x[i] + s * idiag[i]
        its -= 1
    for _ in range(its):
        if fwd:
            for i in range(m):
                general(i)
        if bwd:
            for i in range(m - 1, -1, -1):
                general(i)
    return np.array(x, dtype=np.float64)


def sor_mpi_ref(parts, b, x0, omega, flag, fshift, its, lits):
    """MatSOR_MPIAIJ over the ranks' pieces (orc.mpiaij_split dicts; b, x0: lists of the ranks' local parts); returns the ranks' x.
    A flag without a local sweep, or with a non-local one, is refused as in the contract (ValueError)"""
    if flag & (SYMMETRIC | EISENSTAT | APPLY_UPPER | APPLY_LOWER) or not flag & LOCAL_SYMMETRIC:
        raise ValueError("not supported")
    twin = SYMMETRIC if (flag & LOCAL_SYMMETRIC) == LOCAL_SYMMETRIC else (FORWARD if flag & LOCAL_FORWARD else BACKWARD)
    x = [np.array(v, dtype=np.float64) for v in x0]
    if flag & ZERO_INITIAL_GUESS:
        x = [sor_ref(p["ad_i"], p["ad_j"], p["ad_a"], b[r], x[r], omega, flag, fshift, lits, 1) for r, p in enumerate(parts)]
        its -= 1
    for _ in range(its):
        xg = np.concatenate(x)
        new = []
        for r, p in enumerate(parts):
            lvec = -1.0 * xg[p["garray"]]
            bb1 = orc.spmv_add(p["bo_i"], p["bo_j"], p["bo_a"], lvec, np.array(b[r], dtype=np.float64))
            new.append(sor_ref(p["ad_i"], p["ad_j"], p["ad_a"], bb1, x[r], omega, twin, fshift, lits, 1))
        x = new
    return x


# ---------------------------------------------------------------------------------------------------- levels
def levels_ref(ai, aj):
    """lev[i] = 0, or 1 + max lev[j] over the j < i with a(i,j) or a(j,i) stored"""
    m = len(ai) - 1
    lower = [set() for _ in range(m)]
    for i in range(m):
        for k in range(ai[i], ai[i + 1]):
            j = int(aj[k])
            if j < i:
                lower[i].add(j)
            elif j > i:
                lower[j].add(i)
    lev = np.zeros(m, dtype=np.int32)
    for i in range(m):
        lev[i] = 1 + max(lev[j] for j in lower[i]) if lower[i] else 0
    return lev


def levels_respect_every_dependency(ai, aj, lev):
    """every stored a(i,j), i != j: the smaller index sits in a strictly lower level (dependencies of the forward sweep,
    anti-dependencies of the general sweeps, and both again for the backward direction)"""
    for i in range(len(ai) - 1):
        for k in range(ai[i], ai[i + 1]):
            j = int(aj[k])
            if j != i and not lev[min(i, j)] < lev[max(i, j)]:
                return False
    return True


# ---------------------------------------------------------------------------------------------------- matrices
def perturbed(csr):
    ai, aj, aa = csr
    return ai.astype(np.int32), aj.astype(np.int32), aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))


def from_rows(rows):
    """rows: list of {col: value}; columns stored ascending"""
    ai, aj, aa = [0], [], []
    for r in rows:
        for c in sorted(r):
            aj.append(c); aa.append(r[c])
        ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64)


def nonsym200(n=200, dominant=False):
    """a full diagonal, at most 9 entries per row, many a(i,j) stored without a(j,i)"""
    rng = np.random.RandomState(20)
    rows = []
    for i in range(n):
        cols = set(int(c) for c in rng.randint(0, n, size=rng.randint(0, 9)))
        cols.discard(i)
        r = {c: float(rng.uniform(-1.0, 1.0)) for c in cols}
        r[i] = (sum(abs(v) for v in r.values()) + 1.0 + rng.uniform(0, 1)) if dominant else float(rng.uniform(1.5, 3.0))
        rows.append(r)
    ai, aj, aa = from_rows(rows)
    stored = set(zip(np.repeat(np.arange(n), np.diff(ai)).tolist(), aj.tolist()))
    assert any((j, i) not in stored for (i, j) in stored), "the pattern is meant to be non-symmetric"
    assert np.diff(ai).max() <= 9
    return ai, aj, aa


def tridiag(n=300):
    return from_rows([{c: (2.5 + 0.1 * np.sin(i)) if c == i else -1.0 + 0.05 * np.cos(i + c) for c in (i - 1, i, i + 1) if 0 <= c < n} for i in range(n)])


def one_row():
    return from_rows([{0: 1.75}])


def wide_then_chain(nd=600, nc=100):
    """rows 0 .. nd-1 diagonal only (one level of more than 256 rows), rows nd .. nd+nc-1 couple to them and to each other in a chain
    (one-row levels): a sweep crosses the block boundary, the switch from one launch per level to a fused run, and back"""
    rows = [{i: 2.0 + 0.01 * i} for i in range(nd)]
    for q in range(nc):
        i = nd + q
        r = {i: 3.0 + 0.02 * q, (7 * q) % nd: -0.5, (13 * q + 5) % nd: 0.25}
        if q:
            r[i - 1] = -0.75
        if q + 1 < nc:
            r[i + 1] = 0.4
        rows.append(r)
    return from_rows(rows)


LAYERS = (70, 130, 256, 257, 256, 200, 65)


def layered(sizes=LAYERS):
    """rows in layers, layer L exactly level L: every row reads two or three rows of the layer below (at positions spread over the
    whole layer, so a level's lanes read what other wavefronts wrote) and, without the transposed entry being stored, one or two rows
    of the layer above.  Consecutive coupled levels of 65 .. 256 rows, and a level of exactly 256 next to one of 257: the fused runs
    end at the block size and start again behind it"""
    start = np.concatenate([[0], np.cumsum(sizes)])
    rows = []
    for L, n in enumerate(sizes):
        for q in range(n):
            i = int(start[L]) + q
            r = {i: 4.0 + 0.01 * ((7 * i) % 13)}
            if L > 0:
                nb = sizes[L - 1]
                for s_, v in ((37 * q + 5, -0.5), (101 * q + 64, 0.3), (q + 129, -0.2 if q % 3 else None)):
                    if v is not None:
                        r[int(start[L - 1]) + s_ % nb] = v + 0.001 * (q % 7)
            if L + 1 < len(sizes):
                na = sizes[L + 1]
                r[int(start[L + 1]) + (53 * q + 11) % na] = 0.25 - 0.002 * (q % 5)
                if q % 2:
                    r[int(start[L + 1]) + (17 * q + 200) % na] = -0.15
            rows.append(r)
    return from_rows(rows)


def p7_small():
    return perturbed(orc.gen_p7(5, 4, 3))


MATRICES = {"p7_5x4x3": p7_small, "nonsym200": nonsym200, "tridiag300": tridiag, "one_row": one_row}


def rhs(n):
    return np.cos(0.37 * np.arange(n)) + 0.25, np.sin(0.61 * np.arange(n)) - 0.1     # b, a nonzero x0


def short_grid():
    """every sweep, zero guess on and off, one and two sweeps, two (omega, shift) pairs: for the larger matrices"""
    for name in SWEEPS:
        for zero in (True, False):
            for its, lits in ((1, 1), (2, 1)):
                for omega, fshift in ((1.0, 0.0), (1.3, 0.25)):
                    yield name, zero, its, lits, omega, fshift


def python_pcg(ai, aj, aa, b, rtol, precondition, abstol=1e-50, max_it=10000):
    """KSPSolve_CG of the reference (cg.c, preconditioned norm, zero guess, KSPDefaultConverged) with z = precondition(res); the
    products, updates and reductions are the oracle's, so inside orc.device_reduction_order() the sums take the device's order.
    Returns x, the residual history, the iteration count and the reason"""
    n = b.size
    x, res = np.zeros(n), b.copy()
    z = precondition(res)
    rn = float(orc.vec_norm(z, 1))
    hist, ttol = [rn], max(rtol * rn, abstol)

    def reason_of(rn):
        return 3 if rn < abstol else (2 if rn <= ttol else 0)

    reason, k, its = reason_of(rn), 0, 0
    if reason:
        return x, np.array(hist), 0, reason
    rz, rz_last, d = float(orc.vec_dot(z, res)), 1.0, None
    while True:
        its = k + 1
        if k == 0:
            d = z.copy()
        else:
            orc.vec_aypx(d, rz / rz_last, z)
        ad = orc.matmult(ai, aj, aa, d)[0]
        pap = float(orc.vec_dot(d, ad))
        rz_last = rz
        step = rz / pap
        orc.vec_axpy(x, step, d)
        orc.vec_axpy(res, -step, ad)
        z = precondition(res)
        rn = float(orc.vec_norm(z, 1))
        hist.append(rn)
        reason = reason_of(rn)
        if reason:
            break
        rz = float(orc.vec_dot(z, res))
        k += 1
        if k >= max_it:
            reason = -3
            break
    return x, np.array(hist), its, reason


def grid():
    """(sweep name, zero guess, its, lits, omega, fshift) of the contract's grid"""
    for name in SWEEPS:
        for zero in (True, False):
            for its, lits in ITS:
                for omega, fshift in OMEGA_SHIFT:
                    yield name, zero, its, lits, omega, fshift
