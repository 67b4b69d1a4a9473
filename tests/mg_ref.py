"""A numpy model of PCMG: the three cycle kinds over callable level solvers, and the grid transfers the tests use.

Levels are numbered as in the harness: 0 is the coarsest, n - 1 the finest.  A[l] are dense level operators, P[l] (l >= 1) the dense
interpolation from level l - 1 to level l; restriction is P[l].T.  A level solver is a callable (l, b, x) -> x_new that may use x as
its initial guess; the coarse solver is called with x = 0.  The sequence is the one harness/mg.c runs ("PCMG")."""
import numpy as np


# ---------------------------------------------------------------------------------------------- transfers
def interp1d(nc):
    """(2 nc + 1) x nc linear interpolation, weights 1/2, 1, 1/2 (coarse point j sits at fine point 2 j + 1)"""
    P = np.zeros((2 * nc + 1, nc))
    for j in range(nc):
        P[2 * j, j] += 0.5; P[2 * j + 1, j] = 1.0; P[2 * j + 2, j] += 0.5
    return P


def interp2d(nc):
    P1 = interp1d(nc)
    return np.kron(P1, P1)


def interp3d(nc):
    P1 = interp1d(nc)
    return np.kron(P1, np.kron(P1, P1))


def aggregation(n, size):
    """piecewise-constant prolongation: fine unknown i belongs to aggregate i // size"""
    nc = (n + size - 1) // size
    P = np.zeros((n, nc))
    P[np.arange(n), np.arange(n) // size] = 1.0
    return P


def laplace1d(n):
    return 2.0 * np.eye(n) - np.eye(n, k=1) - np.eye(n, k=-1)


def laplace2d(n):
    T, I = laplace1d(n), np.eye(n)
    return np.kron(T, I) + np.kron(I, T)


def laplace3d(n):
    T, I = laplace1d(n), np.eye(n)
    return np.kron(np.kron(T, I), I) + np.kron(np.kron(I, T), I) + np.kron(np.kron(I, I), T)


def galerkin(A, Ps):
    """[A_0 .. A_{n-1}] from the finest operator and P[1 .. n-1] (Ps[0] is unused)"""
    As = [None] * len(Ps)
    As[-1] = A
    for l in range(len(Ps) - 1, 0, -1):
        As[l - 1] = Ps[l].T @ As[l] @ Ps[l]
    return As


def to_csr(M):
    M = np.asarray(M)
    ai, aj, aa = [0], [], []
    for r in M:
        c = np.flatnonzero(r)
        aj.extend(c); aa.extend(r[c]); ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64)


# ---------------------------------------------------------------------------------------------- level solvers
def jacobi_smoother(As, omega=2.0 / 3.0, steps=1):
    """damped Jacobi (Richardson with scale omega + PCJACOBI): x += omega D^-1 (b - A x), `steps` times"""
    def smooth(l, b, x):
        d = np.diag(As[l])
        for _ in range(steps):
            x = x + omega * (b - As[l] @ x) / d
        return x
    return smooth


def exact_coarse(As):
    def solve(l, b, x):
        return np.linalg.solve(As[l], b)
    return solve


class MG:
    def __init__(self, As, Ps, down, up=None, coarse=None, kind="multiplicative", cycle="v", cycles=1):
        self.A, self.P, self.n = As, Ps, len(As)
        self.down, self.up, self.coarse = down, up or down, coarse or exact_coarse(As)
        self.kind, self.cycle, self.cycles = kind, cycle, cycles

    def _cycle(self, l, b, x):
        if l == 0:
            return self.coarse(0, b[0], x)
        x = self.down(l, b[l], x)
        r = b[l] - self.A[l] @ x
        b[l - 1] = self.P[l].T @ r
        xc = np.zeros(self.A[l - 1].shape[0])
        for _ in range(1 if (l - 1 == 0 or self.cycle == "v") else 2):
            xc = self._cycle(l - 1, b, xc)
        x = x + self.P[l] @ xc
        return self.up(l, b[l], x)

    def apply(self, rhs):
        n = self.n
        b = [None] * n
        b[n - 1] = np.array(rhs, dtype=np.float64)
        if self.kind == "multiplicative":
            x = np.zeros_like(b[n - 1])
            for _ in range(self.cycles):
                x = self._cycle(n - 1, b, x)
            return x
        for l in range(n - 1, 0, -1):
            b[l - 1] = self.P[l].T @ b[l]
        if self.kind == "additive":
            xs = [self.coarse(0, b[0], np.zeros_like(b[0]))] + [self.down(l, b[l], np.zeros_like(b[l])) for l in range(1, n)]
            x = xs[0]
            for l in range(1, n):
                x = xs[l] + self.P[l] @ x
            return x
        assert self.kind == "full"
        x = self.coarse(0, b[0], np.zeros_like(b[0]))
        for l in range(1, n):
            x = self._cycle(l, b, self.P[l] @ x)
        return x

    def matrix(self):
        """B with apply(v) = B v (the level solvers are linear): column by column"""
        m = self.A[-1].shape[0]
        return np.column_stack([self.apply(e) for e in np.eye(m)])


def pcg(A, b, apply_pc, rtol=1e-8, max_it=1000):
    """preconditioned CG from x = 0 that tests the unpreconditioned residual norm (KSP_NORM_UNPRECONDITIONED), so the count means
    the same thing under every preconditioner; -> (x, iterations)"""
    x = np.zeros_like(b)
    r = b.copy()
    z = apply_pc(r)
    p = z.copy()
    rz = r @ z
    n0 = np.sqrt(r @ r)
    for it in range(1, max_it + 1):
        w = A @ p
        a = rz / (p @ w)
        x += a * p
        r -= a * w
        if np.sqrt(r @ r) <= rtol * n0:
            return x, it
        z = apply_pc(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it
