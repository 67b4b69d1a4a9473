"""Random call programs against a host model, for the layer that decides WHEN a Vec / Mat kernel runs and on which copy of the data
(the note queue, the kept dot, the operand ring, the noted and the unwritten product, the split-reduction slots, the per-vector
validity flags of host/vechip.c, and what host/aijhip.c ties into them).

A program is a list of calls -- tuples (kind, arguments...) -- over a small pool: vectors 0..7 of length n, borrowers 8 and 9 of
length m (they only act while they borrow a pool vector's storage), matrices "A" and "B" of one pattern.  generate(index) builds the
program of one entry of TABLE: a motif (the call sequence one of the shortcuts recognises), whole or cut at one position by calls
of one class, with random calls around it.  Model replays a program on plain NumPy arrays, eagerly, with the oracle's loops and the
restatements the suite already has; execute() replays it on the library through the public wrappers.  Importing needs no GPU."""
import copy
import ctypes as C

import numpy as np

import orc
import problems as pb
import sor_ref
from test_mat_value_ops_cpu import bits                                   # noqa: F401  (the tests take it from here)
from test_mat_zero_rows_cpu import ref_zero_rows, ref_zero_rows_columns

NV, BORROWERS = 8, (8, 9)
MAXCALLS = 40
INSERT, ADD = 1, 2
SCALARS = (0.0, -0.0, 1.0, -1.0, 0.37, -0.7, 1.25, 0.5, -1.7, 2.0)
MSCALARS = (0.5, -0.75, 1.25, 2.0)                                        # matrix scalings and shifts: the diagonal stays away from zero
TAME = 1e8

CLASS = {}
for _cls, _kinds in (("elementwise", "set copy swap scale axpy aypx axpby waxpy axpbypcz maxpy pmult pdiv recip"),
                     ("reduction", "dot tdot mdot dotnorm2 norm normalize"),
                     ("split", "dotbegin normbegin srbegin dotend normend"),
                     ("storage", "getarray restorearray getarrayread setvalues placearray resetarray replacearray sharebegin shareend"),
                     ("destroy", "recreate"),
                     ("product", "matmult matmultadd matmulttranspose"),
                     ("matvalue", "matscale matdiagscale matshift matzeroentries mataxpy matcopy matzerorows matzerorowscols matsor")):
    for _k in _kinds.split():
        CLASS[_k] = _cls
KINDS = sorted(CLASS)
CUT_CLASSES = ("elementwise", "reduction", "storage", "matvalue", "destroy", "split")
# what an interrupting call of a class may be: rotated through, so that every kind meets a pending note
CUT_KINDS = {"elementwise": "set copy swap scale axpy aypx axpby waxpy axpbypcz maxpy pmult pdiv recip".split(),
             "reduction": "dot tdot mdot dotnorm2 norm0 norm1 norm3 norm4 normalize".split(),
             "storage": "getrestore restorearray getarrayread setvalues_insert setvalues_add placearray resetarray replacearray share0 share1 shareend".split(),
             "matvalue": "matscale matdiagscale matshift matzeroentries mataxpy matcopy matzerorows matzerorows_b matzerorowscols matzerorowscols_b matsor".split(),
             "destroy": ["recreate"], "split": ["split"]}


# ---------------------------------------------------------------------------------------------------- pool
def matrix(shape):
    if shape == "lap2d":
        ai, aj, aa = pb.lap2d(23, 19)
        aa = aa * (1.0 + 0.2 * np.sin(np.arange(aa.size)))
    elif shape == "nonsym300":
        ai, aj, aa = sor_ref.nonsym200(300, dominant=True)
    else:
        ai, aj, aa = np.array([0, 1]), np.array([0]), np.array([2.5])
    return np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(aa, np.float64)


_POOLS = {}


def pool(shape, seed):
    """the matrix of a shape (built once) and this seed's vectors: entries of magnitude 0.5 .. 1.5, either sign"""
    if shape not in _POOLS:
        ai, aj, aa = matrix(shape)
        _POOLS[shape] = (ai, aj, aa, aa * (0.6 + 0.3 * np.cos(np.arange(aa.size))))
    ai, aj, aa, bb = _POOLS[shape]
    n = ai.size - 1
    m = max(1, n // 3)
    rng = np.random.default_rng([seed, 7])
    vecs = [rng.uniform(0.5, 1.5, k) * rng.choice([-1.0, 1.0], k) for k in [n] * NV + [m] * len(BORROWERS)]
    return dict(shape=shape, n=n, m=m, ai=ai, aj=aj, aa=aa, bb=bb, vecs=vecs)


def buffer(bufid, n):
    """the content of the host array a program places or hands over: 0.25 .. 1.25"""
    return 0.75 + 0.5 * np.cos(0.9 * np.arange(n) + bufid)


def operands(c):
    """(vectors read, vectors written) of a call"""
    k = c[0]
    if k in ("set", "recreate", "placearray", "replacearray", "resetarray"): return ((c[2],) if k == "recreate" else ()), (c[1],)
    if k == "copy": return (c[1],), (c[2],)
    if k == "swap": return (c[1], c[2]), (c[1], c[2])
    if k in ("scale", "recip", "normalize", "restorearray", "setvalues", "getarray"): return (c[1],), (c[1],)
    if k in ("axpy", "aypx"): return (c[1], c[3]), (c[1],)
    if k == "axpby": return (c[1], c[4]), (c[1],)
    if k == "waxpy": return (c[3], c[4]), (c[1],)
    if k == "axpbypcz": return (c[1], c[5], c[6]), (c[1],)
    if k == "maxpy": return (c[1],) + tuple(c[3]), (c[1],)
    if k in ("pmult", "pdiv"): return (c[2], c[3]), (c[1],)
    if k in ("dot", "tdot", "dotnorm2", "dotbegin"): return (c[1], c[2]), ()
    if k == "mdot": return (c[1],) + tuple(c[2]), ()
    if k in ("norm", "normbegin", "getarrayread"): return (c[1],), ()
    if k == "sharebegin": return (c[2],), ((c[1], c[2]) if c[4] else (c[1],))
    if k == "shareend": return (), (c[1],)
    if k in ("matmult", "matmulttranspose"): return (c[2],), (c[3],)
    if k == "matmultadd": return (c[2], c[3]), (c[4],)
    if k == "matdiagscale": return tuple(v for v in c[2:4] if v is not None), ()
    if k in ("matzerorows", "matzerorowscols"): return ((c[4],) if c[4] is not None else ()), ((c[5],) if c[5] is not None else ())
    if k == "matsor": return (c[2], c[3]), (c[3],)
    return (), ()


REDUCING_KINDS = ("dot", "tdot", "mdot", "dotnorm2", "norm", "normalize", "dotend", "normend", "getarrayread")


def show(calls):
    """a program as readable calls, one per line"""
    def arg(a):
        if isinstance(a, tuple) and len(a) > 8:
            return "(%s, ... %d)" % (", ".join(repr(v) for v in a[:3]), len(a))
        return repr(a)
    return "\n".join("%3d  %s(%s)" % (i, c[0], ", ".join(arg(a) for a in c[1:])) for i, c in enumerate(calls))


# ---------------------------------------------------------------------------------------------------- model
class Model:
    """The pool as NumPy arrays, updated call by call.  Reductions come from the oracle, so replay under
    orc.device_reduction_order() for the device's bits.  Besides the values it keeps what the public wrappers keep: the norms a
    vector's object state still vouches for (VecNorm answers from them; VecSet, VecCopy and VecScale carry them along)."""

    def __init__(self, pl):
        self.ai, self.aj, self.n, self.m = pl["ai"], pl["aj"], pl["n"], pl["m"]
        self.M = {"A": pl["aa"].copy(), "B": pl["bb"].copy()}
        self.V = [v.copy() for v in pl["vecs"]]
        self.norms = [dict() for _ in self.V]
        self.lent, self.placed, self.open, self.sr, self.out = {}, {}, set(), [], []
        self.tol = []                                      # per scalar: None (the oracle's bits are asked) or (reference, bound), see loose()
        self.diag = np.flatnonzero(np.repeat(np.arange(self.n), np.diff(self.ai)) == self.aj)
        self.cached = False                                # the last VecNorm was answered by the wrapper alone
        self.srtol = []
        self.world = 1                                     # > 1: MatMult as an MPIAIJ matrix split by rows over that many ranks forms it

    def vec(self, v):
        if v in self.lent:
            p, off, _ = self.lent[v]
            return self.V[p][off:off + self.m]
        return self.V[v]

    def loose(self, *vs):
        """a reduction over a borrower that starts at an odd entry of its parent: the kernels sum from a pointer that is not 16-byte
        aligned in another order than the oracle's tree knows, so such a scalar is held to the worst case of ANY order instead"""
        return any(v in self.lent and self.lent[v][1] % 2 for v in vs)

    @staticmethod
    def bound(kind, x, y=None):
        """(reference in np.longdouble, worst-case distance of any float64 evaluation from it), formed as bsr_reference of
        tests/test_kernels_gpu.py forms its bound: gamma_n S + n 2^-63 S with S the sum of the terms' magnitudes, gamma_n = n u / (1 - n u),
        u = 2^-53; the root of a sum of squares moves by at most gamma_n relative (|sqrt(1 + e) - 1| <= |e|) and rounds once more"""
        ld, u, n = np.longdouble, 2.0 ** -53, x.size
        g = n * u / (1 - n * u)
        if kind == "dot":
            t = x.astype(ld) * y.astype(ld)
            return t.sum(), (g + n * 2.0 ** -63) * np.abs(t).sum()
        if kind == "norm1":
            S = np.abs(x.astype(ld)).sum()
            return S, (g + n * 2.0 ** -63) * S
        rt = np.sqrt((x.astype(ld) ** 2).sum())
        return rt, rt * (g + u * (1 + g) + n * 2.0 ** -63)

    def wrote(self, *vs):
        for v in vs:
            self.norms[v] = {}

    def _norm(self, v, t):
        self.cached = t != 4 and t in self.norms[v]
        if self.cached:
            return self.norms[v][t]
        val = orc.vec_norm(self.vec(v), t)
        if t != 4:
            self.norms[v][t] = val
        return val

    def _scale(self, v, a):
        if a == 1.0:
            return
        old = self.norms[v]
        orc.vec_scale(self.vec(v), a)
        self.norms[v] = {t: abs(a) * val for t, val in old.items()}

    def tame(self):
        return all(np.all(np.isfinite(a)) and (a.size == 0 or np.max(np.abs(a)) < TAME) for a in self.V + list(self.M.values()))

    def apply(self, c):
        self.cached = False
        self._apply(c)
        k, X, B, have = c[0], self.vec, self.bound, len(self.tol)
        if k in ("dot", "tdot") and self.loose(c[1], c[2]): self.tol.append(B("dot", X(c[1]), X(c[2])))
        elif k == "mdot" and self.loose(c[1], *c[2]): self.tol.extend(B("dot", X(c[1]), X(v)) for v in c[2])
        elif k == "dotnorm2" and self.loose(c[1], c[2]): self.tol.extend([B("dot", X(c[1]), X(c[2])), B("dot", X(c[2]), X(c[2]))])
        elif k == "norm" and self.loose(c[1]) and c[2] != 3:
            self.tol.extend({0: [B("norm1", X(c[1]))], 1: [B("norm2", X(c[1]))], 4: [B("norm1", X(c[1])), B("norm2", X(c[1]))]}[c[2]])
        elif k == "dotbegin": self.srtol.append(B("dot", X(c[1]), X(c[2])) if self.loose(c[1], c[2]) else None)
        elif k == "normbegin": self.srtol.append(B("norm2", X(c[1])) if self.loose(c[1]) else None)
        elif k in ("dotend", "normend"): self.tol.append(self.srtol.pop(0))
        self.tol.extend([None] * (len(self.out) - len(self.tol)))
        assert len(self.tol) == len(self.out) and (have == len(self.tol) or k in REDUCING_KINDS), c

    def _apply(self, c):
        k, X, o = c[0], self.vec, orc
        ai, aj = self.ai, self.aj
        if k == "set":
            o.vec_set(X(c[1]), c[2])
            a, N = abs(c[2]), float(X(c[1]).size)
            self.norms[c[1]] = {0: N * a, 3: a, 1: np.sqrt(N) * a}
        elif k == "copy":
            o.vec_copy(X(c[1]), X(c[2])); self.norms[c[2]] = dict(self.norms[c[1]])
        elif k == "swap":
            o.vec_swap(X(c[1]), X(c[2])); self.wrote(c[1], c[2])
        elif k == "scale":
            self._scale(c[1], c[2])
        elif k == "axpy":
            o.vec_axpy(X(c[1]), c[2], X(c[3])); self.wrote(c[1])
        elif k == "aypx":
            o.vec_aypx(X(c[1]), c[2], X(c[3])); self.wrote(c[1])
        elif k == "axpby":
            o.vec_axpby(X(c[1]), c[2], c[3], X(c[4])); self.wrote(c[1])
        elif k == "waxpy":
            o.vec_waxpy(X(c[1]), c[2], X(c[3]), X(c[4])); self.wrote(c[1])
        elif k == "axpbypcz":
            o.vec_axpbypcz(X(c[1]), c[2], c[3], c[4], X(c[5]), X(c[6])); self.wrote(c[1])
        elif k == "maxpy":
            o.vec_maxpy(X(c[1]), np.array(c[2]), [X(v) for v in c[3]]); self.wrote(c[1])
        elif k == "pmult":
            o.vec_pointwise_mult(X(c[1]), X(c[2]), X(c[3])); self.wrote(c[1])
        elif k == "pdiv":
            o.vec_pointwise_divide(X(c[1]), X(c[2]), X(c[3])); self.wrote(c[1])
        elif k == "recip":
            o.vec_reciprocal(X(c[1])); self.wrote(c[1])
        elif k in ("dot", "tdot"):
            self.out.append(o.vec_dot(X(c[1]), X(c[2])))
        elif k == "mdot":
            self.out.extend(o.vec_mdot(X(c[1]), [X(v) for v in c[2]]))
        elif k == "dotnorm2":
            self.out.extend(o.vec_dotnorm2(X(c[1]), X(c[2])))
        elif k == "norm":
            val = self._norm(c[1], c[2])
            self.out.extend(val if c[2] == 4 else [val])
        elif k == "normalize":
            val = self._norm(c[1], 1)
            self.out.append(val)
            if val != 0.0 and val != 1.0:
                self._scale(c[1], 1.0 / val)
        elif k == "dotbegin":
            self.sr.append(o.vec_dot(X(c[1]), X(c[2])))
        elif k == "normbegin":
            self.sr.append(o.vec_norm(X(c[1]), 1))
        elif k in ("dotend", "normend"):
            self.out.append(self.sr.pop(0))
        elif k == "getarray":
            self.open.add(c[1])
        elif k == "restorearray":
            a = X(c[1]); a[c[2] % 3::3] = a[c[2] % 3::3] * 0.5 + 0.125 * c[2]
            self.open.discard(c[1]); self.wrote(c[1])
        elif k == "getarrayread":
            a = X(c[1]); self.out.extend([a[0], a[-1]])
        elif k == "setvalues":
            a, idx, vals = X(c[1]), np.array(c[2], dtype=np.int64), np.array(c[3])
            if c[4] == INSERT: a[idx] = vals
            else: a[idx] = a[idx] + vals
            self.wrote(c[1])
        elif k == "placearray":
            self.placed[c[1]] = X(c[1]).copy(); X(c[1])[:] = buffer(c[2], self.n); self.wrote(c[1])
        elif k == "resetarray":
            X(c[1])[:] = self.placed.pop(c[1]); self.wrote(c[1])
        elif k == "replacearray":
            X(c[1])[:] = buffer(c[2], self.n); self.wrote(c[1])
        elif k == "sharebegin":
            self.lent[c[1]] = (c[2], c[3], c[4]); self.wrote(c[1])
        elif k == "shareend":
            p, _, write = self.lent.pop(c[1])
            self.wrote(c[1])
            if write:
                self.wrote(p)                              # the parent's values changed through the borrower
        elif k == "recreate":
            X(c[1])[:] = 0.0; self.wrote(c[1])
        elif k == "matmult" and self.world > 1:
            # MatMult_MPIAIJ: per rank the diagonal block's product, then the off-diagonal block's added to it.  Each as the reference
            # dispatches it (orc.matmult): the off-diagonal block's runs of empty rows form nodes, and its inode routine sums a row
            # with two entries in another order than the plain loop
            x, y, n = X(c[2]).copy(), X(c[3]), self.n
            for r in range(self.world):
                lo, hi = (n * r) // self.world, (n * (r + 1)) // self.world
                q = o.mpiaij_split(lo, hi, lo, hi, ai, aj, self.M[c[1]])
                d = o.matmult(q["ad_i"], q["ad_j"], q["ad_a"], np.ascontiguousarray(x[lo:hi]))[0]
                y[lo:hi] = o.matmult(q["bo_i"], q["bo_j"], q["bo_a"], np.ascontiguousarray(x[q["garray"]]), d)[0]
            self.wrote(c[3])
        elif k == "matmult":
            X(c[3])[:] = o.spmv(ai, aj, self.M[c[1]], X(c[2])); self.wrote(c[3])
        elif k == "matmultadd":
            X(c[4])[:] = o.spmv_add(ai, aj, self.M[c[1]], X(c[2]), X(c[3])); self.wrote(c[4])
        elif k == "matmulttranspose":
            X(c[3])[:] = o.spmv_t(ai, aj, self.M[c[1]], X(c[2]), self.n); self.wrote(c[3])
        # the matrix value operations as tests/test_mat_value_ops_cpu.py, test_sor_gpu.py and test_mat_zero_rows_cpu.py state them
        elif k == "matscale":
            if c[2] != 1.0: self.M[c[1]] = c[2] * self.M[c[1]]
        elif k == "matdiagscale":
            self.M[c[1]] = o.diagonal_scale(ai, aj, self.M[c[1]], None if c[2] is None else X(c[2]).copy(), None if c[3] is None else X(c[3]).copy())
        elif k == "matshift":
            cur = self.M[c[1]].copy(); cur[self.diag] += c[2]; self.M[c[1]] = cur
        elif k == "matzeroentries":
            self.M[c[1]] = np.zeros_like(self.M[c[1]])
        elif k == "mataxpy":
            self.M[c[1]] = self.M[c[1]] + c[2] * self.M[c[3]]
        elif k == "matcopy":
            self.M[c[2]] = self.M[c[1]].copy()
        elif k in ("matzerorows", "matzerorowscols"):
            ref = ref_zero_rows if k == "matzerorows" else ref_zero_rows_columns
            x = None if c[4] is None else X(c[4]).copy()
            b = None if c[5] is None else X(c[5]).copy()
            self.M[c[1]], bnew = ref(ai, aj, self.M[c[1]], list(c[2]), c[3], x, b)
            if b is not None:
                X(c[5])[:] = bnew; self.wrote(c[5])
        elif k == "matsor":
            X(c[3])[:] = sor_ref.sor_ref(ai, aj, self.M[c[1]], X(c[2]), X(c[3]), flag=sor_ref.SYMMETRIC); self.wrote(c[3])
        elif k != "srbegin":
            raise ValueError(k)


class Pending:
    """The model's own bookkeeping of what the vector type would be holding back after each call: `dq` the noted element-wise
    operations, `pp` a noted product (M, x, t), `pl` a product whose work vector is still unwritten.  It follows the documented
    patterns, not the code: enough to say whether a call met something pending."""

    def __init__(self):
        self.dq, self.pp, self.pl = [], None, None

    def any(self):
        return bool(self.dq or self.pp or self.pl)

    def flush(self):
        self.dq, self.pp = [], None

    def step(self, c, cached=False):
        k, dq = c[0], self.dq
        rd, wr = operands(c)
        if self.pl and k not in ("matmult",) and (self.pl[2] in rd + wr or self.pl[1] in wr or k in ("sharebegin", "shareend")):
            self.pl = None
        if CLASS[k] == "matvalue":
            M = c[2] if k == "matcopy" else c[1]
            if self.pp and self.pp[0] == M: self.pp = None
            if self.pl and self.pl[0] == M: self.pl = None
            if rd or wr: self.flush()
            return
        if k in ("srbegin", "dotend", "normend", "restorearray") or (k == "axpy" and c[2] == 0.0) or (k == "scale" and c[2] == 1.0) or (k == "norm" and cached):
            return
        if k == "axpy":
            if len(dq) == 1 and dq[0][0] == "axpy" and c[2] == -dq[0][2] and c[1] not in (dq[0][1], dq[0][3]) and c[3] != dq[0][1]:
                dq.append(c); return
            self.flush(); self.dq = [c]; return
        if k == "axpbypcz" and c[4] == 1.0:
            self.flush(); self.dq = [c]; return
        if k == "waxpy" and len(dq) == 1 and dq[0][0] == "axpbypcz" and c[2] == -dq[0][3] and c[4] == dq[0][6] and c[1] not in (c[3], c[4], dq[0][1], dq[0][5]) and c[3] != dq[0][1]:
            dq.append(c); return
        if k == "copy" and len(dq) == 2 and dq[0][0] == "axpy" and c[1] == dq[1][1] and c[2] not in (dq[0][1], dq[1][1], dq[0][3]):
            dq.append(c); return
        if k == "maxpy":
            self.flush(); self.dq = [c]; return
        if k == "pmult":
            w, x, y = c[1:]
            if self.pp and (x == self.pp[2]) != (y == self.pp[2]):
                d = y if x == self.pp[2] else x
                if w not in (self.pp[1], self.pp[2], d) and d != self.pp[1]:
                    self.pl, self.pp = self.pp, None; return
            if len(dq) == 2 and dq[0][0] == "axpy" and (x == dq[1][1]) != (y == dq[1][1]):
                r = dq[1][1]; d = y if x == r else x
                if w not in (dq[0][1], r, dq[0][3], d) and d not in (dq[0][1], r):
                    dq.append(c); return
            self.flush()
            if w not in (x, y): self.dq = [c]
            return
        if k == "matmult":
            self.flush()
            if self.pl and self.pl[2] == c[3]: self.pl = None
            if self.pl and self.pl[1] == c[3]: self.pl = None
            self.pp = (c[1], c[2], c[3]); return
        self.flush()


# ---------------------------------------------------------------------------------------------------- generator
def _motifs():
    def cg(third, natural):
        def f(v, a, b):
            x, p, r, w, z, d = v[:6]
            t = ("pmult", z, r, d) if third == "pmult" else ("copy", r, z)
            tail = [("tdot", z, r), ("norm", z, 1)] if natural else [("norm", z, 1), ("tdot", z, r)]
            return [("axpy", x, a, p), ("axpy", r, -a, w), t] + tail
        return f

    def bcgs(norm_first, predot):
        def f(v, a, b):
            x, p, s, r, t, rp = v[:6]
            tail = [("norm", r, 1), ("dot", r, rp)] if norm_first else [("dot", r, rp), ("norm", r, 1)]
            return ([("dot", r, rp)] if predot else []) + [("axpbypcz", x, a, b, 1.0, p, s), ("waxpy", r, -b, t, s)] + tail
        return f

    def maxpy(last):
        return lambda v, a, b: [("maxpy", v[0], (a, b, -0.3, 1.1, 0.01, -2.5)[:1 + int(abs(a * 40)) % 6], tuple(v[1:7])[:1 + int(abs(a * 40)) % 6]), last(v[0])]

    def mm(tail):
        def f(v, a, b):
            x, t, w, d, y = v[:5]
            return [("matmult", "A", x, t), ("pmult", w, t, d)] + {"late": [("tdot", t, y)], "never": [], "over": [("copy", y, t)], "xwrite": [("set", x, a), ("tdot", t, y)]}[tail]
        return f
    return {"cg_pmult": cg("pmult", False), "cg_copy": cg("copy", False), "cg_natural": cg("pmult", True),
            "bcgs_norm_first": bcgs(True, False), "bcgs_norm_first_predot": bcgs(True, True),
            "bcgs_dot_first": bcgs(False, False), "bcgs_dot_first_predot": bcgs(False, True),
            "maxpy_norm": maxpy(lambda y: ("norm", y, 1)), "maxpy_normalize": maxpy(lambda y: ("normalize", y)),
            "pmult_dot": lambda v, a, b: [("pmult", v[0], v[1], v[2]), ("dot", v[0], v[3])],
            "pmult_dotnorm2": lambda v, a, b: [("pmult", v[0], v[1], v[2]), ("dotnorm2", v[3], v[0])],
            "mm_pmult_late": mm("late"), "mm_pmult_never": mm("never"), "mm_pmult_over": mm("over"), "mm_pmult_xwrite": mm("xwrite")}


MOTIFS = _motifs()
MOTIF_LEN = {name: len(f(list(range(8)), 0.37, 0.7)) for name, f in MOTIFS.items()}


def _table():
    t, rot = [], {}
    for name in MOTIFS:
        t.append((name, None, None, 0))
        for cut in range(1, MOTIF_LEN[name]):
            for cls in CUT_CLASSES:
                mv = cls == "matvalue" and name.startswith("mm_")
                key = (cls, cut) if mv else cls            # behind a product the matrix value operations rotate per position, one per program:
                for _ in range(6 if mv else 1):            # each of them meets a noted product, and an unwritten work vector
                    t.append((name, cut, cls, rot.get(key, 0)))
                    rot[key] = rot.get(key, 0) + (1 if mv else 2)
    return t


TABLE = _table()
SEEDS = list(range(len(TABLE)))
RANK_SEEDS = [i for i in SEEDS[::9] if TABLE[i][0] != "maxpy_normalize"]      # the run on two ranks: a sample (no VecNormalize there)
SHAPES = ("lap2d", "nonsym300", "lap2d")


def shape_of(index):
    return "n1" if index % 13 == 6 else SHAPES[index % 3]


class _Gen:
    def __init__(self, index, ranks):
        self.rng = np.random.default_rng([index, 2026])
        self.ranks = ranks
        shape = shape_of(index)
        self.pl = pool("lap2d" if ranks and shape == "n1" else shape, index)      # (a rank without rows would have nothing to show)
        self.model, self.pend = Model(self.pl), Pending()
        self.calls, self.prev, self.buf = [], 0.37, 0
        self.n, self.m = self.pl["n"], self.pl["m"]
        self.limit, self.force_mat, self.force_parent = 10, None, None

    # -- operands
    def sc(self, nonzero=False):
        r = self.rng
        a = -self.prev if r.random() < 0.3 else float(r.choice(SCALARS))
        if nonzero and a == 0.0:
            a = 0.37
        self.prev = a
        return a

    def usable(self, write, among=None):
        m = self.model
        wlent = {p for p, _, w in m.lent.values() if w}
        rlent = {p for p, _, w in m.lent.values() if not w}
        out = [v for v in (range(NV) if among is None else among) if v not in m.open and v not in wlent and not (write and v in rlent)]
        return out

    def pick(self, k, write=False, distinct=True, exclude=()):
        c = [v for v in self.usable(write) if v not in exclude]
        return [int(v) for v in (self.rng.choice(c, size=k, replace=False) if distinct else self.rng.choice(c, size=k))]

    def away_from_zero(self, v):
        return np.min(np.abs(self.model.vec(v))) > 0.05

    # -- emitting
    def emit(self, c, must=True):
        """append the call if the model stays tame under it"""
        if len(self.calls) >= self.limit and not must:
            return False
        trial = copy.deepcopy(self.model)
        try:
            with np.errstate(all="ignore"):
                trial.apply(c)
        except (ValueError, ZeroDivisionError):
            trial = None
        if trial is None or not trial.tame():
            assert not must, ("a motif call went wild", c)
            return False
        self.pend.step(c, trial.cached)
        self.model = trial
        self.calls.append(c)
        return True

    def one(self, kind, must=False):
        """one call of a kind (a few kinds are short sequences) with random operands; False when it did not fit"""
        r, e = self.rng, lambda c: self.emit(c, must)
        if kind in ("set", "scale"):
            return e((kind, self.pick(1, True)[0], self.sc()))
        if kind in ("copy", "swap"):
            x, y = self.pick(2, True); return e((kind, x, y))
        if kind in ("axpy", "aypx"):
            y, x = self.pick(2, True); return e((kind, y, self.sc(), x))
        if kind == "axpby":
            y, x = self.pick(2, True); return e((kind, y, self.sc(), self.sc(), x))
        if kind == "waxpy":
            w = self.pick(1, True)[0]; x, y = self.pick(2, distinct=False, exclude=(w,)); return e((kind, w, self.sc(), x, y))
        if kind == "axpbypcz":
            z, x, y = self.pick(3, True); return e((kind, z, self.sc(), self.sc(), 1.0 if r.random() < 0.6 else self.sc(), x, y))
        if kind == "maxpy":
            y = self.pick(1, True)[0]; nv = int(r.integers(1, 7)); xs = self.pick(nv, distinct=False, exclude=(y,))
            return e((kind, y, tuple(self.sc() for _ in range(nv)), tuple(xs)))
        if kind == "pmult":
            w = self.pick(1, True)[0]; x, y = self.pick(2, distinct=False); return e((kind, w, x, y))
        if kind == "pdiv":
            w = self.pick(1, True)[0]; x, y = self.pick(2, distinct=False)
            return self.away_from_zero(y) and e((kind, w, x, y))
        if kind == "recip":
            v = self.pick(1, True)[0]; return self.away_from_zero(v) and e((kind, v))
        if kind in ("dot", "tdot", "dotnorm2"):
            x, y = self.pick(2, distinct=False); return e((kind, x, y))
        if kind == "mdot":
            x = self.pick(1)[0]; return e((kind, x, tuple(self.pick(int(r.integers(1, 5)), distinct=False))))
        if kind.startswith("norm") and kind != "normalize" and kind != "normbegin":
            t = int(kind[4:]) if len(kind) > 4 else int(r.choice([0, 1, 3, 4])); return e(("norm", self.pick(1)[0], t))
        if kind == "normalize":
            return e((kind, self.pick(1, True)[0]))
        if kind == "split":
            begins = []
            for _ in range(int(r.integers(1, 4))):
                if r.random() < 0.5:
                    x, y = self.pick(2, distinct=False); begins.append(("dotbegin", x, y))
                else:
                    begins.append(("normbegin", self.pick(1)[0]))
            for b in begins: e(b) or self._fail()
            k, at = int(r.integers(0, 4)), int(r.integers(-2, 4))          # PetscCommSplitReductionBegin: before, among or behind the calls between, or left to the first End
            for j in range(k + 1):
                if j == at: e(("srbegin",))
                if j < k: self.one(str(r.choice(["axpy", "maxpy", "pmult", "axpbypcz", "scale", "dot", "norm1", "matmult"])))
            for b in begins: self.emit(("dotend", b[1], b[2]) if b[0] == "dotbegin" else ("normend", b[1]), True)
            return True
        if kind in ("getrestore", "restorearray"):
            v = self.pick(1, True)[0]
            if not e(("getarray", v)): return False
            if kind == "restorearray" or r.random() < 0.5:
                for _ in range(int(r.integers(1, 3))):
                    self.one(str(r.choice(["axpy", "pmult", "dot", "norm1", "scale", "maxpy"])))
            return self.emit(("restorearray", v, int(r.integers(1, 9))), True)
        if kind == "getarrayread":
            return e((kind, self.pick(1)[0]))
        if kind.startswith("setvalues"):
            v = self.pick(1, True)[0]; ni = int(min(self.n, r.integers(1, 6)))
            idx = tuple(int(i) for i in r.choice(self.n, size=ni, replace=False))
            mode = INSERT if kind.endswith("insert") else (ADD if kind.endswith("add") else int(r.choice([INSERT, ADD])))
            return e(("setvalues", v, idx, tuple(float(x) for x in np.round(r.uniform(-2, 2, ni), 3)), mode))
        if kind in ("placearray", "replacearray", "recreate"):
            c = [v for v in self.usable(True) if v not in self.model.placed and v not in {p for p, _, _ in self.model.lent.values()}]
            if not c: return False
            v = int(r.choice(c))
            if kind == "recreate":
                return e((kind, v, self.pick(1, exclude=(v,))[0]))
            self.buf += 1
            return e((kind, v, self.buf))
        if kind == "resetarray":
            if not self.model.placed and not self.one("placearray"): return False
            c = [v for v in self.model.placed if v in self.usable(True)]
            return bool(c) and e((kind, int(r.choice(c))))
        if kind in ("share0", "share1", "shareend"):
            if self.ranks: return False
            free = [s for s in BORROWERS if s not in self.model.lent]
            c = [v for v in self.usable(True) if v not in {p for p, _, _ in self.model.lent.values()}]
            if not free or not c: return False
            s, p, write = free[0], int(r.choice(c)) if self.force_parent is None else self.force_parent, 0 if kind == "share0" else 1
            if write and not self.pend.any(): e(("norm", p, 1))                       # asked again behind the End: a norm kept for the parent must not survive the borrower's writes
            if not e(("sharebegin", s, p, int(r.integers(0, self.n - self.m + 1)), write)): return False
            if write and self.m == self.n:
                self.emit(("set", s, self.sc()), True)       # a borrower that takes the whole vector for writing has promised to write all of it
            if write and self.m < self.n: self.emit(("pmult", s, s, s), False)
            if kind != "shareend":
                self._borrower_calls(s, write)
                self.emit(("shareend", s), True)
                if write: self.emit(("norm", p, 1), True)
            return True
        if kind in ("matmult", "matmulttranspose"):
            x = self.pick(1)[0]; y = self.pick(1, True, exclude=(x,))[0]
            return e((kind if not self.ranks else "matmult", "A" if self.ranks else str(r.choice(["A", "B"])), x, y))
        if kind == "matmultadd":
            x, y = self.pick(2, distinct=False); z = self.pick(1, True, exclude=(x,))[0]
            return e((kind, str(r.choice(["A", "B"])), x, y, z))
        M = self.force_mat or str(r.choice(["A", "A", "B"]))
        if kind in ("matscale", "matshift"):
            return e((kind, M, float(r.choice(MSCALARS))))
        if kind == "matdiagscale":
            ok = [v for v in self.usable(False) if np.max(np.abs(self.model.vec(v))) < 4 and self.away_from_zero(v)]
            if not ok: return False
            l, rr = (int(v) for v in r.choice(ok, size=2)); which = int(r.integers(0, 3))
            return e((kind, M, None if which == 1 else l, None if which == 0 else rr))
        if kind == "matzeroentries":
            return e((kind, M)) and self.emit(("matcopy", "B" if M == "A" else "A", M), True)
        if kind == "mataxpy":
            return e((kind, M, float(r.choice(MSCALARS)) * 0.25, "B" if M == "A" else "A"))
        if kind == "matcopy":
            return e((kind, "B" if M == "A" else "A", M))
        if kind.startswith("matzerorows"):
            rows = tuple(sorted(int(i) for i in r.choice(self.n, size=int(min(self.n, r.integers(1, 5))), replace=False)))
            x = self.pick(1)[0]
            b = self.pick(1, True, exclude=(x,))[0]
            with_b = kind.endswith("_b")
            if with_b and not self.pend.any(): e(("norm", b, 1))                      # (and again behind the call: b changes under a norm the wrapper keeps)
            ok = e((kind.replace("_b", ""), M, rows, float(r.choice([1.0, 2.0, -1.5])), x if with_b else None, b if with_b else None))
            if ok and with_b: self.emit(("norm", b, 1), True)
            return ok
        if kind == "matsor":
            b, x = self.pick(2, True); return e((kind, M, b, x))
        raise ValueError(kind)

    def _fail(self):
        raise AssertionError("a call that cannot go wild was refused")

    def _borrower_calls(self, s, write):
        r = self.rng
        other = [t for t in BORROWERS if t != s and t in self.model.lent]
        for _ in range(int(r.integers(0, 3))):
            odd = self.model.lent[s][1] % 2               # (no VecSet / VecScale there: a kept norm they carry along would need a bound of its own)
            q = str(r.choice((["norm", "dot", "axpy", "pmult"] if odd else ["norm", "dot", "set", "scale", "axpy", "pmult"]) if write else ["norm", "dot"]))
            o = other[0] if other else s
            if q == "norm": self.emit(("norm", s, int(r.choice([0, 1, 3]))), False)
            elif q == "dot": self.emit(("dot", s, o), False)
            elif q in ("set", "scale"): self.emit((q, s, self.sc()), False)
            elif q == "axpy" and o != s: self.emit(("axpy", s, self.sc(), o), False)
            elif q == "pmult": self.emit(("pmult", s, s, o), False)

    def random_calls(self, k):
        kinds = [q for cls in ("elementwise", "reduction", "storage", "matvalue", "destroy", "split") for q in CUT_KINDS[cls]] + ["matmult", "matmultadd", "matmulttranspose"] * 3
        if self.ranks:
            kinds = [q for q in kinds if q not in CUT_KINDS["matvalue"] and q not in ("normalize", "matmultadd", "matmulttranspose")]
        for _ in range(k):
            self.one(str(self.rng.choice(kinds)))

    def close(self):
        """whatever is still open ends, in the order a program would end it"""
        for v in sorted(self.model.open): self.emit(("restorearray", v, 1), True)
        for s in sorted(self.model.lent): self.emit(("shareend", s), True)
        for v in sorted(self.model.placed): self.emit(("resetarray", v), True)


def closing_calls(calls):
    """the calls that end what a prefix of a program left open"""
    opened, lent, placed = [], [], []
    for c in calls:
        if c[0] == "getarray": opened.append(c[1])
        elif c[0] == "restorearray": opened.remove(c[1])
        elif c[0] == "sharebegin": lent.append(c[1])
        elif c[0] == "shareend": lent.remove(c[1])
        elif c[0] == "placearray": placed.append(c[1])
        elif c[0] == "resetarray": placed.remove(c[1])
        elif c[0] == "recreate" and c[1] in placed: placed.remove(c[1])
    nsr = sum(c[0] in ("dotbegin", "normbegin") for c in calls) - sum(c[0] in ("dotend", "normend") for c in calls)
    pend = [c for c in calls if c[0] in ("dotbegin", "normbegin")][-nsr:] if nsr else []
    return ([("dotend", c[1], c[2]) if c[0] == "dotbegin" else ("normend", c[1]) for c in pend] + [("restorearray", v, 1) for v in sorted(opened)]
            + [("shareend", s) for s in sorted(lent)] + [("resetarray", v) for v in sorted(placed)])


def probe_calls(n, ranks=False):
    """the matrices' values as the program's last calls: products with a fixed vector"""
    idx = tuple(range(n))
    vals = tuple(float(v) for v in np.round(1.0 + 0.5 * np.cos(1.3 * np.arange(n)), 6))
    return [("setvalues", 6, idx, vals, INSERT), ("matmult", "A", 6, 7)] + ([] if ranks else [("matmult", "B", 6, 5)])


def generate(index, ranks=False):
    """the program of TABLE[index]: dict(index, shape, n, m, motif, cut, cls, marks -- where the motif's calls sit --, calls); ranks: Vec calls and MatMult alone, for
    the run on two ranks (nothing borrows storage, no VecNormalize: its scale would carry a reduction into the vectors)"""
    name, cut, cls, rot = TABLE[index]
    g = _Gen(index, ranks)
    r = g.rng
    with orc.device_reduction_order():
        g.random_calls(int(r.integers(0, 5)))
        g.close()
        g.limit = 26
        roles = g.pick(8)
        a, b = float(r.choice([0.37, -0.7, 1.25, 0.5, -1.7])), float(r.choice([0.7, -0.37, 1.5]))
        motif = MOTIFS[name](roles, a, b)
        pro = None
        if cls is not None:
            kinds = CUT_KINDS[cls]
            if ranks and cls == "matvalue":
                kinds = ["matmult"]
            pro = [kinds[(rot + j) % len(kinds)] for j in range(1 if (cls == "matvalue" and name.startswith("mm_")) else (2 if (cls == "matvalue" or r.random() < 0.4) else 1))]
            if ranks:
                pro = [q for q in pro if not q.startswith("share") and q != "normalize"] or ["getarrayread"]
            # what ends at the cut has to begin before the motif
            for q in pro:
                if q == "resetarray" and not g.model.placed: g.one("placearray", True)
                if q == "shareend":
                    g.force_parent = roles[7]; g.one("shareend", True); g.force_parent = None       # (the Begin alone)
                if q == "restorearray":
                    g.emit(("getarray", roles[7]), True)
            g.force_mat = "A" if name.startswith("mm_") else None
        marks = []
        for i, c in enumerate(motif):
            if cut is not None and i == cut:
                for q in pro:
                    if q == "shareend": g.emit(("shareend", sorted(g.model.lent)[0]), True)
                    elif q == "restorearray": g.emit(("restorearray", sorted(g.model.open)[0], 3), True)
                    elif not g.one(q, False):
                        g.one({"elementwise": "axpy", "reduction": "dot", "storage": "getarrayread", "matvalue": "matscale", "destroy": "recreate", "split": "split"}[cls], True)
            marks.append(len(g.calls))
            rd, wr = operands(c)
            if any(v in g.model.open or v not in g.usable(bool(v in wr), among=[v]) for v in rd + wr):
                g.close()                                    # an interrupting call left a motif vector open or lent: end that first
            g.emit(c, True)
        g.force_mat = None
        if cut is None and r.random() < 0.7:                 # a second motif on the same vectors while the first one's remains are live
            second = list(MOTIFS)[int(r.integers(0, len(MOTIFS)))]
            for c in MOTIFS[second](roles if r.random() < 0.5 else roles[2:] + roles[:2], -a, b):
                g.emit(c, True)
        g.limit = 30
        g.random_calls(int(r.integers(0, 5)))
        g.close()
        for c in probe_calls(g.n, ranks):
            g.emit(c, True)
    assert len(g.calls) <= MAXCALLS, len(g.calls)
    return dict(index=index, shape=g.pl["shape"], n=g.n, m=g.m, motif=name, cut=cut, cls=cls, marks=marks, calls=g.calls)


def reference(prog, upto=None, world=1):
    """(scalars, final vectors, model) of a program -- or of its first `upto` calls, ended properly -- on the model"""
    calls = prog["calls"] if upto is None else prog["calls"][:upto] + closing_calls(prog["calls"][:upto])
    m = Model(pool(prog["shape"], prog["index"]))
    m.world = world
    with orc.device_reduction_order(), np.errstate(all="ignore"):
        for c in calls:
            m.apply(c)
    return np.array(m.out, dtype=np.float64), [v.copy() for v in m.V], m


# ---------------------------------------------------------------------------------------------------- executor
def share_functions(P, vec):
    """the two methods a vector offers by name: ("VecShareSubArrayBegin_C", "VecShareSubArrayEnd_C") as callables"""
    L = P.lib()
    q = L.raw("PetscObjectQueryFunction")
    q.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]; q.restype = C.c_int
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int)
    fns = []
    for name in (b"VecShareSubArrayBegin_C", b"VecShareSubArrayEnd_C"):
        f = C.c_void_p()
        L.chk(q(vec.h, name, C.byref(f)))
        assert f.value, name
        fns.append(proto(f.value))
    return fns


def execute(P, prog, upto=None, flush_each=False, comm=None, rows=None):
    """Run a program (or its first `upto` calls, ended properly) on the library: (scalars, final vectors).  comm / rows: the
    communicator and this rank's row range (lo, hi) of a run on several ranks; the vectors returned are the local parts."""
    L = P.lib()
    pl = pool(prog["shape"], prog["index"])
    calls = prog["calls"] if upto is None else prog["calls"][:upto] + closing_calls(prog["calls"][:upto])
    n, ai, aj = pl["n"], pl["ai"], pl["aj"]
    lo, hi = rows if rows else (0, n)
    nl = hi - lo
    dp = lambda a: a.ctypes.data_as(C.c_void_p)
    as_array = lambda p, k: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), (k,))
    flush = L.raw("VecHIPMI355XFlushDeferred")
    if rows:
        V = [P.Vec.from_array(v[lo:hi], comm=comm, N=n) for v in pl["vecs"][:NV]]
        sl = lambda a: ((ai[lo:hi + 1] - ai[lo]).astype(np.int32), aj[ai[lo]:ai[hi]].copy(), a[ai[lo]:ai[hi]].copy())
        M = {"A": P.Mat.from_csr_mpi(*sl(pl["aa"]), nl, n, n, comm=comm)}
    else:
        V = [P.Vec.from_array(v, comm=L.COMM_SELF) for v in pl["vecs"]]
        M = {"A": P.Mat.from_csr(ai, aj, pl["aa"]), "B": P.Mat.from_csr(ai, aj, pl["bb"])}
        for A in M.values():
            A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
        share_begin, share_end = share_functions(P, V[8])
    out, keep, opened, lent = [], [], {}, {}
    val, val2, two = C.c_double(), C.c_double(), (C.c_double * 2)()
    h = lambda v: V[v].h
    try:
        for c in calls:
            k = c[0]
            if k in ("set", "scale"): getattr(L, "VecSet" if k == "set" else "VecScale")(h(c[1]), c[2])
            elif k == "copy": L.VecCopy(h(c[1]), h(c[2]))
            elif k == "swap": L.VecSwap(h(c[1]), h(c[2]))
            elif k == "axpy": L.VecAXPY(h(c[1]), c[2], h(c[3]))
            elif k == "aypx": L.VecAYPX(h(c[1]), c[2], h(c[3]))
            elif k == "axpby": L.VecAXPBY(h(c[1]), c[2], c[3], h(c[4]))
            elif k == "waxpy": L.VecWAXPY(h(c[1]), c[2], h(c[3]), h(c[4]))
            elif k == "axpbypcz": L.VecAXPBYPCZ(h(c[1]), c[2], c[3], c[4], h(c[5]), h(c[6]))
            elif k == "maxpy":
                al = np.array(c[2], dtype=np.float64)
                L.VecMAXPY(h(c[1]), len(c[3]), dp(al), P.vec_table([V[v] for v in c[3]]))
            elif k == "pmult": L.VecPointwiseMult(h(c[1]), h(c[2]), h(c[3]))
            elif k == "pdiv": L.VecPointwiseDivide(h(c[1]), h(c[2]), h(c[3]))
            elif k == "recip": L.VecReciprocal(h(c[1]))
            elif k in ("dot", "tdot"):
                getattr(L, "VecDot" if k == "dot" else "VecTDot")(h(c[1]), h(c[2]), C.byref(val)); out.append(val.value)
            elif k == "mdot":
                res = np.zeros(len(c[2]))
                L.VecMDot(h(c[1]), len(c[2]), P.vec_table([V[v] for v in c[2]]), dp(res)); out.extend(res)
            elif k == "dotnorm2":
                L.VecDotNorm2(h(c[1]), h(c[2]), C.byref(val), C.byref(val2)); out.extend([val.value, val2.value])
            elif k == "norm":
                L.VecNorm(h(c[1]), c[2], two); out.extend([two[0], two[1]] if c[2] == 4 else [two[0]])
            elif k == "normalize":
                L.VecNormalize(h(c[1]), C.byref(val)); out.append(val.value)
            elif k == "dotbegin": L.VecDotBegin(h(c[1]), h(c[2]), C.byref(val))
            elif k == "normbegin": L.VecNormBegin(h(c[1]), 1, C.byref(val))
            elif k == "srbegin": L.PetscCommSplitReductionBegin(comm or L.COMM_SELF)
            elif k == "dotend":
                L.VecDotEnd(h(c[1]), h(c[2]), C.byref(val)); out.append(val.value)
            elif k == "normend":
                L.VecNormEnd(h(c[1]), 1, C.byref(val)); out.append(val.value)
            elif k == "getarray":
                opened[c[1]] = C.c_void_p(); L.VecGetArray(h(c[1]), C.byref(opened[c[1]]))
            elif k == "restorearray":
                a = as_array(opened[c[1]], nl)
                q = (c[2] % 3 - lo) % 3                                     # the same global entries on every rank
                a[q::3] = a[q::3] * 0.5 + 0.125 * c[2]
                L.VecRestoreArray(h(c[1]), C.byref(opened.pop(c[1])))
            elif k == "getarrayread":
                p = C.c_void_p(); L.VecGetArrayRead(h(c[1]), C.byref(p))
                a = as_array(p, nl); out.extend([float(a[0]), float(a[-1])])
                L.VecRestoreArrayRead(h(c[1]), C.byref(p))
            elif k == "setvalues":
                mine = [(i, v) for i, v in zip(c[2], c[3]) if lo <= i < hi]     # every rank sets the entries it owns
                idx, vals = np.array([i for i, _ in mine], dtype=np.int32), np.array([v for _, v in mine], dtype=np.float64)
                L.VecSetValues(h(c[1]), idx.size, dp(idx), dp(vals), c[4]); L.VecAssemblyBegin(h(c[1])); L.VecAssemblyEnd(h(c[1]))
            elif k == "placearray":
                keep.append(np.ascontiguousarray(buffer(c[2], n)[lo:hi])); L.VecPlaceArray(h(c[1]), dp(keep[-1]))
            elif k == "resetarray": L.VecResetArray(h(c[1]))
            elif k == "replacearray":
                p = C.c_void_p(); L.PetscMallocFn(max(nl, 1) * 8, C.byref(p))
                as_array(p, nl)[:] = buffer(c[2], n)[lo:hi]
                L.VecReplaceArray(h(c[1]), p)                                # the vector owns the array from here on
            elif k == "sharebegin":
                L.chk(share_begin(h(c[1]), h(c[2]), c[3], c[4])); lent[c[1]] = (c[2], c[3], c[4])
            elif k == "shareend":
                p, off, w = lent.pop(c[1]); L.chk(share_end(h(c[1]), h(p), off, w))
            elif k == "recreate":
                V[c[1]].destroy(); V[c[1]] = V[c[2]].duplicate()           # (destroyed first: the new vector may take the old one's address)
            elif k == "matmult": L.MatMult(M[c[1]].h, h(c[2]), h(c[3]))
            elif k == "matmultadd": L.MatMultAdd(M[c[1]].h, h(c[2]), h(c[3]), h(c[4]))
            elif k == "matmulttranspose": L.MatMultTranspose(M[c[1]].h, h(c[2]), h(c[3]))
            elif k == "matscale": L.MatScale(M[c[1]].h, c[2])
            elif k == "matdiagscale": L.MatDiagonalScale(M[c[1]].h, None if c[2] is None else h(c[2]), None if c[3] is None else h(c[3]))
            elif k == "matshift": M[c[1]].shift(c[2])
            elif k == "matzeroentries": L.MatZeroEntries(M[c[1]].h)
            elif k == "mataxpy": M[c[1]].axpy(c[2], M[c[3]], P.SAME_NONZERO_PATTERN)
            elif k == "matcopy": M[c[1]].copy(M[c[2]], P.SAME_NONZERO_PATTERN)
            elif k in ("matzerorows", "matzerorowscols"):
                f = M[c[1]].zero_rows if k == "matzerorows" else M[c[1]].zero_rows_columns
                f(list(c[2]), c[3], None if c[4] is None else V[c[4]], None if c[5] is None else V[c[5]])
            elif k == "matsor": M[c[1]].sor(V[c[2]], V[c[3]], flag=P.SOR_SYMMETRIC_SWEEP)
            else: raise ValueError(k)
            if flush_each: L.chk(flush())
        finals = [v.array() for v in V]
    finally:
        for v, p in opened.items(): L.VecRestoreArray(h(v), C.byref(p))
        for s, (p, off, w) in lent.items(): share_end(h(s), h(p), off, w)
        for v in V: v.destroy()
        for A in M.values(): A.destroy()
    return np.array(out, dtype=np.float64), finals


COUNTERS = ("cg_sweep", "bcgs_update", "maxpy_norm", "pmult_dot", "pmult_dotnorm2", "scaled_product", "late_product", "kept_dot")


def deferral_counts(P):
    c = (C.c_int * 8)()
    P.lib().VecHIPMI355XGetDeferralCounts(c)
    return np.array(list(c), dtype=np.int64)


def same_scalars(got, m):
    """the scalars of a run against the model's: its bits, or -- where the model says so -- within its bound"""
    ref = np.array(m.out, dtype=np.float64)
    if got.shape != ref.shape:
        return False
    for j, t in enumerate(m.tol):
        if t is None:
            if got[j:j + 1].view(np.uint64)[0] != ref[j:j + 1].view(np.uint64)[0]: return False
        elif not abs(np.longdouble(got[j]) - t[0]) <= t[1]: return False
    return True


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def three_runs(P, prog, upto=None):
    """deferral off, on, and on with everything noted run after each call: [(scalars, vectors)] * 3; the default is back afterwards"""
    setdef = P.lib().raw("VecHIPMI355XSetDeferral")
    runs = []
    try:
        for on, fl in ((0, False), (1, False), (1, True)):
            setdef(on)
            runs.append(execute(P, prog, upto, flush_each=fl))
    finally:
        setdef(-1)
    return runs


def disagreement(P, prog, upto=None):
    """None, or what differs: among the three runs (scalars and vectors), or between them and the model"""
    runs = three_runs(P, prog, upto)
    ref_out, ref_vecs, model = reference(prog, upto)
    names = ("deferral off", "deferral on", "deferral on, flushed after every call")
    for name, (o, vs) in zip(names, runs):
        if not same(o, runs[0][0]):
            return "scalars of '%s' differ from '%s': %s" % (name, names[0], np.flatnonzero(o.view(np.uint64) != runs[0][0].view(np.uint64)) if o.shape == runs[0][0].shape else "count")
        for j, (u, w) in enumerate(zip(vs, runs[0][1])):
            if not same(u, w):
                return "vector %d of '%s' differs from '%s'" % (j, name, names[0])
    for name, (o, vs) in zip(names, runs):
        for j, (u, w) in enumerate(zip(vs, ref_vecs)):
            if not same(u, w):
                return "vector %d of '%s' differs from the model (largest difference %g)" % (j, name, np.max(np.abs(u - w)))
        if not same_scalars(o, model):
            bad = np.flatnonzero(o.view(np.uint64) != ref_out.view(np.uint64)) if o.shape == ref_out.shape else "count"
            return "scalars of '%s' differ from the model at %s: %s against %s" % (name, bad, o[bad][:4] if o.shape == ref_out.shape else o.size, ref_out[bad][:4] if o.shape == ref_out.shape else ref_out.size)
    return None


def explain(P, prog, why):
    """the report of a failing program: seed, pool, and the shortest prefix that still fails (by bisection on the prefix length)"""
    lo, hi = 1, len(prog["calls"])
    while lo < hi:
        mid = (lo + hi) // 2
        if disagreement(P, prog, mid) is not None: hi = mid
        else: lo = mid + 1
    calls = prog["calls"][:lo]
    return ("program %d (%s, n = %d, borrowers of %d; motif %s cut at %s by %s): %s\nshortest failing prefix, %d calls (then %s): %s\n%s"
            % (prog["index"], prog["shape"], prog["n"], prog["m"], prog["motif"], prog["cut"], prog["cls"], why, lo, closing_calls(calls) or "nothing to end",
               disagreement(P, prog, lo), show(calls)))


def pending_trace(prog):
    """per call: (dq kinds, pp, pl) as Pending has them right BEFORE the call"""
    m, p, tr = Model(pool(prog["shape"], prog["index"])), Pending(), []
    with orc.device_reduction_order(), np.errstate(all="ignore"):
        for c in prog["calls"]:
            tr.append((tuple(q[0] for q in p.dq), p.pp, p.pl))
            m.apply(c)
            p.step(c, m.cached)
    return tr
