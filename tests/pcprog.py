"""Random re-set-up programs against a host model, for the factored matrix of host/ilu.c (HipTriFactors): the host factor, the
level-launch copies, the sync-free plans, the Jacobi-sweep form and the device factorisation context, and what survives a second
PCSetUp when the operator's values, pattern or identity, the route, the trisolve mode or the levels of fill change in between.

A program is a list of calls -- tuples (kind, arguments...) -- on ONE long-lived KSP / PC and the two operators "A" and "B" of a pool
entry (same size, different patterns) plus "FA" and "FB", their patterns without the first diagonal entry, whose set-up fails on both
routes.  PCICC has programs of its own over the symmetric positive definite members (generate_icc).
generate(index) builds the program of TABLE[index]: a motif (configuration, change, configuration), whole, with random calls around it.
Model replays a program on NumPy: the operator follows the restatements the suite has, an application is the reference factor of the
operator of the last good set-up applied to b, and PCState predicts what the getters of the PC answer (host/ilu.c's comments, DESIGN 4
and 8).  Executor runs programs on the library and compares.  Importing needs no GPU."""
import ctypes as C
import functools

import numpy as np

import iluk_ref as ik
import orc
import problems as pb
import sor_ref
from sweeps_ref import jacobi_sweeps
from test_mat_zero_rows_cpu import ref_zero_rows_columns, ref_zero_rows_new_pattern

MAXCALLS = 24
ZP = 100.0 * 2.220446049250313e-16                    # PCILU's zeropivot and shiftamount (harness pcfactor.c, ilu.c:388-389)
MISSING_DIAGONAL = 73                                 # PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry"
BOUND = 1e-13                                         # sums in dependency-level order against the column-order routine, relative
OPERATORS = ("p7", "lap2d", "nonsym", "inode")
ICC_OPERATORS = ("icc_p7", "icc_lap2d")               # the symmetric positive definite members, unperturbed
ICC_CFG = ("host", "syncfree", "column", None, None, 0)   # host/icc.c reads no option: host factorisation, sync-free plans, zero fill
MODES = ("syncfree", "level", "sweeps")
ROUTES = ("host", "device")
CHANGES = ("device", "host", "pattern")
CROSSINGS = ("sweeps_to_syncfree", "levels_0_1_0", "a_b_a", "host_device_host_level", "shift_then_clean", "failed_then_good", "use_levels_other_pattern")
KINDS = ("setup", "setup_same", "apply", "apply_in_place", "solve_preonly", "mark_aborted", "matscale", "matdiagscale", "matshift", "mataxpy_same",
         "matzerorowscols", "setvalues_same_pattern", "matzerorows_default", "swap_operator", "load_values")
DEVICE_CHANGES = ("matscale", "matdiagscale", "matshift", "mataxpy_same", "matzerorowscols")


# ---------------------------------------------------------------------------------------------------- pool
def _dominant(ai, aj, aa):
    """the same pattern with |a_ii| = 1 + the sum of the row's other magnitudes"""
    aa = np.array(aa, dtype=np.float64)
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    off = np.zeros(ai.size - 1)
    np.add.at(off, rows[rows != aj], np.abs(aa[rows != aj]))
    aa[rows == aj] = off + 1.0
    return ai.astype(np.int32), aj.astype(np.int32), aa


def _reversed(ai, aj, aa):
    """P A P^T with P the reversal of the numbering: another pattern of the same size, as dominant"""
    n = ai.size - 1
    rows = n - 1 - np.repeat(np.arange(n), np.diff(ai))
    cols = n - 1 - aj
    o = np.lexsort((cols, rows))
    bi = np.zeros(n + 1, np.int32); np.add.at(bi, rows + 1, 1)
    return np.cumsum(bi).astype(np.int32), cols[o].astype(np.int32), aa[o].copy()


def _perturbed(csr):
    ai, aj, aa = csr
    return ai.astype(np.int32), aj.astype(np.int32), aa * (1.0 + 0.05 * np.sin(np.arange(aa.size)))


@functools.lru_cache(maxsize=None)
def operator(name):
    """{"A": csr, "B": csr}: two patterns of one size, full diagonal, diagonally dominant, values O(1)"""
    if name == "icc_p7":
        A, B = orc.gen_p7(10, 12, 11), orc.gen_p7(12, 11, 10)
    elif name == "icc_lap2d":
        A, B = pb.lap2d(23, 19), pb.lap2d(19, 23)
    elif name == "p7":
        A, B = _perturbed(orc.gen_p7(10, 12, 11)), _perturbed(orc.gen_p7(12, 11, 10))
    elif name == "lap2d":
        A, B = pb.lap2d(23, 19), _dominant(*_perturbed(pb.lap2d(19, 23)))
    elif name == "nonsym":
        A = sor_ref.nonsym200(300, dominant=True); B = _reversed(*A)
    else:
        # three nodes in a line is the smallest grid with three node levels; B couples all three nodes
        A = _dominant(*pb.elasticity_like(3, 1, 1)[0])
        rng = np.random.default_rng(5)
        B = _dominant(np.arange(0, 82, 9, dtype=np.int32), np.tile(np.arange(9, dtype=np.int32), 9), rng.standard_normal(81))
    out = {k: tuple(np.ascontiguousarray(a, dtype=t) for a, t in zip(v, (np.int32, np.int32, np.float64))) for k, v in (("A", A), ("B", B))}
    assert out["A"][0].size == out["B"][0].size and not (out["A"][0][-1] == out["B"][0][-1] and np.array_equal(out["A"][1], out["B"][1]))
    return out


def rhs(n, seed):
    rng = np.random.default_rng([seed, 11])
    return rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)


def scaling(n, seed, width):
    return 1.0 + width * np.cos(1.7 * np.arange(n) + seed)


def new_values(base, seed):
    """setvalues_same_pattern: the pool's values, perturbed"""
    return base * (1.0 + 0.04 * np.cos(0.7 * np.arange(base.size) + seed))


def show(calls):
    """a program as readable calls, one per line"""
    return "\n".join("%3d  %s(%s)" % (i, c[0], ", ".join(repr(a) for a in c[1:])) for i, c in enumerate(calls))


def options(cfg, icc=False):
    """the option string of a setup call (route, tri, order, nodes, block_columns, levels); PCICC takes none"""
    if icc: return ""
    route, tri, order, nodes, bc, levels = cfg
    s = "-pc_factor_hipmi355x_numeric %s -pc_factor_hipmi355x_trisolve %s -pc_factor_levels %d" % (route, tri, levels)
    if order is not None: s += " -pc_factor_hipmi355x_trisolve_order " + order
    if nodes is not None: s += " -pc_factor_hipmi355x_trisolve_nodes %d" % nodes
    if bc is not None: s += " -pc_factor_hipmi355x_trisolve_block_columns %d" % bc
    return s


# ---------------------------------------------------------------------------------------------------- reference factors
@functools.lru_cache(maxsize=64)
def _layout(ai_b, aj_b, levels):
    return ik.symbolic(np.frombuffer(ai_b, np.int32), np.frombuffer(aj_b, np.int32), levels)


def layout(ai, aj, levels):
    return _layout(ai.tobytes(), aj.tobytes(), levels)


def level_counts(bi, bj, bd):
    """dependency levels of L and of U of a factor pattern (host/ilu.c row_levels_L / row_levels_U)"""
    n = bi.size - 1
    lo, up = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        c = bj[bi[i]:bi[i + 1]]
        if c.size: lo[i] = lo[c].max() + 1
    for i in range(n - 1, -1, -1):
        c = bj[bd[i + 1] + 1:bd[i]]
        if c.size: up[i] = up[c].max() + 1
    return (int(lo.max()) + 1, int(up.max()) + 1) if n else (0, 0)


def pattern_levels(ai, aj, levels):
    """level_counts of the ILU(levels) factor of a pattern"""
    if levels:
        return level_counts(*layout(ai, aj, levels)[:3])
    n = ai.size - 1
    lo, up = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        c = aj[ai[i]:ai[i + 1]]
        if (c < i).any(): lo[i] = lo[c[c < i]].max() + 1
    for i in range(n - 1, -1, -1):
        c = aj[ai[i]:ai[i + 1]]
        if (c > i).any(): up[i] = up[c[c > i]].max() + 1
    return int(lo.max()) + 1, int(up.max()) + 1


def icc_levels(ai, aj):
    """dependency levels of the two sweeps of ICC(0) (host/icc.c): U^T forward over the columns of A's strict upper triangle, U backward"""
    n = ai.size - 1
    lo, up = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        c = aj[ai[i]:ai[i + 1]]; c = c[c > i]
        if c.size: lo[c] = np.maximum(lo[c], lo[i] + 1)
    for i in range(n - 1, -1, -1):
        c = aj[ai[i]:ai[i + 1]]; c = c[c > i]
        if c.size: up[i] = up[c].max() + 1
    return int(lo.max()) + 1, int(up.max()) + 1


def widest_triangle_row(ai, aj, levels):
    """the longest row of the strict triangles of the ILU(levels) factor of a pattern"""
    if levels:
        bi, _, bd, _ = layout(ai, aj, levels)
        return int(max(np.diff(bi).max(), (bd[:-1] - bd[1:] - 1).max()))
    rows = np.repeat(np.arange(ai.size - 1), np.diff(ai))
    return int(max(np.bincount(rows[aj < rows], minlength=1).max(), np.bincount(rows[aj > rows], minlength=1).max()))


def reference_factor(ai, aj, aa, levels):
    """((bi, bj, bdiag, ba), restarts): MatLUFactorNumeric_SeqAIJ with MatPivotCheck_nz's shifted restarts; zero fill from the oracle,
    with fill from iluk_ref under the same rule (shiftamount, then twice the last shift)"""
    if not levels:
        return orc.ilu0_factor_shift(ai, aj, aa)
    lay = layout(ai, aj, levels)
    shift, ns = 0.0, 0
    while True:
        ba, frow, _, _ = ik.reference_pass(ai, aj, aa, None, [shift], ZP, [1], layout=lay)
        if frow[0] < 0:
            return (lay[0], lay[1], lay[2], ba), ns
        shift = shift * 2.0 if ns else ZP
        ns += 1
        assert ns <= 80


# ---------------------------------------------------------------------------------------------------- model
class PCState:
    """What the long-lived PC and its factored matrix carry from one set-up to the next, as host/ilu.c's comments state it:
    sym / num the counters of PCILUGetNumeric, dev the pattern the device context was built for (operator, pattern serial number,
    levels of fill), factored the operator and state of the last good numeric factorisation, cfg its options, aborted sticky."""

    def __init__(self):
        self.sym = self.num = self.on_device = self.aborted = 0
        self.levels, self.symbolic_done, self.stale = 0, False, True
        self.dev = self.factored = self.cfg = self.snap = None
        self.ok = self.use_levels = False
        self.asked = None                              # the options of the last set-up call, whether or not anything ran under them


class Model:
    """The operators of one program as NumPy arrays, updated call by call, over a PCState that may be older than the program.
    cur: the operator the next set-up announces; per operator: pattern, values, `orig` (where each stored entry sits in the pool's
    arrays), `version` (any change) and `serial` (a new pattern)."""

    def __init__(self, name, index, pc=None):
        self.name, self.index, self.pc = name, index, pc or PCState()
        self.icc = name in ICC_OPERATORS
        self.base = operator(name)
        self.n = self.base["A"][0].size - 1
        self.M = {}
        for k in ("A", "B"):
            ai, aj, aa = self.base[k]
            self.M[k] = dict(ai=ai, aj=aj, aa=aa.copy(), orig=np.arange(aa.size), version=0, serial=0)
            keep = np.ones(aa.size, bool); keep[np.flatnonzero(aj[ai[0]:ai[1]] == 0)[0]] = False
            fi = ai.copy(); fi[1:] -= 1
            self.M["F" + k] = dict(ai=fi, aj=aj[keep].copy(), aa=aa[keep].copy(), orig=np.flatnonzero(keep), version=0, serial=0)
        self.cur, self.back = "A", "A"
        self.bound_only = []                           # per apply-like call: held to the bound only
        self.rc = []                                   # per set-up: the predicted return code

    # -- the operator
    def csr(self, k=None):
        m = self.M[k or self.cur]
        return m["ai"], m["aj"], m["aa"]

    def uid(self):
        return (self.name, self.index, self.cur)

    def axpy_values(self, seed):
        """the Y of mataxpy_same: the current operator's pattern with the pool's values, perturbed -- other values than X holds"""
        return new_values(self.base[self.cur][2], seed)[self.M[self.cur]["orig"]]

    def _diag(self, m):
        return np.flatnonzero(np.repeat(np.arange(self.n), np.diff(m["ai"])) == m["aj"])

    def change(self, c):
        k, m = c[0], self.M[self.cur]
        ai, aj = m["ai"], m["aj"]
        if k == "matscale": m["aa"] = c[1] * m["aa"]
        elif k == "matdiagscale":
            m["aa"] = orc.diagonal_scale(ai, aj, m["aa"], scaling(self.n, c[1], 0.3), None if c[2] is None else scaling(self.n, c[2], 0.05))
        elif k == "matshift":
            a = m["aa"].copy(); a[self._diag(m)] += c[1]; m["aa"] = a
        elif k == "mataxpy_same": m["aa"] = m["aa"] + c[1] * self.axpy_values(c[2])
        elif k == "matzerorowscols": m["aa"] = ref_zero_rows_columns(ai, aj, m["aa"], list(c[1]), c[2])[0]
        elif k == "setvalues_same_pattern": m["aa"] = new_values(self.base[self.cur][2], c[1])[m["orig"]]
        elif k == "matzerorows_default":
            ni, nj, na = ref_zero_rows_new_pattern(ai, aj, m["aa"], list(c[1]), c[2])
            rows = np.repeat(np.arange(self.n), np.diff(ai))
            keep = ~np.isin(rows, np.array(c[1])) | (rows == aj)
            m.update(ai=np.asarray(ni, np.int32), aj=np.asarray(nj, np.int32), aa=np.asarray(na, np.float64), orig=m["orig"][keep])
            assert m["orig"].size == m["aa"].size
            m["serial"] += 1
        elif k == "load_values":
            base = self.base[self.cur][2].copy()
            if c[1] == "shift_case": base[self.base[self.cur][0][0] + np.flatnonzero(self.base[self.cur][1][:self.base[self.cur][0][1]] == 0)[0]] = 0.0
            m["aa"] = base[m["orig"]]
        else: raise ValueError(k)
        m["version"] += 1

    # -- the calls
    def apply(self, c):
        k, pc = c[0], self.pc
        if k == "setup": self.rc.append(self.setup(c[1:]))
        elif k == "setup_same": self.rc.append(self.setup(pc.asked))
        elif k in ("apply", "apply_in_place", "solve_preonly", "mark_aborted"):
            assert pc.ok and (k != "apply_in_place" or pc.cfg[1].startswith("sweeps")) and (k != "mark_aborted" or self.solver()[0] == 1), c
            if k == "mark_aborted": pc.use_levels, pc.aborted = True, 1
            self.bound_only.append(not self.held_to_bits())
        elif k == "swap_operator": self.cur = self.back = c[1]
        elif k == "load_values" and c[1] == "failing_case": self.cur = "F" + self.back
        elif k == "load_values" and self.cur[0] == "F": self.cur = self.back; self.change(c)
        else: self.change(c)

    def setup(self, cfg):
        """PCSetFromOptions + KSPSetOperators + PCSetUp under the options of cfg: the return code"""
        pc, m = self.pc, self.M[self.cur]
        route, levels = cfg[0], cfg[5]
        pc.asked = cfg
        if levels != pc.levels: pc.levels, pc.symbolic_done = levels, False      # PCFactorSetLevels
        if not pc.symbolic_done: pc.factored, pc.stale, pc.symbolic_done = None, True, True   # MatILUFactorSymbolic
        key = (self.uid(), m["version"])
        if pc.factored == key:
            return 0                                   # same operator, same values: nothing to redo, whatever the options say
        pc.factored, pc.ok = None, False
        missing = self._diag(m).size < self.n
        if route == "host":
            pc.dev, pc.on_device = None, 0
            if missing: return MISSING_DIAGONAL
            pc.sym += 1
        else:
            if not (pc.dev is not None and not pc.stale and pc.dev == (self.uid(), m["serial"], levels)):
                pc.dev, pc.on_device = None, 0
                if missing: return MISSING_DIAGONAL
                pc.dev, pc.stale, pc.on_device = (self.uid(), m["serial"], levels), False, 1
                pc.sym += 1
        pc.num += 1
        pc.factored, pc.ok, pc.cfg, pc.use_levels = key, True, cfg, False
        pc.snap = (m["ai"], m["aj"], m["aa"].copy(), levels)
        return 0

    # -- what the last good set-up left
    def inode(self):
        ai, aj, _, levels = self.pc.snap
        nodes, ns = orc.check_inode(ai, aj)
        return (nodes, ns) if nodes > 0 and not levels else (0, None)

    def node_plans(self):
        return self.pc.cfg[1] == "syncfree" and self.inode()[0] > 0 and self.pc.cfg[3] is None

    def solver(self):
        """PCILUGetSolver: (sync-free kernels run, a sync-free application gave up at some time)"""
        return (1 if self.pc.cfg[1] == "syncfree" and not self.pc.use_levels else 0), self.pc.aborted

    def sweeps(self):
        t = self.pc.cfg[1]
        return int(t[7:]) if t.startswith("sweeps") else 0

    def held_to_bits(self):
        """bits are claimed in column order, at the level launches and with sweeps at or above the level count where one lane sums a row
        (host/ilu.c: "bit for bit where a row is summed by one lane"; the row-block kernels do so up to 16 entries, as
        test_add_scaled_short_rows_bit_for_bit states; a wider triangle row is summed by a lane tree); the dependency-level
        order (asked for, or the default on a matrix with inodes) and the block-column node plans agree to rounding, and a small sweep
        count is held to the same figure against its restatement (2k sums of at most a row's length each, on a dominant factor)"""
        route, tri, order, nodes, bc, levels = self.pc.cfg
        ai, aj, _, _ = self.pc.snap
        if tri == "level": return True
        if tri.startswith("sweeps"): return self.sweeps() >= max(pattern_levels(ai, aj, levels)) and widest_triangle_row(ai, aj, levels) <= 16
        if self.node_plans(): return order == "column" and bc is None
        return not ((order == "level") if order is not None else self.inode()[0] > 0)

    def factor(self):
        ai, aj, aa, levels = self.pc.snap
        key = (ai.tobytes(), aj.tobytes(), aa.tobytes(), levels)
        if getattr(self, "_fkey", None) != key:
            self._fkey, self._f = key, orc.icc0_factor(ai, aj, aa) if self.icc else reference_factor(ai, aj, aa, levels)
        return self._f

    def getters(self):
        """after a good set-up: numeric (on_device, symbolic_builds, numeric_runs), fill (levels, nz of the factor, nz of A), shift
        count, sweeps, solver (syncfree, aborted), node plans made"""
        ai, aj, aa, levels = self.pc.snap
        f, ns = self.factor()
        if self.icc: return dict(info=icc_levels(ai, aj) + (ns,))             # PCICCGetInfo: levels of the two sweeps, positive-definite shifts
        return dict(numeric=(self.pc.on_device, self.pc.sym, self.pc.num), fill=(levels, int(f[2][0]) + 1 if levels else int(ai[-1]), int(ai[-1])),
                    shift=ns, sweeps=self.sweeps(), solver=self.solver(), nodes=self.node_plans())

    def expected(self, b):
        """the reference factor of the operator of the last good set-up, applied to b"""
        f, _ = self.factor()
        if self.icc: return orc.icc0_solve(f, b)
        k = self.sweeps()
        ai, aj, _, levels = self.pc.snap
        if k and k < max(pattern_levels(ai, aj, levels)): return jacobi_sweeps(f, b, k)
        if self.node_plans(): return orc.ilu0_solve_inode(f, self.inode()[1], b)
        return orc.ilu0_solve(f, b)


# ---------------------------------------------------------------------------------------------------- generator
def _table():
    t = [("mode", a, b, ch) for a in MODES for b in MODES for ch in CHANGES]
    t += [("route", a, b, ch) for a in ROUTES for b in ROUTES for ch in CHANGES]
    t += [("crossing", x, None, None) for x in CROSSINGS]
    return [e + (rep,) for rep in range(2) for e in t]


TABLE = _table()
SEEDS = list(range(len(TABLE)))
# ICC(0) takes no option, so its motifs are (set-up, change, set-up) over the three kinds of change and the crossings that need none
ICC_CROSSINGS = ("a_b_a", "shift_then_clean", "failed_then_good", "use_levels_other_pattern")
ICC_TABLE = [e + (rep_,) for rep_ in range(2) for e in [("change", ch) for ch in CHANGES] + [("crossing", x) for x in ICC_CROSSINGS]]
ICC_BASE = 1000                                        # ICC programs are numbered from here
ICC_SEEDS = [ICC_BASE + i for i in range(len(ICC_TABLE))]


def operator_of(index):
    return OPERATORS[(index + index // len(OPERATORS)) % len(OPERATORS)]


class _Gen:
    def __init__(self, index):
        self.rng = np.random.default_rng([index, 2027])
        self.name = operator_of(index) if index < ICC_BASE else ICC_OPERATORS[(index + (index - ICC_BASE) // len(ICC_TABLE[::2])) % 2]
        self.icc = index >= ICC_BASE
        self.model = Model(self.name, index)
        self.calls, self.n = [], self.model.n
        self.risky_ops = set()                         # operators holding shift-case values: configurations held to bits, zero fill
        self.small = self.n <= 500                     # fill levels above zero where the reference's Python passes stay short

    @property
    def risky(self):
        return self.model.back in self.risky_ops

    @risky.setter
    def risky(self, on):
        (self.risky_ops.add if on else self.risky_ops.discard)(self.model.back)

    def emit(self, c):
        self.model.apply(c)
        self.calls.append(c)

    def tri(self, mode, levels, small_k=False):
        if mode != "sweeps": return mode
        ai, aj, _ = self.model.csr(self.model.back)      # (never the failing pattern's: its set-up runs no sweep)
        return "sweeps:%d" % (2 if small_k else max(pattern_levels(ai, aj, levels)))

    def cfg(self, route=None, mode=None, levels=None, order="draw", nodes="draw", bc="draw"):
        r = self.rng
        if self.icc: return ICC_CFG
        route = route or str(r.choice(ROUTES))
        mode = mode or str(r.choice(MODES))
        if levels is None: levels = 0 if self.risky else int(r.choice([0, 0, 1, 2])) if self.small else int(r.random() < 0.08)
        if order == "draw": order = "column" if self.risky else [None, "column", "column", "column", "level"][int(r.integers(0, 5))]
        if nodes == "draw": nodes = [None, None, 0][int(r.integers(0, 3))]
        if bc == "draw": bc = 1 if self.name == "inode" and not self.risky and r.random() < 0.15 else None
        if self.name == "inode" and order is None and r.random() < 0.6: order = "column"
        return (route, self.tri(mode, levels, small_k=(mode == "sweeps" and not self.risky and r.random() < 0.12)), order, nodes, bc, levels)

    def setup(self, **kw):
        self.emit(("setup",) + self.cfg(**kw))

    def rows(self):
        """a few rows that still have entries beside the diagonal, never row 0 (the shift case's pivot)"""
        ai = self.model.csr()[0]
        ok = np.flatnonzero(np.diff(ai)[1:] > 1) + 1
        return tuple(sorted(int(i) for i in self.rng.choice(ok, size=min(ok.size, int(self.rng.integers(1, 4))), replace=False)))

    def change(self, kind):
        r = self.rng
        if kind == "device": kind = str(r.choice(DEVICE_CHANGES))
        elif kind == "host": kind = "setvalues_same_pattern"
        elif kind == "pattern": kind = "matzerorows_default" if r.random() < 0.5 else "swap_operator"
        if self.model.cur[0] == "F": self.emit(("load_values", "clean")); self.risky = False
        if kind == "matscale": self.emit((kind, float(r.choice([0.5, 1.25, 2.0] if self.icc else [0.5, -0.75, 1.25, 2.0]))))     # (ICC: the operator stays positive definite)
        elif kind == "matdiagscale": self.emit((kind, int(r.integers(0, 50)), None if r.random() < 0.5 else int(r.integers(0, 50))))
        elif kind == "matshift": self.emit((kind, float(r.choice([0.5, 0.75, 1.25]))))
        elif kind == "mataxpy_same": self.emit((kind, float(r.choice([0.25, 0.5])), int(r.integers(0, 50))))
        elif kind == "matzerorowscols": self.emit((kind, self.rows(), float(r.choice([1.5, 2.0]))))
        elif kind == "setvalues_same_pattern": self.emit((kind, int(r.integers(0, 50)))); self.risky = False
        elif kind == "matzerorows_default": self.emit((kind, self.rows(), float(r.choice([1.5, 2.0]))))
        elif kind == "swap_operator": self.emit((kind, "B" if self.model.back == "A" else "A"))
        else: raise ValueError(kind)

    def applies(self, k=1):
        m, r = self.model, self.rng
        for _ in range(k):
            if not m.pc.ok: return
            kinds = ["apply", "apply", "solve_preonly"] + (["apply_in_place"] if m.sweeps() else []) + (["mark_aborted"] if m.solver()[0] == 1 and r.random() < 0.3 else [])
            self.emit((str(r.choice(kinds)), int(r.integers(0, 1000))))

    def filler(self, k, limit):
        r = self.rng
        for _ in range(k):
            if len(self.calls) > limit: return
            q = r.random()
            if q < 0.35: self.change(str(r.choice(list(DEVICE_CHANGES) + ["setvalues_same_pattern", "matzerorows_default", "swap_operator"]))); self.setup(); self.applies()
            elif q < 0.5 and self.model.pc.ok: self.emit(("setup_same",)); self.applies()
            elif q < 0.6 and not self.risky and self.model.cur[0] != "F":
                self.emit(("load_values", "shift_case")); self.risky = True; self.setup(); self.applies()
            elif q < 0.7 and self.model.cur[0] != "F":
                self.emit(("load_values", "failing_case")); self.setup(); self.emit(("load_values", "clean")); self.risky = False; self.setup(); self.applies()
            else: self.applies()


def generate(index):
    """the program of TABLE[index]: dict(index, operator, n, motif, marks -- where the motif's calls sit --, calls, bound_only)"""
    what, a, b, ch, rep = TABLE[index]
    g = _Gen(index)
    r = g.rng
    g.setup(); g.applies()
    g.filler(int(r.integers(0, 3)), 5)
    g.change("device")                                 # the motif's first set-up finds new values: it runs
    marks = [len(g.calls)]
    if what == "mode":
        route = str(r.choice(ROUTES))
        g.setup(route=route, mode=a); g.applies(); g.change(ch); g.setup(route=route, mode=b); g.applies(2)
    elif what == "route":
        mode = str(r.choice(MODES))
        g.setup(route=a, mode=mode); g.applies(); g.change(ch); g.setup(route=b, mode=mode); g.applies(2)
    elif a == "sweeps_to_syncfree":
        g.setup(route="device", mode="sweeps", levels=0); g.applies(); g.change("device"); g.setup(route="device", mode="syncfree", levels=0); g.applies(2)
    elif a == "levels_0_1_0":
        for lv in (0, 1, 0):
            g.setup(levels=lv); g.applies()
            if lv == 1 or rep: g.change("device")
    elif a == "a_b_a":
        g.emit(("swap_operator", "A")); g.setup(route="device"); g.applies()
        g.emit(("swap_operator", "B")); g.setup(route="device"); g.applies()
        g.emit(("swap_operator", "A")); g.setup(route="device"); g.applies(2)
    elif a == "host_device_host_level":
        for route in ("host", "device", "host"):
            g.setup(route=route, mode="level"); g.applies(); g.change("device" if rep else "host")
        g.setup(route="device", mode="level"); g.applies()
    elif a == "shift_then_clean":
        g.emit(("load_values", "shift_case")); g.risky = True; g.setup(route=ROUTES[rep]); g.applies()
        g.emit(("load_values", "clean")); g.risky = False; g.setup(route=ROUTES[rep]); g.applies(2)
    elif a == "failed_then_good":
        g.setup(route=ROUTES[rep]); g.applies()
        g.emit(("load_values", "failing_case")); g.setup(route=ROUTES[rep])
        g.emit(("load_values", "clean")); g.setup(route=ROUTES[rep]); g.applies(2)
    elif a == "use_levels_other_pattern":
        g.setup(route=ROUTES[rep], mode="syncfree"); g.emit(("mark_aborted", int(r.integers(0, 1000)))); g.applies()
        g.change("pattern"); g.setup(route=ROUTES[rep], mode="syncfree"); g.applies(2)
    marks.append(len(g.calls))
    g.filler(1, MAXCALLS - 7)
    assert len(g.calls) <= MAXCALLS, (index, len(g.calls))
    return dict(index=index, operator=g.name, n=g.n, motif=TABLE[index], marks=marks, calls=g.calls, bound_only=list(g.model.bound_only), rc=list(g.model.rc))


def generate_icc(index):
    """the ICC(0) program of ICC_TABLE[index - ICC_BASE], in the same form"""
    what, a, rep = ICC_TABLE[index - ICC_BASE]
    g = _Gen(index)
    r = g.rng
    g.setup(); g.applies()
    g.filler(int(r.integers(0, 3)), 5)
    g.change(DEVICE_CHANGES[(index - ICC_BASE) % len(DEVICE_CHANGES)])       # rotated: every device-side change meets the ICC factor
    marks = [len(g.calls)]
    if what == "change":
        g.setup(); g.applies(); g.change(a); g.setup(); g.applies(2)
    elif a == "a_b_a":
        for k in ("A", "B", "A"):
            g.emit(("swap_operator", k)); g.setup(); g.applies()
    elif a == "shift_then_clean":
        g.emit(("load_values", "shift_case")); g.risky = True; g.setup(); g.applies()
        g.emit(("load_values", "clean")); g.risky = False; g.setup(); g.applies(2)
    elif a == "failed_then_good":
        g.setup(); g.applies()
        g.emit(("load_values", "failing_case")); g.setup()
        g.emit(("load_values", "clean")); g.setup(); g.applies(2)
    elif a == "use_levels_other_pattern":
        g.setup(); g.emit(("mark_aborted", int(r.integers(0, 1000)))); g.applies()
        g.change("pattern"); g.setup(); g.applies(2)
    marks.append(len(g.calls))
    g.filler(1, MAXCALLS - 7)
    assert len(g.calls) <= MAXCALLS, (index, len(g.calls))
    return dict(index=index, operator=g.name, n=g.n, motif=ICC_TABLE[index - ICC_BASE], marks=marks, calls=g.calls, bound_only=list(g.model.bound_only), rc=list(g.model.rc))


def replay(prog, upto=None):
    m = Model(prog["operator"], prog["index"])
    for c in prog["calls"][:upto]:
        m.apply(c)
    return m


# ---------------------------------------------------------------------------------------------------- executor
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


class Executor:
    """one long-lived KSP and PC per pool operator; run(prog) replays a program on it and on the model and returns None or
    (position of the first failing call, what differed)"""

    def __init__(self, P, name):
        self.P, self.L, self.name = P, P.lib(), name
        L = self.L
        self.pc = C.c_void_p()
        self.icc = name in ICC_OPERATORS
        self.pctype = b"icc" if self.icc else b"ilu"
        self.ran = []                                  # the programs this PC has seen, in order
        self.ksp = P.KSP(comm=L.COMM_SELF); L.KSPGetPC(self.ksp.h, C.byref(self.pc)); L.PCSetType(self.pc, self.pctype)
        self.ksp.set_type("preonly")
        self.state = PCState()
        self.keep = []                                 # the programs' operators outlive the PC that may still name them
        self.reached = dict(syncfree=0, sweeps=0, on_device=0, nodes=0, nshift=0)
        self.counts = dict(programs=0, calls=0, bits=0, bound=0, setups=0)

    def fresh_pc(self):
        L, pc = self.L, C.c_void_p()
        k = self.P.KSP(comm=L.COMM_SELF); L.KSPGetPC(k.h, C.byref(pc)); L.PCSetType(pc, self.pctype)
        return k, pc

    def set_up(self, ksp, pc, A, opts):
        L = self.L
        ksp.set_operators(A)
        L.PetscOptionsClear(); L.PetscOptionsInsertString(opts.encode())
        rc = L.raw("PCSetFromOptions")(pc)
        rc = rc or L.raw("PCSetUp")(pc)
        L.PetscOptionsClear()
        return rc

    def getters(self, pc, full=True):
        L, i = self.L, lambda: C.c_int(-1)
        if self.icc:
            if not full: return {}
            a, b, c = i(), i(), i(); L.PCICCGetInfo_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c))
            return dict(info=(a.value, b.value, c.value))
        a, b, c = i(), i(), i(); L.PCILUGetNumeric_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c))
        out = dict(numeric=(a.value, b.value, c.value))
        if full:
            a, b, c = i(), i(), i(); L.PCILUGetFill_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c)); out["fill"] = (a.value, b.value, c.value)
            a = i(); L.PCILUGetShiftCount_HIPMI355X(pc, C.byref(a)); out["shift"] = a.value
            a = i(); L.PCILUGetSweeps_HIPMI355X(pc, C.byref(a)); out["sweeps"] = a.value
            a, b = i(), i(); L.PCILUGetSolver_HIPMI355X(pc, C.byref(a), C.byref(b)); out["solver"] = (a.value, b.value)
            a, b, c = i(), i(), i(); L.PCILUGetNodeInfo_HIPMI355X(pc, C.byref(a), C.byref(b), C.byref(c)); out["nodes"] = a.value != 0
        return out

    def pc_apply(self, pc, b):
        P, L = self.P, self.L
        vb, vx = P.Vec.from_array(b, comm=L.COMM_SELF), P.Vec.from_array(np.zeros(b.size), comm=L.COMM_SELF)
        rc = L.raw("PCApply")(pc, vb.h, vx.h)
        return rc, vx.array()

    def compare(self, x, ref, to_bits):
        if not np.all(np.isfinite(x)): return "the application is not finite"
        if to_bits:
            return None if np.array_equal(bits(x), bits(ref)) else "application differs from the model in %d entries (largest difference %.3g)" % (int((bits(x) != bits(ref)).sum()), np.max(np.abs(x - ref)))
        rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
        return None if rel <= BOUND else "application is %.3g relative from the model, bound %.3g" % (rel, BOUND)

    def mat(self, csr):
        A = self.P.Mat.from_csr(*csr)
        self.keep.append(A)
        return A

    def host_values(self, A, m, aa):
        """MatZeroEntries, MatSetValues row by row, assembly: new values through the host copy into the same pattern"""
        P, L = self.P, self.L
        ai, aj = m.csr()[:2]
        L.MatZeroEntries(A.h)
        for r in range(m.n):
            lo, hi = int(ai[r]), int(ai[r + 1])
            if hi > lo:
                cols, vals = np.ascontiguousarray(aj[lo:hi]), np.ascontiguousarray(aa[lo:hi])
                L.MatSetValues(A.h, 1, C.byref(C.c_int(r)), hi - lo, cols.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), P.ADD_VALUES)
        L.MatAssemblyBegin(A.h, P.MAT_FINAL_ASSEMBLY); L.MatAssemblyEnd(A.h, P.MAT_FINAL_ASSEMBLY)

    def run(self, prog, upto=None):
        P, L = self.P, self.L
        m = Model(prog["operator"], prog["index"], self.state)
        M = {k: self.mat(m.csr(k)) for k in ("A", "B", "FA", "FB")}
        self.ran.append(prog["index"])
        V = lambda a: P.Vec.from_array(a, comm=L.COMM_SELF)
        self.counts["programs"] += 1
        for pos, c in enumerate(prog["calls"][:upto]):
            k = c[0]
            self.counts["calls"] += 1
            A = M[m.cur]
            # the library's side of a change, before the model moves on
            if k == "matscale": L.MatScale(A.h, c[1])
            elif k == "matdiagscale":
                l, r = V(scaling(m.n, c[1], 0.3)), (None if c[2] is None else V(scaling(m.n, c[2], 0.05)))
                L.MatDiagonalScale(A.h, l.h, None if r is None else r.h)
            elif k == "matshift": A.shift(c[1])
            elif k == "mataxpy_same": A.axpy(c[1], self.mat(m.csr()[:2] + (m.axpy_values(c[2]),)), P.SAME_NONZERO_PATTERN)
            elif k == "matzerorowscols": A.zero_rows_columns(list(c[1]), c[2])
            elif k == "matzerorows_default": A.zero_rows(list(c[1]), c[2])
            m.apply(c)
            A = M[m.cur]
            if k == "setvalues_same_pattern" or (k == "load_values" and c[1] != "failing_case"):
                self.host_values(A, m, m.csr()[2])
            if k in ("setup", "setup_same"):
                self.counts["setups"] += 1
                opts = options(self.state.asked, self.icc)
                rc = self.set_up(self.ksp, self.pc, A, opts)
                if rc != m.rc[-1]: return pos, "PCSetUp returned %d, the model says %d" % (rc, m.rc[-1])
                if rc:
                    got = self.getters(self.pc, full=False)
                    want = {} if self.icc else dict(numeric=(self.state.on_device, self.state.sym, self.state.num))
                else:
                    got, want = self.getters(self.pc), m.getters()
                    for key in ("syncfree", "sweeps", "on_device", "nodes", "nshift"):
                        if not self.icc: self.reached[key] += int(bool({"syncfree": got["solver"][0], "sweeps": got["sweeps"], "on_device": got["numeric"][0], "nodes": got["nodes"], "nshift": got["shift"]}[key]))
                if got != want: return pos, "the getters answer %s, the model says %s" % (got, want)
                # the twin: fresh objects on a fresh matrix of the model's pattern and values, the options of the factorisation in force
                tk, tpc = self.fresh_pc()
                trc = self.set_up(tk, tpc, self.mat(m.csr()), options(self.state.cfg if not rc else self.state.asked, self.icc))
                if bool(trc) != bool(rc): return pos, "the twin's PCSetUp returned %d, the long-lived one %d" % (trc, rc)
                if not rc:
                    b = rhs(m.n, 7000 + pos)
                    (r1, x1), (r2, x2) = self.pc_apply(self.pc, b), self.pc_apply(tpc, b)
                    if r1 or r2: return pos, "PCApply returned %d (long-lived), %d (twin)" % (r1, r2)
                    if not np.array_equal(bits(x1), bits(x2)):
                        return pos, "the long-lived PC and a fresh twin differ in %d entries (largest difference %.3g)" % (int((bits(x1) != bits(x2)).sum()), np.max(np.abs(x1 - x2)))
                    why = self.compare(x1, m.expected(b), m.held_to_bits())
                    if why: return pos, "after the set-up: " + why
                tk.destroy()
            elif k in ("apply", "apply_in_place", "solve_preonly", "mark_aborted"):
                b = rhs(m.n, c[1])
                if k == "apply_in_place":
                    v = V(b); rc = L.raw("PCILUApplyInPlace_HIPMI355X")(self.pc, v.h); x = v.array()
                elif k == "solve_preonly":
                    vb, vx = V(b), V(np.zeros(m.n)); self.ksp.solve(vb, vx); rc, x = 0, vx.array()
                else:
                    vb, vx = V(b), V(np.zeros(m.n))
                    if k == "mark_aborted": L.PCFactorDebugSetAborted_HIPMI355X(self.pc)     # a host flag; the application itself takes the level path
                    rc = L.raw("PCApply")(self.pc, vb.h, vx.h); x = vx.array()
                if rc: return pos, "%s returned %d" % (k, rc)
                to_bits = not m.bound_only[-1]
                self.counts["bits" if to_bits else "bound"] += 1
                why = self.compare(x, m.expected(b), to_bits)
                if why: return pos, why
                if k == "mark_aborted" and not self.icc:
                    a, ab = C.c_int(-1), C.c_int(-1); L.PCILUGetSolver_HIPMI355X(self.pc, C.byref(a), C.byref(ab))
                    if (a.value, ab.value) != m.solver(): return pos, "PCILUGetSolver answers %s, the model says %s" % ((a.value, ab.value), m.solver())
        return None


def explain(P, prog, failure, ran=()):
    """the report of a failing program.  The run stops at the first call that disagrees, so the calls up to it are the shortest failing
    prefix on that PC; the PC carries what the programs before it left (`ran`), so the prefix runs once more on a fresh KSP and PC and
    the report says whether it fails there too -- if not, the state an earlier program left is part of the cause"""
    pos, why = failure
    alone = Executor(P, prog["operator"]).run(prog, upto=pos + 1)
    return ("program %d (%s, n = %d; motif %s at calls %s): call %d: %s\nprograms this PC ran before: %s\non a fresh KSP and PC the prefix %s\n"
            "shortest failing prefix, %d calls:\n%s"
            % (prog["index"], prog["operator"], prog["n"], prog["motif"], prog["marks"], pos, why, list(ran) or "none",
               "passes: the failure needs the earlier programs' state" if alone is None else "fails too, at call %d: %s" % alone, pos + 1, show(prog["calls"][:pos + 1])))
