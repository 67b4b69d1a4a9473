"""MatSOR on the device: the sweep kernels through the C ABI (csrc/sor.hip) against tests/sor_ref.py, bit for bit and between guard
bands, with the fused small-level runs and without; IEEE specials; the Mat type's device route against its host route and the
restatement, with the counts of what it builds; whole solves with -pc_type sor on both routes."""
import ctypes as C

import numpy as np
import pytest

import orc
import sor_ref as sr
from gpu import Dev
from sor_ref import bits

pytestmark = pytest.mark.gpu
GUARD, SENTINEL = 64, -6.02214076e23
ABI_MATRICES = dict(sr.MATRICES, wide_then_chain=sr.wide_then_chain)


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.free_all()


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def V(P, a):
    return P.Vec.from_array(a, comm=P.lib().COMM_SELF)


def set_options(L, s):
    L.PetscOptionsClear()
    if s:
        L.PetscOptionsInsertString(s.encode())


class Banded:
    """n doubles between two guard bands of a sentinel"""

    def __init__(self, dev, a):
        self.dev, self.n = dev, a.size
        self.base = dev.put(np.concatenate([np.full(GUARD, SENTINEL), a, np.full(GUARD, SENTINEL)]))
        self.p = C.c_void_p(self.base.value + 8 * GUARD)

    def set(self, a):
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, self.p, np.ascontiguousarray(a).ctypes.data, 8 * self.n))
        self.dev.sync()

    def get(self):
        full = self.dev.get(self.base, self.n + 2 * GUARD)
        assert np.array_equal(bits(full[:GUARD]), bits(np.full(GUARD, SENTINEL))) and np.array_equal(bits(full[-GUARD:]), bits(np.full(GUARD, SENTINEL))), "a guard band was written"
        return full[GUARD:-GUARD]

    def free(self):
        self.dev.free(self.base)


class AbiCase:
    """one matrix on the device with a plan, the diagonals, and b / t / x between guard bands"""

    def __init__(self, dev, csr, b, create_flags=0):
        self.dev, k = dev, dev.k
        self.ai, self.aj, self.aa = csr
        n = self.n = self.ai.size - 1
        self.d_ai, self.d_aj, self.d_aa = dev.put(self.ai), dev.put(self.aj), dev.put(self.aa)
        self.plan, bad = C.c_void_p(), C.c_int()
        dev.chk(k.mi355x_sor_plan_create(dev.h, n, self.ai.ctypes.data, self.aj.ctypes.data, create_flags, C.byref(self.plan), C.byref(bad)))
        self.b, self.t, self.x = Banded(dev, b), Banded(dev, np.full(n, SENTINEL)), Banded(dev, np.zeros(n))
        self.idiag, self.mdiag = Banded(dev, np.zeros(n)), Banded(dev, np.zeros(n))

    def info(self):
        v = [C.c_int() for _ in range(3)]
        self.dev.chk(self.dev.k.mi355x_sor_plan_info(self.plan, *[C.byref(q) for q in v]))
        return tuple(q.value for q in v)

    def apply(self, x0, omega, flag, fshift, its):
        k, dev = self.dev.k, self.dev
        self.x.set(x0)
        dev.chk(k.mi355x_sor_idiag(dev.h, self.plan, self.d_aa, omega, fshift, self.idiag.p, self.mdiag.p))
        dev.chk(k.mi355x_sor_apply(dev.h, self.plan, self.d_ai, self.d_aj, self.d_aa, self.idiag.p, self.mdiag.p, omega, flag, its, self.b.p, self.t.p, self.x.p))
        x = self.x.get()
        self.t.get(); self.b.get(); self.idiag.get(); self.mdiag.get()
        return x

    def close(self):
        self.dev.chk(self.dev.k.mi355x_sor_plan_destroy(self.plan))
        for p in (self.d_ai, self.d_aj, self.d_aa):
            self.dev.free(p)
        for q in (self.b, self.t, self.x, self.idiag, self.mdiag):
            q.free()


_refs = {}


def reference(name, csr, b, x0, omega, flag, fshift, its, lits):
    key = (name, omega, flag, fshift, its, lits)
    if key not in _refs:
        _refs[key] = sr.sor_ref(csr[0], csr[1], csr[2], b, x0, omega, flag, fshift, its, lits)
    return _refs[key]


# ---------------------------------------------------------------------------------------------------- kernels through the C ABI
@pytest.mark.parametrize("name", list(ABI_MATRICES))
def test_kernels_equal_the_restatement_fused_and_level_by_level(dev, name):
    csr = ABI_MATRICES[name]()
    n = csr[0].size - 1
    b, x0 = sr.rhs(n)
    fused, plain = AbiCase(dev, csr, b), AbiCase(dev, csr, b, create_flags=1)
    nlev, launches, in_runs = fused.info()
    nlev_p, launches_p, in_runs_p = plain.info()
    assert nlev == nlev_p == sr.levels_ref(csr[0], csr[1]).max() + 1
    assert launches_p == nlev and in_runs_p == 0
    if name == "tridiag300":
        assert (nlev, launches, in_runs) == (300, 1, 300)
    if name == "wide_then_chain":                           # one level of 600 rows by its own launch, then the chain's 100 in one
        assert (nlev, launches, in_runs) == (101, 2, 100)
    if name == "one_row":
        assert (nlev, launches, in_runs) == (1, 1, 0)
    for sweep, zero, its, lits, omega, fshift in sr.grid():
        flag = sr.SWEEPS[sweep] | (sr.ZERO_INITIAL_GUESS if zero else 0)
        ref = reference(name, csr, b, x0, omega, flag, fshift, its, lits)
        for case in (fused, plain):
            x = case.apply(x0, omega, flag, fshift, its * lits)
            assert np.array_equal(bits(x), bits(ref)), (name, sweep, zero, its, lits, omega, fshift, case is fused)
    fused.close(); plain.close()


def test_fused_runs_whose_levels_fill_the_workgroup(dev):
    """what the barrier of the fused kernel is for: consecutive coupled levels of 65 .. 256 rows, every wavefront of the workgroup
    reading what the others wrote one level earlier; a level of exactly 256 rows ends a run and the level of 257 behind it takes a
    launch of its own.  The restatement's bits, and the level-by-level plan's"""
    csr = sr.layered()
    n = csr[0].size - 1
    lev = sr.levels_ref(csr[0], csr[1])
    assert tuple(np.bincount(lev)) == sr.LAYERS
    b, x0 = sr.rhs(n)
    fused, plain = AbiCase(dev, csr, b), AbiCase(dev, csr, b, create_flags=1)
    assert fused.info() == (7, 3, 6) and plain.info() == (7, 7, 0)
    for sweep, zero, its, lits, omega, fshift in sr.short_grid():
        flag = sr.SWEEPS[sweep] | (sr.ZERO_INITIAL_GUESS if zero else 0)
        ref = reference("layered", csr, b, x0, omega, flag, fshift, its, lits)
        xf, xp = fused.apply(x0, omega, flag, fshift, its * lits), plain.apply(x0, omega, flag, fshift, its * lits)
        assert np.array_equal(bits(xf), bits(ref)) and np.array_equal(bits(xp), bits(ref)), (sweep, zero, its, lits, omega, fshift)
    fused.close(); plain.close()


def test_fused_runs_on_a_20_cubed_grid(dev):
    """P7 20 x 20 x 20: 58 levels of 1 .. 300 rows; the 22 at either end (up to 244 rows) run fused, the 14 in the middle one by one"""
    csr = sr.perturbed(orc.gen_p7(20, 20, 20))
    n = csr[0].size - 1
    b, x0 = sr.rhs(n)
    fused, plain = AbiCase(dev, csr, b), AbiCase(dev, csr, b, create_flags=1)
    assert fused.info() == (58, 16, 44) and plain.info() == (58, 58, 0)
    for flag, omega, its in ((sr.SYMMETRIC | sr.ZERO_INITIAL_GUESS, 1.0, 1), (sr.SYMMETRIC, 1.3, 2), (sr.FORWARD, 1.3, 1), (sr.BACKWARD | sr.ZERO_INITIAL_GUESS, 1.0, 2)):
        ref = sr.sor_ref(csr[0], csr[1], csr[2], b, x0, omega, flag, 0.0, its, 1)
        xf, xp = fused.apply(x0, omega, flag, 0.0, its), plain.apply(x0, omega, flag, 0.0, its)
        assert np.array_equal(bits(xf), bits(ref)) and np.array_equal(bits(xp), bits(ref)), (flag, omega, its)
    fused.close(); plain.close()


def test_single_sweeps_and_argument_checks(dev):
    csr = sr.p7_small()
    n = csr[0].size - 1
    b, x0 = sr.rhs(n)
    c = AbiCase(dev, csr, b)
    k = dev.k
    dev.chk(k.mi355x_sor_idiag(dev.h, c.plan, c.d_aa, 1.3, 0.0, c.idiag.p, c.mdiag.p))
    mdiag, idiag = sr.inverted_diagonal(csr[0], csr[1], csr[2], 1.3, 0.0)
    assert np.array_equal(bits(c.idiag.get()), bits(idiag)) and np.array_equal(bits(c.mdiag.get()), bits(mdiag))
    for kind, flag in ((3, sr.FORWARD), (4, sr.BACKWARD), (1, sr.BACKWARD | sr.ZERO_INITIAL_GUESS), (0, sr.FORWARD | sr.ZERO_INITIAL_GUESS)):
        c.x.set(x0)
        dev.chk(k.mi355x_sor_sweep(dev.h, c.plan, kind, c.d_ai, c.d_aj, c.d_aa, c.idiag.p, c.mdiag.p, 1.3, c.b.p, c.t.p, c.x.p))
        assert np.array_equal(bits(c.x.get()), bits(sr.sor_ref(*csr, b, x0, 1.3, flag))), kind
    args = (c.d_ai, c.d_aj, c.d_aa, c.idiag.p, c.mdiag.p, 1.3)
    assert k.mi355x_sor_sweep(dev.h, c.plan, 9, *args, c.b.p, c.t.p, c.x.p) != 0
    assert k.mi355x_sor_sweep(dev.h, c.plan, 0, *args, c.b.p, None, c.x.p) != 0          # the zero-guess forward sweep writes t
    assert k.mi355x_sor_sweep(dev.h, c.plan, 3, *args, c.x.p, c.t.p, c.x.p) != 0          # b is x
    assert k.mi355x_sor_apply(dev.h, c.plan, *args, sr.EISENSTAT | 3, 1, c.b.p, c.t.p, c.x.p) != 0
    assert k.mi355x_sor_apply(dev.h, c.plan, *args, 3, 0, c.b.p, c.t.p, c.x.p) != 0
    c.close()
    # what the plan refuses: a row without a diagonal entry, unsorted columns, a column out of range
    plan, bad = C.c_void_p(), C.c_int()
    for ai, aj, row in (([0, 1, 2], [0, 0], 1), ([0, 2, 3], [1, 0, 1], 0), ([0, 2, 3], [0, 2, 1], 0)):
        ai, aj = np.array(ai, np.int32), np.array(aj, np.int32)
        assert k.mi355x_sor_plan_create(dev.h, 2, ai.ctypes.data, aj.ctypes.data, 0, C.byref(plan), C.byref(bad)) != 0
        assert bad.value == row and not plan.value


def test_ieee_specials(dev):
    """a NaN, a +Inf and a -0.0 in b and an Inf in one off-diagonal value: the restatement's bits, also where (1 - omega) x is 0 * x.
    A NaN must be a NaN at the same place; the sign and payload of a NaN that an operation produces are the processor's (the host's
    0 * Inf is the negative quiet NaN, the device's the positive one) and are not compared"""
    ai, aj, aa = sr.p7_small()
    n = ai.size - 1
    b, x0 = sr.rhs(n)
    b = b.copy(); b[3] = np.nan; b[17] = np.inf; b[40] = -0.0
    aa = aa.copy()
    k_off = int(ai[25]) if aj[ai[25]] != 25 else int(ai[25]) + 1
    aa[k_off] = np.inf
    x0 = x0.copy(); x0[11] = np.inf
    for flags in (0, 1):
        c = AbiCase(dev, (ai, aj, aa), b, create_flags=flags)
        for omega, fshift in ((1.0, 0.0), (1.3, 0.0)):
            for flag in (sr.SYMMETRIC | sr.ZERO_INITIAL_GUESS, sr.SYMMETRIC, sr.FORWARD, sr.BACKWARD | sr.ZERO_INITIAL_GUESS):
                x = c.apply(x0, omega, flag, fshift, 2)
                ref = sr.sor_ref(ai, aj, aa, b, x0, omega, flag, fshift, 2, 1)
                assert np.array_equal(np.isnan(x), np.isnan(ref)) and np.isnan(ref).any()
                ok = ~np.isnan(ref)
                assert np.array_equal(bits(x[ok]), bits(ref[ok])), (omega, flag, flags)
        c.close()


# ---------------------------------------------------------------------------------------------------- through the Mat type
def mat_sor(P, A, b, x0, **kw):
    vb, vx = V(P, b), V(P, x0)
    A.sor(vb, vx, **kw)
    return vx.array()


@pytest.mark.parametrize("name", ["p7_5x4x3", "nonsym200", "wide_then_chain"])
def test_device_route_equals_host_route_and_the_restatement(P, name):
    L = P.lib()
    csr = ABI_MATRICES[name]()
    b, x0 = sr.rhs(csr[0].size - 1)
    set_options(L, "")
    A = P.Mat.from_csr(*csr)
    set_options(L, "-mat_hipmi355x_sor host")
    H = P.Mat.from_csr(*csr)
    L.MatSetFromOptions(H.h)
    set_options(L, "")
    for sweep, zero, its, lits, omega, fshift in sr.grid():
        flag = sr.SWEEPS[sweep] | (sr.ZERO_INITIAL_GUESS if zero else 0)
        kw = dict(omega=omega, flag=flag, shift=fshift, its=its, lits=lits)
        ref = reference(name, csr, b, x0, omega, flag, fshift, its, lits)
        xd, xh = mat_sor(P, A, b, x0, **kw), mat_sor(P, H, b, x0, **kw)
        assert np.array_equal(bits(xd), bits(ref)) and np.array_equal(bits(xh), bits(ref)), (name, sweep, zero, its, lits, omega, fshift)
    assert A.sor_info()[3] == 1 and A.sor_info()[4] == 108 and H.sor_info()[3:] == (0, 0)


def test_what_a_call_builds(P):
    L = P.lib()
    set_options(L, "")
    ai, aj, aa = sr.perturbed(orc.gen_p7(6, 5, 4))
    n = ai.size - 1
    b, x0 = sr.rhs(n)
    A = P.Mat.from_csr(ai, aj, aa)
    A.set_option(P.MAT_KEEP_NONZERO_PATTERN, True)
    flag = sr.SYMMETRIC
    assert np.array_equal(bits(mat_sor(P, A, b, x0, flag=flag)), bits(sr.sor_ref(ai, aj, aa, b, x0, 1.0, flag)))
    levels, launches, idiag_builds, plan_builds, applied = A.sor_info()
    assert (idiag_builds, plan_builds, applied) == (1, 1, 1) and levels == 6 + 5 + 4 - 2 and launches == 1
    mat_sor(P, A, b, x0, flag=flag)
    assert A.sor_info()[2:] == (1, 1, 2), "a second call with the same parameters builds nothing"
    mat_sor(P, A, b, x0, flag=flag, omega=1.2)
    assert A.sor_info()[2:] == (2, 1, 3)
    # value changes on the device copy: the diagonal once more, the plan stays
    cur, builds = aa.copy(), 2
    L.MatScale(A.h, 0.5); cur = 0.5 * cur
    for step in ("scale", "shift", "zero_rows_columns"):
        if step == "shift":
            A.shift(0.75); cur = cur.copy(); cur[aj == np.repeat(np.arange(n), np.diff(ai))] += 0.75
        if step == "zero_rows_columns":
            from test_mat_zero_rows_cpu import ref_zero_rows_columns
            A.zero_rows_columns([3, 50, 51], 2.0)
            cur, _ = ref_zero_rows_columns(ai, aj, cur, [3, 50, 51], 2.0)
        builds += 1
        assert np.array_equal(bits(mat_sor(P, A, b, x0, flag=flag, omega=1.2)), bits(sr.sor_ref(ai, aj, cur, b, x0, 1.2, flag))), step
        assert A.sor_info()[2:4] == (builds, 1), step
    up = C.c_int()
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(up))
    assert up.value == 1, "the values never travelled again"
    # a pattern change: MatZeroRows without the keep option
    from test_mat_zero_rows_cpu import ref_zero_rows_new_pattern
    A.set_option(P.MAT_KEEP_NONZERO_PATTERN, False)
    A.zero_rows([7, 8], 1.5)
    ni, nj, na = ref_zero_rows_new_pattern(ai, aj, cur, [7, 8], 1.5)
    assert np.array_equal(bits(mat_sor(P, A, b, x0, flag=flag, omega=1.2)), bits(sr.sor_ref(ni, nj, na, b, x0, 1.2, flag)))
    assert A.sor_info()[2:4] == (builds + 1, 2)


def test_compressed_row_request(P):
    """a compressed-row form holds rows without entries, hence without a diagonal: MatSOR leaves the device alone and the host route
    answers with the missing row, x untouched; a matrix that asks for the form and has no empty row is not given it and runs on the device"""
    L = P.lib()
    set_options(L, "")
    plug = C.CDLL(__import__("petsc_dev_amd").host_lib_path())
    plug.MatSeqAIJHIPSetCompressedRow.argtypes = [C.c_void_p, C.c_int]
    n = 200
    b, x0 = sr.rhs(n)
    ai, aj, aa = sr.from_rows([{i: 2.0 + 0.01 * i} for i in range(n)])
    A = P.Mat.from_csr(ai, aj, aa)
    assert plug.MatSeqAIJHIPSetCompressedRow(A.h, 1) == 0
    assert np.array_equal(bits(mat_sor(P, A, b, x0)), bits(sr.sor_ref(ai, aj, aa, b, x0)))
    assert A.sor_info()[4] == 1
    ei, ej, ea = sr.from_rows([({i: 2.0} if i % 4 == 0 else {}) for i in range(n)])
    E = P.Mat.from_csr(ei, ej, ea)
    assert plug.MatSeqAIJHIPSetCompressedRow(E.h, 1) == 0
    vb, vx = V(P, b), V(P, x0)
    E.mult(vb, vx)                                          # the compressed-row form is on the device now
    vx.set_array(x0)
    with pytest.raises(P.PetscError) as e:
        E.sor(vb, vx)
    assert e.value.code == 73 and "row 1" in str(e.value) and E.sor_info()[3:] == (0, 0)
    assert np.array_equal(bits(vx.array()), bits(x0))


# ---------------------------------------------------------------------------------------------------- whole solves
def solve(P, csr, b, opts, **tol):
    L = P.lib()
    A = P.Mat.from_csr(*csr)
    vb, vx = V(P, b), V(P, np.zeros(b.size))
    k = P.KSP(comm=L.COMM_SELF)
    k.set_operators(A)
    set_options(L, opts)
    if tol:
        k.set_tolerances(**tol)
    k.set_from_options()
    k.record_history()
    k.solve(vb, vx)
    set_options(L, "")
    return vx.array(), k.history(), k.its, k.reason


SOLVES = [("p7", "-ksp_type cg -pc_type sor"), ("p7", "-ksp_type gmres -ksp_gmres_restart 30 -pc_type sor -pc_sor_omega 1.2"),
          ("p7", "-ksp_type bcgs -pc_type sor -pc_sor_its 2"), ("p7", "-ksp_type gmres -pc_type bjacobi -pc_bjacobi_blocks 3 -sub_pc_type sor"),
          ("nonsym", "-ksp_type gmres -ksp_gmres_restart 30 -pc_type sor -pc_sor_omega 1.2"), ("nonsym", "-ksp_type bcgs -pc_type sor -pc_sor_its 2"),
          ("nonsym", "-ksp_type gmres -pc_type bjacobi -pc_bjacobi_blocks 3 -sub_pc_type sor")]


@pytest.mark.parametrize("which,opts", SOLVES)
def test_whole_solves_agree_between_the_routes(P, which, opts):
    csr = orc.gen_p7(6, 5, 4) if which == "p7" else sr.nonsym200(dominant=True)      # (symmetric values: CG's operator)
    n = csr[0].size - 1
    b = orc.spmv(csr[0], csr[1], csr[2], np.cos(0.1 * np.arange(n)))
    xd, hd, itd, rd = solve(P, csr, b, opts, rtol=1e-10)
    xh, hh, ith, rh = solve(P, csr, b, opts + " -mat_hipmi355x_sor host", rtol=1e-10)
    assert rd > 0 and (itd, rd) == (ith, rh) and itd >= 2
    assert np.array_equal(bits(hd), bits(hh)) and np.array_equal(bits(xd), bits(xh))
    assert np.linalg.norm(xd - np.cos(0.1 * np.arange(n))) <= 1e-7 * np.sqrt(n)


@pytest.mark.parametrize("opts,kw", [("", dict(omega=1.0, its=1)), ("-pc_sor_omega 1.3 -pc_sor_its 2", dict(omega=1.3, its=2))])
def test_cg_sor_walks_the_python_pcg_bit_for_bit(P, opts, kw):
    """-ksp_type cg -pc_type sor on P7 6 x 5 x 4, device route and host route: every residual norm, the iteration count, the reason and
    the solution equal a Python PCG whose preconditioner is sor_ref (PCApply_SOR: the local symmetric sweep from a zero guess), with the
    reductions in the device summation order"""
    ai, aj, aa = orc.gen_p7(6, 5, 4)
    n = ai.size - 1
    b = np.cos(0.37 * np.arange(n)) + 0.1

    def precondition(r):
        return sr.sor_ref(ai, aj, aa, r, np.zeros(n), kw["omega"], sr.LOCAL_SYMMETRIC | sr.ZERO_INITIAL_GUESS, 0.0, kw["its"], 1)

    with orc.device_reduction_order():
        xo, ho, ito, ro = sr.python_pcg(ai, aj, aa, b, 1e-10, precondition)
    assert ro == 2 and ito >= 5
    for route in ("", " -mat_hipmi355x_sor host"):
        x, h, its, reason = solve(P, (ai, aj, aa), b, "-ksp_type cg -pc_type sor " + opts + route, rtol=1e-10)
        assert (its, reason) == (ito, ro), route
        assert np.array_equal(bits(h), bits(ho)), (route, np.max(np.abs(h - ho) / ho))
        assert np.array_equal(bits(x), bits(xo)), route


def test_preonly_sor_is_one_application(P):
    csr = orc.gen_p7(6, 5, 4)
    n = csr[0].size - 1
    b, _ = sr.rhs(n)
    x, _, _, _ = solve(P, csr, b, "-ksp_type preonly -pc_type sor -pc_sor_omega 1.3 -pc_sor_its 2")
    ref = sr.sor_ref(csr[0], csr[1], csr[2], b, np.zeros(n), 1.3, sr.LOCAL_SYMMETRIC | sr.ZERO_INITIAL_GUESS, 0.0, 2, 1)
    assert np.array_equal(bits(x), bits(ref))
