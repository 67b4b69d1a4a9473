"""PCMG and MatResidual on the device.

1. Mat.residual carries the bits of mult + aypx on both settings of -mat_hipmi355x_residual, the counters say which route ran, the
   bits follow MatScale / MatShift on the device copy, a column-tiled, a compressed-row and a BAIJ matrix take the calls, the option
   under the matrix's own prefix beats the global one.
2. PC.apply equals, bit for bit, the same cycle written here from KSPSolve on separately built, identically configured level solvers
   plus MatMult, VecAYPX, MatMultTranspose[Add], MatMultAdd, VecSet (class Cycle below): every cycle kind, 2 to 4 levels, three
   problems, Galerkin and user-set operators, each way of giving the transfers, a second up smoother, fused and calls residuals.
3. Against the numpy model (mg_ref) with Richardson(2/3) + Jacobi smoothers and the exact coarse factor: within 1e-10 of max |y| (each
   entry sees fewer than about 200 roundings through maps of norm O(1): five digits above rounding, far below any wrong coefficient).
4. cghipmi355x + mg reaches rtol 1e-8 in the model's count +-1 on 15^2, 31^2, 63^2; Jacobi needs at least four times as many at 31^2.
5. A repeated set-up reuses the Galerkin products; the refusals; the -pc_mg_* options; destruction in either order returns the counts
   of live and of watched factors (host/ilu.c) to what they were."""
import ctypes as C

import numpy as np
import pytest

import mg_ref as mr
from test_kernels_gpu import assert_bitexact, dev  # noqa: F401 (dev: fixture, makes sure a device is there)

pytestmark = pytest.mark.gpu
PETSC_ERR_SUP, PETSC_ERR_ORDER, PETSC_ERR_ARG_SIZ, PETSC_ERR_ARG_IDN = 56, 58, 60, 61


@pytest.fixture(scope="module")
def P(built, dev):  # noqa: F811
    from petsc_dev_amd import petsc
    petsc.lib()
    return petsc


class options:
    def __init__(self, P, text):
        self.P, self.text = P, text

    def __enter__(self):
        if self.text:
            self.P.lib().PetscOptionsInsertString(self.text.encode())

    def __exit__(self, *a):
        self.P.lib().PetscOptionsClear()


def mat(P, M):
    M = np.asarray(M)
    return P.Mat.from_csr(*mr.to_csr(M), ncols=M.shape[1])


# ------------------------------------------------------------------------------------------------ 1. the matrix's own residual
def residual_both_ways(P, A, n, m, seed=0):
    rng = np.random.default_rng(seed)
    x, b = P.Vec.from_array(rng.standard_normal(n)), P.Vec.from_array(rng.standard_normal(m))
    r, w = b.duplicate(), b.duplicate()
    A.mult(x, w)
    P.lib().VecAYPX(w.h, -1.0, b.h)
    A.residual(b, x, r)
    return r.array(), w.array()


def test_residual_routes_counters_and_value_updates(P):
    L = P.lib()
    M = mr.laplace2d(9) + np.diag(np.arange(81) * 0.01)
    for route, want in (("fused", (1, 0)), ("calls", (0, 1))):
        with options(P, "-mat_hipmi355x_residual " + route):
            A = mat(P, M)
            assert A.residual_counts() == (0, 0)
            got, ref = residual_both_ways(P, A, 81, 81)
            assert_bitexact(got, ref)
            assert A.residual_counts() == want, route
            L.MatScale(A.h, 1.7)                                        # on the device copy: the residual follows
            A.shift(0.3)
            got, ref = residual_both_ways(P, A, 81, 81, 1)
            assert_bitexact(got, ref)
            host = (1.7 * M + 0.3 * np.eye(81))
            rng = np.random.default_rng(1)
            x, b = rng.standard_normal(81), rng.standard_normal(81)
            assert np.abs(got - (b - host @ x)).max() <= 1e-13 * (np.abs(b).max() + np.abs(host).sum(axis=1).max() * np.abs(x).max())
            assert A.residual_counts() == tuple(2 * c for c in want)
    with options(P, "-mat_hipmi355x_residual sometimes"):
        A = mat(P, M)
        x, b = P.Vec.from_array(np.ones(81)), P.Vec.from_array(np.ones(81))
        with pytest.raises(P.PetscError):
            A.residual(b, x, b.duplicate())
    A = mat(P, M)
    x, b = P.Vec.from_array(np.ones(81)), P.Vec.from_array(np.ones(81))
    for r in (b, x):
        with pytest.raises(P.PetscError) as e:
            A.residual(b, x, r)
        assert e.value.code == PETSC_ERR_ARG_IDN


def test_rectangular_tiled_and_block_matrices(P):
    rng = np.random.default_rng(3)
    R = mr.interp1d(15).T                                               # 15 x 31
    with options(P, "-mat_hipmi355x_residual fused"):
        A = mat(P, R)
        got, ref = residual_both_ways(P, A, 31, 15)
        assert_bitexact(got, ref)
        assert A.residual_counts() == (1, 0)
    with options(P, "-mat_hipmi355x_residual fused -mat_hipmi355x_tiled 1 -mat_hipmi355x_tiled_stage_min 1 -mat_hipmi355x_index_compression 0"):
        D = rng.standard_normal((96, 96)) * (rng.random((96, 96)) < 0.3)
        A = mat(P, D)
        got, ref = residual_both_ways(P, A, 96, 96)
        assert_bitexact(got, ref)
        staged, rest = C.c_int(), C.c_int()
        P.lib().MatHIPMI355XGetTiledInfo(A.h, C.byref(staged), C.byref(rest))
        assert staged.value > 0                                         # the column-tiled product is the one in force
        assert A.residual_counts() == (0, 1)                            # it has no residual epilogue: the calls, though fused was asked for
        bs, nb = 2, 6
        ai = np.arange(nb + 1, dtype=np.int32) * 2
        aj = np.array([[i, (i + 1) % nb] if i + 1 < nb else [0, i] for i in range(nb)], dtype=np.int32).ravel()
        B = P.Mat.from_bsr(bs, ai, aj, rng.standard_normal(aj.size * bs * bs))
        got, ref = residual_both_ways(P, B, nb * bs, nb * bs)
        assert_bitexact(got, ref)
        assert B.residual_counts() == (0, 0)                            # the block type composes nothing: MatResidual's two calls


def test_compressed_row_matrix_takes_the_calls_and_the_matrix_prefix_beats_the_global_option(P):
    L = P.lib()
    plug = C.CDLL(__import__("petsc_dev_amd").host_lib_path())
    plug.MatSeqAIJHIPSetCompressedRow.argtypes = [C.c_void_p, C.c_int]
    n = 200
    E = np.zeros((n, n))
    E[::4, :] = np.where(np.random.default_rng(5).random((n // 4, n)) < 0.1, 1.5, 0.0)
    E[::4, 0] = 2.0                                                     # three rows in four are empty: the compressed-row form is taken
    with options(P, "-mat_hipmi355x_residual fused"):
        A = mat(P, E)
        assert plug.MatSeqAIJHIPSetCompressedRow(A.h, 1) == 0
        got, ref = residual_both_ways(P, A, n, n)
        assert_bitexact(got, ref)
        empty = np.flatnonzero(np.arange(n) % 4)
        rng = np.random.default_rng(0)
        rng.standard_normal(n)
        assert_bitexact(got[empty], rng.standard_normal(n)[empty])      # the rows that form leaves out are written all the same: b - 0.0
        assert A.residual_counts() == (0, 1)                            # the kernel would answer 801: the plug-in never asks it
    M = mr.laplace2d(9)
    with options(P, "-mat_hipmi355x_residual calls -own_mat_hipmi355x_residual fused"):
        A = mat(P, M)
        L.MatSetOptionsPrefix(A.h, b"own_")
        L.MatSetFromOptions(A.h)
        got, ref = residual_both_ways(P, A, 81, 81)
        assert_bitexact(got, ref)
        assert A.residual_counts() == (1, 0)                            # the matrix's own prefix wins over the global "calls"
        L.PetscOptionsClear()
        L.PetscOptionsInsertString(b"-own_mat_hipmi355x_residual calls")
        L.MatSetFromOptions(A.h)                                        # read again at any time; the global table is read with the device copy only
        got, ref = residual_both_ways(P, A, 81, 81, 1)
        assert_bitexact(got, ref)
        assert A.residual_counts() == (1, 1)
    with options(P, "-mat_hipmi355x_residual calls"):
        B = mat(P, M)
        residual_both_ways(P, B, 81, 81)
        assert B.residual_counts() == (0, 1)
        L.PetscOptionsClear()                                           # the global answer was taken when the device copy was built
        residual_both_ways(P, B, 81, 81)
        assert B.residual_counts() == (0, 2)


def test_transfer_helpers_choose_the_direction_from_the_sizes(P):
    Pd = mr.interp1d(7)
    Pm = mat(P, Pd)
    rng = np.random.default_rng(4)
    xf, xc = rng.standard_normal(15), rng.standard_normal(7)
    vf, vc = P.Vec.from_array(xf), P.Vec.from_array(xc)
    of, oc, t = vf.duplicate(), vc.duplicate(), vc.duplicate()
    Pm.restrict(vf, oc)
    P.lib().MatMultTranspose(Pm.h, vf.h, t.h)
    assert_bitexact(oc.array(), t.array())
    Pm.interpolate(vc, of)
    assert np.abs(of.array() - Pd @ xc).max() < 1e-14
    Pm.interpolate_add(vc, vf, vf)
    assert np.abs(vf.array() - (xf + Pd @ xc)).max() < 1e-14
    for call in (lambda: Pm.restrict(vc, vc.duplicate()), lambda: Pm.interpolate(vf, vf.duplicate()), lambda: Pm.interpolate_add(vc, vc, vf)):
        with pytest.raises(P.PetscError) as e:
            call()
        assert e.value.code == PETSC_ERR_ARG_SIZ


# ------------------------------------------------------------------------------------------------ 2. the cycle, written out
def configure(P, ksp, level, smoother, its):
    """one level solver; the same call configures the PC's own solver and the mirror's"""
    L = P.lib()
    if level == 0:
        ksp.set_type("preonly")
        ksp.set_initial_guess_nonzero(False)
        if smoother == "jacobi":                                        # the exact coarse factor: ILU with enough levels of fill
            ksp.set_pc_type("ilu")
            L.PCFactorSetLevels(ksp.get_pc().h, 64)
        return
    ksp.set_type("richardson")
    ksp.set_norm_type("none")
    ksp.set_tolerances(max_it=its)
    ksp.set_initial_guess_nonzero(True)
    if smoother == "jacobi":
        ksp.set_pc_type("jacobi")
        ksp.set_richardson_scale(2.0 / 3.0)
    else:
        ksp.set_pc_type("sor")


class Cycle:
    """the sequence of harness/mg.c from public calls on level solvers of its own"""
    def __init__(self, P, As, T, smoother, down, up, kind, cycle, cycles):
        self.P, self.L, self.n = P, P.lib(), len(As)
        self.A, self.T, self.kind, self.cycle, self.cycles = As, T, kind, cycle, cycles
        self.kd, self.ku, self.b, self.x, self.r = [], [], [], [], []
        for l, A in enumerate(As):
            kd = P.KSP(comm=self.L.COMM_SELF)
            configure(P, kd, l, smoother, down)
            kd.set_operators(A)
            ku = kd
            if l and up != down:
                ku = P.KSP(comm=self.L.COMM_SELF)
                configure(P, ku, l, smoother, up)
                ku.set_operators(A)
            self.kd.append(kd); self.ku.append(ku)
            x, b = A.get_vecs()
            self.x.append(x); self.b.append(b); self.r.append(b.duplicate())

    def restrict(self, l, src, dst):
        M = self.T[l][1]
        (self.L.MatMult if M.local_size()[0] == dst.n else self.L.MatMultTranspose)(M.h, src.h, dst.h)

    def interpolate(self, l, src, dst, add):
        M = self.T[l][0]
        fwd = M.local_size()[0] == dst.n
        if add:
            (self.L.MatMultAdd if fwd else self.L.MatMultTransposeAdd)(M.h, src.h, dst.h, dst.h)
        else:
            (self.L.MatMult if fwd else self.L.MatMultTranspose)(M.h, src.h, dst.h)

    def mcycle(self, l):
        L = self.L
        self.kd[l].solve(self.b[l], self.x[l])
        if l == 0:
            return
        L.MatMult(self.A[l].h, self.x[l].h, self.r[l].h)
        L.VecAYPX(self.r[l].h, -1.0, self.b[l].h)
        self.restrict(l, self.r[l], self.b[l - 1])
        L.VecSet(self.x[l - 1].h, 0.0)
        for _ in range(1 if (l - 1 == 0 or self.cycle == "v") else 2):
            self.mcycle(l - 1)
        self.interpolate(l, self.x[l - 1], self.x[l], True)
        self.ku[l].solve(self.b[l], self.x[l])

    def apply(self, rhs, y):
        L, n = self.L, self.n
        L.VecCopy(rhs.h, self.b[n - 1].h)
        if self.kind == "multiplicative":
            L.VecSet(self.x[n - 1].h, 0.0)
            for _ in range(self.cycles):
                self.mcycle(n - 1)
        else:
            for l in range(n - 1, 0, -1):
                self.restrict(l, self.b[l], self.b[l - 1])
            if self.kind == "additive":
                for l in range(n):
                    L.VecSet(self.x[l].h, 0.0)
                    self.kd[l].solve(self.b[l], self.x[l])
                for l in range(1, n):
                    self.interpolate(l, self.x[l - 1], self.x[l], True)
            else:
                L.VecSet(self.x[0].h, 0.0)
                self.kd[0].solve(self.b[0], self.x[0])
                for l in range(1, n):
                    self.interpolate(l, self.x[l - 1], self.x[l], False)
                    self.mcycle(l)
        L.VecCopy(self.x[n - 1].h, y.h)


PROBLEMS = {}


def problem(name, levels):
    """dense finest operator and interpolations [None, P_1 .. P_{n-1}], computed once"""
    key = (name, levels)
    if key not in PROBLEMS:
        if name == "1d":
            sizes = [31, 15, 7, 3][:levels][::-1]
            A, Ps = mr.laplace1d(31), [None] + [mr.interp1d(s) for s in sizes[:-1]]
        elif name == "2d":
            sizes = [15, 7, 3][:levels][::-1]
            A, Ps = mr.laplace2d(15), [None] + [mr.interp2d(s) for s in sizes[:-1]]
        else:
            sizes = [512, 64, 8, 2][:levels][::-1]
            A, Ps = mr.laplace3d(8), [None] + [mr.aggregation(f, f // c) for c, f in zip(sizes[:-1], sizes[1:])]
        PROBLEMS[key] = (A, Ps)
    return PROBLEMS[key]


def build(P, name, levels, kind="multiplicative", cycle="v", cycles=1, galerkin=True, transfers="interpolation", smoother="sor", down=1, up=1):
    """-> (ksp that owns the PCMG, its pc, the mirror Cycle, everything that has to stay alive)"""
    L = P.lib()
    Ad, Pd = problem(name, levels)
    A = mat(P, Ad)
    T = [None]
    for l in range(1, levels):
        Pm = mat(P, Pd[l])
        if transfers == "interpolation":
            T.append((Pm, Pm))
        elif transfers == "both":
            T.append((Pm, mat(P, Pd[l].T)))
        else:                                                           # restriction alone, stored coarse x fine
            Rm = mat(P, Pd[l].T)
            T.append((Rm, Rm))
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_type("preonly")
    ksp.set_pc_type("mg")
    ksp.set_operators(A)
    pc = ksp.get_pc()
    pc.mg_set_levels(levels)
    pc.mg_set_type(kind); pc.mg_set_cycle_type(cycle); pc.mg_set_cycles(cycles)
    As = [None] * levels
    As[-1] = A
    if galerkin:
        pc.mg_set_galerkin(True)
        for l in range(levels - 1, 0, -1):
            As[l - 1] = As[l].ptap(T[l][0])
    else:
        Ds = mr.galerkin(Ad, Pd)
        for l in range(levels - 1):
            As[l] = mat(P, Ds[l])
    for l in range(levels):
        configure(P, pc.mg_get_smoother(l), l, smoother, down)
        if not galerkin and l < levels - 1:
            pc.mg_get_smoother(l).set_operators(As[l])
        if l:
            if transfers in ("interpolation", "both"):
                pc.mg_set_interpolation(l, T[l][0])
            if transfers in ("restriction", "both"):
                pc.mg_set_restriction(l, T[l][1])
    if up != down:
        pc.mg_set_number_smooth(up=up)                                  # unequal counts: every level gets a second smoother
        if smoother == "jacobi":                                        # (same type and PC type as the first; the damping is the caller's)
            for l in range(1, levels):
                configure(P, pc.mg_get_smoother_up(l), l, smoother, up)
    mirror = Cycle(P, As, T, smoother, down, up, kind, cycle, cycles)
    return ksp, pc, mirror, (A, T, As)


CASES = [
    ("1d", 2, dict()),
    ("1d", 3, dict(cycle="w", transfers="both", smoother="jacobi")),
    ("1d", 4, dict(cycles=2, galerkin=False, transfers="restriction")),
    ("1d", 4, dict(kind="full")),
    ("1d", 3, dict(kind="additive", galerkin=False, transfers="both")),
    ("2d", 3, dict(kind="additive")),
    ("2d", 2, dict(kind="full", galerkin=False, transfers="both", smoother="jacobi")),
    ("2d", 3, dict(cycle="w", down=1, up=2)),
    ("p7", 3, dict(down=2, up=1, smoother="jacobi")),
    ("p7", 4, dict(cycle="w", cycles=2)),
    ("p7", 2, dict(kind="full", galerkin=False)),
]


@pytest.mark.parametrize("route", ["fused", "calls"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_apply_is_the_cycle_written_out(P, case, route):
    name, levels, kw = CASES[case]
    with options(P, "-mat_hipmi355x_residual " + route):
        ksp, pc, mirror, keep = build(P, name, levels, **kw)
        n = keep[0].local_size()[0]
        rhs = P.Vec.from_array(np.sin(0.7 * np.arange(n)) + 0.25)
        y, z = rhs.duplicate(), rhs.duplicate()
        for _ in range(2):                                              # the second application starts from used level vectors
            pc.apply(rhs, y)
            mirror.apply(rhs, z)
            assert_bitexact(y.array(), z.array())
        assert np.isfinite(y.array()).all() and np.abs(y.array()).max() > 0
        if kw.get("kind", "multiplicative") != "additive" and levels > 1:
            f, c = keep[0].residual_counts()
            assert (f > 0 and c == 0) if route == "fused" else (f == 0 and c > 0), (f, c)   # (none of these matrices is tiled or blocked)
        if kw.get("up", 1) != kw.get("down", 1):
            assert pc.mg_get_smoother_up(levels - 1).h.value != pc.mg_get_smoother(levels - 1).h.value
        del ksp


# ------------------------------------------------------------------------------------------------ 3. the model
@pytest.mark.parametrize("kind,cycle", [("multiplicative", "v"), ("multiplicative", "w"), ("additive", "v"), ("full", "v")])
def test_apply_agrees_with_the_model(P, kind, cycle):
    ksp, pc, mirror, keep = build(P, "1d", 4, kind=kind, cycle=cycle, smoother="jacobi")
    Ad, Pd = problem("1d", 4)
    As = mr.galerkin(Ad, Pd)
    model = mr.MG(As, Pd, mr.jacobi_smoother(As), kind=kind, cycle=cycle)
    rhs = np.cos(0.4 * np.arange(31)) + 0.1
    v = P.Vec.from_array(rhs)
    y = v.duplicate()
    pc.apply(v, y)
    ref = model.apply(rhs)
    err = np.abs(y.array() - ref).max()
    print("%s %s: max error %.3g of max |y| %.3g" % (kind, cycle, err, np.abs(ref).max()))
    assert err <= 1e-10 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------------ 4. the solver
MODEL_COUNTS = {}


def model_counts(n):
    if n not in MODEL_COUNTS:
        sizes = [n]
        while sizes[-1] > 3:
            sizes.append((sizes[-1] - 1) // 2)
        Ps = [None] + [mr.interp2d(s) for s in sizes[::-1][:-1]]
        As = mr.galerkin(mr.laplace2d(n), Ps)
        b = np.sin(0.3 * np.arange(n * n)) + 0.5
        d = np.diag(As[-1])
        MODEL_COUNTS[n] = (mr.pcg(As[-1], b, mr.MG(As, Ps, mr.jacobi_smoother(As)).apply)[1], mr.pcg(As[-1], b, lambda r: r / d)[1], Ps, b)
    return MODEL_COUNTS[n]


@pytest.mark.parametrize("n", [15, 31, 63])
def test_cg_with_mg_converges_in_the_models_count(P, n):
    L = P.lib()
    mg_its, jac_its, Ps, b = model_counts(n)
    ai, aj, aa = mr.to_csr(mr.laplace2d(n)) if n < 63 else laplace2d_csr(n)
    A = P.Mat.from_csr(ai, aj, aa)
    Tm = [None] + [mat(P, Pl) for Pl in Ps[1:]]
    bv = P.Vec.from_array(b)

    def solve(pctype):
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_type("cghipmi355x")
        ksp.set_norm_type("unpreconditioned")
        ksp.set_tolerances(rtol=1e-8)
        ksp.set_pc_type(pctype)
        ksp.set_operators(A)
        if pctype == "mg":
            pc = ksp.get_pc()
            pc.mg_set_levels(len(Ps)); pc.mg_set_galerkin(True)
            for l in range(len(Ps)):
                configure(P, pc.mg_get_smoother(l), l, "jacobi", 1)
                if l:
                    pc.mg_set_interpolation(l, Tm[l])
        x = bv.duplicate()
        ksp.solve(bv, x)
        r = bv.duplicate()
        A.residual(bv, x, r)
        assert ksp.reason > 0 and r.norm() <= 2e-8 * bv.norm(), (pctype, ksp.reason, r.norm() / bv.norm())
        return ksp.its

    its = solve("mg")
    print("n = %d: cg + mg %d iterations (model %d)" % (n, its, mg_its))
    assert abs(its - mg_its) <= 1
    if n == 31:
        jac = solve("jacobi")
        print("n = 31: cg + jacobi %d iterations (model %d)" % (jac, jac_its))
        assert abs(jac - jac_its) <= 1 and jac >= 4 * its


def laplace2d_csr(n):
    ai, aj, aa = [0], [], []
    for i in range(n):
        for j in range(n):
            for di, dj, v in ((-1, 0, -1.0), (0, -1, -1.0), (0, 0, 4.0), (0, 1, -1.0), (1, 0, -1.0)):
                if 0 <= i + di < n and 0 <= j + dj < n:
                    aj.append((i + di) * n + j + dj); aa.append(v)
            ai.append(len(aj))
    return np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa)


# ------------------------------------------------------------------------------------------------ 5. set-up again, refusals, destruction
def test_repeated_set_up_reuses_the_products_and_level_options(P):
    L = P.lib()
    with options(P, "-mg_levels_ksp_max_it 3 -mg_levels_2_ksp_max_it 2"):
        ksp, pc, mirror, keep = build(P, "1d", 3, smoother="jacobi")
        A = keep[0]
        rhs = P.Vec.from_array(np.ones(31))
        y = rhs.duplicate()
        pc.apply(rhs, y)
        assert pc.mg_get_smoother(1).get_tolerances()[3] == 3 and pc.mg_get_smoother(2).get_tolerances()[3] == 2   # mg_levels_<l>_ beats mg_levels_
        first = y.array()
        coarse = []
        for l in (0, 1):
            a, p = C.c_void_p(), C.c_void_p()
            L.PCGetOperators(pc.mg_get_smoother(l).get_pc().h, C.byref(a), C.byref(p), None)
            coarse.append(P.Mat(handle=a, own=False))
        before = [m.product_counts() for m in coarse]
        assert all(c[0] == 1 for c in before)
        L.MatScale(A.h, 2.0)
        ksp.set_operators(A)
        pc.apply(rhs, y)                                                # sets up again
        after = [m.product_counts() for m in coarse]
        assert all(a[0] == 1 and a[1] + a[2] == b[1] + b[2] + 1 for a, b in zip(after, before)), (before, after)
        assert np.abs(2.0 * y.array() - first).max() <= 1e-13 * np.abs(first).max()     # B(2 A) = B(A) / 2
        with pytest.raises(P.PetscError) as e:
            pc.mg_set_levels(2)
        assert e.value.code == PETSC_ERR_ORDER


def test_refusals_that_need_a_device(P):
    L = P.lib()
    Ad, Pd = problem("1d", 2)
    # Galerkin with the transfer stored coarse x fine
    ksp = P.KSP(comm=L.COMM_SELF)
    ksp.set_pc_type("mg")
    A, Rm = mat(P, Ad), mat(P, Pd[1].T)
    ksp.set_operators(A)
    pc = ksp.get_pc()
    pc.mg_set_levels(2); pc.mg_set_galerkin(True); pc.mg_set_restriction(1, Rm)
    with pytest.raises(P.PetscError) as e:
        pc.set_up()
    assert e.value.code == PETSC_ERR_SUP
    # a matrix type whose MatPtAP refuses: the refusal is passed on
    nb = 8
    ai = np.arange(nb + 1, dtype=np.int32)
    B = P.Mat.from_bsr(2, ai, np.arange(nb, dtype=np.int32), np.tile(np.array([2.0, 0.0, 0.0, 2.0]), nb))
    k2 = P.KSP(comm=L.COMM_SELF)
    k2.set_pc_type("mg")
    k2.set_operators(B)
    p2 = k2.get_pc()
    Pm = mat(P, mr.aggregation(16, 2))
    p2.mg_set_levels(2); p2.mg_set_galerkin(True); p2.mg_set_interpolation(1, Pm)
    with pytest.raises(P.PetscError) as e:
        p2.set_up()
    assert e.value.code == PETSC_ERR_SUP


def test_the_pc_options_configure_what_the_calls_configure(P):
    """-pc_mg_levels, _galerkin, _smoothdown, _smoothup, _multiplicative_cycles, _cycle_type through PCSetFromOptions: the application
    equals the written-out cycle of the same settings, bit for bit; -pc_mg_type additive likewise"""
    L = P.lib()
    Ad, Pd = problem("2d", 3)
    for text, kw in (("-pc_mg_levels 3 -pc_mg_galerkin 1 -pc_mg_smoothdown 2 -pc_mg_smoothup 1 -pc_mg_multiplicative_cycles 2 -pc_mg_cycle_type w",
                      dict(kind="multiplicative", cycle="w", cycles=2, down=2, up=1)),
                     ("-pc_mg_levels 3 -pc_mg_galerkin 1 -pc_mg_type additive", dict(kind="additive", cycle="v", cycles=1, down=1, up=1))):
        with options(P, text):
            A = mat(P, Ad)
            T = [None] + [(Pm, Pm) for Pm in (mat(P, Pl) for Pl in Pd[1:])]
            ksp = P.KSP(comm=L.COMM_SELF)
            ksp.set_type("preonly")
            ksp.set_pc_type("mg")
            ksp.set_operators(A)
            pc = ksp.get_pc()
            pc.set_from_options()
            assert pc.mg_get_levels() == 3
            for l in (1, 2):
                pc.mg_set_interpolation(l, T[l][0])
            As = [None, None, A]
            for l in (2, 1):
                As[l - 1] = As[l].ptap(T[l][0])
            mirror = Cycle(P, As, T, "sor", kw["down"], kw["up"], kw["kind"], kw["cycle"], kw["cycles"])
            rhs = P.Vec.from_array(np.sin(0.7 * np.arange(225)) + 0.25)
            y, z = rhs.duplicate(), rhs.duplicate()
            pc.apply(rhs, y)
            mirror.apply(rhs, z)
            assert_bitexact(y.array(), z.array())
            assert np.abs(y.array()).max() > 0
            if kw["down"] != kw["up"]:
                assert pc.mg_get_smoother(2).get_tolerances()[3] == 2 and pc.mg_get_smoother_up(2).get_tolerances()[3] == 1
            del ksp


def live_factors(P):
    """(ILU / ICC factors alive in this process, those of them on the watch list of host/ilu.c)"""
    import gc
    gc.collect()
    live, watched = C.c_int(), C.c_int()
    P.lib().HIPMI355XGetLiveFactors(C.byref(live), C.byref(watched))
    return live.value, watched.value


@pytest.mark.parametrize("matrix_first", [True, False])
def test_destruction_in_either_order(P, matrix_first):
    """the coarse solver's ILU factor, forced to the sync-free solves so that it sits on the watch list of host/ilu.c, is released and
    taken off the list whichever of the KSP and its matrix goes first: the counts of live and of watched factors return to what they were"""
    L = P.lib()
    before = live_factors(P)
    with options(P, "-mg_coarse_pc_factor_hipmi355x_trisolve syncfree"):
        ksp, pc, mirror, keep = build(P, "1d", 3, smoother="jacobi")   # the coarse solver holds an ILU factor
        rhs = P.Vec.from_array(np.ones(31))
        y = rhs.duplicate()
        pc.apply(rhs, y)
    syncfree, aborted = C.c_int(), C.c_int()
    L.PCILUGetSolver_HIPMI355X(pc.mg_get_coarse_solve().get_pc().h, C.byref(syncfree), C.byref(aborted))
    assert (syncfree.value, aborted.value) == (1, 0)
    assert live_factors(P) == (before[0] + 1, before[1] + 1)            # (the mirror's solvers were never set up: the factor is the PC's)
    A, T, As = keep
    del mirror, pc
    if matrix_first:
        A.destroy(); A.own = False
        assert live_factors(P) == (before[0] + 1, before[1] + 1)        # the factor is the solver's, not the matrix's
        ksp.destroy(); ksp.own = False
    else:
        ksp.destroy(); ksp.own = False
        assert live_factors(P) == before
        A.destroy(); A.own = False
    assert live_factors(P) == before
    k3, p3, m3, keep3 = build(P, "1d", 2)                               # a later solve walks the watch list at its host waits
    p3.apply(rhs, y)
    assert np.isfinite(y.norm())
