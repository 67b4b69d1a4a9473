"""Matrix norms and row / column reductions on the device: the kernels of csrc/mat_reduce.hip through the C ABI against the model
(matred_ref.py) bit for bit -- row lengths around a wavefront and a workgroup, guard bands, poisoned surroundings, both alignments,
IEEE specials, the BCSR instances against the expanded matrix -- then the plug-in: device and host route agree, results follow
every device-side value update, the derived product forms change nothing, and the worked example of the README."""
import ctypes as C
import functools

import numpy as np
import pytest

import matred_ref as R
import orc
import problems as pb
import specials as S
from gpu import Dev

pytestmark = pytest.mark.gpu
bits = R.bits
GUARD = 64
LENS = (0, 1, 2, 63, 64, 65, 127, 129, 257)
NCOLS = 300


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.free_all()


def same(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


@functools.lru_cache(maxsize=None)
def shape(m, seed=0, specials=False):
    """m rows whose lengths walk LENS (starting at another place per m), columns ascending, values over seven decades"""
    rng = np.random.default_rng(100 + m + seed)
    lens = [LENS[(r + m) % len(LENS)] for r in range(m)]
    cols = [np.sort(rng.choice(NCOLS, size=ln, replace=False)) for ln in lens]
    ai = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    aj = (np.concatenate(cols) if ai[-1] else np.zeros(0)).astype(np.int32)
    aa = rng.standard_normal(int(ai[-1])) * 10.0 ** rng.integers(-3, 4, int(ai[-1]))
    if specials:   # NaN, +-Inf, -0.0, a denormal at the first, middle and last position of rows of every length
        vals = list(S.SPECIALS) + [-0.0, 4.9406564584124654e-324, -2.5e-310]
        q = 0
        for r in range(m):
            k0, k1 = int(ai[r]), int(ai[r + 1])
            if k1 > k0 and r % 2 == 0:
                pos = (k0, (k0 + k1) // 2, k1 - 1)[q % 3]
                aa[pos] = vals[(q // 3) % len(vals)]
                q += 1
    return ai, aj, aa


@functools.lru_cache(maxsize=None)
def model(m, seed=0, specials=False):
    """the reference of a shape, computed once: {op: values or (values, columns)}"""
    ai, aj, aa = shape(m, seed, specials)
    with np.errstate(all="ignore"):
        out = {op: R.row_sums(op, ai, aa) for op in (R.SUM, R.ABSSUM, R.SQSUM)}
        out.update({op: R.row_extrema(op, ai, aj, aa, NCOLS) for op in (R.MAXABS, R.MAX, R.MIN)})
    return out


def reduce_guarded(dev, op, mbs, bs, ncols, d_ai, d_aj, d_aa, with_idx=True, acc=None, rows=None, nout=None):
    """one call with guard bands around out (and idx): returns (values, columns or None); asserts the bands are intact"""
    n = mbs * bs if nout is None else nout
    sent = -7.25e77
    out = np.full(n + 2 * GUARD, sent)
    if acc is not None:
        out[GUARD:GUARD + n] = acc
    d_out = dev.put(out)
    idx = np.full(n + 2 * GUARD, -77, np.int32)
    d_idx = dev.put(idx) if (with_idx and op >= R.MAXABS) else None
    o = C.c_void_p(d_out.value + 8 * GUARD)
    dev.chk(dev.k.mi355x_mat_row_reduce(dev.h, op, mbs, bs, ncols, d_ai, d_aj, d_aa, rows, o if acc is not None else None, o,
                                        C.c_void_p(d_idx.value + 4 * GUARD) if d_idx else None))
    got = dev.get(d_out, n + 2 * GUARD)
    assert np.all(got[:GUARD] == sent) and np.all(got[GUARD + n:] == sent), "values written outside [0, m)"
    gi = None
    if d_idx:
        gi = dev.get(d_idx, n + 2 * GUARD, np.int32)
        assert np.all(gi[:GUARD] == -77) and np.all(gi[GUARD + n:] == -77), "columns written outside [0, m)"
        gi = gi[GUARD:GUARD + n]
        dev.free(d_idx)
    dev.free(d_out)
    return got[GUARD:GUARD + n], gi


def put_values(dev, aa, shift):
    """aa inside a NaN-filled buffer, `shift` doubles after a 16-byte boundary: what a pair load reads next to the array, and the idle
    lanes' re-reads, is poison that must not reach a result; shift 1 takes the scalar stream"""
    buf = np.full(aa.size + 8, np.nan)
    buf[2 + shift:2 + shift + aa.size] = aa
    p = dev.put(buf)
    return p, C.c_void_p(p.value + 8 * (2 + shift))


@pytest.mark.parametrize("specials", [False, True])
@pytest.mark.parametrize("m", [1, 2, 64, 65, 1000])
def test_kernels_equal_the_model(dev, m, specials):
    """every operation, with and without the column output, 16-byte aligned and not, guard bands and poisoned surroundings"""
    ai, aj, aa = shape(m, 0, specials)
    ref = model(m, 0, specials)
    d_ai, d_aj = dev.put(ai), dev.put(aj)
    for shift in (0, 1):
        base, d_aa = put_values(dev, aa, shift)
        for op in range(6):
            for with_idx in ((True, False) if op >= R.MAXABS else (False,)):
                v, i = reduce_guarded(dev, op, m, 1, NCOLS, d_ai, d_aj, d_aa, with_idx)
                rv = ref[op][0] if op >= R.MAXABS else ref[op]
                assert same(v, rv), (m, op, shift, np.flatnonzero(bits(v) != bits(rv))[:5])
                if i is not None:
                    assert np.array_equal(i, ref[op][1]), (m, op, shift, np.flatnonzero(i != ref[op][1])[:5])
        dev.free(base)
    if not specials:
        # the ADD form continues from an accumulator (in place), and the compressed-row form writes the listed rows only
        base, d_aa = put_values(dev, aa, 0)
        acc = np.cos(np.arange(m)) * 3.0
        v, _ = reduce_guarded(dev, R.ABSSUM, m, 1, NCOLS, d_ai, d_aj, d_aa, acc=acc)
        assert same(v, R.row_sums(R.ABSSUM, ai, aa, acc))
        rows = (2 * np.arange(m) + 1).astype(np.int32)
        keep = np.sin(np.arange(2 * m + 2)) - 2.0
        v, _ = reduce_guarded(dev, R.ABSSUM, m, 1, NCOLS, d_ai, d_aj, d_aa, acc=keep, rows=dev.put(rows), nout=2 * m + 2)
        exp = keep.copy(); exp[rows] = R.row_sums(R.ABSSUM, ai, aa, keep[rows])
        assert same(v, exp)
        dev.free(base)


def test_row_sums_are_the_product_with_ones(dev):
    """rows of at most 16 entries: the product sums every row on one lane, in storage order -- the bits of the row-sum instance"""
    rng = np.random.default_rng(77)
    m = 600
    lens = [(0, 1, 2, 7, 16)[r % 5] for r in range(m)]
    cols = [np.sort(rng.choice(NCOLS, size=ln, replace=False)) for ln in lens]
    ai = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    aj = np.concatenate(cols).astype(np.int32)
    aa = rng.standard_normal(aj.size) * 10.0 ** rng.integers(-8, 9, aj.size)
    assert S.one_lane_rows(ai, S.row_blocks(ai)[0]).all()
    d_ai, d_aj, d_aa = dev.put(ai), dev.put(np.concatenate((aj, [0, 0])).astype(np.int32)), dev.put(np.concatenate((aa, [0.0, 0.0])))
    ones = dev.put(np.ones(NCOLS)); d_y = dev.put(np.zeros(m)); plan = C.c_void_p()
    dev.chk(dev.k.mi355x_spmv_plan_create(dev.h, m, ai.ctypes.data_as(C.c_void_p), None, C.byref(plan)))
    dev.chk(dev.k.mi355x_spmv_csr(dev.h, plan, d_ai, d_aj, d_aa, ones, d_y))
    y = dev.get(d_y, m)
    dev.chk(dev.k.mi355x_spmv_plan_destroy(plan))
    v, _ = reduce_guarded(dev, R.SUM, m, 1, NCOLS, d_ai, d_aj, d_aa)
    assert np.array_equal(bits(v), bits(y)) and np.array_equal(bits(v), bits(R.row_sums(R.SUM, ai, aa)))


def test_compressed_row_plan_supplies_the_row_list(dev):
    """what the MPIAIJ infinity norm does with the off-diagonal block: the row list of a compressed-row plan (mi355x_spmv_plan_rows)
    as `rows`, the ADD form in place; rows the plan does not list keep their value"""
    ai, aj, aa = shape(65)
    m = 65
    rows = (3 * np.arange(m) + 1).astype(np.int32)
    plan, d_rows, nrows = C.c_void_p(), C.c_void_p(), C.c_int(-1)
    dev.chk(dev.k.mi355x_spmv_plan_create(dev.h, m, ai.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p), C.byref(plan)))
    dev.sync()
    dev.chk(dev.k.mi355x_spmv_plan_rows(plan, C.byref(d_rows), C.byref(nrows)))
    assert nrows.value == m and d_rows.value
    assert np.array_equal(dev.get(d_rows, m, np.int32), rows)
    keep = np.cos(np.arange(3 * m + 2)) + 2.0
    base, d_aa = put_values(dev, aa, 0)
    v, _ = reduce_guarded(dev, R.ABSSUM, m, 1, NCOLS, dev.put(ai), dev.put(aj), d_aa, acc=keep, rows=d_rows, nout=3 * m + 2)
    exp = keep.copy(); exp[rows] = R.row_sums(R.ABSSUM, ai, aa, keep[rows])
    assert same(v, exp)
    dev.chk(dev.k.mi355x_spmv_plan_destroy(plan))
    plain = C.c_void_p()
    dev.chk(dev.k.mi355x_spmv_plan_create(dev.h, m, ai.ctypes.data_as(C.c_void_p), None, C.byref(plain)))
    dev.chk(dev.k.mi355x_spmv_plan_rows(plain, C.byref(d_rows), C.byref(nrows)))
    assert not d_rows.value and nrows.value == m
    dev.chk(dev.k.mi355x_spmv_plan_destroy(plain))
    assert dev.k.mi355x_spmv_plan_rows(None, C.byref(d_rows), C.byref(nrows)) != 0


@pytest.mark.parametrize("bs", [2, 3, 4, 7])
def test_bcsr_instances_equal_the_expanded_matrix(dev, bs):
    """block rows of 0 .. 30 blocks and one of 90 (a point row of 630 entries at bs = 7; more block rows than one workgroup takes)"""
    rng = np.random.default_rng(40 + bs)
    mbs, nbs = 300, 120
    lens = rng.integers(0, 31, mbs); lens[5] = 0; lens[17] = 90; lens[mbs - 1] = 1
    cols = [np.sort(rng.choice(nbs, size=int(ln), replace=False)) for ln in lens]
    bi = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    bj = np.concatenate(cols).astype(np.int32)
    ba = rng.standard_normal(bj.size * bs * bs) * 10.0 ** rng.integers(-3, 4, bj.size * bs * bs)
    pai, paj, paa = S.bsr_to_csr(bs, bi, bj, ba)
    d_bi, d_bj = dev.put(bi), dev.put(bj)
    base, d_ba = put_values(dev, ba, 0)
    for op in range(6):
        v, i = reduce_guarded(dev, op, mbs, bs, nbs * bs, d_bi, d_bj, d_ba)
        if op >= R.MAXABS:
            rv, ri = R.row_extrema(op, pai, paj, paa, nbs * bs)
            assert np.array_equal(i, ri), (bs, op)
        else:
            rv = R.row_sums(op, pai, paa)
        assert np.array_equal(bits(v), bits(rv)), (bs, op, np.flatnonzero(bits(v) != bits(rv))[:5])
    dev.free(base)


# ---------------------------------------------------------------------------------------------------- through the plug-in
def queries(P, A, route):
    """every query of A on one route: a dict of arrays"""
    L = P.lib()
    L.PetscOptionsSetValue(b"-mat_hipmi355x_reductions", route)
    L.MatSetFromOptions(A.h)                            # the route is resolved once per matrix: read it again
    try:
        out = {"inf": np.array([A.norm(P.NORM_INFINITY)]), "one": np.array([A.norm(P.NORM_1)]), "fro": np.array([A.norm(P.NORM_FROBENIUS)])}
        for name, call in (("maxabs", A.row_max_abs), ("max", A.row_max), ("min", A.row_min)):
            v, idx = call()
            out[name] = v.array(); out[name + "_idx"] = idx.astype(np.float64)
        for name, kind in (("c1", P.NORM_1), ("c2", P.NORM_2), ("cinf", P.NORM_INFINITY)):
            out[name] = A.column_norms(kind)
    finally:
        L.PetscOptionsClear()
    return out


@functools.lru_cache(maxsize=None)
def _norm_dev():
    return Dev()


def device_square_sum(stored):
    """mi355x_vec_norm (type 2: the sum of squares, before the root) of a value array on the device"""
    if not stored.size:
        return 0.0
    d = _norm_dev()
    p = d.put(stored)
    d.chk(d.k.mi355x_vec_norm(d.h, stored.size, 2, p, d.host_scratch()))
    out = float(d.scalar_out(1)[0])
    d.free(p)
    return out


def check_routes(P, A, what, point_csr=None, stored=None):
    """device == host bit for bit (Frobenius: within the summation bound), and both equal the model on the matrix's host copy"""
    dv, hv = queries(P, A, b"device"), queries(P, A, b"host")
    ai, aj, aa = point_csr if point_csr is not None else A.csr()
    stored = aa if stored is None else stored
    n = A.local_size()[1]
    for k in dv:
        if k != "fro":
            assert same(dv[k], hv[k]), (what, k)
    ss = R.sum_squares(stored)
    pre = device_square_sum(stored)                      # the device sum before the root: VecNorm's tree over the value array
    assert abs(pre - ss) <= R.sum_bound(stored.size, ss), (what, pre, ss)
    assert bits(dv["fro"])[0] == bits(np.sqrt(np.array([pre])))[0], (what, dv["fro"], pre)
    assert hv["fro"][0] == np.sqrt(ss)
    assert dv["inf"][0] == R.norm_inf(ai, aa) and dv["one"][0] == R.norm_1(ai, aj, aa, n), what
    for name, op in (("maxabs", R.MAXABS), ("max", R.MAX), ("min", R.MIN)):
        rv, ri = R.row_extrema(op, ai, aj, aa, n)
        assert same(dv[name], rv) and np.array_equal(dv[name + "_idx"], ri), (what, name)
    for name, kind in (("c1", 0), ("c2", 1), ("cinf", 3)):
        assert same(dv[name], R.column_norms(kind, ai, aj, aa, n)), (what, name)
    return dv


def V(P, a):
    return P.Vec.from_array(a, comm=P.lib().COMM_SELF)


def test_routes_agree_and_follow_device_side_updates(P):
    """P7(6,5,4) and a rectangular 60 x 37 operator: used on the device first, then after each of MatShift, MatAXPY, MatDiagonalScale
    and MatZeroRows on the device copy"""
    L = P.lib()
    ai, aj, aa = orc.gen_p7(6, 5, 4)
    aa = aa * (1.0 + 0.3 * np.sin(np.arange(aa.size)))
    n = ai.size - 1
    A = P.Mat.from_csr(ai, aj, aa); Z = P.Mat.from_csr(ai, aj, np.cos(np.arange(aa.size)))
    A.set_option(P.MAT_KEEP_NONZERO_PATTERN)
    x, y = V(P, np.ones(n)), V(P, np.zeros(n))
    A.mult(x, y)
    check_routes(P, A, "p7 fresh")
    up = C.c_int(-1)
    vl, vr = V(P, 1.0 + 0.1 * np.cos(np.arange(n))), V(P, 2.0 - 0.1 * np.sin(np.arange(n)))
    before = A.csr()[2]
    for name, op in (("shift", lambda: A.shift(0.37)), ("axpy", lambda: A.axpy(-1.3, Z)), ("diagonalscale", lambda: L.MatDiagonalScale(A.h, vl.h, vr.h)),
                     ("zerorows", lambda: A.zero_rows([0, 7, n - 1], 2.5))):
        op()
        after = A.csr()[2]
        assert not np.array_equal(before, after), name          # the update did change the values
        before = after
        check_routes(P, A, "p7 after " + name)
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(up))
    assert up.value == 1, "an update went through an upload instead of the device copy"
    # rectangular: more rows than columns, a full row and an empty one
    rng = np.random.default_rng(9)
    cols = [np.sort(rng.choice(37, size=int(rng.integers(0, 12)), replace=False)) for _ in range(60)]
    cols[3] = np.arange(37); cols[11] = np.arange(0)
    ri = np.concatenate(([0], np.cumsum([c.size for c in cols]))).astype(np.int32)
    rj = np.concatenate(cols).astype(np.int32); ra = rng.standard_normal(rj.size)
    B = P.Mat.from_csr(ri, rj, ra, ncols=37)
    dv = check_routes(P, B, "60 x 37")
    # NORM_1(A) == NORM_INFINITY(A^T), A^T from MatTranspose; row sums: MatMult with ones
    Bt = B.transpose()
    L.PetscOptionsSetValue(b"-mat_hipmi355x_reductions", b"device")
    try:
        assert bits(np.array([Bt.norm(P.NORM_INFINITY)]))[0] == bits(dv["one"])[0] and bits(np.array([Bt.norm(P.NORM_1)]))[0] == bits(dv["inf"])[0]
    finally:
        L.PetscOptionsClear()


def test_setvaluesbatch_then_reductions(P):
    """a chain of two-node elements assembled by MatSetValuesBatch: first through MatSetValues, then on the device copy"""
    L = P.lib()
    nn, bs = 200, 2
    ne = nn - 1
    rows = np.stack([np.arange(ne), np.arange(ne) + 1], axis=1).astype(np.int32).ravel()
    A = P.Mat(); L.MatCreate(L.COMM_SELF, C.byref(A.h))
    L.MatSetSizes(A.h, nn, nn, nn, nn); L.MatSetType(A.h, b"seqaijhipmi355x"); L.MatSetUp(A.h)
    up = C.c_int(-1)
    for step in range(2):
        v = np.random.default_rng(50 + step).standard_normal(ne * bs * bs)
        if step:
            L.MatZeroEntries(A.h)
        L.MatSetValuesBatch(A.h, ne, bs, rows.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
        L.MatAssemblyBegin(A.h, 0); L.MatAssemblyEnd(A.h, 0)
        check_routes(P, A, "batch step %d" % step)
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(up))
    assert up.value == 1


def test_block_matrix_and_derived_forms(P, dev):
    """a three-dof block matrix as BAIJ and as AIJ through its blocked companion; the value-pattern, tiled and blocked forms switched
    on and off give the same bits; Frobenius is mi355x_vec_norm of the value array"""
    L = P.lib()
    (ai, aj, aa), _ = pb.elasticity_like(6, 5, 4)
    ai, aj = ai.astype(np.int32), aj.astype(np.int32)
    n = ai.size - 1
    x, y = V(P, np.ones(n)), V(P, np.zeros(n))
    got = {}
    for opts in ("-mat_hipmi355x_blocked 1", "-mat_hipmi355x_blocked 0", "-mat_hipmi355x_blocked 0 -mat_hipmi355x_tiled 1 -mat_hipmi355x_index_compression 0"):
        L.PetscOptionsInsertString(opts.encode())
        A = P.Mat.from_csr(ai, aj, aa)
        L.MatSetFromOptions(A.h)
        A.mult(x, y)                                    # the device copy and its product form exist before the queries
        if "blocked 1" in opts:
            b, nb = C.c_int(), C.c_int()
            L.MatHIPMI355XGetBlockedInfo(A.h, C.byref(b), C.byref(nb))
            assert b.value == 3
        L.PetscOptionsClear()
        got[opts] = check_routes(P, A, opts)
    first = got["-mat_hipmi355x_blocked 1"]
    for o, g in got.items():
        for k in g:
            assert same(g[k], first[k]), (o, k)
    # constant coefficients: the value-pattern dictionary multiplies, the reductions read the plain array
    ci, cj, ca = orc.gen_p7(8, 8, 8)
    for vp in (b"1", b"0"):
        L.PetscOptionsSetValue(b"-mat_hipmi355x_value_patterns", vp)
        Ac = P.Mat.from_csr(ci, cj, ca)
        xc, yc = V(P, np.ones(512)), V(P, np.zeros(512))
        Ac.mult(xc, yc)
        nv = C.c_int(-1)
        L.MatHIPMI355XGetValuePatterns(Ac.h, C.byref(nv))
        assert (nv.value > 0) == (vp == b"1")
        L.PetscOptionsClear()
        g = check_routes(P, Ac, "p7 value patterns " + vp.decode())
        got[vp] = g
    assert all(same(got[b"1"][k], got[b"0"][k]) for k in got[b"1"])
    # Frobenius == sqrt(mi355x_vec_norm(values)) bit for bit
    d_a = dev.put(aa)
    dev.chk(dev.k.mi355x_vec_norm(dev.h, aa.size, 2, d_a, dev.host_scratch()))
    assert bits(first["fro"])[0] == bits(np.sqrt(dev.scalar_out(1)))[0]
    # the same matrix as BAIJ, bs = 3
    mbs = n // 3
    rowsb = np.repeat(np.arange(n), np.diff(ai))
    bkey = np.unique(np.stack([rowsb // 3, aj // 3], axis=1), axis=0)
    bi = np.concatenate(([0], np.cumsum(np.bincount(bkey[:, 0], minlength=mbs)))).astype(np.int32)
    bj = bkey[:, 1].astype(np.int32)
    D = np.zeros((n, n)); D[rowsb, aj] = aa
    ba = np.concatenate([D[3 * I:3 * I + 3, 3 * J:3 * J + 3].T.ravel() for I, J in bkey])
    Bm = P.Mat.from_bsr(3, bi, bj, ba)
    gb = check_routes(P, Bm, "baij 3", point_csr=S.bsr_to_csr(3, bi, bj, ba), stored=ba)
    for k in ("inf", "one", "maxabs", "c1", "cinf"):
        if np.array_equal(np.diff(S.bsr_to_csr(3, bi, bj, ba)[0]), np.diff(ai)):      # no block holds a structural zero: the same stored entries
            assert same(gb[k], first[k]), k


def chebyshev_residuals(sym, dhalf, b, emin, emax, steps):
    """||B r_k||, k = 0 .. steps, of the Chebyshev iteration from a zero guess, stated without the iteration: B r_k = p_k(B A) B b with
    the residual polynomial p_k(l) = T_k((th - l) / de) / T_k(th / de), th = (emax + emin) / 2, de = (emax - emin) / 2.  sym = D^-1/2 A D^-1/2
    (B = D^-1, dhalf = sqrt(diag))"""
    lam, Q = np.linalg.eigh(sym)
    th, de = 0.5 * (emax + emin), 0.5 * (emax - emin)
    c = Q.T @ (dhalf * (b / dhalf ** 2))

    def T(k, x):
        return np.real(np.cosh(k * np.arccosh(np.asarray(x, dtype=complex))))
    return np.array([np.linalg.norm((Q @ (T(k, (th - lam) / de) / T(k, th / de) * c)) / dhalf) for k in range(steps + 1)])


def test_row_sum_on_an_order_sensitive_row(P):
    """MatGetRowSum is MatMult with a vector of ones: the bits of the model on a row holding 1e16, 1, -1e16 (left to right 0.0, not 1.0),
    for AIJ and for the same matrix as a one-rank MPIAIJ"""
    si = np.array([0, 3, 4, 4], np.int32); sj = np.array([0, 1, 2, 1], np.int32); sa = np.array([1e16, 1.0, -1e16, 2.0])
    ref = R.row_sums(R.SUM, si, sa)
    assert ref[0] == 0.0 and ref[1] == 2.0 and ref[2] == 0.0
    for Sm in (P.Mat.from_csr(si, sj, sa, ncols=3), P.Mat.from_csr_mpi(si, sj, sa, 3, comm=P.lib().COMM_SELF)):
        assert np.array_equal(bits(Sm.row_sum().array()), bits(ref))


def test_equilibrate_then_bound_chebyshev(P):
    """the worked example: D^-1 A by MatDiagonalScale, emax = ||D^-1 A||_inf >= the largest eigenvalue (Gershgorin); Chebyshev with
    that bound (and emin = emax / 10) reduces the residual monotonically over 10 iterations.

    Which right-hand side: the Chebyshev residual is p_k(B A) applied to the first one, and |p_k(l)| falls with k for every eigenvalue
    l <= emin (T_k+1 / T_k grows with its argument beyond 1) while inside (emin, emax] p_k oscillates -- p_1 has its root at the middle
    of the interval, where |p_2| has its maximum.  So a monotone residual is a theorem for a right-hand side made of the eigenvectors
    with l <= emin, the smooth part that a guessed emin leaves outside the interval and that converges slowest; that is the case the
    monotone assertion runs on, counted from the start residual.  For a right-hand side in the middle of the spectrum it is not:
    b = cos(i) has 53 % of its weight at 0.8 < l < 1.4 and the exact polynomials give 2.667, 0.8687, 0.9658, 0.6140, 0.2071 ...; on
    that one the solver's recorded norms are held to the polynomials' instead.  The history's first entry is the norm after the first
    step (KSPSolve_Chebychev records the residual of p[k], cheby.c): entry i is ||B r_(i+1)||."""
    L = P.lib()
    ai, aj, aa = orc.gen_p7(8, 8, 8)
    n = ai.size - 1
    rows = np.repeat(np.arange(n), np.diff(ai))
    diag = aa[rows == aj]
    dhalf = np.sqrt(diag)
    Dm = np.zeros((n, n)); Dm[rows, aj] = aa
    sym = Dm / np.outer(dhalf, dhalf)                                         # D^-1 A is similar to the symmetric D^-1/2 A D^-1/2
    lam, Q = np.linalg.eigh(sym)
    A = P.Mat.from_csr(ai, aj, aa); S_ = P.Mat.from_csr(ai, aj, aa)
    dinv = V(P, 1.0 / diag)
    L.MatDiagonalScale(S_.h, dinv.h, None)
    emax = S_.norm(P.NORM_INFINITY)
    assert emax >= lam[-1] and emax <= 2.0 + 1e-12
    emin = 0.1 * emax
    low = lam <= emin
    assert 4 <= low.sum() < n // 8
    for name, rhs in (("smooth", dhalf * (Q[:, low] @ np.ones(int(low.sum())))), ("cos", np.cos(np.arange(n)))):
        b, x = V(P, rhs), V(P, np.zeros(n))
        ksp = P.KSP(comm=L.COMM_SELF)
        ksp.set_operators(A); ksp.set_type("chebychevhipmi355x"); ksp.set_pc_type("jacobi")
        ksp.set_chebychev_eigenvalues(emax, emin)
        ksp.set_tolerances(rtol=1e-30, max_it=10)
        ksp.record_history()
        ksp.solve(b, x)
        h = np.asarray(ksp.history())
        ref = chebyshev_residuals(sym, dhalf, rhs, emin, emax, 11)
        print(name, "recorded", h, "polynomials", ref)
        assert h.size == 11
        # the iteration is 11 steps of a few rounded operations each on vectors of norm <= |B b|, and |p_k| <= 1 amplifies nothing:
        # the recorded norms stay within 1e-12 |B b| of the exact ones (the eigendecomposition behind `ref` is good to about 1e-14)
        assert np.all(np.abs(h - ref[1:]) <= 1e-12 * ref[0]), (name, h - ref[1:])
        if name == "smooth":
            seq = np.concatenate(([ref[0]], h))                               # the start residual, then after each of the iterations
            assert np.all(np.diff(seq[:11]) < 0.0) and np.all(np.diff(seq) < 0.0), seq
