"""csrc/vec_kernels.hip (and the pack / unpack kernels) on IEEE specials, scalar special cases and behind guard bands.

Every operand is a view into an allocation of the test's own with NaN guards on both sides (vecspecials.Guarded); every check
ends with the guards of every operand, read-only ones included, and a read-only operand must come back unchanged.  Vectors are
compared with the oracle's loops under vecspecials.same (any NaN equals any NaN, all else bit for bit); reductions with
orc.device_reduction_order() bit for bit where every operand is 16-byte aligned, and where one is not (the scalar grid-stride
path, another fixed tree) to the suite's stated 1e-13 * sum|terms|, finite.  test_vec_specials_cpu.py shows with the oracle
alone that the inputs used here tell every special branch from the general form.

A guard bands and alignment on finite data, every entry point     B element-wise kernels on special data, every scalar branch
C fused sweeps on special data                                     D reductions: class of non-finite results, bits of finite ones
E more vectors than one sweep takes                                F scalars formed on the device"""
import ctypes as C

import numpy as np
import pytest

import orc
import vecspecials as vs
from vecspecials import INF, NAN, K, KINDS, FINITE_KINDS, Guarded, guards_intact, same

pytestmark = pytest.mark.gpu

A_SIZES = [1, 2, 3, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1535, 1537, 2047, 2049, 4095, 4096, 4097, 8193]
B_SIZES = [3, 513, 1025, 4097]
D_SIZES = [3, 4097, 8193, (1 << 21) + 1]
E_SIZES = [3, 1025, 4097]
TOL = 1e-13          # the suite's stated bound for a reduction in another fixed order: |err| <= TOL * sum|terms|


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


class Run:
    """the device side of one case at one size and alignment pattern: a Guarded allocation per operand, 64 device scalars, the
    pinned result slots"""

    def __init__(self, dev, ops, n, pattern):
        self.dev, self.k, self.h, self.n, self.ops = dev, dev.k, dev.h, n, list(ops)
        self.g = {name: Guarded(dev, n, off, tag=j + 1) for j, (name, off) in enumerate(zip(ops, pattern))}
        self.p = {name: g.ptr for name, g in self.g.items()}
        self.res = dev.host_scratch()
        self.scal_ptr = dev.alloc(8 * 64)
        self._perm = None
        self.v = None

    def scal(self, values):
        a = np.zeros(64)
        a[:len(values)] = values
        self.dev.chk(self.k.mi355x_memcpy_h2d(self.h, self.scal_ptr, a.ctypes.data, a.nbytes))
        self.dev.sync()
        return self.scal_ptr

    def table(self, names):
        return self.dev.ptr_table([self.p[name] for name in names])

    def perm(self):
        if self._perm is None:
            self._perm = self.dev.put(self.v["__perm__"])
        return self._perm, self.v["__perm__"]

    def load(self, v):
        self.v = v
        for name, g in self.g.items():
            g.load(v[name])

    def free(self):
        for g in self.g.values():
            g.free()
        self.dev.free(self.scal_ptr)
        if self._perm is not None:
            self.dev.free(self._perm)


def check(X, case, t, v, aligned, what):
    """load, launch, compare every operand and every sum, then the guards"""
    dev = X.dev
    X.load(v)
    with np.errstate(all="ignore"):
        ref, sums = case.ref(t, v)
        if aligned:
            with orc.device_reduction_order():
                vals = [vs.sum_value(s) for s in sums]
        else:
            vals = [vs.sum_value(s) for s in sums]
    dev.chk(case.call(X, t))
    got = dev.scalar_out(max(len(sums), 1))
    for name, g in X.g.items():
        same(g.get(), ref.get(name, v[name]), "%s: %s" % (what, name if name in ref else name + " (read only)"))
    for j, (s, (val, scale)) in enumerate(zip(sums, vals)):
        if aligned or s[0] in ("max", "val"):
            same(got[j], val, "%s: sum %d" % (what, j))
        else:
            assert np.isfinite(got[j]) and abs(got[j] - val) <= TOL * scale, "%s: sum %d: %r against %r (sum|terms| %g)" % (what, j, got[j], val, scale)
    guards_intact(*X.g.values(), names=X.ops)


# ------------------------------------------------------------------------------------------------------------------- A
A_CASES = vs.guard_band_cases()


@pytest.mark.parametrize("case", A_CASES, ids=[c.name for c in A_CASES])
def test_a_guard_bands_and_alignment(dev, case):
    """finite data at the edges of the 512-double2 map tile, the 256-lane half tile, the 4x-unrolled reduction sweep and the
    first multi-workgroup reduction; all operands aligned, all 8 bytes off, each single one 8 bytes off.  A kernel that stores
    past its view changes a guard; a reduction that reads x[n] or x[-1] returns NaN against a finite reference."""
    tuples = vs.finite_tuples(case)
    for n in A_SIZES:
        v = vs.operands(case, n, 0, finite=True)
        for pattern in vs.alignment_patterns(len(case.ops)):
            X = Run(dev, case.ops, n, pattern)
            for t in tuples:
                check(X, case, t, v, not any(pattern), "%s%r n = %d offsets %r" % (case.name, t, n, pattern))
            X.free()


# ------------------------------------------------------------------------------------------------------------------- B
B_CASES = vs.ELEMENTWISE + [vs.MAXPY_SPECIAL]


@pytest.mark.parametrize("case", B_CASES, ids=[c.name for c in B_CASES])
def test_b_elementwise_on_special_data(dev, case):
    """every scalar tuple that selects a branch of the reference, on vectors of NaN, +-Inf, signed zeros, subnormals and values
    at the ends of the range, every kind in turn at element 0, at the odd tail and in the last tile; even rotations on aligned
    views (the double2 body), odd ones 8 bytes off (the scalar loop)"""
    for n in B_SIZES:
        Xs = [Run(dev, case.ops, n, (off,) * len(case.ops)) for off in (0, 1)]
        for rot in range(K):
            v = vs.operands(case, n, rot)
            for t in case.tuples:
                check(Xs[rot & 1], case, t, v, not rot & 1, "%s%r n = %d rot %d" % (case.name, t, n, rot))
        for X in Xs:
            X.free()


# ------------------------------------------------------------------------------------------------------------------- C
C_CASES = vs.FUSED + [vs.SCALE_RNORM]


@pytest.mark.parametrize("case", C_CASES, ids=[c.name for c in C_CASES])
def test_c_fused_sweeps_on_special_data(dev, case):
    """the fused CG / BiCGStab / GMRES sweeps against the oracle's loops for the calls they replace: every refused CG step
    leaves x, r, z and sol alone with sums of +0.0, a zero step length or a zero numerator takes the reference's branch.  All
    kinds of specials (the sums are then mostly NaN or Inf: their class must be the device-order oracle's), and finite
    specials only -- signed zeros, subnormals, subnormal products -- where the sums are finite and compared bit for bit."""
    for n in B_SIZES:
        X = Run(dev, case.ops, n, (0,) * len(case.ops))
        for kinds in (KINDS, FINITE_KINDS):
            for rot in range(0, kinds.size, 2 if n > 3 else 1):
                v = vs.operands(case, n, rot, kinds=kinds)
                for t in case.tuples:
                    check(X, case, t, v, True, "%s%r n = %d rot %d" % (case.name, t, n, rot))
        X.free()


@pytest.mark.parametrize("with_d", [True, False])
def test_c_cg_update_against_the_separate_calls(dev, with_d):
    """mi355x_vec_cg_update, a in {0.0, -0.0, 0.731}: x, r, z and the three sums are those of mi355x_vec_axpy, mi355x_vec_axpy,
    mi355x_vec_pointwise_mult (a copy without d), mi355x_vec_norm(2), mi355x_vec_dot, mi355x_vec_norm(2) issued separately;
    the accepted device-scalar step is the host-scalar step"""
    k = dev.k
    case = vs.FUSED[0] if with_d else vs.FUSED[1]
    ops = case.ops
    for n in B_SIZES:
        X, Y = Run(dev, ops, n, (0,) * len(ops)), Run(dev, ops, n, (0,) * len(ops))
        for rot in range(0, K, 2):
            v = vs.operands(case, n, rot)
            for a in (0.0, -0.0, 0.731):
                X.load(v); Y.load(v)
                dev.chk(case.call(X, (a,)))
                fused = dev.scalar_out(3)
                dev.chk(k.mi355x_vec_axpy(dev.h, n, a, Y.p["p"], Y.p["x"]))
                dev.chk(k.mi355x_vec_axpy(dev.h, n, -a, Y.p["w"], Y.p["r"]))
                if with_d:
                    dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, Y.p["r"], Y.p["d"], Y.p["z"]))
                else:
                    dev.chk(k.mi355x_vec_copy(dev.h, n, Y.p["r"], Y.p["z"]))
                sep = []
                dev.chk(k.mi355x_vec_norm(dev.h, n, 2, Y.p["z"], dev.host_scratch())); sep.append(dev.scalar_out()[0])
                dev.chk(k.mi355x_vec_dot(dev.h, n, Y.p["z"], Y.p["r"], dev.host_scratch())); sep.append(dev.scalar_out()[0])
                dev.chk(k.mi355x_vec_norm(dev.h, n, 2, Y.p["r"], dev.host_scratch())); sep.append(dev.scalar_out()[0])
                what = "a = %r n = %d rot %d" % (a, n, rot)
                for name in ops:
                    same(X.g[name].get(), Y.g[name].get(), what + ": " + name)
                same(fused, np.array(sep), what + ": sums")
                guards_intact(*X.g.values(), *Y.g.values(), names=ops + ops)
            # the device-scalar step, accepted: a = beta / dpi formed in the kernel
            beta, dpi = 0.83, 1.37
            X.load(v); Y.load(v)
            dev.chk(case.call(X, (np.float64(beta) / np.float64(dpi),)))
            host = dev.scalar_out(3)
            d = Y.p["d"] if with_d else None
            dev.chk(k.mi355x_vec_cg_update_dev(dev.h, n, beta, Y.scal([dpi]), 0.5, 1, Y.p["p"], Y.p["w"], d, Y.p["x"], Y.p["r"], Y.p["z"], dev.host_scratch(), 0))
            same(dev.scalar_out(4), np.append(host, dpi), "device-scalar sums")
            for name in ops:
                same(X.g[name].get(), Y.g[name].get(), "device-scalar step: " + name)
        X.free(); Y.free()


def test_c_maxpy_dev_norm2_zero_coefficient_then_scale_rnorm_dev(dev):
    """the fused Gram-Schmidt update with a zero coefficient against Inf / NaN columns (NaN must appear, as in VecMAXPY), its sum
    left in device memory, and VecNormalize's scaling by that sum right after it"""
    k = dev.k
    case = vs.FUSED[-1]
    for n in B_SIZES:
        X = Run(dev, case.ops, n, (0,) * len(case.ops))
        out = dev.alloc(16)
        for kinds in (KINDS, FINITE_KINDS):
            for rot in range(0, kinds.size, 3):
                v = vs.operands(case, n, rot, kinds=kinds)
                for t in case.tuples:
                    X.load(v)
                    dev.chk(k.mi355x_vec_maxpy_dev_norm2(dev.h, n, 3, X.scal(t), -1.0, X.table(case.ops[1:]), X.p["x"], out))
                    dev.chk(k.mi355x_vec_scale_rnorm_dev(dev.h, n, out, X.p["x"]))
                    dev.sync()
                    with np.errstate(all="ignore"):
                        ref, sums = case.ref(t, v)
                        with orc.device_reduction_order():
                            n2 = vs.sum_value(sums[0])[0]
                        xs = vs._scale_rnorm_ref(n2, ref["x"])
                    same(dev.get(out, 1), n2, "sum")
                    same(X.g["x"].get(), xs, "x, n = %d rot %d %r" % (n, rot, t))
                    if kinds is KINDS and n > 3:
                        j = [i for i in range(3) if t[i] == 0.0][0]
                        assert np.all(np.isnan(ref["x"][~np.isfinite(v["y%d" % j])]))
                    guards_intact(*X.g.values(), names=case.ops)
        dev.free(out); X.free()


# ------------------------------------------------------------------------------------------------------------------- D
D_OPS, reduction_positions = vs.D_OPS, vs.reduction_positions


def run_reductions(X, v, mode, what):
    """every reduction on the loaded operands: mode "class" -- the class of each result is the sequential oracle's; mode "bits"
    -- each result carries the bits of the device-order oracle"""
    dev = X.dev
    for case in vs.REDUCTIONS:
        with np.errstate(all="ignore"):
            _, sums = case.ref((), v)
            if mode == "bits":
                with orc.device_reduction_order():
                    vals = [vs.sum_value(s)[0] for s in sums]
            else:
                vals = [vs.sum_value(s)[0] for s in sums]
        dev.chk(case.call(X, ()))
        got = dev.scalar_out(len(sums))
        for j in range(len(sums)):
            if mode == "bits":
                assert np.isfinite(vals[j])
                same(got[j], vals[j], "%s: %s sum %d" % (what, case.name, j))
            else:
                assert vs.klass(got[j]) == vs.klass(vals[j]), "%s: %s sum %d: %r, the oracle has %r" % (what, case.name, j, got[j], vals[j])


@pytest.mark.parametrize("n", D_SIZES)
def test_d_reductions_on_special_data(dev, n):
    """dot, the five norms, dot + norm2 and MDot(5): a single NaN / +Inf / -Inf, or +Inf with -Inf, at every structural position
    gives the class the sequential oracle gives; vectors of signed zeros and subnormals (subnormal products among them) give the
    bits of the device-order oracle.  2^21 + 1 elements are 512 workgroups: the last one reads the partials four at a time."""
    X = Run(dev, D_OPS, n, (0,) * len(D_OPS))
    base = {name: np.abs(np.random.default_rng(31 + j).standard_normal(n)) for j, name in enumerate(D_OPS)}    # positive: Inf * y keeps its sign
    base["__perm__"] = None
    X.load(base)
    pos = reduction_positions(n)
    names = list(pos)
    for label, vals in [("nan", (NAN,)), ("+inf", (INF,)), ("-inf", (-INF,)), ("+inf and -inf", (INF, -INF))]:
        for i, pname in enumerate(names):
            p = pos[pname]
            spots = [(p, vals[0])]
            if len(vals) > 1:
                q = pos[names[(i + 1) % len(names)]]
                spots.append((q if q != p else (p + 1) % n, vals[1]))
            v = {name: (a.copy() if name in ("x", "t") else a) for name, a in base.items()}
            for name in ("x", "t"):
                for at, val in spots:
                    X.g[name].poke(at, val); v[name][at] = val
            run_reductions(X, v, "class", "%s at %s, n = %d" % (label, pname, n))
            if len(vals) == 1:                                            # the class is known without any oracle as well
                dev.chk(dev.k.mi355x_vec_norm(dev.h, n, 3, X.p["x"], X.res))
                assert vs.klass(dev.scalar_out()[0]) == ("nan" if label == "nan" else "+inf")
                dev.chk(dev.k.mi355x_vec_dot(dev.h, n, X.p["x"], X.p["y"], X.res))
                assert vs.klass(dev.scalar_out()[0]) == label
            for name in ("x", "t"):
                for at, _ in spots:
                    X.g[name].poke(at, base[name][at])
    # the special vectors: every kind at once (class), finite kinds (bits)
    for kinds, mode in ((KINDS, "class"), (FINITE_KINDS, "bits")):
        for rot in ((0, 4, 9) if n < (1 << 20) else (4,)):
            v = vs.reduction_vectors(n, rot, kinds)
            X.load(v)
            run_reductions(X, v, mode, "special vectors rot %d n = %d" % (rot, n))
    # norm(3) of all -0.0 is +0.0; a square that overflows is +Inf, not NaN
    X.g["x"].load(np.full(n, -0.0))
    dev.chk(dev.k.mi355x_vec_norm(dev.h, n, 3, X.p["x"], X.res))
    assert vs.bits(dev.scalar_out())[0] == 0
    big = base["x"].copy(); big[n // 2] = 1e200
    X.g["x"].load(big)
    for ntype in (1, 2, 4):
        dev.chk(dev.k.mi355x_vec_norm(dev.h, n, ntype, X.p["x"], X.res))
        assert dev.scalar_out(2)[1 if ntype == 4 else 0] == INF
    guards_intact(*X.g.values(), names=D_OPS)
    X.free()


# ------------------------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize("nv", [32, 33, 35, 36, 61, 64])
def test_e_maxpy_beyond_one_sweep(dev, nv):
    """more than 32 vectors: a second sweep of mi355x_vec_maxpy and of mi355x_vec_maxpy_dev_norm2, whose earlier sweeps park
    their sums in the last device scratch slot: x of orc.vec_maxpy bit for bit, x and the sum of the fused form those of
    mi355x_vec_maxpy + mi355x_vec_norm(2), every other device scratch slot untouched"""
    k = dev.k
    case, fused = vs._maxpy_case(nv), vs._maxpy_norm_case(nv)
    scratch = C.c_void_p(k.mi355x_handle_device_scratch(dev.h))
    for n in E_SIZES:
        v = vs.operands(case, n, 0, finite=True)
        X = Run(dev, case.ops, n, (0,) * len(case.ops))
        check(X, case, case.tuples[0], v, True, "maxpy nv = %d n = %d" % (nv, n))
        t = fused.tuples[0]
        mt = tuple(-1.0 * np.array(t))
        X.load(v)
        dev.chk(case.call(X, mt))
        dev.chk(k.mi355x_vec_norm(dev.h, n, 2, X.p["x"], X.res))
        sep_n2, sep_x = dev.scalar_out()[0], X.g["x"].get()
        marks = 1000.0 + np.arange(64)
        dev.chk(k.mi355x_memcpy_h2d(dev.h, scratch, marks.ctypes.data, marks.nbytes)); dev.sync()
        X.load(v)
        dev.chk(k.mi355x_vec_maxpy_dev_norm2(dev.h, n, nv, X.scal(t), -1.0, X.table(case.ops[1:]), X.p["x"], scratch))
        dev.sync()
        after = dev.get(scratch, 64)
        same(after[0], sep_n2, "sum, nv = %d n = %d" % (nv, n))
        same(after[1:63], marks[1:63], "device scratch slots 1 .. 62")
        same(X.g["x"].get(), sep_x, "x, nv = %d n = %d" % (nv, n))
        with np.errstate(all="ignore"), orc.device_reduction_order():
            ref, sums = fused.ref(t, v)
            same(after[0], vs.sum_value(sums[0])[0], "sum against the oracle")
        same(sep_x, ref["x"], "x against the oracle")
        guards_intact(*X.g.values(), names=case.ops)
        X.free()


@pytest.mark.parametrize("nv", [16, 18, 23, 24, 32, 33, 40])
def test_e_mdot_beyond_one_pass(dev, nv):
    """mi355x_vec_mdot splits at 16 vectors per pass (17 .. 23 into two halves): 16 + 16 + a remainder and every split below it,
    bit for bit the device-order oracle"""
    case = vs._mdot_case(nv)
    for n in E_SIZES:
        X = Run(dev, case.ops, n, (0,) * len(case.ops))
        check(X, case, (), vs.operands(case, n, 0, finite=True), True, "mdot nv = %d n = %d" % (nv, n))
        check(X, case, (), vs.operands(case, n, 3, kinds=FINITE_KINDS), True, "mdot on finite specials nv = %d n = %d" % (nv, n))
        X.free()


@pytest.mark.parametrize("n", [1 << 19, (1 << 19) + 3])
def test_e_gram_schmidt_sweeps_at_the_streaming_threshold(dev, n):
    """32 basis vectors on either side of gs_streams()'s threshold (nv * n * 8 > 128 MiB): at n = 2^19 the sweep of
    mi355x_vec_maxpy and of mi355x_vec_maxpy_dev_norm2 loads the basis through the caches, at 2^19 + 3 (an odd tail) non-temporally.
    A cache hint is not a result: x of both is that of the oracle's MAXPY loop bit for bit, the fused sum that of the device-order
    oracle and of mi355x_vec_norm(2) on the updated x, the 32 sums of mi355x_vec_mdot (two passes of 16 at the default width, whose
    basis of 64 MiB stays cacheable at both sizes) those of the device-order oracle; the basis comes back unchanged, every guard intact."""
    k, nv = dev.k, 32
    case, fused, md = vs._maxpy_case(nv), vs._maxpy_norm_case(nv), vs._mdot_case(nv)
    ys = case.ops[1:]
    v = vs.operands(case, n, 0, finite=True)
    X = Run(dev, case.ops, n, (0,) * len(case.ops))
    X.load(v)
    what = "nv = %d n = %d" % (nv, n)
    dev.chk(md.call(X, ()))
    got = dev.scalar_out(nv)
    with orc.device_reduction_order():
        same(got, [vs.dsum(v["x"], v[y]) for y in ys], "mdot " + what)
    t = case.tuples[0]
    dev.chk(case.call(X, t))
    dev.sync()
    same(X.g["x"].get(), case.ref(t, v)[0]["x"], "maxpy x " + what)
    X.g["x"].load(v["x"])
    t = fused.tuples[0]
    dev.chk(fused.call(X, t))
    n2 = dev.scalar_out()[0]
    ref, sums = fused.ref(t, v)
    same(X.g["x"].get(), ref["x"], "maxpy_dev_norm2 x " + what)
    with orc.device_reduction_order():
        same(n2, vs.sum_value(sums[0])[0], "maxpy_dev_norm2 sum against the oracle " + what)
    dev.chk(k.mi355x_vec_norm(dev.h, n, 2, X.p["x"], X.res))
    same(dev.scalar_out()[0], n2, "maxpy_dev_norm2 sum against mi355x_vec_norm " + what)
    for y in ys:
        same(X.g[y].get(), v[y], y + " (read only) " + what)
    guards_intact(*X.g.values(), names=case.ops)
    X.free()


# ------------------------------------------------------------------------------------------------------------------- F
def test_f_scale_rnorm_dev_over_the_range(dev):
    """x *= 1 / sqrt(*norm2) for 300 norm2 values log-uniform in [1e-320, 1e300] and the edges: numpy's sqrt and division are
    correctly rounded and are the reference; a zero norm and a norm of one leave x alone, an infinite norm sets zero"""
    case = vs.SCALE_RNORM
    rng = np.random.default_rng(77)
    values = list(10.0 ** rng.uniform(-320, 300, 300)) + vs.RNORM_EDGES
    assert min(values[:300]) < 1e-308 and max(values[:300]) > 1e290          # subnormal norms and huge ones are among them
    x = np.array([1.5, -0.3333333333333333, 7.123e10])
    X = Run(dev, case.ops, 3, (0,))
    for val in values:
        check(X, case, (val,), {"x": x, "__perm__": None}, True, "norm2 = %r" % val)
    X.free()


def quotient_pairs():
    """(numerator, denominator) whose quotient is subnormal, underflows to zero, is near overflow, or is exactly representable"""
    rng = np.random.default_rng(78)
    pairs = []
    for _ in range(60):
        a, b = rng.uniform(1.0, 2.0, 2) * rng.choice([-1.0, 1.0], 2)
        pairs += [(a * 1e-160, b * 1e155), (a * 1e-170, b * 1e150), (a * 1e150, b * 1e-157), (a * 1e150, b * 1e-158)]
        m = float(rng.integers(1, 1 << 20))
        pairs += [(m * 3.0, 3.0), (m, 2.0 ** int(rng.integers(-40, 40)))]
    pairs += [(5e-324, 2.0), (5e-324, -4.0), (1e-300, 1e300), (vs.DBL_MAX, 1.0), (vs.DBL_MAX, 0.9999999999999999), (1.0, 3.0)]
    return pairs


def test_f_quotients_formed_on_the_device(dev):
    """a = beta / *dpi in mi355x_vec_cg_update_dev and alpha = *num / den in mi355x_vec_aypx_dev: vectors are those of the
    host-scalar forms called with numpy's quotient -- subnormal, flushed to zero by underflow, near overflow and exact ones"""
    k = dev.k
    pairs = quotient_pairs()
    with np.errstate(all="ignore"):
        q = np.array([np.float64(a) / np.float64(b) for a, b in pairs])
    assert ((q != 0) & (np.abs(q) < vs.DBL_MIN)).sum() >= 50 and (q == 0).sum() >= 1 and (np.abs(q) > 1e306).sum() >= 50 and np.isinf(q).sum() >= 1
    cg, ay = vs.FUSED[0], vs.FUSED[6]
    assert ay.name == "aypx_dev"
    v = {"p": [1.5, -2.25, 3e-3], "w": [0.7, 1e3, -4.5], "d": [0.5, 0.25, 3.0], "x": [1.0, -1e-3, 2.0], "r": [-0.3, 8.0, 1e-2], "z": [9.0, 9.0, 9.0],
         "y": [2.0, -3e5, 0.125]}
    v = {name: np.array(a) for name, a in v.items()}
    X, Y = Run(dev, cg.ops, 3, (0,) * 6), Run(dev, cg.ops, 3, (0,) * 6)
    A, B = Run(dev, ay.ops, 3, (0, 0)), Run(dev, ay.ops, 3, (0, 0))
    for (num, den), quo in zip(pairs, q):
        what = "%r / %r" % (num, den)
        X.load(v); Y.load(v)
        dev.chk(k.mi355x_vec_cg_update_dev(dev.h, 3, num, X.scal([den]), 1.0, 0, X.p["p"], X.p["w"], X.p["d"], X.p["x"], X.p["r"], X.p["z"], X.res, 0))
        dsums = dev.scalar_out(3)
        dev.chk(k.mi355x_vec_cg_update(dev.h, 3, quo, Y.p["p"], Y.p["w"], Y.p["d"], Y.p["x"], Y.p["r"], Y.p["z"], Y.res))
        same(dsums, dev.scalar_out(3), what + ": sums")
        for name in cg.ops:
            same(X.g[name].get(), Y.g[name].get(), what + ": cg " + name)
        A.load(v); B.load(v)
        dev.chk(k.mi355x_vec_aypx_dev(dev.h, 3, A.scal([num]), den, A.p["x"], A.p["y"]))
        dev.chk(k.mi355x_vec_aypx(dev.h, 3, quo, B.p["x"], B.p["y"]))
        dev.sync()
        same(A.g["y"].get(), B.g["y"].get(), what + ": aypx y")
    guards_intact(*X.g.values(), *Y.g.values(), *A.g.values(), *B.g.values())
    for r in (X, Y, A, B):
        r.free()
