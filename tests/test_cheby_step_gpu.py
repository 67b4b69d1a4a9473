"""mi355x_vec_cheby_step / mi355x_vec_rich_step through the C ABI on guarded views: every output bit for bit against the host model
(tests/cheby_ref.py) and against the existing kernels run one call at a time (mi355x_vec_aypx, _pointwise_mult / _copy, _scale,
_axpy x2); the sums of an aligned view carry the bits of mi355x_vec_norm over the op-by-op z and r; guard bands and read-only
operands keep their bits; the special cases of VecScale / VecAXPY keep a skipped operand out of the result."""
import math

import numpy as np
import pytest

import cheby_ref as cr
import orc
from vecspecials import bits, guarded, guards_intact, same

pytestmark = pytest.mark.gpu

# 1023, 1024, 1025: one tile of 256 x 2 double2 (1024 doubles) and its edges; 4097: the first hand-off between workgroups of the
# reduction (16 doubles per lane: 4096 per workgroup); (1 << 21) + 1: beyond the 512-workgroup cap of the reduction's grid
SIZES = [1, 2, 3, 1023, 1024, 1025, 4097]
BIG = (1 << 21) + 1
POISON = 0x7FF8DEADBEEF0001


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def vec(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


def diag(n):
    return 1.0 / (2.0 + vec(n, 9) ** 2)


class Run:
    """operands on the device in guarded views `off` doubles off a 16-byte boundary, and the same data in plain (aligned) allocations
    for the op-by-op run"""

    def __init__(self, dev, n, off, host):
        self.dev, self.n, self.off, self.host = dev, n, off, host
        self.g = {name: guarded(dev, a, off, tag=j + 1) for j, (name, a) in enumerate(host.items()) if a is not None}
        self.out = dev.put(np.array([POISON, POISON], dtype=np.uint64))

    def p(self, name):
        return self.g[name].ptr if name in self.g else None

    def sums(self):
        return self.dev.get(self.out, 2)

    def check_readonly(self, written):
        for name, g in self.g.items():
            if name not in written:
                assert np.array_equal(bits(g.get()), bits(self.host[name])), "read-only operand %s changed" % name
        guards_intact(*self.g.values(), names=list(self.g))

    def free(self):
        for g in self.g.values():
            g.free()
        self.dev.free(self.out)


def op_by_op(dev, n, s, a, c, w, b, d, pm, pk):
    """the existing kernels, one call each: (r, z = B r, pn, sum z^2, sum r^2)"""
    k = dev.k
    dr, db, dz = dev.put(w), dev.put(b), dev.alloc(8 * max(n, 2))
    dev.chk(k.mi355x_vec_aypx(dev.h, n, -1.0, db, dr))
    if d is None:
        dev.chk(k.mi355x_vec_copy(dev.h, n, dr, dz))
    else:
        dd = dev.put(d)
        dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, dr, dd, dz))
    r, z = dev.get(dr, n), dev.get(dz, n)
    hs = dev.host_scratch()
    dev.chk(k.mi355x_vec_norm(dev.h, n, 1, dz, hs)); zz = dev.scalar_out(1)[0]
    dev.chk(k.mi355x_vec_norm(dev.h, n, 1, dr, hs)); rr = dev.scalar_out(1)[0]
    dev.chk(k.mi355x_vec_scale(dev.h, n, s, dz))
    if pm is not None:
        dpm = dev.put(pm); dev.chk(k.mi355x_vec_axpy(dev.h, n, a, dpm, dz)); dev.free(dpm)
    if pk is not None:
        dpk = dev.put(pk); dev.chk(k.mi355x_vec_axpy(dev.h, n, c, dpk, dz)); dev.free(dpk)
    pn = dev.get(dz, n)
    for q in (dr, db, dz) + ((dd,) if d is not None else ()):
        dev.free(q)
    return r, z, pn, zz, rr


def check_sums(got, z, r, zz, rr, aligned):
    if aligned:
        same(got, [zz, rr], "sums against mi355x_vec_norm over the op-by-op z, r")
    else:                                   # another walk over the same terms: every term is >= 0, so the sum is well conditioned
        for g, v in zip(got, (z, r)):
            sq = np.square(v)               # each square rounded, as the kernel rounds it: fsum adds the same terms exactly
            if not np.all(np.isfinite(sq)):
                assert (np.isnan(g) and (np.isnan(sq).any() or np.isinf(sq).any())) or (np.isinf(g) and not np.isnan(sq).any()), (g, "non-finite terms")
                continue
            t = math.fsum(sq)
            assert abs(g - t) <= 1e-13 * t, (g, t)


def cheby_case(dev, n, off, s, a, c, with_d=True, rmode="store", sums=True, host=None):
    """one launch, every check; rmode: "store" (r its own vector), "alias" (r is w), "null" """
    h = host or dict(w=vec(n, 1), b=vec(n, 2), d=diag(n) if with_d else None, pm=vec(n, 3), pk=vec(n, 4))
    h = dict(h, r=np.full(n, 7.0) if rmode == "store" else None, pn=np.full(n, -3.0))
    X = Run(dev, n, off, h)
    rp = {"store": X.p("r"), "alias": X.p("w"), "null": None}[rmode]
    dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, n, s, a, c, X.p("w"), X.p("b"), X.p("d"), X.p("pm"), X.p("pk"), rp, X.p("pn"), 1 if sums else 0, X.out))
    dev.sync()
    rm, zm, pnm = cr.step_ref(s, a, c, h["w"], h["b"], h["d"], h["pm"], h["pk"])
    r1, z1, pn1, zz, rr = op_by_op(dev, n, s, a, c, h["w"], h["b"], h["d"], h["pm"], h["pk"])
    pn = X.g["pn"].get()
    same(pn, pnm, "pn against the model"); same(pn, pn1, "pn against the kernels one by one")
    if rmode != "null":
        r = X.g["r" if rmode == "store" else "w"].get()
        same(r, rm, "r against the model"); same(r, r1, "r against the kernels one by one")
    if sums:
        check_sums(X.sums(), z1, r1, zz, rr, off == 0)
    else:
        assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64)), "out touched without sums"
    X.check_readonly({"pn", "r"} | ({"w"} if rmode == "alias" else set()))
    X.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_cheby_step_forms(dev, n, off):
    for s in (0.0, 1.0, 0.37):
        cheby_case(dev, n, off, s, 0.6, -1.4, sums=True)
    cheby_case(dev, n, off, 0.37, 0.6, -1.4, sums=False, rmode="null")            # the KSP_NORM_NONE form
    cheby_case(dev, n, off, 0.37, 0.6, -1.4, with_d=False, sums=True, rmode="alias")
    cheby_case(dev, n, off, 1.0, 0.6, -1.4, with_d=False, sums=False, rmode="store")
    cheby_case(dev, n, off, 0.37, 0.6, -1.4, sums=True, rmode="null")


@pytest.mark.parametrize("off", [0, 1])
def test_cheby_step_sums_beyond_the_grid_cap(dev, off):
    cheby_case(dev, BIG, off, 0.37, 0.6, -1.4, sums=True, rmode="null")


@pytest.mark.parametrize("off", [0, 1])
def test_cheby_step_special_cases_keep_skipped_operands_out(dev, off):
    n = 1025
    bad = vec(n, 5)
    bad[[0, 1, 511, 512, 1023, 1024]] = [np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan]
    base = dict(w=vec(n, 1), b=vec(n, 2), d=diag(n), pm=vec(n, 3), pk=vec(n, 4))
    for sums in (True, False):
        # a == 0: pm (Inf / NaN) must not reach pn (0 * Inf would be NaN); c == 0: the same for pk
        cheby_case(dev, n, off, 0.37, 0.0, -1.4, sums=sums, host=dict(base, pm=bad))
        cheby_case(dev, n, off, 0.37, -0.0, -1.4, sums=sums, host=dict(base, pm=bad))
        cheby_case(dev, n, off, 0.37, 0.6, 0.0, sums=sums, host=dict(base, pk=bad))
        cheby_case(dev, n, off, 0.37, 0.0, 0.0, sums=sums, host=dict(base, pm=bad, pk=bad))
        # s == 0: VecSet(0), not 0 * z -- an Inf in the residual stays out of pn (but is in r and in the sums)
        binf = base["b"].copy(); binf[[0, 700, 1024]] = [np.inf, -np.inf, np.inf]
        cheby_case(dev, n, off, 0.0, 0.6, -1.4, sums=sums, host=dict(base, b=binf))
        # NaN / Inf in b propagate as in the op-by-op run
        bnan = base["b"].copy(); bnan[[0, 3, 1023, 1024]] = [np.nan, np.inf, -np.inf, np.nan]
        cheby_case(dev, n, off, 0.37, 0.6, -1.4, sums=sums, host=dict(base, b=bnan))
    # the operands a form does not read may be NULL
    h = dict(base, pm=None, pk=None, r=None, pn=np.full(n, -3.0))
    X = Run(dev, n, off, h)
    dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, n, 0.37, 0.0, 0.0, X.p("w"), X.p("b"), X.p("d"), None, None, None, X.p("pn"), 0, None))
    dev.sync()
    same(X.g["pn"].get(), 0.37 * ((h["b"] - h["w"]) * h["d"]), "pn = s z")
    X.check_readonly({"pn"})
    X.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [3, 1025])
def test_cheby_step_with_the_preconditioned_residual_given(dev, n, off):
    """b == NULL: w is z itself, and may be pn (the update alone, in place): the route of a general preconditioner"""
    z, pm, pk = vec(n, 1), vec(n, 3), vec(n, 4)
    s, a, c = 0.37, 0.6, -1.4
    ref = z.copy()
    orc.vec_scale(ref, s); orc.vec_axpy(ref, a, pm); orc.vec_axpy(ref, c, pk)
    X = Run(dev, n, off, dict(pn=z, pm=pm, pk=pk))
    dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, n, s, a, c, X.p("pn"), None, None, X.p("pm"), X.p("pk"), None, X.p("pn"), 0, None))
    dev.sync()
    same(X.g["pn"].get(), ref, "in-place update")
    X.check_readonly({"pn"})
    assert dev.k.mi355x_vec_cheby_step(dev.h, n, s, a, c, X.p("pn"), None, X.p("pm"), X.p("pm"), X.p("pk"), None, X.p("pn"), 0, None) != 0   # d without b: refused
    X.free()


def test_steps_on_empty_vectors(dev):
    out = dev.put(np.array([POISON, POISON], dtype=np.uint64))
    p = dev.alloc(64)
    dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, 0, 0.37, 0.6, -1.4, p, p, p, p, p, None, p, 1, out))
    assert np.array_equal(bits(dev.get(out, 2)), bits(np.zeros(2)))                # with sums: zeros
    dev.chk(dev.k.mi355x_memcpy_h2d(dev.h, out, np.array([POISON, POISON], dtype=np.uint64).ctypes.data, 16)); dev.sync()
    dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, 0, 0.37, 0.6, -1.4, p, p, p, p, p, None, p, 0, out))
    dev.chk(dev.k.mi355x_vec_rich_step(dev.h, 0, 0.8, p, p, p, None, None, p))
    assert np.array_equal(dev.get(out, 2).view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    dev.free(out); dev.free(p)


# ---------------------------------------------------------------------------------------------------------------- Richardson
def rich_case(dev, n, off, scale, with_d=True, rmode="store", with_z=True, host=None):
    h = host or dict(w=vec(n, 1), b=vec(n, 2), d=diag(n) if with_d else None, x=vec(n, 6))
    h = dict(h, r=np.full(n, 7.0) if rmode == "store" else None, z=np.full(n, -3.0) if with_z else None)
    X = Run(dev, n, off, h)
    rp = {"store": X.p("r"), "alias": X.p("w"), "null": None}[rmode]
    dev.chk(dev.k.mi355x_vec_rich_step(dev.h, n, scale, X.p("w"), X.p("b"), X.p("d"), rp, X.p("z"), X.p("x")))
    dev.sync()
    rm, zm, xm = cr.rich_step_ref(scale, h["w"], h["b"], h["d"], h["x"])
    r1, z1, _, _, _ = op_by_op(dev, n, 1.0, 0.0, 0.0, h["w"], h["b"], h["d"], None, None)
    dx, dz = dev.put(h["x"]), dev.put(z1)
    dev.chk(dev.k.mi355x_vec_axpy(dev.h, n, scale, dz, dx))
    x1 = dev.get(dx, n)
    dev.free(dx); dev.free(dz)
    x = X.g["x"].get()
    same(x, xm, "x against the model"); same(x, x1, "x against the kernels one by one")
    if rmode != "null":
        r = X.g["r" if rmode == "store" else "w"].get()
        same(r, rm, "r against the model"); same(r, r1, "r against the kernels one by one")
    if with_z:
        same(X.g["z"].get(), zm, "z against the model"); same(X.g["z"].get(), z1, "z against the kernels one by one")
    assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    X.check_readonly({"x", "r", "z"} | ({"w"} if rmode == "alias" else set()))
    X.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_rich_step_forms(dev, n, off):
    for scale in (0.0, 1.0, 0.8):
        rich_case(dev, n, off, scale)
    rich_case(dev, n, off, 0.8, with_d=False, rmode="alias")
    rich_case(dev, n, off, 0.8, rmode="null", with_z=False)                       # the form the solver runs
    rich_case(dev, n, off, 0.8, with_d=False, rmode="null", with_z=True)


@pytest.mark.parametrize("off", [0, 1])
def test_rich_step_specials(dev, off):
    n = 1025
    base = dict(w=vec(n, 1), b=vec(n, 2), d=diag(n), x=vec(n, 6))
    bnan = base["b"].copy(); bnan[[0, 3, 1023, 1024]] = [np.nan, np.inf, -np.inf, np.nan]
    rich_case(dev, n, off, 0.8, host=dict(base, b=bnan))
    rich_case(dev, n, off, 0.0, host=dict(base, b=bnan))                          # scale == 0: x keeps its bits whatever z holds
    rich_case(dev, n, off, -0.0, host=dict(base, b=bnan), rmode="null", with_z=False)
