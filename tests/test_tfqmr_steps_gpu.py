"""mi355x_vec_tfqmr_qt, mi355x_vec_tfqmr_resid and mi355x_vec_tfqmr_update through the C ABI on guarded views: every written vector bit
for bit against the host model (tests/tfqmr_ref.py) and against the existing kernels run one call at a time (mi355x_vec_waxpy, _axpy,
_aypx); the sums of an aligned view carry the bits of mi355x_vec_norm(type 1) and mi355x_vec_dot over the op-by-op result; guard bands and
read-only operands keep their bits; a special case keeps the operand it skips out of every result; IEEE specials in live operands
propagate as in the op-by-op run; n == 0, missing and aliased arguments return as the header says."""
import math

import numpy as np
import pytest

import tfqmr_ref as tr
from vecspecials import bits, guarded, guards_intact, same, special_vector

pytestmark = pytest.mark.gpu

# 1023, 1024, 1025: one tile of 256 x 2 double2 (1024 doubles) and its edges; 4097: the first hand-off between workgroups of the
# reduction (16 doubles per lane: 4096 per workgroup); (1 << 21) + 1: beyond the 512-workgroup cap of the reduction's grid
SIZES = [1, 2, 3, 1023, 1024, 1025, 4097]
BIG = (1 << 21) + 1
POISON = 0x7FF8DEADBEEF0001
Q_OPS = ("u", "v", "q", "t", "x")
R_OPS = ("auq", "rp", "r")
U_OPS = ("d", "x", "u", "q", "r", "p")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def vec(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


def operands(n, names):
    return {name: vec(n, j + 1) for j, name in enumerate(names)}


class Run:
    """operands on the device in guarded views `off` doubles off a 16-byte boundary"""

    def __init__(self, dev, off, host):
        self.dev, self.host = dev, host
        self.g = {name: guarded(dev, a, off, tag=j + 1) for j, (name, a) in enumerate(host.items()) if a is not None}
        self.out = dev.put(np.array([POISON, POISON], dtype=np.uint64))

    def p(self, name):
        return self.g[name].ptr if name in self.g else None

    def sums(self):
        return self.dev.get(self.out, 2)

    def check_readonly(self, written):
        for name, g in self.g.items():
            if name not in written:
                assert np.array_equal(bits(g.get()), bits(self.host[name])), "operand %s changed" % name
        guards_intact(*self.g.values(), names=list(self.g))

    def free(self):
        for g in self.g.values():
            g.free()
        self.dev.free(self.out)


def compare(X, model, one, what):
    got = {name: X.g[name].get() for name in model}
    for name, v in got.items():
        same(v, model[name], "%s: %s against the model" % (what, name))
        same(v, one[name], "%s: %s against the kernels one by one" % (what, name))
    return got


# ------------------------------------------------------------------------------------------------ qt
def qt_op_by_op(dev, n, a, h, with_x):
    k = dev.k
    D = {name: dev.put(h[name]) for name in Q_OPS if name != "x" or with_x}
    dev.chk(k.mi355x_vec_waxpy(dev.h, n, -a, D["v"], D["u"], D["q"]))
    dev.chk(k.mi355x_vec_waxpy(dev.h, n, 1.0, D["u"], D["q"], D["t"]))
    if with_x:
        dev.chk(k.mi355x_vec_axpy(dev.h, n, a, D["t"], D["x"]))
    out = {name: dev.get(D[name], n) for name in ("q", "t") + (("x",) if with_x else ())}
    for p in D.values():
        dev.free(p)
    return out


def qt_case(dev, n, off, a=0.41, with_x=True, host=None):
    h = dict(host or operands(n, Q_OPS))
    h["q"], h["t"] = np.full(n, -3.0), np.full(n, -4.0)
    X = Run(dev, off, h)
    dev.chk(dev.k.mi355x_vec_tfqmr_qt(dev.h, n, a, X.p("u"), X.p("v"), X.p("q"), X.p("t"), X.p("x") if with_x else None))
    dev.sync()
    q, t, xn = tr.qt_ref(a, h["u"], h["v"], h["x"] if with_x else None)
    model = {"q": q, "t": t}
    written = {"q", "t"}
    if with_x and a != 0.0:
        model["x"] = xn
        written.add("x")
    got = compare(X, model, qt_op_by_op(dev, n, a, h, with_x), "qt n %d off %d a %r x %r" % (n, off, a, with_x))
    assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    X.check_readonly(written)
    X.free()
    return got


# ------------------------------------------------------------------------------------------------ resid
def check_sum(got, terms, ref, aligned, what):
    if aligned:
        same(got, ref, what + " against the separate reduction over the op-by-op vector")
        return
    if not np.all(np.isfinite(terms)):        # another walk over the same rounded terms: the margin scales with sum |terms|
        assert not np.isfinite(got), (got, "non-finite terms")
        return
    if np.max(np.abs(terms), initial=0.0) > 1e290:      # partial sums may overflow in one order and not in another: no margin to state
        return
    exact = math.fsum(terms)
    assert abs(got - exact) <= 1e-13 * math.fsum(np.abs(terms)), (what, got, exact)


def resid_op_by_op(dev, n, a, h):
    k = dev.k
    D = {name: dev.put(h[name]) for name in R_OPS}
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -a, D["auq"], D["r"]))
    dev.chk(k.mi355x_vec_norm(dev.h, n, 1, D["r"], dev.host_scratch()))
    rr = dev.scalar_out(1)[0]
    dev.chk(k.mi355x_vec_dot(dev.h, n, D["r"], D["rp"], dev.host_scratch()))
    rrp = dev.scalar_out(1)[0]
    r = dev.get(D["r"], n)
    for p in D.values():
        dev.free(p)
    return {"r": r}, rr, rrp


def resid_case(dev, n, off, a=0.41, host=None):
    h = dict(host or operands(n, R_OPS))
    X = Run(dev, off, h)
    dev.chk(dev.k.mi355x_vec_tfqmr_resid(dev.h, n, a, X.p("auq"), X.p("rp"), X.p("r"), X.out))
    dev.sync()
    one, rr, rrp = resid_op_by_op(dev, n, a, h)
    got = compare(X, {"r": tr.resid_ref(a, h["auq"], h["r"])}, one, "resid n %d off %d a %r" % (n, off, a))
    if a == 0.0:
        assert np.array_equal(bits(got["r"]), bits(h["r"])), "r touched with a == 0"
    s = X.sums()
    with np.errstate(all="ignore"):
        check_sum(s[0], one["r"] * one["r"], rr, off == 0, "r'r")
        check_sum(s[1], one["r"] * h["rp"], rrp, off == 0, "r'rp")
    X.check_readonly({"r"})
    X.free()
    return got["r"], s


# ------------------------------------------------------------------------------------------------ update
def update_op_by_op(dev, n, nhalves, cf0, eta0, cf1, eta1, tail, b, h):
    k = dev.k
    D = {name: dev.put(h[name]) for name in U_OPS}
    if nhalves >= 1:
        dev.chk(k.mi355x_vec_aypx(dev.h, n, cf0, D["u"], D["d"]))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, eta0, D["d"], D["x"]))
    if nhalves == 2:
        dev.chk(k.mi355x_vec_aypx(dev.h, n, cf1, D["q"], D["d"]))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, eta1, D["d"], D["x"]))
    if tail:
        dev.chk(k.mi355x_vec_waxpy(dev.h, n, b, D["q"], D["r"], D["u"]))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, b, D["p"], D["q"]))
        dev.chk(k.mi355x_vec_waxpy(dev.h, n, b, D["q"], D["u"], D["p"]))
    out = {name: dev.get(D[name], n) for name in U_OPS}
    for p in D.values():
        dev.free(p)
    return out


def update_case(dev, n, off, nhalves=2, cf0=0.83, eta0=-0.29, cf1=1.7, eta1=0.61, tail=True, b=0.47, host=None):
    h = dict(host or operands(n, U_OPS))
    X = Run(dev, off, h)
    dev.chk(dev.k.mi355x_vec_tfqmr_update(dev.h, n, nhalves, cf0, eta0, cf1, eta1, 1 if tail else 0, b,
                                          X.p("d"), X.p("x"), X.p("u"), X.p("q"), X.p("r"), X.p("p")))
    dev.sync()
    model = tr.update_ref(nhalves, cf0, eta0, cf1, eta1, tail, b, h["d"], h["x"], h["u"], h["q"], h["r"], h["p"])
    what = "update n %d off %d nhalves %d cf %r %r eta %r %r tail %r b %r" % (n, off, nhalves, cf0, cf1, eta0, eta1, tail, b)
    got = compare(X, model, update_op_by_op(dev, n, nhalves, cf0, eta0, cf1, eta1, tail, b, h), what)
    for name in U_OPS:                                   # what the form does not write keeps its bits (r never changes)
        if name not in model:
            assert np.array_equal(bits(X.g[name].get()), bits(h[name])), (what, name)
    if not ((nhalves >= 1 and eta0 != 0.0) or (nhalves == 2 and eta1 != 0.0)):
        assert np.array_equal(bits(X.g["x"].get()), bits(h["x"])), (what, "x touched")
    if tail and b == 0.0:
        assert np.array_equal(bits(X.g["q"].get()), bits(h["q"])), (what, "q touched")
    assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    X.check_readonly(set(model))
    X.free()
    return got


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_qt_forms(dev, n, off):
    for with_x in (False, True):
        for a in (0.41, 0.0, -0.0, 1.0, -1.0):
            qt_case(dev, n, off, a=a, with_x=with_x)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_resid_forms(dev, n, off):
    for a in (0.41, 0.0, -0.0, 1.0, -1.0):
        resid_case(dev, n, off, a=a)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_update_forms(dev, n, off):
    for nhalves in (0, 1, 2):
        for tail in (False, True):
            update_case(dev, n, off, nhalves=nhalves, tail=tail)
    for kw in (dict(cf0=0.0), dict(cf0=1.0), dict(cf0=-1.0), dict(cf1=0.0), dict(cf1=1.0), dict(cf1=-1.0), dict(cf0=-0.0, cf1=-0.0),
               dict(eta0=0.0), dict(eta1=0.0), dict(eta0=0.0, eta1=-0.0), dict(b=0.0), dict(b=-0.0), dict(b=1.0), dict(b=-1.0),
               dict(nhalves=1, eta0=0.0), dict(nhalves=1, cf0=0.0, tail=False), dict(nhalves=0, b=0.0), dict(nhalves=1, b=0.0)):
        update_case(dev, n, off, **kw)


def test_sweeps_beyond_the_grid_cap(dev):
    qt_case(dev, BIG, 0)
    resid_case(dev, BIG, 0)
    update_case(dev, BIG, 0)


@pytest.mark.parametrize("off", [0, 1])
def test_special_cases_keep_skipped_operands_out(dev, off):
    n = 1025
    nan = np.full(n, np.nan)
    qb = operands(n, Q_OPS)
    for with_x in (False, True):
        got = qt_case(dev, n, off, a=0.0, with_x=with_x, host=dict(qb, v=nan, x=nan.copy()))     # q = u: v is not loaded, x not touched
        assert np.all(np.isfinite(got["q"])) and np.all(np.isfinite(got["t"]))
    got = qt_case(dev, n, off, a=1.0, host=dict(qb, v=nan))                                       # -a == -1 skips nothing
    assert np.all(np.isnan(got["q"])) and np.all(np.isnan(got["x"]))
    rb = operands(n, R_OPS)
    r, s = resid_case(dev, n, off, a=0.0, host=dict(rb, auq=nan))
    assert np.all(np.isfinite(r)) and np.all(np.isfinite(s))
    r, s = resid_case(dev, n, off, a=-1.0, host=dict(rb, auq=nan))
    assert np.all(np.isnan(r)) and np.all(np.isnan(s))
    ub = operands(n, U_OPS)
    for kw, poisoned in ((dict(cf0=0.0), ("d",)), (dict(nhalves=1, cf0=-0.0, tail=False), ("d", "q", "r", "p")),
                         (dict(nhalves=0), ("d", "x")), (dict(nhalves=0, b=0.0), ("d", "x", "p")), (dict(nhalves=1, b=0.0), ("p",)),
                         (dict(tail=False), ("r", "p")), (dict(nhalves=1, tail=False), ("q", "r", "p")), (dict(nhalves=0, tail=False), U_OPS)):
        got = update_case(dev, n, off, host=dict(ub, **{name: nan.copy() for name in poisoned}), **kw)
        assert all(np.all(np.isfinite(v)) for v in got.values()), (kw, poisoned)
    got = update_case(dev, n, off, eta0=0.0, eta1=-0.0, host=dict(ub, x=nan))                     # x neither read nor written
    assert np.all(np.isfinite(got["d"])) and np.all(np.isnan(got["x"]))
    got = update_case(dev, n, off, b=0.0, host=dict(ub, p=nan))                                   # VecAXPY(Q, 0, P) skipped, p = u copied over it
    assert np.all(np.isfinite(got["p"])) and np.all(np.isfinite(got["u"]))
    got = update_case(dev, n, off, nhalves=1, b=0.0, host=dict(ub, q=nan))                        # b == 0 copies: q is not loaded and keeps its NaNs
    assert all(np.all(np.isfinite(got[name])) for name in ("d", "x", "u", "p")) and np.all(np.isnan(got["q"]))
    got = update_case(dev, n, off, cf0=1.0, host=dict(ub, d=nan))                               # cf == 1 skips the multiply, not the operand
    assert np.all(np.isnan(got["d"])) and np.all(np.isnan(got["x"]))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [3, 1025])
def test_ieee_specials_in_live_operands(dev, n, off):
    """Inf, NaN, -0, denormals in every operand in turn: compared by position for NaNs and by bits elsewhere"""
    qb, rb, ub = operands(n, Q_OPS), operands(n, R_OPS), operands(n, U_OPS)
    for rot in (0, 7):
        for j, name in enumerate(("u", "v", "x")):
            host = dict(qb, **{name: special_vector(n, 31 + j, 0.25, rot)})
            qt_case(dev, n, off, host=host)
            qt_case(dev, n, off, a=-0.0 if rot else 1.0, host=host)
        for j, name in enumerate(R_OPS):
            host = dict(rb, **{name: special_vector(n, 41 + j, 0.25, rot)})
            resid_case(dev, n, off, host=host)
            resid_case(dev, n, off, a=0.0 if rot else -1.0, host=host)
        for j, name in enumerate(U_OPS):
            host = dict(ub, **{name: special_vector(n, 51 + j, 0.25, rot)})
            update_case(dev, n, off, host=host)
            update_case(dev, n, off, cf0=0.0, b=1.0, host=host)
            update_case(dev, n, off, nhalves=1, eta0=0.0, b=0.0, host=host)
    for a in (np.inf, np.nan):
        qt_case(dev, n, off, a=a)
        resid_case(dev, n, off, a=a)
    update_case(dev, n, off, cf0=np.inf)
    update_case(dev, n, off, eta1=np.nan)
    update_case(dev, n, off, b=np.nan)


def test_empty_vectors_and_bad_arguments(dev):
    poison = np.array([POISON, POISON], dtype=np.uint64)
    out = dev.put(poison)
    q = [dev.put(np.full(8, 5.0)) for _ in range(6)]
    k = dev.k

    def untouched():
        dev.sync()
        assert np.array_equal(dev.get(out, 2).view(np.uint64), poison), "a refused call touched out"
        for p in q:
            assert np.array_equal(dev.get(p, 8), np.full(8, 5.0)), "a refused call touched a vector"

    dev.chk(k.mi355x_vec_tfqmr_qt(dev.h, 0, 0.4, q[0], q[1], q[2], q[3], q[4]))
    dev.chk(k.mi355x_vec_tfqmr_update(dev.h, 0, 2, 0.8, 0.3, 1.7, 0.6, 1, 0.5, *q))
    dev.chk(k.mi355x_vec_tfqmr_update(dev.h, 8, 0, 0.8, 0.3, 1.7, 0.6, 0, 0.5, None, None, None, None, None, None))   # nothing to do
    untouched()
    dev.chk(k.mi355x_vec_tfqmr_resid(dev.h, 0, 0.4, q[0], q[1], q[2], out)); dev.sync()
    assert np.array_equal(bits(dev.get(out, 2)), bits(np.zeros(2)))                  # n == 0: zeros
    dev.chk(k.mi355x_memcpy_h2d(dev.h, out, poison.ctypes.data, 16)); dev.sync()
    for missing in range(4):                                                          # x may be missing (TFQMR), nothing else
        a = list(q[:5]); a[missing] = None
        assert k.mi355x_vec_tfqmr_qt(dev.h, 8, 0.4, *a) != 0
    for missing in range(4):
        a = [q[0], q[1], q[2], out]; a[missing] = None
        assert k.mi355x_vec_tfqmr_resid(dev.h, 8, 0.4, *a) != 0
    for missing in range(6):
        a = list(q); a[missing] = None
        assert k.mi355x_vec_tfqmr_update(dev.h, 8, 2, 0.8, 0.3, 1.7, 0.6, 1, 0.5, *a) != 0
    for nhalves in (-1, 3):
        assert k.mi355x_vec_tfqmr_update(dev.h, 8, nhalves, 0.8, 0.3, 1.7, 0.6, 1, 0.5, *q) != 0
    # a written vector that is another operand of the call
    assert k.mi355x_vec_tfqmr_qt(dev.h, 8, 0.4, q[0], q[1], q[0], q[3], q[4]) != 0
    assert k.mi355x_vec_tfqmr_qt(dev.h, 8, 0.4, q[0], q[1], q[2], q[1], q[4]) != 0
    assert k.mi355x_vec_tfqmr_qt(dev.h, 8, 0.4, q[0], q[1], q[2], q[2], None) != 0
    assert k.mi355x_vec_tfqmr_qt(dev.h, 8, 0.4, q[0], q[1], q[2], q[3], q[0]) != 0
    assert k.mi355x_vec_tfqmr_resid(dev.h, 8, 0.4, q[2], q[1], q[2], out) != 0
    assert k.mi355x_vec_tfqmr_resid(dev.h, 8, 0.4, q[0], q[2], q[2], out) != 0
    for i, j in ((0, 1), (0, 2), (1, 3), (2, 4), (3, 5), (2, 3), (4, 5)):
        a = list(q); a[j] = a[i]
        assert k.mi355x_vec_tfqmr_update(dev.h, 8, 2, 0.8, 0.3, 1.7, 0.6, 1, 0.5, *a) != 0
    untouched()
    # the forms that leave operands out accept NULL there
    dev.chk(k.mi355x_vec_tfqmr_update(dev.h, 8, 0, 0.0, 0.0, 0.0, 0.0, 1, 2.0, None, None, q[2], q[3], q[4], q[5])); dev.sync()
    assert np.array_equal(dev.get(q[2], 8), np.full(8, 15.0)) and np.array_equal(dev.get(q[3], 8), np.full(8, 15.0))
    assert np.array_equal(dev.get(q[5], 8), np.full(8, 45.0))
    dev.chk(k.mi355x_vec_tfqmr_update(dev.h, 8, 1, 2.0, 1.0, 0.0, 0.0, 0, 0.0, q[0], q[1], q[2], None, None, None)); dev.sync()
    assert np.array_equal(dev.get(q[0], 8), np.full(8, 25.0)) and np.array_equal(dev.get(q[1], 8), np.full(8, 30.0))
    for p in q:
        dev.free(p)
    dev.free(out)
