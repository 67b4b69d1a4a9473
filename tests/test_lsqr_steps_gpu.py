"""mi355x_vec_lsqr_bidiag and mi355x_vec_lsqr_update through the C ABI on guarded views: every written vector bit for bit against the host
model (tests/lsqr_ref.py) and against the existing kernels run one call at a time (mi355x_vec_axpy, _norm, _scale, _copy,
_pointwise_mult, _aypx); the sum of an aligned view carries the bits of mi355x_vec_norm(type 2) over the op-by-op result; the host
coefficient and the one rooted on the device from a slot agree, the root against numpy.sqrt on bits; guard bands and read-only operands
keep their bits; a special case keeps the operand it skips out of every result; IEEE specials in live operands propagate as in the
op-by-op run."""
import math

import numpy as np
import pytest

import lsqr_ref as lr
from vecspecials import bits, guarded, guards_intact, same, special_vector

pytestmark = pytest.mark.gpu

# 1023, 1024, 1025: one tile of 256 x 2 double2 (1024 doubles) and its edges; 4097: the first hand-off between workgroups of the
# reduction (16 doubles per lane: 4096 per workgroup); (1 << 21) + 1: beyond the 512-workgroup cap of the reduction's grid
SIZES = [1, 2, 3, 1023, 1024, 1025, 4097]
BIG = (1 << 21) + 1
POISON = 0x7FF8DEADBEEF0001
U_OPS = ("v1", "x", "w", "se")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def vec(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


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
                assert np.array_equal(bits(g.get()), bits(self.host[name])), "read-only operand %s changed" % name
        guards_intact(*self.g.values(), names=list(self.g))

    def free(self):
        for g in self.g.values():
            g.free()
        self.dev.free(self.out)


def bidiag_op_by_op(dev, n, coef, h):
    """mi355x_vec_axpy and mi355x_vec_norm(type 2) on plain allocations: the new y and the sum"""
    k = dev.k
    dx, dy = dev.put(h["x"]), dev.put(h["y"])
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -coef, dx, dy))
    dev.chk(k.mi355x_vec_norm(dev.h, n, 2, dy, dev.host_scratch()))
    s = dev.scalar_out(1)[0]
    y = dev.get(dy, n)
    dev.free(dx); dev.free(dy)
    return y, s


def check_sum(got, terms, ref, aligned):
    if aligned:
        same(got, ref, "the sum against mi355x_vec_norm(type 2) over the op-by-op vector")
        return
    if not np.all(np.isfinite(terms)):        # another walk over the same rounded terms: the margin scales with sum |terms|
        assert not np.isfinite(got), (got, "non-finite terms")
        return
    if np.max(np.abs(terms), initial=0.0) > 1e290:      # partial sums may overflow in one order and not in another: no margin to state
        return
    exact = math.fsum(terms)
    assert abs(got - exact) <= 1e-13 * math.fsum(np.abs(terms)), (got, exact)


def bidiag_case(dev, n, off, coef=0.41, host=None):
    """one launch per coefficient route, every check; returns (y, sum)"""
    h = dict(host or {"x": vec(n, 1), "y": vec(n, 2)})
    routes = ["host"]
    coef2 = None
    if coef >= 0.0 and np.isfinite(coef):                             # a root can come from a slot: the coefficient of the whole case IS
        coef2 = np.array([coef]) ** 2                                 # numpy's root of the double the slot holds, so both routes run
        coef = float(np.sqrt(coef2)[0])
        routes.append("device")
    model, _ = lr.bidiag_ref(coef, h["x"], h["y"])
    one, s1 = bidiag_op_by_op(dev, n, coef, h)
    got = None
    for route in routes:
        X = Run(dev, off, h)
        slot = dev.put(coef2) if route == "device" else None
        host_coef = coef if route == "host" else 1234.5                # ignored when the coefficient comes from the slot
        dev.chk(dev.k.mi355x_vec_lsqr_bidiag(dev.h, n, host_coef, slot, X.p("x"), X.p("y"), X.out))
        dev.sync()
        y = X.g["y"].get()
        same(y, model, "y against the model (%s coefficient)" % route)
        same(y, one, "y against the kernels one by one (%s coefficient)" % route)
        if coef == 0.0:
            assert np.array_equal(bits(y), bits(h["y"])), "y touched with coef == 0"
        s = X.sums()
        with np.errstate(all="ignore"):
            check_sum(s[0], one * one, s1, off == 0)
        assert bits(s[1:])[0] == POISON, "more than one double written to out"
        if got is not None:
            assert bits(got[1]) == bits(s[0]) or np.isnan(s[0]), "the two coefficient routes differ in the sum"
        X.check_readonly({"y"})
        X.free()
        if slot is not None:
            dev.free(slot)
        got = (y, s[0])
    assert len(routes) == 2 or not (coef >= 0.0 and np.isfinite(coef)), "a coefficient that could come from a slot ran on the host route only"
    return got


def update_op_by_op(dev, n, ialpha, step, cf, irho2, skip_w, with_se, h):
    k = dev.k
    D = {name: dev.put(h[name]) for name in U_OPS}
    dev.chk(k.mi355x_vec_scale(dev.h, n, ialpha, D["v1"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, step, D["w"], D["x"]))
    if with_se:
        w2 = dev.alloc(8 * max(n, 2))
        dev.chk(k.mi355x_vec_copy(dev.h, n, D["w"], w2))
        dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, w2, w2, w2))
        dev.chk(k.mi355x_vec_scale(dev.h, n, irho2, w2))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, 1.0, w2, D["se"]))
        dev.free(w2)
    if not skip_w:
        dev.chk(k.mi355x_vec_aypx(dev.h, n, cf, D["v1"], D["w"]))
    out = {name: dev.get(D[name], n) for name in U_OPS}
    for q in D.values():
        dev.free(q)
    return out


def update_case(dev, n, off, ialpha=2.3, step=0.61, cf=-0.83, irho2=1.7, skip_w=False, with_se=True, host=None):
    h = dict(host or {name: vec(n, j + 1) for j, name in enumerate(U_OPS)})
    X = Run(dev, off, h)
    dev.chk(dev.k.mi355x_vec_lsqr_update(dev.h, n, ialpha, step, cf, irho2, 1 if skip_w else 0, X.p("v1"), X.p("x"), X.p("w"), X.p("se") if with_se else None))
    dev.sync()
    v1, x, w, se = lr.update_ref(ialpha, step, cf, irho2, skip_w, h["v1"], h["x"], h["w"], h["se"] if with_se else None)
    model = {"v1": v1, "x": x, "w": w, "se": se if with_se else h["se"]}
    one = update_op_by_op(dev, n, ialpha, step, cf, irho2, skip_w, with_se, h)
    got = {name: X.g[name].get() for name in U_OPS}
    for name, v in got.items():
        same(v, model[name], "%s against the model" % name)
        same(v, one[name], "%s against the kernels one by one" % name)
    untouched = [name for name, cond in (("x", step == 0.0), ("se", not with_se), ("w", skip_w), ("v1", ialpha == 1.0)) if cond]
    for name in untouched:
        assert np.array_equal(bits(got[name]), bits(h[name])), "%s touched" % name
    assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    X.check_readonly(set(U_OPS) - set(untouched))
    X.free()
    return got


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_bidiag_forms(dev, n, off):
    for coef in (0.41, 0.0, -0.0, 1.0, -1.3, 0.75, float(np.sqrt(np.float64(0.3))), float(np.sqrt(np.float64(7.0)))):
        bidiag_case(dev, n, off, coef=coef)


def test_the_root_of_the_slot_is_numpys(dev):
    """y = 0, x = 1: the updated y is -sqrt(slot) everywhere, bit for bit numpy's correctly rounded root"""
    n = 8
    for v in (2.0, 0.3, 1e-300, 5e-324, 1.7976931348623157e308, 0.1 + 0.2, 4.0, float(np.nextafter(1.0, 2.0))):
        slot = dev.put(np.array([v]))
        dx, dy, out = dev.put(np.ones(n)), dev.put(np.zeros(n)), dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_lsqr_bidiag(dev.h, n, 99.0, slot, dx, dy, out))
        y = dev.get(dy, n)
        assert np.array_equal(bits(y), bits(np.full(n, 0.0 + (-np.sqrt(np.float64(v))) * 1.0))), (v, y[0])
        for p in (slot, dx, dy, out):
            dev.free(p)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_update_forms(dev, n, off):
    update_case(dev, n, off)
    for kw in (dict(ialpha=0.0), dict(ialpha=1.0), dict(step=0.0), dict(step=-0.0), dict(cf=0.0), dict(cf=1.0), dict(cf=-1.0), dict(with_se=False),
               dict(irho2=0.0), dict(irho2=1.0), dict(skip_w=True), dict(skip_w=True, ialpha=1.0), dict(skip_w=True, ialpha=1.0, with_se=False),
               dict(skip_w=True, step=0.0, with_se=False), dict(ialpha=0.0, cf=0.0), dict(ialpha=1.0, step=0.0, with_se=False)):
        update_case(dev, n, off, **kw)


def test_sweeps_beyond_the_grid_cap(dev):
    bidiag_case(dev, BIG, 0, coef=0.75)
    update_case(dev, BIG, 0)


@pytest.mark.parametrize("off", [0, 1])
def test_special_cases_keep_skipped_operands_out(dev, off):
    n = 1025
    nan = np.full(n, np.nan)
    y, s = bidiag_case(dev, n, off, coef=0.0, host={"x": nan, "y": vec(n, 2)})
    assert np.all(np.isfinite(y)) and np.isfinite(s)
    y, s = bidiag_case(dev, n, off, coef=0.41, host={"x": nan, "y": vec(n, 2)})            # a live x: the NaN must arrive
    assert np.all(np.isnan(y)) and np.isnan(s)
    ub = {name: vec(n, j + 1) for j, name in enumerate(U_OPS)}
    # (the form, the operands it neither loads nor stores: NaN there stays there and reaches nothing else)
    for kw, poisoned, stays in ((dict(ialpha=0.0), ("v1",), ()), (dict(skip_w=True, ialpha=1.0), ("v1",), ("v1",)),
                                (dict(skip_w=True, step=0.0, with_se=False), ("w", "x", "se"), ("w", "x", "se")),
                                (dict(cf=0.0, step=0.0, with_se=False), ("w", "x", "se"), ("x", "se"))):
        got = update_case(dev, n, off, host=dict(ub, **{name: nan.copy() for name in poisoned}), **kw)
        for name in U_OPS:
            assert np.all(np.isnan(got[name])) if name in stays else np.all(np.isfinite(got[name])), (kw, name)
    got = update_case(dev, n, off, step=0.0, host=dict(ub, x=nan))                          # x neither read nor written: its NaN stays where it is
    assert np.all(np.isfinite(got["w"])) and np.all(np.isnan(got["x"]))
    got = update_case(dev, n, off, ialpha=1.0, host=dict(ub, v1=nan))                       # ialpha == 1 skips the store, not the operand
    assert np.all(np.isnan(got["w"]))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [3, 1025])
def test_ieee_specials_in_live_operands(dev, n, off):
    """Inf, NaN, -0, denormals in every operand in turn: compared by position for NaNs and by bits elsewhere"""
    for j, name in enumerate(("x", "y")):
        for rot in (0, 7):
            host = {"x": vec(n, 1), "y": vec(n, 2)}
            host[name] = special_vector(n, 31 + j, 0.25, rot)
            bidiag_case(dev, n, off, host=host)
            bidiag_case(dev, n, off, coef=-0.0 if rot else 1.0, host=host)
    ub = {name: vec(n, j + 1) for j, name in enumerate(U_OPS)}
    for j, name in enumerate(U_OPS):
        for rot in (0, 7):
            host = dict(ub, **{name: special_vector(n, 51 + j, 0.25, rot)})
            update_case(dev, n, off, host=host)
            update_case(dev, n, off, ialpha=1.0, cf=0.0, host=host)
            update_case(dev, n, off, skip_w=True, cf=1.0, host=host)
    for coef in (np.inf, np.nan):
        bidiag_case(dev, n, off, coef=coef)
    update_case(dev, n, off, ialpha=np.inf)
    update_case(dev, n, off, step=np.nan)
    update_case(dev, n, off, irho2=np.inf)


def test_empty_vectors_and_bad_arguments(dev):
    poison = np.array([POISON, POISON], dtype=np.uint64)
    out = dev.put(poison)
    q = [dev.put(np.full(8, 5.0)) for _ in range(4)]
    k = dev.k
    dev.chk(k.mi355x_vec_lsqr_bidiag(dev.h, 0, 0.41, None, q[0], q[1], out)); dev.sync()
    got = dev.get(out, 2)
    assert bits(got)[0] == bits(np.array([0.0]))[0] and bits(got)[1] == POISON          # n == 0: { 0 }
    dev.chk(k.mi355x_memcpy_h2d(dev.h, out, poison.ctypes.data, 16)); dev.sync()
    dev.chk(k.mi355x_vec_lsqr_update(dev.h, 0, 2.3, 0.6, -0.8, 1.7, 0, *q)); dev.sync()
    assert k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.41, None, None, q[1], out) != 0          # a live x missing
    assert k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.0, out, None, q[1], out) != 0            # the slot route always reads x
    assert k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.41, None, q[0], None, out) != 0
    assert k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.41, None, q[0], q[1], None) != 0
    assert k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.41, None, q[1], q[1], out) != 0          # the written vector is the other operand
    for missing in range(3):
        a = list(q); a[missing] = None
        assert k.mi355x_vec_lsqr_update(dev.h, 8, 2.3, 0.6, -0.8, 1.7, 0, *a) != 0
    for flag in (-1, 2, 7):
        assert k.mi355x_vec_lsqr_update(dev.h, 8, 2.3, 0.6, -0.8, 1.7, flag, *q) != 0
    for i in range(4):
        for j in range(i + 1, 4):
            a = list(q); a[j] = a[i]
            assert k.mi355x_vec_lsqr_update(dev.h, 8, 2.3, 0.6, -0.8, 1.7, 0, *a) != 0, (i, j)
    assert k.mi355x_vec_lsqr_update(dev.h, 8, 1.0, 0.6, -0.8, 1.7, 1, None, q[1], None, None) != 0   # x steps along w: w missing
    dev.sync()
    assert np.array_equal(dev.get(out, 2).view(np.uint64), poison), "a refused call touched out"
    for p in q:
        assert np.array_equal(dev.get(p, 8), np.full(8, 5.0)), "a refused call touched a vector"
    dev.chk(k.mi355x_vec_lsqr_bidiag(dev.h, 8, 0.0, None, None, q[1], out)); dev.sync()  # coef == 0: x may be missing
    assert dev.get(out, 1)[0] == 8 * 25.0
    dev.chk(k.mi355x_vec_lsqr_update(dev.h, 8, 2.0, 0.0, 0.0, 0.0, 1, q[0], None, None, None)); dev.sync()   # the plain scaling form
    assert np.array_equal(dev.get(q[0], 8), np.full(8, 10.0))
    for p in q:
        dev.free(p)
    dev.free(out)
