"""mi355x_vec_sum / _shift / _shift_dev / _max / _min through the C ABI, operands in guarded views (vecspecials.Guarded), aligned and
one double off.  Sizes: 4096 is the largest that fits one workgroup, 4097 the first that takes the hand-off between workgroups,
(1 << 21) + 1 the first beyond the cap of 512 workgroups.

sum: the bits of the oracle's device-order dot(x, ones) and of mi355x_vec_dot(x, ones) where the view is 16-byte aligned; the
unaligned view runs the scalar grid-stride loop, another fixed tree, and is held to the suite's 1e-13 * sum|x|.
max / min: value bits and location of a sequential loop that restates VecMax_Seq / VecMin_Seq (start from x[0], replace on a strict
comparison)."""
import ctypes as C

import numpy as np
import pytest

import orc
import vecspecials as vs
from vecspecials import Guarded, guards_intact

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 257, 4095, 4096, 4097, 8193, (1 << 21) + 1]
INF, NAN = np.inf, np.nan


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


@pytest.fixture(scope="module")
def data():
    """one random vector per size, shared and left unchanged"""
    rng = np.random.default_rng(7)
    return {n: rng.standard_normal(n) for n in SIZES}


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a), dtype=np.float64).view(np.uint64)


def result(dev, count):
    return dev.scalar_out(count)


def dev_sum(dev, g):
    dev.chk(dev.k.mi355x_vec_sum(dev.h, g.n, g.ptr, dev.host_scratch()))
    return result(dev, 1)[0]


def unchanged(g):
    assert np.array_equal(bits(g.get()), bits(g.host)), "a read-only operand was written"
    guards_intact(g)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_sum_has_the_bits_of_dot_with_ones(dev, data, n, off):
    x = data[n]
    g, ones = Guarded(dev, n, off, 1).load(x), Guarded(dev, n, off, 2).load(np.ones(n))
    s = dev_sum(dev, g)
    dev.chk(dev.k.mi355x_vec_dot(dev.h, n, g.ptr, ones.ptr, dev.host_scratch()))
    d = result(dev, 1)[0]
    assert bits(s)[0] == bits(d)[0], (s, d)
    with orc.device_reduction_order():
        ref = float(orc.vec_dot(x, np.ones(n)))
    if off == 0:
        assert bits(s)[0] == bits(ref)[0], (s, ref)
    else:
        assert abs(s - ref) <= 1e-13 * np.sum(np.abs(x))
    unchanged(g); unchanged(ones)
    g.free(); ones.free()


@pytest.mark.parametrize("n", [3, 4097, 8193])
def test_sum_of_non_finite_data(dev, data, n):
    for off in (0, 1):
        for pokes, want in (((0, INF),), "+inf"), (((n - 1, -INF),), "-inf"), (((0, INF), (n - 1, -INF)), "nan"), (((n // 2, NAN),), "nan"):
            g = Guarded(dev, n, off, 3).load(data[n])
            for i, v in pokes:
                g.poke(i, v)
            s = dev_sum(dev, g)
            got = "nan" if np.isnan(s) else ("+inf" if s == INF else ("-inf" if s == -INF else "finite"))
            assert got == want, (n, off, pokes, s)
            unchanged(g)
            g.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_shift_is_x_plus_a(dev, data, n, off):
    x = data[n].copy()
    x[0] = -0.0
    for a in (0.0, -0.0, 1.5, INF, NAN):
        g = Guarded(dev, n, off, 4).load(x)
        dev.chk(dev.k.mi355x_vec_shift(dev.h, n, C.c_double(a), g.ptr))
        dev.sync()
        with np.errstate(all="ignore"):
            vs.same(g.get(), x + a, "shift by %r" % a)
        guards_intact(g)
        g.free()


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_shift_dev_forms_the_quotient_of_the_kernel_sum(dev, data, n, off):
    x = data[n]
    slot = dev.alloc(16)
    for den in (-1.0 * n, 3.0):
        g = Guarded(dev, n, off, 5).load(x)
        dev.chk(dev.k.mi355x_vec_sum(dev.h, n, g.ptr, slot))           # the sum stays on the device
        dev.chk(dev.k.mi355x_vec_shift_dev(dev.h, n, slot, C.c_double(den), g.ptr))
        dev.sync()
        s = dev.get(slot, 1)[0]
        assert np.array_equal(bits(g.get()), bits(x + (s / den))), den
        guards_intact(g)
        g.free()
    dev.free(slot)


def seq_extremum(x, is_max):
    """VecMax_Seq / VecMin_Seq (dvec2.c): from x[0], replaced on a strict > (<)"""
    if x.size == 0:
        return (-1.7976931348623157e308 if is_max else 1.7976931348623157e308), -1
    v, j = x[0], 0
    for i in range(1, x.size):
        if (x[i] > v) if is_max else (x[i] < v):
            v, j = x[i], i
    return v, j


def np_extremum(x, is_max):
    """the same answer without a Python loop, for the large sizes (checked against seq_extremum below)"""
    if np.isnan(x[0]):
        return x[0], 0
    y = np.where(np.isnan(x), -INF if is_max else INF, x)
    j = int(np.argmax(y) if is_max else np.argmin(y))
    if np.isnan(x[j]):                              # nothing but NaN after a finite x[0] that is -inf (max) / +inf (min)
        j = 0
    return x[j], j


def check_extremum(dev, x, off, what=""):
    g = Guarded(dev, x.size, off, 6).load(x)
    for is_max, fn in ((True, dev.k.mi355x_vec_max), (False, dev.k.mi355x_vec_min)):
        dev.chk(fn(dev.h, x.size, g.ptr, dev.host_scratch()))
        v, loc = result(dev, 2)
        rv, rj = seq_extremum(x, is_max) if x.size <= 8193 else np_extremum(x, is_max)
        assert loc == float(rj), (what, is_max, loc, rj)
        assert bits(v)[0] == bits(rv)[0] or (np.isnan(v) and np.isnan(rv)), (what, is_max, v, rv)
    unchanged(g)
    g.free()


def test_vectorised_reference_is_the_sequential_loop():
    rng = np.random.default_rng(3)
    for trial in range(200):
        x = rng.integers(-2, 3, size=rng.integers(1, 9)).astype(np.float64)
        x[rng.random(x.size) < 0.2] = NAN
        x[rng.random(x.size) < 0.1] = -0.0
        for is_max in (True, False):
            a, b = seq_extremum(x, is_max), np_extremum(x, is_max)
            assert a[1] == b[1] and (bits(a[0])[0] == bits(b[0])[0] or (np.isnan(a[0]) and np.isnan(b[0]))), (x, is_max, a, b)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_max_min_are_the_reference_loop(dev, data, n, off):
    x = data[n]
    check_extremum(dev, x, off, "random")
    check_extremum(dev, np.full(n, 2.5), off, "all equal")
    if n >= 2:
        z = np.zeros(n); z[0] = -0.0
        check_extremum(dev, z, off, "-0.0 before +0.0")
        z = np.zeros(n); z[1:] = -0.0
        check_extremum(dev, z, off, "+0.0 before -0.0")
        y = x.copy(); y[0] = NAN
        check_extremum(dev, y, off, "NaN at 0")
        y = x.copy(); y[n - 1] = NAN; y[n // 2] = NAN
        check_extremum(dev, y, off, "NaN elsewhere")
        y = x.copy(); y[n // 3] = INF; y[n - 1] = -INF
        check_extremum(dev, y, off, "infinities")
    if n == 2:
        check_extremum(dev, np.array([1.0, NAN]), off, "NaN the only other element")
        check_extremum(dev, np.array([NAN, 1.0]), off, "NaN first of two")
    if n > 4096:
        # the extremum twice, in two different workgroups (lane t of workgroup b meets double2's b * 256 + t, ...): the lowest index wins
        y = x.copy()
        lo, hi = 300, n - 2
        y[lo] = y[hi] = 9.0
        y[lo + 1] = y[hi - 1] = -9.0
        check_extremum(dev, y, off, "duplicated across workgroups")


def test_no_entries_through_the_vec_type(built):
    from petsc_dev_amd import petsc as P
    v = P.Vec.create(0, comm=P.lib().COMM_SELF)
    assert v.max() == (-1, -1.7976931348623157e308)
    assert v.min() == (-1, 1.7976931348623157e308)
    assert v.sum() == 0.0
