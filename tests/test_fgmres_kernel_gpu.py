"""mi355x_vec_scale_rnorm_dev_pmult through the C ABI against numpy, bit for bit (any NaN equals any NaN, vecspecials.same): x scaled by
1 / sqrt(*norm2_dev) under mi355x_vec_scale_rnorm_dev's rules and z = d .* x_new (d NULL: z = x_new) from the same pass.  Sizes around
the tile of 256 x 2 double2's and its edge cases, every operand one double off 16-byte alignment in turn (the scalar path), the norm slot's
special values, IEEE specials inside x and d, 64-double guard bands around x and z, and the refusals.

The norm slot holds the SQUARE of the norm, so a subnormal slot value has a normal root (sqrt(5e-324) = 2.2e-162) and alpha stays finite
(4.5e161): alpha cannot overflow to inf through this entry point.  The subnormal slot is tested for what numpy computes from it."""
import ctypes as C

import numpy as np
import pytest

from vecspecials import same

pytestmark = pytest.mark.gpu

GUARD = 64
SIZES = [0, 1, 2, 3, 255, 256, 257, 1023, 1025, 4099]
SLOTS = [0.0, 1.0, 4.0, 5e-324, np.inf, np.nan, 0.731]


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def reference(norm2, x, d):
    """(x_new, z, stored): VecNormalize's and VecScale's rules, then VecPointwiseMult(z, x_new, d) or VecCopy"""
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float64(norm2))
        alpha = np.float64(1.0) / nrm
        stored = not (nrm == 0.0 or nrm == 1.0 or alpha == 1.0)
        xn = x.copy() if not stored else (np.zeros_like(x) if alpha == 0.0 else x * alpha)
        z = xn * d if d is not None else xn.copy()
    return xn, z, stored


class Banded:
    """n doubles on the device between two guard bands of GUARD doubles, the view `off` doubles past a 16-byte boundary"""

    def __init__(self, dev, a, off, fill):
        self.dev, self.n, self.off = dev, a.size, off
        self.host = np.full(GUARD + off + a.size + GUARD, fill)
        self.host[GUARD + off:GUARD + off + a.size] = a
        self.base = dev.put(self.host)
        self.ptr = C.c_void_p(self.base.value + 8 * (GUARD + off))

    def read(self):
        """(the view, True when both guard bands and the slack in front of the view are as they were)"""
        got = self.dev.get(self.base, self.host.size)
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        return got[lo:hi], bool(np.array_equal(got[:lo].view(np.uint64), self.host[:lo].view(np.uint64))
                                and np.array_equal(got[hi:].view(np.uint64), self.host[hi:].view(np.uint64)))

    def free(self):
        self.dev.free(self.base)


def operands(n, specials):
    rng = np.random.default_rng(4200 + n)
    x, d = rng.standard_normal(n), rng.uniform(0.5, 2.0, n)
    if n:
        x[0] = -0.0
    if specials and n >= 3:
        x[1], d[2] = np.nan, np.inf                              # different entries: which payload a NaN * NaN keeps is the hardware's business
        x[n - 1] = np.inf
        if n >= 256:
            d[200], x[n // 2] = np.nan, -np.inf
    return x, d


def run(dev, n, slot, with_d, offs, specials=False):
    x, d = operands(n, specials)
    X, Z = Banded(dev, x, offs[0], 7.25), Banded(dev, np.full(n, -3.5), offs[1], 9.5)
    D = Banded(dev, d, offs[2], 1.0) if with_d else None
    dn = dev.put(np.array([slot]))
    dev.chk(dev.k.mi355x_vec_scale_rnorm_dev_pmult(dev.h, n, dn, X.ptr, D.ptr if D else None, Z.ptr))
    dev.sync()
    xn, z, stored = reference(slot, x, d if with_d else None)
    gx, xband = X.read()
    gz, zband = Z.read()
    what = "n %d slot %r d %s offsets %r" % (n, slot, with_d, offs)
    assert xband and zband, "guard band touched: " + what
    if stored:
        same(gx, xn, "x " + what)
    else:
        assert np.array_equal(gx.view(np.uint64), x.view(np.uint64)), "x must stay as it was: " + what
    same(gz, z, "z " + what)
    if D:
        gd, dband = D.read()
        assert dband and np.array_equal(gd.view(np.uint64), d.view(np.uint64)), "d touched: " + what
        D.free()
    for b in (X, Z):
        b.free()
    dev.free(dn)


@pytest.mark.parametrize("n", SIZES)
def test_against_numpy_over_slots_and_alignments(dev, n):
    """aligned operands for every slot value, with and without d; x, z, d one double off alignment in turn for the scaling slot 4, the
    not-stored slot 1 and the zero-storing slot inf"""
    for with_d in (True, False):
        for slot in SLOTS:
            run(dev, n, slot, with_d, (0, 0, 0))
        for offs in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            if offs[2] and not with_d:
                continue
            for slot in (4.0, 1.0, np.inf):
                run(dev, n, slot, with_d, offs)


@pytest.mark.parametrize("n", [3, 257, 1025])
def test_specials_inside_x_and_d(dev, n):
    for with_d in (True, False):
        for slot in (4.0, 1.0, 0.0, np.inf, np.nan, 5e-324):
            run(dev, n, slot, with_d, (0, 0, 0), specials=True)
        run(dev, n, 4.0, with_d, (1, 0, 0), specials=True)


def test_refusals_touch_nothing(dev):
    """z == x, z == d, d == x, a NULL x, z or norm slot: hipErrorInvalidValue, every operand as it was"""
    k, n = dev.k, 300
    x, d = operands(n, False)
    X, Z, D = Banded(dev, x, 0, 7.25), Banded(dev, np.full(n, -3.5), 0, 9.5), Banded(dev, d, 0, 1.0)
    dn = dev.put(np.array([4.0]))
    bad = [(dn, X.ptr, D.ptr, X.ptr), (dn, X.ptr, D.ptr, D.ptr), (dn, X.ptr, X.ptr, Z.ptr), (dn, None, D.ptr, Z.ptr), (dn, X.ptr, D.ptr, None),
           (dn, X.ptr, None, X.ptr), (None, X.ptr, D.ptr, Z.ptr)]
    for args in bad:
        assert k.mi355x_vec_scale_rnorm_dev_pmult(dev.h, n, *args) == 1, args        # hipErrorInvalidValue
        assert k.mi355x_vec_scale_rnorm_dev_pmult(dev.h, 0, *args) == 1, args        # refused before n is looked at
    dev.sync()
    for b, was in ((X, x), (Z, np.full(n, -3.5)), (D, d)):
        got, band = b.read()
        assert band and np.array_equal(got.view(np.uint64), was.view(np.uint64))
        b.free()
    dev.free(dn)
