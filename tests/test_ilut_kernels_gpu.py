"""The transposed triangular solves on the device through the C ABI: mi355x_ilut_first_level / _second_level over the output of
mi355x_ilut_build_host against the reference's scatter loop (bicg_ref.ilu_solve_transpose) bit for bit, and the value gather the
plug-in refills the transposed factor with (mi355x_pack through a permutation).  x, b and every value array live between guard bands
of a marker; every comparison of a solution is on bit patterns.  The model is checked on its own, without a GPU, by test_bicg_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import bicg_ref as br
from ilufactor import MARK, bits
from test_bicg_cpu import build_host, factor, rhs
from test_ilu_factor_specials_gpu import Guarded
from test_kernels_gpu import dev  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
_extra = {}


def named(name):
    if name in ("ilu0_1025", "ilu1_1025"):
        if name not in _extra:
            csr = br.convdiff(41, 25)
            _extra[name] = br.iluk_factor(*csr, 1) if name == "ilu1_1025" else br.orc.ilu0_factor(*csr)
        return _extra[name]
    return factor(name)


class Transposed:
    """a transposed factor on the device: the two patterns, ta / sa / dinv each between guard bands, the rows of every level"""

    def __init__(self, dev, f):
        self.dev, self.f = dev, f
        rc, T = build_host(dev.k, f)
        assert rc == 0
        self.T, self.n = T, f[0].size - 1
        ba = f[3]
        self.vals = {}
        for key, v in (("ta", ba[T["tperm"]]), ("sa", ba[T["sperm"]]), ("dinv", ba[f[2][:self.n]])):
            g = Guarded(dev, v.size)
            if v.size:
                g.put(v)
            self.vals[key] = g
        self.d = {key: dev.put(T[key]) for key in ("ti", "tj", "si", "sj")}
        self.rows1 = [np.flatnonzero(T["lev1"] == l).astype(np.int32) for l in range(T["nlev1"])]
        self.rows2 = [np.flatnonzero(T["lev2"] == l).astype(np.int32) for l in range(T["nlev2"])]
        self.d1, self.d2 = [dev.put(r) for r in self.rows1], [dev.put(r) for r in self.rows2]

    def solve(self, b, alias=False, what=""):
        dev, k = self.dev, self.dev.k
        gx = Guarded(dev, self.n)
        gb = gx if alias else Guarded(dev, self.n)
        gb.put(b)
        for r, d in zip(self.rows1, self.d1):
            dev.chk(k.mi355x_ilut_first_level(dev.h, r.size, d, self.d["ti"], self.d["tj"], self.vals["ta"].ptr, self.vals["dinv"].ptr, gb.ptr, gx.ptr))
        for r, d in zip(self.rows2, self.d2):
            dev.chk(k.mi355x_ilut_second_level(dev.h, r.size, d, self.d["si"], self.d["sj"], self.vals["sa"].ptr, gx.ptr))
        dev.sync()
        x = gx.get(what + " x")
        if not alias:
            assert np.array_equal(bits(gb.get(what + " b")), bits(b)), "b was written"
            gb.free()
        for key, g in self.vals.items():
            g.get(what + " " + key)
        gx.free()
        return x


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("name", ["ilu0", "ilu1", "ilu0_1025", "ilu1_1025", "chain70", "diag300", "upper40", "n1"])
def test_level_kernels_carry_the_scatter_loops_bits(dev, name, alias):
    f = named(name)
    T = Transposed(dev, f)
    for k in range(2):
        b = rhs(T.n, 10 + k)
        x = T.solve(b, alias=alias, what=name)
        assert np.array_equal(bits(x), bits(br.ilu_solve_transpose(f, b))), (name, alias, k)
    dev.free_all()


def test_no_rows_launch_nothing(dev):
    T = Transposed(dev, factor("chain70"))
    gx = Guarded(dev, 70)
    dev.chk(dev.k.mi355x_ilut_first_level(dev.h, 0, T.d1[0], T.d["ti"], T.d["tj"], T.vals["ta"].ptr, T.vals["dinv"].ptr, gx.ptr, gx.ptr))
    dev.chk(dev.k.mi355x_ilut_second_level(dev.h, 0, T.d2[0], T.d["si"], T.d["sj"], T.vals["sa"].ptr, gx.ptr))
    dev.sync()
    assert (bits(gx.get("no rows")) == bits(np.array([MARK]))[0]).all()
    dev.free_all()


def test_a_nan_reaches_its_dependents_only(dev):
    f = factor("ilu0")
    T = Transposed(dev, f)
    for c in (0, 517, T.n - 1):
        b = rhs(T.n, 20)
        b[c] = np.nan
        x = T.solve(b, what="nan at %d" % c)
        assert np.array_equal(np.isnan(x), br.dependents(f, c)), c
        ok = ~np.isnan(x)
        assert np.array_equal(bits(x[ok]), bits(br.ilu_solve_transpose(f, b)[ok]))
    dev.free_all()


def test_specials_carry_the_models_bits(dev):
    """Inf and -0.0 among the factor's values and in b: the bits of the scatter loop, NaNs where it has them"""
    bi, bj, bd, ba = factor("ilu0")
    ba = ba.copy()
    n = bi.size - 1
    ba[bd[40] - 1] = np.inf                                         # a strict-upper entry of row 40
    ba[bi[200]] = -0.0                                              # an L entry of row 200
    ba[bd[300]] = -0.0                                              # an inverted diagonal
    f = (bi, bj, bd, ba)
    T = Transposed(dev, f)
    b = rhs(n, 21)
    b[700] = -0.0
    b[701] = np.inf
    x, want = T.solve(b, what="specials"), br.ilu_solve_transpose(f, b)
    assert np.array_equal(np.isnan(x), np.isnan(want)) and not np.isnan(want).all()
    ok = ~np.isnan(want)
    assert np.array_equal(bits(x[ok]), bits(want[ok]))
    dev.free_all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_value_gather_through_a_permutation(dev, n):
    """dst[k] = src[perm[k]]: how a factorisation on an unchanged pattern refills ta / sa / dinv from the factor's device values"""
    rng = np.random.default_rng(900 + n)
    src = rng.standard_normal(max(2 * n, 1))
    perm = rng.permutation(src.size)[:n].astype(np.int32)
    gs, gd = Guarded(dev, src.size), Guarded(dev, max(n, 1))
    gs.put(src)
    dperm = dev.put(perm)
    dev.chk(dev.k.mi355x_pack(dev.h, n, dperm, gs.ptr, gd.ptr))
    dev.sync()
    out = gd.get("gather dst")
    assert np.array_equal(bits(out[:n]), bits(src[perm]))
    assert (bits(out[n:]) == bits(np.array([MARK]))[0]).all()
    assert np.array_equal(bits(gs.get("gather src")), bits(src))
    dev.free_all()
