"""mi355x_vec_bicg_dirs and mi355x_vec_bicg_update through the C ABI on guarded views: every written vector bit for bit against the
existing kernels run one call at a time (mi355x_vec_copy, _aypx, _axpy, _pointwise_mult) and against the oracle's Vec calls; the sums
carry the bits of mi355x_vec_dot and mi355x_vec_norm(type 1)'s sum over the op-by-op result; guard bands and read-only operands keep
their bits; a == 0 and b == 0 take the special cases of the separate calls; NaN / Inf propagate as in the op-by-op run; bad arguments
return an error and write nothing."""
import numpy as np
import pytest

import orc
from vecspecials import bits, guarded, guards_intact, same

pytestmark = pytest.mark.gpu
SIZES = [1, 63, 64, 65, 1023, 4097]
POISON = 0x7FF8DEADBEEF0001
INVALID = 1
D_OPS = ("zr", "zl", "pr", "pl")
U_OPS = ("pr", "d", "x", "rr", "rl", "zr", "zl")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def operands(n, names, seed=0):
    return {name: np.random.default_rng([n, seed, j]).standard_normal(n) for j, name in enumerate(names)}


class Run:
    def __init__(self, dev, off, host):
        self.dev, self.host = dev, host
        self.g = {name: guarded(dev, a, off, tag=j + 1) for j, (name, a) in enumerate(host.items())}
        self.out = dev.put(np.array([POISON, POISON], dtype=np.uint64))

    def p(self, name):
        return self.g[name].ptr

    def check(self, want, what, nan_is_nan=False):
        """nan_is_nan: any NaN equals any NaN (vecspecials.same: the payload and sign of a NaN are not part of the contract)"""
        for name, g in self.g.items():
            ref = want.get(name, self.host[name])
            got = g.get()
            if nan_is_nan:
                same(got, ref, "%r %s" % (what, name))
            else:
                assert np.array_equal(bits(got), bits(ref)), (what, name, "written" if name in want else "read-only operand changed")
        guards_intact(*self.g.values(), names=list(self.g))

    def free(self):
        for g in self.g.values():
            g.free()
        self.dev.free(self.out)


def dirs_model(h, first, b):
    pr, pl = h["pr"].copy(), h["pl"].copy()
    if first:
        orc.vec_copy(h["zr"], pr); orc.vec_copy(h["zl"], pl)
    else:
        orc.vec_aypx(pr, b, h["zr"]); orc.vec_aypx(pl, b, h["zl"])
    return {"pr": pr, "pl": pl}


def dirs_kernels(dev, h, first, b):
    k, n = dev.k, h["pr"].size
    p = {name: dev.put(a) for name, a in h.items()}
    if first:
        dev.chk(k.mi355x_vec_copy(dev.h, n, p["zr"], p["pr"])); dev.chk(k.mi355x_vec_copy(dev.h, n, p["zl"], p["pl"]))
    else:
        dev.chk(k.mi355x_vec_aypx(dev.h, n, b, p["zr"], p["pr"])); dev.chk(k.mi355x_vec_aypx(dev.h, n, b, p["zl"], p["pl"]))
    out = {"pr": dev.get(p["pr"], n), "pl": dev.get(p["pl"], n)}
    for q in p.values():
        dev.free(q)
    return out


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_dirs_carries_the_bits_of_the_separate_calls(dev, n, off):
    for first, b in ((1, 0.7), (0, 0.7), (0, 0.0), (0, 1.0), (0, -1.0)):
        h = operands(n, D_OPS, 1)
        X = Run(dev, off, h)
        dev.chk(dev.k.mi355x_vec_bicg_dirs(dev.h, n, first, b, X.p("zr"), X.p("zl"), X.p("pr"), X.p("pl")))
        dev.sync()
        model, kern = dirs_model(h, first, b), dirs_kernels(dev, h, first, b)
        for name in model:
            assert np.array_equal(bits(model[name]), bits(kern[name])), (n, first, b, name)
        X.check(model, (n, off, first, b))
        X.free()


def update_model(h, a, pcmode):
    x, rr, rl, zr, zl = (h[k].copy() for k in ("x", "rr", "rl", "zr", "zl"))
    orc.vec_axpy(x, a, h["pr"]); orc.vec_axpy(rr, -a, h["zr"]); orc.vec_axpy(rl, -a, h["zl"])
    if pcmode == 1:
        orc.vec_pointwise_mult(zr, rr, h["d"]); orc.vec_pointwise_mult(zl, rl, h["d"])
    elif pcmode == 2:
        orc.vec_copy(rr, zr); orc.vec_copy(rl, zl)
    out = {"x": x, "rr": rr, "rl": rl}
    if pcmode:
        out.update(zr=zr, zl=zl)
    return out


def update_kernels(dev, h, a, pcmode, which):
    """the separate launches; returns (vectors, [dot, norm sum])"""
    k, n = dev.k, h["x"].size
    p = {name: dev.put(v) for name, v in h.items()}
    dev.chk(k.mi355x_vec_axpy(dev.h, n, a, p["pr"], p["x"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -a, p["zr"], p["rr"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -a, p["zl"], p["rl"]))
    if pcmode == 1:
        dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, p["rr"], p["d"], p["zr"])); dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, p["rl"], p["d"], p["zl"]))
    elif pcmode == 2:
        dev.chk(k.mi355x_vec_copy(dev.h, n, p["rr"], p["zr"])); dev.chk(k.mi355x_vec_copy(dev.h, n, p["rl"], p["zl"]))
    o = dev.put(np.zeros(2))
    o1 = type(o)(o.value + 8)
    sums = [0.0, 0.0]
    if pcmode:
        dev.chk(k.mi355x_vec_dot(dev.h, n, p["zr"], p["rl"], o))
    t = p["zr"] if (pcmode and which == 0) else p["rr"]
    dev.chk(k.mi355x_vec_dot(dev.h, n, t, t, o1))                # x'x under mi355x_vec_dot: the sum mi355x_vec_norm(type 1) roots
    got = dev.get(o, 2)
    sums = [got[0] if pcmode else 0.0, got[1]]
    nrm = dev.put(np.zeros(1))
    dev.chk(k.mi355x_vec_norm(dev.h, n, 1, t, nrm))
    root = dev.get(nrm, 1)[0]                                    # (type 1 leaves the SUM; the caller takes the root)
    out = {name: dev.get(p[name], n) for name in ("x", "rr", "rl", "zr", "zl")}
    for q in list(p.values()) + [o, nrm]:
        dev.free(q)
    return out, sums, root


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_update_carries_the_bits_of_the_separate_calls(dev, n, off):
    for pcmode in (0, 1, 2):
        for which in (0, 1):
            for a in (0.37, 0.0):
                h = operands(n, U_OPS, 2)
                if pcmode != 1:
                    del h["d"]
                X = Run(dev, off, h)
                dev.chk(dev.k.mi355x_vec_bicg_update(dev.h, n, a, pcmode, which, X.p("pr"), X.p("d") if pcmode == 1 else None, X.p("x"),
                                                     X.p("rr"), X.p("rl"), X.p("zr"), X.p("zl"), X.out))
                dev.sync()
                model = update_model(h, a, pcmode)
                kern, sums, root = update_kernels(dev, h, a, pcmode, which)
                what = (n, off, pcmode, which, a)
                for name in model:
                    assert np.array_equal(bits(model[name]), bits(kern[name])), (what, name)
                X.check(model, what)
                got = dev.get(X.out, 2)
                if off == 0:                                      # the aligned view meets its elements as the separate reductions do
                    assert np.array_equal(bits(got), bits(np.array(sums))), (what, got, sums)
                    assert np.array_equal(bits(np.array([got[1]])), bits(np.array([root])))
                else:
                    assert np.allclose(got, sums, rtol=1e-13, atol=1e-13 * n)
                X.free()


@pytest.mark.parametrize("special", [np.nan, np.inf])
def test_specials_propagate_as_in_the_separate_calls(dev, special):
    n = 1023
    for where in ("zr", "rl", "pr", "d"):
        h = operands(n, U_OPS, 3)
        h[where][517] = special
        X = Run(dev, 0, h)
        dev.chk(dev.k.mi355x_vec_bicg_update(dev.h, n, 0.5, 1, 0, X.p("pr"), X.p("d"), X.p("x"), X.p("rr"), X.p("rl"), X.p("zr"), X.p("zl"), X.out))
        dev.sync()
        kern, sums, _ = update_kernels(dev, h, 0.5, 1, 0)
        X.check(kern, (special, where), nan_is_nan=True)
        assert any(not np.isfinite(kern[name]).all() for name in kern)
        same(dev.get(X.out, 2), np.array(sums), "sums %r %s" % (special, where))
        X.free()
    h = operands(n, D_OPS, 4)
    h["pl"][3] = special
    X = Run(dev, 0, h)
    dev.chk(dev.k.mi355x_vec_bicg_dirs(dev.h, n, 0, 0.0, X.p("zr"), X.p("zl"), X.p("pr"), X.p("pl")))    # b == 0: a copy, the special is gone
    dev.sync()
    X.check({"pr": h["zr"], "pl": h["zl"]}, "b == 0 skips pl", nan_is_nan=True)
    assert np.isfinite(X.g["pl"].get()).all()
    X.free()


def test_bad_arguments_write_nothing(dev):
    n = 65
    h = operands(n, U_OPS, 5)
    X = Run(dev, 0, h)
    k = dev.k
    a = dict(pr=X.p("pr"), d=X.p("d"), x=X.p("x"), rr=X.p("rr"), rl=X.p("rl"), zr=X.p("zr"), zl=X.p("zl"))

    def upd(pcmode=1, which=0, **kw):
        v = dict(a, **kw)
        return k.mi355x_vec_bicg_update(dev.h, n, 0.5, pcmode, which, v["pr"], v["d"], v["x"], v["rr"], v["rl"], v["zr"], v["zl"], X.out)
    assert upd(pcmode=3) == INVALID and upd(which=2) == INVALID and upd(pcmode=0) == INVALID and upd(pcmode=1, d=None) == INVALID
    assert upd(x=None) == INVALID and upd(zr=a["rr"]) == INVALID and upd(pr=a["x"]) == INVALID and upd(d=a["zl"]) == INVALID
    assert k.mi355x_vec_bicg_dirs(dev.h, n, 0, 0.5, a["zr"], a["zl"], a["pr"], a["pr"]) == INVALID
    assert k.mi355x_vec_bicg_dirs(dev.h, n, 0, 0.5, a["zr"], a["zl"], a["zr"], a["x"]) == INVALID
    assert k.mi355x_vec_bicg_dirs(dev.h, n, 0, 0.5, None, a["zl"], a["pr"], a["x"]) == INVALID
    dev.sync()
    X.check({}, "refused calls")
    assert dev.get(X.out, 2, dtype=np.uint64).tolist() == [POISON, POISON]
    assert k.mi355x_vec_bicg_dirs(dev.h, 0, 0, 0.5, a["zr"], a["zl"], a["pr"], a["x"]) == 0                 # n == 0: nothing
    dev.sync()
    X.check({}, "n == 0")
    X.free()
