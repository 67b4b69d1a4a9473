"""mi355x_vec_minres_lanczos and mi355x_vec_minres_update through the C ABI on guarded views: every written vector bit for bit against
the host model (tests/minres_ref.py) and against the existing kernels run one call at a time (mi355x_vec_copy, _axpy, _scale,
_pointwise_mult); the sum of an aligned view carries the bits of mi355x_vec_dot over the op-by-op result; the host-alpha and the
device-alpha routes agree and hand alpha back; guard bands and read-only operands keep their bits; a special case keeps the operand it
skips out of every result; IEEE specials in live operands propagate as in the op-by-op run."""
import math

import numpy as np
import pytest

import minres_ref as mr
from vecspecials import bits, guarded, guards_intact, same, special_vector

pytestmark = pytest.mark.gpu

# 1023, 1024, 1025: one tile of 256 x 2 double2 (1024 doubles) and its edges; 4097: the first hand-off between workgroups of the
# reduction (16 doubles per lane: 4096 per workgroup); (1 << 21) + 1: beyond the 512-workgroup cap of the reduction's grid
SIZES = [1, 2, 3, 1023, 1024, 1025, 4097]
BIG = (1 << 21) + 1
POISON = 0x7FF8DEADBEEF0001
L_OPS = ("r", "z", "v", "u", "vold", "uold")
U_OPS = ("u", "w", "wold", "x", "r", "z", "vnew", "unew")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def vec(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


def operands(n, names):
    h = {name: vec(n, j + 1) for j, name in enumerate(names)}
    h["d"] = 1.0 / (2.0 + vec(n, 19) ** 2)
    return h


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


def lanczos_op_by_op(dev, n, alpha, beta, h):
    """the existing kernels, one call each, on plain allocations: the new r, z and mi355x_vec_dot(r, z)"""
    k = dev.k
    D = {name: dev.put(h[name]) for name in L_OPS}
    if h["d"] is not None:
        dd = dev.put(h["d"])
        dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, D["r"], dd, D["z"]))
        dev.free(dd)
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -alpha, D["v"], D["r"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -alpha, D["u"], D["z"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -beta, D["vold"], D["r"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -beta, D["uold"], D["z"]))
    dev.chk(k.mi355x_vec_dot(dev.h, n, D["r"], D["z"], dev.host_scratch()))
    dp = dev.scalar_out(1)[0]
    out = {"r": dev.get(D["r"], n), "z": dev.get(D["z"], n)}
    for q in D.values():
        dev.free(q)
    return out, dp


def check_sum(got, terms, ref, aligned):
    if aligned:
        same(got, ref, "r'z against mi355x_vec_dot over the op-by-op vectors")
        return
    if not np.all(np.isfinite(terms)):        # another walk over the same rounded terms: the margin scales with sum |terms|
        assert not np.isfinite(got), (got, "non-finite terms")
        return
    if np.max(np.abs(terms), initial=0.0) > 1e290:      # partial sums may overflow in one order and not in another: no margin to state
        return
    exact = math.fsum(terms)
    assert abs(got - exact) <= 1e-13 * math.fsum(np.abs(terms)), (got, exact)


def lanczos_case(dev, n, off, alpha=0.41, beta=0.77, with_d=True, host=None):
    """one launch per alpha route, every check; returns the new (r, z)"""
    h = dict(host or operands(n, L_OPS))
    if not with_d:
        h["d"] = None
    model = dict(zip(("r", "z"), mr.lanczos_ref(alpha, beta, h["d"], *(h[v] for v in L_OPS))))
    one, dp1 = lanczos_op_by_op(dev, n, alpha, beta, h)
    got = None
    for route in ("host", "device"):
        X = Run(dev, off, h)
        adev = dev.put(np.array([alpha])) if route == "device" else None
        host_alpha = alpha if route == "host" else 1234.5            # ignored when alpha comes from the device
        dev.chk(dev.k.mi355x_vec_minres_lanczos(dev.h, n, host_alpha, adev, beta, X.p("d"), X.p("r"), X.p("z"), X.p("v"), X.p("u"), X.p("vold"), X.p("uold"), X.out))
        dev.sync()
        now = {name: X.g[name].get() for name in ("r", "z")}
        for name, v in now.items():
            same(v, model[name], "%s against the model (%s alpha)" % (name, route))
            same(v, one[name], "%s against the kernels one by one (%s alpha)" % (name, route))
        if alpha == 0.0 and beta == 0.0:
            assert np.array_equal(bits(now["r"]), bits(h["r"])), "r touched with alpha == beta == 0"
        s = X.sums()
        with np.errstate(all="ignore"):
            check_sum(s[0], one["r"] * one["z"], dp1, off == 0)
        assert s[1] == alpha or (np.isnan(alpha) and np.isnan(s[1])), (s[1], alpha)
        if got is not None:
            assert np.array_equal(bits(got[2]), bits(s)) or np.isnan(s).any(), "the two alpha routes differ in the sums"
        X.check_readonly({"r", "z"})
        X.free()
        if adev is not None:
            dev.free(adev)
        got = (now["r"], now["z"], s)
    return got


def update_op_by_op(dev, n, first, rho2, rho3, irho1, ceta, ibeta, h):
    k = dev.k
    D = {name: dev.put(h[name]) for name in ("u", "w", "wold", "x", "r", "z")}
    out = {}
    if not first:
        wn = dev.alloc(8 * max(n, 2))
        dev.chk(k.mi355x_vec_copy(dev.h, n, D["u"], wn))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, -rho2, D["w"], wn))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, -rho3, D["wold"], wn))
        dev.chk(k.mi355x_vec_scale(dev.h, n, irho1, wn))
        dev.chk(k.mi355x_vec_axpy(dev.h, n, ceta, wn, D["x"]))
        out["wold"], out["x"] = dev.get(wn, n), dev.get(D["x"], n)
        dev.free(wn)
    for src, name in (("r", "vnew"), ("z", "unew")):
        q = dev.alloc(8 * max(n, 2))
        dev.chk(k.mi355x_vec_copy(dev.h, n, D[src], q))
        dev.chk(k.mi355x_vec_scale(dev.h, n, ibeta, q))
        out[name] = dev.get(q, n)
        dev.free(q)
    for q in D.values():
        dev.free(q)
    return out


def update_case(dev, n, off, first=False, rho2=0.83, rho3=-0.29, irho1=1.7, ceta=0.61, ibeta=2.3, host=None):
    h = dict(host or operands(n, U_OPS))
    h.pop("d", None)
    h["vnew"], h["unew"] = np.full(n, -3.0), np.full(n, -4.0)
    X = Run(dev, off, h)
    dev.chk(dev.k.mi355x_vec_minres_update(dev.h, n, 1 if first else 0, rho2, rho3, irho1, ceta, ibeta, X.p("u"), X.p("w"), X.p("wold"), X.p("x"),
                                           X.p("r"), X.p("z"), X.p("vnew"), X.p("unew")))
    dev.sync()
    wn, xn, vn, un = mr.update_ref(first, rho2, rho3, irho1, ceta, ibeta, h["u"], h["w"], h["wold"], h["x"], h["r"], h["z"])
    model = {"vnew": vn, "unew": un} if first else {"wold": wn, "x": xn, "vnew": vn, "unew": un}
    one = update_op_by_op(dev, n, first, rho2, rho3, irho1, ceta, ibeta, h)
    got = {name: X.g[name].get() for name in model}
    for name, v in got.items():
        same(v, model[name], "%s against the model" % name)
        same(v, one[name], "%s against the kernels one by one" % name)
    if first or ceta == 0.0:
        assert np.array_equal(bits(X.g["x"].get()), bits(h["x"])), "x touched"
    assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64))
    X.check_readonly(set(model))
    X.free()
    return got


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_lanczos_forms(dev, n, off):
    for with_d in (True, False):
        lanczos_case(dev, n, off, with_d=with_d)
        for alpha, beta in ((0.0, 0.77), (-0.0, 0.77), (0.41, 0.0), (0.0, 0.0), (-1.3, 1.0)):
            lanczos_case(dev, n, off, alpha=alpha, beta=beta, with_d=with_d)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_update_forms(dev, n, off):
    update_case(dev, n, off)
    update_case(dev, n, off, first=True)
    for kw in (dict(rho3=0.0), dict(rho2=0.0), dict(rho2=-0.0, rho3=-0.0), dict(ceta=0.0), dict(ceta=-0.0), dict(irho1=1.0), dict(irho1=0.0),
               dict(ibeta=1.0), dict(ibeta=0.0), dict(first=True, ibeta=1.0)):
        update_case(dev, n, off, **kw)


def test_sweeps_beyond_the_grid_cap(dev):
    lanczos_case(dev, BIG, 0)
    update_case(dev, BIG, 0)


@pytest.mark.parametrize("off", [0, 1])
def test_special_cases_keep_skipped_operands_out(dev, off):
    n = 1025
    nan = np.full(n, np.nan)
    base = operands(n, L_OPS)
    for with_d in (True, False):
        r, z, s = lanczos_case(dev, n, off, alpha=0.0, with_d=with_d, host=dict(base, v=nan, u=nan.copy()))
        assert np.all(np.isfinite(r)) and np.all(np.isfinite(z)) and np.isfinite(s[0])
        r, z, s = lanczos_case(dev, n, off, beta=0.0, with_d=with_d, host=dict(base, vold=nan, uold=nan.copy()))
        assert np.all(np.isfinite(r)) and np.all(np.isfinite(z)) and np.isfinite(s[0])
    r, z, s = lanczos_case(dev, n, off, with_d=True, host=dict(base, z=nan))          # Jacobi rides: the old z is not read
    assert np.all(np.isfinite(z)) and np.isfinite(s[0])
    r, z, s = lanczos_case(dev, n, off, with_d=False, host=dict(base, z=nan))         # z as given: the NaN must arrive
    assert np.all(np.isnan(z)) and np.isnan(s[0])
    ub = operands(n, U_OPS)
    for kw, poisoned in ((dict(rho2=0.0), ("w",)), (dict(rho3=0.0), ("wold",)), (dict(rho2=0.0, rho3=-0.0), ("w", "wold")),
                         (dict(irho1=0.0), ("u", "w", "wold")), (dict(first=True), ("u", "w", "wold", "x")), (dict(ibeta=0.0), ("r", "z"))):
        got = update_case(dev, n, off, host=dict(ub, **{name: nan.copy() for name in poisoned}), **kw)
        assert all(np.all(np.isfinite(v)) for v in got.values()), (kw, poisoned)
    got = update_case(dev, n, off, ceta=0.0, host=dict(ub, x=nan))                     # x neither read nor written: its NaN stays where it is
    assert np.all(np.isfinite(got["wold"])) and np.all(np.isnan(got["x"]))
    got = update_case(dev, n, off, irho1=1.0, host=dict(ub, u=nan))                    # irho1 == 1 skips the scale, not the operand
    assert np.all(np.isnan(got["wold"]))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [3, 1025])
def test_ieee_specials_in_live_operands(dev, n, off):
    """Inf, NaN, -0, denormals in every operand in turn: compared by position for NaNs and by bits elsewhere"""
    base = operands(n, L_OPS)
    for j, name in enumerate(L_OPS + ("d",)):
        for rot in (0, 7):
            host = dict(base, **{name: special_vector(n, 31 + j, 0.25, rot)})
            lanczos_case(dev, n, off, with_d=True, host=host)
            if name != "d":
                lanczos_case(dev, n, off, with_d=False, alpha=-0.0 if rot else 0.41, host=host)
    ub = operands(n, U_OPS)
    for j, name in enumerate(("u", "w", "wold", "x", "r", "z")):
        for rot in (0, 7):
            host = dict(ub, **{name: special_vector(n, 51 + j, 0.25, rot)})
            update_case(dev, n, off, host=host)
            update_case(dev, n, off, rho3=0.0, irho1=1.0, host=host)
    for alpha in (np.inf, np.nan):
        lanczos_case(dev, n, off, alpha=alpha)
    update_case(dev, n, off, irho1=np.inf)
    update_case(dev, n, off, ceta=np.nan)


def test_empty_vectors_and_bad_arguments(dev):
    poison = np.array([POISON, POISON], dtype=np.uint64)
    out = dev.put(poison)
    q = [dev.put(np.full(8, 5.0)) for _ in range(8)]
    k = dev.k
    dev.chk(k.mi355x_vec_minres_lanczos(dev.h, 0, 0.41, None, 0.77, None, q[0], q[1], q[2], q[3], q[4], q[5], out)); dev.sync()
    assert np.array_equal(bits(dev.get(out, 2)), bits(np.array([0.0, 0.41])))        # n == 0: { 0, alpha }
    dev.chk(k.mi355x_memcpy_h2d(dev.h, out, poison.ctypes.data, 16)); dev.sync()
    dev.chk(k.mi355x_vec_minres_update(dev.h, 0, 0, 0.8, 0.3, 1.7, 0.6, 2.3, *q)); dev.sync()
    for missing in range(6):
        a = list(q[:6]); a[missing] = None
        assert k.mi355x_vec_minres_lanczos(dev.h, 8, 0.41, None, 0.77, None, a[0], a[1], a[2], a[3], a[4], a[5], out) != 0
    assert k.mi355x_vec_minres_lanczos(dev.h, 8, 0.41, None, 0.77, None, q[0], q[1], q[2], q[3], q[4], q[5], None) != 0
    for missing in range(8):
        a = list(q); a[missing] = None
        assert k.mi355x_vec_minres_update(dev.h, 8, 0, 0.8, 0.3, 1.7, 0.6, 2.3, *a) != 0
    for missing in (4, 5, 6, 7):
        a = list(q); a[missing] = None
        assert k.mi355x_vec_minres_update(dev.h, 8, 1, 0.8, 0.3, 1.7, 0.6, 2.3, *a) != 0
    dev.chk(k.mi355x_vec_minres_update(dev.h, 8, 1, 0.0, 0.0, 0.0, 0.0, 2.0, None, None, None, None, q[4], q[5], q[6], q[7])); dev.sync()
    assert np.array_equal(dev.get(q[6], 8), np.full(8, 10.0)) and np.array_equal(dev.get(q[7], 8), np.full(8, 10.0))
    assert np.array_equal(dev.get(out, 2).view(np.uint64), poison), "a refused call touched out"
    for p in q[:6]:
        assert np.array_equal(dev.get(p, 8), np.full(8, 5.0)), "a refused call touched a vector"
    for p in q:
        dev.free(p)
    dev.free(out)
