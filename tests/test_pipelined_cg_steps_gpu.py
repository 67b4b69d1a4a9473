"""mi355x_vec_pipecg_step through the C ABI on guarded views: every written vector bit for bit against the host model
(tests/pipecg_ref.py) and against the existing kernels run one call at a time (mi355x_vec_copy / _aypx x4, mi355x_vec_axpy x4,
mi355x_vec_pointwise_mult / _copy); the sums of an aligned view carry the bits of mi355x_vec_dot / mi355x_vec_norm(type 1) over the
op-by-op results; guard bands and read-only operands keep their bits; a special case keeps the operand it skips out of every result."""
import math

import numpy as np
import pytest

import pipecg_ref as pr
from vecspecials import bits, guarded, guards_intact, same

pytestmark = pytest.mark.gpu

# 1023, 1024, 1025: one tile of 256 x 2 double2 (1024 doubles) and its edges; 4097: the first hand-off between workgroups of the
# reduction (16 doubles per lane: 4096 per workgroup); (1 << 21) + 1: beyond the 512-workgroup cap of the reduction's grid
SIZES = [1, 2, 3, 1023, 1024, 1025, 4097]
BIG = (1 << 21) + 1
POISON = 0x7FF8DEADBEEF0001
RECS = ("zrec", "qrec", "p", "s")
ITER = ("x", "u", "w", "r")


@pytest.fixture(scope="module")
def dev(built):
    from gpu import Dev
    d = Dev()
    yield d
    d.free_all()


def vec(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


def operands(n):
    h = {name: vec(n, j + 1) for j, name in enumerate(("nv", "mv") + RECS + ITER)}
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


def op_by_op(dev, n, first, ratio, step, h, with_m, rides):
    """the existing kernels, one call each, on plain allocations: the nine results and the two sums"""
    k = dev.k
    D = {name: dev.put(h[name]) for name in ("nv", "mv") + RECS + ITER}
    uo, wo = dev.put(h["u"]), dev.put(h["w"])                      # p and s take the OLD u and w
    for rec, src in (("zrec", D["nv"]), ("qrec", D["mv"]), ("p", uo), ("s", wo)):
        if first:
            dev.chk(k.mi355x_vec_copy(dev.h, n, src, D[rec]))
        else:
            dev.chk(k.mi355x_vec_aypx(dev.h, n, ratio, src, D[rec]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, step, D["p"], D["x"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -step, D["qrec"], D["u"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -step, D["zrec"], D["w"]))
    dev.chk(k.mi355x_vec_axpy(dev.h, n, -step, D["s"], D["r"]))
    out = {name: dev.get(D[name], n) for name in RECS + ITER}
    if with_m:
        dm = dev.alloc(8 * max(n, 2))
        if h["d"] is None:
            dev.chk(k.mi355x_vec_copy(dev.h, n, D["w"], dm))
        else:
            dd = dev.put(h["d"])
            dev.chk(k.mi355x_vec_pointwise_mult(dev.h, n, D["w"], dd, dm))
            dev.free(dd)
        out["m_next"] = dev.get(dm, n)
        dev.free(dm)
    sums = None
    if rides:
        hs = dev.host_scratch()
        dev.chk(k.mi355x_vec_dot(dev.h, n, D["w"], D["u"], hs)); wu = dev.scalar_out(1)[0]
        if rides == 1:
            dev.chk(k.mi355x_vec_norm(dev.h, n, 1, D["r"], hs))
        elif rides == 2:
            dev.chk(k.mi355x_vec_norm(dev.h, n, 1, D["u"], hs))
        else:
            dev.chk(k.mi355x_vec_dot(dev.h, n, D["r"], D["u"], hs))
        sums = [wu, dev.scalar_out(1)[0]]
    for q in list(D.values()) + [uo, wo]:
        dev.free(q)
    return out, sums


def check_sums(got, terms, ref, aligned):
    if aligned:
        same(got, ref, "sums against mi355x_vec_dot / mi355x_vec_norm over the op-by-op vectors")
        return
    for g, t in zip(got, terms):                # another walk over the same rounded terms; a dot's terms cancel: the margin scales with sum |terms|
        if not np.all(np.isfinite(t)):
            assert not np.isfinite(g), (g, "non-finite terms")
            continue
        exact = math.fsum(t)
        assert abs(g - exact) <= 1e-13 * math.fsum(np.abs(t)), (g, exact)


def step_case(dev, n, off, first=False, ratio=0.37, step=0.8, with_d=True, mmode="own", rides=1, host=None):
    """one launch, every check; mmode: "own" (m_next its own vector), "alias" (m_next is mv), "null"; rides 0: out == NULL"""
    h = dict(host or operands(n))
    if not with_d:
        h["d"] = None
    if mmode == "own":
        h["m_next"] = np.full(n, -3.0)
    X = Run(dev, off, h)
    mp = {"own": X.p("m_next"), "alias": X.p("mv"), "null": None}[mmode]
    dev.chk(dev.k.mi355x_vec_pipecg_step(dev.h, n, 1 if first else 0, ratio, step, X.p("nv"), X.p("mv"), X.p("d"), X.p("zrec"), X.p("qrec"), X.p("p"),
                                         X.p("s"), X.p("x"), X.p("u"), X.p("w"), X.p("r"), mp, rides, X.out if rides else None))
    dev.sync()
    model = dict(zip(RECS + ITER + ("m_next",), pr.step_ref(first, ratio, step, h["nv"], h["mv"], h["d"], *(h[v] for v in RECS + ITER), with_m=mmode != "null")))
    one, sums1 = op_by_op(dev, n, first, ratio, step, h, mmode != "null", rides)
    got = {name: X.g[name].get() for name in RECS + ITER}
    if mmode != "null":
        got["m_next"] = X.g["m_next" if mmode == "own" else "mv"].get()
    for name, v in got.items():
        same(v, model[name], "%s against the model" % name)
        same(v, one[name], "%s against the kernels one by one" % name)
    if step == 0.0:
        for name in ITER:
            assert np.array_equal(bits(got[name]), bits(h[name])), "step 0 touched %s" % name
    if rides:
        check_sums(X.sums(), pr.sum_terms(rides, one["u"], one["w"], one["r"]), sums1, off == 0)
    else:
        assert np.array_equal(X.sums().view(np.uint64), np.array([POISON, POISON], dtype=np.uint64)), "out touched without sums"
    X.check_readonly(set(RECS + ITER) | {"m_next"} | ({"mv"} if mmode == "alias" else set()))
    X.free()
    return got


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_pipecg_step_forms(dev, n, off):
    step_case(dev, n, off, first=True, rides=3)                                     # iteration 0's sweep
    for ratio in (0.0, -0.0, 1.0, -1.0, 0.37):
        step_case(dev, n, off, ratio=ratio, rides=1)
    for step in (0.0, -0.0, 0.8):
        step_case(dev, n, off, step=step, rides=2)
    step_case(dev, n, off, with_d=False, mmode="alias", rides=3)                    # PCNONE, the form the solver runs
    step_case(dev, n, off, mmode="alias", rides=1)                                  # PCJACOBI, the form the solver runs
    step_case(dev, n, off, mmode="null", rides=2)                                   # a general preconditioner
    step_case(dev, n, off, mmode="alias", rides=0)                                  # the last permitted iteration: nothing reduced
    step_case(dev, n, off, first=True, with_d=False, mmode="null", rides=0, step=0.0)


def test_pipecg_step_sums_beyond_the_grid_cap(dev):
    step_case(dev, BIG, 0, mmode="alias", rides=1)


@pytest.mark.parametrize("off", [0, 1])
def test_pipecg_step_special_cases_keep_skipped_operands_out(dev, off):
    n = 1025
    bad = vec(n, 5)
    bad[[0, 1, 511, 512, 1023, 1024]] = [np.inf, np.nan, -np.inf, np.nan, np.inf, np.nan]
    base = operands(n)
    old_bad = dict(base, zrec=bad, qrec=bad.copy(), p=bad.copy(), s=bad.copy())
    for rides in (1, 0):
        # first, ratio 0: the old recurrence vectors (Inf / NaN) are not read -- 0 * Inf would be NaN
        for kw in (dict(first=True), dict(ratio=0.0), dict(ratio=-0.0)):
            got = step_case(dev, n, off, rides=rides, host=old_bad, **kw)
            assert all(np.all(np.isfinite(v)) for v in got.values())
        # step 0: whatever the recurrences hold, x, u, w, r keep their bits and the sums stay finite
        got = step_case(dev, n, off, step=0.0, rides=rides, host=dict(base, nv=bad, mv=bad.copy()))
        assert not np.all(np.isfinite(got["zrec"])) and all(np.all(np.isfinite(got[v])) for v in ITER + ("m_next",))
        got = step_case(dev, n, off, step=-0.0, rides=rides, host=old_bad)
        assert all(np.all(np.isfinite(got[v])) for v in ITER)
        # elsewhere Inf / NaN propagate as in the op-by-op run
        got = step_case(dev, n, off, rides=rides, host=dict(base, nv=bad))
        assert np.isnan(got["w"][1]) and np.isinf(got["w"][0])
        step_case(dev, n, off, rides=rides, host=old_bad)
        step_case(dev, n, off, ratio=1.0, rides=3 if rides else 0, host=dict(base, u=bad))


def test_pipecg_step_on_empty_vectors_and_bad_arguments(dev):
    poison = np.array([POISON, POISON], dtype=np.uint64)
    out = dev.put(poison)
    q = [dev.put(np.full(8, 5.0)) for _ in range(12)]
    k = dev.k

    def call(n, rides, o, ptrs=None):
        a = list(ptrs or q)
        return k.mi355x_vec_pipecg_step(dev.h, n, 0, 0.37, 0.8, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], rides, o)

    dev.chk(call(0, 1, out)); dev.sync()
    assert np.array_equal(bits(dev.get(out, 2)), bits(np.zeros(2)))               # with sums: zeros
    dev.chk(k.mi355x_memcpy_h2d(dev.h, out, poison.ctypes.data, 16)); dev.sync()
    dev.chk(call(0, 0, None)); dev.sync()                                         # without: nothing touched
    for rides in (0, 4, -1):                                                      # rides outside 1..3 with out
        assert call(8, rides, out) != 0
    for missing in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10):                               # a required vector missing (d and m_next may be NULL)
        a = list(q); a[missing] = None
        assert call(8, 1, out, a) != 0
    dev.sync()
    assert np.array_equal(dev.get(out, 2).view(np.uint64), poison), "a refused call touched out"
    for p in q:
        assert np.array_equal(dev.get(p, 8), np.full(8, 5.0)), "a refused call touched a vector"
        dev.free(p)
    dev.free(out)
