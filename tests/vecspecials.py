"""Host-side machinery of the Vec IEEE-special / guard-band tests (test_vec_specials_gpu.py), checked on its own by
test_vec_specials_cpu.py; pure numpy + the oracle, nothing here touches the GPU until a Dev is handed in.

What is here: the comparator `same` (any NaN equals any NaN, everything else bit for bit), vectors of normal data with IEEE
specials sprinkled in and forced into the structural positions of the kernels (first element, odd tail, last tile), device
allocations with NaN guard bands on both sides of a view that starts 0 or 8 bytes off a 16-byte boundary, and CASES: one
entry per Vec entry point of csrc/vec_kernels.hip with its operands, its scalar tuples, the call, the reference and -- for a
tuple that selects a special branch of the reference -- the WRONG form a kernel without that branch would compute."""
import ctypes as C

import numpy as np

import orc

NAN, INF = np.nan, np.inf
MIN_SUB = 5e-324
MID_SUB = 2.0 ** -1050
DBL_MIN = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308
# the overwrite values; 1e-160: its square is subnormal
KINDS = np.array([NAN, INF, -INF, 0.0, -0.0, MIN_SUB, -MIN_SUB, MID_SUB, -MID_SUB, DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX, 1e-160, -1e-160])
FINITE_KINDS = np.array([0.0, -0.0, MIN_SUB, -MIN_SUB, MID_SUB, -MID_SUB, DBL_MIN, -DBL_MIN, 1e-160, -1e-160])   # no overflow either
K = KINDS.size
# The one NaN bit pattern of every guard double of an allocation.  A signalling NaN, the low byte the operand's number in its case:
# arithmetic on a guard quiets it and a copy from another operand's guard carries that operand's number, so a kernel that
# stores guard-derived values past its view changes the bits (with one quiet pattern everywhere, NaN + a * NaN would store back
# the very bits it read).
GUARD = np.uint64(0x7FF4A5A55A5AA500)
SHARE = 0.25                                   # share of overwritten entries in the special vectors of the tests


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differing(a, b):
    """mask of the entries `same` rejects"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return ~((np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b)))


def same(a, b, what=""):
    """any NaN equals any NaN (payload and sign of a NaN may differ between x86 and the device); every other value bit for
    bit: -0.0 != +0.0, subnormals exact"""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64)).ravel(); b = np.atleast_1d(np.asarray(b, dtype=np.float64)).ravel()
    d = differing(a, b)
    if d.any():
        i = int(np.flatnonzero(d)[0])
        raise AssertionError("%s: %d of %d entries differ, first at %d: %#018x (%r) != %#018x (%r)"
                             % (what, int(d.sum()), d.size, i, int(bits(a)[i]), float(a[i]), int(bits(b)[i]), float(b[i])))


def is_same(a, b):
    return not differing(np.atleast_1d(a).ravel(), np.atleast_1d(b).ravel()).any()


def structural_positions(n):
    """element 0, element n - 1 (the odd tail) and one element of the last, partially filled tile: the second half of the last
    16-byte pair (for an even n the first half, n - 1 being taken)"""
    pos = [0, n - 1, 2 * (n >> 1) - 1 if (n & 1) else n - 2]
    return [p for p in dict.fromkeys(pos) if 0 <= p < n]


def special_vector(n, seed, share, rot=0, kinds=KINDS):
    """standard normal data with round(share * n) entries overwritten by `kinds`: a third of them signed zeros (the values
    whose branch matters most: y + 0 * x == y unless y is -0.0), the rest uniform over all kinds.  The structural positions get
    kind rot + seed, + 5, + 10 (mod the number of kinds): over rot = 0 .. len(kinds) - 1 every kind meets every position."""
    rng = np.random.default_rng([seed, rot])
    x = rng.standard_normal(n)
    m = int(round(share * n))
    if m:
        idx = rng.choice(n, size=m, replace=False)
        kind = rng.integers(0, kinds.size, size=m)
        zero = rng.random(m) < 1.0 / 3.0
        z0 = int(np.flatnonzero(kinds == 0.0)[0])                  # +0.0 and -0.0 are neighbours in both tables
        kind[zero] = z0 + rng.integers(0, 2, size=int(zero.sum()))
        x[idx] = kinds[kind]
    for j, p in enumerate(structural_positions(n)):
        x[p] = kinds[(rot + seed + 5 * j) % kinds.size]
    return x


# ---------------------------------------------------------------------------------------------------------- guard bands
class Guarded:
    """front + n + back doubles of device memory, guards of GUARD on both sides (>= 2 doubles each); the view of n doubles
    starts `offset` doubles off a 16-byte boundary"""

    def __init__(self, dev, n, offset, tag=0):
        assert offset in (0, 1) and 0 <= tag < 256
        self.guard = GUARD | np.uint64(tag)
        self.dev, self.n, self.front, self.back = dev, n, 2 + offset, 3 - offset
        self.total = self.front + n + self.back
        self.base = dev.alloc(8 * self.total)
        assert self.base.value % 16 == 0
        self.ptr = C.c_void_p(self.base.value + 8 * self.front)
        self.host = None

    def load(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        assert host.size == self.n
        buf = np.empty(self.total)
        bits(buf)[:] = self.guard
        buf[self.front:self.front + self.n] = host
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, self.base, buf.ctypes.data, buf.nbytes))
        self.dev.sync()
        self.host = host.copy()
        return self

    def poke(self, i, value):
        """overwrite element i of the view"""
        assert 0 <= i < self.n
        v = np.array([value], dtype=np.float64)
        self.dev.chk(self.dev.k.mi355x_memcpy_h2d(self.dev.h, C.c_void_p(self.ptr.value + 8 * i), v.ctypes.data, 8))
        self.dev.sync()
        self.host[i] = value

    def whole(self):
        return self.dev.get(self.base, self.total)

    def get(self):
        return self.whole()[self.front:self.front + self.n].copy()

    def free(self):
        self.dev.free(self.base)


def guarded(dev, host_array, offset, tag=0):
    return Guarded(dev, np.asarray(host_array).size, offset, tag).load(host_array)


def guard_damage(whole, front, n, guard=GUARD):
    """indices (relative to the view) of guard doubles that no longer hold their pattern"""
    b = bits(whole)
    idx = np.concatenate([np.arange(-front, 0), np.arange(n, whole.size - front)])
    return [int(i) for i in idx if b[front + i] != guard]


def guards_intact(*gs, names=None):
    """reads every allocation back whole: the guard bits are unchanged"""
    for j, g in enumerate(gs):
        bad = guard_damage(g.whole(), g.front, g.n, g.guard)
        assert not bad, "operand %s (n = %d, view %d doubles off): guard overwritten at view index %s" % (
            names[j] if names else j, g.n, g.front - 2, bad)


# ------------------------------------------------------------------------------------------------------------ the cases
def dsum(a, b):
    """sum a_i b_i in the oracle's current order (sequential, or the device tree under orc.device_reduction_order())"""
    return orc.vec_dot(np.ascontiguousarray(a), np.ascontiguousarray(b))


def asum(a):
    return orc.vec_norm(np.ascontiguousarray(a), 0)


def _o(fn, out, *args):
    out = out.copy()
    fn(out, *args)
    return out


class Case:
    """ops: operand names in the order the alignment patterns walk them; outs: those the kernel writes.  call(X, t) launches
    (X.k, X.h, X.n, X.p[name] device pointers, X.res result pointer, X.scal(values) device scalars, X.table(names) pointer
    table); ref(t, v) -> (dict of output vectors, list of sums), a sum being ("dot", a, b), ("abs", a), ("max", a) or
    ("val", value); wrong(t, v) -> the outputs of the general form for a tuple that selects a special branch, else None."""

    def __init__(self, name, ops, outs, tuples, call, ref, wrong=None, fin=None):
        self.name, self.ops, self.outs, self.tuples, self.call, self.ref = name, ops, outs, tuples, call, ref
        self.wrong = wrong or (lambda t, v: None)
        self.fin = fin            # operands that must stay finite, non-zero normal data (a Jacobi diagonal)


ALPHAS = [(0.0,), (-0.0,), (1.0,), (-1.0,), (0.37,), (INF,), (NAN,)]
AB = [(a, b) for a in (0.0, 1.0, 0.37, -2.5) for b in (0.0, 1.0, 0.37, -2.5)]
ABC = [(1.0, 0.5, 2.0), (0.37, -2.5, 1.0), (0.37, -2.5, 0.0), (0.37, -2.5, 0.61), (1.0, 0.5, 0.0), (-1.2, 0.0, -0.0)]
BCGS = [(0.37, -1.21), (1.0, 0.5), (0.2, 1.0), (0.2, -1.0), (0.3, 0.0), (0.3, -0.0)]


def _axpby_wrong(t, v):
    return {"y": t[0] * v["x"] + t[1] * v["y"]} if (t[0] == 0.0 or t[1] == 0.0) else None


def _axpbypcz_wrong(t, v):
    a, b, g = t
    if a == 1.0 and g == 0.0:         # the reference tests alpha == 1 first: z still counts; a kernel that tested gamma first would drop it
        return {"z": a * v["x"] + b * v["y"]}
    if a != 1.0 and g == 0.0:
        return {"z": a * v["x"] + b * v["y"] + g * v["z"]}
    return None


def _maxpy_case(nv, coefs=None):
    ys = ["y%d" % j for j in range(nv)]
    tuples = coefs if coefs is not None else [tuple(np.random.default_rng(900 + nv).standard_normal(nv))]

    def call(X, t):
        al = np.array(t, dtype=np.float64)
        return X.k.mi355x_vec_maxpy(X.h, X.n, nv, al.ctypes.data_as(C.POINTER(C.c_double)), X.table(ys), X.p["x"])

    def ref(t, v):
        x = v["x"].copy(); orc.vec_maxpy(x, np.array(t), [v[y] for y in ys])
        return {"x": x}, []

    def wrong(t, v):                  # a kernel that skipped zero coefficients (the reference does not: dvec2.c:853-900)
        if not any(c == 0.0 for c in t):
            return None
        keep = [j for j in range(nv) if t[j] != 0.0]
        x = v["x"].copy()
        if keep:
            orc.vec_maxpy(x, np.array([t[j] for j in keep]), [v[ys[j]] for j in keep])
        return {"x": x}
    return Case("maxpy%d" % nv, ["x"] + ys, ["x"], tuples, call, ref, wrong)


def _maxpy_norm_case(nv, coefs=None):
    ys = ["y%d" % j for j in range(nv)]
    tuples = coefs if coefs is not None else [tuple(np.random.default_rng(950 + nv).standard_normal(nv))]

    def call(X, t):
        return X.k.mi355x_vec_maxpy_dev_norm2(X.h, X.n, nv, X.scal(t), -1.0, X.table(ys), X.p["x"], X.res)

    def ref(t, v):
        x = v["x"].copy(); orc.vec_maxpy(x, -1.0 * np.array(t), [v[y] for y in ys])
        return {"x": x}, [("dot", x, x)]
    return Case("maxpy_dev_norm2_%d" % nv, ["x"] + ys, ["x"], tuples, call, ref)


def _mdot_case(nv):
    ys = ["y%d" % j for j in range(nv)]
    return Case("mdot%d" % nv, ["x"] + ys, [], [()],
                lambda X, t: X.k.mi355x_vec_mdot(X.h, X.n, nv, X.p["x"], X.table(ys), X.res),
                lambda t, v: ({}, [("dot", v["x"], v[y]) for y in ys]))


def _cg_step(a, v, with_d, with_x=True):
    x, r = v.get("x"), v["r"]
    if a != 0.0:
        if with_x:
            x = x + a * v["p"]
        r = r + (-a) * v["w"]
    z = r * v["d"] if with_d else r.copy()
    return x, r, z


def _cg_refused(beta, dpi, dpiold, chk):
    return bool(np.isnan(dpi) or np.isinf(dpi) or dpi == 0.0 or (chk and dpi * dpiold <= 0.0))


def _cg_update_case(with_d):
    ops = ["p", "w"] + (["d"] if with_d else []) + ["x", "r", "z"]

    def call(X, t):
        return X.k.mi355x_vec_cg_update(X.h, X.n, t[0], X.p["p"], X.p["w"], X.p["d"] if with_d else None, X.p["x"], X.p["r"], X.p["z"], X.res)

    def ref(t, v):
        x, r, z = _cg_step(t[0], v, with_d)
        return {"x": x, "r": r, "z": z}, [("dot", z, z), ("dot", z, r), ("dot", r, r)]

    def wrong(t, v):                  # a sweep without VecAXPY's alpha == 0 exit (bvec1.c:253)
        if t[0] != 0.0:
            return None
        return {"x": v["x"] + t[0] * v["p"], "r": v["r"] + (-t[0]) * v["w"]}
    return Case("cg_update" + ("" if with_d else "_nod"), ops, ["x", "r", "z"], [(0.0,), (-0.0,), (0.731,)], call, ref, wrong)


# (beta, dpi, dpiold, check_sign): two accepted steps, then every refusal of cg.c:196-199
CG_DEV = [(0.83, 1.37, 0.5, 1), (0.83, -1.37, 0.5, 0), (0.83, 0.0, 1.0, 0), (0.83, -0.0, 1.0, 0), (0.83, NAN, 1.0, 0), (0.83, INF, 1.0, 0),
          (0.83, -INF, 1.0, 0), (0.83, -1.0, 2.0, 1)]


def _cg_update_dev_case(with_x, with_d=True):
    ops = (["p"] if with_x else []) + ["w"] + (["d"] if with_d else []) + (["x"] if with_x else []) + ["r", "z"]
    outs = (["x"] if with_x else []) + ["r", "z"]

    def call(X, t):
        beta, dpi, dpiold, chk = t
        d = X.p["d"] if with_d else None
        if with_x:
            return X.k.mi355x_vec_cg_update_dev(X.h, X.n, beta, X.scal([dpi]), dpiold, chk, X.p["p"], X.p["w"], d, X.p["x"], X.p["r"], X.p["z"], X.res, 0)
        return X.k.mi355x_vec_cg_update_dev_nox(X.h, X.n, beta, X.scal([dpi]), dpiold, chk, X.p["w"], d, X.p["r"], X.p["z"], X.res, 0)

    def ref(t, v):
        beta, dpi, dpiold, chk = t
        if _cg_refused(*t):           # nothing is modified, the sums are the +0.0 every lane starts from, dpi is handed through
            out = {"r": v["r"], "z": v["z"]}
            if with_x:
                out["x"] = v["x"]
            return out, [("val", 0.0), ("val", 0.0), ("val", 0.0), ("val", dpi + 0.0)]      # every other lane adds +0.0: -0.0 arrives as +0.0
        x, r, z = _cg_step(np.float64(beta) / np.float64(dpi), v, with_d, with_x)
        out = {"r": r, "z": z}
        if with_x:
            out["x"] = x
        return out, [("dot", z, z), ("dot", z, r), ("dot", r, r), ("val", dpi + 0.0)]
    return Case("cg_update_dev" + ("" if with_x else "_nox") + ("" if with_d else "_nod"), ops, outs, CG_DEV, call, ref)


# (num, den) then CGStepLen's (beta, dpi, dpiold, check_sign)
AYPX_DEV = [(0.9, 0.77), (0.0, 0.77), (-0.0, 0.77), (0.77, 0.77), (-0.77, 0.77)]
AYPX_DEV_X = [(0.9, 0.77) + t for t in CG_DEV] + [(0.0, 0.77) + CG_DEV[0], (-0.0, 0.77) + CG_DEV[2]]


def _aypx_alpha(num, den, v):
    alpha = np.float64(num) / np.float64(den)
    return v["x"].copy() if alpha == 0.0 else v["x"] + alpha * v["y"]


def _aypx_dev_x_ref(t, v):
    a = 0.0 if _cg_refused(*t[2:]) else np.float64(t[2]) / np.float64(t[3])
    return {"sol": v["sol"] + a * v["y"] if a != 0.0 else v["sol"], "y": _aypx_alpha(t[0], t[1], v)}, []


def _bcgs_ref(t, v):
    al, om = t
    x = _o(orc.vec_axpbypcz, v["x"], al, om, 1.0, v["p"], v["s"])
    r = np.zeros_like(x); orc.vec_waxpy(r, -om, v["t"], v["s"])
    return {"x": x, "r": r}, [("dot", r, r), ("dot", r, v["rp"])]


def _pmult(with_d, two):
    ops = ["x"] + (["d"] if with_d else []) + ["s" if two else "y", "w"]
    fn = "mi355x_vec_pmult_dotnorm2" if two else "mi355x_vec_pmult_dot"

    def call(X, t):
        return getattr(X.k, fn)(X.h, X.n, X.p["x"], X.p["d"] if with_d else None, X.p[ops[-2]], X.p["w"], X.res)

    def ref(t, v):
        w = v["x"] * v["d"] if with_d else v["x"].copy()
        return {"w": w}, ([("dot", v["s"], w), ("dot", w, w)] if two else [("dot", w, v["y"])])
    return Case(fn[len("mi355x_vec_"):] + ("" if with_d else "_nod"), ops, ["w"], [()], call, ref)


def _scale_rnorm_ref(norm2, x):
    """VecNormalize (rvector.c:308-314) on VecScale_Seq (bvec1.c:183) with numpy's correctly rounded sqrt and division"""
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float64(norm2))
        if nrm == 0.0 or nrm == 1.0:
            return x.copy()
        alpha = np.float64(1.0) / nrm
        if alpha == 1.0:
            return x.copy()
        return np.zeros_like(x) if alpha == 0.0 else x * alpha


def _scatter(kind):
    """pack / unpack through a permutation of [0, n) (X.perm(): device int array and its host copy)"""
    def call(X, t):
        k = X.k
        idx, _ = X.perm()
        if kind == "pack":
            return k.mi355x_pack(X.h, X.n, idx, X.p["x"], X.p["buf"])
        return getattr(k, "mi355x_unpack_" + kind)(X.h, X.n, idx, X.p["buf"], X.p["y"])

    def ref(t, v):
        pm = v["__perm__"]
        if kind == "pack":
            return {"buf": v["x"][pm]}, []
        y = v["y"].copy()
        if kind == "insert":
            y[pm] = v["buf"]
        elif kind == "add":
            y[pm] = y[pm] + v["buf"]
        else:
            a, b = y[pm], v["buf"]
            y[pm] = np.where(a < b, b, a)
        return {"y": y}, []
    return Case(kind if kind == "pack" else "unpack_" + kind, ["x", "buf"] if kind == "pack" else ["buf", "y"],
                ["buf"] if kind == "pack" else ["y"], [()], call, ref)


def _recip_ref(t, v):
    return {"x": _o(lambda x: orc.vec_reciprocal(x), v["x"])}, []


def _jac_ref(t, v):
    with np.errstate(all="ignore"):
        return {"d": np.where(v["d"] == 0.0, 1.0, 1.0 / v["d"])}, []


def _div_ref(t, v):
    w = np.zeros_like(v["x"]); orc.vec_pointwise_divide(w, v["x"], v["y"])
    return {"w": w}, []


def _mul_ref(out):
    def ref(t, v):
        w = np.zeros_like(v["x"]); orc.vec_pointwise_mult(w, v["x"], v["y"])
        return {out: w}, []
    return ref


def _waxpy_ref(t, v):
    w = np.zeros_like(v["x"]); orc.vec_waxpy(w, t[0], v["x"], v["y"])
    return {"w": w}, []


# the 14 element-wise entry points (+ the aliased forms of pointwise_mult), jacobi_invert and stream_triad
ELEMENTWISE = [
    Case("axpy", ["x", "y"], ["y"], ALPHAS, lambda X, t: X.k.mi355x_vec_axpy(X.h, X.n, t[0], X.p["x"], X.p["y"]),
         lambda t, v: ({"y": _o(orc.vec_axpy, v["y"], t[0], v["x"])}, []),
         lambda t, v: {"y": v["y"] + t[0] * v["x"]} if t[0] == 0.0 else None),
    Case("aypx", ["x", "y"], ["y"], ALPHAS, lambda X, t: X.k.mi355x_vec_aypx(X.h, X.n, t[0], X.p["x"], X.p["y"]),
         lambda t, v: ({"y": _o(orc.vec_aypx, v["y"], t[0], v["x"])}, []),
         lambda t, v: {"y": v["x"] + t[0] * v["y"]} if t[0] == 0.0 else None),
    Case("waxpy", ["x", "y", "w"], ["w"], ALPHAS, lambda X, t: X.k.mi355x_vec_waxpy(X.h, X.n, t[0], X.p["x"], X.p["y"], X.p["w"]),
         _waxpy_ref, lambda t, v: {"w": v["y"] + t[0] * v["x"]} if t[0] == 0.0 else None),
    Case("scale", ["x"], ["x"], ALPHAS[:6], lambda X, t: X.k.mi355x_vec_scale(X.h, X.n, t[0], X.p["x"]),
         lambda t, v: ({"x": _o(orc.vec_scale, v["x"], t[0])}, []),
         lambda t, v: {"x": t[0] * v["x"]} if t[0] == 0.0 else None),
    Case("axpby", ["x", "y"], ["y"], AB, lambda X, t: X.k.mi355x_vec_axpby(X.h, X.n, t[0], t[1], X.p["x"], X.p["y"]),
         lambda t, v: ({"y": _o(orc.vec_axpby, v["y"], t[0], t[1], v["x"])}, []), _axpby_wrong),
    Case("axpbypcz", ["x", "y", "z"], ["z"], ABC,
         lambda X, t: X.k.mi355x_vec_axpbypcz(X.h, X.n, t[0], t[1], t[2], X.p["x"], X.p["y"], X.p["z"]),
         lambda t, v: ({"z": _o(orc.vec_axpbypcz, v["z"], t[0], t[1], t[2], v["x"], v["y"])}, []), _axpbypcz_wrong),
    Case("pointwise_mult", ["x", "y", "w"], ["w"], [()], lambda X, t: X.k.mi355x_vec_pointwise_mult(X.h, X.n, X.p["x"], X.p["y"], X.p["w"]), _mul_ref("w")),
    Case("pointwise_mult_w_is_x", ["x", "y"], ["x"], [()], lambda X, t: X.k.mi355x_vec_pointwise_mult(X.h, X.n, X.p["x"], X.p["y"], X.p["x"]), _mul_ref("x")),
    Case("pointwise_mult_w_is_y", ["x", "y"], ["y"], [()], lambda X, t: X.k.mi355x_vec_pointwise_mult(X.h, X.n, X.p["x"], X.p["y"], X.p["y"]), _mul_ref("y")),
    Case("pointwise_divide", ["x", "y", "w"], ["w"], [()], lambda X, t: X.k.mi355x_vec_pointwise_divide(X.h, X.n, X.p["x"], X.p["y"], X.p["w"]), _div_ref),
    Case("reciprocal", ["x"], ["x"], [()], lambda X, t: X.k.mi355x_vec_reciprocal(X.h, X.n, X.p["x"]), _recip_ref),
    Case("jacobi_invert", ["d"], ["d"], [()], lambda X, t: X.k.mi355x_vec_jacobi_invert(X.h, X.n, X.p["d"], None), _jac_ref),
    Case("set", ["x"], ["x"], [(3.25,), (-0.0,), (MIN_SUB,), (-INF,)], lambda X, t: X.k.mi355x_vec_set(X.h, X.n, t[0], X.p["x"]),
         lambda t, v: ({"x": np.full(v["x"].size, t[0])}, [])),
    Case("copy", ["x", "y"], ["y"], [()], lambda X, t: X.k.mi355x_vec_copy(X.h, X.n, X.p["x"], X.p["y"]), lambda t, v: ({"y": v["x"].copy()}, [])),
    Case("swap", ["x", "y"], ["x", "y"], [()], lambda X, t: X.k.mi355x_vec_swap(X.h, X.n, X.p["x"], X.p["y"]),
         lambda t, v: ({"x": v["y"].copy(), "y": v["x"].copy()}, [])),
    Case("stream_triad", ["b", "c", "a"], ["a"], [(0.37,), (0.0,)], lambda X, t: X.k.mi355x_stream_triad(X.h, X.n, t[0], X.p["b"], X.p["c"], X.p["a"]),
         lambda t, v: ({"a": v["b"] + t[0] * v["c"]}, [])),
]
MAXPY_ZERO = [(0.0, 0.37, -1.2), (0.9, -0.0, 0.4), (0.3, 0.7, 0.0)]
MAXPY_SPECIAL = _maxpy_case(3, MAXPY_ZERO)                 # a zero coefficient against Inf / NaN columns: NaN must appear

REDUCTIONS = [
    Case("dot", ["x", "y"], [], [()], lambda X, t: X.k.mi355x_vec_dot(X.h, X.n, X.p["x"], X.p["y"], X.res), lambda t, v: ({}, [("dot", v["x"], v["y"])])),
    Case("norm0", ["x"], [], [()], lambda X, t: X.k.mi355x_vec_norm(X.h, X.n, 0, X.p["x"], X.res), lambda t, v: ({}, [("abs", v["x"])])),
    Case("norm1", ["x"], [], [()], lambda X, t: X.k.mi355x_vec_norm(X.h, X.n, 1, X.p["x"], X.res), lambda t, v: ({}, [("dot", v["x"], v["x"])])),
    Case("norm2", ["x"], [], [()], lambda X, t: X.k.mi355x_vec_norm(X.h, X.n, 2, X.p["x"], X.res), lambda t, v: ({}, [("dot", v["x"], v["x"])])),
    Case("norm3", ["x"], [], [()], lambda X, t: X.k.mi355x_vec_norm(X.h, X.n, 3, X.p["x"], X.res), lambda t, v: ({}, [("max", v["x"])])),
    Case("norm4", ["x"], [], [()], lambda X, t: X.k.mi355x_vec_norm(X.h, X.n, 4, X.p["x"], X.res), lambda t, v: ({}, [("abs", v["x"]), ("dot", v["x"], v["x"])])),
    Case("dotnorm2", ["s", "t"], [], [()], lambda X, t: X.k.mi355x_vec_dotnorm2(X.h, X.n, X.p["s"], X.p["t"], X.res),
         lambda t, v: ({}, [("dot", v["s"], v["t"]), ("dot", v["t"], v["t"])])),
    _mdot_case(5),
]

FUSED = [
    _cg_update_case(True), _cg_update_case(False),
    _cg_update_dev_case(True), _cg_update_dev_case(True, False), _cg_update_dev_case(False), _cg_update_dev_case(False, False),
    Case("aypx_dev", ["x", "y"], ["y"], AYPX_DEV, lambda X, t: X.k.mi355x_vec_aypx_dev(X.h, X.n, X.scal([t[0]]), t[1], X.p["x"], X.p["y"]),
         lambda t, v: ({"y": _aypx_alpha(t[0], t[1], v)}, []),
         lambda t, v: {"y": v["x"] + (np.float64(t[0]) / t[1]) * v["y"]} if t[0] == 0.0 else None),
    Case("aypx_dev_x", ["x", "y", "sol"], ["y", "sol"], AYPX_DEV_X,
         lambda X, t: X.k.mi355x_vec_aypx_dev_x(X.h, X.n, X.scal([t[0], t[3]]), t[1], X.p["x"], X.p["y"], t[2], C.c_void_p(X.scal_ptr.value + 8), t[4], t[5], X.p["sol"]),
         _aypx_dev_x_ref),
    _pmult(True, False), _pmult(False, False), _pmult(True, True), _pmult(False, True),
    Case("bcgs_update", ["p", "s", "t", "rp", "x", "r"], ["x", "r"], BCGS,
         lambda X, t: X.k.mi355x_vec_bcgs_update(X.h, X.n, t[0], t[1], X.p["p"], X.p["s"], X.p["t"], X.p["rp"], X.p["x"], X.p["r"], X.res),
         _bcgs_ref, lambda t, v: {"r": v["s"] + (-t[1]) * v["t"]} if t[1] == 0.0 else None),
    _maxpy_norm_case(3, [(0.0, 0.37, -1.2), (0.9, -0.0, 0.4)]),
]
# norm2 values for scale_rnorm_dev after the fused MAXPY (Part C) and the edges of Part F
RNORM_EDGES = [0.0, -0.0, 1.0, float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0)), 4.0, INF, NAN, MIN_SUB, DBL_MAX, DBL_MIN]
SCALE_RNORM = Case("scale_rnorm_dev", ["x"], ["x"], [(v,) for v in RNORM_EDGES + [0.731, 1e-200, 3e200]],
                   lambda X, t: X.k.mi355x_vec_scale_rnorm_dev(X.h, X.n, X.scal([t[0]]), X.p["x"]),
                   lambda t, v: ({"x": _scale_rnorm_ref(t[0], v["x"])}, []),
                   lambda t, v: {"x": v["x"] * 0.0} if np.isinf(t[0]) else None)      # 1/Inf = 0: VecScale sets zero, it does not multiply
SCATTER = [_scatter("pack"), _scatter("insert"), _scatter("add"), _scatter("max")]


def guard_band_cases():
    """Part A: every Vec entry point"""
    return (ELEMENTWISE + [_maxpy_case(nv) for nv in (1, 3, 4, 7)] + REDUCTIONS[:-1] + [_mdot_case(1), _mdot_case(5)] + FUSED[:-1]
            + [_maxpy_norm_case(5), SCALE_RNORM] + SCATTER)


def alignment_patterns(nops):
    """all aligned, all 8 bytes off, each single operand 8 bytes off"""
    pats = [(0,) * nops, (1,) * nops]
    if nops > 1:
        pats += [tuple(int(i == j) for i in range(nops)) for j in range(nops)]
    return pats


def operands(case, n, rot, share=SHARE, kinds=KINDS, finite=False):
    """the host operands of a case: special vectors (or plain normal data for `finite`), one seed per operand"""
    v = {}
    for j, name in enumerate(case.ops):
        seed = 11 + 7 * j
        v[name] = np.random.default_rng(seed + 1000 * n).standard_normal(n) if finite else special_vector(n, seed, share, rot, kinds)
    v["__perm__"] = np.random.default_rng(5 + n).permutation(n).astype(np.int32)
    return v


def finite_tuples(case):
    return [t for t in case.tuples if all(np.isfinite(s) for s in t)]


def sum_value(s):
    """the reference value of one sum in the oracle's current order, and sum |terms|"""
    with np.errstate(all="ignore"):
        if s[0] == "dot":
            return dsum(s[1], s[2]), float(np.sum(np.abs(s[1] * s[2])))
        if s[0] == "abs":
            return asum(s[1]), float(np.sum(np.abs(s[1])))
        if s[0] == "max":
            return orc.vec_norm(np.ascontiguousarray(s[1]), 3), 0.0
        return s[1], 0.0


def klass(v):
    v = float(v)
    return "nan" if np.isnan(v) else "+inf" if v == INF else "-inf" if v == -INF else "finite"


# ---- Part D: where a special is placed, and the special vectors of the reductions
D_OPS = ["x", "y", "s", "t"] + ["y%d" % j for j in range(5)]


def reduction_grid(n):
    """workgroups of a reduction over a vector that fits the caches (launch_reduce)"""
    return min(max((n + 4095) // 4096, 1), 512)


def reduction_positions(n):
    """element 0, the odd tail, the middle of workgroup 0, an element of the last workgroup, and at the largest size an element
    whose workgroup index is >= 256 (grid-stride: pair i belongs to workgroup (i / 256) mod grid)"""
    grid = reduction_grid(n)
    pos = {"first": 0, "tail": n - 1, "mid_wg0": min(2 * 128 + 1, n - 1), "last_wg": min(2 * (256 * (grid - 1) + 37), n - 2) if n > 2 else 0}
    if grid > 256:
        pos["wg>=256"] = 2 * (256 * 300 + 5) + 1
    return pos


def reduction_vectors(n, rot, kinds):
    """x, y, s, t special vectors of their own, the five MDot columns y rolled"""
    v = {name: special_vector(n, 40 + j, SHARE, rot, kinds) for j, name in enumerate(D_OPS[:4])}
    for j in range(5):
        v["y%d" % j] = np.roll(v["y"], 37 * (j + 1))
    return v
