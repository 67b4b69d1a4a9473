"""The fused Vec forms of host/vechip.c called directly (P.lib().raw), not through a KSP solve.

Refusals -- an operand of another local size, a written operand passed again in another slot (but for the permitted pairs), a required
operand missing, an enum or a count out of range, an operand that never got a type -- return 0 with done == 0, leave every operand bit for
bit as it was and take none of the Vec type's shortcuts.  Accepted calls -- the normal form, every permitted alias pair, every special case
that leaves a written operand unmarked -- give every operand the bits the wrapped kernel leaves in raw device buffers from the same inputs,
return the kernel's own sums, and leave every operand's norm() equal to that of a fresh vector with the same entries (a missing state
increase would answer from the norm kept per object state, a missing restore would show the old host copy).

The local size is 5; 1025 as well for the accepted calls, so that the reductions cross a tile.  The kernels have their own files.

VecCGUpdate / VecCGUpdateCheck: x or r given again as p, w or d is not among the refusals here -- the chain of comparisons this file was
first written against lets those through, the operand gate refuses them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
PD, PI = C.POINTER(dbl), C.POINTER(i32)
N = 5
SIZES = [5, 1025]


@pytest.fixture(scope="module")
def env(built):
    from gpu import Dev
    from petsc_dev_amd import petsc as P
    d = Dev()
    yield d, P
    d.free_all()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def data(n, seed):
    return np.random.default_rng([n, seed]).standard_normal(n)


class Form:
    """One wrapper: `ops` in the order of its C arguments, the names it writes, the pairs that may be one object, what may be NULL."""

    def __init__(self, name, argtypes, ops, written, optional=(), permitted=(), scalars=None, nsums=0):
        self.name, self.argtypes, self.ops, self.written = name, argtypes, ops, written
        self.optional, self.permitted = set(optional), {frozenset(p) for p in permitted}
        self.scalars, self.nsums = dict(scalars or {}), nsums

    def fn(self, P):
        f = P.lib().raw(self.name)
        f.argtypes, f.restype = self.argtypes, i32
        return f

    def call(self, P, V, s):
        """-> (return code, done, sums); V: name -> Vec handle or None"""
        raise NotImplementedError

    def kernel(self, dev, n, B, s):
        """the wrapped kernel(s) on raw buffers B: name -> pointer or None; -> sums"""
        raise NotImplementedError


def outs(k):
    return [dbl(-7.0) for _ in range(k)]


def handles(V, names):
    return [V.get(n) for n in names]


# ------------------------------------------------------------------------------------------------ the forms
class CGUpdate(Form):
    def __init__(self):
        super().__init__("VecCGUpdate_HIPMI355X", [vp] * 6 + [dbl, PD, PD, PD, PI], ("x", "r", "z", "p", "w", "d"), ("x", "r", "z"),
                         optional=("d",), permitted=[("z", "w")], scalars=dict(a=0.37), nsums=3)

    def call(self, P, V, s):
        o, done = outs(3), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["a"], *[C.byref(v) for v in o], C.byref(done))
        return rc, done.value, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(4))
        dev.chk(dev.k.mi355x_vec_cg_update(dev.h, n, s["a"], B["p"], B["w"], B.get("d"), B["x"], B["r"], B["z"], out))
        return list(dev.get(out, 3))


class CGCheck(Form):
    def __init__(self):
        super().__init__("VecCGUpdateCheck_HIPMI355X", [vp] * 6 + [PI], ("x", "r", "z", "p", "w", "d"), ("x", "r", "z"), optional=("d",),
                         permitted=[("z", "w")])

    def call(self, P, V, s):
        ok = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), C.byref(ok))
        return rc, ok.value, []

    def kernel(self, dev, n, B, s):
        return []


class TDotBegin(Form):
    def __init__(self):
        super().__init__("VecTDotBegin_HIPMI355X", [vp, vp, PI], ("x", "y"), ())

    def call(self, P, V, s):
        ok = i32(-1)
        rc = self.fn(P)(V.get("x"), V.get("y"), C.byref(ok))
        return rc, ok.value, []

    def kernel(self, dev, n, B, s):
        return []


class CGDev(Form):
    """VecTDotBegin(p, w); VecCGUpdateDevBegin; VecAYPXDev(p, den, z); VecCGUpdateDevEnd -- or, nox, the x-less sweep and VecAYPXDevX"""

    def __init__(self, nox):
        self.nox = nox
        super().__init__("VecCGUpdateDevBegin%s_HIPMI355X" % ("NoX" if nox else ""), None, ("x", "r", "z", "p", "w", "d"), ("x", "r", "z", "p"),
                         optional=("d",), permitted=[("z", "w")], scalars=dict(beta=0.7, dpiold=1.0, chk=0, den=0.9), nsums=4)

    def call(self, P, V, s):
        L = P.lib()
        ok, o = i32(-1), outs(4)

        def raw(name, argtypes):
            f = L.raw(name)
            f.argtypes, f.restype = argtypes, i32
            return f
        rc = raw("VecTDotBegin_HIPMI355X", [vp, vp, PI])(V["p"], V["w"], C.byref(ok))
        assert rc == 0 and ok.value == 1
        if self.nox:
            rc = raw("VecCGUpdateDevBeginNoX_HIPMI355X", [vp] * 4 + [dbl, dbl, i32])(V["r"], V["z"], V["w"], V.get("d"), s["beta"], s["dpiold"], s["chk"])
            assert rc == 0
            rc = raw("VecAYPXDevX_HIPMI355X", [vp, dbl, vp, vp, dbl, dbl, i32])(V["p"], s["den"], V["z"], V["x"], s["beta"], s["dpiold"], s["chk"])
        else:
            rc = raw("VecCGUpdateDevBegin_HIPMI355X", [vp] * 6 + [dbl, dbl, i32])(*handles(V, self.ops), s["beta"], s["dpiold"], s["chk"])
            assert rc == 0
            rc = raw("VecAYPXDev_HIPMI355X", [vp, dbl, vp])(V["p"], s["den"], V["z"])
        assert rc == 0
        rc = raw("VecCGUpdateDevEnd_HIPMI355X", [vp, PD, PD, PD, PD])(V["x"], *[C.byref(v) for v in o])
        return rc, 1, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        k = dev.k
        out, dpi = dev.put(np.zeros(4)), dev.put(np.zeros(2))
        one = C.c_void_p(out.value + 8)
        dev.chk(k.mi355x_vec_dot(dev.h, n, B["p"], B["w"], dpi))
        if self.nox:
            dev.chk(k.mi355x_vec_cg_update_dev(dev.h, n, s["beta"], dpi, s["dpiold"], s["chk"], None, B["w"], B.get("d"), None, B["r"], B["z"], out, 0))
            dev.chk(k.mi355x_vec_aypx_dev_x(dev.h, n, one, s["den"], B["z"], B["p"], s["beta"], dpi, s["dpiold"], s["chk"], B["x"]))
        else:
            dev.chk(k.mi355x_vec_cg_update_dev(dev.h, n, s["beta"], dpi, s["dpiold"], s["chk"], B["p"], B["w"], B.get("d"), B["x"], B["r"], B["z"], out, 0))
            dev.chk(k.mi355x_vec_aypx_dev(dev.h, n, one, s["den"], B["z"], B["p"]))
        return list(dev.get(out, 4))


class PMultDot(Form):
    def __init__(self, two):
        self.two = two
        super().__init__("VecPMultDotNorm2_HIPMI355X" if two else "VecPMultDot_HIPMI355X", [vp] * 4 + [PD] * (2 if two else 1) + [PI],
                         ("w", "x", "d", "y"), ("w",), optional=("d",), nsums=2 if two else 1)

    def call(self, P, V, s):
        o, done = outs(self.nsums), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), *[C.byref(v) for v in o], C.byref(done))
        return rc, done.value, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        f = dev.k.mi355x_vec_pmult_dotnorm2 if self.two else dev.k.mi355x_vec_pmult_dot
        dev.chk(f(dev.h, n, B["x"], B.get("d"), B["y"], B["w"], out))
        return list(dev.get(out, self.nsums))


class BCGSUpdate(Form):
    def __init__(self):
        super().__init__("VecBCGSUpdate_HIPMI355X", [vp] * 6 + [dbl, dbl, PD, PD, PI], ("x", "r", "p", "s", "t", "rp"), ("x", "r"),
                         scalars=dict(alpha=0.4, omega=-0.6), nsums=2)

    def call(self, P, V, s):
        o, done = outs(2), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["alpha"], s["omega"], C.byref(o[0]), C.byref(o[1]), C.byref(done))
        return rc, done.value, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_bcgs_update(dev.h, n, s["alpha"], s["omega"], B["p"], B["s"], B["t"], B["rp"], B["x"], B["r"], out))
        return list(dev.get(out, 2))


class ChebyStep(Form):
    def __init__(self):
        super().__init__("VecChebyStep_HIPMI355X", [vp] * 7 + [dbl, dbl, dbl, PD, PD, PI], ("pn", "r", "w", "b", "d", "pm", "pk"), ("pn", "r"),
                         optional=("r", "b", "d"), permitted=[("r", "w")], scalars=dict(s=0.8, a=0.3, c=-0.2, sums=1), nsums=2)

    def call(self, P, V, s):
        o, done = outs(2), i32(-1)
        zz, rr = (C.byref(o[0]), C.byref(o[1])) if s["sums"] else (None, None)
        rc = self.fn(P)(*handles(V, self.ops), s["s"], s["a"], s["c"], zz, rr, C.byref(done))
        return rc, done.value, [v.value for v in o] if s["sums"] else []

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_cheby_step(dev.h, n, s["s"], s["a"], s["c"], B["w"], B.get("b"), B.get("d"), B["pm"], B["pk"], B.get("r"), B["pn"],
                                            s["sums"], out if s["sums"] else None))
        return list(dev.get(out, 2)) if s["sums"] else []


class RichStep(Form):
    def __init__(self):
        super().__init__("VecRichStep_HIPMI355X", [vp] * 6 + [dbl, PI], ("x", "r", "z", "w", "b", "d"), ("x", "r", "z"), optional=("r", "z", "d"),
                         permitted=[("r", "w")], scalars=dict(scale=0.9))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["scale"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        dev.chk(dev.k.mi355x_vec_rich_step(dev.h, n, s["scale"], B["w"], B["b"], B.get("d"), B.get("r"), B.get("z"), B["x"]))
        return []


class PipeCGStep(Form):
    def __init__(self):
        super().__init__("VecPipeCGStep_HIPMI355X", [vp] * 12 + [i32, dbl, dbl, i32, PI],
                         ("x", "u", "w", "r", "zrec", "qrec", "p", "s", "nv", "mv", "d", "m_next"), ("x", "u", "w", "r", "zrec", "qrec", "p", "s", "m_next"),
                         optional=("d", "m_next"), permitted=[("m_next", "mv")], scalars=dict(first=0, ratio=0.6, step=0.3, rides=0), nsums=2)

    def call(self, P, V, s):
        done, L = i32(-1), P.lib()
        if s["rides"] and V.get("w") and V.get("u"):        # one split phase of the public calls first, as every solver start has: it names the type's phase to the library
            t = dbl()
            L.VecDotBegin(V["w"], V["u"], C.byref(t))
            L.PetscCommSplitReductionBegin(L.COMM_SELF)
            L.VecDotEnd(V["w"], V["u"], C.byref(t))
        rc = self.fn(P)(*handles(V, self.ops), s["first"], s["ratio"], s["step"], s["rides"], C.byref(done))
        sums = []
        if rc == 0 and done.value == 1 and s["rides"]:      # the two sums are pending as a Begin of what rides and VecDotBegin(w, u) leave them
            a, b = dbl(), dbl()
            L.PetscCommSplitReductionBegin(L.COMM_SELF)
            if s["rides"] == 3:
                L.VecDotEnd(V["r"], V["u"], C.byref(a))
            else:
                L.VecNormEnd(V["r"] if s["rides"] == 1 else V["u"], P.NORM_2, C.byref(a))
            L.VecDotEnd(V["w"], V["u"], C.byref(b))
            sums = [b.value, a.value]
        return rc, done.value, sums

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_pipecg_step(dev.h, n, s["first"], s["ratio"], s["step"], B["nv"], B["mv"], B.get("d"), B["zrec"], B["qrec"], B["p"], B["s"],
                                             B["x"], B["u"], B["w"], B["r"], B.get("m_next"), s["rides"], out if s["rides"] else None))
        if not s["rides"]:
            return []
        v = dev.get(out, 2)
        return [v[0], v[1] if s["rides"] == 3 else np.sqrt(v[1])]


class MinresLanczos(Form):
    def __init__(self):
        super().__init__("VecMinresLanczos_HIPMI355X", [vp] * 7 + [dbl, i32, dbl, PD, PD, PI], ("r", "z", "v", "u", "vold", "uold", "d"), ("r", "z"),
                         optional=("d",), scalars=dict(alpha=0.45, beta=-0.35), nsums=2)

    def call(self, P, V, s):
        o, done = outs(2), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["alpha"], 0, s["beta"], C.byref(o[0]), C.byref(o[1]), C.byref(done))
        return rc, done.value, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_minres_lanczos(dev.h, n, s["alpha"], None, s["beta"], B.get("d"), B["r"], B["z"], B["v"], B["u"], B["vold"], B["uold"], out))
        return list(dev.get(out, 2))


class MinresUpdate(Form):
    def __init__(self):
        super().__init__("VecMinresUpdate_HIPMI355X", [vp] * 8 + [i32] + [dbl] * 5 + [PI], ("x", "u", "w", "wold", "r", "z", "vnew", "unew"),
                         ("x", "wold", "vnew", "unew"), scalars=dict(first=0, rho2=0.3, rho3=-0.2, irho1=1.7, ceta=0.4, ibeta=0.8))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["first"], s["rho2"], s["rho3"], s["irho1"], s["ceta"], s["ibeta"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        dev.chk(dev.k.mi355x_vec_minres_update(dev.h, n, s["first"], s["rho2"], s["rho3"], s["irho1"], s["ceta"], s["ibeta"], B.get("u"), B.get("w"),
                                               B.get("wold"), B.get("x"), B["r"], B["z"], B["vnew"], B["unew"]))
        return []


class TfqmrQT(Form):
    def __init__(self):
        super().__init__("VecTfqmrQT_HIPMI355X", [vp] * 5 + [dbl, PI], ("u", "v", "q", "t", "x"), ("q", "t", "x"), optional=("x",), scalars=dict(a=0.41))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["a"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        dev.chk(dev.k.mi355x_vec_tfqmr_qt(dev.h, n, s["a"], B["u"], B["v"], B["q"], B["t"], B.get("x")))
        return []


class TfqmrResid(Form):
    def __init__(self):
        super().__init__("VecTfqmrResid_HIPMI355X", [vp] * 3 + [dbl, PD, PD, PI], ("r", "auq", "rp"), ("r",), scalars=dict(a=0.41), nsums=2)

    def call(self, P, V, s):
        o, done = outs(2), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["a"], C.byref(o[0]), C.byref(o[1]), C.byref(done))
        return rc, done.value, [v.value for v in o]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        dev.chk(dev.k.mi355x_vec_tfqmr_resid(dev.h, n, s["a"], B["auq"], B["rp"], B["r"], out))
        return list(dev.get(out, 2))


class TfqmrUpdate(Form):
    def __init__(self):
        super().__init__("VecTfqmrUpdate_HIPMI355X", [vp] * 6 + [i32, dbl, dbl, dbl, dbl, i32, dbl, PI], ("d", "x", "u", "q", "r", "p"),
                         ("d", "x", "u", "q", "p"), scalars=dict(nhalves=2, cf0=0.83, eta0=-0.29, cf1=1.7, eta1=0.61, tail=1, b=0.47))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["nhalves"], s["cf0"], s["eta0"], s["cf1"], s["eta1"], s["tail"], s["b"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        nh, tail = s["nhalves"], s["tail"]
        if nh == 0 and not tail:
            return []
        g = lambda name, used: B.get(name) if used else None     # the wrapper hands the kernel only what the form touches
        dev.chk(dev.k.mi355x_vec_tfqmr_update(dev.h, n, nh, s["cf0"], s["eta0"], s["cf1"], s["eta1"], tail, s["b"], g("d", nh >= 1), g("x", nh >= 1),
                                              g("u", nh >= 1 or tail), g("q", nh == 2 or tail), g("r", tail), g("p", tail)))
        return []


class BicgDirs(Form):
    def __init__(self):
        super().__init__("VecBicgDirs_HIPMI355X", [vp] * 4 + [dbl, i32, PI], ("pr", "pl", "zr", "zl"), ("pr", "pl"), scalars=dict(b=0.55, first=0))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["b"], s["first"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        dev.chk(dev.k.mi355x_vec_bicg_dirs(dev.h, n, s["first"], s["b"], B["zr"], B["zl"], B["pr"], B["pl"]))
        return []


class BicgUpdate(Form):
    def __init__(self):
        super().__init__("VecBicgUpdate_HIPMI355X", [vp] * 7 + [i32, dbl, i32, PD, PD, PI], ("x", "rr", "rl", "pr", "zr", "zl", "d"),
                         ("x", "rr", "rl", "zr", "zl"), optional=("d",), scalars=dict(identity=0, a=0.33, which=0), nsums=2)

    def call(self, P, V, s):
        o, done = outs(2), i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["identity"], s["a"], s["which"], C.byref(o[0]), C.byref(o[1]), C.byref(done))
        pcmode = 1 if V.get("d") else (2 if s["identity"] else 0)
        return rc, done.value, [o[0].value if pcmode else None, o[1].value]

    def kernel(self, dev, n, B, s):
        out = dev.put(np.zeros(2))
        pcmode = 1 if B.get("d") else (2 if s["identity"] else 0)
        dev.chk(dev.k.mi355x_vec_bicg_update(dev.h, n, s["a"], pcmode, s["which"], B["pr"], B.get("d"), B["x"], B["rr"], B["rl"], B["zr"], B["zl"], out))
        v = dev.get(out, 2)
        return [v[0] if pcmode else None, v[1]]


WAIT, QUEUE, FINISH = 0, 1, 2


class LsqrBidiag(Form):
    def __init__(self):
        super().__init__("VecLsqrBidiag_HIPMI355X", [vp, vp, dbl, i32, PD, PI], ("x", "y"), ("y",), scalars=dict(coef=0.6, route=WAIT), nsums=1)

    def call(self, P, V, s):
        o, done = (dbl * 2)(-7.0, -7.0), i32(-1)
        rc = self.fn(P)(V.get("x"), V.get("y"), s["coef"], s["route"], o, C.byref(done))
        return rc, done.value, {WAIT: [o[0]], QUEUE: [], FINISH: [o[0], o[1]]}.get(s["route"], [])

    def kernel(self, dev, n, B, s):
        out = s.get("slot") or dev.put(np.zeros(2))
        nxt = C.c_void_p(out.value + 8)
        if s["route"] == WAIT:
            dev.chk(dev.k.mi355x_vec_lsqr_bidiag(dev.h, n, s["coef"], None, B["x"], B["y"], out))
            return list(dev.get(out, 1))
        if s["route"] == QUEUE:
            dev.chk(dev.k.mi355x_vec_lsqr_bidiag(dev.h, n, s["coef"], None, B["x"], B["y"], out))
            dev.chk(dev.k.mi355x_vec_scale_rnorm_dev(dev.h, n, out, B["y"]))
            return []
        dev.chk(dev.k.mi355x_vec_lsqr_bidiag(dev.h, n, 0.0, out, B["x"], B["y"], nxt))
        return list(dev.get(out, 2))


class LsqrUpdate(Form):
    def __init__(self):
        super().__init__("VecLsqrUpdate_HIPMI355X", [vp] * 4 + [dbl] * 4 + [i32, PI], ("v1", "x", "w", "se"), ("v1", "x", "w", "se"), optional=("se",),
                         scalars=dict(ialpha=0.7, step=0.35, cf=-0.45, irho2=0.2, skip_w=0))

    def call(self, P, V, s):
        done = i32(-1)
        rc = self.fn(P)(*handles(V, self.ops), s["ialpha"], s["step"], s["cf"], s["irho2"], s["skip_w"], C.byref(done))
        return rc, done.value, []

    def kernel(self, dev, n, B, s):
        skip, se = s["skip_w"], B.get("se")
        v1 = None if skip and s["ialpha"] == 1.0 else B.get("v1")
        x = None if s["step"] == 0.0 else B.get("x")
        w = None if skip and s["step"] == 0.0 and not se else B.get("w")
        if not (v1 or x or w or se):
            return []
        dev.chk(dev.k.mi355x_vec_lsqr_update(dev.h, n, s["ialpha"], s["step"], s["cf"], s["irho2"], skip, v1, x, w, se))
        return []


class Orthog(Form):
    """VecGMRESOrthogNormalize (flexible: VecFgmresOrthogNormalizePC) with nv basis vectors V0, V1, ..."""

    def __init__(self, flexible, nv=3):
        self.flexible, self.nv = flexible, nv
        basis = tuple("V%d" % j for j in range(nv))
        if flexible:
            super().__init__("VecFgmresOrthogNormalizePC_HIPMI355X", [vp, i32, vp, vp, i32, vp, PD, PD, PI], ("w",) + basis + ("d", "z"), ("w", "z"),
                             optional=("d",), scalars=dict(identity=0, nv=nv), nsums=nv + 1)
        else:
            super().__init__("VecGMRESOrthogNormalize_HIPMI355X", [vp, i32, vp, PD, PD, PI], ("w",) + basis, ("w",), scalars=dict(nv=nv), nsums=nv + 1)

    def call(self, P, V, s):
        nv = self.nv
        tab = (vp * 34)()                                   # room for the 33 a refused count names
        for j in range(34):
            h = V.get("V%d" % min(j, nv - 1))
            tab[j] = h.value if h is not None else None
        dots, nrm, done = (dbl * 34)(), dbl(-7.0), i32(-1)
        if self.flexible:
            rc = self.fn(P)(V.get("w"), s["nv"], tab, V.get("d"), s["identity"], V.get("z"), dots, C.byref(nrm), C.byref(done))
        else:
            rc = self.fn(P)(V.get("w"), s["nv"], tab, dots, C.byref(nrm), C.byref(done))
        return rc, done.value, [dots[j] for j in range(nv)] + [nrm.value]

    def kernel(self, dev, n, B, s):
        nv, k = self.nv, dev.k
        ds = dev.put(np.zeros(nv + 2))
        last = C.c_void_p(ds.value + 8 * nv)
        tab = dev.ptr_table([B["V%d" % j] for j in range(nv)])
        dev.chk(k.mi355x_vec_mdot(dev.h, n, nv, B["w"], tab, ds))
        dev.chk(k.mi355x_vec_maxpy_dev_norm2(dev.h, n, nv, ds, -1.0, tab, B["w"], last))
        if self.flexible:
            dev.chk(k.mi355x_vec_scale_rnorm_dev_pmult(dev.h, n, last, B["w"], B.get("d"), B["z"]))
        else:
            dev.chk(k.mi355x_vec_scale_rnorm_dev(dev.h, n, last, B["w"]))
        v = dev.get(ds, nv + 1)
        return list(v[:nv]) + [np.sqrt(v[nv])]


GATED = [CGUpdate(), CGCheck(), TDotBegin(), PMultDot(False), PMultDot(True), BCGSUpdate(), ChebyStep(), RichStep(), PipeCGStep(), MinresLanczos(), MinresUpdate(),
         TfqmrQT(), TfqmrResid(), TfqmrUpdate(), BicgDirs(), BicgUpdate(), LsqrBidiag(), LsqrUpdate(), Orthog(False), Orthog(True)]
IDS = [f.name.replace("_HIPMI355X", "") for f in GATED]


# ------------------------------------------------------------------------------------------------ the two checks
def counts(P):
    c = (i32 * 8)()
    P.lib().VecHIPMI355XGetDeferralCounts(c)
    return list(c)


def make(P, form, n, absent=(), alias=None, sizes=None, untyped=None):
    """-> (host: name -> array, vecs: name -> Vec); alias: slot -> the slot whose vector it gets too"""
    L = P.lib()
    host, vecs = {}, {}
    for j, name in enumerate(form.ops):
        if name in absent or (alias and name in alias):
            continue
        if name == untyped:                                  # created and sized, never given a type: no storage, not a HIPMI355X vector
            v = P.Vec()
            L.VecCreate(L.COMM_SELF, C.byref(v.h))
            L.VecSetSizes(v.h, n, n)
            vecs[name] = v
            continue
        host[name] = data((sizes or {}).get(name, n), j + 1)
        vecs[name] = P.Vec.from_array(host[name], comm=L.COMM_SELF)
    for name, src in (alias or {}).items():
        vecs[name] = vecs[src]
        if src in host:
            host[name] = host[src]
    return host, vecs


def refused(P, form, what, scalars=None, **kw):
    host, vecs = make(P, form, N, **kw)
    s = dict(form.scalars, **(scalars or {}))
    for name in host:
        vecs[name].norm()
    before = counts(P)
    rc, done, _ = form.call(P, {name: v.h for name, v in vecs.items()}, s)
    assert rc == 0 and done == 0, "%s, %s: return code %d, done %d" % (form.name, what, rc, done)
    for name, a in host.items():
        assert np.array_equal(bits(vecs[name].array()), bits(a)), "%s, %s: %s changed" % (form.name, what, name)
    assert counts(P) == before, "%s, %s: a shortcut was counted" % (form.name, what)


def accepted(env, form, n, what, scalars=None, absent=(), alias=None, readonly=None):
    """readonly: the operands this case must leave as they were (default: every operand the form never writes; named with an alias)"""
    dev, P = env
    host, vecs = make(P, form, n, absent=absent, alias=alias)
    s = dict(form.scalars, **(scalars or {}))
    uniq = {name: v for name, v in vecs.items() if not (alias and name in alias)}
    B = {name: dev.put(host[name]) for name in uniq}
    for name, src in (alias or {}).items():
        B[name] = B[src]
    for v in uniq.values():
        v.norm()                                             # the norm kept per object state is filled
    rc, done, sums = form.call(P, {name: v.h for name, v in vecs.items()}, s)
    assert rc == 0 and done == 1, "%s, %s: return code %d, done %d" % (form.name, what, rc, done)
    ksums = form.kernel(dev, n, B, s)
    dev.sync()
    if readonly is None:
        assert not alias
        readonly = [name for name in uniq if name not in form.written]
    for name, v in uniq.items():
        got = v.array()
        assert np.array_equal(bits(got), bits(dev.get(B[name], n))), "%s, %s: %s differs from the kernel's" % (form.name, what, name)
        if name in readonly:
            assert np.array_equal(bits(got), bits(host[name])), "%s, %s: %s is not written by this form and changed" % (form.name, what, name)
        fresh = P.Vec.from_array(got, comm=P.lib().COMM_SELF)
        assert bits(v.norm()) == bits(fresh.norm()), "%s, %s: norm of %s is not the norm of its entries" % (form.name, what, name)
    assert len(sums) == len(ksums), (form.name, what)
    for j, (a, b) in enumerate(zip(sums, ksums)):
        assert (a is None and b is None) or bits(a) == bits(b), "%s, %s: sum %d is %r, the kernel's %r" % (form.name, what, j, a, b)
    for p in set(q.value for q in B.values()):
        dev.free(C.c_void_p(p))
    return vecs, B


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("form", GATED, ids=IDS)
def test_refused_operands(env, form):
    _, P = env
    required = [name for name in form.ops if name not in form.optional]
    # the forms take every operand here; Chebyshev's sums and Jacobi diagonal need b, the flexible step needs d without `identity`
    for name in (form.ops[0], form.ops[-1], required[-1]):
        refused(P, form, "%s of local size 6" % name, sizes={name: 6})
    for w in form.written:
        for o in form.ops:
            if o == w or frozenset((o, w)) in form.permitted or (form.name.startswith("VecCGUpdate") and w in ("x", "r") and o in ("p", "w", "d")):
                continue
            refused(P, form, "%s given again as %s" % (w, o), alias={o: w})
    for name in required:
        if form.name.startswith(("VecPMult", "VecBCGS")):
            continue                                         # these two never promised to look at a missing operand: their callers hold all of them
        refused(P, form, "%s missing" % name, absent=(name,))
    refused(P, form, "%s without a type" % required[-1], untyped=required[-1])
    refused(P, form, "%s without a type" % form.ops[0], untyped=form.ops[0])


def test_refused_enums_and_counts(env):
    _, P = env
    for rides in (-1, 4):
        refused(P, PipeCGStep(), "rides %d" % rides, scalars=dict(rides=rides))
    for nhalves in (-1, 3):
        refused(P, TfqmrUpdate(), "nhalves %d" % nhalves, scalars=dict(nhalves=nhalves))
    for which in (-1, 2):
        refused(P, BicgUpdate(), "which %d" % which, scalars=dict(which=which))
    refused(P, BicgUpdate(), "d together with identity", scalars=dict(identity=1))
    for route in (-1, 3):
        refused(P, LsqrBidiag(), "route %d" % route, scalars=dict(route=route))
    for flexible in (False, True):
        for nv in (0, 33):
            refused(P, Orthog(flexible), "nv %d" % nv, scalars=dict(nv=nv))
    refused(P, Orthog(True), "neither d nor identity", absent=("d",))
    refused(P, Orthog(True), "a basis vector given again as d", alias={"d": "V1"})
    # Chebyshev without b: w is the preconditioned residual already and nothing else may be asked for
    refused(P, ChebyStep(), "d without b", absent=("b", "r"), scalars=dict(sums=0))
    refused(P, ChebyStep(), "r without b", absent=("b", "d"), scalars=dict(sums=0))
    refused(P, ChebyStep(), "sums without b", absent=("b", "d", "r"))
    refused(P, ChebyStep(), "pn given again as w, with b", alias={"w": "pn"})
    # forms that leave operands out still look at the ones they touch
    refused(P, MinresUpdate(), "first: vnew given again as r", scalars=dict(first=1), alias={"r": "vnew"})
    refused(P, TfqmrUpdate(), "no tail: d given again as q", scalars=dict(tail=0), alias={"q": "d"})
    refused(P, TfqmrUpdate(), "no halves: u missing", scalars=dict(nhalves=0), absent=("u",))
    refused(P, LsqrUpdate(), "skip_w: x given again as w", scalars=dict(skip_w=1), alias={"w": "x"})
    refused(P, LsqrUpdate(), "step 0 and w missing", scalars=dict(step=0.0), absent=("w",))


# ------------------------------------------------------------------------------------------------ acceptances
@pytest.mark.parametrize("n", SIZES)
def test_accepted_cg(env, n):
    accepted(env, CGUpdate(), n, "normal")
    accepted(env, CGUpdate(), n, "identity", absent=("d",))
    accepted(env, CGUpdate(), n, "z is w", alias={"w": "z"}, readonly=("p", "d"))
    for nox in (False, True):
        accepted(env, CGDev(nox), n, "normal")
        accepted(env, CGDev(nox), n, "identity", absent=("d",))
        accepted(env, CGDev(nox), n, "z is w", alias={"w": "z"}, readonly=("d",))
        for dpiold in (1.0, -1.0):                           # one of the two is refused on the device: x, r, z, p'w's sign as the kernel says
            accepted(env, CGDev(nox), n, "sign test, dpiold %r" % dpiold, scalars=dict(dpiold=dpiold, chk=1))
    _, P = env
    host, vecs = make(P, TDotBegin(), n)
    rc, ok, _ = TDotBegin().call(P, {k: v.h for k, v in vecs.items()}, {})
    assert rc == 0 and ok == 1
    _, zw = make(P, CGCheck(), n, alias={"w": "z"})
    rc, ok, _ = CGCheck().call(P, {k: v.h for k, v in zw.items()}, {})
    assert rc == 0 and ok == 1
    for name, a in host.items():
        assert np.array_equal(bits(vecs[name].array()), bits(a))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_bcgs(env, n):
    for two in (False, True):
        accepted(env, PMultDot(two), n, "normal")
        accepted(env, PMultDot(two), n, "identity", absent=("d",))
    accepted(env, BCGSUpdate(), n, "normal")


@pytest.mark.parametrize("n", SIZES)
def test_accepted_cheby_and_rich(env, n):
    accepted(env, ChebyStep(), n, "normal")
    accepted(env, ChebyStep(), n, "no sums, no r, no d", absent=("r", "d"), scalars=dict(sums=0))
    accepted(env, ChebyStep(), n, "r is w", alias={"r": "w"}, readonly=("b", "d", "pm", "pk"))
    accepted(env, ChebyStep(), n, "w alone", absent=("b", "d", "r"), scalars=dict(sums=0))
    accepted(env, ChebyStep(), n, "w alone, pn is w", absent=("b", "d", "r"), alias={"pn": "w"}, scalars=dict(sums=0), readonly=("pm", "pk"))
    accepted(env, RichStep(), n, "normal")
    accepted(env, RichStep(), n, "x alone", absent=("r", "z", "d"))
    accepted(env, RichStep(), n, "r is w", alias={"r": "w"}, readonly=("b", "d"))
    accepted(env, RichStep(), n, "scale 0", scalars=dict(scale=0.0))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_pipecg(env, n):
    accepted(env, PipeCGStep(), n, "normal")
    accepted(env, PipeCGStep(), n, "m_next is mv", alias={"m_next": "mv"}, readonly=("nv", "d"))
    accepted(env, PipeCGStep(), n, "identity, no m_next", absent=("d", "m_next"))
    accepted(env, PipeCGStep(), n, "first", scalars=dict(first=1))
    accepted(env, PipeCGStep(), n, "step 0", scalars=dict(step=0.0))
    for rides in (1, 2, 3):
        accepted(env, PipeCGStep(), n, "rides %d" % rides, scalars=dict(rides=rides))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_minres(env, n):
    accepted(env, MinresLanczos(), n, "normal")
    accepted(env, MinresLanczos(), n, "z as given", absent=("d",))
    accepted(env, MinresLanczos(), n, "alpha 0, beta 0", scalars=dict(alpha=0.0, beta=0.0))
    accepted(env, MinresUpdate(), n, "normal")
    accepted(env, MinresUpdate(), n, "first", scalars=dict(first=1), readonly=("x", "u", "w", "wold", "r", "z"))
    accepted(env, MinresUpdate(), n, "first, the rest missing", scalars=dict(first=1), absent=("x", "u", "w", "wold"))
    accepted(env, MinresUpdate(), n, "ceta 0", scalars=dict(ceta=0.0))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_tfqmr(env, n):
    for a in (0.41, 0.0):
        accepted(env, TfqmrQT(), n, "a %r" % a, scalars=dict(a=a), readonly=("u", "v") + (("x",) if a == 0.0 else ()))
        accepted(env, TfqmrQT(), n, "a %r, no x" % a, scalars=dict(a=a), absent=("x",))
        accepted(env, TfqmrResid(), n, "a %r" % a, scalars=dict(a=a), readonly=("auq", "rp") + (("r",) if a == 0.0 else ()))
    for nhalves in (0, 1, 2):
        for tail in (0, 1):
            keep = ["r"] + (["d", "x"] if nhalves == 0 else []) + (["p"] if not tail else []) + (["u", "q"] if not tail else [])
            accepted(env, TfqmrUpdate(), n, "nhalves %d tail %d" % (nhalves, tail), scalars=dict(nhalves=nhalves, tail=tail), readonly=keep)
    accepted(env, TfqmrUpdate(), n, "eta 0: x kept", scalars=dict(eta0=0.0, eta1=0.0), readonly=("r", "x"))
    accepted(env, TfqmrUpdate(), n, "one half, eta1 not looked at", scalars=dict(nhalves=1, eta0=0.0, tail=0), readonly=("r", "x", "u", "q", "p"))
    accepted(env, TfqmrUpdate(), n, "b 0: q kept", scalars=dict(b=0.0), readonly=("r", "q"))
    accepted(env, TfqmrUpdate(), n, "CGS: tail alone, d and x missing", scalars=dict(nhalves=0), absent=("d", "x"))
    accepted(env, TfqmrUpdate(), n, "one half alone, q, r, p missing", scalars=dict(nhalves=1, tail=0), absent=("q", "r", "p"))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_bicg(env, n):
    for first in (0, 1):
        for b in (0.55, 0.0):
            accepted(env, BicgDirs(), n, "first %d b %r" % (first, b), scalars=dict(first=first, b=b))
    for a in (0.33, 0.0):
        moved = () if a else ("x", "rr", "rl")
        for which in (0, 1):
            accepted(env, BicgUpdate(), n, "Jacobi a %r which %d" % (a, which), scalars=dict(a=a, which=which), readonly=("pr", "d") + moved)
            accepted(env, BicgUpdate(), n, "identity a %r which %d" % (a, which), scalars=dict(a=a, which=which, identity=1), absent=("d",), readonly=("pr",) + moved)
            accepted(env, BicgUpdate(), n, "general PC a %r which %d" % (a, which), scalars=dict(a=a, which=which), absent=("d",), readonly=("pr", "zr", "zl") + moved)


@pytest.mark.parametrize("n", SIZES)
def test_accepted_lsqr(env, n):
    dev, P = env
    accepted(env, LsqrBidiag(), n, "WAIT")
    accepted(env, LsqrBidiag(), n, "WAIT, coef 0", scalars=dict(coef=0.0))
    # QUEUE leaves its sum in a device slot; FINISH roots it for its own coefficient and brings both sums home
    slot = dev.put(np.zeros(2))
    accepted(env, LsqrBidiag(), n, "QUEUE", scalars=dict(route=QUEUE, slot=slot))
    accepted(env, LsqrBidiag(), n, "FINISH", scalars=dict(route=FINISH, slot=slot))
    dev.free(slot)
    accepted(env, LsqrUpdate(), n, "normal")
    accepted(env, LsqrUpdate(), n, "no se", absent=("se",))
    accepted(env, LsqrUpdate(), n, "ialpha 1: v1 kept", scalars=dict(ialpha=1.0), readonly=("v1",))
    accepted(env, LsqrUpdate(), n, "skip_w: w kept", scalars=dict(skip_w=1), readonly=("w",))
    accepted(env, LsqrUpdate(), n, "skip_w, ialpha 1, v1 missing", scalars=dict(skip_w=1, ialpha=1.0), absent=("v1",), readonly=("w",))
    accepted(env, LsqrUpdate(), n, "step 0: x kept", scalars=dict(step=0.0), readonly=("x",))
    accepted(env, LsqrUpdate(), n, "step 0, x missing", scalars=dict(step=0.0), absent=("x",))
    accepted(env, LsqrUpdate(), n, "skip_w, step 0, no se: v1 alone", scalars=dict(skip_w=1, step=0.0), absent=("x", "w", "se"))
    accepted(env, LsqrUpdate(), n, "nothing to do", scalars=dict(skip_w=1, step=0.0, ialpha=1.0), absent=("se",), readonly=("v1", "x", "w"))


@pytest.mark.parametrize("n", SIZES)
def test_accepted_gram_schmidt(env, n):
    for nv in (1, 3, 32):
        accepted(env, Orthog(False, nv), n, "nv %d" % nv)
    accepted(env, Orthog(True), n, "Jacobi")
    accepted(env, Orthog(True), n, "identity", absent=("d",), scalars=dict(identity=1))
    accepted(env, Orthog(True, 32), n, "32 vectors")


@pytest.mark.parametrize("n", SIZES)
def test_noted_maxpy_runs_inside_the_norm(env, n):
    """VecMAXPY then VecNorm: the update and the sum of squares in one sweep (the type's own shortcut, counted)"""
    dev, P = env
    L = P.lib()
    nv = 3
    hy, hx, coef = data(n, 1), [data(n, 2 + j) for j in range(nv)], np.array([0.3, -0.7, 1.1])
    y, xs = P.Vec.from_array(hy, comm=L.COMM_SELF), [P.Vec.from_array(a, comm=L.COMM_SELF) for a in hx]
    for v in [y] + xs:
        v.norm()
    before = counts(P)
    L.VecMAXPY(y.h, nv, coef.ctypes.data_as(vp), P.vec_table(xs))
    nrm = y.norm()
    after = counts(P)
    assert sum(after) == sum(before) + 1, (before, after)
    by, bx, bc, out = dev.put(hy), [dev.put(a) for a in hx], dev.put(coef), dev.put(np.zeros(2))
    dev.chk(dev.k.mi355x_vec_maxpy_dev_norm2(dev.h, n, nv, bc, 1.0, dev.ptr_table(bx), by, out))
    assert np.array_equal(bits(y.array()), bits(dev.get(by, n)))
    assert bits(nrm) == bits(np.sqrt(dev.get(out, 1)[0]))
    assert bits(y.norm()) == bits(P.Vec.from_array(y.array(), comm=L.COMM_SELF).norm())
    for a, v in zip(hx, xs):
        assert np.array_equal(bits(v.array()), bits(a))
    for p in [by, bc, out] + bx:
        dev.free(p)
