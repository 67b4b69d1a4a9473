"""Random re-set-up programs (tests/pcprog.py) on the device against the host model.  Every program runs on ONE long-lived KSP and PC
per pool operator, so a program meets whatever the programs before it left in the factored matrix.  Every application is compared
with the model: bit for bit in column order, at the level launches and with enough sweeps, else within DESIGN 7's 1e-13 relative.
After every set-up the getters are compared with the model's prediction, and the same right-hand side goes through a twin -- a fresh
KSP and PC on a fresh matrix of the model's pattern and values under the options in force -- which the long-lived PC equals bit for
bit in every mode.  PCICC runs its own programs (host/icc.c takes no option) against orc.icc0_factor / icc0_solve, PCICCGetInfo and a
twin.  A failing program is reported with its shortest failing prefix, run once more on a fresh PC."""
import ctypes as C
import time

import pytest

import pcprog as pp

pytestmark = pytest.mark.gpu
CHUNK = 8
ALL = pp.SEEDS + pp.ICC_SEEDS
CHUNKS = [ALL[k:k + CHUNK] for k in range(0, len(ALL), CHUNK)]
_EXEC, _DONE = {}, {}


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


def run_chunk(P, k):
    """the programs of a chunk, each on the long-lived executor of its operator; kept, so that the last test runs nothing twice"""
    if k not in _DONE:
        t0, out = time.perf_counter(), []
        for i in CHUNKS[k]:
            prog = pp.generate(i) if i < pp.ICC_BASE else pp.generate_icc(i)
            before = list(_EXEC[prog["operator"]].ran) if prog["operator"] in _EXEC else []
            if prog["operator"] not in _EXEC:
                _EXEC[prog["operator"]] = pp.Executor(P, prog["operator"])
            out.append((prog, _EXEC[prog["operator"]].run(prog), before))
        print("chunk %d: %d programs, %d calls, %.2f s" % (k, len(out), sum(len(p["calls"]) for p, _, _ in out), time.perf_counter() - t0))
        _DONE[k] = out
    return _DONE[k]


@pytest.mark.parametrize("k", range(len(CHUNKS)))
def test_programs_agree_with_the_model_and_with_a_fresh_twin(P, k):
    for prog, failure, before in run_chunk(P, k):
        if failure is not None:
            pytest.fail(pp.explain(P, prog, failure, before), pytrace=False)


def test_every_form_is_reached_over_the_whole_list(P):
    for k in range(len(CHUNKS)):
        run_chunk(P, k)
    total = {key: sum(ex.counts[key] for ex in _EXEC.values()) for key in ("programs", "calls", "setups", "bits", "bound")}
    print("over the list: %s" % total)
    assert set(_EXEC) == set(pp.OPERATORS + pp.ICC_OPERATORS) and total["programs"] == len(ALL)
    for name, ex in _EXEC.items():
        print("%s: set-ups that reached each form: %s" % (name, ex.reached))
        assert ex.reached["syncfree"] > 0 or ex.icc, name
    for key in ("sweeps", "on_device", "nodes", "nshift"):
        assert sum(ex.reached[key] for ex in _EXEC.values()) > 0, key
    assert total["bound"] * 4 <= total["bits"] + total["bound"]


def test_icc_with_levels_stays_refused(P):
    """ICC keeps to zero fill: -pc_factor_levels 1 is refused at set-up, on an operator of the pool, and levels 0 sets up"""
    L = P.lib()
    A = P.Mat.from_csr(*pp.operator("lap2d")["A"])
    for levels, ok in ((1, False), (0, True)):
        pc = C.c_void_p()
        k = P.KSP(comm=L.COMM_SELF); k.set_operators(A); L.KSPGetPC(k.h, C.byref(pc)); L.PCSetType(pc, b"icc")
        L.PetscOptionsClear(); L.PetscOptionsInsertString(("-pc_factor_levels %d" % levels).encode())
        rc = L.raw("PCSetFromOptions")(pc) or L.raw("PCSetUp")(pc)
        L.PetscOptionsClear()
        assert (rc == 0) == ok and (ok or rc == 56), (levels, rc)
