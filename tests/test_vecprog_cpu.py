"""The coverage contract of the random call programs (tests/vecprog.py), checked from the programs alone, and the model against
the obvious NumPy formulas.  No GPU."""
import numpy as np
import pytest

import orc
import vecprog as vp


@pytest.fixture(scope="module")
def programs(built):
    return [vp.generate(i) for i in vp.SEEDS]


def test_same_seed_same_program(programs):
    for i in (0, 17, 101, len(vp.SEEDS) - 1):
        again = vp.generate(i)
        assert again["calls"] == programs[i]["calls"] and again["shape"] == programs[i]["shape"]
    r = vp.generate(5, ranks=True)
    assert r["calls"] == vp.generate(5, ranks=True)["calls"]


def test_size_and_values(programs):
    """at most 40 calls; every program ends everything it opened; values stay finite and tame; n = 1 has its pool"""
    assert {p["shape"] for p in programs} == {"lap2d", "nonsym300", "n1"}
    for p in programs:
        assert len(p["calls"]) <= vp.MAXCALLS
        assert vp.closing_calls(p["calls"]) == []
        out, vecs, m = vp.reference(p)
        assert m.tame() and np.all(np.isfinite(out)), p["index"]
        assert not m.open and not m.lent and not m.placed and not m.sr


def test_model_against_numpy_formulas(built):
    """every call kind once, on the small pool: the model's update is the plain formula to rounding"""
    pl = vp.pool("nonsym300", 3)
    n, ai, aj = pl["n"], pl["ai"], pl["aj"]
    close = lambda a, b: np.allclose(a, b, rtol=1e-12, atol=1e-12)
    v = [a.copy() for a in pl["vecs"]]

    def after(*calls):
        m = vp.Model(pl)
        for c in calls:
            m.apply(c)
        return m
    assert close(after(("set", 0, 1.5)).V[0], 1.5) and close(after(("copy", 1, 0)).V[0], v[1])
    m = after(("swap", 0, 1)); assert close(m.V[0], v[1]) and close(m.V[1], v[0])
    assert close(after(("scale", 0, -0.7)).V[0], -0.7 * v[0])
    assert close(after(("axpy", 0, 0.37, 1)).V[0], v[0] + 0.37 * v[1]) and close(after(("aypx", 0, 0.37, 1)).V[0], 0.37 * v[0] + v[1])
    assert close(after(("axpby", 0, 0.37, -1.7, 1)).V[0], 0.37 * v[1] - 1.7 * v[0])
    assert close(after(("waxpy", 0, 0.37, 1, 2)).V[0], 0.37 * v[1] + v[2])
    assert close(after(("axpbypcz", 0, 0.37, -1.7, 2.0, 1, 2)).V[0], 0.37 * v[1] - 1.7 * v[2] + 2.0 * v[0])
    assert close(after(("maxpy", 0, (0.37, -1.7, 0.5), (1, 2, 1))).V[0], v[0] + 0.87 * v[1] - 1.7 * v[2])
    assert close(after(("pmult", 0, 1, 2)).V[0], v[1] * v[2]) and close(after(("pdiv", 0, 1, 2)).V[0], v[1] / v[2])
    assert close(after(("recip", 0)).V[0], 1.0 / v[0])
    m = after(("dot", 0, 1), ("tdot", 1, 2), ("mdot", 0, (1, 2)), ("dotnorm2", 0, 1), ("norm", 0, 0), ("norm", 0, 1), ("norm", 0, 3), ("norm", 0, 4), ("normalize", 0),
              ("dotbegin", 0, 1), ("normbegin", 2), ("srbegin",), ("dotend", 0, 1), ("normend", 2), ("getarrayread", 3))
    nrm = np.linalg.norm(v[0])
    assert close(m.out, [v[0] @ v[1], v[1] @ v[2], v[0] @ v[1], v[0] @ v[2], v[0] @ v[1], v[1] @ v[1], np.abs(v[0]).sum(), nrm, np.abs(v[0]).max(),
                         np.abs(v[0]).sum(), nrm, nrm, (v[0] / nrm) @ v[1], np.linalg.norm(v[2]), v[3][0], v[3][-1]])
    assert close(m.V[0], v[0] / nrm)
    # the norms the wrappers keep: a constant vector's, carried by a copy and a scaling, dropped by any other write
    m = after(("set", 0, -2.0), ("copy", 0, 1), ("scale", 1, 0.5), ("norm", 1, 1), ("norm", 1, 0), ("axpy", 1, 0.0, 2), ("norm", 1, 1))
    assert m.out[0] == 0.5 * (np.sqrt(float(n)) * 2.0) and m.out[1] == 0.5 * (n * 2.0) and close(m.out[2], np.sqrt(n)) and m.norms[1] == {1: m.out[2]}
    # storage
    m = after(("getarray", 0), ("axpy", 1, 1.0, 2), ("restorearray", 0, 4))
    e = v[0].copy(); e[1::3] = e[1::3] * 0.5 + 0.5
    assert close(m.V[0], e) and not m.open
    m = after(("setvalues", 0, (3, 7), (1.0, -2.0), vp.INSERT), ("setvalues", 1, (3, 7), (1.0, -2.0), vp.ADD))
    assert m.V[0][3] == 1.0 and m.V[0][7] == -2.0 and close(m.V[1][[3, 7]], v[1][[3, 7]] + [1.0, -2.0])
    m = after(("placearray", 0, 2), ("scale", 0, 2.0)); assert close(m.V[0], 2.0 * vp.buffer(2, n))
    assert close(after(("placearray", 0, 2), ("scale", 0, 2.0), ("resetarray", 0)).V[0], v[0])
    assert close(after(("replacearray", 0, 5)).V[0], vp.buffer(5, n)) and close(after(("recreate", 0, 1)).V[0], 0.0)
    m = after(("sharebegin", 8, 0, 11, 1), ("set", 8, 3.0), ("norm", 8, 3), ("shareend", 8))
    e = v[0].copy(); e[11:11 + pl["m"]] = 3.0
    assert close(m.V[0], e) and close(m.V[8], v[8]) and m.out == [3.0] and not m.lent
    # products and matrix values
    A, B = _dense(ai, aj, pl["aa"], n), _dense(ai, aj, pl["bb"], n)
    assert close(after(("matmult", "A", 1, 0)).V[0], A @ v[1]) and close(after(("matmultadd", "B", 1, 2, 0)).V[0], B @ v[1] + v[2])
    assert close(after(("matmulttranspose", "A", 1, 0)).V[0], A.T @ v[1])
    D = lambda m_, name="A": _dense(ai, aj, m_.M[name], n)
    assert close(D(after(("matscale", "A", 0.5))), 0.5 * A) and close(D(after(("matshift", "A", 2.0))), A + 2.0 * np.eye(n))
    assert close(D(after(("matdiagscale", "A", 1, 2))), v[1][:, None] * A * v[2][None, :]) and close(D(after(("matdiagscale", "A", None, 2))), A * v[2][None, :])
    assert close(D(after(("mataxpy", "A", -0.75, "B"))), A - 0.75 * B) and close(D(after(("matcopy", "A", "B")), "B"), A)
    assert close(D(after(("matzeroentries", "A"))), 0.0)
    rows = (2, 40, 41)
    Z = A.copy(); Z[list(rows), :] = 0.0; Z[list(rows), list(rows)] = 2.0
    m = after(("matzerorows", "A", rows, 2.0, 1, 0))
    e = v[0].copy(); e[list(rows)] = 2.0 * v[1][list(rows)]
    assert close(D(m), Z) and close(m.V[0], e)
    m = after(("matzerorowscols", "A", rows, 2.0, 1, 0))
    xz = np.zeros(n); xz[list(rows)] = v[1][list(rows)]
    e = v[0] - A @ xz; e[list(rows)] = 2.0 * v[1][list(rows)]
    Z[:, list(rows)] = 0.0; Z[list(rows), list(rows)] = 2.0
    assert close(D(m), Z) and close(m.V[0], e)
    L_, U_, d = np.tril(A, -1), np.triu(A, 1), np.diag(A)
    x = np.linalg.solve(L_ + np.diag(d), v[1] - U_ @ v[0])              # forward, then backward Gauss-Seidel
    x = np.linalg.solve(U_ + np.diag(d), v[1] - L_ @ x)
    assert close(after(("matsor", "A", 1, 0)).V[0], x)


def _dense(ai, aj, aa, n):
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(ai)), aj] = aa
    return A


def test_every_call_kind_appears(programs):
    seen = {c[0] for p in programs for c in p["calls"]}
    assert seen == set(vp.KINDS)
    nv = {len(c[3]) for p in programs for c in p["calls"] if c[0] == "maxpy"}
    assert nv == {1, 2, 3, 4, 5, 6}
    assert {c[2] for p in programs for c in p["calls"] if c[0] == "norm"} == {0, 1, 3, 4}
    assert {c[4] for p in programs for c in p["calls"] if c[0] == "sharebegin"} == {0, 1} and any(c[3] % 2 for p in programs for c in p["calls"] if c[0] == "sharebegin")
    scal = {repr(a) for p in programs for c in p["calls"] if c[0] in ("set", "scale", "axpy", "aypx") for a in c[2:3]}
    assert {"0.0", "-0.0", "1.0", "-1.0"} <= scal


def test_every_motif_whole_and_cut_at_every_position_by_every_class(programs):
    seen = set()
    for p in programs:
        marks = p["marks"]
        assert len(marks) == vp.MOTIF_LEN[p["motif"]]
        if p["cut"] is None:
            assert marks == list(range(marks[0], marks[0] + len(marks))), p["index"]
            seen.add((p["motif"], None, None))
            continue
        for i in range(1, len(marks)):
            between = p["calls"][marks[i - 1] + 1:marks[i]]
            if i != p["cut"]:
                assert not between, p["index"]
            else:
                assert any(vp.CLASS[c[0]] == p["cls"] for c in between), (p["index"], between)
                seen.add((p["motif"], i, p["cls"]))
    want = {(m, None, None) for m in vp.MOTIFS} | {(m, i, cls) for m in vp.MOTIFS for i in range(1, vp.MOTIF_LEN[m]) for cls in vp.CUT_CLASSES}
    assert seen == want


def test_matrix_value_operations_meet_a_product_and_storage_calls_meet_a_note(programs):
    """by the model's own bookkeeping of what would be pending: every matrix value operation is called on a matrix whose product
    is noted (between the MatMult and the first reader of its result) and on one whose work vector is still unwritten; every storage
    call -- and a destroy, and each phase of a split reduction -- is called while something is pending"""
    noted, unwritten, met = set(), set(), set()
    for p in programs:
        for c, (dq, pp, pl) in zip(p["calls"], vp.pending_trace(p)):
            k = c[0]
            if vp.CLASS[k] == "matvalue":
                M = c[2] if k == "matcopy" else c[1]
                tag = k + ("_b" if k.startswith("matzerorows") and c[5] is not None else "")
                if pp and pp[0] == M: noted.add(tag)
                if pl and pl[0] == M: unwritten.add(tag)
            if (dq or pp or pl) and vp.CLASS[k] in ("storage", "destroy", "split"):
                met.add(k + ("%d" % c[4] if k in ("setvalues", "sharebegin") else ""))
    ops = {"matscale", "matdiagscale", "matshift", "matzeroentries", "mataxpy", "matcopy", "matzerorows", "matzerorows_b", "matzerorowscols", "matzerorowscols_b", "matsor"}
    assert noted >= ops, ops - noted
    assert unwritten >= ops, ops - unwritten
    want = {"getarray", "restorearray", "getarrayread", "setvalues1", "setvalues2", "placearray", "resetarray", "replacearray", "sharebegin0", "sharebegin1", "shareend",
            "recreate", "dotbegin", "normbegin", "srbegin", "dotend", "normend"}
    assert met >= want, want - met


def test_the_programs_for_two_ranks_keep_to_vectors_and_matmult():
    assert len(vp.RANK_SEEDS) >= 20
    for i in vp.RANK_SEEDS:
        p = vp.generate(i, ranks=True)
        for c in p["calls"]:
            assert vp.CLASS[c[0]] != "matvalue" and c[0] not in ("sharebegin", "shareend", "normalize", "matmultadd", "matmulttranspose"), (i, c)
            assert all(v < vp.NV for v in sum(vp.operands(c), ()))
