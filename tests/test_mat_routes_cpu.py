"""The route options of the sequential AIJ type without a GPU: -mat_hipmi355x_sor, _product, _reductions, _coarsen <device|host> and
-mat_hipmi355x_residual <fused|calls>.  What is pinned: the one error of a word that is neither of the two (code, text, nothing
changed), the matrix's prefix before the global database, when each option reads the global database ("Route options"),
what the result of a product takes over from its operand, and the answer of the query entry points to a NULL handle.

Host routes only, so every case also holds on a machine with a device; matrices of 12 rows."""
import ctypes as C

import numpy as np
import pytest

ARG_WRONG = 62
WORDS = {"sor": ("device", "host"), "product": ("device", "host"), "reductions": ("device", "host"), "residual": ("fused", "calls"),
         "coarsen": ("device", "host")}
HOST_OPS = ["sor", "product", "reductions", "coarsen"]          # the routes that can be taken without a device
KEPT = {"sor": True, "product": False, "reductions": True, "coarsen": False}   # the global answer of the first use stays with the matrix
N = 12


@pytest.fixture(scope="module")
def P(built):
    from petsc_dev_amd import petsc as P
    P.lib()
    return P


@pytest.fixture()
def L(P):
    lib = P.lib()
    lib.PetscOptionsClear()
    yield lib
    lib.PetscOptionsClear()


def tridiag():
    rows = [[c for c in (r - 1, r, r + 1) if 0 <= c < N] for r in range(N)]
    ai = np.concatenate([[0], np.cumsum([len(q) for q in rows])]).astype(np.int32)
    aj = np.concatenate(rows).astype(np.int32)
    aa = np.array([2.5 + 0.125 * r if c == r else -1.0 - 0.0625 * c for r in range(N) for c in rows[r]])
    return ai, aj, aa


def tall():
    """12 x 7: row r has entries in columns r // 2 and (r // 2 + 1) % 7"""
    cols = [sorted({r // 2, (r // 2 + 1) % 7}) for r in range(N)]
    ai = np.concatenate([[0], np.cumsum([len(q) for q in cols])]).astype(np.int32)
    aj = np.concatenate(cols).astype(np.int32)
    return ai, aj, 1.0 + 0.25 * np.arange(aj.size)


def matrix(P, L, prefix=None):
    A = P.Mat.from_csr(*tridiag())
    if prefix:
        L.MatSetOptionsPrefix(A.h, prefix.encode())
    return A


def opt(name, prefix=""):
    return ("-%smat_hipmi355x_%s" % (prefix, name)).encode()


def use(P, L, name, A):
    """one operation that asks for the route `name` of A; what it returns tells the host route by its counter"""
    if name == "sor":
        b = P.Vec.from_array(np.ones(N), comm=L.COMM_SELF)
        x = P.Vec.from_array(np.full(N, 0.5), comm=L.COMM_SELF)
        A.sor(b, x)
        assert not np.array_equal(x.array(), np.full(N, 0.5))
        return A.sor_info()[4] == 0                                  # no application on the device
    if name == "product":
        B = P.Mat.from_csr(*tall(), ncols=7)
        Cm = A.matmult(B)
        return Cm.product_counts()[1:] == (0, 1)                     # one host numeric phase
    if name == "reductions":
        ai, aj, aa = A.csr()
        assert A.norm(P.NORM_INFINITY) == max(np.abs(aa[ai[r]:ai[r + 1]]).sum() for r in range(N))
        return True                                                  # (the two routes give the same bits: no counter)
    before = A.coarsen_counts()
    agg, nagg = A.aggregate()
    assert nagg >= 1 and agg.min() == 0 and agg.max() == nagg - 1
    after = A.coarsen_counts()
    return after[0] == before[0] and after[1] == before[1] + 1       # one more coarsening on the host


def raises62(P, call):
    with pytest.raises(P.PetscError) as e:
        call()
    assert e.value.code == ARG_WRONG, str(e.value)
    return str(e.value)


def same_csr(x, y):
    return all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y))


# ---------------------------------------------------------------------------------------------------- the one parser
@pytest.mark.parametrize("name", HOST_OPS)
def test_bad_word_in_the_global_database(P, L, name):
    A = matrix(P, L)
    before = A.csr()
    L.PetscOptionsSetValue(opt(name), b"sideways")
    text = raises62(P, lambda: use(P, L, name, A))
    a, b = WORDS[name]
    assert "-mat_hipmi355x_%s <%s|%s>, got sideways" % (name, a, b) in text
    assert same_csr(before, A.csr())


@pytest.mark.parametrize("name", list(WORDS))
def test_bad_word_under_the_prefix(P, L, name):
    A, B = matrix(P, L, "p_"), matrix(P, L, "q_")
    before = A.csr()
    L.PetscOptionsSetValue(opt(name, "p_"), b"sideways")
    text = raises62(P, lambda: L.MatSetFromOptions(A.h))
    a, b = WORDS[name]
    assert "-mat_hipmi355x_%s <%s|%s>, got sideways" % (name, a, b) in text
    assert same_csr(before, A.csr())
    L.MatSetFromOptions(B.h)                                          # another prefix: not this matrix's option
    if name in HOST_OPS:
        L.PetscOptionsSetValue(opt(name, "q_"), WORDS[name][1].encode())
        L.MatSetFromOptions(B.h)
        assert use(P, L, name, B)


@pytest.mark.parametrize("name", list(WORDS))
def test_both_words_are_taken_under_the_prefix(P, L, name):
    A = matrix(P, L, "p_")
    for word in WORDS[name]:
        L.PetscOptionsSetValue(opt(name, "p_"), word.encode())
        L.MatSetFromOptions(A.h)


# ---------------------------------------------------------------------------------------------------- prefix, then global
@pytest.mark.parametrize("name", HOST_OPS)
def test_prefix_beats_global(P, L, name):
    A = matrix(P, L, "p_")
    L.PetscOptionsSetValue(opt(name), b"device")
    L.PetscOptionsSetValue(opt(name, "p_"), b"host")
    L.MatSetFromOptions(A.h)
    assert use(P, L, name, A)
    assert use(P, L, name, A)


@pytest.mark.parametrize("name", HOST_OPS)
def test_when_the_global_database_is_read(P, L, name):
    A = matrix(P, L, "p_")
    L.PetscOptionsSetValue(opt(name), b"host")
    assert use(P, L, name, A)
    L.PetscOptionsSetValue(opt(name), b"sideways")
    if KEPT[name]:                                                    # once per matrix: the first use's answer stays
        assert use(P, L, name, A)
    else:                                                             # every use
        raises62(P, lambda: use(P, L, name, A))
    raises62(P, lambda: use(P, L, name, matrix(P, L)))                # a new matrix asks the database
    L.PetscOptionsSetValue(opt(name, "p_"), b"host")                  # asked under its prefix: the global entry no longer matters
    L.MatSetFromOptions(A.h)
    assert use(P, L, name, A)
    B = matrix(P, L, "q_")
    L.PetscOptionsSetValue(opt(name, "q_"), b"host")
    L.MatSetFromOptions(B.h)
    assert use(P, L, name, B)


# ---------------------------------------------------------------------------------------------------- product results
def test_a_product_result_takes_over_product_sor_and_coarsen(P, L):
    A = matrix(P, L, "p_")
    for name in ("product", "sor", "coarsen"):
        L.PetscOptionsSetValue(opt(name, "p_"), b"host")
    L.MatSetFromOptions(A.h)
    Cm = A.matmult(A)
    assert Cm.product_counts() == (1, 0, 1)
    L.PetscOptionsClear()
    # the device route is these options' default: a result that had not taken the operand's answers over would take it
    for name in ("product", "sor", "coarsen"):
        L.PetscOptionsSetValue(opt(name), b"device")
    assert use(P, L, "product", Cm) and use(P, L, "sor", Cm) and use(P, L, "coarsen", Cm)
    # -mat_hipmi355x_reductions is not handed on: the result asks the database like a new matrix
    L.PetscOptionsSetValue(opt("reductions"), b"sideways")
    raises62(P, lambda: use(P, L, "reductions", Cm))
    L.PetscOptionsSetValue(opt("reductions"), b"host")
    assert use(P, L, "reductions", Cm)


def test_a_product_result_does_not_take_over_reductions(P, L):
    A = matrix(P, L, "p_")
    L.PetscOptionsSetValue(opt("product", "p_"), b"host")
    L.PetscOptionsSetValue(opt("reductions", "p_"), b"host")
    L.MatSetFromOptions(A.h)
    Cm = A.matmult(A)
    L.PetscOptionsSetValue(opt("reductions"), b"sideways")
    assert use(P, L, "reductions", A)
    raises62(P, lambda: use(P, L, "reductions", Cm))


# ---------------------------------------------------------------------------------------------------- the type guard
ERRORING_QUERIES = {   # entry point -> number of result pointers; each answers 62 to a matrix that is not a sequential one of this type
    "MatHIPMI355XGetUploadCount": 1, "MatHIPMI355XGetBlockedInfo": 2, "MatHIPMI355XGetTransposeCounts": 2,
    "MatHIPMI355XGetResidualCounts": 2, "MatHIPMI355XGetZeroRowsCounts": 2, "MatHIPMI355XGetSORInfo": 5,
    "MatHIPMI355XGetProductCounts": 3, "MatHIPMI355XGetTiming": 2}


@pytest.mark.parametrize("entry", sorted(ERRORING_QUERIES))
def test_null_handle(P, L, entry):
    """(MatHIPMI355XGetCoarsenCounts is not here: its NULL handle asks for the totals of the process)"""
    out = [C.c_double() if entry == "MatHIPMI355XGetTiming" and k == 1 else C.c_int() for k in range(ERRORING_QUERIES[entry])]
    raises62(P, lambda: getattr(L, entry)(None, *[C.byref(q) for q in out]))


def test_queries_of_a_matrix_without_a_device_copy(P, L):
    A = matrix(P, L)
    n = C.c_int(-1)
    L.MatHIPMI355XGetUploadCount(A.h, C.byref(n))
    assert n.value == 0
    bs, nb = C.c_int(-1), C.c_int(-1)
    L.MatHIPMI355XGetBlockedInfo(A.h, C.byref(bs), C.byref(nb))
    assert (bs.value, nb.value) == (0, 0)
    b, r = C.c_int(-1), C.c_int(-1)
    L.MatHIPMI355XGetTransposeCounts(A.h, C.byref(b), C.byref(r))
    assert (b.value, r.value) == (0, 0)
    assert A.residual_counts() == (0, 0) and A.coarsen_counts() == (0, 0, 0) and A.sor_info() == (0, 0, 0, 0, 0)
    raises62(P, lambda: A.product_counts())                           # not the result of a product
    assert P.Mat.coarsen_counts_total()[2] >= 0
