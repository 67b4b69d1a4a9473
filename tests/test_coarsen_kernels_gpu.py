"""The coarsening kernels of csrc/coarsen.hip through the C ABI against the model (tests/gamg_ref.py): the strength mask byte for byte,
the distance-2 MIS aggregation as integers.  Outputs live between guard bands of a marker; the inputs are read back."""
import ctypes as C

import numpy as np
import pytest

import gamg_ref as gr
from gpu import Dev
from test_gamg_cpu import SHAPES

pytestmark = pytest.mark.gpu
BAND = 64
INVALID = 1


@pytest.fixture(scope="module")
def dev(built):
    d = Dev()
    yield d
    d.free_all()


def device_strength(dev, ai, aj, aa, diag, theta, check_inputs=True):
    m, nz = len(ai) - 1, len(aj)
    host = [np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(aa, np.float64), np.ascontiguousarray(diag, np.float64)]
    d = [dev.put(a) for a in host]
    out = dev.put(np.full(nz + 2 * BAND, 0xA5, dtype=np.uint8))
    dev.chk(dev.k.mi355x_csr_strength(dev.h, m, d[0], d[1], d[2], d[3], float(theta), C.c_void_p(out.value + BAND)))
    got = dev.get(out, nz + 2 * BAND, np.uint8)
    assert np.all(got[:BAND] == 0xA5) and np.all(got[BAND + nz:] == 0xA5), "strong: written outside its nz bytes"
    for p, a in zip(d, host) if check_inputs else ():
        assert dev.get(p, a.size, a.dtype).tobytes() == a.tobytes()
    for p in d + [out]:
        dev.free(p)
    return got[BAND:BAND + nz].copy()


def device_mis2(dev, ai, aj, strong):
    m = len(ai) - 1
    host = [np.ascontiguousarray(ai, np.int32), np.ascontiguousarray(aj, np.int32), np.ascontiguousarray(strong, np.uint8)]
    d = [dev.put(a) for a in host]
    out = dev.put(np.full(m + 2 * BAND, -77, dtype=np.int32))
    n, rounds = C.c_int(-1), C.c_int(-1)
    dev.chk(dev.k.mi355x_coarsen_mis2(dev.h, m, d[0], d[1], d[2], C.c_void_p(out.value + 4 * BAND), C.byref(n), C.byref(rounds)))
    got = dev.get(out, m + 2 * BAND, np.int32)
    assert np.all(got[:BAND] == -77) and np.all(got[BAND + m:] == -77), "agg: written outside its m numbers"
    for p, a in zip(d, host):
        assert dev.get(p, a.size, a.dtype).tobytes() == a.tobytes()
    for p in d + [out]:
        dev.free(p)
    return got[BAND:BAND + m].copy(), n.value, rounds.value


def rows_of_lengths(lengths, seed):
    """one row per length, columns spread over the matrix, the diagonal among them when the length allows"""
    rng = np.random.default_rng(seed)
    m = len(lengths)
    rows = {}
    for i, n in enumerate(lengths):
        cols = set(int(c) for c in rng.choice(m, size=min(n, m), replace=False)) if n else set()
        if n and i not in cols:
            cols.pop(); cols.add(i)
        rows[i] = {c: float(rng.integers(-3, 4)) * 0.5 for c in cols}
    return gr.from_rows(m, rows)


def test_strength_equals_the_model_for_every_m_to_1000(dev):
    """the leading m x m blocks of one random pentadiagonal matrix, m = 1 .. 1000"""
    rng = np.random.default_rng(11)
    N = 1000
    I = np.repeat(np.arange(N), 5)
    J = I + np.tile(np.arange(-2, 3), N)
    V = rng.choice([1.0, -1.0, 0.5, 0.01, 0.0, -3.0], size=I.size)
    V[J == I] = rng.choice([4.0, 1.0, 0.25, 0.0], size=N, p=[0.5, 0.3, 0.15, 0.05])
    ok = (J >= 0) & (J < N)
    I, J, V = I[ok], J[ok], V[ok]
    dfull = V[J == I]
    ai, aj, aa = gr.from_rows(3, {0: {0: 4.0, 1: -1.0}, 1: {0: 0.01, 1: 1.0, 2: 0.5}, 2: {1: -3.0, 2: 0.0}})
    assert gr.strength_np(ai, aj, aa, 0.3, gr.diagonal(ai, aj, aa)).tobytes() == gr.strength(ai, aj, aa, 0.3).tobytes()
    for m in range(1, N + 1):
        keep = (I < m) & (J < m)
        ai = np.concatenate([[0], np.cumsum(np.bincount(I[keep], minlength=m))]).astype(np.int32)
        aj, aa, d = J[keep].astype(np.int32), V[keep], dfull[:m]
        got = device_strength(dev, ai, aj, aa, d, 0.3, check_inputs=(m % 100 == 0))
        assert got.tobytes() == gr.strength_np(ai, aj, aa, 0.3, d).tobytes(), m


def test_strength_over_row_lengths_0_to_257(dev):
    ai, aj, aa = rows_of_lengths(list(range(258)), 7)
    d = gr.diagonal(ai, aj, aa)
    d[::5] = 0.0
    for theta in (0.0, 0.6):
        assert device_strength(dev, ai, aj, aa, d, theta).tobytes() == gr.strength(ai, aj, aa, theta, d).tobytes(), theta


def test_strength_specials_by_position(dev):
    nan, inf = float("nan"), float("inf")
    vals = [nan, inf, -inf, 0.0, -0.0, 1e-300, -1e-300, 1.0, -2.0, 1e300]
    m = len(vals)
    rows = {i: {j: vals[(i * 3 + j) % m] for j in range(m)} for i in range(m)}          # every value against every diagonal pair
    for i in range(m):
        rows[i][i] = vals[i]
    ai, aj, aa = gr.from_rows(m, rows)
    d = gr.diagonal(ai, aj, aa)
    for theta in (0.0, 0.5, 1e300, inf, nan):
        with np.errstate(all="ignore"):
            want = gr.strength(ai, aj, aa, theta, d)
        assert device_strength(dev, ai, aj, aa, d, theta).tobytes() == want.tobytes(), theta


GRAPHS = SHAPES + [
    ("sym5000", gr.random_graph(5000, 3, 1, True), 0.0), ("asym4099", gr.random_graph(4099, 2, 2, False), 0.0),
    ("asym513_thresholded", gr.random_graph(513, 4, 3, False), 0.6), ("p2d_40", gr.poisson2d(40), 0.0)]


@pytest.fixture(scope="module")
def rounds_seen():
    return {}


@pytest.mark.parametrize("name,csr,theta", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_mis2_equals_the_greedy_model(dev, rounds_seen, name, csr, theta):
    ai, aj, aa = (np.asarray(v) for v in csr)
    strong = gr.strength(ai, aj, aa, theta)
    root, agg, nagg = gr.greedy_mis2(ai, aj, strong)
    got, n, rounds = device_mis2(dev, ai, aj, strong)
    assert n == nagg and np.array_equal(got, agg), name
    assert 1 <= rounds <= dev.k.mi355x_coarsen_round_cap()
    rounds_seen[name] = rounds
    gr.check_invariants(ai, aj, strong, root, got, n)
    again, n2, rounds2 = device_mis2(dev, ai, aj, strong)                # the maxima do not depend on the order they arrive in
    assert n2 == n and rounds2 == rounds and np.array_equal(again, got)


def test_some_graph_needs_several_rounds(rounds_seen):
    assert rounds_seen and max(rounds_seen.values()) >= 2, rounds_seen
    print(rounds_seen)


def test_nothing_to_do_and_bad_arguments(dev):
    n, rounds = C.c_int(5), C.c_int(5)
    assert dev.k.mi355x_coarsen_mis2(dev.h, 0, None, None, None, None, C.byref(n), C.byref(rounds)) == 0 and (n.value, rounds.value) == (0, 0)
    assert dev.k.mi355x_csr_strength(dev.h, 0, None, None, None, None, 0.0, None) == 0
    ai, aj, aa = gr.path(4)
    d = [dev.put(a) for a in (np.array(ai, np.int32), np.array(aj, np.int32), np.array(aa, np.float64))]
    s = dev.put(np.zeros(len(aj), np.uint8)); agg = dev.put(np.zeros(4, np.int32))
    assert dev.k.mi355x_coarsen_mis2(dev.h, -1, d[0], d[1], s, agg, C.byref(n), C.byref(rounds)) == INVALID
    assert dev.k.mi355x_coarsen_mis2(dev.h, 4, None, d[1], s, agg, C.byref(n), C.byref(rounds)) == INVALID
    assert dev.k.mi355x_coarsen_mis2(dev.h, 4, d[0], d[1], None, agg, C.byref(n), C.byref(rounds)) == INVALID
    assert dev.k.mi355x_coarsen_mis2(dev.h, 4, d[0], d[1], s, None, C.byref(n), C.byref(rounds)) == INVALID
    assert dev.k.mi355x_coarsen_mis2(dev.h, 4, d[0], d[1], s, agg, None, C.byref(rounds)) == INVALID
    assert dev.k.mi355x_csr_strength(dev.h, -1, d[0], d[1], d[2], d[2], 0.0, s) == INVALID
    assert dev.k.mi355x_csr_strength(dev.h, 4, d[0], d[1], d[2], None, 0.0, s) == INVALID
    assert dev.k.mi355x_csr_strength(dev.h, 4, d[0], d[1], d[2], d[2], 0.0, None) == INVALID
    dev.sync()
    for p in d + [s, agg]:
        dev.free(p)
