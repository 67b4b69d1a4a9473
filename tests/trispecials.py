"""Host-side machinery of the triangular-solve containment / IEEE-special / re-arming tests (test_tri_specials_gpu.py), checked on
its own by test_tri_specials_cpu.py; pure numpy + the oracle, nothing here touches the GPU.

The sync-free kernels of csrc/trisolve.hip tell a solution value from "not computed yet" by its bit pattern (TRI_SENTINEL, a NaN
with a payload), gather list entries behind guards (q0 + j < ncol, live(j), row >= 0, k < nsz), pad lists with entries that name
slot 0 of the solution with value 0.0 and clamp indices to entry 0 of a list.  With finite data a guard that is off by one forms
0.0 * w[slot 0] and changes no bit; with NaN / +-Inf in the right-hand side it changes the class of a row.  What is here:
  Part A  the rows a set S of poisoned right-hand-side entries can reach through L's, then U's dependency graph; S chosen so
          that the rows the padding entries, clamps and slice edges name are poisoned in some round (targets);
  Part B  hand-built factors of IEEE special cases with the class of every row stated;
  Part C  the right-hand sides of a sequence of applications on one plan pair (nothing stale).
Factors are the dicts of tri.tri_factor (row plans) and, with `nstart`, of node_factor (node plans: one cj / cv for both halves)."""
import functools

import numpy as np

import orc
import tri
from specials import FIN, MAX_ROUNDS, NAN, NINF, PINF, SPECIALS, bits, classify  # noqa: F401 (re-exported to the two test modules)
from vecspecials import DBL_MIN, MID_SUB, MIN_SUB, differing, same  # noqa: F401

W = 64                                  # MI355X_WAVE: positions of a slice
ALIGN_MIN = 32                          # TRI_ALIGN_MIN: node plans start a level of this many items on a slice boundary
# the split-role kernels' LDS (csrc/trisolve.hip, TriSplitGeom<NB> and TRI_SPLIT_LDS_BYTES): columns per batch of single-row plans, and
# how many batches the ring holds at most: (LDS - 64 - 2 headers) / stage
SPLIT_LDS_BYTES = 150 * 1024            # TRI_SPLIT_LDS_BYTES
SPLIT_B1 = 8                            # TRI_SPLIT_B1


def split_ring_batches(nb, cols=SPLIT_B1):
    nd = nb * (nb - 1) // 2 + nb
    header = 64 + 3 * 256 + (nb + nd) * 512          # TriSplitGeom::HB
    stage = cols * 256 + cols * nb * 512             # TriSplitGeom::SB
    return (SPLIT_LDS_BYTES - 64 - 2 * header) // stage


SENTINEL = 0xFFF8DEADBEEFCAFE           # TRI_SENTINEL: no test feeds it or a NaN with its payload
PAYLOAD = 0xDEADBEEFCAFE
ROUNDS = 3                              # rounds per case at least; more while a target is still open (MAX_ROUNDS)
MIN_REACH, MIN_REST = 0.05, 0.25        # the conditions of Part A on the shares of reachable / untouched rows
A_SHAPES = ["wide", "ragged", "chain", "empty_rows", "n64", "n65", "longrow", "tiny", "n1"]
CONFIGS = ["L", "U", "both"]
NODE_FACTORS = ["mixed", "fixed3"]


def is_nodes(f):
    return "nstart" in f


def reference(f, b):
    with np.errstate(all="ignore"):
        return tri.tri_node_reference_apply(f, b) if is_nodes(f) and f["nstart"].size - 1 < f["n"] else tri.tri_reference_apply(f, b)


def numpy_reference(f, b):
    """the same two sweeps restated with numpy float64 scalars and an explicit product / sum / difference per step (no Python
    float arithmetic): the check of the references before they are used on specials"""
    n = f["n"]
    ns = f["nstart"] if is_nodes(f) else np.arange(n + 1)
    pair = is_nodes(f) and ns.size - 1 < n
    mul, add, sub = np.multiply, np.add, np.subtract
    with np.errstate(all="ignore"):
        def sweep(rp, rl, cj, cv, src, upper):
            x = np.zeros(n)
            for u in (range(ns.size - 2, -1, -1) if upper else range(ns.size - 1)):
                r0, rL = int(ns[u]), int(ns[u + 1]) - 1
                lead = rL if upper else r0
                sh, p0 = int(rl[lead]), int(rp[lead])
                for k in range(rL - r0 + 1):
                    r = rL - k if upper else r0 + k
                    p = int(rp[r]) + (k if upper else 0)
                    s = src[r]
                    j = 0
                    while pair and j < sh - 1:
                        s = sub(s, add(mul(cv[p + j], x[cj[p0 + j]]), mul(cv[p + j + 1], x[cj[p0 + j + 1]])))
                        j += 2
                    while j < sh:
                        s = sub(s, mul(cv[p + j], x[cj[p0 + j]]))
                        j += 1
                    for l in range(k):
                        s = sub(s, mul(cv[p - 1 - l], x[rL - l])) if upper else sub(s, mul(cv[p + sh + l], x[r0 + l]))
                    x[r] = mul(s, f["dinv"][r]) if upper else s
            return x
        z = sweep(f["rp"], f["rl"], f["cj"], f["cv"], np.asarray(b, dtype=np.float64), False)
        if f.get("rscale") is not None:
            z = mul(z, f["rscale"])
        return sweep(f["rpu"], f["rlu"], f["cju"], f["cvu"], z, True)


# ------------------------------------------------------------------------------------------------ factors
@functools.lru_cache(maxsize=None)
def row_factor(shape):
    """tri.tri_factor with a right-hand-side scale; the unscaled form is the same dict with rscale = None (unscaled())"""
    f = tri.tri_factor(shape, 7000 + tri.TRI_SHAPES.index(shape), True)
    f["nlevu"] = f["nlev"]
    return f


def unscaled(f):
    g = dict(f)
    g["rscale"] = None
    return g


@functools.lru_cache(maxsize=None)
def node_factor(name):
    """ILU(0) factor of a random node graph (every node a dense block of dofs, a path so that the levels are deep), as
    test_ilu0_node_blocked_solves_carry_the_bits_of_the_inode_routine builds it: `mixed` 300 nodes of 1..5 rows, `fixed3` 250 nodes
    of 3 rows (block columns).  The arguments of mi355x_trisolve_plan_create_nodes_pair, in the keys of tri.tri_factor."""
    import scipy.sparse as sp
    rng = np.random.default_rng(41 if name == "mixed" else 43)
    nn = 300 if name == "mixed" else 250
    dof = rng.integers(1, 6, nn) if name == "mixed" else np.full(nn, 3)
    G = sp.random(nn, nn, density=4.0 / nn, random_state=int(rng.integers(1 << 30)), format="csr")
    G = ((G + G.T + sp.diags([np.ones(nn - 1)], [1]) + sp.diags([np.ones(nn - 1)], [-1]) + sp.eye(nn)) != 0).tocsr()
    start = np.concatenate([[0], np.cumsum(dof)])
    n = int(start[-1])
    rows, cols = [], []
    for u in range(nn):
        cc = np.concatenate([np.arange(start[v], start[v + 1]) for v in sorted(G.indices[G.indptr[u]:G.indptr[u + 1]])])
        for r in range(start[u], start[u + 1]):
            rows.append(np.full(cc.size, r)); cols.append(cc)
    rows = np.concatenate(rows); cols = np.concatenate(cols)
    A = sp.csr_matrix((-rng.random(rows.size), (rows, cols)), shape=(n, n)); A.sort_indices()
    A = (A + sp.diags(np.asarray(abs(A).sum(axis=1)).ravel() + 1.0)).tocsr(); A.sort_indices()
    ai, aj, aa = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.copy()
    nodes, ns = orc.check_inode(ai, aj)
    assert nodes > 0 and ns.max() <= 5 and int(ns.sum()) == n
    fac = orc.ilu0_factor(ai, aj, aa)
    bi, bj, bd, ba = fac
    f = dict(n=n, nstart=np.concatenate(([0], np.cumsum(ns))).astype(np.int32), rp=np.ascontiguousarray(bi[:n]), rl=np.diff(bi).astype(np.int32),
             rpu=(bd[1:] + 1).astype(np.int32), rlu=(bd[:-1] - bd[1:] - 1).astype(np.int32), cj=bj, cv=ba, cju=bj, cvu=ba,
             dinv=ba[bd[:n]].copy(), rscale=None, ilu=fac, ns=ns)
    return with_node_levels(f)


def with_node_levels(f):
    """lev / levu: the dependency level of every NODE, from its first row's list (lower) / its last row's (upper)"""
    ns = f["nstart"]
    nodes = ns.size - 1
    nodeof = np.repeat(np.arange(nodes), np.diff(ns))
    lev = np.zeros(nodes, dtype=np.int32); levu = np.zeros(nodes, dtype=np.int32)
    for u in range(nodes):
        r = ns[u]
        c = nodeof[f["cj"][f["rp"][r]:f["rp"][r] + f["rl"][r]]]
        lev[u] = lev[c].max() + 1 if c.size else 0
    for u in range(nodes - 1, -1, -1):
        r = ns[u + 1] - 1
        c = nodeof[f["cju"][f["rpu"][r]:f["rpu"][r] + f["rlu"][r]]]
        levu[u] = levu[c].max() + 1 if c.size else 0
    f.update(lev=lev, levu=levu, nlev=int(lev.max()) + 1, nlevu=int(levu.max()) + 1)
    return f


def one_sided(f, config):
    """`L`: the upper factor without off-diagonal entries (dinv kept; node factors keep the couplings inside the nodes, which the
    plan's shape check asks for); `U`: the lower factor without entries; `both`: f itself"""
    if config == "both":
        return f
    g = dict(f)
    n = f["n"]
    if not is_nodes(f):
        if config == "L":
            g.update(rlu=np.zeros(n, dtype=np.int32), levu=np.zeros(n, dtype=np.int32), nlevu=1)
        else:
            g.update(rl=np.zeros(n, dtype=np.int32), lev=np.zeros(n, dtype=np.int32), nlev=1)
        return g
    ns = f["nstart"]
    first = np.repeat(ns[:-1], np.diff(ns)); last = np.repeat(ns[1:] - 1, np.diff(ns))
    r = np.arange(n)
    if config == "L":
        g["rlu"] = (last - r).astype(np.int32)                               # the couplings come first in an upper row
    else:
        g["rp"] = (f["rp"] + f["rl"][first]).astype(np.int32)               # ... and last in a lower row
        g["rl"] = (r - first).astype(np.int32)
    return with_node_levels(g)


# ------------------------------------------------------------------------------------------------ layout, graph, targets
def items(f, upper):
    """(level, list length, first row, last row) of every item a position holds: a row, or a node with its shared list"""
    ns = f["nstart"] if is_nodes(f) else np.arange(f["n"] + 1)
    lead = (ns[1:] - 1) if upper else ns[:-1]
    rl = (f["rlu"] if upper else f["rl"])[lead]
    lev = f["levu"] if upper else f["lev"]
    return np.asarray(lev), np.asarray(rl), ns[:-1], ns[1:] - 1


def layout(lev, length, align):
    """tri_level_layout: items by level, longer lists first (stable in the item number); with `align` a level of ALIGN_MIN items or
    more starts on a slice boundary.  Returns the item at every position (-1: padding) up to the end of the last slice."""
    order = np.lexsort((np.arange(lev.size), -length.astype(np.int64), lev))
    pos, cur = np.empty(lev.size, dtype=np.int64), 0
    lo = 0
    counts = np.bincount(lev)
    for c in counts:
        if align and c >= ALIGN_MIN and cur % W:
            cur += W - cur % W
        pos[lo:lo + c] = np.arange(cur, cur + c)
        cur += int(c); lo += int(c)
    at = np.full(((cur + W - 1) // W) * W, -1, dtype=np.int64)
    at[pos] = order
    return at


def shared_list(f, upper, u):
    lev, rl, r0, rL = items(f, upper)
    lead = rL[u] if upper else r0[u]
    rp = (f["rpu"] if upper else f["rp"])[lead]              # (the last row of a node has no couplings in front of the shared list)
    cj = f["cju"] if upper else f["cj"]
    return cj[rp:rp + rl[u]]


def targets(f, aligns=(False, True)):
    """name -> row: the rows Part A must have poisoned in some round (see the module's docstring and the issue): the row at
    position 0 of each plan, the first and the last row of a slice, the first and the last entry of the longest list, entry 0 of a
    list of at least 9 entries, the first and the last row of a node of more than one row."""
    t = {}
    if is_nodes(f):
        aligns = (True,)
    for upper in (False, True):
        lev, rl, r0, rL = items(f, upper)
        side = "U" if upper else "L"
        for align in aligns:
            at = layout(lev, rl, align)
            tag = side + (".aligned" if align and len(aligns) > 1 else "")
            real = np.flatnonzero(at >= 0)
            first = W if at.size > W and at[W] >= 0 else int(real[0])
            last = W - 1 if at.size > W and at[W - 1] >= 0 else int(real[-1])
            named = {"pos0": int(r0[at[0]]), "slice_first": int(r0[at[first]]), "slice_last": int(rL[at[last]])}
            if at.size > W:
                named["last_position"] = int(rL[at[real[-1]]])
            for k, r in named.items():
                if t.get(side + "." + k) != r:                # (the aligned layout is named only where it differs)
                    t[tag + "." + k] = r
        if rl.max() > 0:
            u = int(np.argmax(rl))
            cols = shared_list(f, upper, u)
            t[side + ".list_first"] = int(cols[0]); t[side + ".list_last"] = int(cols[-1])
        if rl.max() >= 9:
            u = int(np.flatnonzero(rl >= 9)[0])
            t[side + ".entry0_of_9"] = int(shared_list(f, upper, u)[0])
            odd = np.flatnonzero((rl >= 9) & (rl % 2 == 1))
            if odd.size:
                t[side + ".entry0_of_odd"] = int(shared_list(f, upper, int(odd[0]))[0])
    if is_nodes(f):
        sz = np.diff(f["nstart"])
        multi = np.flatnonzero(sz > 1)
        if multi.size:
            u = int(multi[multi.size // 2])
            t["node_first"] = int(f["nstart"][u]); t["node_last"] = int(f["nstart"][u + 1] - 1)
    return t


def reach_matrix(f, seeds):
    """bool [n, len(seeds)]: column k = the rows seed k can reach, forward through L's dependency graph, then U's graph seeded with
    everything L reached (rscale and dinv add no rows)"""
    n = f["n"]
    R = np.zeros((n, len(seeds)), dtype=bool)
    R[np.asarray(seeds, dtype=np.int64), np.arange(len(seeds))] = True
    rp, rl, cj = f["rp"], f["rl"], f["cj"]
    for i in np.flatnonzero(rl > 0):
        R[i] |= R[cj[rp[i]:rp[i] + rl[i]]].any(axis=0)
    rp, rl, cj = f["rpu"], f["rlu"], f["cju"]
    for i in np.flatnonzero(rl > 0)[::-1]:
        R[i] |= R[cj[rp[i]:rp[i] + rl[i]]].any(axis=0)
    return R


def choose_rounds(f, seed):
    """The rounds of a case: each a set S of poisoned rows and the rows S reaches.  A round takes the targets no earlier round
    held first, then random rows, each unless it would leave fewer than MIN_REST of the rows untouched; random rows are added
    until 30 % of the rows are reached.  Rounds are added while one of them takes an open target, up to MAX_ROUNDS.  Returns
    (list of (S, reach), names of the targets held, names of the targets no round could hold)."""
    n = f["n"]
    tg = targets(f)
    trows = list(dict.fromkeys(tg.values()))
    rng = np.random.default_rng(seed)
    nrand = min(n, 24 + (n // 16 if n <= 9000 else 0))
    cand = trows + [int(r) for r in rng.choice(n, size=nrand, replace=False) if int(r) not in trows]
    R = reach_matrix(f, cand)
    cap = n - int(np.ceil(MIN_REST * n))
    rounds, held = [], set()
    while len(rounds) < MAX_ROUNDS:
        open_ = [k for k in range(len(trows)) if trows[k] not in held]
        if len(rounds) >= ROUNDS and not open_:
            break
        s = len(rounds) % max(1, len(open_))
        order = open_[s:] + open_[:s] + [int(k) for k in len(trows) + np.random.default_rng(seed + 100 * len(rounds)).permutation(len(cand) - len(trows))]
        S, reach = [], np.zeros(n, dtype=bool)
        for i, k in enumerate(order):
            if i >= len(open_) and reach.sum() >= 0.3 * n:
                break
            new = reach | R[:, k]
            if new.sum() <= cap:
                S.append(cand[k]); reach = new
        took = set(S) & {trows[k] for k in open_}
        if len(rounds) >= ROUNDS and not took:
            break
        rounds.append((np.array(sorted(S), dtype=np.int64), reach))
        held |= set(S)
    return rounds, sorted(k for k, r in tg.items() if r in held), sorted(k for k, r in tg.items() if r not in held)


def conditions_met(f, rounds):
    n = f["n"]
    need = 1 if n <= 65 else int(np.ceil(MIN_REACH * n))
    return bool(rounds) and all(S.size and reach.sum() >= need and (~reach).sum() >= MIN_REST * n for S, reach in rounds)


def poison(b, S, shift=0):
    """b with the entries S overwritten, cycling NaN, +Inf, -Inf (numpy's default quiet NaN)"""
    bp = b.copy()
    bp[S] = SPECIALS[(np.arange(S.size) + shift) % SPECIALS.size]
    return bp


def clean_b(n, seed):
    return np.clip(np.random.default_rng(seed).standard_normal(n), -1e3, 1e3)


def base_factor(name):
    return node_factor(name) if name in NODE_FACTORS else row_factor(name)


@functools.lru_cache(maxsize=None)
def part_a_case(name, config):
    """dict(f, b, rounds, held, unreached, kept): the factor of shape / node factor `name` in configuration `config` (scaled where it
    is a row factor), the clean right-hand side, the rounds; kept: the conditions of Part A hold in every round"""
    f = one_sided(base_factor(name), config)
    rounds, held, unreached = choose_rounds(f, 5 + 17 * CONFIGS.index(config))
    return dict(f=f, b=clean_b(f["n"], 31), rounds=rounds, held=held, unreached=unreached, kept=conditions_met(f, rounds))


@functools.lru_cache(maxsize=None)
def part_a_refs(name, config, scaled):
    """(reference of the clean right-hand side, [(poisoned right-hand side, its reference) per round]), computed once"""
    c = part_a_case(name, config)
    f = c["f"] if scaled or is_nodes(c["f"]) else unscaled(c["f"])
    out = []
    for j, (S, _) in enumerate(c["rounds"]):
        bp = poison(c["b"], S, j)
        out.append((bp, reference(f, bp)))
    return reference(f, c["b"]), out


# Pairs dropped from Part A by name: no set S leaves a quarter of the rows untouched and reaches a twentieth (or, n <= 65, one
# row).  n1 is a single row: the row S reaches is all there is; with both factors the dense 5 x 5 triangle of tiny is reached whole
# from any row, and one poisoned entry of wide, ragged and the node factors (a path through all nodes) reaches nearly every row
# behind it in L and from there nearly every row in U.  (tiny one-sided and chain with both factors do have such sets -- rows 2 mod
# 3 of chain are named by no row -- and stay.)
DROPPED = {("tiny", "both"), ("n1", "L"), ("n1", "U"), ("n1", "both"), ("wide", "both"), ("ragged", "both"), ("mixed", "both"), ("fixed3", "both")}


# Targets no round of a kept pair could hold: the row alone reaches more than three quarters of the rows (the row at position 0 is a
# row of level 0 -- on a chain or a path the first one, and everything hangs on it).  Asserted to be exactly this.
UNREACHED = {
    ("chain", "L"): ["L.list_first", "L.list_last", "L.pos0", "L.slice_first", "L.slice_last", "U.pos0", "U.slice_first", "U.slice_last"],
    ("chain", "U"): ["L.last_position", "U.pos0", "U.slice_first"],
    ("chain", "both"): ["L.last_position", "L.list_first", "L.list_last", "L.pos0", "L.slice_first", "L.slice_last", "U.last_position", "U.pos0",
                        "U.slice_first", "U.slice_last"],
    ("empty_rows", "both"): ["L.list_first", "L.list_last", "L.pos0", "U.pos0"],
    ("fixed3", "L"): ["L.entry0_of_9", "L.entry0_of_odd", "L.list_first", "L.pos0", "U.pos0"],
    ("fixed3", "U"): ["L.last_position", "U.list_last", "U.pos0"],
    ("mixed", "L"): ["L.entry0_of_9", "L.entry0_of_odd", "L.list_first", "L.pos0", "L.slice_first", "L.slice_last", "U.pos0", "U.slice_first",
                     "U.slice_last"],
    ("mixed", "U"): ["L.last_position", "U.list_last", "U.pos0", "U.slice_first", "U.slice_last"],
    ("ragged", "L"): ["L.entry0_of_9", "L.entry0_of_odd", "L.list_first", "L.list_last", "L.pos0", "L.slice_first", "L.slice_last", "U.pos0",
                      "U.slice_first", "U.slice_last"],
    ("ragged", "U"): ["L.last_position"],
    ("tiny", "L"): ["L.list_first", "L.pos0", "L.slice_first", "U.pos0", "U.slice_first"],
    ("tiny", "U"): ["L.slice_last", "U.list_last", "U.pos0", "U.slice_first"],
    ("wide", "L"): ["L.list_first", "L.list_last", "L.pos0", "L.slice_first", "L.slice_last", "U.pos0"],
    ("wide", "U"): ["L.last_position", "U.pos0", "U.slice_first", "U.slice_last"],
}


def part_a_cases():
    return [(s, c) for s in A_SHAPES + NODE_FACTORS for c in CONFIGS if (s, c) not in DROPPED]


def check_rule(got, ref, rows, what):
    """the comparison rule on `rows`: NaN where the reference is NaN (sign and payload not compared), every other value -- +-Inf,
    +-0.0, subnormals -- the same bits"""
    bad = rows & differing(got, ref)
    assert not bad.any(), "%s: %d rows differ from the reference, first %s: got %r, reference %r" % (
        what, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:8], ref[bad][:8])


def check_containment(clean, pois, ref, reach, what):
    """rows S cannot reach: the poisoned run equals the clean one bit for bit; rows it can: the comparison rule"""
    leak = ~reach & (bits(pois) != bits(clean))
    assert not leak.any(), "%s: rows %s are out of reach of the poisoned entries and changed: %r -> %r" % (
        what, np.flatnonzero(leak)[:8], clean[leak][:8], pois[leak][:8])
    check_rule(pois, ref, reach, what)


# ------------------------------------------------------------------------------------------------ Part B: hand-built factors
INF, QNAN = np.inf, np.nan
NB_ROWS = 130


def _factor_from_rows(n, lower, upper, dinv, rscale):
    """tri.tri_factor's dict from row -> [(column, value)] tables (entries in the order given)"""
    def arrays(tab):
        rl = np.array([len(tab.get(i, ())) for i in range(n)], dtype=np.int32)
        rp, cj, _ = tri.tri_arrays(n, rl, [[c for c, _ in tab.get(i, ())] for i in range(n)])
        cv = np.full(cj.size, np.nan)
        for i in range(n):
            cv[rp[i]:rp[i] + rl[i]] = [v for _, v in tab.get(i, ())]
        return rp, rl, cj, cv
    rp, rl, cj, cv = arrays(lower)
    lev = tri.tri_levels(n, rp, rl, cj)
    rpu, rlu, cju, cvu = arrays(upper)
    levu = np.zeros(n, dtype=np.int32)
    for i in range(n - 1, -1, -1):
        d = cju[rpu[i]:rpu[i] + rlu[i]]
        levu[i] = levu[d].max() + 1 if d.size else 0
    return dict(n=n, nlev=int(lev.max()) + 1, nlevu=int(levu.max()) + 1, lev=lev, rp=rp, rl=rl, cj=cj, cv=cv, levu=levu, rpu=rpu, rlu=rlu,
                cju=cju, cvu=cvu, dinv=np.array(dinv, dtype=np.float64), rscale=None if rscale is None else np.array(rscale, dtype=np.float64))


def _mirror(n, tab):
    return {n - 1 - i: [(n - 1 - c, v) for c, v in ent] for i, ent in tab.items()}


def arith_table():
    """130 rows: rows 0..39 have no entries (sources, the value is b itself), rows 40..64 are the special cases, rows 65..129 finite
    filler on three sources (three slices of positions, the fillers cross the slice boundaries).  Row 0 and row 129 hold a NaN
    and no list names them: they sit at position 0 of the plans (slot 0 of w, which padding entries and clamped indices name) in the
    table and in its mirror image, so a leaked 0.0 * w[slot 0] turns a row stated finite into NaN.  Returns (b, lower rows, z: the
    lower result stated by hand -- None: NaN --, dinv, rscale).  dinv and rscale differ from 1.0 only on rows no other row names,
    rscale only on rows without entries, so that the result is (z * rscale) * dinv row by row whichever half holds the entries."""
    n = NB_ROWS
    b = np.arange(n, dtype=np.float64)
    b[:22] = [QNAN, -1.0, 2.0, INF, -INF, QNAN, 0.0, -0.0, 1e-160, 1e300, 3.0, 0.5, 1e300, MIN_SUB, MID_SUB, DBL_MIN, 1.5, -1e300,
              3.25, INF, -0.0, -INF]
    b[22] = 1.0                                                 # what the lists below call column 0: row 22 (row 0 is the NaN no list names)
    z = {i: (None if np.isnan(b[i]) else float(b[i])) for i in range(40)}
    L = {}

    def row(r, rhs, ent, val):
        b[r] = rhs; L[r] = [(22 if c == 0 else c, v) for c, v in ent]; z[r] = val
    row(40, -0.0, [], -0.0)                                     # -0.0 on a row without entries: itself
    row(41, 1.0, [(0, 1.0)], 0.0)                               # 1 - 1 * 1 = +0.0
    row(42, 0.0, [(0, 1.0), (1, 1.0)], 0.0)                     # (0 - 1) - (1 * -1) = -1 + 1: the products cancel exactly to +0.0
    row(43, 1.0, [(3, 0.0)], None)                              # an entry 0.0 against +Inf: NaN
    row(44, 1.0, [(5, 0.0)], None)                              # ... against NaN
    row(45, 1.0, [(4, -0.0)], None)                             # -0.0 against -Inf
    row(46, 1.0, [(2, 0.0)], 1.0)                               # an entry 0.0 against a finite dependency: nothing changes
    row(47, -0.0, [(2, 0.0)], -0.0)                             # -0.0 - (+0.0) = -0.0: a sum that started from +0.0 would lose the sign
    row(48, -0.0, [(2, -0.0)], 0.0)                             # -0.0 - (-0.0) = +0.0
    row(49, 1.0, [(3, 1.0), (4, 1.0)], None)                    # (1 - Inf) - (-Inf) = -Inf + Inf: NaN
    row(50, 1.0, [(9, 1e10)], -INF)                             # 1e10 * 1e300 overflows: 1 - Inf
    row(51, 1.0, [(9, -1e10)], INF)
    row(52, 0.0, [(3, 2.0)], -INF)
    row(53, 0.0, [(8, -1e-160)], 1e-160 * 1e-160)               # a subnormal product
    row(54, 3 * MIN_SUB, [(13, 1.0)], 2 * MIN_SUB)              # subnormal b, subnormal dependency
    row(55, 2.5e-308, [(0, 2.4e-308)], 2.5e-308 - 2.4e-308)     # normal operands, the difference underflows
    row(56, 0.0, [(2, MIN_SUB)], -2 * MIN_SUB)                  # a subnormal entry
    row(57, MID_SUB, [], MID_SUB)
    row(58, 1.0, [(c, 1.0) for c in (0, 1, 2, 3, 6, 7, 10, 11, 16)], -INF)           # 9 entries (a second batch of one), +Inf among them
    row(59, 0.0, [(c, 1.0) for c in (0, 1, 2, 6, 7, 10, 11, 16)], -7.0)             # 8 entries: 0-1+1-2-0+0-3-0.5-1.5
    row(60, 0.0, [(c, 1.0) for c in (0, 1, 2, 6, 7, 10, 11)], -5.5)                 # 7 entries
    row(61, 0.0, [(c, 1.0) for c in (0, 1, 2, 6, 7, 10, 11, 16, 40)], -7.0)         # 9 entries, the last one -0.0
    row(62, 1.0, [(49, 1.0)], None)                             # a NaN one level on
    row(63, 1.0, [(50, 0.0)], None)                             # 0.0 * -Inf one level on
    row(64, 0.0, [(53, 1.0)], -(1e-160 * 1e-160))               # a subnormal value handed on
    src = (1.0, -1.0, 2.0)
    for r in range(65, n):
        row(r, 0.25 * r, [((r - 65) % 3, 0.5)], 0.25 * r - 0.5 * src[(r - 65) % 3])
    row(66, -0.0, [(7, -1.0)], -0.0)                            # -0.0 - (-1.0 * -0.0) = -0.0: one more product -1.0 * 0.0 would make it +0.0
    row(129, QNAN, [], None)                                    # the mirror image's row 0
    for r in range(22, 40):
        z[r] = float(b[r])
    dinv = np.ones(n); rs = np.ones(n)
    dinv[41] = -2.0; dinv[47] = 2.0; dinv[48] = -3.0            # +-0.0 * dinv: the sign follows dinv
    dinv[51] = 0.0; dinv[52] = -1.0                             # Inf * 0.0 = NaN, -Inf * -1 = +Inf
    dinv[70], dinv[71], dinv[72], dinv[73], dinv[74], dinv[75] = 0.0, INF, -INF, QNAN, MIN_SUB, -0.0     # what a zero pivot leaves
    dinv[57] = 0.5; dinv[54] = 0.5                              # subnormal * 0.5: rounds, not flushed
    rs[18] = -2.0; rs[19] = 0.0; rs[20] = -1.0; rs[21] = 2.0    # finite, 0.0 * Inf = NaN, -0.0 * -1 = +0.0, 2 * -Inf
    rs[24] = INF; rs[23] = MIN_SUB; rs[57] = 2.0
    dinv[20] = -2.0                                             # (-0.0 * -1) * -2 = -0.0
    return b, L, z, dinv, rs


def special_tables():
    """name -> dict(f, b, expect, kinds): the hand-built row factors of Part B.  expect[row]: the stated result (None: NaN), for
    every row; kinds: what the table is about.  `arith_lower` holds the entries in the lower factor, `arith_upper` is its mirror
    image (row and column i -> n - 1 - i) in the upper factor; `nan_chain_*`: a NaN in b through a chain of 77 rows."""
    n = NB_ROWS
    b, L, z, dinv, rs = arith_table()
    with np.errstate(all="ignore"):
        zz = np.array([np.nan if z[i] is None else z[i] for i in range(n)])
        x_scaled, x_plain = (zz * rs) * dinv, zz * dinv
    out = {}
    for scaled in (False, True):
        x = x_scaled if scaled else x_plain
        tag = "_scaled" if scaled else ""
        out["arith_lower" + tag] = dict(f=_factor_from_rows(n, L, {}, dinv, rs if scaled else None), b=b, expect=x)
        out["arith_upper" + tag] = dict(f=_factor_from_rows(n, {}, _mirror(n, L), dinv[::-1], rs[::-1] if scaled else None), b=b[::-1].copy(), expect=x[::-1].copy())
    # the NaN chain: row i names row i - 1 for 1 <= i < 80 (80 levels of one row: sub-steps inside a slice, then a slice boundary);
    # b[3] = NaN: rows 3..79 are NaN, everything else finite.  Rows 80..129 name row 0 or 1.
    chain = {i: [(i - 1, 0.5)] for i in range(1, 80)}
    chain.update({i: [(i % 2, 0.25)] for i in range(80, n)})
    bc = 1.0 + 0.125 * np.arange(n)
    bc[3] = QNAN
    expect = np.zeros(n)
    for i in range(n):                                         # exact in binary: halves of multiples of 1/8 down to 2^-82
        expect[i] = bc[i] - (0.5 * expect[i - 1] if 1 <= i < 80 else (0.25 * expect[i % 2] if i >= 80 else 0.0))
    expect[3:80] = QNAN
    out["nan_chain_lower"] = dict(f=_factor_from_rows(n, chain, {}, np.ones(n), None), b=bc, expect=expect)
    out["nan_chain_upper"] = dict(f=_factor_from_rows(n, {}, _mirror(n, chain), np.ones(n), None), b=bc[::-1].copy(), expect=expect[::-1].copy())
    both = _factor_from_rows(n, chain, _mirror(n, chain), np.full(n, 0.5), None)
    # both halves: L makes rows 3..79 NaN; in U row i names row i + 1 for 50 <= i <= 128 and rows below 50 name row 129 or 128, which
    # are finite: the NaN rows of the result are rows 3..79 (expect: None, the classes are stated)
    nan_rows = np.zeros(n, dtype=bool); nan_rows[3:80] = True
    out["nan_chain_both"] = dict(f=both, b=bc, expect=None, nan_rows=nan_rows)
    return out


def _assemble_nodes(nodes):
    """node factor from (rows, shared columns, values [row][column], lower couplings [row][earlier row], b, upper couplings, dinv) per
    node, in row order.  Upper couplings: one value for every coupling, or {row of the node: [values for its later rows]}.  The upper
    factor holds only the couplings inside the nodes and the inverted diagonals.  One cj / cv for both halves, as the node ABI
    takes them: L's rows first, then U's."""
    n = sum(nd[0] for nd in nodes)
    assert n <= NB_ROWS
    b, dinv, nstart = np.zeros(n), np.ones(n), [0]
    rowsL, rowsU = [[] for _ in range(n)], [[] for _ in range(n)]
    r = 0
    for sz, cols, vals, lcoup, rhs, ucoup, dv in nodes:
        for k in range(sz):
            rowsL[r + k] = [(c, vals[k][q]) for q, c in enumerate(cols)] + [(r + l, lcoup[k][l]) for l in range(k)]
            later = range(r + k + 1, r + sz)
            rowsU[r + k] = list(zip(later, ucoup[k])) if isinstance(ucoup, dict) else [(c, ucoup) for c in later]
            b[r + k] = rhs[k]; dinv[r + k] = dv[k]
        r += sz
        nstart.append(r)
    rl = np.array([len(e) for e in rowsL], dtype=np.int32); rlu = np.array([len(e) for e in rowsU], dtype=np.int32)
    rp = (tri.PAD + np.concatenate(([0], np.cumsum(rl)[:-1]))).astype(np.int32)
    rpu = (tri.PAD + int(rl.sum()) + 3 + np.concatenate(([0], np.cumsum(rlu)[:-1]))).astype(np.int32)
    cj = np.full(tri.PAD + int(rl.sum()) + 3 + int(rlu.sum()) + 5, 0, dtype=np.int32)
    cv = np.full(cj.size, np.nan)
    for i in range(n):
        for q, (c, v) in enumerate(rowsL[i]):
            cj[rp[i] + q], cv[rp[i] + q] = c, v
        for q, (c, v) in enumerate(rowsU[i]):
            cj[rpu[i] + q], cv[rpu[i] + q] = c, v
    f = with_node_levels(dict(n=n, nstart=np.array(nstart, dtype=np.int32), rp=rp, rl=rl, rpu=rpu, rlu=rlu, cj=cj, cv=cv, cju=cj, cvu=cv,
                              dinv=dinv, rscale=None))
    return f, b


B_UPPER = {0: [0.25, -0.25], 1: [0.25], 2: []}      # upper couplings of the (-Inf, +Inf, -Inf) nodes: no Inf meets its opposite


def node_table():
    """The hand-built node factor of Part B: 16 single-row nodes without entries (sources), the special nodes A .. I of 2, 3, 5, 2, 3,
    3, 2, 5 and 2 rows, and 43 finite nodes of 2 rows (68 positions: two slices).  Row 0 -- position 0 of both plans, slot 0 of w,
    which padding entries and clamped indices name -- holds a NaN and no list names it: every row stated finite stays finite only
    if no such entry leaks.  Returns dict(f, b, seq_row): seq_row the row whose pair of shared columns overflows only when the two
    products are added to each other first."""
    src = [QNAN, -1.0, 2.0, INF, -INF, 1.0, 0.0, -0.0, 1e-160, 1e300, 3.0, 0.5, -1e300, MIN_SUB, 1.5, 1e300]
    nodes = [(1, [], [[]], [[]], [v], 0.0, [1.0]) for v in src]
    # A (2 rows): the two products of a pair are +Inf and -Inf: NaN in row 16 whichever the order; row 17: +Inf + +Inf, then its coupling to the NaN
    nodes.append((2, [3, 4], [[1.0, 1.0], [1.0, -1.0]], [[], [0.0]], [1.0, 1.0], 0.25, [1.0, 1.0]))
    # B (3 rows): x9 = x15 = 1e300, b = 1e308: added first the products give 1e308 + 1e308 = Inf, so row 18 is -Inf; one after the
    # other 1e308 - 1e308 - 1e308 = -1e308, finite.  Row 19: 2 - (1e300 - 1e300) = 2, minus 1.0 * -Inf: +Inf.  Row 20: -0.0 - 0.0 = -0.0,
    # minus -1.0 * -Inf: -Inf, minus 1.0 * +Inf: -Inf.
    nodes.append((3, [9, 15], [[1e8, 1e8], [1.0, -1.0], [0.0, 0.0]], [[], [1.0], [-1.0, 1.0]], [1e308, 2.0, -0.0], B_UPPER, [1.0, 1.0, 1.0]))
    # C (5 rows): three shared columns (an odd last column alone), finite and exact
    nodes.append((5, [5, 1, 2], [[k + 1.0] * 3 for k in range(5)], [[0.5] * k for k in range(5)], [10.0] * 5, 0.25, [1.0, 0.5, -1.0, 2.0, 0.25]))
    # D (2 rows): a subnormal product, a subnormal coupling result
    nodes.append((2, [8], [[1e-160], [1.0]], [[], [1.0]], [0.0, 1e-160], 0.0, [1.0, 0.5]))
    # E (3 rows): signed zeros: 1 * 0.0 + 1 * -0.0 = +0.0; -0.0 - 0.0 = -0.0
    nodes.append((3, [6, 7], [[1.0, 1.0], [1.0, 1.0], [2.0, 0.5]], [[], [-1.0], [0.0, 0.0]], [-0.0, 0.0, 3.0], 0.0, [1.0, 1.0, 1.0]))
    # F (3 rows), G (2 rows), H (5 rows): finite sums, inverted diagonals 0.0, +-Inf, NaN, subnormal
    nodes.append((3, [5, 2], [[1.0, 1.0]] * 3, [[0.5] * k for k in range(3)], [7.0, 8.0, 9.0], 0.0, [0.0, INF, MIN_SUB]))
    nodes.append((2, [1], [[1.0], [2.0]], [[], [0.5]], [1.0, 2.0], 0.0, [-INF, 1.0]))
    nodes.append((5, [5, 1, 2, 10], [[1.0, 0.5, 0.25, 2.0]] * 5, [[0.25] * k for k in range(5)], [1.0, 2.0, 3.0, 4.0, 5.0], 0.0, [1.0, QNAN, 1.0, 0.0, 1.0]))
    # I (2 rows): ONE shared column, x7 = -0.0: row 41 is -0.0 - (1.0 * -0.0) = +0.0.  An odd last column paired with anything -- even
    # with 1.0 * 0.0 -- gives -0.0 - (-0.0 + 0.0) = -0.0 instead.
    nodes.append((2, [7], [[1.0], [0.0]], [[], [0.0]], [-0.0, 1.0], 0.0, [1.0, 1.0]))
    for g in range(43):
        nodes.append((2, [(5, 1, 2)[g % 3], 10 + g % 2], [[0.5, 0.25], [0.25, 0.5]], [[], [0.5]], [1.0 + g, 2.0 + g], 0.25, [0.5, 2.0]))
    f, b = _assemble_nodes(nodes)
    return dict(f=f, b=b, seq_row=18, nsrc=len(src))


def block_node_table():
    """The hand-built factor of Part B for block columns: 43 nodes of 3 rows (129 rows, one slice: 130 rows do not hold 65 nodes
    of 3), every shared list a run of whole dependency nodes.  Source nodes S0 .. S7 (no shared columns; their rows are coupled,
    so a node holds one kind of value), consumers a .. h, 28 finite nodes.  Node 0 -- position 0 of both plans -- is NaN and no
    list names it.  The result of a source node is its b where the couplings are 0.0 against finite values, and all +Inf / all
    -Inf for S2 / S3 (couplings -1.0: Inf never meets its opposite).  Returns dict(f, b, seq_row)."""
    z3, m3 = [[], [0.0], [0.0, 0.0]], [[], [-1.0], [-1.0, -1.0]]
    none = [[], [], []]

    def source(b3, coup, uc):
        return (3, [], none, coup, b3, uc, [1.0, 1.0, 1.0])
    nodes = [source([1.0, 2.0, QNAN], z3, 0.0),                  # S0 rows 0..2: NaN, unnamed
             source([1.0, -1.0, 2.0], z3, 0.0),                  # S1 rows 3..5
             source([INF, 1.0, 1.0], m3, -1.0),                  # S2 rows 6..8: 1 - (-1 * Inf) = +Inf in every row
             source([-INF, 1.0, 1.0], m3, -1.0),                 # S3 rows 9..11: all -Inf
             source([0.0, -0.0, 0.0], z3, 0.0),                  # S4 rows 12..14
             source([1e300, 1e300, 1e300], z3, 0.0),             # S5 rows 15..17
             source([1e-160, MIN_SUB, 3.0], z3, 0.0),            # S6 rows 18..20
             source([0.0, 0.0, -0.0], z3, 0.0)]                  # S7 rows 21..23
    S = lambda k: [3 * k, 3 * k + 1, 3 * k + 2]                  # noqa: E731
    # a (rows 24..26): columns of S2 then S3; the middle pair is x8 = +Inf with x9 = -Inf: NaN, and the couplings hand it on
    nodes.append((3, S(2) + S(3), [[1.0] * 6, [1.0, 1.0, 1.0, -1.0, -1.0, -1.0], [1.0] * 6], z3, [1.0, 1.0, 1.0], 0.0, [1.0] * 3))
    # b (rows 27..29): three columns of 1e300; the pair 1e8 * 1e300 + 1e8 * 1e300 overflows added first (row 27 = 1e308 - Inf = -Inf;
    # one after the other -1e308), the odd third column has value 0.0.  Rows 28, 29 as node B of node_table: +Inf, -Inf.
    nodes.append((3, S(5), [[1e8, 1e8, 0.0], [1.0, -1.0, 0.0], [0.0, 0.0, 0.0]], [[], [1.0], [-1.0, 1.0]], [1e308, 2.0, -0.0], B_UPPER, [1.0] * 3))
    # c (rows 30..32): an entry 0.0 against -Inf: NaN
    nodes.append((3, S(3), [[0.0, 0.0, 0.0]] * 3, z3, [1.0, 1.0, 1.0], 0.0, [1.0] * 3))
    # d (rows 33..35): signed zeros against S4 = (0.0, -0.0, 0.0), entries 0.0 against the finite S1: row 33 stays -0.0, row 34 +0.0
    nodes.append((3, S(4) + S(1), [[1.0, 1.0, 1.0, 0.0, 0.0, 0.0]] * 3, z3, [-0.0, 0.0, 3.0], 0.0, [1.0] * 3))
    # e (rows 36..38): a subnormal product (1e-160 * 1e-160), a subnormal dependency, a subnormal inverted diagonal
    nodes.append((3, S(6), [[1e-160, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], [[], [1.0], [0.0, 0.0]], [0.0, 0.0, 4.0], 0.0, [1.0, 1.0, MIN_SUB]))
    # f (rows 39..41), g (rows 42..44): finite sums, inverted diagonals 0.0, +Inf, subnormal / -Inf
    nodes.append((3, S(1), [[1.0, 1.0, 1.0]] * 3, [[0.5] * k for k in range(3)], [7.0, 8.0, 9.0], 0.0, [0.0, INF, MIN_SUB]))
    nodes.append((3, S(1) + S(6), [[1.0, 0.5, 0.25, 0.0, 0.0, 1.0]] * 3, [[0.25] * k for k in range(3)], [1.0, 2.0, 3.0], 0.0, [-INF, 1.0, 0.5]))
    # h (rows 45..47): the odd last column is x23 = -0.0: row 45 is (-0.0 - (0 * 0 + 0 * 0)) - (1.0 * -0.0) = +0.0; paired with anything it is -0.0
    nodes.append((3, S(7), [[0.0, 0.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], z3, [-0.0, 1.0, 2.0], 0.0, [1.0] * 3))
    for g in range(27):
        nodes.append((3, S(1) + (S(6) if g % 2 else []), [[0.5, 0.25, 0.125] + ([0.0, 0.0, 1.0] if g % 2 else [])] * 3, [[0.5] * k for k in range(3)],
                      [1.0 + g, 2.0 + g, 3.0 + g], 0.25, [0.5, 2.0, 1.0]))
    f, b = _assemble_nodes(nodes)
    return dict(f=f, b=b, seq_row=27)


# ------------------------------------------------------------------------------------------------ Part C: nothing stale
C_FACTORS = ["ragged", "chain", "n65", "mixed"]


@functools.lru_cache(maxsize=None)
def part_c_case(name):
    """(factor, [(right-hand side, its reference or None)]): clean b0, poisoned b, clean b1, all-NaN b, clean b2; the reference of
    the clean ones only (the poisoned ones are there for what they leave behind)"""
    f = base_factor(name)
    f = f if is_nodes(f) else unscaled(f)
    n = f["n"]
    rng = np.random.default_rng(77)
    seq = []
    for j in range(5):
        if j == 1:
            seq.append((poison(clean_b(n, 90), np.sort(rng.choice(n, size=max(1, n // 7), replace=False))), None))
        elif j == 3:
            seq.append((np.full(n, np.nan), None))
        else:
            b = clean_b(n, 91 + j)
            seq.append((b, reference(f, b)))
    return f, seq
