"""Synthetic triangular structures for the row-plan tests and the plain float64 restatement of the two sweeps the solve
kernels are compared with (used by test_kernels_gpu.py, test_abi_kernels_gpu.py and, for its own validation, test_host_cpu.py)."""
import numpy as np

TRI_SHAPES = ["wide", "ragged", "chain", "tiny", "empty_rows", "n1", "n64", "n65", "longrow", "deepchain"]
TRI_SIZES = {"wide": 40000, "ragged": 9000, "chain": 700, "tiny": 5, "empty_rows": 3000, "n1": 1, "n64": 64, "n65": 65, "longrow": 4000, "deepchain": 70000}
PAD = 17                                                  # the rows' entries do not start at the arrays' first element


def tri_levels(n, rp, rl, cj):
    lev = np.zeros(n, dtype=np.int32)
    for i in range(n):
        d = cj[rp[i]:rp[i] + rl[i]]
        lev[i] = (lev[d].max() + 1) if d.size else 0
    return lev


def tri_structure(shape, rng):
    """(n, rl, cols): a strictly lower-triangular dependency structure, cols[i] the sorted columns of row i"""
    n = TRI_SIZES[shape]
    rl = np.zeros(n, dtype=np.int32)
    cols = []
    for i in range(n):
        if shape == "wide":
            cand = sorted(c for c in (i - 7000, i - 200, i - 1) if c >= 0 and not (c == i - 1 and i % 200 == 0))   # a 3-D stencil's lower part
        elif shape == "ragged":
            m = int(rng.integers(0, 40)) if i % 11 else 0
            cand = sorted(set(int(c) for c in rng.integers(max(0, i - 3000), max(i, 1), size=m) if c < i)) if i else []
        elif shape in ("chain", "deepchain"):
            cand = [i - 1] if i and i % 3 else ([i - 2] if i > 1 else [])
        elif shape in ("n1", "n64", "n65"):
            cand = [c for c in (i - 1, i - 9) if c >= 0 and i % 4]
        elif shape == "longrow":                            # a few rows with thousands of entries among short ones
            cand = list(range(0, i, 1 if i in (1500, 3999) else max(i, 1))) if i in (1500, 3999) else ([i - 1] if i % 2 else [])
        elif shape == "tiny":
            cand = list(range(i))
        else:
            cand = [] if i % 2 else sorted(set(int(c) for c in rng.integers(0, max(i, 1), size=3) if c < i))
        rl[i] = len(cand); cols.append(cand)
    return n, rl, cols


def tri_arrays(n, rl, cols):
    """(rp, cj, nz): row starts and the column array with PAD leading and 5 trailing entries no row names (an invalid column)"""
    rp = (PAD + np.concatenate(([0], np.cumsum(rl)[:-1]))).astype(np.int32)
    nz = int(rl.sum())
    cj = np.full(PAD + nz + 5, -7, dtype=np.int32)
    for i in range(n):
        cj[rp[i]:rp[i] + rl[i]] = cols[i]
    return rp, cj, nz


def tri_factor(shape, seed, scaled):
    """A lower factor on the structure of `shape` (unit diagonal implied) and an upper factor on its mirror image (row and column
    i -> n - 1 - i, so a row's dependencies are later rows; columns ascending) with an inverted diagonal, |dinv| in [0.5, 2], and,
    scaled, a right-hand-side scale of the same kind (ICC(0)'s 1/D(i)).  Off-diagonal values N(0,1) / (row length + 1).
    Returns a dict of the arguments of mi355x_trisolve_plan_create_pair."""
    rng = np.random.default_rng(seed)
    n, rl, cols = tri_structure(shape, rng)
    rp, cj, nz = tri_arrays(n, rl, cols)
    lev = tri_levels(n, rp, rl, cj)
    cv = np.full(cj.size, np.nan)
    cvu = np.full(cj.size, np.nan)
    for i in range(n):
        cv[rp[i]:rp[i] + rl[i]] = rng.standard_normal(rl[i]) / (rl[i] + 1.0)
    rlu = np.ascontiguousarray(rl[::-1])
    colsu = [sorted(n - 1 - c for c in cols[n - 1 - i]) for i in range(n)]
    rpu, cju, _ = tri_arrays(n, rlu, colsu)
    for i in range(n):
        cvu[rpu[i]:rpu[i] + rlu[i]] = rng.standard_normal(rlu[i]) / (rlu[i] + 1.0)
    levu = np.ascontiguousarray(lev[::-1])

    def signed(k):
        return rng.uniform(0.5, 2.0, k) * np.where(rng.random(k) < 0.5, -1.0, 1.0)
    dinv = signed(n)
    rscale = signed(n) if scaled else None
    return dict(n=n, nlev=int(lev.max()) + 1 if n else 0, lev=lev, rp=rp, rl=rl, cj=cj, cv=cv,
                levu=levu, rpu=rpu, rlu=rlu, cju=cju, cvu=cvu, dinv=dinv, rscale=rscale)


def tri_reference_apply(f, b):
    """y = U^-1 L^-1 b as the header and trisolve_level_kernel state it: one row after the other, entries in stored order,
    sum -= v * x[c]; lower: x[i] = sum; upper: sum starts from the lower result (times rscale[i] if scaled), x[i] = sum * dinv[i].
    Plain Python floats (IEEE double, a rounded product then a rounded subtraction)."""
    n = f["n"]
    rp, rl, cj, cv = f["rp"].tolist(), f["rl"].tolist(), f["cj"].tolist(), f["cv"].tolist()
    z = [0.0] * n
    bl = b.tolist()
    for i in range(n):
        s = bl[i]
        for q in range(rp[i], rp[i] + rl[i]):
            s -= cv[q] * z[cj[q]]
        z[i] = s
    rp, rl, cj, cv = f["rpu"].tolist(), f["rlu"].tolist(), f["cju"].tolist(), f["cvu"].tolist()
    dinv = f["dinv"].tolist()
    rs = f["rscale"].tolist() if f["rscale"] is not None else None
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = z[i]
        if rs is not None:
            s = s * rs[i]
        for q in range(rp[i], rp[i] + rl[i]):
            s -= cv[q] * x[cj[q]]
        x[i] = s * dinv[i]
    return np.array(x, dtype=np.float64).reshape(n)


def tri_node_reference_apply(f, b):
    """y = U^-1 L^-1 b as MatSolve_SeqAIJ_Inode sums it (inode.c:2327-2760; the oracle's orc_ilu0_solve_inode restated on row-level
    arrays): the rows nstart[u] .. nstart[u + 1] of node u share one column list (the first row's in L, the last row's in U); every
    row's sum takes the shared columns two at a time, sum -= v0 * x0 + v1 * x1 (the two rounded products added first), an odd last
    column alone, then the couplings inside the node -- lower: the node's earlier rows in row order; upper: its later rows, nearest
    row last -- and, upper, times the inverted diagonal.  f: the row-level arrays of tri_factor's dict (lower: shared columns, then
    the couplings; upper: the couplings, then the shared columns) and nstart.  Plain Python floats."""
    n = f["n"]
    ns = f["nstart"].tolist()
    rp, rl, cj, cv = f["rp"].tolist(), f["rl"].tolist(), f["cj"].tolist(), f["cv"].tolist()
    z = [0.0] * n
    bl = b.tolist()
    for u in range(len(ns) - 1):
        r0, sz = ns[u], ns[u + 1] - ns[u]
        sh, p0 = rl[r0], rp[r0]
        for k in range(sz):
            p, s, j = rp[r0 + k], bl[r0 + k], 0
            while j < sh - 1:
                s -= cv[p + j] * z[cj[p0 + j]] + cv[p + j + 1] * z[cj[p0 + j + 1]]
                j += 2
            if j == sh - 1:
                s -= cv[p + j] * z[cj[p0 + j]]
            for l in range(k):
                s -= cv[p + sh + l] * z[r0 + l]
            z[r0 + k] = s
    rp, rl, cj, cv = f["rpu"].tolist(), f["rlu"].tolist(), f["cju"].tolist(), f["cvu"].tolist()
    dinv = f["dinv"].tolist()
    x = [0.0] * n
    for u in range(len(ns) - 2, -1, -1):
        sz, rL = ns[u + 1] - ns[u], ns[u + 1] - 1
        sh, p0 = rl[rL], rp[rL]
        for k in range(sz):
            p, s, j = rp[rL - k] + k, z[rL - k], 0
            while j < sh - 1:
                s -= cv[p + j] * x[cj[p0 + j]] + cv[p + j + 1] * x[cj[p0 + j + 1]]
                j += 2
            if j == sh - 1:
                s -= cv[p + j] * x[cj[p0 + j]]
            for l in range(k):
                s -= cv[p - 1 - l] * x[rL - l]
            x[rL - k] = s * dinv[rL - k]
    return np.array(x, dtype=np.float64).reshape(n)
