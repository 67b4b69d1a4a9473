// Numeric ILU(0) on the device, one launch per dependency level of L (MatLUFactorNumeric_SeqAIJ, reference
// src/mat/impls/aij/seq/aijfact.c:505-570, on the factor layout of :1628-1700: L rows forward, U rows stored from the last row
// backwards, the inverted pivot at bdiag[i]; the pivot test is MatPivotCheck_nz, include/petsc-private/matimpl.h:512-528).
//
// Rows of one dependency level of L do not read each other, and every row's own arithmetic is the sequential loop's: the work row
// starts from A's values (+ shift on the diagonal), the L columns k are taken in column order, m = w_k * (1 / u_kk) is stored as
// l_ik, and w_j = w_j - m u_kj (product rounded, then the difference: -ffp-contract=off) for every strict-upper entry of row k whose
// column is in row i's pattern -- everything else ILU(0) discards, so the work row is the row's own pattern and no dense row exists.
// For a fixed j the updates arrive in ascending k as in the sequential loop; within one k the lanes work on different j.
//
// ilu0_factor_level_kernel<W>: W lanes per row, W a power of two <= 64 chosen per matrix from its widest row.
//   * a row of <= W entries lives in registers, one entry per lane (position p of A's sorted row in lane p);
//   * a wider row (W = 64 only) keeps its work row in its own slots of ba; lane l owns the positions p = l, l + 64, ... and is the
//     only lane that ever reads or writes them, so no value passes between lanes through memory.
// Matching u_kj to the row's columns: the strict-upper part of row k is loaded cooperatively, W entries at a time (one coalesced
// load of columns and values), and every lane looks its own column up in that chunk by a binary search over the lanes' registers
// (log2 W shuffles).  Chosen over a search in the sorted list in memory (log2 |U(k)| DEPENDENT loads per lane and per k, each a
// cache round trip) and over a linear scan of the chunk by shuffles (|U(k)| steps: 40 for a 3-dof FEM row against 6).
// rs = sum |l_ij| then sum |u_ij| is added in storage order from shuffled values (every lane forms the same sum), the pivot's lane
// tests |w_i| <= zeropivot rs and stores 1 / w_i, or records the row with an ordinary atomicMin on its block's word (and leaves
// |w_i| in the pivot's slot for the report).  Rows that see their block's word set skip their work (read by lane 0, broadcast: a
// row's lanes always decide together).  No workgroup waits for another: level order comes from the launch boundaries alone.
// When several rows of one block fail, the word names the smallest failing row among those that RAN: a failing row of a smaller
// index but a later level is skipped once the word is set, so the row reported may differ from the sequential loop's first failing
// row (the message of error 71 only; shift counts and the factor's bits do not depend on it, the whole block runs again).
#include "common.hpp"
#include <limits.h>
#include <math.h>
#include <vector>

template <int W>
__device__ __forceinline__ int ilu0_chunk_find(int uc, int c) {   // position of the first chunk entry >= c among the row's W lanes (W - 1 at most)
  int lo = 0;
#pragma unroll
  for (int step = W / 2; step > 0; step >>= 1) {
    const int v = __shfl(uc, lo + step - 1, W);
    if (v < c) lo += step;
  }
  return lo;
}

template <int W>
__global__ __launch_bounds__(MI355X_BLOCK) void ilu0_factor_level_kernel(int nrows, const int *__restrict__ rows,
                                                                        const int *__restrict__ ai, const int *__restrict__ aj,
                                                                        const double *__restrict__ aa, const int *__restrict__ bi,
                                                                        const int *__restrict__ bj, const int *__restrict__ bdiag,
                                                                        double *ba, const int *__restrict__ blkof,
                                                                        const int *__restrict__ pending, const double *__restrict__ shift,
                                                                        int *flag, double zeropivot) {
  const int g = (int)((blockIdx.x * (unsigned)MI355X_BLOCK + threadIdx.x) / W), l = (int)(threadIdx.x % W);
  if (g >= nrows) return;                                     // (a row's lanes leave together)
  const int i = rows[g];
  const int b = blkof[i];
  int skip = 0;
  if (l == 0) skip = !pending[b] || __atomic_load_n(&flag[b], __ATOMIC_RELAXED) != INT_MAX;
  if (__shfl(skip, 0, W)) return;
  const int a0 = ai[i], rowlen = ai[i + 1] - a0, bL = bi[i], nzl = bi[i + 1] - bL, bU = bdiag[i + 1] + 1, bD = bdiag[i];
  if (rowlen <= W) {   // ---- the row in registers
    int c = INT_MAX; double w = 0.0;
    if (l < rowlen) { c = aj[a0 + l]; w = aa[a0 + l]; }
    if (l == nzl) w += shift[b];
    int us = 0, un = 0; double piv = 0.0;                      // strict-upper part and inverted pivot of the row this lane's L column names
    if (l < nzl) { const int d1 = bdiag[c + 1], d0 = bdiag[c]; us = d1 + 1; un = d0 - d1 - 1; piv = ba[d0]; }
    for (int kk = 0; kk < nzl; ++kk) {
      const double wk = __shfl(w, kk, W), pk = __shfl(piv, kk, W);
      const int s = __shfl(us, kk, W), nu = __shfl(un, kk, W);
      if (wk != 0.0) {
        const double m = wk * pk;
        if (l == kk) w = m;
        for (int t0 = 0; t0 < nu; t0 += W) {
          int uc = INT_MAX; double uv = 0.0;
          if (t0 + l < nu) { uc = bj[s + t0 + l]; uv = ba[s + t0 + l]; }
          const int at = ilu0_chunk_find<W>(uc, c);
          const int vc = __shfl(uc, at, W); const double vv = __shfl(uv, at, W);
          if (l > kk && l < rowlen && vc == c) w = w - m * vv;
        }
      }
    }
    double rs = 0.0;
    for (int p = 0; p < rowlen; ++p) { const double v = __shfl(w, p, W); if (p != nzl) rs += fabs(v); }
    if (l < nzl) ba[bL + l] = w;
    else if (l > nzl && l < rowlen) ba[bU + (l - nzl - 1)] = w;
    else if (l == nzl) {
      if (fabs(w) <= zeropivot * rs) { atomicMin(&flag[b], i); ba[bD] = fabs(w); }
      else ba[bD] = 1.0 / w;
    }
    return;
  }
  if constexpr (W == MI355X_WAVE) {   // (narrower W: the host chose it from the widest row, every row fits)
  // ---- a row wider than the wavefront: the work row in its own slots of ba, position p owned by lane p % 64
#define ILU0_SLOT(p) ((p) < nzl ? bL + (p) : ((p) == nzl ? bD : bU + ((p) - nzl - 1)))
  for (int p = l; p < rowlen; p += W) { double v = aa[a0 + p]; if (p == nzl) v += shift[b]; ba[ILU0_SLOT(p)] = v; }
  for (int kk = 0; kk < nzl; ++kk) {
    const int k = aj[a0 + kk], owner = kk % W;
    double mine = 0.0;
    if (l == owner) mine = ba[bL + kk];
    const double wk = __shfl(mine, owner, W);
    if (wk != 0.0) {
      const int d1 = bdiag[k + 1], d0 = bdiag[k], s = d1 + 1, nu = d0 - d1 - 1;
      const double m = wk * ba[d0];
      if (l == owner) ba[bL + kk] = m;
      for (int t0 = 0; t0 < nu; t0 += W) {
        int uc = INT_MAX; double uv = 0.0;
        if (t0 + l < nu) { uc = bj[s + t0 + l]; uv = ba[s + t0 + l]; }
        for (int pb = ((kk + 1) / W) * W; pb < rowlen; pb += W) {
          const int p = pb + l;
          const int c = p < rowlen ? aj[a0 + p] : INT_MAX;
          const int at = ilu0_chunk_find<W>(uc, c);
          const int vc = __shfl(uc, at, W); const double vv = __shfl(uv, at, W);
          if (p > kk && p < rowlen && vc == c) { const int q = ILU0_SLOT(p); ba[q] = ba[q] - m * vv; }
        }
      }
    }
  }
  double rs = 0.0, wd = 0.0;
  for (int pb = 0; pb < rowlen; pb += W) {
    const int p = pb + l;
    const double v = p < rowlen ? ba[ILU0_SLOT(p)] : 0.0;
    const int cnt = rowlen - pb < W ? rowlen - pb : W;
    for (int s = 0; s < cnt; ++s) { const double x = __shfl(v, s, W); if (pb + s != nzl) rs += fabs(x); else wd = x; }
  }
#undef ILU0_SLOT
  if (l == nzl % W) {
    if (fabs(wd) <= zeropivot * rs) { atomicMin(&flag[b], i); ba[bD] = fabs(wd); }
    else ba[bD] = 1.0 / wd;
  }
  }
}

// ---- the same factorisation on a pattern with fill (ILU(k), mi355x_ilu0_factor_create_fill): the factor's row is wider than A's.
// ilu0_factor_fill_level_kernel<W>: the work row is the FACTOR's row (L columns, diagonal, U columns, ascending), position p in
// lane p (registers) or in the row's own slot of ba owned by lane p % 64 (a factor row wider than the wavefront).  Its starting
// value is A's entry at that column or +0.0 where A stores none: A's row is loaded cooperatively, W entries at a time, and every
// lane looks its own column up in the chunk (ilu0_chunk_find) -- no map array, no zero-and-scatter pass over ba, and a block that
// runs again after a failed pass starts from A's values and zeros, never from the fill values of the pass before.  A's row may be
// wider or narrower than W whatever the factor's row is.  From there on the arithmetic is the ILU(0) kernel's over the factor's
// columns: a fill entry of L that nothing has touched is == 0.0 and skipped like a stored zero.
template <int W>
__global__ __launch_bounds__(MI355X_BLOCK) void ilu0_factor_fill_level_kernel(int nrows, const int *__restrict__ rows,
                                                                             const int *__restrict__ ai, const int *__restrict__ aj,
                                                                             const double *__restrict__ aa, const int *__restrict__ bi,
                                                                             const int *__restrict__ bj, const int *__restrict__ bdiag,
                                                                             double *ba, const int *__restrict__ blkof,
                                                                             const int *__restrict__ pending, const double *__restrict__ shift,
                                                                             int *flag, double zeropivot) {
  const int g = (int)((blockIdx.x * (unsigned)MI355X_BLOCK + threadIdx.x) / W), l = (int)(threadIdx.x % W);
  if (g >= nrows) return;                                     // (a row's lanes leave together)
  const int i = rows[g];
  const int b = blkof[i];
  int skip = 0;
  if (l == 0) skip = !pending[b] || __atomic_load_n(&flag[b], __ATOMIC_RELAXED) != INT_MAX;
  if (__shfl(skip, 0, W)) return;
  const int a0 = ai[i], alen = ai[i + 1] - a0, bL = bi[i], nzl = bi[i + 1] - bL, bU = bdiag[i + 1] + 1, bD = bdiag[i];
  const int rowlen = nzl + 1 + (bD - bU);                      // the factor's row
#define ILU0_SLOT(p) ((p) < nzl ? bL + (p) : ((p) == nzl ? bD : bU + ((p) - nzl - 1)))
  if (rowlen <= W) {   // ---- the row in registers
    int c = INT_MAX; double w = 0.0;
    if (l < rowlen) c = bj[ILU0_SLOT(l)];
    for (int t0 = 0; t0 < alen; t0 += W) {                      // A's entry at this lane's column, where there is one
      int ac = INT_MAX; double av = 0.0;
      if (t0 + l < alen) { ac = aj[a0 + t0 + l]; av = aa[a0 + t0 + l]; }
      const int at = ilu0_chunk_find<W>(ac, c);
      const int vc = __shfl(ac, at, W); const double vv = __shfl(av, at, W);
      if (l < rowlen && vc == c) w = vv;
    }
    if (l == nzl) w += shift[b];
    int us = 0, un = 0; double piv = 0.0;                      // strict-upper part and inverted pivot of the row this lane's L column names
    if (l < nzl) { const int d1 = bdiag[c + 1], d0 = bdiag[c]; us = d1 + 1; un = d0 - d1 - 1; piv = ba[d0]; }
    for (int kk = 0; kk < nzl; ++kk) {
      const double wk = __shfl(w, kk, W), pk = __shfl(piv, kk, W);
      const int s = __shfl(us, kk, W), nu = __shfl(un, kk, W);
      if (wk != 0.0) {
        const double m = wk * pk;
        if (l == kk) w = m;
        for (int t0 = 0; t0 < nu; t0 += W) {
          int uc = INT_MAX; double uv = 0.0;
          if (t0 + l < nu) { uc = bj[s + t0 + l]; uv = ba[s + t0 + l]; }
          const int at = ilu0_chunk_find<W>(uc, c);
          const int vc = __shfl(uc, at, W); const double vv = __shfl(uv, at, W);
          if (l > kk && l < rowlen && vc == c) w = w - m * vv;
        }
      }
    }
    double rs = 0.0;
    for (int p = 0; p < rowlen; ++p) { const double v = __shfl(w, p, W); if (p != nzl) rs += fabs(v); }
    if (l < nzl) ba[bL + l] = w;
    else if (l > nzl && l < rowlen) ba[bU + (l - nzl - 1)] = w;
    else if (l == nzl) {
      if (fabs(w) <= zeropivot * rs) { atomicMin(&flag[b], i); ba[bD] = fabs(w); }
      else ba[bD] = 1.0 / w;
    }
    return;
  }
  if constexpr (W == MI355X_WAVE) {   // (narrower W: the host chose it from the widest factor row, every row fits)
  // ---- a factor row wider than the wavefront: the work row in its own slots of ba, position p owned by lane p % 64, which
  // initialises it from the match against A and is the only lane that ever reads or writes it
  for (int pb = 0; pb < rowlen; pb += W) {
    const int p = pb + l;
    const int c = p < rowlen ? bj[ILU0_SLOT(p)] : INT_MAX;
    double v = 0.0;
    for (int t0 = 0; t0 < alen; t0 += W) {
      int ac = INT_MAX; double av = 0.0;
      if (t0 + l < alen) { ac = aj[a0 + t0 + l]; av = aa[a0 + t0 + l]; }
      const int at = ilu0_chunk_find<W>(ac, c);
      const int vc = __shfl(ac, at, W); const double vv = __shfl(av, at, W);
      if (p < rowlen && vc == c) v = vv;
    }
    if (p == nzl) v += shift[b];
    if (p < rowlen) ba[ILU0_SLOT(p)] = v;
  }
  for (int kk = 0; kk < nzl; ++kk) {
    const int k = bj[bL + kk], owner = kk % W;
    double mine = 0.0;
    if (l == owner) mine = ba[bL + kk];
    const double wk = __shfl(mine, owner, W);
    if (wk != 0.0) {
      const int d1 = bdiag[k + 1], d0 = bdiag[k], s = d1 + 1, nu = d0 - d1 - 1;
      const double m = wk * ba[d0];
      if (l == owner) ba[bL + kk] = m;
      for (int t0 = 0; t0 < nu; t0 += W) {
        int uc = INT_MAX; double uv = 0.0;
        if (t0 + l < nu) { uc = bj[s + t0 + l]; uv = ba[s + t0 + l]; }
        for (int pb = ((kk + 1) / W) * W; pb < rowlen; pb += W) {
          const int p = pb + l;
          const int c = p < rowlen ? bj[ILU0_SLOT(p)] : INT_MAX;
          const int at = ilu0_chunk_find<W>(uc, c);
          const int vc = __shfl(uc, at, W); const double vv = __shfl(uv, at, W);
          if (p > kk && p < rowlen && vc == c) { const int q = ILU0_SLOT(p); ba[q] = ba[q] - m * vv; }
        }
      }
    }
  }
  double rs = 0.0, wd = 0.0;
  for (int pb = 0; pb < rowlen; pb += W) {
    const int p = pb + l;
    const double v = p < rowlen ? ba[ILU0_SLOT(p)] : 0.0;
    const int cnt = rowlen - pb < W ? rowlen - pb : W;
    for (int s = 0; s < cnt; ++s) { const double x = __shfl(v, s, W); if (pb + s != nzl) rs += fabs(x); else wd = x; }
  }
  if (l == nzl % W) {
    if (fabs(wd) <= zeropivot * rs) { atomicMin(&flag[b], i); ba[bD] = fabs(wd); }
    else ba[bD] = 1.0 / wd;
  }
  }
#undef ILU0_SLOT
}

// the sweep form's arrays from the factor (host/ilu.c, -pc_factor_hipmi355x_trisolve sweeps:<k>): the negated strict triangles as
// CSR and the inverted pivots
__global__ __launch_bounds__(MI355X_BLOCK) void ilu0_negate_kernel(size_t n, const double *__restrict__ in, double *__restrict__ out) {
  for (size_t q = blockIdx.x * (size_t)MI355X_BLOCK + threadIdx.x; q < n; q += (size_t)gridDim.x * MI355X_BLOCK) out[q] = -in[q];
}
// (lanes consecutive threads per row, the matrix's lanes-per-row: a row's entries are read and written side by side)
__global__ __launch_bounds__(MI355X_BLOCK) void ilu0_upper_to_csr_kernel(int n, int lanes, const int *__restrict__ bdiag, const int *__restrict__ iU,
                                                                        const double *__restrict__ ba, double *__restrict__ aU,
                                                                        double *__restrict__ dinv) {
  const size_t t = blockIdx.x * (size_t)MI355X_BLOCK + threadIdx.x;
  const int l = (int)(t % (size_t)lanes);
  if (t / (size_t)lanes >= (size_t)n) return;
  const int i = (int)(t / (size_t)lanes);
  const int s = bdiag[i + 1] + 1, nu = bdiag[i] - bdiag[i + 1] - 1, o = iU[i];
  for (int q = l; q < nu; q += lanes) aU[o + q] = -ba[s + q];
  if (l == 0) dinv[i] = ba[s + nu];
}

struct mi355x_ilu0_factor_s {
  int n = 0, nz = 0, nzL = 0, nlev = 0, nblk = 1, lanes = 1;
  bool fill = false;                                          // made by _create_fill: A's rows are subsets of the factor's, the fill kernel runs
  int *d_bi = nullptr, *d_bj = nullptr, *d_bdiag = nullptr, *d_rows = nullptr, *d_blkof = nullptr, *d_flag = nullptr, *d_pending = nullptr;
  double *d_shift = nullptr;
  std::vector<int> levptr, pending, flag;
  ~mi355x_ilu0_factor_s() {
    void *dev[] = {d_bi, d_bj, d_bdiag, d_rows, d_blkof, d_flag, d_pending, d_shift};
    for (void *p : dev) if (p) (void)hipFree(p);
  }
};

template <int W>
static void ilu0_launch_level(hipStream_t st, int nrows, const int *rows, const int *ai, const int *aj, const double *aa,
                              const mi355x_ilu0_factor_s *c, double *ba, double zeropivot) {
  const long threads = (long)nrows * W;
  hipLaunchKernelGGL(ilu0_factor_level_kernel<W>, dim3((unsigned)((threads + MI355X_BLOCK - 1) / MI355X_BLOCK)), dim3(MI355X_BLOCK), 0, st,
                     nrows, rows, ai, aj, aa, c->d_bi, c->d_bj, c->d_bdiag, ba, c->d_blkof, c->d_pending, c->d_shift, c->d_flag, zeropivot);
}
template <int W>
static void ilu0_launch_fill_level(hipStream_t st, int nrows, const int *rows, const int *ai, const int *aj, const double *aa,
                                   const mi355x_ilu0_factor_s *c, double *ba, double zeropivot) {
  const long threads = (long)nrows * W;
  hipLaunchKernelGGL(ilu0_factor_fill_level_kernel<W>, dim3((unsigned)((threads + MI355X_BLOCK - 1) / MI355X_BLOCK)), dim3(MI355X_BLOCK), 0, st,
                     nrows, rows, ai, aj, aa, c->d_bi, c->d_bj, c->d_bdiag, ba, c->d_blkof, c->d_pending, c->d_shift, c->d_flag, zeropivot);
}
static int ilu0_launch_fill_chain(hipStream_t st, const mi355x_ilu0_factor_s *c, const int *ai, const int *aj, const double *aa, double *ba, double zeropivot) {
  for (int lv = 0; lv < c->nlev; ++lv) {
    const int nrows = c->levptr[lv + 1] - c->levptr[lv];
    const int *rows = c->d_rows + c->levptr[lv];
    if (nrows <= 0) continue;
    switch (c->lanes) {
      case 1: ilu0_launch_fill_level<1>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 2: ilu0_launch_fill_level<2>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 4: ilu0_launch_fill_level<4>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 8: ilu0_launch_fill_level<8>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 16: ilu0_launch_fill_level<16>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 32: ilu0_launch_fill_level<32>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      default: ilu0_launch_fill_level<64>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
    }
    MI355X_LAUNCH_CHECK();
  }
  return 0;
}
static int ilu0_launch_chain(hipStream_t st, const mi355x_ilu0_factor_s *c, const int *ai, const int *aj, const double *aa, double *ba, double zeropivot) {
  for (int lv = 0; lv < c->nlev; ++lv) {
    const int nrows = c->levptr[lv + 1] - c->levptr[lv];
    const int *rows = c->d_rows + c->levptr[lv];
    if (nrows <= 0) continue;
    switch (c->lanes) {
      case 1: ilu0_launch_level<1>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 2: ilu0_launch_level<2>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 4: ilu0_launch_level<4>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 8: ilu0_launch_level<8>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 16: ilu0_launch_level<16>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      case 32: ilu0_launch_level<32>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
      default: ilu0_launch_level<64>(st, nrows, rows, ai, aj, aa, c, ba, zeropivot); break;
    }
    MI355X_LAUNCH_CHECK();
  }
  return 0;
}

// the context of one pattern.  ai / aj (host, both or neither): A's pattern where the factor's has fill (_create_fill)
static int ilu0_factor_make(mi355x_handle_t h, int n, const int *ai, const int *aj, const int *bi, const int *bj, const int *bdiag, int nlev,
                            const int *levptr, const int *rows, int nblk, const int *blk, mi355x_ilu0_factor_t *ctx) {
  if (!ctx) return (int)hipErrorInvalidValue;
  *ctx = nullptr;
  if (n < 0 || nlev < 0 || (n > 0 && (!bi || !bj || !bdiag || !levptr || !rows || nlev < 1)) || (nblk > 1 && !blk)) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    std::unique_ptr<mi355x_ilu0_factor_s> c(new mi355x_ilu0_factor_s);   // (its destructor frees whatever was allocated when a step below fails)
    c->n = n; c->nlev = n ? nlev : 0; c->nblk = nblk > 1 ? nblk : 1; c->fill = ai != nullptr;
    c->nz = n ? bdiag[0] + 1 : 0; c->nzL = n ? bi[n] : 0;
    // the layout the kernel indexes by, checked before anything runs on it: L columns below the row, U columns above it and inside
    // the matrix, every row listed once, level by level
    int widest = 1;
    if (n) {
      if (bi[0] != 0 || bdiag[n] != bi[n] - 1 || levptr[0] != 0 || levptr[c->nlev] != n) return (int)hipErrorInvalidValue;
      std::vector<char> seen((size_t)n, 0);
      for (int lv = 0; lv < c->nlev; ++lv) if (levptr[lv + 1] < levptr[lv]) return (int)hipErrorInvalidValue;
      for (int t = 0; t < n; ++t) { const int r = rows[t]; if (r < 0 || r >= n || seen[r]) return (int)hipErrorInvalidValue; seen[r] = 1; }
      for (int i = 0; i < n; ++i) {
        const int nzl = bi[i + 1] - bi[i], nzu = bdiag[i] - bdiag[i + 1] - 1;
        if (nzl < 0 || nzu < 0 || bdiag[i] >= c->nz || bj[bdiag[i]] != i) return (int)hipErrorInvalidValue;
        for (int q = bi[i]; q < bi[i + 1]; ++q) if (bj[q] < 0 || bj[q] >= i || (q > bi[i] && bj[q] <= bj[q - 1])) return (int)hipErrorInvalidValue;
        for (int q = bdiag[i + 1] + 1; q < bdiag[i]; ++q) if (bj[q] <= i || bj[q] >= n || (q > bdiag[i + 1] + 1 && bj[q] <= bj[q - 1])) return (int)hipErrorInvalidValue;
        if (nzl + 1 + nzu > widest) widest = nzl + 1 + nzu;
      }
      // with fill: every row of A a sorted subset of its factor row (the kernel finds a factor column in A's row by a search in
      // sorted chunks, and an entry of A the factor lacks would be dropped without a word)
      if (ai) {
        if (ai[0] != 0) return (int)hipErrorInvalidValue;
        for (int i = 0; i < n; ++i) {
          if (ai[i + 1] < ai[i]) return (int)hipErrorInvalidValue;
          const int nzl = bi[i + 1] - bi[i], u0 = bdiag[i + 1] + 1, len = nzl + 1 + (bdiag[i] - u0);
          auto col_at = [&](int p) { return p < nzl ? bj[bi[i] + p] : (p == nzl ? i : bj[u0 + (p - nzl - 1)]); };   // the factor's row, ascending
          int p = 0;
          for (int t = ai[i]; t < ai[i + 1]; ++t) {
            if (t > ai[i] && aj[t] <= aj[t - 1]) return (int)hipErrorInvalidValue;
            while (p < len && col_at(p) < aj[t]) ++p;
            if (p == len || col_at(p) != aj[t]) return (int)hipErrorInvalidValue;
          }
        }
      }
    }
    c->lanes = 1;
    while (c->lanes < widest && c->lanes < MI355X_WAVE) c->lanes *= 2;
    if (n) c->levptr.assign(levptr, levptr + c->nlev + 1);
    else c->levptr.assign(1, 0);
    std::vector<int> blkof((size_t)(n > 0 ? n : 1), 0);
    if (nblk > 1) {
      if (blk[0] != 0 || blk[nblk] != n) return (int)hipErrorInvalidValue;
      for (int b = 0; b < nblk; ++b) if (blk[b + 1] < blk[b]) return (int)hipErrorInvalidValue;   // (every range inside [0, n] before blkof is written)
      for (int b = 0; b < nblk; ++b) for (int i = blk[b]; i < blk[b + 1]; ++i) blkof[i] = b;
    }
    c->pending.assign((size_t)c->nblk, 1);
    c->flag.assign((size_t)c->nblk, INT_MAX);
    const size_t ni = sizeof(int) * (size_t)(n + 1), nj = sizeof(int) * (size_t)(c->nz + 1), nn = sizeof(int) * (size_t)(n > 0 ? n : 1), nb = (size_t)c->nblk;
    MI355X_TRY(hipMalloc((void **)&c->d_bi, ni));
    MI355X_TRY(hipMalloc((void **)&c->d_bj, nj));
    MI355X_TRY(hipMalloc((void **)&c->d_bdiag, ni));
    MI355X_TRY(hipMalloc((void **)&c->d_rows, nn));
    MI355X_TRY(hipMalloc((void **)&c->d_blkof, nn));
    MI355X_TRY(hipMalloc((void **)&c->d_flag, sizeof(int) * nb));
    MI355X_TRY(hipMalloc((void **)&c->d_pending, sizeof(int) * nb));
    MI355X_TRY(hipMalloc((void **)&c->d_shift, sizeof(double) * nb));
    if (n) {
      MI355X_TRY(hipMemcpyAsync(c->d_bi, bi, ni, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(c->d_bj, bj, sizeof(int) * (size_t)c->nz, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(c->d_bdiag, bdiag, ni, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(c->d_rows, rows, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(c->d_blkof, blkof.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    }
    MI355X_TRY(hipStreamSynchronize(h->stream));               // (the host arrays are the caller's, blkof goes away here)
    *ctx = c.release();
    return 0;
  });
}

extern "C" {

int mi355x_ilu0_factor_create(mi355x_handle_t h, int n, const int *bi, const int *bj, const int *bdiag, int nlev, const int *levptr,
                              const int *rows, int nblk, const int *blk, mi355x_ilu0_factor_t *ctx) {
  return ilu0_factor_make(h, n, nullptr, nullptr, bi, bj, bdiag, nlev, levptr, rows, nblk, blk, ctx);
}

int mi355x_ilu0_factor_create_fill(mi355x_handle_t h, int n, const int *ai_host, const int *aj_host, const int *bi, const int *bj, const int *bdiag,
                                   int nlev, const int *levptr, const int *rows, int nblk, const int *blk, mi355x_ilu0_factor_t *ctx) {
  static const int none[1] = {0};                             // (n = 0: a context of the fill kind whatever the caller passed)
  if (ctx) *ctx = nullptr;
  if (n > 0 && (!ai_host || (ai_host[n] > 0 && !aj_host))) return (int)hipErrorInvalidValue;
  if (n <= 0 || !ai_host) { ai_host = none; aj_host = none; }
  if (!aj_host) aj_host = none;
  return ilu0_factor_make(h, n, ai_host, aj_host, bi, bj, bdiag, nlev, levptr, rows, nblk, blk, ctx);
}

// Symbolic ILU(k), natural ordering (MatILUFactorSymbolic_SeqAIJ): host arrays, no device call.  A stored a_ij has level 0.  Row i
// starts as the sorted list of A's columns; for every list column k < i in ascending order -- fill that entered earlier included --
// incr = lev(i,k) + 1, and every strict-upper entry (k,j) of row k with lev(k,j) + incr <= levels enters the list with that level
// (an entry already there keeps the smaller level).  The list is a linked list over the columns (next[], head in slot n): U(k) is
// ascending and all of it lies behind k, so one walk from k merges it.
// ONE thread on purpose: row i reads the levels of the U rows before it, the rows depend on each other in sequence.
int mi355x_iluk_symbolic_host(int n, const int *ai, const int *aj, int levels, int *bi, int *bdiag, int *bj, int *bjlev, int *bad_row) {
  if (bad_row) *bad_row = -1;
  if (n < 0 || levels < 0 || !bi || !bdiag || (n > 0 && !ai)) return (int)hipErrorInvalidValue;
  if (n > 0 && ai[n] > 0 && !aj) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    const bool fillin = bj != nullptr;                         // second call: bi / bdiag are the first call's
    std::vector<int> next((size_t)n + 1), lv((size_t)(n > 0 ? n : 1)), uptr((size_t)n + 1, 0), ucol, ulev, nzl((size_t)(n > 0 ? n : 1)), nzu((size_t)(n > 0 ? n : 1));
    if (n > 0) { ucol.reserve((size_t)ai[n]); ulev.reserve((size_t)ai[n]); }
    for (int i = 0; i < n; ++i) {
      const int a0 = ai[i], a1 = ai[i + 1];
      bool diag = false;
      if (bad_row) *bad_row = i;
      if (a1 <= a0) return (int)hipErrorInvalidValue;            // an empty row
      for (int q = a0; q < a1; ++q) {
        if (aj[q] < 0 || aj[q] >= n || (q > a0 && aj[q] <= aj[q - 1])) return (int)hipErrorInvalidValue;   // unsorted, or outside the matrix
        diag = diag || aj[q] == i;
      }
      if (!diag) return (int)hipErrorInvalidValue;               // a missing diagonal
      int prev = n;
      for (int q = a0; q < a1; ++q) { next[(size_t)prev] = aj[q]; lv[(size_t)aj[q]] = 0; prev = aj[q]; }
      next[(size_t)prev] = n;
      for (int k = next[(size_t)n]; k < i; k = next[(size_t)k]) {
        const int incr = lv[(size_t)k] + 1;
        if (incr > levels) continue;                             // (no entry of row k can come in: levels are >= 0)
        int at = k;
        for (int q = uptr[(size_t)k]; q < uptr[(size_t)k + 1]; ++q) {
          const int j = ucol[(size_t)q], nl = ulev[(size_t)q] + incr;
          if (nl > levels) continue;
          while (next[(size_t)at] < j) at = next[(size_t)at];
          if (next[(size_t)at] == j) { if (lv[(size_t)j] > nl) lv[(size_t)j] = nl; }
          else { next[(size_t)j] = next[(size_t)at]; next[(size_t)at] = j; lv[(size_t)j] = nl; }
          at = j;
        }
      }
      int cl = 0, cu = 0;
      for (int k = next[(size_t)n]; k < n; k = next[(size_t)k]) {
        if (k < i) { if (fillin) { if (cl >= bi[i + 1] - bi[i]) return (int)hipErrorInvalidValue; bj[bi[i] + cl] = k; if (bjlev) bjlev[bi[i] + cl] = lv[(size_t)k]; } cl++; }
        else if (k > i) {
          if (fillin) { if (cu >= bdiag[i] - bdiag[i + 1] - 1) return (int)hipErrorInvalidValue; bj[bdiag[i + 1] + 1 + cu] = k; if (bjlev) bjlev[bdiag[i + 1] + 1 + cu] = lv[(size_t)k]; }
          ucol.push_back(k); ulev.push_back(lv[(size_t)k]); cu++;
        }
      }
      uptr[(size_t)i + 1] = (int)ucol.size();
      if (ucol.size() > (size_t)2147483000) return (int)hipErrorInvalidValue;   // (32-bit offsets)
      if (fillin) {
        if (cl != bi[i + 1] - bi[i] || cu != bdiag[i] - bdiag[i + 1] - 1) return (int)hipErrorInvalidValue;   // not the first call's arrays
        bj[bdiag[i]] = i; if (bjlev) bjlev[bdiag[i]] = 0;
      }
      nzl[(size_t)i] = cl; nzu[(size_t)i] = cu;
    }
    if (bad_row) *bad_row = -1;
    if (!fillin) {
      long total = 0;
      for (int i = 0; i < n; ++i) total += (long)nzl[(size_t)i] + nzu[(size_t)i] + 1;
      if (total > 2147483000L) return (int)hipErrorInvalidValue;
      bi[0] = 0;
      for (int i = 0; i < n; ++i) bi[i + 1] = bi[i] + nzl[(size_t)i];
      bdiag[n] = bi[n] - 1;
      for (int i = n - 1; i >= 0; --i) bdiag[i] = bdiag[i + 1] + nzu[(size_t)i] + 1;
    }
    return 0;
  });
}

int mi355x_ilu0_factor_destroy(mi355x_ilu0_factor_t ctx) {
  delete ctx;
  return 0;
}

int mi355x_ilu0_factor_reset(mi355x_ilu0_factor_t ctx) {
  if (!ctx) return (int)hipErrorInvalidValue;
  for (auto &p : ctx->pending) p = 1;
  return 0;
}

int mi355x_ilu0_factor_info(mi355x_ilu0_factor_t ctx, int *lanes, int *nlev) {
  if (!ctx) return (int)hipErrorInvalidValue;
  if (lanes) *lanes = ctx->lanes;
  if (nlev) *nlev = ctx->nlev;
  return 0;
}

int mi355x_ilu0_factor_arrays(mi355x_ilu0_factor_t ctx, const int **bi, const int **bj, const int **bdiag, const int **rows) {
  if (!ctx) return (int)hipErrorInvalidValue;
  if (bi) *bi = ctx->d_bi;
  if (bj) *bj = ctx->d_bj;
  if (bdiag) *bdiag = ctx->d_bdiag;
  if (rows) *rows = ctx->d_rows;
  return 0;
}

int mi355x_ilu0_factor_run(mi355x_handle_t h, mi355x_ilu0_factor_t c, const int *ai, const int *aj, const double *aa, double zeropivot,
                           const double *shift_per_block, double *ba, int *failed_row, double *failed_abs) {
  if (!c || !failed_row || !shift_per_block) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    const size_t nb = (size_t)c->nblk;
    for (size_t b = 0; b < nb; ++b) { failed_row[b] = -1; if (failed_abs) failed_abs[b] = 0.0; }
    if (!c->n) { for (auto &p : c->pending) p = 0; return 0; }
    if (!ai || !aj || !aa || !ba) return (int)hipErrorInvalidValue;
    for (auto &f : c->flag) f = INT_MAX;
    MI355X_TRY(hipMemcpyAsync(c->d_pending, c->pending.data(), sizeof(int) * nb, hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipMemcpyAsync(c->d_flag, c->flag.data(), sizeof(int) * nb, hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipMemcpyAsync(c->d_shift, shift_per_block, sizeof(double) * nb, hipMemcpyHostToDevice, h->stream));
    // Plain launches, one per level.  Replaying the chain from a graph was measured and gains nothing (P7(256), 766 levels: 8.90 ms
    // against 8.85 ms; FEM stand-in, 6432 levels: 603.1 ms both ways, profiles/ilu_device_factor_graph_trial.log): a level costs
    // 12-94 us of dependent loads inside its rows, the launches are queued well ahead of the kernels.
    { const int rc = c->fill ? ilu0_launch_fill_chain(h->stream, c, ai, aj, aa, ba, zeropivot) : ilu0_launch_chain(h->stream, c, ai, aj, aa, ba, zeropivot);
      if (rc) return rc; }
    MI355X_TRY(hipMemcpyAsync(c->flag.data(), c->d_flag, sizeof(int) * nb, hipMemcpyDeviceToHost, h->stream));
    MI355X_TRY(hipStreamSynchronize(h->stream));               // the pass's one host wait
    int nfailed = 0;
    for (size_t b = 0; b < nb; ++b) {
      if (!c->pending[b]) continue;
      if (c->flag[b] != INT_MAX) { failed_row[b] = c->flag[b]; nfailed++; }
      else c->pending[b] = 0;
    }
    if (nfailed && failed_abs) {                               // (the failing pivot's lane left |w_i| in the pivot's slot)
      std::vector<int> bd((size_t)c->nblk, 0);
      for (size_t b = 0; b < nb; ++b) if (failed_row[b] >= 0) MI355X_TRY(hipMemcpyAsync(&bd[b], c->d_bdiag + failed_row[b], sizeof(int), hipMemcpyDeviceToHost, h->stream));
      MI355X_TRY(hipStreamSynchronize(h->stream));
      for (size_t b = 0; b < nb; ++b) if (failed_row[b] >= 0) MI355X_TRY(hipMemcpyAsync(&failed_abs[b], ba + bd[b], sizeof(double), hipMemcpyDeviceToHost, h->stream));
      MI355X_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
  });
}

int mi355x_ilu0_factor_to_sweeps(mi355x_handle_t h, mi355x_ilu0_factor_t c, const int *iU, const double *ba, double *aL, double *aU, double *dinv) {
  if (!c) return (int)hipErrorInvalidValue;
  if (!c->n) return 0;
  if (!iU || !ba || !aL || !aU || !dinv) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    const int nzL = c->nzL;
    if (nzL > 0) {
      hipLaunchKernelGGL(ilu0_negate_kernel, dim3(mi355x_grid_for((size_t)nzL, 4)), dim3(MI355X_BLOCK), 0, h->stream, (size_t)nzL, ba, aL);
      MI355X_LAUNCH_CHECK();
    }
    const size_t threads = (size_t)c->n * (size_t)c->lanes;
    hipLaunchKernelGGL(ilu0_upper_to_csr_kernel, dim3((unsigned)((threads + MI355X_BLOCK - 1) / MI355X_BLOCK)), dim3(MI355X_BLOCK), 0, h->stream, c->n, c->lanes, c->d_bdiag, iU, ba, aU, dinv);
    MI355X_LAUNCH_CHECK();
    return 0;
  });
}

}  // extern "C"
