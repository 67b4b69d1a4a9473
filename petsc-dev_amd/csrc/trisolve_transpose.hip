// Transposed triangular solves for the ILU(k) factors: MatSolveTranspose_SeqAIJ (reference src/mat/impls/aij/seq/aijfact.c) with the
// natural ordering, on the factor layout of aijfact.c:1628-1700 (L rows forward from bi, U rows stored from the last row backwards,
// each followed by its INVERTED diagonal at bdiag[i]).
//
// The reference scatters: row i of U^T's forward solve scales t[i] by the inverted diagonal and subtracts s * u(i,j) from every t[j]
// its strict row names, i ascending; then row i of L^T's backward solve subtracts t[i] * l(i,j) from every t[j], i descending.  Entry c
// therefore receives its subtractions one after the other in the order of the rows that hold column c -- ascending for U^T, descending
// for L^T -- and that is a GATHER over the transposed triangles whose rows are stored in exactly that order:
//     U^T:  x[c] = (b[c] - u(i1,c) x[i1] - u(i2,c) x[i2] - ...) * dinv[c]      i1 < i2 < ... < c
//     L^T:  x[c] =  x[c] - l(i1,c) x[i1] - l(i2,c) x[i2] - ...                 i1 > i2 > ... > c      (unit diagonal)
// every product rounded before its subtraction (-ffp-contract=off), so x carries the scatter loop's bits without an atomic.
// mi355x_ilut_build_host makes the two transposed patterns (CSR, rows in the order above), the position in ba of every value, and
// the dependency level of every row; the kernels take one level's rows per launch, one lane per row, walking the row in storage order.
// Rows of one level do not read each other and a kernel boundary separates the levels: nothing here waits on anything.
#include "common.hpp"
#include <vector>

// the accumulation both solves share: s - a[q] x[j[q]] over the row's entries in storage order
__device__ __forceinline__ double ilut_row_minus(double s, int q0, int q1, const int *__restrict__ rj, const double *__restrict__ ra,
                                                 const double *x) {
  for (int q = q0; q < q1; ++q) s -= ra[q] * x[rj[q]];
  return s;
}

// SCALED: the first solve (U^T) -- starts from b[c], ends in the product with the inverted diagonal.  Else the second (L^T), in place
// on x with the unit diagonal.  b may be x: row c reads b[c] before it writes x[c] and no other row reads b[c].
template <bool SCALED>
__global__ __launch_bounds__(MI355X_BLOCK) void ilut_level_kernel(int nrows, const int *__restrict__ rows, const int *__restrict__ ri,
                                                                  const int *__restrict__ rj, const double *__restrict__ ra,
                                                                  const double *__restrict__ dinv, const double *b, double *x) {
  const int t = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (t >= nrows) return;
  const int c = rows[t];
  const double s = ilut_row_minus(SCALED ? b[c] : x[c], ri[c], ri[c + 1], rj, ra, x);
  x[c] = SCALED ? s * dinv[c] : s;
}

template <bool SCALED>
static int ilut_launch(mi355x_handle_t h, int nrows, const int *rows, const int *ri, const int *rj, const double *ra, const double *dinv,
                       const double *b, double *x) {
  if (nrows <= 0) return 0;
  hipLaunchKernelGGL((ilut_level_kernel<SCALED>), dim3((nrows + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream,
                     nrows, rows, ri, rj, ra, dinv, b, x);
  MI355X_LAUNCH_CHECK();
  return 0;
}

// the host side: both transposed patterns, their permutations into ba and the row levels; throws (std::vector) -- called under the guard
static int ilut_build(int n, const int *bi, const int *bj, const int *bdiag, int *ti, int *tj, int *tperm, int *si, int *sj, int *sperm,
                      int *levT_first, int *nlev_first, int *levT_second, int *nlev_second) {
  // the layout, before anything is written through it
  if (bi[0] != 0 || bdiag[n] != bi[n] - 1) return (int)hipErrorInvalidValue;
  for (int i = 0; i < n; ++i) {
    if (bi[i + 1] < bi[i] || bdiag[i] <= bdiag[i + 1]) return (int)hipErrorInvalidValue;
    for (int q = bi[i]; q < bi[i + 1]; ++q) if (bj[q] < 0 || bj[q] >= i) return (int)hipErrorInvalidValue;
    for (int q = bdiag[i + 1] + 1; q < bdiag[i]; ++q) if (bj[q] <= i || bj[q] >= n) return (int)hipErrorInvalidValue;
  }
  std::vector<int> next((size_t)n + 1, 0);
  // U^T: counts per column, then the rows i ascending -- every row of U^T ends up with ascending columns
  for (int c = 0; c <= n; ++c) ti[c] = 0;
  for (int i = 0; i < n; ++i) for (int q = bdiag[i + 1] + 1; q < bdiag[i]; ++q) ti[bj[q] + 1]++;
  for (int c = 0; c < n; ++c) ti[c + 1] += ti[c];
  for (int c = 0; c < n; ++c) next[c] = ti[c];
  for (int i = 0; i < n; ++i)
    for (int q = bdiag[i + 1] + 1; q < bdiag[i]; ++q) { const int p = next[bj[q]]++; tj[p] = i; tperm[p] = q; }
  // L^T: the rows i descending -- every row of L^T ends up with descending columns
  for (int c = 0; c <= n; ++c) si[c] = 0;
  for (int i = 0; i < n; ++i) for (int q = bi[i]; q < bi[i + 1]; ++q) si[bj[q] + 1]++;
  for (int c = 0; c < n; ++c) si[c + 1] += si[c];
  for (int c = 0; c < n; ++c) next[c] = si[c];
  for (int i = n - 1; i >= 0; --i)
    for (int q = bi[i]; q < bi[i + 1]; ++q) { const int p = next[bj[q]]++; sj[p] = i; sperm[p] = q; }
  // levels: a row without entries is level 0, else one more than the deepest row it reads.  U^T's rows read smaller rows (forward),
  // L^T's larger ones (backward); every level 0 .. nlev - 1 then holds a row
  int nl = 0;
  for (int c = 0; c < n; ++c) {
    int l = 0;
    for (int q = ti[c]; q < ti[c + 1]; ++q) if (levT_first[tj[q]] + 1 > l) l = levT_first[tj[q]] + 1;
    levT_first[c] = l; if (l + 1 > nl) nl = l + 1;
  }
  *nlev_first = nl;
  nl = 0;
  for (int c = n - 1; c >= 0; --c) {
    int l = 0;
    for (int q = si[c]; q < si[c + 1]; ++q) if (levT_second[sj[q]] + 1 > l) l = levT_second[sj[q]] + 1;
    levT_second[c] = l; if (l + 1 > nl) nl = l + 1;
  }
  *nlev_second = nl;
  return 0;
}

extern "C" {

int mi355x_ilut_first_level(mi355x_handle_t h, int nrows, const int *rows, const int *ti, const int *tj, const double *ta,
                            const double *dinv, const double *b, double *x) {
  return ilut_launch<true>(h, nrows, rows, ti, tj, ta, dinv, b, x);
}

int mi355x_ilut_second_level(mi355x_handle_t h, int nrows, const int *rows, const int *si, const int *sj, const double *sa, double *x) {
  return ilut_launch<false>(h, nrows, rows, si, sj, sa, nullptr, nullptr, x);
}

int mi355x_ilut_build_host(int n, const int *bi, const int *bj, const int *bdiag, int *ti, int *tj, int *tperm, int *si, int *sj,
                           int *sperm, int *levT_first, int *nlev_first, int *levT_second, int *nlev_second) {
  if (n < 0 || !bi || !bdiag || !ti || !si || !nlev_first || !nlev_second) return (int)hipErrorInvalidValue;
  if (n > 0 && (!bj || !levT_first || !levT_second)) return (int)hipErrorInvalidValue;
  if (n > 0 && bi[n] > 0 && (!sj || !sperm)) return (int)hipErrorInvalidValue;
  if (n > 0 && bdiag[0] + 1 - bi[n] - n > 0 && (!tj || !tperm)) return (int)hipErrorInvalidValue;
  return mi355x_guard([&] { return ilut_build(n, bi, bj, bdiag, ti, tj, tperm, si, sj, sperm, levT_first, nlev_first, levT_second, nlev_second); });
}

}  // extern "C"
