/* In-place inverse of a small dense block by LINPACK dgefa + dgedi, the algorithm of PetscKernel_A_gets_inverse_A_N (dgefa.c,
 * dgefa2.c .. dgefa7.c, dgedi.c): what MatInvertBlockDiagonal_SeqBAIJ (baij.c:13-160) and the diagonal blocks of
 * MatLUFactorNumeric_SeqBAIJ_N (baijfact.c) run.  One definition for its two users: PCPBJACOBI's set-up (petsc-dev_amd/host/pbjacobi.c, C)
 * and the block ILU numeric pass of the kernel library (petsc-dev_amd/csrc/bilu.hip, C++).  Host code; every product and every sum is
 * rounded on its own (both users are built with -ffp-contract=off). */
#ifndef MI355X_BLOCK_INVERSE_H
#define MI355X_BLOCK_INVERSE_H
#include <math.h>

/* a: column-major n x n block, n <= 16; returns the 1-based zero-pivot row or 0 */
static inline int mi355x_block_inverse(int n, double *a) {
  int ipvt[16]; double work[16];
#define MI355X_BI_E(i, j) a[(i) + (j) * n]
  for (int k = 0; k + 1 < n; k++) {                       /* dgefa: elimination with partial pivoting, multipliers negated */
    int l = k; double big = fabs(MI355X_BI_E(k, k));
    for (int i = k + 1; i < n; i++) if (fabs(MI355X_BI_E(i, k)) > big) { big = fabs(MI355X_BI_E(i, k)); l = i; }
    ipvt[k] = l;
    if (MI355X_BI_E(l, k) == 0.0) return k + 1;
    if (l != k) { double t = MI355X_BI_E(l, k); MI355X_BI_E(l, k) = MI355X_BI_E(k, k); MI355X_BI_E(k, k) = t; }
    const double m = -1. / MI355X_BI_E(k, k);
    for (int i = k + 1; i < n; i++) MI355X_BI_E(i, k) *= m;
    for (int j = k + 1; j < n; j++) {
      const double t = MI355X_BI_E(l, j);
      if (l != k) { MI355X_BI_E(l, j) = MI355X_BI_E(k, j); MI355X_BI_E(k, j) = t; }
      for (int i = k + 1; i < n; i++) MI355X_BI_E(i, j) += t * MI355X_BI_E(i, k);
    }
  }
  ipvt[n - 1] = n - 1;
  if (MI355X_BI_E(n - 1, n - 1) == 0.0) return n;
  for (int k = 0; k < n; k++) {                           /* dgedi: inverse(U) ... */
    MI355X_BI_E(k, k) = 1.0 / MI355X_BI_E(k, k);
    const double t0 = -MI355X_BI_E(k, k);
    for (int i = 0; i < k; i++) MI355X_BI_E(i, k) *= t0;
    for (int j = k + 1; j < n; j++) {
      const double t = MI355X_BI_E(k, j);
      MI355X_BI_E(k, j) = 0.0;
      for (int i = 0; i <= k; i++) MI355X_BI_E(i, j) += t * MI355X_BI_E(i, k);
    }
  }
  for (int k = n - 2; k >= 0; k--) {                      /* ... times inverse(L), interchanges undone */
    for (int i = k + 1; i < n; i++) { work[i] = MI355X_BI_E(i, k); MI355X_BI_E(i, k) = 0.0; }
    for (int j = k + 1; j < n; j++) { const double t = work[j]; for (int i = 0; i < n; i++) MI355X_BI_E(i, k) += t * MI355X_BI_E(i, j); }
    const int l = ipvt[k];
    if (l != k) for (int i = 0; i < n; i++) { const double t = MI355X_BI_E(i, k); MI355X_BI_E(i, k) = MI355X_BI_E(i, l); MI355X_BI_E(i, l) = t; }
  }
#undef MI355X_BI_E
  return 0;
}
#endif
