// SOR / SSOR point sweeps on a square CSR matrix as it is stored (MatSOR_SeqAIJ, reference src/mat/impls/aij/seq/aij.c:1463-1640;
// the inverted diagonal of MatInvertDiagonal_SeqAIJ, aij.c:1430-1460).  No second copy of the values: the sweeps read the
// matrix's own device arrays, plus every row's diagonal position.
//
// Levels.  lev[i] = 1 + max lev[j] over the j < i with a(i,j) OR a(j,i) stored (0 without such a j): the dependency levels of the
// lower triangle of the pattern of A + A^T.  Every coupled pair j < i therefore has lev[j] < lev[i], whichever of the two entries
// is stored, and rows of one level share no entry.  Run in ascending level order, a row i finds every coupled j < i already
// updated and every coupled j > i not yet -- which is all the sequential loop i = 0 .. m-1 guarantees a row: a forward sweep.
// Run in descending level order it finds every coupled j > i updated and every coupled j < i not yet: the loop i = m-1 .. 0.
// The same strict inequality serves both directions, so ONE level set does.  (The general sweeps read the OLD x[j] of the other
// side, hence the anti-dependency through a(i,j) alone; the lower triangle of A by itself would let row j > i overtake row i.)
//
// Kernels.  One lane per row; the products of a row are subtracted in storage order, product and difference each rounded
// (-ffp-contract=off), so x carries the sequential loop's bits.  One launch per level in stream order; a maximal run of
// consecutive levels of at most MI355X_BLOCK rows each is ONE launch of ONE workgroup that walks the run with __syncthreads()
// between levels.  x and t go through plain pointers (no __restrict__, no scalar loads): what a lane stored before the barrier
// is what every lane of the workgroup loads after it.  No flags, no spinning, no hand-off between workgroups.
#include "common.hpp"
#include <vector>
#include <memory>

enum { SOR_FLAG_FORWARD = 1 | 4, SOR_FLAG_BACKWARD = 2 | 8, SOR_FLAG_ZERO = 16, SOR_FLAG_KNOWN = 1 | 2 | 4 | 8 | 16 };

struct sor_step { int l0, l1, fused; };   // levels [l0, l1): one launch per level (fused == 0) or one launch for the run

struct mi355x_sor_plan_s {
  int m = 0, nlev = 0, fused_levels = 0;
  std::vector<int> levptr;          // host: where each level's rows start, nlev + 1
  std::vector<sor_step> steps;      // ascending
  int *d_rows = nullptr, *d_diag = nullptr, *d_levptr = nullptr;
};

// what every row body starts from: the row's range, split at its diagonal position
struct sor_args {
  const int *__restrict__ ai; const int *__restrict__ aj; const double *__restrict__ aa; const int *__restrict__ diag;
  const double *__restrict__ idiag; const double *__restrict__ mdiag;
  double omega;
  const double *b; double *t; double *x;      // plain: written and read across the barriers of a fused run
};
__device__ __forceinline__ double sor_minus_dot(double sum, int k0, int k1, const sor_args &a) {   // PetscSparseDenseMinusDot, aij.h:337-339
  for (int k = k0; k < k1; ++k) sum -= a.aa[k] * a.x[a.aj[k]];
  return sum;
}
template <int KIND> __device__ __forceinline__ void sor_row(int i, const sor_args &a) {
  const int k0 = a.ai[i], kd = a.diag[i], k1 = a.ai[i + 1];
  if (KIND == MI355X_SOR_ZERO_FORWARD) {
    const double sum = sor_minus_dot(a.b[i], k0, kd, a);
    a.t[i] = sum;
    a.x[i] = sum * a.idiag[i];
  } else if (KIND == MI355X_SOR_ZERO_BACKWARD) {
    const double sum = sor_minus_dot(a.b[i], kd + 1, k1, a);
    a.x[i] = sum * a.idiag[i];
  } else if (KIND == MI355X_SOR_ZERO_BACKWARD_AFTER) {
    const double sum = sor_minus_dot(a.t[i], kd + 1, k1, a);
    a.x[i] = (1. - a.omega) * a.x[i] + sum * a.idiag[i];        // the product with 1 - omega also when it is 0: 0 * Inf is NaN
  } else {                                                       // FORWARD and BACKWARD: one body, the level order is the direction
    const double sum = sor_minus_dot(a.b[i], k0, k1, a);
    a.x[i] = (1. - a.omega) * a.x[i] + (sum + a.mdiag[i] * a.x[i]) * a.idiag[i];
  }
}

template <int KIND> __global__ __launch_bounds__(MI355X_BLOCK) void sor_level_kernel(int nrows, const int *__restrict__ rows, sor_args a) {
  const int t = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (t < nrows) sor_row<KIND>(rows[t], a);
}
// levels [l0, l1), each of at most MI355X_BLOCK rows, by one workgroup.  Every thread reaches every barrier: a thread without a
// row skips the row body only.
template <int KIND> __global__ __launch_bounds__(MI355X_BLOCK) void sor_fused_kernel(int l0, int l1, int descending, const int *__restrict__ levptr,
                                                                                  const int *__restrict__ rows, sor_args a) {
  for (int s = 0; s < l1 - l0; ++s) {
    const int l = descending ? l1 - 1 - s : l0 + s;
    const int r0 = levptr[l], n = levptr[l + 1] - r0;
    if ((int)threadIdx.x < n) sor_row<KIND>(rows[r0 + (int)threadIdx.x], a);
    __syncthreads();
  }
}
__global__ __launch_bounds__(MI355X_BLOCK) void sor_idiag_kernel(int m, const int *__restrict__ diag, const double *__restrict__ aa, double omega,
                                                                double fshift, int plain, double *__restrict__ idiag, double *__restrict__ mdiag) {
  for (size_t i = (size_t)blockIdx.x * MI355X_BLOCK + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * MI355X_BLOCK) {
    const double d = aa[diag[i]];
    mdiag[i] = d;
    idiag[i] = plain ? 1.0 / d : omega / (fshift + d);
  }
}

template <int KIND> static int sor_run(mi355x_handle_t h, const mi355x_sor_plan_s *p, int descending, const sor_args &a) {
  const int ns = (int)p->steps.size();
  for (int q = 0; q < ns; ++q) {
    const sor_step &st = p->steps[(size_t)(descending ? ns - 1 - q : q)];
    if (st.fused) {
      hipLaunchKernelGGL(sor_fused_kernel<KIND>, dim3(1), dim3(MI355X_BLOCK), 0, h->stream, st.l0, st.l1, descending, p->d_levptr, p->d_rows, a);
      MI355X_LAUNCH_CHECK();
      continue;
    }
    for (int s = 0; s < st.l1 - st.l0; ++s) {
      const int l = descending ? st.l1 - 1 - s : st.l0 + s;
      const int r0 = p->levptr[(size_t)l], n = p->levptr[(size_t)l + 1] - r0;
      hipLaunchKernelGGL(sor_level_kernel<KIND>, dim3((n + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream, n, p->d_rows + r0, a);
      MI355X_LAUNCH_CHECK();
    }
  }
  return 0;
}

// lev[] of the header; pend[c] carries 1 + max lev[j] over the rows j < c passed so far that store a(j,c)
static int sor_levels(int m, const int *ai, const int *aj, int *lev) {
  std::vector<int> pend((size_t)(m > 0 ? m : 1), 0);
  int nlev = 0;
  for (int i = 0; i < m; ++i) {
    int l = pend[(size_t)i];
    for (int k = ai[i]; k < ai[i + 1]; ++k) { const int c = aj[k]; if (c < i && lev[c] + 1 > l) l = lev[c] + 1; }
    lev[i] = l;
    if (l + 1 > nlev) nlev = l + 1;
    for (int k = ai[i]; k < ai[i + 1]; ++k) { const int c = aj[k]; if (c > i && l + 1 > pend[(size_t)c]) pend[(size_t)c] = l + 1; }
  }
  return nlev;
}
// the pattern the kernels may be handed: first offending row, or -1; diag[i] (may be NULL) = position of a(i,i)
static int sor_check_pattern(int m, const int *ai, const int *aj, int *diag) {
  if (m < 0 || (m > 0 && ai[0] != 0)) return 0;
  const int nth = m < 200000 ? 1 : mi355x_host_threads(16);
  std::vector<int> bad((size_t)nth, -1);
  mi355x_parallel_chunks(nth, [&](int k) {
    const int lo = (int)((long)m * k / nth), hi = (int)((long)m * (k + 1) / nth);
    for (int i = lo; i < hi; ++i) {
      int d = -1, ok = ai[i + 1] >= ai[i];
      for (int q = ai[i]; ok && q < ai[i + 1]; ++q) {
        const int c = aj[q];
        if (c < 0 || c >= m || (q > ai[i] && c <= aj[q - 1])) ok = 0;
        if (c == i) d = q;
      }
      if (!ok || d < 0) { bad[(size_t)k] = i; return; }
      if (diag) diag[i] = d;
    }
  });
  for (int k = 0; k < nth; ++k) if (bad[(size_t)k] >= 0) return bad[(size_t)k];   // chunks are in row order: the first row
  return -1;
}

extern "C" {

int mi355x_sor_levels_host(int m, const int *ai, const int *aj, int *lev, int *nlev) {
  return mi355x_guard([&] {
    if (m < 0 || (m > 0 && (!ai || !lev))) return (int)hipErrorInvalidValue;
    for (int i = 0; i < m; ++i) {
      if (ai[i + 1] < ai[i]) return (int)hipErrorInvalidValue;
      for (int k = ai[i]; k < ai[i + 1]; ++k) if (aj[k] < 0 || aj[k] >= m) return (int)hipErrorInvalidValue;
    }
    const int n = sor_levels(m, ai, aj, lev);
    if (nlev) *nlev = n;
    return 0;
  });
}

int mi355x_sor_plan_destroy(mi355x_sor_plan_t p) {
  if (!p) return 0;
  if (p->d_rows) (void)hipFree(p->d_rows);
  if (p->d_diag) (void)hipFree(p->d_diag);
  if (p->d_levptr) (void)hipFree(p->d_levptr);
  delete p;
  return 0;
}

int mi355x_sor_plan_create(mi355x_handle_t h, int m, const int *ai, const int *aj, int flags, mi355x_sor_plan_t *plan, int *bad_row) {
  if (!plan || !h) return (int)hipErrorInvalidValue;
  *plan = nullptr;
  if (bad_row) *bad_row = -1;
  return mi355x_guard([&] {
    if (m < 0 || !ai || (m > 0 && ai[m] > 0 && !aj)) return (int)hipErrorInvalidValue;
    std::unique_ptr<mi355x_sor_plan_s, decltype(&mi355x_sor_plan_destroy)> p(new mi355x_sor_plan_s(), mi355x_sor_plan_destroy);
    std::vector<int> diag((size_t)(m > 0 ? m : 1)), lev((size_t)(m > 0 ? m : 1)), rows((size_t)(m > 0 ? m : 1));
    const int bad = sor_check_pattern(m, ai, aj, diag.data());
    if (bad >= 0) { if (bad_row) *bad_row = bad; return (int)hipErrorInvalidValue; }
    p->m = m;
    p->nlev = sor_levels(m, ai, aj, lev.data());
    // rows sorted by level, ascending row inside a level
    p->levptr.assign((size_t)p->nlev + 1, 0);
    for (int i = 0; i < m; ++i) p->levptr[(size_t)lev[(size_t)i] + 1]++;
    for (int l = 0; l < p->nlev; ++l) p->levptr[(size_t)l + 1] += p->levptr[(size_t)l];
    { std::vector<int> next(p->levptr.begin(), p->levptr.end());
      for (int i = 0; i < m; ++i) rows[(size_t)next[(size_t)lev[(size_t)i]]++] = i; }
    // the launches of a sweep: runs of >= 2 consecutive small levels are fused, everything else goes level by level
    for (int l = 0; l < p->nlev;) {
      int e = l;
      const bool small = p->levptr[(size_t)l + 1] - p->levptr[(size_t)l] <= MI355X_BLOCK;
      while (e < p->nlev && (p->levptr[(size_t)e + 1] - p->levptr[(size_t)e] <= MI355X_BLOCK) == small) ++e;
      const int fuse = small && e - l >= 2 && !(flags & MI355X_SOR_NO_FUSE);
      if (fuse) p->fused_levels += e - l;
      if (!p->steps.empty() && !fuse && !p->steps.back().fused) p->steps.back().l1 = e;
      else p->steps.push_back({l, e, fuse});
      l = e;
    }
    MI355X_TRY(hipMalloc((void **)&p->d_rows, sizeof(int) * rows.size()));
    MI355X_TRY(hipMalloc((void **)&p->d_diag, sizeof(int) * diag.size()));
    MI355X_TRY(hipMalloc((void **)&p->d_levptr, sizeof(int) * p->levptr.size()));
    MI355X_TRY(hipMemcpyAsync(p->d_rows, rows.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipMemcpyAsync(p->d_diag, diag.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipMemcpyAsync(p->d_levptr, p->levptr.data(), sizeof(int) * p->levptr.size(), hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipStreamSynchronize(h->stream));      // once per pattern: the host vectors are pageable and go out of scope
    *plan = p.release();
    return 0;
  });
}

int mi355x_sor_plan_info(mi355x_sor_plan_t p, int *nlev, int *launches_per_sweep, int *fused_levels) {
  if (!p) return (int)hipErrorInvalidValue;
  int launches = 0;
  for (const sor_step &st : p->steps) launches += st.fused ? 1 : st.l1 - st.l0;
  if (nlev) *nlev = p->nlev;
  if (launches_per_sweep) *launches_per_sweep = launches;
  if (fused_levels) *fused_levels = p->fused_levels;
  return 0;
}

int mi355x_sor_idiag(mi355x_handle_t h, mi355x_sor_plan_t p, const double *aa, double omega, double fshift, double *idiag, double *mdiag) {
  if (!p || !idiag || !mdiag) return (int)hipErrorInvalidValue;
  if (p->m <= 0) return 0;
  hipLaunchKernelGGL(sor_idiag_kernel, dim3(mi355x_grid_for((size_t)p->m, 1)), dim3(MI355X_BLOCK), 0, h->stream, p->m, p->d_diag, aa, omega, fshift,
                     (int)(omega == 1.0 && fshift == 0.0), idiag, mdiag);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_sor_sweep(mi355x_handle_t h, mi355x_sor_plan_t p, int kind, const int *ai, const int *aj, const double *aa, const double *idiag,
                     const double *mdiag, double omega, const double *b, double *t, double *x) {
  if (!p || !b || !x || b == x) return (int)hipErrorInvalidValue;
  if ((kind == MI355X_SOR_ZERO_FORWARD || kind == MI355X_SOR_ZERO_BACKWARD_AFTER) && !t) return (int)hipErrorInvalidValue;
  const sor_args a = {ai, aj, aa, p->d_diag, idiag, mdiag, omega, b, t, x};
  switch (kind) {
    case MI355X_SOR_ZERO_FORWARD: return sor_run<MI355X_SOR_ZERO_FORWARD>(h, p, 0, a);
    case MI355X_SOR_ZERO_BACKWARD: return sor_run<MI355X_SOR_ZERO_BACKWARD>(h, p, 1, a);
    case MI355X_SOR_ZERO_BACKWARD_AFTER: return sor_run<MI355X_SOR_ZERO_BACKWARD_AFTER>(h, p, 1, a);
    case MI355X_SOR_FORWARD: return sor_run<MI355X_SOR_FORWARD>(h, p, 0, a);
    case MI355X_SOR_BACKWARD: return sor_run<MI355X_SOR_FORWARD>(h, p, 1, a);      // the same row body, levels descending
  }
  return (int)hipErrorInvalidValue;
}

int mi355x_sor_apply(mi355x_handle_t h, mi355x_sor_plan_t p, const int *ai, const int *aj, const double *aa, const double *idiag,
                     const double *mdiag, double omega, int flag, int its, const double *b, double *t, double *x) {
  if (!p || its <= 0 || (flag & ~SOR_FLAG_KNOWN)) return (int)hipErrorInvalidValue;
  const bool fwd = (flag & SOR_FLAG_FORWARD) != 0, bwd = (flag & SOR_FLAG_BACKWARD) != 0;
#define SOR_SWEEP(kind) do { const int rc_ = mi355x_sor_sweep(h, p, (kind), ai, aj, aa, idiag, mdiag, omega, b, t, x); if (rc_) return rc_; } while (0)
  if (flag & SOR_FLAG_ZERO) {
    if (fwd) SOR_SWEEP(MI355X_SOR_ZERO_FORWARD);
    if (bwd) SOR_SWEEP(fwd ? MI355X_SOR_ZERO_BACKWARD_AFTER : MI355X_SOR_ZERO_BACKWARD);
    its--;
  }
  while (its--) {
    if (fwd) SOR_SWEEP(MI355X_SOR_FORWARD);
    if (bwd) SOR_SWEEP(MI355X_SOR_BACKWARD);
  }
#undef SOR_SWEEP
  return 0;
}

}  // extern "C"
