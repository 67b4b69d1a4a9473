// C = A B for CSR matrices (MatMatMult_SeqAIJ_SeqAIJ: symbolic pass on the host once per pattern, numeric pass on the device), the
// building block of MatPtAP = P^T (A P).  A is m x k, B is k x n, every row's columns ascending.
//
// The contract (include/mi355x_kernels.h, DESIGN.md "Sparse matrix products"): row i of C stores the union of the column lists of the
// rows B[aj[t], :], t over row i of A, ascending, whether or not a value comes out zero.  Every c_ij starts at +0.0; the stored
// entries t of A's row i are taken in storage order and every stored b = B[aj[t], j] gives c_ij = c_ij + (a_it * b): the product
// rounded, then the sum (-ffp-contract=off).  Nothing is skipped: a stored 0.0 in A against an Inf in B is a NaN in C.
//
// spgemm_numeric_kernel<W>: W lanes per row of C (W = 8, 16, 32 or 64, chosen per product from the mean length of the B rows the
// product visits), 64 / W rows per wavefront, 256 / W per workgroup.  A row's accumulator and its column list live in that row
// group's SPGEMM_LDS_ENTRIES slots of LDS.  One STEP per stored entry t of A's row, taken by the row's W lanes together: the lanes
// take the entries of B's row aj[t] strided by W, each finds its column's slot by a binary search over the column list in LDS and
// does the read-add-write there.  The columns of one B row are distinct, so within a step no two lanes touch one slot: no atomics.
// For a fixed slot the updates arrive in ascending t, the sequential loop's order, whatever W and whatever the launch shape:
// the bits depend on neither.
//
// A row of C longer than SPGEMM_LDS_ENTRIES is processed in column WINDOWS of that many entries: for each window all steps run
// again, and a lane whose column is not in the window (its search misses) does nothing.  Per slot the order is unchanged, so are
// the bits.  The accumulator never passes through global memory between steps; ca is written once per slot, when its window is
// done, and no lane reads from global memory what another lane wrote.
//
// Cross-lane visibility between steps.  A slot written by one lane in step t is read by whichever lane meets that column in step
// t' > t.  There is ONE path: W <= 64, so a row never spans two wavefronts, and what orders a step's LDS writes before the next
// step's LDS reads is the in-order execution of one wavefront's LDS instructions (the DS queue of a wave is served in issue order;
// lgkmcnt counts it in order).  The steps of a row are iterations of a loop all its W lanes run together, and the wavefront runs
// an iteration's instructions for all its active lanes before the next iteration's -- rows of one wavefront with fewer steps or
// shorter B rows sit masked out meanwhile -- so program order of the wavefront IS step order for every row it carries.  What is
// left is the compiler: SPGEMM_STEP_ORDER (a wavefront-scope release/acquire fence pair around a wave barrier, no instruction
// beyond a wait on the LDS counter) keeps it from moving or caching an LDS access across a step boundary.  No workgroup barrier
// is needed and none is used: rows of different wavefronts share nothing, and a row group that runs out of rows leaves alone.
#include "common.hpp"
#include <algorithm>
#include <vector>

#define SPGEMM_LDS_ENTRIES 128   // slots (a double and a column index: 12 bytes) per row group; DESIGN.md "Sparse matrix products" on the choice

#define SPGEMM_STEP_ORDER() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                                 __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

template <int W>
__global__ __launch_bounds__(MI355X_BLOCK) void spgemm_numeric_kernel(int nrows, const int *__restrict__ rows, const int *__restrict__ ai,
                                                                     const int *__restrict__ aj, const double *__restrict__ aa,
                                                                     const int *__restrict__ bi, const int *__restrict__ bj,
                                                                     const double *__restrict__ ba, const int *__restrict__ ci,
                                                                     const int *__restrict__ cj, double *__restrict__ ca) {
  constexpr int G = MI355X_BLOCK / W;                          // row groups of a workgroup
  __shared__ double lds_acc[G * SPGEMM_LDS_ENTRIES];
  __shared__ int lds_col[G * SPGEMM_LDS_ENTRIES];
  const int grp = (int)(threadIdx.x / W), l = (int)(threadIdx.x % W);
  const long g = (long)blockIdx.x * G + grp;
  if (g >= nrows) return;                                      // (a row's lanes leave together; nobody waits for them)
  double *acc = lds_acc + grp * SPGEMM_LDS_ENTRIES;
  int *col = lds_col + grp * SPGEMM_LDS_ENTRIES;
  const int i = rows[g];
  const int a0 = ai[i], a1 = ai[i + 1], c0 = ci[i], clen = ci[i + 1] - c0;
  for (int w0 = 0; w0 < clen; w0 += SPGEMM_LDS_ENTRIES) {      // one window for a row within the budget
    const int wn = clen - w0 < SPGEMM_LDS_ENTRIES ? clen - w0 : SPGEMM_LDS_ENTRIES;
    for (int p = l; p < wn; p += W) { col[p] = cj[c0 + w0 + p]; acc[p] = 0.0; }
    SPGEMM_STEP_ORDER();
    for (int t = a0; t < a1; ++t) {                            // a step: the row's lanes together, B's row aj[t] strided by W
      const int r = aj[t];
      const double av = aa[t];
      const int b1 = bi[r + 1];
      for (int q = bi[r] + l; q < b1; q += W) {
        const int c = bj[q];
        int lo = 0, hi = wn;                                   // first slot whose column is >= c
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < c) lo = mid + 1; else hi = mid; }
        if (lo < wn && col[lo] == c) acc[lo] = acc[lo] + av * ba[q];
      }
      SPGEMM_STEP_ORDER();
    }
    for (int p = l; p < wn; p += W) ca[c0 + w0 + p] = acc[p];
    SPGEMM_STEP_ORDER();                                       // (the next window fills the same slots)
  }
}

struct mi355x_spgemm_plan_s {
  int m = 0, k = 0, n = 0, lanes = 8, nrows = 0, nwindowed = 0;
  int *d_rows = nullptr;                                       // the rows of C with entries: those within the budget first, the windowed ones after them
  size_t workspace = 0;
  ~mi355x_spgemm_plan_s() { if (d_rows) (void)hipFree(d_rows); }
};

template <int W>
static void spgemm_launch(hipStream_t st, const mi355x_spgemm_plan_s *p, const int *ai, const int *aj, const double *aa, const int *bi,
                          const int *bj, const double *ba, const int *ci, const int *cj, double *ca) {
  constexpr int G = MI355X_BLOCK / W;
  hipLaunchKernelGGL(spgemm_numeric_kernel<W>, dim3((unsigned)((p->nrows + G - 1) / G)), dim3(MI355X_BLOCK), 0, st, p->nrows, p->d_rows, ai, aj,
                     aa, bi, bj, ba, ci, cj, ca);
}

namespace {
struct SymbolicArgs { int n; const int *ai, *aj, *bi, *bj; int *ci, *cj; };
// rows [lo, hi): the union of the B rows a row of A names, by a marker per column; counted into ci[i + 1], or written sorted at ci[i]
int spgemm_symbolic_rows(void *ctx, long lo, long hi) {
  const SymbolicArgs *s = (const SymbolicArgs *)ctx;
  return mi355x_guard([&]() -> int {
    std::vector<int> mark((size_t)(s->n > 0 ? s->n : 1), -1);
    for (long i = lo; i < hi; ++i) {
      int cnt = 0;
      int *out = s->cj ? s->cj + s->ci[i] : nullptr;
      for (int t = s->ai[i]; t < s->ai[i + 1]; ++t) {
        const int r = s->aj[t];
        for (int q = s->bi[r]; q < s->bi[r + 1]; ++q) {
          const int c = s->bj[q];
          if (mark[(size_t)c] != (int)i) { mark[(size_t)c] = (int)i; if (out) out[cnt] = c; cnt++; }
        }
      }
      if (out) std::sort(out, out + cnt);
      else s->ci[i + 1] = cnt;
    }
    return 0;
  });
}
bool spgemm_csr_ok(int nrows, int ncols, const int *pi, const int *pj) {   // row pointer ascending from 0, columns strictly ascending inside [0, ncols)
  if (pi[0] != 0) return false;
  for (int i = 0; i < nrows; ++i) {
    if (pi[i + 1] < pi[i]) return false;
    for (int q = pi[i]; q < pi[i + 1]; ++q) if (pj[q] < 0 || pj[q] >= ncols || (q > pi[i] && pj[q] <= pj[q - 1])) return false;
  }
  return true;
}
}  // namespace

extern "C" {

int mi355x_spgemm_symbolic_host(int m, int n, const int *ai, const int *aj, const int *bi, const int *bj, int *ci, int *cj, int nthreads) {
  if (m < 0 || n < 0 || !ci || (m > 0 && (!ai || !bi))) return (int)hipErrorInvalidValue;
  if (m == 0) { ci[0] = 0; return 0; }
  if (ai[m] > 0 && (!aj || !bj)) return (int)hipErrorInvalidValue;
  int nth = nthreads > 0 ? nthreads : (ai[m] < 200000 ? 1 : mi355x_host_threads(16));
  if (nth > m) nth = m;
  SymbolicArgs s = {n, ai, aj, bi, bj, ci, cj};
  const int rc = mi355x_host_parallel_ranges((long)m, nth, spgemm_symbolic_rows, &s);
  if (rc) return rc;
  if (!cj) {
    ci[0] = 0;
    for (int i = 0; i < m; ++i) {
      if ((long)ci[i] + (long)ci[i + 1] > 2147483000L) return (int)hipErrorInvalidValue;   // (32-bit row pointers)
      ci[i + 1] += ci[i];
    }
  }
  return 0;
}

int mi355x_spgemm_geometry(int *lds_entries_per_row_group, int *block) {
  if (lds_entries_per_row_group) *lds_entries_per_row_group = SPGEMM_LDS_ENTRIES;
  if (block) *block = MI355X_BLOCK;
  return 0;
}

int mi355x_spgemm_plan_create(mi355x_handle_t h, int m, int k, int n, const int *ai, const int *aj, const int *bi, const int *bj, const int *ci,
                              const int *cj, mi355x_spgemm_plan_t *plan) {
  if (!plan) return (int)hipErrorInvalidValue;
  *plan = nullptr;
  if (!h || m < 0 || k < 0 || n < 0 || !ai || !bi || !ci) return (int)hipErrorInvalidValue;
  if ((ai[m] > 0 && !aj) || (bi[k] > 0 && !bj) || (ci[m] > 0 && !cj)) return (int)hipErrorInvalidValue;
  return mi355x_guard([&]() -> int {
    // what the kernel indexes by, checked before anything runs on it: A's columns name rows of B, B's and C's columns are sorted
    // and inside the matrix (a column of B that C's list lacks is a search that misses, never a write)
    if (!spgemm_csr_ok(m, k, ai, aj) || !spgemm_csr_ok(k, n, bi, bj) || !spgemm_csr_ok(m, n, ci, cj)) return (int)hipErrorInvalidValue;
    std::unique_ptr<mi355x_spgemm_plan_s> p(new mi355x_spgemm_plan_s);
    p->m = m; p->k = k; p->n = n;
    double visited = 0.0;                                      // entries of B the product reads, one B row per entry of A
    for (int t = 0; t < ai[m]; ++t) visited += (double)(bi[aj[t] + 1] - bi[aj[t]]);
    const double mean = ai[m] > 0 ? visited / (double)ai[m] : 0.0;
    p->lanes = 8;
    while ((double)p->lanes < mean && p->lanes < MI355X_WAVE) p->lanes *= 2;
    std::vector<int> rows, wide;
    for (int i = 0; i < m; ++i) {
      const int len = ci[i + 1] - ci[i];
      if (len > SPGEMM_LDS_ENTRIES) wide.push_back(i);
      else if (len > 0) rows.push_back(i);
    }
    p->nwindowed = (int)wide.size();
    rows.insert(rows.end(), wide.begin(), wide.end());
    p->nrows = (int)rows.size();
    p->workspace = sizeof(int) * (size_t)(p->nrows > 0 ? p->nrows : 1);
    MI355X_TRY(hipMalloc((void **)&p->d_rows, p->workspace));
    if (p->nrows) MI355X_TRY(hipMemcpyAsync(p->d_rows, rows.data(), sizeof(int) * (size_t)p->nrows, hipMemcpyHostToDevice, h->stream));
    MI355X_TRY(hipStreamSynchronize(h->stream));               // (rows goes away here)
    *plan = p.release();
    return 0;
  });
}

int mi355x_spgemm_plan_destroy(mi355x_spgemm_plan_t plan) {
  delete plan;
  return 0;
}

int mi355x_spgemm_plan_info(mi355x_spgemm_plan_t plan, int *lanes, int *nwindowed_rows, size_t *workspace_bytes) {
  if (!plan) return (int)hipErrorInvalidValue;
  if (lanes) *lanes = plan->lanes;
  if (nwindowed_rows) *nwindowed_rows = plan->nwindowed;
  if (workspace_bytes) *workspace_bytes = plan->workspace;
  return 0;
}

int mi355x_spgemm_numeric(mi355x_handle_t h, mi355x_spgemm_plan_t p, const int *ai, const int *aj, const double *aa, const int *bi, const int *bj,
                          const double *ba, const int *ci, const int *cj, double *ca) {
  if (!h || !p) return (int)hipErrorInvalidValue;
  if (!p->nrows) return 0;                                     // C stores nothing
  if (!ai || !aj || !aa || !bi || !bj || !ba || !ci || !cj || !ca) return (int)hipErrorInvalidValue;
  switch (p->lanes) {
    case 8: spgemm_launch<8>(h->stream, p, ai, aj, aa, bi, bj, ba, ci, cj, ca); break;
    case 16: spgemm_launch<16>(h->stream, p, ai, aj, aa, bi, bj, ba, ci, cj, ca); break;
    case 32: spgemm_launch<32>(h->stream, p, ai, aj, aa, bi, bj, ba, ci, cj, ca); break;
    default: spgemm_launch<64>(h->stream, p, ai, aj, aa, bi, bj, ba, ci, cj, ca); break;
  }
  MI355X_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
