// Block ILU(k) of MATSEQBAIJ: level-scheduled block triangular solves on the device and the numeric factorisation restated on the
// host (mi355x_kernels.h, "Block ILU").  Reference: MatSolve_SeqBAIJ_<bs>_NaturalOrdering (src/mat/impls/baij/seq/baijfact2.c) and
// MatLUFactorNumeric_SeqBAIJ_<bs>_NaturalOrdering (baijfact*.c) on the factor layout of the point ILU (aijfact.c:1628-1700) with
// one bs x bs column-major block per stored entry: L block rows forward from bi, U block rows stored from the last row backwards,
// each followed by its INVERTED diagonal block at bdiag[i].
//
// Solves.  One lane per scalar row; the bs lanes of a block row are one group, padded to a power of two (2, 4 or 8 lanes) so that
// 256 / width groups tile a workgroup and no group straddles a wavefront.  A lane walks the stored blocks of its block row in
// storage order; the bs solution values of the dependency block are loaded by every lane of the group from the same addresses (one
// broadcast load each), the lane's own row of the block is a strided read of ba.  The upper solve ends in the product with the
// inverted diagonal block, which needs the group's bs sums: they travel by cross-lane shuffles, never through memory.  Padding
// lanes and the groups past nrows take part in the shuffles with an empty block range and neither load nor store.
// Rows of one dependency level do not read each other, a kernel boundary separates the levels: nothing here waits on anything.
// The chain kernels run the same body for a run of consecutive levels in one launch of ONE workgroup of 1024 threads, with a
// workgroup barrier where the level route has a kernel boundary (worth it for levels well under one pass of that workgroup:
// DESIGN.md, "Block ILU(k)"); mi355x_bilu_chain_plan_host says which levels to chain.
#include "common.hpp"
#include "mi355x_block_inverse.h"
#include <string.h>
#include <stdlib.h>

#define BILU_MIN_BS 2
#define BILU_MAX_BS 7

// lanes of a block row's group: the smallest power of two >= BS
template <int BS> struct BiluGroup { static constexpr int W = BS <= 2 ? 2 : (BS <= 4 ? 4 : 8); };

// s - (v[r] x[0] + v[r + BS] x[1] + ...): row r of one column-major block times the dependency block's values, the products summed
// left to right, then one subtraction (-ffp-contract=off: every product and every sum rounded)
template <int BS> __device__ __forceinline__ double bilu_minus_row(double s, const double *__restrict__ v, int r, const double *xk) {
  double t = v[r] * xk[0];
#pragma unroll
  for (int c = 1; c < BS; ++c) t = t + v[r + c * BS] * xk[c];
  return s - t;
}

// the accumulation both solves share: the blocks q0 .. q1 - 1 of ba against the x values their block columns name
template <int BS> __device__ __forceinline__ double bilu_sweep(double s, int q0, int q1, int r, const int *__restrict__ bj,
                                                               const double *__restrict__ ba, const double *x) {
  for (int q = q0; q < q1; ++q) s = bilu_minus_row<BS>(s, ba + (size_t)q * (BS * BS), r, x + (size_t)bj[q] * BS);
  return s;
}

// One pass of a level: group g of `nrows` block rows, lane r of the group.  UPPER = false: x_i = b_i - sum_k L_ik x_k (bdiag unused).
// UPPER = true: x_i = D_i^-1 (x_i - sum_k U_ik x_k) in place.  Every lane of the wavefront calls this, a lane without a scalar row
// (padding, g >= nrows) with an empty block range: it takes part in the shuffles and neither loads nor stores.  The level kernel and
// the chain kernel both run this body and nothing else on the values.
template <int BS, bool UPPER>
__device__ __forceinline__ void bilu_pass(int g, int nrows, int r, const int *__restrict__ rows, const int *__restrict__ bi,
                                          const int *__restrict__ bj, const double *__restrict__ ba, const int *__restrict__ bdiag,
                                          const double *b, double *x) {
  constexpr int W = BiluGroup<BS>::W;
  const bool live = g < nrows && r < BS;
  int i = 0, q0 = 0, q1 = 0;
  double s = 0.0;
  if (live) {
    i = rows[g];
    if (UPPER) { q0 = bdiag[i + 1] + 1; q1 = bdiag[i]; s = x[(size_t)i * BS + r]; }
    else { q0 = bi[i]; q1 = bi[i + 1]; s = b[(size_t)i * BS + r]; }
  }
  s = bilu_sweep<BS>(s, q0, q1, r, bj, ba, x);      // (an idle lane: an empty range)
  if (UPPER) {
    // every lane of the wavefront is here: the group's sums, lane by lane
    const int first = (threadIdx.x & (MI355X_WAVE - 1)) & ~(W - 1);
    double sv[BS];
#pragma unroll
    for (int c = 0; c < BS; ++c) sv[c] = __shfl(s, first + c, MI355X_WAVE);
    if (live) {
      const double *__restrict__ d = ba + (size_t)q1 * (BS * BS);     // the inverted diagonal block at bdiag[i]
      double acc = d[r] * sv[0];
#pragma unroll
      for (int c = 1; c < BS; ++c) acc = acc + d[r + c * BS] * sv[c];
      x[(size_t)i * BS + r] = acc;
    }
  } else if (live) x[(size_t)i * BS + r] = s;
}

template <int BS, bool UPPER>
__global__ __launch_bounds__(MI355X_BLOCK) void bilu_level_kernel(int nrows, const int *__restrict__ rows, const int *__restrict__ bi,
                                                                  const int *__restrict__ bj, const double *__restrict__ ba,
                                                                  const int *__restrict__ bdiag, const double *b, double *x) {
  constexpr int W = BiluGroup<BS>::W;
  const int t = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  bilu_pass<BS, UPPER>(t / W, nrows, t & (W - 1), rows, bi, bj, ba, bdiag, b, x);
}

// The levels 0 .. nlev - 1 of levptr by ONE workgroup of BILU_CHAIN_BLOCK threads: level l is the block rows rows[levptr[l]] ..
// rows[levptr[l + 1] - 1], taken BILU_CHAIN_BLOCK / W at a time, then one barrier (the rows of a level do not read each other).
// nlev is a kernel argument and levptr[l] one address for the whole workgroup, so every trip count is the same in every thread:
// every thread runs every pass (past the level's end with an empty block range) and reaches every barrier.  x is written with
// plain stores and read after __syncthreads() by the waves of the same workgroup, which share one L1: the barrier's
// workgroup-scope fence is all the ordering there is, and x and b are plain pointers so that no load of x moves across it.
#define BILU_CHAIN_BLOCK 1024
template <int BS, bool UPPER>
__global__ __launch_bounds__(BILU_CHAIN_BLOCK) void bilu_chain_kernel(int nlev, const int *__restrict__ levptr, const int *__restrict__ rows,
                                                                      const int *__restrict__ bi, const int *__restrict__ bj,
                                                                      const double *__restrict__ ba, const int *__restrict__ bdiag,
                                                                      const double *b, double *x) {
  constexpr int W = BiluGroup<BS>::W, PER_PASS = BILU_CHAIN_BLOCK / W;
  const int g = (int)threadIdx.x / W, r = (int)threadIdx.x & (W - 1);
  int r0 = levptr[0];
  for (int l = 0; l < nlev; ++l) {
    const int r1 = levptr[l + 1], n = r1 - r0;
    for (int base = 0; base < n; base += PER_PASS) bilu_pass<BS, UPPER>(base + g, n, r, rows + r0, bi, bj, ba, bdiag, b, x);
    __syncthreads();
    r0 = r1;
  }
}

template <int BS, bool UPPER>
static int bilu_launch(mi355x_handle_t h, int nrows, const int *rows, const int *bi, const int *bj, const double *ba, const int *bdiag,
                       const double *b, double *x) {
  constexpr int per_block = MI355X_BLOCK / BiluGroup<BS>::W;       // block rows per workgroup
  const unsigned grid = (unsigned)(((long)nrows + per_block - 1) / per_block);
  hipLaunchKernelGGL((bilu_level_kernel<BS, UPPER>), dim3(grid), dim3(MI355X_BLOCK), 0, h->stream, nrows, rows, bi, bj, ba, bdiag, b, x);
  MI355X_LAUNCH_CHECK();
  return 0;
}
template <int BS, bool UPPER>
static int bilu_chain_launch(mi355x_handle_t h, int nlev, const int *levptr, const int *rows, const int *bi, const int *bj, const double *ba,
                             const int *bdiag, const double *b, double *x) {
  hipLaunchKernelGGL((bilu_chain_kernel<BS, UPPER>), dim3(1), dim3(BILU_CHAIN_BLOCK), 0, h->stream, nlev, levptr, rows, bi, bj, ba, bdiag, b, x);
  MI355X_LAUNCH_CHECK();
  return 0;
}
// nlev == 0: one level launch of `count` block rows of `rows`; nlev > 0: one chain launch over the levels of levptr
template <bool UPPER>
static int bilu_dispatch(mi355x_handle_t h, int count, int nlev, const int *levptr, const int *rows, int bs, const int *bi, const int *bj,
                         const double *ba, const int *bdiag, const double *b, double *x) {
  if (bs < BILU_MIN_BS || bs > BILU_MAX_BS) return (int)hipErrorInvalidValue;
  if (count <= 0 && nlev <= 0) return 0;
#define BILU_CASE(BS) case BS: return nlev > 0 ? bilu_chain_launch<BS, UPPER>(h, nlev, levptr, rows, bi, bj, ba, bdiag, b, x) \
                                               : bilu_launch<BS, UPPER>(h, count, rows, bi, bj, ba, bdiag, b, x)
  switch (bs) {
    BILU_CASE(2); BILU_CASE(3); BILU_CASE(4); BILU_CASE(5); BILU_CASE(6);
    default: BILU_CASE(7);
  }
#undef BILU_CASE
}

// ---------------------------------------------------------------------------------------------------- numeric factorisation, host
// c = a b for column-major bs x bs blocks: every entry a left-to-right sum of bs products
static void bilu_block_mult(int bs, const double *a, const double *b, double *c) {
  for (int col = 0; col < bs; ++col)
    for (int r = 0; r < bs; ++r) {
      double t = a[r] * b[col * bs];
      for (int k = 1; k < bs; ++k) t = t + a[r + k * bs] * b[k + col * bs];
      c[r + col * bs] = t;
    }
}
// w = w - m u: the same sums, then one subtraction per entry
static void bilu_block_minus_mult(int bs, double *w, const double *m, const double *u) {
  for (int col = 0; col < bs; ++col)
    for (int r = 0; r < bs; ++r) {
      double t = m[r] * u[col * bs];
      for (int k = 1; k < bs; ++k) t = t + m[r + k * bs] * u[k + col * bs];
      w[r + col * bs] = w[r + col * bs] - t;
    }
}

extern "C" {

int mi355x_bilu_lower_level(mi355x_handle_t h, int nrows, const int *rows, int bs, const int *bi, const int *bj, const double *ba,
                            const double *b, double *x) {
  return bilu_dispatch<false>(h, nrows, 0, nullptr, rows, bs, bi, bj, ba, nullptr, b, x);
}

int mi355x_bilu_upper_level(mi355x_handle_t h, int nrows, const int *rows, int bs, const int *bj, const double *ba, const int *bdiag,
                            double *x) {
  return bilu_dispatch<true>(h, nrows, 0, nullptr, rows, bs, nullptr, bj, ba, bdiag, nullptr, x);
}

int mi355x_bilu_lower_chain(mi355x_handle_t h, int nlev, const int *levptr, const int *rows, int bs, const int *bi, const int *bj,
                            const double *ba, const double *b, double *x) {
  return bilu_dispatch<false>(h, 0, nlev, levptr, rows, bs, bi, bj, ba, nullptr, b, x);
}

int mi355x_bilu_upper_chain(mi355x_handle_t h, int nlev, const int *levptr, const int *rows, int bs, const int *bj, const double *ba,
                            const int *bdiag, double *x) {
  return bilu_dispatch<true>(h, 0, nlev, levptr, rows, bs, nullptr, bj, ba, bdiag, nullptr, x);
}

int mi355x_bilu_chain_plan_host(int nlev, const int *levptr, int max_rows, int *seg_ptr, int *seg_fused, int *nseg) {
  if (!nseg) return (int)hipErrorInvalidValue;
  *nseg = 0;
  if (nlev < 0) return (int)hipErrorInvalidValue;
  if (nlev == 0) return 0;
  if (!levptr || !seg_ptr || !seg_fused) return (int)hipErrorInvalidValue;
  for (int l = 0; l < nlev; ++l) if (levptr[l + 1] < levptr[l]) return (int)hipErrorInvalidValue;
  int ns = 0;
  for (int l = 0; l < nlev;) {
    int e = l + 1;                                                     // a wide level: a segment of its own
    const bool narrow = max_rows > 0 && levptr[l + 1] - levptr[l] <= max_rows;
    if (narrow) while (e < nlev && levptr[e + 1] - levptr[e] <= max_rows) ++e;   // the maximal run of narrow levels from l
    seg_ptr[ns] = l; seg_fused[ns] = narrow ? 1 : 0; ++ns;
    l = e;
  }
  seg_ptr[ns] = nlev;
  *nseg = ns;
  return 0;
}

int mi355x_bilu_numeric_host(int mbs, int bs, const int *ai, const int *aj, const double *aa, const int *bi, const int *bj,
                             const int *bdiag, double *ba, int *zero_pivot_row) {
  if (zero_pivot_row) *zero_pivot_row = -1;
  if (bs < BILU_MIN_BS || bs > BILU_MAX_BS || mbs < 0 || !ai || !bi || !bdiag) return (int)hipErrorInvalidValue;
  if (mbs == 0) return 0;
  if (!aj || !aa || !bj || !ba) return (int)hipErrorInvalidValue;
  const size_t bs2 = (size_t)bs * bs;
  // one work block per block column; in_row[j] == i: block column j belongs to the factor's row i
  double *work = (double *)malloc(sizeof(double) * bs2 * (size_t)mbs);
  int *in_row = (int *)malloc(sizeof(int) * (size_t)mbs);
  if (!work || !in_row) { free(work); free(in_row); return (int)hipErrorOutOfMemory; }
  for (int j = 0; j < mbs; ++j) in_row[j] = -1;
  double m[BILU_MAX_BS * BILU_MAX_BS];
  int rc = 0;
  for (int i = 0; i < mbs && !rc; ++i) {
    const int l0 = bi[i], l1 = bi[i + 1], u0 = bdiag[i + 1] + 1, u1 = bdiag[i];     // L blocks, strict-upper blocks; the diagonal at u1
    if (l0 > l1 || u0 > u1 || bj[u1] != i) { rc = (int)hipErrorInvalidValue; break; }
    for (int q = l0; q < l1 && !rc; ++q) { if (bj[q] < 0 || bj[q] >= i) rc = (int)hipErrorInvalidValue; else { in_row[bj[q]] = i; memset(work + bs2 * bj[q], 0, sizeof(double) * bs2); } }
    for (int q = u0; q <= u1 && !rc; ++q) { if (bj[q] < i || bj[q] >= mbs) rc = (int)hipErrorInvalidValue; else { in_row[bj[q]] = i; memset(work + bs2 * bj[q], 0, sizeof(double) * bs2); } }
    for (int q = ai[i]; q < ai[i + 1] && !rc; ++q) {                                 // A's blocks: the factor's pattern contains A's
      if (aj[q] < 0 || aj[q] >= mbs || in_row[aj[q]] != i) rc = (int)hipErrorInvalidValue;
      else memcpy(work + bs2 * aj[q], aa + bs2 * q, sizeof(double) * bs2);
    }
    if (rc) break;
    for (int q = l0; q < l1; ++q) {                                                  // ascending k, fill included
      const int k = bj[q];
      double *wk = work + bs2 * k;
      bool any = false;
      for (size_t e = 0; e < bs2; ++e) if (wk[e] != 0.0) { any = true; break; }
      if (!any) continue;
      bilu_block_mult(bs, wk, ba + bs2 * bdiag[k], m);                               // M = W_k D_k^-1
      memcpy(wk, m, sizeof(double) * bs2);
      for (int p = bdiag[k + 1] + 1; p < bdiag[k]; ++p)
        if (in_row[bj[p]] == i) bilu_block_minus_mult(bs, work + bs2 * bj[p], m, ba + bs2 * p);
    }
    for (int q = l0; q < l1; ++q) memcpy(ba + bs2 * q, work + bs2 * bj[q], sizeof(double) * bs2);
    for (int q = u0; q <= u1; ++q) memcpy(ba + bs2 * q, work + bs2 * bj[q], sizeof(double) * bs2);
    const int z = mi355x_block_inverse(bs, ba + bs2 * u1);                           // D_i^-1 in the diagonal's slot
    if (z) { if (zero_pivot_row) *zero_pivot_row = i * bs + z - 1; rc = (int)hipErrorUnknown; }
  }
  free(work); free(in_row);
  return rc;
}

}  // extern "C"
