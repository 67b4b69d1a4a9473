// Row reductions over CSR / BCSR for gfx950: what MatNorm, MatGetRowMaxAbs / Max / Min and MatGetColumnNorms ask of the stored
// values (MatNorm_SeqAIJ aij.c, MatGetRowMaxAbs_SeqAIJ / MatGetRowMax_SeqAIJ / MatGetRowMin_SeqAIJ aij.c, MatNorm_SeqBAIJ baij.c).
//
// One templated body, one instance per operation and block size.  It is a member of the row-block family (rowblock.hpp): a
// 256-thread workgroup owns 256 / bs block rows, streams their slice of the value array through the LDS stage with the family's
// coalesced pair loads -- the operation's transform (|a|, a * a, a) applied on the way in -- and then every lane walks ITS point
// row out of LDS, one lane per row, in storage order: the sums by the family's in-order accumulate (the bits of the sequential
// loop, and of the one-lane product path with a vector of ones), the extrema by a strict comparison.  A slice longer than the
// stage is streamed in pieces; a lane keeps its accumulator and its place in the row across pieces, so a row of any length is
// still summed left to right.  Plain loads and stores; a lane writes only out[row] / idx[row] of its own row.
//
// Point row i = I bs + r of a BCSR matrix (blocks column-major, baij.h:13-30) stores its entries at S + j bs, j = 0 .. (a1 - a0) bs - 1,
// S = a0 bs^2 + r: block order, and column order inside a block.  bs = 1 is CSR (S = a0, stride 1).
#include "common.hpp"
#include "rowblock.hpp"

#define RED_SUM_OP(OP) ((OP) <= MI355X_ROW_SQSUM)
static_assert(MI355X_ROW_SUM == 0 && MI355X_ROW_ABSSUM == 1 && MI355X_ROW_SQSUM == 2 && MI355X_ROW_MAXABS == 3 && MI355X_ROW_MAX == 4 && MI355X_ROW_MIN == 5,
              "the sums come first");

// what an entry contributes (a * a is a product and a separate add: the build sets -ffp-contract=off)
template <int OP> __device__ __forceinline__ double red_value(double v) {
  return (OP == MI355X_ROW_ABSSUM || OP == MI355X_ROW_MAXABS) ? fabs(v) : (OP == MI355X_ROW_SQSUM ? v * v : v);
}

// entries j0 .. j1 - 1 of a point row added to sum in order; entry j lies at stage[base + j * BS] (the strided form of row_sum_lds)
template <int BS> __device__ __forceinline__ double row_sum_lds_strided(const double *stage, int base, int j0, int j1, double sum) {
  if (BS == 1) return row_sum_lds(stage, base + j0, base + j1, sum, 0);
  for (int k = j0; k < j1; k += 8) {
    double t[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) t[q] = stage[base + ((k + q < j1) ? k + q : j1 - 1) * BS];
    sum = accumulate8(sum, k, j1, 0, [&](int q) { return t[q]; });
  }
  return sum;
}

// the scalar column of entry j of a point row whose block row starts at a0
template <int BS> __device__ __forceinline__ int entry_column(const int *__restrict__ aj, int a0, int j) {
  return BS == 1 ? aj[a0 + j] : aj[a0 + j / BS] * BS + j % BS;
}

template <int OP, int BS>
__global__ __launch_bounds__(SPMV_THREADS) void mat_row_reduce_kernel(int mbs, int ncols, const int *__restrict__ ai, const int *__restrict__ aj,
                                                                      const double *__restrict__ aa, int vec, const int *__restrict__ rows,
                                                                      const double *acc, double *out, int *idx) {
  constexpr int RB = SPMV_THREADS / BS, BS2 = BS * BS;          // block rows per workgroup
  __shared__ double stage[SPMV_BLOCK_NNZ];
  const int tid = threadIdx.x;
  const int R0 = blockIdx.x * RB, R1 = (mbs - R0 < RB) ? mbs : R0 + RB;   // the grid has no workgroup with R0 >= mbs
  const int nrows = (R1 - R0) * BS;
  const row_lanes rl = lanes_per_row(nrows, 0, tid);             // one lane per point row: the in-order path
  const bool has_row = rl.r < nrows;
  const int I = R0 + (has_row ? rl.r / BS : 0), r = has_row ? rl.r % BS : 0;
  const int a0 = ai[I], a1 = ai[I + 1];
  const int e0 = ai[R0] * BS2, e1 = ai[R1] * BS2;                // the workgroup's slice of the value array
  const int n = has_row ? (a1 - a0) * BS : 0, S = a0 * BS2 + r;  // this lane's entries: aa[S + j BS], j < n
  const int prow = I * BS + r, orow = (has_row && rows) ? rows[prow] : prow;
  const bool full = n > 0 && n == ncols;                         // max / min: no implicit zero, the scan starts from the first entry
  double cur = (RED_SUM_OP(OP) && has_row && acc) ? acc[orow] : 0.0;
  int best = -1;                                                 // the entry that holds the extremum; -1: the starting value
  int j = 0;                                                     // entries consumed so far

  for (int c0 = e0; c0 < e1; c0 += SPMV_BLOCK_CAP) {
    const int c1 = (e1 - c0 > SPMV_BLOCK_CAP) ? c0 + SPMV_BLOCK_CAP : e1;
    if (vec) {
      v2d v[SPMV_PAIRS];
#pragma unroll
      for (int p = 0; p < SPMV_PAIRS; ++p) v[p] = load_pair<v2d>(aa, c0, c1, pair_k(c0, tid, p));
#pragma unroll
      for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(stage, pair_k(c0, tid, p), c0, c1, red_value<OP>(v[p].x), red_value<OP>(v[p].y));
    } else {
      for (int k = c0 + tid; k < c1; k += SPMV_THREADS) stage[k - c0] = red_value<OP>(SPMV_LOAD(aa + k));
    }
    __syncthreads();
    // this lane's entries inside [c0, c1): j .. jend - 1 (the pieces before this one held entries 0 .. j - 1)
    int jend = c1 > S ? (c1 - S + BS - 1) / BS : 0;
    jend = jend > n ? n : jend;
    if (jend > j) {
      if (RED_SUM_OP(OP)) cur = row_sum_lds_strided<BS>(stage, S - c0, j, jend, cur);
      else {
        for (int k = j; k < jend; ++k) {
          const double v = stage[S - c0 + k * BS];
          const bool first = OP != MI355X_ROW_MAXABS && k == 0 && full;
          if (first || (OP == MI355X_ROW_MIN ? v < cur : cur < v)) { cur = v; best = k; }
        }
      }
      j = jend;
    }
    __syncthreads();                                             // the stage is refilled by the next piece
  }

  if (!has_row) return;
  out[orow] = cur;
  if (!RED_SUM_OP(OP) && idx) {
    int col = 0;
    if (best >= 0) col = entry_column<BS>(aj, a0, best);
    else if (OP != MI355X_ROW_MAXABS && n > 0) {                 // the implicit zero won: the smallest column the (ascending) row does not store
      while (col < n && entry_column<BS>(aj, a0, col) == col) ++col;
    }
    idx[orow] = col;
  }
}

template <int OP>
static int launch_row_reduce(mi355x_handle_t h, int mbs, int bs, int ncols, const int *ai, const int *aj, const double *aa, const int *rows,
                             const double *acc, double *out, int *idx) {
  const int vec = mi355x_aligned16(aa) ? 1 : 0;
  const dim3 block(SPMV_THREADS);
#define RED_GO(B) hipLaunchKernelGGL((mat_row_reduce_kernel<OP, B>), dim3((unsigned)((mbs + SPMV_THREADS / B - 1) / (SPMV_THREADS / B))), block, 0, \
                                     h->stream, mbs, ncols, ai, aj, aa, vec, rows, acc, out, idx)
  switch (bs) {
    case 1: RED_GO(1); break;
    case 2: RED_GO(2); break;
    case 3: RED_GO(3); break;
    case 4: RED_GO(4); break;
    case 5: RED_GO(5); break;
    case 6: RED_GO(6); break;
    case 7: RED_GO(7); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef RED_GO
  MI355X_LAUNCH_CHECK();
  return 0;
}

extern "C" int mi355x_mat_row_reduce(mi355x_handle_t h, int op, int mbs, int bs, int ncols, const int *ai, const int *aj, const double *aa,
                                     const int *rows, const double *acc, double *out, int *idx) {
  return mi355x_guard([&]() -> int {
    if (!h || mbs < 0 || ncols < 0 || bs < 1 || bs > 7 || op < MI355X_ROW_SUM || op > MI355X_ROW_MIN) return (int)hipErrorInvalidValue;
    if ((long)mbs * bs > 2147483647L) return (int)hipErrorInvalidValue;
    if (acc && !RED_SUM_OP(op)) return (int)hipErrorInvalidValue;       // an accumulator continues a sum
    if (idx && RED_SUM_OP(op)) return (int)hipErrorInvalidValue;        // a location belongs to an extremum
    if (rows && bs != 1) return (int)hipErrorInvalidValue;              // compressed rows are a CSR form
    if (mbs == 0) return 0;
    if (!ai || !aa || !out || (idx && !aj)) return (int)hipErrorInvalidValue;
    switch (op) {
      case MI355X_ROW_SUM: return launch_row_reduce<MI355X_ROW_SUM>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
      case MI355X_ROW_ABSSUM: return launch_row_reduce<MI355X_ROW_ABSSUM>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
      case MI355X_ROW_SQSUM: return launch_row_reduce<MI355X_ROW_SQSUM>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
      case MI355X_ROW_MAXABS: return launch_row_reduce<MI355X_ROW_MAXABS>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
      case MI355X_ROW_MAX: return launch_row_reduce<MI355X_ROW_MAX>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
      default: return launch_row_reduce<MI355X_ROW_MIN>(h, mbs, bs, ncols, ai, aj, aa, rows, acc, out, idx);
    }
  });
}
