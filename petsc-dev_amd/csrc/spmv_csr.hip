// CSR SpMV for gfx950: y = A x and z = y + A x  (MatMult_SeqAIJ / MatMultAdd_SeqAIJ,
// reference src/mat/impls/aij/seq/aij.c:1225-1358).
//
// "Row-block streaming" (HBM-bound, AI = 0.125 flop/B): host analysis cuts the rows into row blocks of <= 256 rows and
// <= 2046 nonzeros; one 256-thread workgroup per row block streams the block's slice of the matrix with coalesced,
// unconditional, non-temporal pair loads (x is the only reused operand), parks the products in LDS and, after one
// barrier, sums each row out of LDS -- one lane per row in the reference's order (bit-identical to its non-FMA C loop),
// or 2..64 lanes and a shuffle tree for blocks of few, long rows.  A row longer than the stage gets a whole workgroup.
// The family -- plain, 8-bit offsets, row patterns, value patterns, grouped rows, BCSR -- differs in where the column of
// a nonzero comes from; the steps they share (block -> XCD map, lanes per row, pair loads, pair sources, LDS parking, row
// result, 8-wide accumulate, ordered workgroup sum) are the helpers of rowblock.hpp, written once.
#include "common.hpp"
#include "rowblock.hpp"
#include <map>
#include <array>
#include <memory>
#include <vector>
#include <stdlib.h>
#include <string.h>

struct mi355x_spmv_plan_s {
  int nrows;       // rows of the (possibly compressed) row pointer
  int nblocks;     // row blocks
  int nlong;       // of which single long rows
  int2 *d_rowblk;  // nblocks+1 entries {first row, first nonzero}
  int *d_rows;     // compressed-row output indices or NULL
  // offset-dictionary index compression (col = row + table[idx8]); NULL when the matrix has > 256 distinct offsets
  unsigned char *d_idx8;
  int *d_offtab;
  int ntab;
  // row patterns (stencil matrices): the offset lists of the rows come from a small dictionary; per row the start of its
  // list in the table and its first nonzero relative to its row block (one 4-byte word per ROW instead of 1 byte per nonzero)
  unsigned int *d_prow;
  int *d_pattab;       // SPMV_PAT_CAP ints
  int npat, use_pat;
  // run-coded patterns: per row block SPMV_RUN_WORDS words that describe its rows as <= SPMV_RUNS runs of equal patterns (see
  // spmv_pattern_runs); a block they describe does not read d_prow.  Structure only: lives and dies with d_prow / d_pattab
  unsigned int *d_pruns;
  int nruncoded, use_runs;
  int ch;              // run length (row blocks) of the row-pattern kernel's block -> XCD map, from the operator's largest offset
  // value patterns (constant-coefficient operators): rows whose offsets AND values repeat; per row 2 bytes, the values
  // live in the table.  Valid only for the values they were derived from (mi355x_spmv_plan_value_patterns / _drop_)
  unsigned short *d_vrow;
  int *d_vpattab;      // SPMV_PAT_CAP ints   {length, offsets ...}
  double *d_vpatval;   // SPMV_PAT_CAP doubles, value q of an entry at the index of its offset q
  int nvpat, vtablen, vpat_valid, use_vpat;
  double *d_dotpart;   // per-row-block x'y values of mi355x_spmv_csr_dot (allocated on first use)
  int ndotpart;        // how many of them the last mi355x_spmv_csr_dot wrote
  // rows summed the way MatMult_SeqAIJ_Inode does (two products at a time, inode.c:392-578): set when the reference's
  // Mat_CheckInode would switch this matrix to its inode routines
  int pairsum;
  // grouped rows (the MI355X form of the reference's inodes): consecutive rows with one column pattern share ONE
  // stored column list; d_rowblk4 = {first row, first nonzero, first shared column index, 0} per row block
  int4 *d_rowblk4;
  int *d_goff;         // per row: where its group's column list starts in d_gj
  int *d_gj;           // the groups' column lists, one after the other
  int ngroups;
  long ngj;
};

// ---------------------------------------------------------------------------------------------
// Plain kernel: the column of a nonzero is aj[k], streamed in pairs next to the values (VEC: aa 16-byte and aj 8-byte
// aligned; otherwise a scalar stream).  CPROW: compressed rows, row r of the plan is row rows[r] of y.
template <int ADD, bool CPROW, bool VEC>
__global__ __launch_bounds__(SPMV_THREADS, SPMV_MINWAVES) void spmv_csr_rowblock_kernel(
    const int2 *__restrict__ rowblk, int nblocks, const int *__restrict__ ai, const int *__restrict__ aj,
    const double *__restrict__ aa, const double *__restrict__ x, const double *yin, double *yout,
    const int *__restrict__ rows, int pairsum, const double *__restrict__ dsc, int nty) {
  // ADD == 3 only: dsc scales the row's result; nty: y is a stream of 256 MiB or more, stored past the caches
  const bool nt = ADD == 3 && nty;
  __shared__ double prod[SPMV_BLOCK_NNZ];
  const int lb = rowblock_of_workgroup(SPMV_CH);
  if (lb >= nblocks) return;

  // {first row, first nonzero} of this row block and of the next: one round trip, no dependent chain
  const int2 b0 = rowblk[lb];
  const int2 b1 = rowblk[lb + 1];
  const int r0 = b0.x, r1 = b1.x, k0 = b0.y, k1 = b1.y;
  const int nnz = k1 - k0;
  const int nrows = r1 - r0;
  const int tid = threadIdx.x;

  if (nnz > SPMV_BLOCK_CAP) {
    // one long row: strided partial sums, then a fixed tree
    double s = 0.0;
    for (int k = k0 + tid; k < k1; k += SPMV_THREADS) {
      double v = SPMV_LOAD(aa + k);
      int c = SPMV_LOAD(aj + k);
      s += v * x[c];
    }
    const double t = workgroup_sum_ordered<SPMV_WAVES>(s);
    if (tid == 0) {
      const int orow = CPROW ? rows[r0] : r0;
      spmv_store(yout + orow, spmv_out<ADD>(ADD ? yin[orow] : 0.0, t, ADD == 3 ? dsc[orow] : 1.0), nt);
    }
    return;
  }
  if (nnz == 0) {   // only empty rows
    if (tid < nrows) {
      const int orow = CPROW ? rows[r0 + tid] : r0 + tid;
      spmv_store(yout + orow, spmv_empty<ADD>(ADD ? yin[orow] : 0.0, ADD == 3 ? dsc[orow] : 1.0), nt);
    }
    return;
  }

  // lanes past the last row re-read the last row's extent: these loads are unconditional too
  const row_lanes rl = lanes_per_row(nrows, nnz, tid);
  const int tpr = rl.tpr, r = rl.r, sub = rl.sub;
  const int rc = r < nrows ? r : nrows - 1;
  const int a0 = ai[r0 + rc], a1 = ai[r0 + rc + 1];
  const int orow = CPROW ? rows[r0 + rc] : r0 + rc;
  double ysum = 0.0;
  if (ADD) ysum = yin[orow];
  const double dv = ADD == 3 ? dsc[orow] : 1.0;

  // ---- stream the block's nonzeros: product -> LDS -----------------------
  if (VEC) {
    v2d v[SPMV_PAIRS];
    v2i c[SPMV_PAIRS];
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) {
      v[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
      c[p] = load_pair<v2i>(aj, k0, k1, pair_k(k0, tid, p));
    }
    double xa[SPMV_PAIRS], xb[SPMV_PAIRS];
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) {
      const pair_src s = pair_source(pair_k(k0, tid, p), k0, k1);
      xa[p] = x[s.s0 ? c[p].y : c[p].x];
      xb[p] = x[s.s1 ? c[p].y : c[p].x];
    }
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(prod, pair_k(k0, tid, p), k0, k1, v[p].x * xa[p], v[p].y * xb[p]);
  } else {
    for (int k = k0 + tid; k < k1; k += SPMV_THREADS)
      prod[k - k0] = SPMV_LOAD(aa + k) * x[SPMV_LOAD(aj + k)];
  }
  __syncthreads();

  // ---- per-row sums out of LDS -------------------------------------------
  const int rs = r < nrows ? a0 - k0 : 0, re = r < nrows ? a1 - k0 : 0;
  row_result_lds<ADD>(prod, tpr, sub, r < nrows, rs, re, ysum, dv, pairsum, yout + orow, nt);
}

// ---------------------------------------------------------------------------------------------
// Index-compressed variant.  A matrix whose entries use at most 256 distinct offsets (col - row) -- every
// stencil operator: 7 for the 3-D Poisson matrix, 135 for 3-dof 27-point elasticity -- gets, at analysis time,
// one byte per nonzero (the position of its offset in a table) next to the unchanged CSR arrays.  The kernel
// streams val (8 B) + idx8 (1 B) instead of val + col (12 B): 25 % fewer matrix bytes.  The row of each nonzero,
// which the offset needs, comes from an LDS marker array written by the lanes that own the rows (they hold the
// row extents anyway).  Arithmetic and summation order are those of the plain kernel: same bits.
// DOT: the block also leaves the sum of x_r y_r over its rows in dotpart[block] (square matrix; KSPSolve_CG's p'w from the pass that
// makes w = A p), in a fixed order; mi355x_spmv_dot_finish adds the blocks' values in block order.
template <int ADD, bool DOT>
__global__ __launch_bounds__(SPMV_THREADS, SPMV_MINWAVES) void spmv_csr_rowblock_idx8_kernel(
    const int2 *__restrict__ rowblk, int nblocks, const int *__restrict__ ai, const unsigned char *__restrict__ idx8,
    const int *__restrict__ offtab_g, int ntab, const double *__restrict__ aa, const double *__restrict__ x,
    const double *yin, double *yout, double *__restrict__ dotpart, int pairsum) {
  __shared__ double prod[SPMV_BLOCK_NNZ];
  __shared__ unsigned char rowof[SPMV_BLOCK_NNZ];
  __shared__ int offtab[256];
  static_assert(!(DOT && ADD != 0), "the x'y by-product is provided for y = A x only");
  const int lb = rowblock_of_workgroup(SPMV_CH);
  if (lb >= nblocks) return;
  const int2 b0 = rowblk[lb];
  const int2 b1 = rowblk[lb + 1];
  const int r0 = b0.x, r1 = b1.x, k0 = b0.y, k1 = b1.y;
  const int nnz = k1 - k0;
  const int nrows = r1 - r0;
  const int tid = threadIdx.x;
  const int tabv = offtab_g[tid];   // 256 initialised entries (zeros past ntab)
  (void)ntab;
  // No block of this kernel exceeds the stage: a row of more than SPMV_BLOCK_CAP nonzeros makes the analysis decline
  // (spmv_compress_indices: nlong), and such a plan runs the plain kernel.
  if (nnz == 0) {               // only empty rows
    if (tid < nrows) yout[r0 + tid] = spmv_empty<ADD>(ADD ? yin[r0 + tid] : 0.0);
    if (DOT && tid == 0) dotpart[lb] = 0.0;
    return;
  }

  const row_lanes rl = lanes_per_row(nrows, nnz, tid);
  const int tpr = rl.tpr, r = rl.r, sub = rl.sub;
  const int rc = r < nrows ? r : nrows - 1;
  const int a0 = ai[r0 + rc], a1 = ai[r0 + rc + 1];
  double ysum = 0.0;
  if (ADD) ysum = yin[r0 + rc];
  double xrow = 0.0;
  if (DOT) xrow = x[r0 + rc];   // square matrix: x entry of this lane's row, for the x'y by-product
  // this lane's slice of the value / index streams
  v2d v[SPMV_PAIRS];
  unsigned int ix[SPMV_PAIRS];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) {
    v[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
    ix[p] = load_pair<unsigned short>(idx8, k0, k1, pair_k(k0, tid, p));
  }
  const int rs = r < nrows ? a0 - k0 : 0, re = r < nrows ? a1 - k0 : 0;
  // row markers: the lanes of row r tag its nonzeros
  for (int k = rs + sub; k < re; k += tpr) rowof[k] = (unsigned char)r;
  offtab[tid] = tabv;
  __syncthreads();
  double xa[SPMV_PAIRS], xb[SPMV_PAIRS];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) {
    const pair_src s = pair_source(pair_k(k0, tid, p), k0, k1);
    xa[p] = x[r0 + rowof[s.kk + s.s0 - k0] + offtab[(ix[p] >> (8 * s.s0)) & 0xff]];
    xb[p] = x[r0 + rowof[s.kk + s.s1 - k0] + offtab[(ix[p] >> (8 * s.s1)) & 0xff]];
  }
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(prod, pair_k(k0, tid, p), k0, k1, v[p].x * xa[p], v[p].y * xb[p]);
  __syncthreads();
  // this lane's row result (lanes without a row: 0)
  const double yval = row_result_lds<ADD>(prod, tpr, sub, r < nrows, rs, re, ysum, 1.0, pairsum, yout + r0 + rc, false);
  if (DOT) {
    const double t = workgroup_sum_ordered<SPMV_WAVES>((r < nrows && sub == 0) ? yval * xrow : 0.0);
    if (tid == 0) dotpart[lb] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// Row-pattern variant for stencil matrices.  When the rows' offset lists (col - row, in column order) come from a small
// dictionary -- 27 lists of <= 7 offsets for the 7-point operator on a box: interior rows and the boundary cases -- the
// analysis stores, per ROW, one 4-byte word -- where its list starts in a table, and the row's first nonzero relative to its row
// block -- and nothing per nonzero; the row pointer is not read at all (a table entry carries its list's length).
// Run-coded blocks: along a row block of a stencil matrix the pattern changes a few times only (a block of P7(256) is one x-line:
// first row, 254 interior rows, last row), and inside a run of equal patterns a row's first nonzero is the run's plus
// (row - run's first row) * length.  The analysis therefore describes each block by up to SPMV_RUNS runs in one 32-byte
// descriptor, indexed by block like rowblk -- the same kind of workgroup-uniform load, issued with it, no new dependent load --
// and a lane finds its run with SPMV_RUNS - 1 compares instead of loading its row word: the kernel streams the values (8 B per
// nonzero) and 32 B per block where it streamed 4 B per row (1024 B per full block).  SPMV_RUNS = 4: an x-line needs 3 runs, a
// block that crosses from one line into the next (line lengths that are no multiple of 256) needs 4 -- interior, last, first,
// interior -- and 4 runs of {row word of the run's first row, first row : 16 | length : 16} are 32 bytes, one aligned 8-dword load;
// the length travels with the run, so a run-coded lane does not read it from LDS either.  Unused runs start at row 0xffff, which no lane
// reaches; a block with more runs (many short lines per block, irregular patterns) has no run at row 0 and reads the row words,
// which stay complete for every row.
// Work layout: the block's values go to LDS with coalesced 16-byte loads; after ONE
// barrier lane r owns row r and gathers x[row + offset_q] itself -- for a fixed q the lanes of a wavefront read
// consecutive x entries (the rows are consecutive, the offsets equal), so the gathers are coalesced, which the per-nonzero
// layouts above cannot offer -- multiplies with the staged values and adds in column order (or two at a time, pairsum):
// the arithmetic and order of the other kernels, same bits.  No row markers, no per-nonzero index stream, one barrier less.
// DOT as in the idx8 kernel; ch: run length of the block -> XCD map (mi355x_spmv_plan_compress_indices); pruns == nullptr: row words only.
#define SPMV_PAT_CAP 512
#define SPMV_RUNS 4
#define SPMV_RUN_WORDS (2 * SPMV_RUNS)     // per row block: SPMV_RUNS x {row word of the run's first row, first row : 16 | length : 16}
#define SPMV_RUN_NONE 0xffffu              // first row of an unused run
static_assert(SPMV_RUNS == 4, "the kernel loads a block's runs as two uint4");
template <int ADD, bool DOT>
__global__ __launch_bounds__(SPMV_THREADS, SPMV_MINWAVES) void spmv_csr_rowblock_pat_kernel(
    const int2 *__restrict__ rowblk, int nblocks, const unsigned int *__restrict__ prow, const uint4 *__restrict__ pruns,
    const int *__restrict__ pattab_g, const double *__restrict__ aa, const double *__restrict__ x, const double *yin, double *yout,
    double *__restrict__ dotpart, int pairsum, int ch, int nty) {
  __shared__ double vs[SPMV_BLOCK_NNZ];
  __shared__ int pattab[SPMV_PAT_CAP];
  const int lb = rowblock_of_workgroup(ch);
  if (lb >= nblocks) return;
  const int2 b0 = rowblk[lb];
  const int2 b1 = rowblk[lb + 1];
  uint4 d0 = make_uint4(0u, SPMV_RUN_NONE, 0u, SPMV_RUN_NONE), d1 = d0;   // the block's runs (workgroup-uniform)
  if (pruns) { d0 = pruns[2 * (size_t)lb]; d1 = pruns[2 * (size_t)lb + 1]; }
  const int r0 = b0.x, r1 = b1.x, k0 = b0.y, k1 = b1.y;
  const int nrows = r1 - r0;
  const int tid = threadIdx.x;
  const int t0 = pattab_g[tid], t1 = pattab_g[tid + SPMV_THREADS];     // SPMV_PAT_CAP initialised entries
  if (k1 == k0) {               // only empty rows
    if (tid < nrows) yout[r0 + tid] = spmv_empty<ADD>(ADD ? yin[r0 + tid] : 0.0);
    if (DOT && tid == 0) dotpart[lb] = 0.0;
    return;
  }
  const int rc = tid < nrows ? tid : nrows - 1;
  const bool coded = (d0.y & 0xffffu) == 0u;      // run-coded block: its first run starts at row 0
  // this lane's run, the last one that starts at or before its row: pw = {where the row's list starts in the table : 16, first nonzero
  // in the block : 16} of the run's first row, rn = {the run's first row : 16, length : 16}.  Selects on uniform values and no branch
  // around them; a block without runs holds unused runs only (length 0, so the row's offset in its run below is 0) and loads its row's word.
  unsigned int pw = d0.x, rn = d0.y;
  if ((unsigned int)rc >= (d0.w & 0xffffu)) { pw = d0.z; rn = d0.w; }
  if ((unsigned int)rc >= (d1.y & 0xffffu)) { pw = d1.x; rn = d1.y; }
  if ((unsigned int)rc >= (d1.w & 0xffffu)) { pw = d1.z; rn = d1.w; }
  if (!coded) pw = prow[r0 + rc];
  const int pst = (int)(pw & 0xffffu);
  const int rs = (int)(pw >> 16) + (rc - (int)(rn & 0xffffu)) * (int)(rn >> 16);
  double ysum = 0.0;
  if (ADD) ysum = yin[r0 + rc];
  v2d v[SPMV_PAIRS];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) v[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
  pattab[tid] = t0;
  pattab[tid + SPMV_THREADS] = t1;
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(vs, pair_k(k0, tid, p), k0, k1, v[p].x, v[p].y);
  __syncthreads();
  if (!DOT && tid >= nrows) return;
  const int len = tid < nrows ? (coded ? (int)(rn >> 16) : pattab[pst]) : 0;   // table entry: {length, offsets ...}
  const long xbase = (long)r0 + rc;
  double sum = (ADD == 1) ? ysum : 0.0;
  for (int q0 = 0; q0 < len; q0 += 8) {
    double xv[8], av[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int qq = (q0 + j < len) ? q0 + j : len - 1;
      xv[j] = x[xbase + pattab[pst + 1 + qq]];
      av[j] = vs[rs + qq];
    }
    sum = accumulate8(sum, q0, len, pairsum, [&](int j) { return av[j] * xv[j]; });
  }
  const double yv = spmv_fin<ADD>(ysum, sum);
  if (tid < nrows) spmv_store(yout + r0 + tid, yv, nty);
  if (DOT) {
    const double t = workgroup_sum_ordered<SPMV_WAVES>(tid < nrows ? yv * x[xbase] : 0.0);
    if (tid == 0) dotpart[lb] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// Value-pattern variant for constant-coefficient operators (value indexing in the sense of CSR-VI, taken per row).  When
// whole rows repeat -- the same offsets AND bit-for-bit the same values: the 27 row kinds of the 7-point operator on a
// box, any stencil with constant coefficients -- the analysis keeps ONE copy of each distinct row {length, offsets, values}
// in a table of at most SPMV_PAT_CAP entries and 2 bytes per ROW saying which; the value array is not read at all.  The
// kernel streams 2 B + y per row and gathers x (coalesced: consecutive lanes own consecutive rows, see the row-pattern
// kernel); products and their order are those of the other kernels, so the result carries the same bits.  The table
// describes the values it was derived from: every path that changes values on the device drops it
// (mi355x_spmv_plan_drop_value_patterns), every upload derives it again.
// What bounds it is not memory: rocprofv3 counts 0.36 GB per launch on P7(256) (ideal 0.30: x once, y once, 2 B per row; x is
// fetched 1.45 times, neighbouring planes by more than one XCD's L2) at 3.3 TB/s.  The launch is a latency chain -- row word -> table -> gathers -> store -- run by as many wavefronts as a CU holds:
// probe builds take 0.046 ms with every global access removed and 0.02-0.04 ms more for each of the three phases.  Per nonzero
// the work is therefore kept minimal (table entries padded to a multiple of 8 slots and holding BYTE offsets, a gather's
// address = the uniform base of x + one 32-bit add, no index clamped; stores after all of a lane's rows, because loads and
// stores share one in-order completion counter).  Measured and not kept, all within +-10 % of this form or slower: an LDS copy
// of the x window around the block's rows for the near offsets, all of a lane's gathers issued before any is used, two
// adjacent rows per lane with 16-byte gathers, wavefront tiles of 512 rows with one 16-byte word load per lane, a persistent
// grid walking the rows, an XCD-contiguous block map, wavefront-uniform table entries through scalar registers.
#ifndef SPMV_VPAT_RPL
#define SPMV_VPAT_RPL 4       // rows per lane (inside the CG iteration on P7(256): 1 -> 0.127 ms, 2 -> 0.116, 4 -> 0.106, 8 -> 0.107)
#endif
#define SPMV_VPAT_ROWS (SPMV_VPAT_RPL * SPMV_THREADS)      // rows per workgroup
#define SPMV_VPAT_MAXROWS (1 << 28)                        // 32-bit byte offsets into x

// one row out of the table, the other kernels' arithmetic and order; rb8 = 8 * row, xb = x as bytes
__device__ __forceinline__ double vpat_row(const int *pattab, const double *patval, int ps, unsigned int rb8, const char *__restrict__ xb,
                                           double sum, int pairsum) {
  const int len = pattab[ps];                      // table entry: {length, byte offsets ... (padded to 8 k slots)}; values at the offsets' indices
  for (int q0 = 0; q0 < len; q0 += 8) {
    double xv[8], av[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {                  // the gathers are what the launch pays for (texture addresser 76 % busy): a slot beyond
      xv[i] = 0.0;                                 // the row's length is not loaded -- and not issued at all when no lane of the wavefront needs it
      if (q0 + i < len) xv[i] = *reinterpret_cast<const double *>(xb + (unsigned int)(rb8 + (unsigned int)pattab[ps + 1 + q0 + i]));
      av[i] = patval[ps + 1 + q0 + i];
    }
    sum = accumulate8(sum, q0, len, pairsum, [&](int i) { return av[i] * xv[i]; });   // (each product where it is added: nothing waits between the guarded gathers)
  }
  return sum;
}

template <int ADD, bool DOT>
__global__ __launch_bounds__(SPMV_THREADS) void spmv_csr_valpat_kernel(
    int nrows, const unsigned short *__restrict__ vrow, const int *__restrict__ pattab_g, const double *__restrict__ patval_g, int tablen,
    const double *__restrict__ x, const double *yin, double *yout, double *__restrict__ dotpart, int pairsum) {
  __shared__ int pattab[SPMV_PAT_CAP];
  __shared__ double patval[SPMV_PAT_CAP];
  const int tid = threadIdx.x;
  for (int t = tid; t < tablen; t += SPMV_THREADS) { pattab[t] = pattab_g[t]; patval[t] = patval_g[t]; }
  const long rbase = (long)blockIdx.x * SPMV_VPAT_ROWS + tid;          // the grid covers the rows exactly: no block without one
  int pst[SPMV_VPAT_RPL];
  double yv[SPMV_VPAT_RPL];
#pragma unroll
  for (int j = 0; j < SPMV_VPAT_RPL; ++j) {
    const long row = rbase + (long)j * SPMV_THREADS;
    const long rc = row < nrows ? row : (long)nrows - 1;
    pst[j] = vrow[rc];
    yv[j] = ADD == 2 ? __builtin_nontemporal_load(yin + rc) : (ADD ? yin[rc] : 0.0);   // ADD == 2: the Jacobi diagonal, a stream read once per product
  }
  __syncthreads();
  const char *xb = reinterpret_cast<const char *>(x);
  // the stores wait until every row of the lane has its sum: loads and stores share one in-order completion counter on this
  // ISA, so a store issued between two rows' gathers would put its acknowledgement (an HBM round trip) on the second row's path
  double res[SPMV_VPAT_RPL];
#pragma unroll
  for (int j = 0; j < SPMV_VPAT_RPL; ++j) {
    const long row = rbase + (long)j * SPMV_THREADS;
    res[j] = 0.0;
    if (row < nrows) res[j] = spmv_fin<ADD>(yv[j], vpat_row(pattab, patval, pst[j], (unsigned int)row * 8u, xb, (ADD == 1) ? yv[j] : 0.0, pairsum));
  }
#pragma unroll
  for (int j = 0; j < SPMV_VPAT_RPL; ++j) {
    const long row = rbase + (long)j * SPMV_THREADS;
    if (row < nrows) yout[row] = res[j];
  }
  if (DOT) {   // x_r y_r over the workgroup's rows: a lane's rows in order, then the fixed tree of the other kernels
    double c = 0.0;
#pragma unroll
    for (int j = 0; j < SPMV_VPAT_RPL; ++j) {
      const long row = rbase + (long)j * SPMV_THREADS;
      if (row < nrows) c += res[j] * x[row];
    }
    const double t = workgroup_sum_ordered<SPMV_WAVES>(c);
    if (tid == 0) dotpart[blockIdx.x] = t;
  }
}

// ---------------------------------------------------------------------------------------------
// Grouped-row variant: the MI355X form of the reference's inodes (Mat_CheckInode inode.c:3964-4034,
// MatMult_SeqAIJ_Inode inode.c:392-578).  Consecutive rows with one and the same column pattern -- the dof rows of
// one node of a finite-element matrix -- form a group whose column list is stored ONCE (gj); the value array is the
// untouched CSR `a`.  A 3-dof matrix streams 8 + 4/3 bytes per nonzero instead of 12.  Work layout as above: row
// blocks of whole groups (<= 256 rows, <= 2046 nonzeros, <= SPMV_GJ_CAP shared column indices), values streamed with
// coalesced 16-byte loads, the block's column lists staged in LDS by one coalesced load, and the column of nonzero k
// looked up as gjs[rbase[row(k)] + k] with row(k) from the LDS marker array the row-owning lanes write (a per-nonzero
// 16-bit marker that saves one LDS level was measured 5 % slower: 0.252 against 0.239 ms on the FEM stand-in).  Row sums as in
// the other kernels (pairsum: the inode routine's two-at-a-time order, so the result carries the reference's bits).
template <int ADD>
__global__ __launch_bounds__(SPMV_THREADS, SPMV_MINWAVES) void spmv_csr_rowblock_inode_kernel(
    const int4 *__restrict__ rowblk, int nblocks, const int *__restrict__ ai, const int *__restrict__ goff,
    const int *__restrict__ gj, const double *__restrict__ aa, const double *__restrict__ x, const double *yin, double *yout,
    int pairsum) {
  __shared__ double prod[SPMV_BLOCK_NNZ];
  __shared__ int gjs[SPMV_GJ_CAP + 2];               // +2: parking slots for the halves of a pair outside the block
  __shared__ int rbase[SPMV_BLOCK_ROWS];             // per row: its nonzero e of the block has column gjs[rbase + e]
  __shared__ unsigned char rowof[SPMV_BLOCK_NNZ];    // per nonzero of the block: its row (written by the lanes that own the row)
  static_assert(SPMV_GJ_CAP + 2 <= 4 * SPMV_THREADS, "index staging: two int2 loads per lane");
  const int lb = rowblock_of_workgroup(SPMV_CH);
  if (lb >= nblocks) return;
  const int4 b0 = rowblk[lb];
  const int4 b1 = rowblk[lb + 1];
  const int r0 = b0.x, r1 = b1.x, k0 = b0.y, k1 = b1.y, g0 = b0.z, g1 = b1.z;
  const int nnz = k1 - k0;
  const int nrows = r1 - r0;
  const int tid = threadIdx.x;
  if (nnz == 0) {               // only empty rows
    if (tid < nrows) yout[r0 + tid] = spmv_empty<ADD>(ADD ? yin[r0 + tid] : 0.0);
    return;
  }
  const row_lanes rl = lanes_per_row(nrows, nnz, tid);
  const int tpr = rl.tpr, r = rl.r, sub = rl.sub;
  const int rc = r < nrows ? r : nrows - 1;
  const int a0 = ai[r0 + rc], a1 = ai[r0 + rc + 1];
  const int go = goff[r0 + rc];
  double ysum = 0.0;
  if (ADD) ysum = yin[r0 + rc];
  // this lane's slices of the value stream and of the block's shared column lists [g0, g1)
  v2d v[SPMV_PAIRS];
  v2i gv[2];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) v[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
#pragma unroll
  for (int q = 0; q < 2; ++q) gv[q] = load_pair<v2i>(gj, g0, g1, pair_k(g0, tid, q));
  const int rs = r < nrows ? a0 - k0 : 0, re = r < nrows ? a1 - k0 : 0;
  for (int k = rs + sub; k < re; k += tpr) rowof[k] = (unsigned char)r;
  if (r < nrows && sub == 0) rbase[r] = (go - g0) - rs;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int g = pair_k(g0, tid, q);
    gjs[(g >= g0 && g < g1) ? g - g0 : SPMV_GJ_CAP] = gv[q].x;
    gjs[(g + 1 < g1) ? g + 1 - g0 : SPMV_GJ_CAP + 1] = gv[q].y;
  }
  __syncthreads();
  double xa[SPMV_PAIRS], xb[SPMV_PAIRS];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) {
    const pair_src s = pair_source(pair_k(k0, tid, p), k0, k1);
    const int e0 = s.kk + s.s0 - k0, e1 = s.kk + s.s1 - k0;   // elements of this block to take the columns from
    xa[p] = x[gjs[rbase[rowof[e0]] + e0]];
    xb[p] = x[gjs[rbase[rowof[e1]] + e1]];
  }
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(prod, pair_k(k0, tid, p), k0, k1, v[p].x * xa[p], v[p].y * xb[p]);
  __syncthreads();
  row_result_lds<ADD>(prod, tpr, sub, r < nrows, rs, re, ysum, 1.0, pairsum, yout + r0 + rc, false);
}

// ---------------------------------------------------------------------------------------------
// BCSR (MatMult_SeqBAIJ_3/_4/_N, reference src/mat/impls/baij/seq/baij2.c:331-436,981) with the same
// row-block streaming structure: the plan is built over the block-row pointer scaled by bs*bs (so it
// counts values), a workgroup streams <= 2046 values of consecutive block rows with 16-byte loads,
// looks the block column up once per value (e / bs^2), multiplies by x[col*bs + c] and parks the
// products in LDS; point row (br, r) then owns the LDS entries s + bs*j + r, j < nblocks*bs
// (blocks are column-major, baij.h:13-30) and is summed by 1..64 lanes + a shuffle tree.
// XLDS: the x entries of the row block's block columns are staged in LDS ONCE per block (bs doubles per stored block, requested
// together with the value stream, before the barrier) and the products read them from there: bs^2 values share bs staged entries,
// so the global gathers drop from one per value to one per bs values, and none of them sits behind the barrier.
#ifndef MI355X_BSR_XLDS_DEFAULT
#define MI355X_BSR_XLDS_DEFAULT 1   // measured at 128^3 nodes (profiles/r03_cfg5.log): bs = 3 0.781 -> 0.728 ms, bs = 4 1.420 -> 1.290 ms; same bits
#endif
template <int BS, bool XLDS>
__global__ __launch_bounds__(SPMV_THREADS) void bsr_rowblock_kernel(const int2 *__restrict__ rowblk, int nblocks,
                                                                   const int *__restrict__ ai, const int *__restrict__ aj,
                                                                   const double *__restrict__ aa,
                                                                   const double *__restrict__ x, const double *yin, double *y) {
  // yin != NULL: y = yin + A x (MatMultAdd_SeqBAIJ_N, baij2.c:1168-1480; y may alias yin: every point row is read and written by one lane)
  __shared__ double prod[SPMV_BLOCK_NNZ];
  __shared__ int ajs[XLDS ? 1 : SPMV_BLOCK_NNZ / 4 + 1];   // block columns of the row block (bs >= 2: at most NNZ/4 blocks)
  __shared__ double xs[XLDS ? (SPMV_BLOCK_NNZ / (BS * BS) + 1) * BS : 1];   // XLDS: x[bs * col .. + bs) of every stored block
  constexpr int BS2 = BS * BS;
  // the CSR kernels' block -> XCD map: a block column's x entries are pulled into ONE XCD's L2 instead of all eight (PMC at
  // 128^3 nodes: 4.75 GB fetched for 4.35 GB without it)
  const int lb = rowblock_of_workgroup(SPMV_CH);
  if (lb >= nblocks) return;
  const int2 b0 = rowblk[lb];
  const int2 b1 = rowblk[lb + 1];
  const int r0 = b0.x, r1 = b1.x, k0 = b0.y, k1 = b1.y;   // block rows [r0,r1), values [k0,k1)
  const int tid = threadIdx.x;
  const int nv = (r1 - r0) * BS;                           // point rows of this workgroup
  if (k1 - k0 > SPMV_BLOCK_CAP) {
    // one block row wider than the LDS stage: strided partial sums per point row, tree at the end
    double acc[BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) acc[r] = 0.0;
    for (int e = k0 + tid; e < k1; e += SPMV_THREADS) {
      const int blk = e / BS2, q = e - blk * BS2, c = q / BS, r = q - c * BS;
      const double p = SPMV_LOAD(aa + e) * x[(long)aj[blk] * BS + c];
#pragma unroll
      for (int rr = 0; rr < BS; ++rr) acc[rr] += (rr == r) ? p : 0.0;
    }
    __shared__ double part[SPMV_WAVES][BS];
#pragma unroll
    for (int r = 0; r < BS; ++r) { double v = wave_sum(acc[r]); if ((tid & 63) == 0) part[tid / 64][r] = v; }
    __syncthreads();
    if (tid < BS) { double t = part[0][tid]; for (int w = 1; w < SPMV_WAVES; ++w) t += part[w][tid]; y[(long)r0 * BS + tid] = yin ? yin[(long)r0 * BS + tid] + t : t; }
    return;
  }
  if (k1 == k0) {   // only empty block rows: up to SPMV_BLOCK_ROWS of them, i.e. up to BS times as many point rows as lanes
    for (int v = tid; v < nv; v += SPMV_THREADS) y[(long)r0 * BS + v] = yin ? yin[(long)r0 * BS + v] : 0.0;
    return;
  }
  const row_lanes rl = lanes_per_row(nv, 0, tid, false);   // (no one-lane rule: point rows are summed with stride bs whatever their length)
  // extents of this lane's point row, requested before the stream
  const int tpr = rl.tpr, v = rl.r, sub = rl.sub;
  const int vc = v < nv ? v : nv - 1;
  const int br = r0 + vc / BS;
  const int rr_ = vc - (vc / BS) * BS;
  const int a0 = ai[br], a1 = ai[br + 1];
  // block columns of this row block: one coalesced load into LDS instead of a global gather per value (a block's bs^2
  // values share one entry); k0 is a multiple of bs^2 because row blocks start at block-row boundaries
  const int kb0 = k0 / BS2, nblk = (k1 - k0) / BS2;
  v2d vv[SPMV_PAIRS];
  if (XLDS) {
    // the value stream first (it is the long pole), then one block column per lane and its bs x entries
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) vv[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
    for (int b = tid; b < nblk; b += SPMV_THREADS) {
      const long c = (long)aj[kb0 + b] * BS;
#pragma unroll
      for (int q = 0; q < BS; ++q) xs[b * BS + q] = x[c + q];
    }
  } else {
    for (int b = tid; b < nblk; b += SPMV_THREADS) ajs[b] = aj[kb0 + b];
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) vv[p] = load_pair<v2d>(aa, k0, k1, pair_k(k0, tid, p));
  }
  __syncthreads();
  double xa[SPMV_PAIRS], xb[SPMV_PAIRS];
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) {
    const pair_src s = pair_source(pair_k(k0, tid, p), k0, k1);
    const int f0 = s.kk + s.s0 - k0, f1 = s.kk + s.s1 - k0;   // value index each half takes its block column from
    const int blk0 = f0 / BS2, blk1 = f1 / BS2;
    if (XLDS) {
      xa[p] = xs[blk0 * BS + (f0 - blk0 * BS2) / BS];
      xb[p] = xs[blk1 * BS + (f1 - blk1 * BS2) / BS];
    } else {
      xa[p] = x[(long)ajs[blk0] * BS + (f0 - blk0 * BS2) / BS];
      xb[p] = x[(long)ajs[blk1] * BS + (f1 - blk1 * BS2) / BS];
    }
  }
#pragma unroll
  for (int p = 0; p < SPMV_PAIRS; ++p) park_pair(prod, pair_k(k0, tid, p), k0, k1, vv[p].x * xa[p], vv[p].y * xb[p]);
  __syncthreads();
  const int s = a0 * BS2 - k0;
  const int cnt = v < nv ? (a1 - a0) * BS : 0;
  double sum = 0.0;
  for (int j = sub; j < cnt; j += tpr) sum += prod[s + BS * j + rr_];
  for (int off = tpr >> 1; off > 0; off >>= 1) sum += __shfl_down(sum, off, MI355X_WAVE);
  // (a block row without blocks is yin itself, as in the only-empty block above: yin + 0.0 would turn yin = -0.0 into +0.0)
  if (v < nv && sub == 0) y[(long)br * BS + rr_] = yin ? (cnt ? yin[(long)br * BS + rr_] + sum : yin[(long)br * BS + rr_]) : sum;
  // block rows with very few blocks: the row block can hold more point rows than the workgroup has lanes
  // (<= 256 block rows x bs); the remaining ones are summed the same way, one lane per point row (tpr is 1 here)
  for (int v2 = tid + SPMV_THREADS; v2 < nv; v2 += SPMV_THREADS) {
    const int br2 = r0 + v2 / BS, rr2 = v2 - (v2 / BS) * BS;
    const int b0_ = ai[br2], b1_ = ai[br2 + 1];
    const int s2 = b0_ * BS2 - k0, cnt2 = (b1_ - b0_) * BS;
    double sum2 = 0.0;
    for (int j = 0; j < cnt2; ++j) sum2 += prod[s2 + BS * j + rr2];
    y[(long)br2 * BS + rr2] = yin ? (cnt2 ? yin[(long)br2 * BS + rr2] + sum2 : yin[(long)br2 * BS + rr2]) : sum2;
  }
}

// sum of the per-row-block x'y values in block order: 1024 lanes stride over them, fixed tree
__global__ __launch_bounds__(1024) void dot_partials_kernel(const double *__restrict__ part, int n, double *out) {
  // eight loads in flight per lane (one dependent load per step took 22 us for the 57 K values of P7(256)); a fixed order of
  // additions whatever n is: lane t owns values t, t + 1024, ..., added eight accumulators wide, the accumulators in a fixed tree
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
  int i = threadIdx.x;
  for (; i + 7 * 1024 < n; i += 8 * 1024) {
    const double v0 = part[i], v1 = part[i + 1024], v2 = part[i + 2 * 1024], v3 = part[i + 3 * 1024];
    const double v4 = part[i + 4 * 1024], v5 = part[i + 5 * 1024], v6 = part[i + 6 * 1024], v7 = part[i + 7 * 1024];
    a0 += v0; a1 += v1; a2 += v2; a3 += v3; a4 += v4; a5 += v5; a6 += v6; a7 += v7;
  }
  for (; i < n; i += 1024) a0 += part[i];
  const double t = workgroup_sum_ordered<1024 / MI355X_WAVE>(((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7)));
  if (threadIdx.x == 0) out[0] = t;
}

// Value assembly through a precomputed map (MatSetValuesBatch with an unchanged pattern): nonzero `segslot[s]` receives
// the contributions v[order[k]], k in [segptr[s], segptr[s+1]), added to its current value one after the other in the
// order the reference's loop of MatSetValues(ADD_VALUES) would add them (matrix.c:1715-1718) -- one lane per nonzero,
// no atomics, same bits as the host loop.
__global__ __launch_bounds__(MI355X_BLOCK) void csr_assemble_kernel(int nseg, const int *__restrict__ segptr, const int *__restrict__ segslot,
                                                                   const int *__restrict__ order, const double *__restrict__ v, double *aa) {
  const int s = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (s >= nseg) return;
  const int slot = segslot[s];
  double sum = aa[slot];
  for (int k = segptr[s]; k < segptr[s + 1]; ++k) sum += v[order[k]];
  aa[slot] = sum;
}

// MatDiagonalScale_SeqAIJ (aij.c:2055-2092): a[k] = (a[k] * l[row]) * r[col]; either vector may be absent.  One lane per row.
__global__ __launch_bounds__(MI355X_BLOCK) void csr_diagscale_kernel(int m, const int *__restrict__ ai, const int *__restrict__ aj,
                                                                    double *aa, const double *__restrict__ l, const double *__restrict__ r) {
  const int row = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (row >= m) return;
  const double lv = l ? l[row] : 1.0;
  for (int k = ai[row]; k < ai[row + 1]; ++k) {
    double v = aa[k];
    if (l) v = v * lv;
    if (r) v = v * r[aj[k]];
    aa[k] = v;
  }
}

__global__ __launch_bounds__(MI355X_BLOCK) void csr_diag_kernel(int m, const int *__restrict__ ai,
                                                               const int *__restrict__ aj,
                                                               const double *__restrict__ aa, double *d) {
  int r = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (r >= m) return;
  double v = 0.0;
  for (int k = ai[r]; k < ai[r + 1]; ++k) {
    if (aj[k] == r) { v = aa[k]; break; }
  }
  d[r] = v;
}

// MatShift (axpy.c:170-200) with an unchanged pattern: a[k] = a[k] + alpha at the diagonal entry of every row, found by
// csr_diag_kernel's search.  A row without one is counted (when a counter is given) and not touched.  One lane per row.
__global__ __launch_bounds__(MI355X_BLOCK) void csr_shift_kernel(int m, const int *__restrict__ ai, const int *__restrict__ aj,
                                                                double alpha, double *aa, int *nmissing) {
  int r = blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (r >= m) return;
  for (int k = ai[r]; k < ai[r + 1]; ++k) {
    if (aj[k] == r) { aa[k] = aa[k] + alpha; return; }
  }
  if (nmissing) atomicAdd(nmissing, 1);
}

// MatAXPY_SeqAIJ with SUBSET_NONZERO_PATTERN (aij.c:2621-2640): ya[xtoy[k]] = ya[xtoy[k]] + alpha * xa[k], product and sum rounded
// separately.  xtoy is injective: one lane per entry of X, plain loads and stores.  xa may be ya (X == Y, the identity map).
__global__ __launch_bounds__(MI355X_BLOCK) void csr_axpy_map_kernel(int nzx, const int *__restrict__ xtoy, double alpha,
                                                                   const double *xa, double *ya) {
  const long k = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  if (k >= nzx) return;
  const int t = xtoy[k];
  ya[t] = ya[t] + alpha * xa[k];
}

// MatZeroRows_SeqAIJ with the pattern kept (aij.c): every stored entry of a listed row becomes +0.0 -- a store, so whatever was there is
// gone -- and the diagonal entry becomes diag when diag != 0 (-0.0 counts as zero, NaN does not).  Each entry is written exactly once with
// its final value: there is no zeroing pass and diagonal pass to order.  A group of ZR_GROUP lanes per listed row loops over the row;
// the group's first lane writes b[row] = diag * x[row].  A row listed twice is written twice with the same values.
// ZR_GROUP = 16: the rows this serves (boundary rows of stencil and FEM matrices) hold 5 to ~80 entries, so a group needs one to a few
// steps, and one step of a group covers one 128-byte line of the value array; a wavefront per row would idle three quarters of its
// lanes on a 7-point row, a lane per row would write 8 bytes per line touched.
#define ZR_GROUP 16
static_assert(MI355X_BLOCK % ZR_GROUP == 0 && MI355X_WAVE % ZR_GROUP == 0, "whole groups per wavefront");
__global__ __launch_bounds__(MI355X_BLOCK) void csr_zero_rows_kernel(int nrows, const int *__restrict__ rows, const int *__restrict__ ai,
                                                                    const int *__restrict__ aj, double *aa, double diag,
                                                                    const double *__restrict__ x, double *b) {
  const long t = (long)blockIdx.x * MI355X_BLOCK + threadIdx.x;
  const long g = t / ZR_GROUP;
  const int sub = (int)(t % ZR_GROUP);
  if (g >= nrows) return;
  const int row = rows[g];
  const bool set = diag != 0.0;
  const int end = ai[row + 1];
  for (int k = ai[row] + sub; k < end; k += ZR_GROUP) aa[k] = (set && aj[k] == row) ? diag : 0.0;
  if (sub == 0 && b) b[row] = diag * x[row];
}

// The column half of MatZeroRowsColumns_SeqAIJ (aij.c): in every row i that is NOT listed, an entry whose column is listed gives
// b[i] = b[i] - a_ij * x[col] (product and difference rounded separately, in stored column order) and becomes +0.0.  Listed rows and
// columns are the same set (square matrix), kept as a bitmap on the device: one bit per column, 2 MiB for 16.8 M columns, so the
// gathers of a sweep stay in the L2 where a byte map (16 MiB) or the list itself (a search per entry) would not.
// The matrix's own row-block plan: a workgroup sweeps its block's column indices with the family's unconditional pair loads and tests
// the bitmap.  A block without a hit -- almost every block when the listed rows are a boundary -- leaves after that sweep: it has read
// its indices and a few bitmap words, never a, x or b, and has written nothing.  In a block with hits the sweeping lane parks
// a_ij * x[col] in the entry's LDS slot and marks the slot; after one barrier lane r, owner of row r as in the SpMV family, walks its
// row's slots in column order, subtracts the parked products from b[r] one after the other -- the reference's bits -- and stores the
// +0.0 (the owner knows whether its row is listed; the sweeping lane does not know the entry's row).  No atomics anywhere; rows of a
// block belong to one workgroup, so b[r] has one writer.  Listed rows are left to csr_zero_rows_kernel.
__device__ __forceinline__ bool zc_listed(const unsigned *__restrict__ mask, int c) { return (mask[c >> 5] >> (c & 31)) & 1u; }
#define ZC_PER_LANE (SPMV_BLOCK_NNZ / SPMV_THREADS)
// entry e of lane tid in the chunk [c0, c1) of the stream: the halves of the lane's pairs (VEC), else a stride of the workgroup's width
template <bool VEC> __device__ __forceinline__ int zc_entry_k(int c0, int tid, int e) {
  return VEC ? pair_k(c0, tid, e >> 1) + (e & 1) : c0 + tid + e * SPMV_THREADS;
}
// Sweep of one chunk of at most SPMV_BLOCK_NNZ entries (VEC: at most SPMV_BLOCK_CAP, any alignment of the first pair).  Returns false on
// every lane when no entry of the chunk has a listed column.  Otherwise hit[k - c0] says whether entry k has, prod[k - c0] holds
// a_k * x[col] for those (x given), and with zero_now the entries hit are already +0.0.  Every lane of the workgroup must call it: one
// voting barrier, and one more when there is a hit.
template <bool VEC>
__device__ __forceinline__ bool zc_sweep(const int *__restrict__ aj, double *aa, const unsigned *__restrict__ mask, const double *__restrict__ x,
                                         int c0, int c1, int tid, double *prod, unsigned char *hit, bool zero_now) {
  int col[ZC_PER_LANE];
  if (VEC) {
#pragma unroll
    for (int p = 0; p < SPMV_PAIRS; ++p) {
      const v2i c = load_pair<v2i>(aj, c0, c1, pair_k(c0, tid, p));
      const pair_src s = pair_source(pair_k(c0, tid, p), c0, c1);   // a half outside the chunk takes a column of the chunk: no gather is predicated
      col[2 * p] = s.s0 ? c.y : c.x;
      col[2 * p + 1] = s.s1 ? c.y : c.x;
    }
  } else {
#pragma unroll
    for (int e = 0; e < ZC_PER_LANE; ++e) { const int k = zc_entry_k<false>(c0, tid, e); col[e] = SPMV_LOAD(aj + (k < c1 ? k : c0)); }
  }
  unsigned h = 0;
#pragma unroll
  for (int e = 0; e < ZC_PER_LANE; ++e) {
    const int k = zc_entry_k<VEC>(c0, tid, e);
    const bool listed = zc_listed(mask, col[e]);
    if (k >= c0 && k < c1 && listed) h |= 1u << e;
  }
  if (!__syncthreads_or(h != 0)) return false;
#pragma unroll
  for (int e = 0; e < ZC_PER_LANE; ++e) {
    const int k = zc_entry_k<VEC>(c0, tid, e);
    if (k >= c0 && k < c1) {
      const bool is = (h >> e) & 1u;
      hit[k - c0] = is;
      if (is) {
        if (x) prod[k - c0] = aa[k] * x[col[e]];
        if (zero_now) aa[k] = 0.0;
      }
    }
  }
  __syncthreads();
  return true;
}
template <bool VEC>
__global__ __launch_bounds__(SPMV_THREADS) void csr_zero_columns_kernel(const int2 *__restrict__ rowblk, int nblocks, const int *__restrict__ ai,
                                                                       const int *__restrict__ aj, double *aa, const unsigned *__restrict__ mask,
                                                                       const double *__restrict__ x, double *b) {
  __shared__ double prod[SPMV_BLOCK_NNZ];
  __shared__ unsigned char hit[SPMV_BLOCK_NNZ];
  const int lb = rowblock_of_workgroup(SPMV_CH);
  if (lb >= nblocks) return;
  const int2 b0 = rowblk[lb];
  const int2 b1 = rowblk[lb + 1];
  const int r0 = b0.x, nrows = b1.x - b0.x, k0 = b0.y, k1 = b1.y;
  const int tid = threadIdx.x;
  if (k1 == k0) return;
  if (k1 - k0 > SPMV_BLOCK_CAP) {
    // one long row, a stage at a time (every branch here is taken by the whole workgroup).  The row is not listed, so the sweeping
    // lanes store the +0.0 themselves; lane 0 carries b[r0] through the stages
    if (zc_listed(mask, r0)) return;
    double bv = 0.0;
    bool touched = false;
    for (int c0 = k0; c0 < k1; c0 += SPMV_BLOCK_NNZ) {
      const int c1 = c0 + SPMV_BLOCK_NNZ < k1 ? c0 + SPMV_BLOCK_NNZ : k1;
      if (!zc_sweep<false>(aj, aa, mask, x, c0, c1, tid, prod, hit, true)) continue;
      if (tid == 0 && b) {
        if (!touched) { bv = b[r0]; touched = true; }
        for (int k = 0; k < c1 - c0; ++k) if (hit[k]) bv = bv - prod[k];
      }
      __syncthreads();   // the next stage overwrites the slots
    }
    if (tid == 0 && touched) b[r0] = bv;
    return;
  }
  if (!zc_sweep<VEC>(aj, aa, mask, x, k0, k1, tid, prod, hit, false)) return;
  if (tid < nrows && !zc_listed(mask, r0 + tid)) {
    const int r = r0 + tid;
    const int rs = ai[r] - k0, re = ai[r + 1] - k0;
    double bv = 0.0;
    bool touched = false;
    for (int k = rs; k < re; ++k) {
      if (!hit[k]) continue;
      if (b) {
        if (!touched) { bv = b[r]; touched = true; }
        bv = bv - prod[k];
      }
      aa[k0 + k] = 0.0;
    }
    if (touched) b[r] = bv;
  }
}

// Which kernel a plan runs with these arrays: the one decision behind mi355x_spmv_csr / _add / _scaled, mi355x_spmv_csr_dot
// and mi355x_spmv_plan_dot_available (CG relies on y carrying the same bits from the first two).  In order of precedence;
// the compressed forms need whole rows (no compressed-row plan) and, all but the value patterns, 16-byte aligned values.
enum spmv_form_t { SPMV_PLAIN_SCALAR, SPMV_PLAIN, SPMV_IDX8, SPMV_ROWPAT, SPMV_GROUPED, SPMV_VALPAT };
static spmv_form_t spmv_form(const mi355x_spmv_plan_s *p, const double *aa, const int *aj, bool plain_only = false) {
  const bool a16 = mi355x_aligned16(aa);
  if (!p->d_rows && !plain_only) {
    if (p->vpat_valid && p->use_vpat) return SPMV_VALPAT;
    if (p->d_gj && a16) return SPMV_GROUPED;
    if (p->d_prow && p->use_pat && a16) return SPMV_ROWPAT;
    if (p->d_idx8 && a16) return SPMV_IDX8;
  }
  return (a16 && (((uintptr_t)aj) & 7u) == 0) ? SPMV_PLAIN : SPMV_PLAIN_SCALAR;   // pair loads of aa and aj, or the scalar stream
}

static inline const uint4 *spmv_runs_of(const mi355x_spmv_plan_s *p) { return p->use_runs ? reinterpret_cast<const uint4 *>(p->d_pruns) : nullptr; }

template <int ADD>
static int launch_spmv(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai, const int *aj, const double *aa,
                       const double *x, const double *yin, double *yout, const double *dsc = nullptr) {
  if (p->nblocks == 0) return 0;
  const dim3 grid(rowblock_grid(p->nblocks, SPMV_CH)), block(SPMV_THREADS);
  const spmv_form_t form = spmv_form(p, aa, aj, ADD == 3);   // (ADD == 3 exists in the plain row-block kernel only)
  if constexpr (ADD != 3) switch (form) {
    case SPMV_VALPAT:
      hipLaunchKernelGGL((spmv_csr_valpat_kernel<ADD, false>), dim3((p->nrows + SPMV_VPAT_ROWS - 1) / SPMV_VPAT_ROWS), block, 0, h->stream,
                         p->nrows, p->d_vrow, p->d_vpattab, p->d_vpatval, p->vtablen, x, yin, yout, (double *)nullptr, p->pairsum);
      break;
    case SPMV_GROUPED:
      hipLaunchKernelGGL((spmv_csr_rowblock_inode_kernel<ADD>), grid, block, 0, h->stream, p->d_rowblk4, p->nblocks,
                         ai, p->d_goff, p->d_gj, aa, x, yin, yout, p->pairsum);
      break;
    case SPMV_ROWPAT:
      hipLaunchKernelGGL((spmv_csr_rowblock_pat_kernel<ADD, false>), dim3(rowblock_grid(p->nblocks, p->ch)), block, 0, h->stream, p->d_rowblk,
                         p->nblocks, p->d_prow, spmv_runs_of(p), p->d_pattab, aa, x, yin, yout, (double *)nullptr, p->pairsum, p->ch, spmv_y_streams(p->nrows));
      break;
    case SPMV_IDX8:
      hipLaunchKernelGGL((spmv_csr_rowblock_idx8_kernel<ADD, false>), grid, block, 0, h->stream, p->d_rowblk,
                         p->nblocks, ai, p->d_idx8, p->d_offtab, p->ntab, aa, x, yin, yout, (double *)nullptr, p->pairsum);
      break;
    default: break;
  }
#define SPMV_GO(C, V)                                                                                                  \
  hipLaunchKernelGGL((spmv_csr_rowblock_kernel<ADD, C, V>), grid, block, 0, h->stream, p->d_rowblk, p->nblocks, ai, aj, \
                     aa, x, yin, yout, p->d_rows, p->pairsum, dsc, spmv_y_streams(p->nrows))
  if (form == SPMV_PLAIN)             { if (p->d_rows) SPMV_GO(true, true); else SPMV_GO(false, true); }
  else if (form == SPMV_PLAIN_SCALAR) { if (p->d_rows) SPMV_GO(true, false); else SPMV_GO(false, false); }
#undef SPMV_GO
  MI355X_LAUNCH_CHECK();
  return 0;
}

extern "C" {

static int spmv_plan_create(mi355x_handle_t h, int nrows, const int *ai_host, const int *rows_host, mi355x_spmv_plan_t *plan) {
  // one cleanup path: a failure frees what was allocated so far
  std::unique_ptr<mi355x_spmv_plan_s, decltype(&mi355x_spmv_plan_destroy)> p(new mi355x_spmv_plan_s(), mi355x_spmv_plan_destroy);   // (zeroed)
  p->nrows = nrows;
  p->use_pat = 1; p->use_runs = 1; p->ch = SPMV_CH; p->use_vpat = 1;
  std::vector<int2> rb;
  rb.reserve((size_t)nrows / 128 + 2);
  rb.push_back(make_int2(0, ai_host[0]));
  int r = 0;
  while (r < nrows) {
    const int start = r;
    int nnz = 0;
    while (r < nrows && (r - start) < SPMV_BLOCK_ROWS) {
      const int len = ai_host[r + 1] - ai_host[r];
      if (nnz + len > SPMV_BLOCK_CAP) break;
      nnz += len;
      ++r;
    }
    if (r == start) {  // a single row longer than the LDS stage
      ++r;
      p->nlong++;
    }
    rb.push_back(make_int2(r, ai_host[r]));
  }
  p->nblocks = (int)rb.size() - 1;
  MI355X_TRY(hipMalloc((void **)&p->d_rowblk, sizeof(int2) * rb.size()));
  MI355X_TRY(hipMemcpyAsync(p->d_rowblk, rb.data(), sizeof(int2) * rb.size(), hipMemcpyHostToDevice, h->stream));
  if (rows_host) {
    MI355X_TRY(hipMalloc((void **)&p->d_rows, sizeof(int) * (size_t)(nrows > 0 ? nrows : 1)));
    MI355X_TRY(hipMemcpyAsync(p->d_rows, rows_host, sizeof(int) * (size_t)nrows, hipMemcpyHostToDevice, h->stream));
  }
  MI355X_TRY(hipStreamSynchronize(h->stream));  // rb is a local
  *plan = p.release();
  return 0;
}
int mi355x_spmv_plan_create(mi355x_handle_t h, int nrows, const int *ai_host, const int *rows_host, mi355x_spmv_plan_t *plan) {
  *plan = nullptr;
  return mi355x_guard([&] { return spmv_plan_create(h, nrows, ai_host, rows_host, plan); });
}

// host threads of the pattern analyses: up to `cap`, one below 400 000 rows; MI355X_ANALYSIS_THREADS=<n> in the environment
// forces a count (tests: the merge of the chunks' tables on small matrices), never more than one thread per row
static int analysis_threads(int m, int cap) {
  int nth = mi355x_host_threads(cap);
  if (m < 400000) nth = 1;
  const char *e = getenv("MI355X_ANALYSIS_THREADS");
  if (e && atoi(e) > 0) nth = atoi(e) > 64 ? 64 : atoi(e);
  if (nth > m) nth = m > 0 ? m : 1;
  return nth;
}

// Run descriptors of the row-pattern kernel, from the finished row words (host arrays; no device involved): block b's rows
// [rowblk[2 b], rowblk[2 b + 2]) as maximal runs of consecutive rows with one table start -- an empty row is the pattern of length
// 0 and forms runs like any other.  Inside a run the rows' first nonzeros advance by the pattern's length (CSR rows lie one after
// the other), so the run keeps its first row's word.  runs[SPMV_RUN_WORDS * b ...]: per run {that word, first row in the block : 16 |
// length : 16}, unused runs {0, SPMV_RUN_NONE}; a block of more than SPMV_RUNS runs gets unused runs only and keeps its row words.
// *ncoded: blocks described by runs.
static void spmv_pattern_runs(int nblocks, const int *rowblk, const unsigned int *prow, const int *pattab, unsigned int *runs, int b_lo, int b_hi, int *ncoded) {
  int coded = 0;
  for (int b = b_lo; b < b_hi; ++b) {
    unsigned int *d = runs + (size_t)SPMV_RUN_WORDS * (size_t)b;
    const int r0 = rowblk[2 * (size_t)b], r1 = rowblk[2 * (size_t)b + 2];
    int n = 0;
    for (int r = r0; r < r1; ++r) {
      if (r > r0 && (prow[r] & 0xffffu) == (prow[r - 1] & 0xffffu)) continue;
      if (n == SPMV_RUNS) { n = SPMV_RUNS + 1; break; }
      d[2 * n] = prow[r];
      d[2 * n + 1] = (unsigned int)(r - r0) | ((unsigned int)pattab[prow[r] & 0xffffu] << 16);
      ++n;
    }
    if (n > SPMV_RUNS) n = 0; else ++coded;
    for (; n < SPMV_RUNS; ++n) { d[2 * n] = 0u; d[2 * n + 1] = SPMV_RUN_NONE; }
  }
  (void)nblocks;
  *ncoded = coded;
}
int mi355x_spmv_pattern_runs_host(int nblocks, const int *rowblk, const unsigned int *prow, const int *pattab, unsigned int *runs, int *nblocks_run_coded) {
  if (nblocks < 0 || (nblocks > 0 && (!rowblk || !prow || !pattab || !runs))) return (int)hipErrorInvalidValue;
  int coded = 0;
  spmv_pattern_runs(nblocks, rowblk, prow, pattab, runs, 0, nblocks, &coded);
  if (nblocks_run_coded) *nblocks_run_coded = coded;
  return 0;
}

// Offset-dictionary analysis: idx8[k] = position of (aj[k] - row) in a table of <= 256 distinct offsets.
// Returns 0 and leaves the plan uncompressed when the matrix has more distinct offsets.
static int spmv_compress_indices(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host) {
  if (!p || p->d_rows || p->d_idx8 || p->nrows == 0) return 0;
  if (p->nlong) return 0;   // a row longer than the LDS stage: the plain kernel's whole-workgroup path (distinct columns would need > 256 offsets anyway)
  const int m = p->nrows;
  const long nnz = ai_host[m];
  // The rows are analysed in contiguous chunks by host threads (one pass over the column indices of P7(256) on one thread: 0.3 s
  // before the first product): every chunk collects its offsets / its rows' slot lists in order of first appearance, the chunks'
  // tables are merged in chunk order -- which gives the table of a single pass over all rows -- and the chunks renumber their part.
  int nth = analysis_threads(m, 16);
  auto chunk_lo = [&](int k) { return (int)((long)m * k / nth); };
  std::unique_ptr<unsigned char[]> idx(new unsigned char[(size_t)(nnz > 0 ? nnz : 1)]);
  struct OffTab { int tab[256]; int n = 0; bool ok = true; };
  std::vector<OffTab> lt((size_t)nth);
  mi355x_parallel_chunks(nth, [&](int k) {
    OffTab &t = lt[(size_t)k];
    int last = 0;      // (offsets of a stencil matrix repeat row after row, so the slot after the previous one is tried first)
    for (int r = chunk_lo(k); r < chunk_lo(k + 1); ++r) {
      for (int q = ai_host[r]; q < ai_host[r + 1]; ++q) {
        const int off = aj_host[q] - r;
        int slot = -1;
        if (t.n && t.tab[last] == off) slot = last;
        else for (int e = 0; e < t.n; ++e) if (t.tab[e] == off) { slot = e; break; }
        if (slot < 0) {
          if (t.n == 256) { t.ok = false; return; }   // too many distinct offsets: keep plain CSR
          t.tab[t.n] = off;
          slot = t.n++;
        }
        idx[(size_t)q] = (unsigned char)slot;
        last = (slot + 1 < t.n) ? slot + 1 : 0;
      }
    }
  });
  for (auto &t : lt) if (!t.ok) return 0;
  int tab[256];
  int ntab = 0;
  std::vector<std::array<unsigned char, 256>> remap((size_t)nth);
  std::vector<char> identity((size_t)nth, 1);
  for (int k = 0; k < nth; ++k) {
    for (int e = 0; e < lt[(size_t)k].n; ++e) {
      int g = -1;
      for (int f = 0; f < ntab; ++f) if (tab[f] == lt[(size_t)k].tab[e]) { g = f; break; }
      if (g < 0) { if (ntab == 256) return 0; tab[ntab] = lt[(size_t)k].tab[e]; g = ntab++; }
      remap[(size_t)k][(size_t)e] = (unsigned char)g;
      if (g != e) identity[(size_t)k] = 0;
    }
  }
  mi355x_parallel_chunks(nth, [&](int k) {
    if (identity[(size_t)k]) return;
    const unsigned char *mp = remap[(size_t)k].data();
    for (long q = ai_host[chunk_lo(k)]; q < ai_host[chunk_lo(k + 1)]; ++q) idx[(size_t)q] = mp[idx[(size_t)q]];
  });
  std::vector<int2> blk((size_t)p->nblocks + 1);       // (row patterns below; allocated here: a throw must not leave copies out of idx, tab in flight)
  MI355X_TRY(hipMalloc((void **)&p->d_idx8, (size_t)(nnz > 0 ? nnz : 1) + 16));
  MI355X_TRY(hipMalloc((void **)&p->d_offtab, sizeof(int) * 256));
  MI355X_TRY(hipMemsetAsync(p->d_offtab, 0, sizeof(int) * 256, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_idx8, idx.get(), (size_t)nnz, hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_offtab, tab, sizeof(int) * (size_t)ntab, hipMemcpyHostToDevice, h->stream));
  p->ntab = ntab;
  // Run length of the block -> XCD map for this operator.  XCD x owns runs of `ch` consecutive row blocks, dealt round-robin, so the
  // rows a run covers come back to the SAME XCD every 8 * ch blocks.  With 8 * ch * 256 rows = the operator's largest offset (the plane
  // of a 3-D stencil) the x entries a row reads at that offset were fetched into this XCD's own L2 when it worked on the plane before:
  // P7(256) ch = 32 (the value tuned by hand in round 2), P7(512) ch = 128: 1.96 -> 1.77 ms per product there
  // (profiles/r04_spmv_map_sweep.log); any other ch leaves those gathers to the Infinity Cache.  MI355X_SPMV_CH=<n> overrides.
  {
    long maxoff = 0;
    for (int e = 0; e < ntab; ++e) { const long o = tab[e] < 0 ? -(long)tab[e] : (long)tab[e]; if (o > maxoff) maxoff = o; }
    long ch = (maxoff + (long)MI355X_NXCD * SPMV_BLOCK_ROWS / 2) / ((long)MI355X_NXCD * SPMV_BLOCK_ROWS);
    if (ch < 8) ch = 8;
    if (ch > 1024) ch = 1024;
    const char *e_ = getenv("MI355X_SPMV_CH");
    if (e_ && atoi(e_) > 0) ch = atoi(e_);
    p->ch = (int)ch;
  }
  // row patterns: the rows' slot lists as a dictionary of at most SPMV_PAT_CAP table entries in all (stencil operators: a
  // handful of lists); rows too long for the row block's one-lane-per-row sums (> SPMV_BLOCK_CAP never happens here) or a
  // table that would not fit leave the plan at the per-nonzero bytes
  {
    // first nonzero of every row block (the rows carry their offset from it in 16 bits: a block holds <= 2046 nonzeros)
    MI355X_TRY(hipMemcpyAsync(blk.data(), p->d_rowblk, sizeof(int2) * ((size_t)p->nblocks + 1), hipMemcpyDeviceToHost, h->stream));
    MI355X_TRY(hipStreamSynchronize(h->stream));          // (also: idx and tab have left the host)
    std::unique_ptr<unsigned int[]> prow(new unsigned int[(size_t)m]);
    struct PatDict { std::vector<int> ptab; std::vector<int> starts; std::vector<std::vector<unsigned char>> keys; bool ok = true; };
    std::vector<PatDict> pd((size_t)nth);
    mi355x_parallel_chunks(nth, [&](int k) {
      PatDict &d = pd[(size_t)k];
      std::map<std::vector<unsigned char>, int> dict;
      std::vector<unsigned char> cur, prev;
      int prev_start = -1;
      const int r0 = chunk_lo(k), r1 = chunk_lo(k + 1);
      int b = 0;
      { int lo = 0, hi = p->nblocks;                       // the block that holds row r0: the last one starting at or before it
        while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (blk[(size_t)mid].x <= r0) lo = mid; else hi = mid - 1; }
        b = lo; }
      for (int r = r0; r < r1; ++r) {
        while (b + 1 <= p->nblocks && blk[(size_t)b + 1].x <= r) ++b;
        const int len = ai_host[r + 1] - ai_host[r];
        const int rs = ai_host[r] - blk[(size_t)b].y;
        if (len > SPMV_BLOCK_CAP || rs < 0 || rs > 0xffff) { d.ok = false; return; }
        cur.assign(idx.get() + ai_host[r], idx.get() + ai_host[r + 1]);
        int start;
        if (prev_start >= 0 && cur == prev) start = prev_start;
        else {
          auto it = dict.find(cur);
          if (it != dict.end()) start = it->second;
          else {
            start = (int)d.ptab.size();
            if (start + 1 + len > SPMV_PAT_CAP) { d.ok = false; return; }
            d.ptab.push_back(len);                                          // table entry: {length, offsets ...}
            for (int q = 0; q < len; ++q) d.ptab.push_back(tab[cur[(size_t)q]]);
            dict.emplace(cur, start);
            d.starts.push_back(start); d.keys.push_back(cur);
          }
          prev = cur; prev_start = start;
        }
        prow[(size_t)r] = (unsigned int)start | ((unsigned int)rs << 16);
      }
    });
    bool ok = true;
    for (auto &d : pd) ok = ok && d.ok;
    std::vector<int> ptab;
    std::map<std::vector<unsigned char>, int> gdict;
    std::vector<std::vector<int>> to((size_t)nth);
    std::vector<char> same((size_t)nth, 1);
    for (int k = 0; k < nth && ok; ++k) {
      const PatDict &d = pd[(size_t)k];
      to[(size_t)k].assign((size_t)SPMV_PAT_CAP, -1);
      for (size_t e = 0; e < d.starts.size() && ok; ++e) {
        const int ls = d.starts[e], len = d.ptab[(size_t)ls];
        int g;
        auto it = gdict.find(d.keys[e]);
        if (it != gdict.end()) g = it->second;
        else {
          g = (int)ptab.size();
          if (g + 1 + len > SPMV_PAT_CAP) { ok = false; break; }
          ptab.insert(ptab.end(), d.ptab.begin() + ls, d.ptab.begin() + ls + 1 + len);
          gdict.emplace(d.keys[e], g);
        }
        to[(size_t)k][(size_t)ls] = g;
        if (g != ls) same[(size_t)k] = 0;
      }
    }
    if (ok) {
      mi355x_parallel_chunks(nth, [&](int k) {
        if (same[(size_t)k]) return;
        const int *t = to[(size_t)k].data();
        for (int r = chunk_lo(k); r < chunk_lo(k + 1); ++r) prow[(size_t)r] = (prow[(size_t)r] & 0xffff0000u) | (unsigned int)t[prow[(size_t)r] & 0xffffu];
      });
      ptab.resize(SPMV_PAT_CAP, 0);
      // the blocks' runs of equal patterns, from the row words just finished (chunks of blocks this time)
      const size_t nb = (size_t)p->nblocks;
      std::unique_ptr<unsigned int[]> runs(new unsigned int[SPMV_RUN_WORDS * nb]);
      std::vector<int> coded((size_t)nth, 0);
      mi355x_parallel_chunks(nth, [&](int k) {
        spmv_pattern_runs(p->nblocks, reinterpret_cast<const int *>(blk.data()), prow.get(), ptab.data(), runs.get(), (int)((long)nb * k / nth), (int)((long)nb * (k + 1) / nth), &coded[(size_t)k]);
      });
      p->nruncoded = 0;
      for (int c : coded) p->nruncoded += c;
      MI355X_TRY(hipMalloc((void **)&p->d_prow, sizeof(unsigned int) * (size_t)m + 16));
      MI355X_TRY(hipMalloc((void **)&p->d_pattab, sizeof(int) * SPMV_PAT_CAP));
      MI355X_TRY(hipMalloc((void **)&p->d_pruns, sizeof(unsigned int) * SPMV_RUN_WORDS * nb));
      MI355X_TRY(hipMemcpyAsync(p->d_pruns, runs.get(), sizeof(unsigned int) * SPMV_RUN_WORDS * nb, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(p->d_prow, prow.get(), sizeof(unsigned int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipMemcpyAsync(p->d_pattab, ptab.data(), sizeof(int) * SPMV_PAT_CAP, hipMemcpyHostToDevice, h->stream));
      MI355X_TRY(hipStreamSynchronize(h->stream));
      p->npat = (int)gdict.size();
    }
  }
  return 0;
}
int mi355x_spmv_plan_compress_indices(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host) {
  return mi355x_guard([&] { return spmv_compress_indices(h, p, ai_host, aj_host); });
}

// A/B switch for the row-pattern kernel (on by default when the analysis found a dictionary); *npat: its size, 0 if none
int mi355x_spmv_plan_use_patterns(mi355x_spmv_plan_t p, int on, int *npat) {
  if (!p) return (int)hipErrorInvalidValue;
  if (on >= 0) p->use_pat = on ? 1 : 0;
  if (npat) *npat = p->d_prow ? p->npat : 0;
  return 0;
}

// A/B switch for the run-coded blocks of the row-pattern kernel (on by default): on = 0 makes every block read its row words,
// on < 0 only asks; *nblocks_run_coded: row blocks the analysis described by runs, 0 when the plan has no row patterns
int mi355x_spmv_plan_use_pattern_runs(mi355x_spmv_plan_t p, int on, int *nblocks_run_coded) {
  if (!p) return (int)hipErrorInvalidValue;
  if (on >= 0) p->use_runs = on ? 1 : 0;
  if (nblocks_run_coded) *nblocks_run_coded = p->d_pruns ? p->nruncoded : 0;
  return 0;
}

// Value-pattern analysis (see spmv_csr_valpat_kernel): one table entry per distinct row {length, offsets, values},
// values compared bit for bit.  Gives up as soon as the table would exceed SPMV_PAT_CAP entries -- after a few dozen
// rows for a matrix with varying coefficients -- and then leaves the plan as it was.  To be called with the values that
// are (about to be) on the device, after every change of them.  *nvpat: distinct rows found, 0 when not applicable.
static int spmv_value_patterns(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host, const double *aa_host, int *nvpat) {
  if (nvpat) *nvpat = 0;
  if (!p) return (int)hipErrorInvalidValue;
  p->vpat_valid = 0;
  if (p->d_rows || p->nrows == 0 || !p->use_vpat) return 0;
  const int m = p->nrows;
  if (m > SPMV_VPAT_MAXROWS) return 0;              // byte offsets into x are 32-bit
  std::vector<unsigned short> vrow((size_t)m);
  // table entry: {length, byte offsets of the columns relative to the row ..., padded to a multiple of 8 slots with copies of the
  // first offset}; values at the offsets' indices (pads 0.0, never used in a sum).  Entries in order of first appearance.
  // The rows are analysed in contiguous chunks by a few host threads, each with a dictionary of its own (a pass over 0.94 GB of
  // values on one thread cost 0.2 s at every upload of P7(256)); the chunks' dictionaries are then merged in chunk order -- the
  // merged table is the one a single pass over all rows builds -- and the rows' entries renumbered.
  struct Dict { std::vector<int> ptab; std::vector<double> pval; std::vector<int> starts; bool ok = true; };
  auto analyse = [&](int r0, int r1, Dict &d) {
    d.ptab.reserve(SPMV_PAT_CAP); d.pval.reserve(SPMV_PAT_CAP);
    auto same = [&](int s_, int r, int len) {
      if (d.ptab[(size_t)s_] != len) return false;
      const int k0 = ai_host[r];
      for (int q = 0; q < len; ++q) if ((aj_host[k0 + q] - r) * 8 != d.ptab[(size_t)s_ + 1 + q]) return false;
      return len == 0 || memcmp(aa_host + k0, d.pval.data() + s_ + 1, sizeof(double) * (size_t)len) == 0;
    };
    int prev = -1;
    for (int r = r0; r < r1; ++r) {
      const int len = ai_host[r + 1] - ai_host[r];
      int start = -1;
      if (prev >= 0 && same(prev, r, len)) start = prev;
      else for (size_t e = 0; e < d.starts.size(); ++e) if (same(d.starts[e], r, len)) { start = d.starts[e]; break; }
      if (start < 0) {
        const int slots = (len + 7) / 8 * 8;
        start = (int)d.ptab.size();
        if (start + 1 + slots > SPMV_PAT_CAP) { d.ok = false; return; }      // not a constant-coefficient operator
        d.ptab.push_back(len); d.pval.push_back(0.0);
        for (int q = 0; q < slots; ++q) {
          const int col = aj_host[ai_host[r] + (q < len ? q : 0)];
          if (col >= SPMV_VPAT_MAXROWS) { d.ok = false; return; }
          d.ptab.push_back((col - r) * 8);
          d.pval.push_back(q < len ? aa_host[ai_host[r] + q] : 0.0);
        }
        d.starts.push_back(start);
      }
      prev = start;
      vrow[(size_t)r] = (unsigned short)start;
    }
  };
  const int nth = analysis_threads(m, 8);
  std::vector<Dict> dicts((size_t)nth);
  mi355x_parallel_chunks(nth, [&](int k) { analyse((int)((long)m * k / nth), (int)((long)m * (k + 1) / nth), dicts[(size_t)k]); });
  for (auto &d : dicts) if (!d.ok) return 0;
  std::vector<int> ptab(std::move(dicts[0].ptab)), starts(std::move(dicts[0].starts));
  std::vector<double> pval(std::move(dicts[0].pval));
  for (int k = 1; k < nth; ++k) {
    const Dict &d = dicts[(size_t)k];
    std::vector<int> to((size_t)SPMV_PAT_CAP, -1);             // this chunk's entry (by its start) -> the merged table's
    for (size_t e = 0; e < d.starts.size(); ++e) {
      const int ls = d.starts[e], len = d.ptab[(size_t)ls], slots = (len + 7) / 8 * 8;
      int g = -1;
      for (size_t f = 0; f < starts.size() && g < 0; ++f) {
        const int gs = starts[f];
        if (ptab[(size_t)gs] == len && memcmp(&ptab[(size_t)gs + 1], &d.ptab[(size_t)ls + 1], sizeof(int) * (size_t)len) == 0 &&
            (len == 0 || memcmp(&pval[(size_t)gs + 1], &d.pval[(size_t)ls + 1], sizeof(double) * (size_t)len) == 0)) g = gs;
      }
      if (g < 0) {
        g = (int)ptab.size();
        if (g + 1 + slots > SPMV_PAT_CAP) return 0;
        ptab.insert(ptab.end(), d.ptab.begin() + ls, d.ptab.begin() + ls + 1 + slots);
        pval.insert(pval.end(), d.pval.begin() + ls, d.pval.begin() + ls + 1 + slots);
        starts.push_back(g);
      }
      to[(size_t)ls] = g;
    }
    const int r0 = (int)((long)m * k / nth), r1 = (int)((long)m * (k + 1) / nth);
    for (int r = r0; r < r1; ++r) vrow[(size_t)r] = (unsigned short)to[(size_t)vrow[(size_t)r]];
  }
  if (!p->d_vrow) {
    MI355X_TRY(hipMalloc((void **)&p->d_vrow, sizeof(unsigned short) * (size_t)m + 16));
    MI355X_TRY(hipMalloc((void **)&p->d_vpattab, sizeof(int) * SPMV_PAT_CAP));
    MI355X_TRY(hipMalloc((void **)&p->d_vpatval, sizeof(double) * SPMV_PAT_CAP));
  }
  MI355X_TRY(hipMemcpyAsync(p->d_vrow, vrow.data(), sizeof(unsigned short) * (size_t)m, hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_vpattab, ptab.data(), sizeof(int) * ptab.size(), hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_vpatval, pval.data(), sizeof(double) * pval.size(), hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipStreamSynchronize(h->stream));   // the vectors are locals
  p->vtablen = (int)ptab.size();
  p->nvpat = (int)starts.size();
  p->vpat_valid = 1;
  if (nvpat) *nvpat = p->nvpat;
  return 0;
}
int mi355x_spmv_plan_value_patterns(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host,
                                    const double *aa_host, int *nvpat) {
  return mi355x_guard([&] { return spmv_value_patterns(h, p, ai_host, aj_host, aa_host, nvpat); });
}

// the values on the device no longer are the ones the table was derived from
int mi355x_spmv_plan_drop_value_patterns(mi355x_spmv_plan_t p) {
  if (p) p->vpat_valid = 0;
  return 0;
}

// A/B switch (on by default); on < 0 only queries.  *nvpat: size of the dictionary in use, 0 if none
int mi355x_spmv_plan_use_value_patterns(mi355x_spmv_plan_t p, int on, int *nvpat) {
  if (!p) return (int)hipErrorInvalidValue;
  if (on >= 0) { p->use_vpat = on ? 1 : 0; if (!on) p->vpat_valid = 0; }
  if (nvpat) *nvpat = p->vpat_valid ? p->nvpat : 0;
  return 0;
}

// Row grouping (the analysis half of the reference's inode machinery).  The caller passes the node sizes the
// reference's Mat_CheckInode finds (ns[nnodes], consecutive rows with identical column lists, at most `limit` rows
// each; inode.c:3981-3998) -- the host library computes them with the reference's loop so that they can be compared
// with it.  This routine stores one column list per group and rebuilds the row blocks from whole groups.  It leaves
// the plan as it is (returns 0) when grouping would not pay (shared indices > 2/3 of the nonzeros), when a row has
// more than SPMV_GJ_CAP entries, or for compressed-row / index-compressed plans.
static int spmv_group_rows(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host, int nnodes, const int *ns) {
  if (!p || p->d_rows || p->d_idx8 || p->d_gj || p->nrows == 0 || nnodes <= 0) return 0;
  const int m = p->nrows;
  const long nnz = ai_host[m];
  // groups: a node whose rows together exceed the LDS stage is cut into smaller groups
  std::vector<int> gstart;          // first row of each group (+ m at the end)
  gstart.reserve((size_t)nnodes + 1);
  long ngj = 0;
  int row = 0;
  for (int g = 0; g < nnodes; ++g) {
    const int nc = ai_host[row + 1] - ai_host[row];
    if (nc > SPMV_GJ_CAP) return 0;
    int left = ns[g];
    if (left < 1 || row + left > m) return (int)hipErrorInvalidValue;
    int per = left;
    while ((long)per * nc > SPMV_BLOCK_CAP) --per;          // nc <= SPMV_GJ_CAP: per >= 2
    while (left > 0) {
      const int take = left < per ? left : per;
      gstart.push_back(row);
      ngj += nc;
      row += take;
      left -= take;
    }
  }
  if (row != m) return (int)hipErrorInvalidValue;
  gstart.push_back(m);
  if (3 * ngj > 2 * nnz) return 0;                            // not enough shared structure to pay for the lookups
  const int ngroups = (int)gstart.size() - 1;
  std::vector<int> goff((size_t)m), gjh((size_t)(ngj > 0 ? ngj : 1));
  std::vector<int4> rb;
  rb.reserve((size_t)m / 64 + 2);
  rb.push_back(make_int4(0, ai_host[0], 0, 0));
  long gpos = 0;
  int brows = 0, bnnz = 0, bgj = 0;
  for (int g = 0; g < ngroups; ++g) {
    const int ra = gstart[g], rbn = gstart[g + 1];
    const int nc = ai_host[ra + 1] - ai_host[ra];
    const int gn = (rbn - ra) * nc;
    if (brows + (rbn - ra) > SPMV_BLOCK_ROWS || bnnz + gn > SPMV_BLOCK_CAP || bgj + nc > SPMV_GJ_CAP) {
      rb.push_back(make_int4(ra, ai_host[ra], (int)gpos, 0));
      brows = bnnz = bgj = 0;
    }
    for (int r = ra; r < rbn; ++r) goff[(size_t)r] = (int)gpos;
    for (int c = 0; c < nc; ++c) gjh[(size_t)(gpos + c)] = aj_host[ai_host[ra] + c];
    gpos += nc;
    brows += rbn - ra; bnnz += gn; bgj += nc;
  }
  rb.push_back(make_int4(m, ai_host[m], (int)gpos, 0));
  MI355X_TRY(hipMalloc((void **)&p->d_rowblk4, sizeof(int4) * rb.size()));
  MI355X_TRY(hipMalloc((void **)&p->d_goff, sizeof(int) * (size_t)m));
  MI355X_TRY(hipMalloc((void **)&p->d_gj, sizeof(int) * (size_t)(ngj > 0 ? ngj : 1) + 16));   // +16: the last pair load may straddle the end
  MI355X_TRY(hipMemcpyAsync(p->d_rowblk4, rb.data(), sizeof(int4) * rb.size(), hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_goff, goff.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipMemcpyAsync(p->d_gj, gjh.data(), sizeof(int) * (size_t)ngj, hipMemcpyHostToDevice, h->stream));
  MI355X_TRY(hipStreamSynchronize(h->stream));
  p->nblocks = (int)rb.size() - 1;
  p->nlong = 0;
  p->ngroups = ngroups;
  p->ngj = ngj;
  return 0;
}
int mi355x_spmv_plan_group_rows(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai_host, const int *aj_host, int nnodes,
                                const int *ns) {
  return mi355x_guard([&] { return spmv_group_rows(h, p, ai_host, aj_host, nnodes, ns); });
}

int mi355x_spmv_plan_set_pairsum(mi355x_spmv_plan_t p, int on) {
  if (p) p->pairsum = on ? 1 : 0;
  return 0;
}

int mi355x_spmv_plan_group_info(mi355x_spmv_plan_t p, int *ngroups, long *nshared_indices, int *pairsum) {
  if (ngroups) *ngroups = p->d_gj ? p->ngroups : 0;
  if (nshared_indices) *nshared_indices = p->d_gj ? p->ngj : 0;
  if (pairsum) *pairsum = p->pairsum;
  return 0;
}

int mi355x_spmv_plan_destroy(mi355x_spmv_plan_t p) {
  if (!p) return 0;
  // (hipFree(nullptr) is a no-op)
  hipFree(p->d_rowblk);
  hipFree(p->d_idx8);
  hipFree(p->d_offtab);
  hipFree(p->d_prow);
  hipFree(p->d_pattab);
  hipFree(p->d_pruns);
  hipFree(p->d_vrow);
  hipFree(p->d_vpattab);
  hipFree(p->d_vpatval);
  hipFree(p->d_rows);
  hipFree(p->d_dotpart);
  hipFree(p->d_rowblk4);
  hipFree(p->d_goff);
  hipFree(p->d_gj);
  delete p;
  return 0;
}

int mi355x_spmv_plan_is_compressed(mi355x_spmv_plan_t p, int *ntab) {
  if (ntab) *ntab = p->d_idx8 ? p->ntab : 0;
  return 0;
}

// would mi355x_spmv_csr_dot run on this plan with this value array?
int mi355x_spmv_plan_dot_available(mi355x_spmv_plan_t p, const double *aa, int *yes) {
  const spmv_form_t form = spmv_form(p, aa, nullptr);
  if (yes) *yes = (form == SPMV_VALPAT || form == SPMV_ROWPAT || form == SPMV_IDX8) ? 1 : 0;
  return 0;
}

int mi355x_spmv_plan_info(mi355x_spmv_plan_t p, int *nblocks, int *nlong, size_t *workspace_bytes) {
  if (nblocks) *nblocks = p->nblocks;
  if (nlong) *nlong = p->nlong;
  if (workspace_bytes) *workspace_bytes = sizeof(int) * (2 * ((size_t)p->nblocks + 1) + (p->d_rows ? (size_t)p->nrows : 0) +
                                                              (p->d_pruns ? SPMV_RUN_WORDS * (size_t)p->nblocks : 0));
  return 0;
}

// the compressed-row list of a plan (device array, the plan's own) and the plan's row count; rows NULL: not compressed
int mi355x_spmv_plan_rows(mi355x_spmv_plan_t p, const int **rows_dev, int *nrows) {
  if (!p) return (int)hipErrorInvalidValue;
  if (rows_dev) *rows_dev = p->d_rows;
  if (nrows) *nrows = p->nrows;
  return 0;
}

int mi355x_spmv_csr(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                    const double *x, double *y) {
  return launch_spmv<0>(h, plan, ai, aj, aa, x, nullptr, y);
}

// y = d .* (A x): MatMult followed by PCApply_Jacobi's VecPointwiseMult (jacobi.c:266) in the product's epilogue
int mi355x_spmv_csr_scaled(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                           const double *x, const double *d, double *y) {
  return launch_spmv<2>(h, plan, ai, aj, aa, x, d, y);
}

// y = A x and x'y from one pass over the matrix (KSPSolve_CG's w = A p, dpi = p'w): every row block leaves its sum of
// x_r y_r in the plan; mi355x_spmv_dot_finish adds them in block order (a second, tiny launch).  Needs the
// index-compressed plan and a square matrix; hipErrorNotSupported otherwise (the caller then uses mi355x_spmv_csr +
// mi355x_vec_dot).
int mi355x_spmv_csr_dot(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai, const int *aj, const double *aa,
                        const double *x, double *y) {
  // the kernel mi355x_spmv_csr runs on these arrays (spmv_form), with the per-block sums where that kernel has them
  const spmv_form_t form = spmv_form(p, aa, aj);
  if (form != SPMV_VALPAT && form != SPMV_ROWPAT && form != SPMV_IDX8) return (int)hipErrorNotSupported;
  if (p->nblocks == 0) return 0;
  const int nvb = (p->nrows + SPMV_VPAT_ROWS - 1) / SPMV_VPAT_ROWS;
  { const size_t need = (size_t)(p->nblocks > nvb ? p->nblocks : nvb);
    if (!p->d_dotpart) MI355X_TRY(hipMalloc((void **)&p->d_dotpart, sizeof(double) * need)); }
  const dim3 block(SPMV_THREADS);
  const double *const no_yin = nullptr;
  switch (form) {
    case SPMV_VALPAT:
      hipLaunchKernelGGL((spmv_csr_valpat_kernel<0, true>), dim3(nvb), block, 0, h->stream, p->nrows, p->d_vrow, p->d_vpattab,
                         p->d_vpatval, p->vtablen, x, no_yin, y, p->d_dotpart, p->pairsum);
      break;
    case SPMV_ROWPAT:
      hipLaunchKernelGGL((spmv_csr_rowblock_pat_kernel<0, true>), dim3(rowblock_grid(p->nblocks, p->ch)), block, 0, h->stream, p->d_rowblk,
                         p->nblocks, p->d_prow, spmv_runs_of(p), p->d_pattab, aa, x, no_yin, y, p->d_dotpart, p->pairsum, p->ch, spmv_y_streams(p->nrows));
      break;
    default:   // SPMV_IDX8
      hipLaunchKernelGGL((spmv_csr_rowblock_idx8_kernel<0, true>), dim3(rowblock_grid(p->nblocks, SPMV_CH)), block, 0, h->stream, p->d_rowblk,
                         p->nblocks, ai, p->d_idx8, p->d_offtab, p->ntab, aa, x, no_yin, y, p->d_dotpart, p->pairsum);
      break;
  }
  p->ndotpart = form == SPMV_VALPAT ? nvb : p->nblocks;
  MI355X_LAUNCH_CHECK();
  return 0;
}
int mi355x_spmv_dot_finish(mi355x_handle_t h, mi355x_spmv_plan_t p, double *out) {
  if (p->nblocks == 0 || !p->d_dotpart || p->ndotpart <= 0) { MI355X_TRY(hipMemsetAsync(out, 0, sizeof(double), h->stream)); return 0; }
  hipLaunchKernelGGL(dot_partials_kernel, dim3(1), dim3(1024), 0, h->stream, p->d_dotpart, p->ndotpart, out);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_spmv_csr_add(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                        const double *x, const double *y, double *z) {
  return launch_spmv<1>(h, plan, ai, aj, aa, x, y, z);
}

// z = d .* (y + A x): one step of a Jacobi-sweep triangular solve with inverted pivots (x^j = dinv .* (y^k - Us x^(j-1)), A = -Us),
// where mi355x_spmv_csr_add is the step of the unit triangle.  The plan's plain row-block kernel whatever else the plan holds:
// rows of a block with <= SPMV_SEQ_AVG nonzeros per row on average are summed by one lane, s = y_r; s += a_j x_j in column order,
// then d_r * s; longer rows by the family's lane tree.  z may alias y; x must not alias z.
int mi355x_spmv_csr_add_scaled(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                               const double *x, const double *y, const double *d, double *z) {
  if (!d || !y) return (int)hipErrorInvalidValue;
  return launch_spmv<3>(h, plan, ai, aj, aa, x, y, z, d);
}

// r = b - A x: the product's row sum (mi355x_spmv_csr's, whatever form the plan runs) and one subtraction from b_r in the epilogue --
// the bits of mi355x_spmv_csr into a work vector followed by mi355x_vec_aypx(w, -1, b), without the write and the re-read of w.
// r may alias b (a row's b is read by the lanes that write its r); x must not alias r.  A compressed-row plan visits the listed
// rows only, and a residual has to write every row: hipErrorNotSupported, nothing written.
int mi355x_spmv_csr_residual(mi355x_handle_t h, mi355x_spmv_plan_t plan, const int *ai, const int *aj, const double *aa,
                             const double *x, const double *b, double *r) {
  if (!h || !plan || !ai || !aj || !aa || !x || !b || !r || x == r) return (int)hipErrorInvalidValue;
  if (plan->d_rows) return (int)hipErrorNotSupported;
  return launch_spmv<4>(h, plan, ai, aj, aa, x, b, r);
}

static int spmv_bsr_planned_impl(mi355x_handle_t h, mi355x_spmv_plan_t p, int bs, const int *ai, const int *aj,
                                 const double *aa, const double *x, const double *yin, double *y, bool xlds) {
  if (p->nblocks == 0) return 0;
  const dim3 grid(rowblock_grid(p->nblocks, SPMV_CH)), block(SPMV_THREADS);
#define BSR_GO(B) do { if (xlds) hipLaunchKernelGGL((bsr_rowblock_kernel<B, true>), grid, block, 0, h->stream, p->d_rowblk, p->nblocks, ai, aj, aa, x, yin, y); \
                       else hipLaunchKernelGGL((bsr_rowblock_kernel<B, false>), grid, block, 0, h->stream, p->d_rowblk, p->nblocks, ai, aj, aa, x, yin, y); } while (0)
  switch (bs) {
    case 2: BSR_GO(2); break;
    case 3: BSR_GO(3); break;
    case 4: BSR_GO(4); break;
    case 5: BSR_GO(5); break;
    case 6: BSR_GO(6); break;
    case 7: BSR_GO(7); break;
    case 8: BSR_GO(8); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef BSR_GO
  MI355X_LAUNCH_CHECK();
  return 0;
}
// development / A-B entry points: the two forms of the row-block BCSR kernel side by side (tests/tools/cfg5_baij.py)
int mi355x_spmv_bsr_planned_form(mi355x_handle_t h, mi355x_spmv_plan_t p, int bs, int x_in_lds, const int *ai, const int *aj,
                                 const double *aa, const double *x, double *y) {
  return spmv_bsr_planned_impl(h, p, bs, ai, aj, aa, x, nullptr, y, x_in_lds != 0);
}
int mi355x_spmv_bsr_planned(mi355x_handle_t h, mi355x_spmv_plan_t p, int bs, const int *ai, const int *aj,
                            const double *aa, const double *x, double *y) {
  return spmv_bsr_planned_impl(h, p, bs, ai, aj, aa, x, nullptr, y, MI355X_BSR_XLDS_DEFAULT != 0);
}
// z = y + A x (MatMultAdd_SeqBAIJ_N, baij2.c:1168-1480); z may alias y
int mi355x_spmv_bsr_planned_add(mi355x_handle_t h, mi355x_spmv_plan_t p, int bs, const int *ai, const int *aj,
                                const double *aa, const double *x, const double *y, double *z) {
  return spmv_bsr_planned_impl(h, p, bs, ai, aj, aa, x, y, z, MI355X_BSR_XLDS_DEFAULT != 0);
}

int mi355x_csr_assemble(mi355x_handle_t h, int nseg, const int *segptr, const int *segslot, const int *order, const double *v, double *aa) {
  if (nseg <= 0) return 0;
  hipLaunchKernelGGL(csr_assemble_kernel, dim3((nseg + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream, nseg, segptr, segslot, order, v, aa);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_diagonal_scale(mi355x_handle_t h, int m, const int *ai, const int *aj, double *aa, const double *l, const double *r) {
  if (m <= 0 || (!l && !r)) return 0;
  hipLaunchKernelGGL(csr_diagscale_kernel, dim3((m + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream, m, ai, aj, aa, l, r);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_get_diagonal(mi355x_handle_t h, int m, const int *ai, const int *aj, const double *aa, double *d) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(csr_diag_kernel, dim3((m + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream, m,
                     ai, aj, aa, d);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_shift(mi355x_handle_t h, int m, const int *ai, const int *aj, double alpha, double *aa, int *nmissing_dev) {
  if (nmissing_dev) MI355X_TRY(hipMemsetAsync(nmissing_dev, 0, sizeof(int), h->stream));
  if (m <= 0) return 0;
  hipLaunchKernelGGL(csr_shift_kernel, dim3((m + MI355X_BLOCK - 1) / MI355X_BLOCK), dim3(MI355X_BLOCK), 0, h->stream, m, ai, aj, alpha, aa, nmissing_dev);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_zero_rows(mi355x_handle_t h, int nrows, const int *rows, const int *ai, const int *aj, double *aa, double diag,
                         const double *x, double *b) {
  if ((x == nullptr) != (b == nullptr)) return (int)hipErrorInvalidValue;
  if (nrows <= 0) return 0;
  const long groups_per_block = MI355X_BLOCK / ZR_GROUP;
  hipLaunchKernelGGL(csr_zero_rows_kernel, dim3((unsigned)(((long)nrows + groups_per_block - 1) / groups_per_block)), dim3(MI355X_BLOCK), 0, h->stream,
                     nrows, rows, ai, aj, aa, diag, x, b);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_zero_columns(mi355x_handle_t h, mi355x_spmv_plan_t p, const int *ai, const int *aj, double *aa, const unsigned int *mask,
                            const double *x, double *b) {
  if (!p || !mask || (x == nullptr) != (b == nullptr)) return (int)hipErrorInvalidValue;
  if (p->d_rows) return (int)hipErrorNotSupported;   // compressed rows: the plan's rows are not the matrix's
  if (p->nblocks == 0) return 0;
  const dim3 grid(rowblock_grid(p->nblocks, SPMV_CH)), block(SPMV_THREADS);
  if ((((uintptr_t)aj) & 7u) == 0) hipLaunchKernelGGL((csr_zero_columns_kernel<true>), grid, block, 0, h->stream, p->d_rowblk, p->nblocks, ai, aj, aa, mask, x, b);
  else hipLaunchKernelGGL((csr_zero_columns_kernel<false>), grid, block, 0, h->stream, p->d_rowblk, p->nblocks, ai, aj, aa, mask, x, b);
  MI355X_LAUNCH_CHECK();
  return 0;
}

int mi355x_csr_axpy_map(mi355x_handle_t h, int nzx, const int *xtoy, double alpha, const double *xa, double *ya) {
  if (nzx <= 0) return 0;
  hipLaunchKernelGGL(csr_axpy_map_kernel, dim3((unsigned)(((long)nzx + MI355X_BLOCK - 1) / MI355X_BLOCK)), dim3(MI355X_BLOCK), 0, h->stream, nzx, xtoy, alpha, xa, ya);
  MI355X_LAUNCH_CHECK();
  return 0;
}

// Host only.  Rows lo .. hi - 1 of the map: both rows ascending in the (translated) column, so one merge walk per row.  Returns the
// first row of the range in which X stores an entry Y lacks, or -1.
static int subset_map_rows(int lo, int hi, const int *xi, const int *xj, const int *xcols, const int *yi, const int *yj, const int *ycols, int *xtoy) {
  for (int r = lo; r < hi; ++r) {
    int q = yi[r];
    const int qe = yi[r + 1];
    for (int k = xi[r]; k < xi[r + 1]; ++k) {
      const int c = xcols ? xcols[xj[k]] : xj[k];
      while (q < qe && (ycols ? ycols[yj[q]] : yj[q]) < c) ++q;
      if (q == qe || (ycols ? ycols[yj[q]] : yj[q]) != c) return r;
      xtoy[k] = q++;
    }
  }
  return -1;
}
int mi355x_csr_subset_map(int m, const int *xi, const int *xj, const int *xcols, const int *yi, const int *yj, const int *ycols, int *xtoy, int *bad_row) {
  if (bad_row) *bad_row = -1;
  if (m <= 0) return 0;
  return mi355x_guard([&]() -> int {
    // one thread below 200 000 entries of X, unless MI355X_HOST_THREADS asks for a count; never more than one thread per row
    int nth = (xi[m] < 200000 && !getenv("MI355X_HOST_THREADS")) ? 1 : mi355x_host_threads(16);
    if (nth > m) nth = m;
    std::vector<int> bad((size_t)nth, -1);
    mi355x_parallel_chunks(nth, [&](int k) {
      bad[(size_t)k] = subset_map_rows((int)((long)m * k / nth), (int)((long)m * (k + 1) / nth), xi, xj, xcols, yi, yj, ycols, xtoy);
    });
    for (int k = 0; k < nth; ++k)
      if (bad[(size_t)k] >= 0) { if (bad_row) *bad_row = bad[(size_t)k]; return (int)hipErrorInvalidValue; }   // chunks are in row order: the first row
    return 0;
  });
}

}  // extern "C"
