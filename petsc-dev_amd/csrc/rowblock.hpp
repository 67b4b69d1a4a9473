// The row-block family's tuning knobs and the steps its kernels share, written once: the product kernels (spmv_csr.hip) and the
// row reductions (mat_reduce.hip) both stream a block's slice of the value array through LDS and walk a row out of it in order.
#pragma once
#include "common.hpp"

// tuning knobs (the defaults are the measured best on MI355X for the 7-point operator)
#ifndef SPMV_THREADS
#define SPMV_THREADS 256
#endif
#ifndef SPMV_NT
#define SPMV_NT 1            // non-temporal loads for the val/col streams
#endif
#ifndef SPMV_REMAP
#define SPMV_REMAP 2         // 0 = dispatch order; 2 = runs of SPMV_CH row blocks dealt round-robin to the XCDs (same speed as 0, 18 % less fabric traffic: x lines stay in one XCD's L2)
#endif
#ifndef SPMV_CH
#define SPMV_CH 32
#endif
#ifndef SPMV_MINWAVES
#define SPMV_MINWAVES 1      // __launch_bounds__ second argument (waves per SIMD the register allocator must allow)
#endif
#ifndef SPMV_SEQ_AVG
#define SPMV_SEQ_AVG 16      // row blocks with <= this many nonzeros per row on average: one lane per row, reference summation order
#endif
#define SPMV_GJ_CAP 960      // grouped-row kernel: shared column indices per row block (LDS sized for 7 workgroups per CU)
#define SPMV_BLOCK_NNZ (8 * SPMV_THREADS)   // LDS stage (doubles): 4 pairs per lane
#define SPMV_BLOCK_CAP (SPMV_BLOCK_NNZ - 2)   // nonzeros per row block: any alignment of the first pair still fits
#define SPMV_BLOCK_ROWS SPMV_THREADS
#define SPMV_PAIRS (SPMV_BLOCK_NNZ / (2 * SPMV_THREADS))   // pairs of the stream per lane
#define SPMV_WAVES (SPMV_THREADS / MI355X_WAVE)
#if SPMV_NT
#define SPMV_LOAD(p) __builtin_nontemporal_load(p)
#else
#define SPMV_LOAD(p) (*(p))
#endif
static_assert(SPMV_THREADS == 256 && MI355X_WAVE == 64, "one lane per row of a block with byte row markers, 256-entry offset table and 512-entry pattern tables staged one / two per lane");
static_assert(SPMV_REMAP == 0 || SPMV_REMAP == 2, "SPMV_REMAP == 1 (each XCD walks a contiguous eighth of the row blocks) was removed: only the plain kernel ever had it; use 0 or 2");

typedef double v2d __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));

// ---- the steps the row-block kernels share ----------------------------------------------------

// Block -> XCD map and the grid it needs.  Workgroups b, b+8, b+16.. share an XCD.  SPMV_REMAP == 2: XCD x owns runs of `ch`
// consecutive row blocks, runs dealt round-robin over the XCDs, so all XCDs stream one window of 8*ch blocks while each
// re-uses its own x lines; the grid is rounded up to whole rounds and a workgroup whose block is >= nblocks leaves.
static inline int rowblock_grid(int nblocks, int ch) {
  const int per = SPMV_REMAP == 2 ? MI355X_NXCD * ch : 1;
  return ((nblocks + per - 1) / per) * per;
}
__device__ __forceinline__ int rowblock_of_workgroup(int ch) {
  if (SPMV_REMAP != 2) return blockIdx.x;
  const int xcd = blockIdx.x % MI355X_NXCD, slot = blockIdx.x / MI355X_NXCD;
  return ((slot / ch) * MI355X_NXCD + xcd) * ch + (slot % ch);
}

// Lanes per row: tpr, the largest power of two with nrows * tpr <= 256, at most one wavefront; lane tid is lane `sub` of row `r`
// of the block (r >= nrows: no row).  short_rows_one_lane: a block with <= SPMV_SEQ_AVG nonzeros per row on average (the
// stencil case) gets one lane per row and the reference's summation order.
struct row_lanes { int tpr, r, sub; };
__device__ __forceinline__ row_lanes lanes_per_row(int nrows, int nnz, int tid, bool short_rows_one_lane = true) {
  int lg = 0;                                          // (log2 of tpr: the row of a lane is a shift, not a division)
  while (lg < 6 && ((nrows * 2) << lg) <= SPMV_THREADS) ++lg;
  if (short_rows_one_lane && nnz <= SPMV_SEQ_AVG * nrows) lg = 0;
  return {1 << lg, tid >> lg, tid & ((1 << lg) - 1)};
}

// The stream [k0, k1) of a block is read in aligned pairs (16 bytes of values), SPMV_PAIRS per lane: pair_k is the element
// at which pair p of lane tid starts.  The first pair may start one element before k0, the last end one after k1.
// Every load is unconditional and there is no control flow between the loads, so the compiler keeps all of them in flight
// behind one wait (the earlier predicated form serialised them pair by pair): a lane whose pair lies past the block
// re-reads the block's first pair (lane 0's address: merged by the coalescer), a pair cut by the block boundary is loaded
// whole (an aligned 16-byte access cannot leave the page its first half lies in).
__device__ __forceinline__ int pair_k(int k0, int tid, int p) { return (k0 & ~1) + 2 * tid + p * 2 * SPMV_THREADS; }
template <typename PAIR, typename T> __device__ __forceinline__ PAIR load_pair(const T *a, int k0, int k1, int k) {
  return SPMV_LOAD(reinterpret_cast<const PAIR *>(a + (k < k1 ? k : (k0 & ~1))));
}
// Which element addresses x for each half of the pair at k: kk is the pair that load_pair read, s0 / s1 (0 or 1) the element of
// it whose column the first / second half gathers with.  A half outside the block takes the pair's other element, an idle
// lane (it holds the block's first pair) element k0: always a column of this block, so no gather is predicated either.
struct pair_src { int kk, s0, s1; };
__device__ __forceinline__ pair_src pair_source(int k, int k0, int k1) {
  const bool in = k < k1;                       // the pair touches the block
  const bool v0 = in && k >= k0, v1 = in && (k + 1 < k1);
  return {in ? k : (k0 & ~1), v0 ? 0 : (in ? 1 : (k0 & 1)), v1 ? 1 : (in ? 0 : (k0 & 1))};
}
// The pair's two values (or products) into the LDS stage at their place in the block; halves outside the block go to
// the stage's last slot, which no block uses (nnz <= SPMV_BLOCK_CAP).
__device__ __forceinline__ void park_pair(double *stage, int k, int k0, int k1, double a, double b) {
  stage[(k >= k0 && k < k1) ? k - k0 : SPMV_BLOCK_NNZ - 1] = a;
  stage[(k + 1 < k1) ? k + 1 - k0 : SPMV_BLOCK_NNZ - 1] = b;
}

// sum + the products prod(j), j < 8 with k + j < end, in order.  pairsum == 0: one at a time (PetscSparseDensePlusDot, aij.h:383-386).
// pairsum != 0: two at a time, sum += p[j] + p[j+1], odd tail alone (MatMult_SeqAIJ_Inode / MatMultAdd_SeqAIJ_Inode,
// inode.c:430-440,619-631); k advances in eights from the row's start, so the pairs stay aligned with it.
template <class PROD> __device__ __forceinline__ double accumulate8(double sum, int k, int end, int pairsum, PROD prod) {
  if (!pairsum) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { const double u = sum + prod(j); sum = (k + j < end) ? u : sum; }
  } else {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const double pa = prod(j), pb = prod(j + 1);
      const double inc = (k + j + 1 < end) ? pa + pb : pa;
      const double u = sum + inc;
      sum = (k + j < end) ? u : sum;
    }
  }
  return sum;
}
// one lane's row sum out of the LDS product stage, 8 reads in flight (the order is chosen outside the loop)
__device__ __forceinline__ double row_sum_lds(const double *prod, int rs, int re, double sum, int pairsum) {
  auto run = [&](int pairs) {
    for (int k = rs; k < re; k += 8) {
      double t[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) t[j] = prod[(k + j < re) ? k + j : re - 1];
      sum = accumulate8(sum, k, re, pairs, [&](int j) { return t[j]; });
    }
  };
  if (!pairsum) run(0); else run(1);
  return sum;
}

// How a row's sum reaches y.  ADD == 0: y = A x.  ADD == 1: y = yin + A x (MatMultAdd).  ADD == 2: y = yin .* (A x), yin being a
// diagonal scaling (PCApply_Jacobi's VecPointwiseMult fused into the product: same bits as the two separate sweeps).
// ADD == 3: y = dv .* (yin + A x), one step of a Jacobi-sweep upper triangular solve (A the negated strict triangle, dv the
// inverted pivots; host/ilu.c); the plain row-block kernel only.  The sum starts from yin as for ADD == 1, so a one-lane row
// carries the bits of s = yin; s = s + a_j x_j ...; dv * s.
// ADD == 4: y = yin - A x, the residual r = b - A x (yin = b).  The row sum is the one ADD == 0 forms -- started from 0.0, the form's own
// order -- followed by ONE subtraction: the bits of the product into a work vector and VecAYPX(w, -1, b) behind it (b - w), without
// the write and the re-read of w.  A row without entries is b - 0.0.
template <int ADD> __device__ __forceinline__ double spmv_out(double yv, double t, double dv = 1.0) { return ADD == 4 ? yv - t : (ADD == 3 ? dv * (yv + t) : (ADD == 1 ? yv + t : (ADD == 2 ? yv * t : t))); }
template <int ADD> __device__ __forceinline__ double spmv_empty(double yv, double dv = 1.0) { return ADD == 4 ? yv - 0.0 : (ADD == 3 ? dv * yv : (ADD == 1 ? yv : (ADD == 2 ? yv * 0.0 : 0.0))); }
// same, for a sum that was started from yv when ADD == 1 or 3 (from 0.0 otherwise)
template <int ADD> __device__ __forceinline__ double spmv_fin(double yv, double s, double dv = 1.0) { return ADD == 4 ? yv - s : (ADD == 3 ? dv * s : (ADD == 2 ? yv * s : s)); }
static inline int spmv_y_streams(long nrows) { return (size_t)nrows * sizeof(double) >= ((size_t)256 << 20); }   // (vec_kernels.hip: vec_streams)
// nt: y beyond the Infinity Cache (vectors of >= 256 MiB) is written once and read by another kernel much later: a non-temporal store
// there (+3 % on P7(512), three of three alternations on one box: profiles/r04_spmv_p7_512_ab.log; nothing either way at P7(256))
__device__ __forceinline__ void spmv_store(double *p, double v, bool nt) { if (nt) __builtin_nontemporal_store(v, p); else *p = v; }

// A row's result out of the LDS product stage [rs, re) to *dst, by the row's tpr lanes (this one is lane `sub` of them; has_row:
// it has a row at all).  One lane: products added in column order starting from yv (ADD 1, 3) or 0.0 -- the reference's bits.
// Several: strided partial sums and a shuffle tree.  Returns what was stored, 0.0 on lanes that stored nothing.
template <int ADD>
__device__ __forceinline__ double row_result_lds(const double *prod, int tpr, int sub, bool has_row, int rs, int re, double yv, double dv,
                                                 int pairsum, double *dst, bool nt) {
  double res = 0.0;
  if (tpr == 1) {
    if (has_row) { res = spmv_fin<ADD>(yv, row_sum_lds(prod, rs, re, (ADD & 1) ? yv : 0.0, pairsum), dv); spmv_store(dst, res, nt); }
  } else {
    double sum = 0.0;
    if (has_row) for (int k = rs + sub; k < re; k += tpr) sum += prod[k];
    for (int off = tpr >> 1; off > 0; off >>= 1) sum += __shfl_down(sum, off, MI355X_WAVE);
    // (a row without entries is yv itself, as on the one-lane path: yv + 0.0 would turn yv = -0.0 into +0.0)
    if (has_row && sub == 0) { res = re == rs ? spmv_empty<ADD>(yv, dv) : spmv_out<ADD>(yv, sum, dv); spmv_store(dst, res, nt); }
  }
  return res;
}

// Sum of v over a workgroup of NW wavefronts in a fixed order: lanes -> wavefront tree -> lane 0 adds the wavefronts' values
// 0, 1, 2 ... in order.  The result is valid on lane 0 only.  Every lane of the workgroup must arrive (one barrier); the LDS
// slots are the helper's own and are not re-armed, so a kernel calls this at most once on any path.
template <int NW> __device__ __forceinline__ double workgroup_sum_ordered(double v) {
  __shared__ double wave_slot[NW];
  const int tid = threadIdx.x;
  v = wave_sum(v);
  if ((tid & (MI355X_WAVE - 1)) == 0) wave_slot[tid / MI355X_WAVE] = v;
  __syncthreads();
  double t = 0.0;
  if (tid == 0) {
    t = wave_slot[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) t += wave_slot[w];
  }
  return t;
}
