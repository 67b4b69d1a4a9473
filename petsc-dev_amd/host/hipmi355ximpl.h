/* Private header of the PLUGIN (libpetschipmi355x.so): the HIPMI355X Vec/Mat/PC implementations.
 *
 * Object model: in a PETSc tree (PETSCHIPMI355X_WITH_PETSC, integration/petsc-3.3/) PETSc's own private headers; on a box
 * without PETSc the harness's stand-ins (petsc-dev_amd/harness/petscimpl.h), which keep the reference's names for the
 * header fields (hdr.comm, hdr.type_name, hdr.state), the layouts (map->n, rmap, cmap), data / spptr, the flags
 * (petscnative, assembled, preallocated) and every function-table slot the types fill, so that the sources in this
 * directory compile against either.  What differs between the two is collected in the HIPOBJ_* / HipComm* names below. */
#ifndef HIPMI355XIMPL_H
#define HIPMI355XIMPL_H
#include "petschipmi355x.h"
#if defined(PETSCHIPMI355X_WITH_PETSC)
#include "hipmi355x_petsc33.h"          /* integration/petsc-3.3/: real petsc-private headers + the names below over MPI */
#else
#include "../harness/petscimpl.h"
#define MPI_Comm PetscComm               /* the plugin's sources use PETSc's spelling */
/* ---- what the plugin needs from "Sys" beyond the public API (all of it exists in libpetsc under these names) ---- */
#define HipCommSize(comm) ((comm)->size)
#define HipCommRank(comm) ((comm)->rank)
/* host collectives of the reference's set-up phase (MPI_Allgather / MPI_Allreduce / persistent send-recv pairs) */
#define HipCommAllgather(comm, sbuf, nbytes, rbuf) ((comm)->allgather((comm)->ctx, (sbuf), (nbytes), (rbuf)))
#define HipCommAllreduce(comm, buf, count, is_double, op) ((comm)->allreduce((comm)->ctx, (buf), (count), (is_double), (op)))
#define HipCommHasExchange(comm) ((comm)->exchange != NULL)
#define HipCommExchange(comm, ns, sp, sb, sbytes, nr, rp, rb, rbytes) ((comm)->exchange((comm)->ctx, (ns), (sp), (sb), (sbytes), (nr), (rp), (rb), (rbytes)))
/* the RCCL communicators hung on the communicator: slot 0 reductions (compute stream), slot 1 halo (halo stream) */
#define HipCommDevice(comm) ((mi355x_comm_t)(comm)->plugin[0])
#define HipCommDeviceHalo(comm) ((mi355x_comm_t)(comm)->plugin[1])
#define HipObjComm(obj) (((PetscObject)(obj))->comm)
#define HipObjTypeName(obj) (((PetscObject)(obj))->type_name)
#define HipObjPrefix(obj) (((PetscObject)(obj))->prefix)
#define HipObjState(obj) (((PetscObject)(obj))->state)
#define HipStateIncrease(obj) PetscObjectStateIncrease(obj)
#define HipFree(p) free(p)
#endif
#include "mi355x_kernels.h"
#include "mi355x_comm.h"

/* map a kernel-library (hipError_t) failure to PETSC_ERR_LIB like CHKERRCUSP, cuspvecimpl.h:79 */
#define CHKHIP(e) do { int e__ = (e); if (e__) SETERRQ(PETSC_COMM_SELF, PETSC_ERR_LIB, "HIP/RCCL error %d: %s", e__, mi355x_comm_error_string(e__)); } while (0)

/* ---- device context of this process (one GPU, two streams) ---- */
typedef struct {
  int initialized, device;
  mi355x_handle_t h;        /* compute stream */
  mi355x_handle_t hcomm;    /* halo stream ("second HIP stream" of the north star) */
} PetscDeviceCtx;
PetscErrorCode PetscDeviceGet(PetscDeviceCtx **ctx);   /* lazily creates handles; PETSC_ERR_LIB without a GPU */

/* ---- off-process entries set with VecSetValues / MatSetValues (harness flavour; inside a PETSc tree the parent classes stash:
 * src/vec/vec/utils/vecstash.c, src/mat/utils/matstash.c).  Entries wait here until the assembly, which hands every rank the
 * entries of all ranks in RANK order (the reference processes messages in arrival order). ---- */
typedef struct { PetscInt n, cap, *i, *j; PetscScalar *v; int mode; /* 0 unset, else InsertMode */ } HipStash;
PetscErrorCode HipStashAdd(HipStash *s, PetscInt i, PetscInt j, PetscScalar v, int mode);
PetscErrorCode HipStashExchange(MPI_Comm comm, HipStash *s, PetscInt *nrecv, PetscInt **ri, PetscInt **rj, PetscScalar **rv, int *mode);
void HipStashFree(HipStash *s);

/* ---- Vec ---- */
/* coherence flags, as PETSC_CUSP_UNALLOCATED/CPU/GPU/BOTH (include/petsc-private/vecimpl.h) */
enum { VALID_NONE = 0, VALID_HOST = 1, VALID_DEVICE = 2, VALID_BOTH = 3 };
typedef struct {
  PetscScalar *host;        /* host mirror, allocated on first host access; FIRST member, as VECHEADER (vecimpl.h:446-449) */
  PetscScalar *dev;         /* HBM */
  int valid;
  PetscScalar *placed_save; /* VecPlaceArray */
  int host_owned;
  PetscScalar *alias_save; int alias_valid;   /* "VecShareArrayBegin_C": the storage this vector owns while it borrows another's */
  HipStash stash;           /* off-process VecSetValues (harness flavour) */
} Vec_HIPMI355X;

PetscErrorCode VecCreate_SeqHIPMI355X(Vec v);
PetscErrorCode VecCreate_MPIHIPMI355X(Vec v);
PetscErrorCode VecCreate_HIPMI355X(Vec v);
PetscErrorCode VecCreateSeqHIPMI355X(MPI_Comm comm, PetscInt n, Vec *v);
/* device pointers with coherence (analogue of VecCUSPGetArrayRead/Write, cuspvecimpl.h:95-150) */
PetscErrorCode VecHIPGetRead(Vec v, const PetscScalar **d);
PetscErrorCode VecHIPGetWrite(Vec v, PetscScalar **d);       /* contents will be overwritten */
PetscErrorCode VecHIPGetReadWrite(Vec v, PetscScalar **d);
PetscErrorCode VecHIPRestoreWrite(Vec v);                    /* device newer; state++ */
PetscErrorCode VecHIPFlushBorrowed(Vec v);                   /* v borrows another vector's device storage and was written on the host: the values go there now (else nothing) */
#define PETSC_HIP_DPI_SLOT 8   /* device scratch slot holding p'w between the dot (or the SpMV by-product) and the CG update */
PetscErrorCode MatMultTDotBegin_HIPMI355X(Mat A, Vec x, Vec y, PetscBool *ok);   /* y = A x, x'y left on the device */
PetscErrorCode MatMultDiagonalScale_HIPMI355X(Mat A, Vec d, Vec x, Vec y, PetscBool *ok);   /* y = d .* (A x) */

/* ---- VecScatter (VecScatter_MPI_General, include/petsc-private/vecimpl.h:509-555) ---- */
typedef struct {
  PetscInt n;                 /* number of neighbours */
  PetscInt *procs, *starts, *indices;
  PetscInt *d_indices;        /* device copy */
  PetscScalar *d_values;      /* device message buffer */
  PetscBool contiq;           /* indices contiguous: exchange in place (vpscat.c:1951-1960) */
  PetscInt local_n;
  PetscInt *local_slots, *d_local_slots;
} VecScatterSide;
/* the plugin's own scatter context: device index lists, message buffers, events.  On the harness it IS the VecScatter
 * (there is no other); inside a PETSc tree it lives beside the reference's Mvctx, which MatMult no longer uses. */
#if !defined(PETSCHIPMI355X_WITH_PETSC)
typedef struct _p_VecScatter *HipScatter;
struct _p_VecScatter {
#else
typedef struct _p_HipScatter *HipScatter;
struct _p_HipScatter {
#endif
  MPI_Comm comm;
  VecScatterSide to, from;
  PetscBool inuse;            /* guard, vscat.c:1637 */
  mi355x_event_t ev_packed, ev_done;
  int device_ready;
  int ready_marked;           /* ev_packed already recorded by VecScatterMarkReady */
  PetscScalar *h_send, *h_recv;   /* host staging buffers of the host-staged transport */
  void *nbr_work;                 /* per-neighbour work arrays of an exchange (pointers, counts, ranks, byte counts): sized for max(to.n, from.n) */
  PetscScalar *d_local_tmp;       /* device staging of the local (self) part, local_n doubles */
  /* per-exchange device timing for bench.py: event pairs on the HALO stream around each forward exchange (first operation after the
   * wait on "x is final" .. last operation before "halo done") */
  PetscBool timing; PetscInt time_n, time_cap; mi355x_event_t *time_ev;
};
PetscErrorCode HipScatterCreate_PtoS_MPIAIJ(MPI_Comm comm, PetscLayout xmap, PetscInt ec, const PetscInt *garray, HipScatter *ctx);
PetscErrorCode HipScatterMarkReady(HipScatter ctx, Vec x);
PetscErrorCode HipScatterBegin(HipScatter ctx, Vec x, Vec y, InsertMode addv, ScatterMode mode);
PetscErrorCode HipScatterEnd(HipScatter ctx, Vec x, Vec y, InsertMode addv, ScatterMode mode);
PetscErrorCode HipScatterDestroy(HipScatter *ctx);
PetscErrorCode HipScatterSetTiming(HipScatter ctx, PetscBool on);
PetscErrorCode HipScatterGetLists(HipScatter ctx, PetscInt *nrecv, const PetscInt **rprocs, const PetscInt **rstarts, const PetscInt **rindices,
                                  PetscInt *nsend, const PetscInt **sprocs, const PetscInt **sstarts, const PetscInt **sindices,
                                  PetscInt *nlocal, const PetscInt **lto, const PetscInt **lfrom);

/* ---- Mat ---- */
/* host CSR container: the part of Mat_SeqAIJ the path needs (src/mat/impls/aij/seq/aij.h:10-39,99-115), same member
 * names.  On the harness it IS the container (A->data) and aijhip.c assembles into it; inside a PETSc tree the parent
 * type MATSEQAIJ owns the container (aij.h) and this struct is a VIEW of its arrays, refreshed at MatAssemblyEnd and
 * kept in the device mirror (integration/petsc-3.3/aijhipmi355x.c) -- the kernels' callers read the same fields. */
typedef struct {
  PetscInt m, n;            /* local rows / columns */
  PetscInt *i, *j;          /* row pointer / column index */
  PetscScalar *a;
  PetscInt *ilen, *imax;    /* used / allocated per row during assembly */
  PetscInt nz, maxnz;
  PetscInt bs;              /* block size (BAIJ reuse: i,j index blocks, a holds bs*bs per block) */
  PetscBool compact;        /* rows are packed (after assembly) */
  PetscInt nonzerorows;
  PetscInt inode_count, *inode_size;   /* Mat_SeqAIJ_Inode node_count / size (aij.h:99-115); 0 / NULL: plain routines */
  PetscBool keepnonzeropattern;        /* MAT_KEEP_NONZERO_PATTERN (aij.h); on the harness only: inside a PETSc tree the parent's member is read */
} HipAIJ;

/* ---- factored matrices: what MatGetFactor(A, "petsc", MAT_FACTOR_ILU | MAT_FACTOR_ICC, &F) hangs on F (host/ilu.c, host/icc.c;
 * the role of Mat_SeqAIJCUSPARSETriFactors, src/mat/impls/aij/seq/seqcusparse/cusparsematimpl.h) ---- */
typedef struct {
  MatFactorType kind;                                      /* MAT_FACTOR_ILU or MAT_FACTOR_ICC */
  PetscInt n, nz;                                          /* rows; stored entries of the FACTOR (the operator's with zero fill) */
  PetscInt levels, nzA;                                    /* ILU(k): the levels of fill of the last factorisation and the operator's entry count */
  /* one member per form of the factor; releasing a form frees its members and zeroes it (host/ilu.c, "releasing a factor") */
  /* ILU(0): host factor in the reference's L / reversed-U layout (aijfact.c:1628-1700); owns: ours (harness), or the arrays of F's own Mat_SeqAIJ (inside PETSc) */
  struct { PetscInt *bi, *bj, *bdiag; PetscScalar *ba; PetscBool owns; } host;
  /* dependency levels of L / U, and the level of every row: for the time of the solves' analysis; the device route keeps them with its context (else NULL) */
  struct { PetscInt nlevL, nlevU, *rlevL, *rlevU; } lev;
  struct {                                                 /* the level-scheduled ILU kernels, one launch per level */
    PetscInt *d_bi, *d_bj, *d_bdiag; PetscScalar *d_ba;    /* device copies of the factor (d_ba: the device route's factor itself) */
    PetscInt *levptrL, *levptrU;                           /* where each level's rows start (host) */
    PetscInt *d_rowsL, *d_rowsU;                           /* rows ordered by level (device) */
    PetscScalar *d_work; void *graph; int graph_tried;     /* hipGraph of the level launches working in place on d_work */
    int borrowed;                                          /* d_bi / d_bj / d_bdiag / d_rowsL are the device route's context's: not ours to free */
  } launch;
  struct {
    mi355x_trisolve_plan_t tri_lo, tri_up;                 /* sync-free solves (NULL: level launches) */
    int by_level;                                          /* rows summed in dependency-level order (inode matrices) instead of column order */
    int block_columns;                                     /* node plans whose columns are whole dependency nodes */
    PetscInt nodes, nlevL_nodes, nlevU_nodes;              /* node-blocked plans (the factor of a matrix with inodes): nodes and their levels; 0: row-granular */
    int use_levels;                                        /* a sync-free application gave up: THESE plans run level by level from now on; the next factorisation builds new plans and starts sync-free again (f->aborted remembers) */
  } syncfree;
  /* -pc_factor_hipmi355x_trisolve sweeps:<k>: k Jacobi sweeps per triangle instead of the exact solves (sweeps 0: exact).  The negated
   * strict triangles as CSR with their SpMV plans, the inverted pivots, two work vectors.  A numeric factorisation with the pattern
   * they were built for re-sends values only: the host route keeps that pattern (bi / bj / bdiag) and compares; the device route's
   * (from_device) is the pattern of its context, which forgets this form when it is rebuilt */
  struct {
    PetscInt sweeps, n, nz, *bi, *bj, *bdiag; int from_device;
    mi355x_spmv_plan_t planL, planU;
    PetscInt *iL, *jL, *iU, *jU; PetscScalar *aL, *aU, *dinv, *work[2];
  } sw;
  /* -pc_factor_hipmi355x_numeric device: the numeric factorisation runs on the device (mi355x_ilu0_factor_*), level by level, into
   * launch.d_ba.  The context is built once per pattern; with it stay the host pattern (host.bi / bj / bdiag), the row levels
   * (lev.rlevL / rlevU) and what the level-launch solves borrow from it (launch.borrowed).  gen / n / nz: the serial number of the
   * operator's pattern upload (Mat_SeqAIJHIP.pattern_gen) and its sizes at the time, levels: the levels of fill the factor's pattern was built
   * with -- what "the pattern of the last factorisation" is told by */
  struct { mi355x_ilu0_factor_t dfac; int stale; unsigned long long gen; PetscInt n, nz, levels, nblk, *blk; } dev;
  /* MatSolveTranspose (host/ilu.c, "the transposed factor"): U^T and L^T as two CSR triangles on the device, rows in the order the
   * reference's scatter loop reaches an entry (csrc/trisolve_transpose.hip), built at the first transposed solve after a factorisation.
   * Pattern side, once per pattern: the index arrays, perm (position in ba of every value: U^T's, L^T's, then the n inverted diagonals),
   * the level lists, the captured graph of the nlev1 + nlev2 launches, and the host pattern they were built for (bi / bj / bdiag: a
   * factorisation that leaves the same one refills val only).  fresh: val holds the current factor's values */
  struct {
    PetscInt n, nz, levels, nzU, nzL, *bi, *bj, *bdiag, *perm;   /* (perm: host copy, for a factor whose values are on the host only) */
    PetscInt *d_ti, *d_tj, *d_si, *d_sj, *d_perm; PetscScalar *d_val;
    PetscInt nlev1, nlev2, *levptr1, *levptr2, *d_rows1, *d_rows2;
    PetscScalar *d_work; void *graph; int graph_tried;
    int built, fresh;
    PetscInt pattern_builds, value_refreshes;              /* (the counts outlive the form) */
  } tr;
  PetscInt symbolic_builds, numeric_runs;                  /* host symbolic passes / numeric factorisations so far (both routes) */
  int aborted;                                             /* a sync-free application of this factor gave up at some time (kept over re-factorisations) */
  PetscInt nshift;                                         /* restarts / shifts the factorisation took (largest count over the blocks) */
  int factored_state; void *factored_of;                   /* operator and operator state of the last numeric factorisation */
  PetscInt nblk, *blk;                                     /* "MatFactorSetIndependentBlocks_C": the matrix stands for that many separate matrices (row ranges) */
  PetscErrorCode (*parent_destroy)(Mat);                   /* inside PETSc: the parent factor matrix's destroy */
} HipTriFactors;
PetscErrorCode HipTriFactorsDestroy(HipTriFactors **f);
void HipTriFactorsResetNumeric(HipTriFactors *f);                /* forget one numeric factorisation (host/ilu.c) */
PetscInt HipTriFactorsBlocks(const HipTriFactors *f, PetscInt n, PetscInt whole[2], const PetscInt **blk);   /* the independent blocks a factorisation of n rows runs over */
/* where the set-up time goes, on stderr under PETSC_HIPMI355X_SETUP_TIMING: a line; the line of the phase that began at clock (moved on) */
double HipWallSeconds(void);
#define HipSetupNote(...) do { if (getenv("PETSC_HIPMI355X_SETUP_TIMING")) fprintf(stderr, "[hipmi355x] " __VA_ARGS__); } while (0)
#define HipSetupTick(clock, what) do { const double t__ = HipWallSeconds(); HipSetupNote("  %-34s %.6f s\n", what, t__ - (clock)); (clock) = t__; } while (0)
PetscErrorCode HipTriFactorsApply(Mat F, HipTriFactors *f, Vec b, Vec x, PetscLogDouble flops);
typedef void (*HipRangeFn)(void *ctx, PetscInt lo, PetscInt hi);
void HipParallelRanges(PetscInt n, HipRangeFn fn, void *ctx);   /* fn over contiguous parts of [0, n) on HipHostThreads(16) host threads (hipsys.c); one thread below 200 000 */
int HipHostThreads(int cap);                                    /* host threads this RANK may use for set-up passes: affinity mask, cgroup quota, ranks on the node (hipsys.c) */
typedef PetscErrorCode (*HipProductNowFn)(Mat A, Vec x, Vec t);                           /* t = A x, launched now */
typedef PetscErrorCode (*HipProductScaledFn)(Mat A, Vec d, Vec x, Vec w, PetscBool *ok);   /* w = d .* (A x) in one kernel */
PetscErrorCode VecHIPNoteProduct(Mat A, Vec x, Vec t, HipProductNowFn now, HipProductScaledFn scaled, PetscBool *noted);   /* host/vechip.c, "a noted product" */
PetscErrorCode VecHIPProductMatrixChanges(Mat A);              /* to be called before A's device values change or go away */
PetscErrorCode VecHIPMI355XFlushDeferred(void);                /* host/vechip.c: run the noted element-wise operations */
PetscErrorCode VecHIPMI355XSetDeferral(PetscInt on);
PetscErrorCode VecHIPMI355XGetDeferralCounts(PetscInt counts[8]);   /* shortcuts taken so far: CG sweep, BiCGStab update, MAXPY + norm, product + dot, product + dotnorm2, scaled product, work vector written late, dot answered from the kept value */
void HipFactorJoinHelpers(void);                              /* host/ilu.c: the thread that returns the factorisation's work arrays */
PetscErrorCode HipTriWatchCheck(void);                     /* at every host wait: did a sync-free solve queued earlier give up? */
void HipTriWatchAdd(HipTriFactors *f);
PetscErrorCode MatICCFactorSymbolic_SeqAIJHIP(Mat F, Mat A, IS perm, const MatFactorInfo *info);
PetscErrorCode MatGetFactor_seqaijhipmi355x_petsc(Mat A, MatFactorType ftype, Mat *B);
PetscErrorCode MatGetFactorAvailable_seqaijhipmi355x_petsc(Mat A, MatFactorType ftype, PetscBool *flg);

/* ---- block ILU(k) of MATSEQBAIJHIPMI355X (host/bilu.c; harness flavour -- inside a PETSc tree the BAIJ type composes no factor): what
 * MatGetFactor(A, "petsc", MAT_FACTOR_ILU, &F) hangs on F for a block matrix.  The factor in the point factor's layout over block rows
 * and columns, one column-major bs x bs block per stored entry, the inverted diagonal block at bdiag[i].  Two forms, each released by
 * one function: the pattern side (host layout, level lists, their device copies, the launch plans; once per pattern) and the values
 * (host ba, d_ba). ---- */
#define HIP_BILU_CHAIN_ROWS 128                            /* default of -pc_factor_hipmi355x_bilu_chain_rows: the best value of the measured sweep (block ILU(k)) */
typedef struct {
  PetscInt mbs, bs, levels, nzb, nzbA;                     /* block rows, block size, levels of fill, stored blocks of the factor / of the operator */
  struct {
    PetscInt *bi, *bj, *bdiag;                             /* host layout (mi355x_iluk_symbolic_host on the block pattern) */
    PetscInt nlevL, nlevU, *levptrL, *levptrU;             /* dependency levels of L / U over block rows; where each level's rows start (host) */
    PetscInt *d_bi, *d_bj, *d_bdiag, *d_rowsL, *d_rowsU;   /* device: the layout, the block rows ordered by level */
    PetscInt *d_levptrL, *d_levptrU;                       /* device copies of levptrL / levptrU: what a chain launch walks (trisolve fused) */
    PetscInt nsegL, nsegU, *segL, *segU, plan_rows;        /* host: the launches of one application per triangle (mi355x_bilu_chain_plan_host): seg[0 .. nseg] where each
                                                              segment's levels start, then seg[nlev + 1 + s] != 0: segment s is one chain launch; the max_rows they were cut for */
    int stale; unsigned long long gen;                     /* a new symbolic phase was asked for; serial number of the operator's pattern upload the layout was built for */
  } pat;
  PetscScalar *ba, *d_ba;                                  /* the factor's (nzb + 1) bs^2 values, host and device */
  PetscInt symbolic_builds, numeric_runs;                  /* pattern passes / numeric factorisations so far */
  int factored_state; void *factored_of;                   /* operator and operator state of the last numeric factorisation */
  int fused; PetscInt chain_rows;                          /* -pc_factor_hipmi355x_trisolve fused, -pc_factor_hipmi355x_bilu_chain_rows of the last set-up */
} HipBlockFactors;
PetscErrorCode HipBlockFactorsDestroy(HipBlockFactors **f);
PetscErrorCode MatGetFactor_seqbaijhipmi355x_petsc(Mat A, MatFactorType ftype, Mat *B);
PetscErrorCode MatGetFactorAvailable_seqbaijhipmi355x_petsc(Mat A, MatFactorType ftype, PetscBool *flg);

/* one device form of the product: (B)CSR arrays (bs = 1: CSR) with the row-block plan over their value stream, and the column-tiled layout
 * when one was chosen for it.  The device copy of the matrix is one; the forms derived from it (the cached transpose, the blocked companion
 * and its block transpose) hold the matrix's values in another order, a = d_a[perm], refreshed by one gather (host/aijhip.c) */
typedef struct {
  PetscInt *i, *j, *perm;           /* device; perm NULL: the matrix's own arrays, or values placed from the host (the BAIJ transpose) */
  PetscScalar *a;
  mi355x_spmv_plan_t plan;
  PetscInt bs, nblocks;             /* block size (1: CSR), stored blocks */
  mi355x_spmv_tiled_t tiled;        /* column-tiled layout (csrc/spmv_tiled.hip: x staged in LDS) for gathers that miss the caches; NULL: the row-block kernels */
  PetscBool fresh;                  /* a (and the tiled layout's copy of it) hold the matrix's current device values */
} HipDevForm;

/* what the result of MatMatMult / MatTranspose / MatPtAP carries (host/aijhip.c, "Sparse matrix products"): the operands it was built
 * from -- told by address, sizes, entry counts and the serial numbers of their pattern uploads (0: never uploaded, the host route), never
 * dereferenced through here -- and what a repeated numeric phase on unchanged patterns needs */
typedef struct {
  int kind;                                  /* 1: C = A B; 2: B = A^T; 3: C = P^T A P */
  int route;                                 /* 1 device, 2 host: as the symbolic phase found -mat_hipmi355x_product */
  void *op[2]; PetscInt op_nz[2]; unsigned long long op_gen[2];
  mi355x_spgemm_plan_t plan;                 /* kind 1, and kind 3 for Pt (AP) */
  PetscInt *perm_h, *perm_d;                 /* kind 2: position in A^T -> position in A (device copy on the device route) */
  Mat Pt, AP;                                /* kind 3: the inner results, products of kind 2 and 1 themselves */
  PetscInt symbolic_builds, device_numerics, host_numerics;
} HipMatProduct;

/* the options of the sequential AIJ types (host/aijhip.c, "the type's options"): the integer ones, HOPT_*, index Mat_SeqAIJHIP.opt[] and
 * opt_set[]; the route options, HROUTE_* -- one of two words each -- index route[] and the route table hroute[] */
enum { HOPT_IC = 0, HOPT_RP, HOPT_VP, HOPT_TILED, HOPT_TILED_SMIN, HOPT_BLOCKED, HOPT_UPDATE_DEV, HOPT_PR, HOPT_N };
enum { HROUTE_SOR = 0, HROUTE_PRODUCT, HROUTE_REDUCTIONS, HROUTE_RESIDUAL, HROUTE_COARSEN, HROUTE_N };

/* device mirror */
typedef struct {
  HipDevForm mat;           /* the device copy of the matrix (compressed rows: the rows with entries only) */
  int uploaded_state;        /* Mat state at last upload (compare state instead of valid_GPU_matrix) */
  /* compressed-row form for mostly-empty blocks (src/mat/utils/compressedrow.c:28) */
  PetscBool cprow;            /* compressed-row form requested (off-diagonal block) */
  PetscBool baij4_mfma;       /* BAIJ bs = 4: MatMult on the matrix cores (mi355x_spmv_bsr4_mfma) */
  PetscInt pattern_nz;        /* nz of the pattern the mirror was built for (-1: none) */
  unsigned long long pattern_gen;   /* serial number of that pattern upload, unique in the process over all matrices (0: none): what a
                                     * consumer that keeps pattern-derived state compares, never addresses (host/ilu.c, the device route) */
  HipDevForm t;               /* cached explicit transpose for MatMultTranspose (perm: position in A^T -> position in A); its column-tiled
                               * layout is built when the matrix itself took that form */
  PetscInt t_builds, t_refreshes;   /* host builds / device refreshes so far */
  PetscInt n_uploads;        /* value uploads so far */
  /* MatSetValuesBatch map for one connectivity (rows array): contributions grouped by nonzero, in call order */
  PetscInt bm_nb, bm_bs, bm_nseg; unsigned long long bm_hash; size_t bm_T, bm_vcap;
  PetscInt *bm_order, *bm_segptr, *bm_segslot;   /* device */
  PetscScalar *bm_v;                             /* device staging of the element values */
  /* the blocked companion of an AIJ matrix whose nodes are complete bs x bs blocks (3-dof FEM matrices): BCSR arrays multiplied by the
   * BAIJ row-block kernel (host/aijhip.c, "blocked companion"), and its block transpose, for the transpose products */
  HipDevForm b, tb;
  /* MatShift / MatAXPY / MatCopy with an unchanged pattern (host/aijhip.c, "MatShift, MatAXPY and MatCopy"): the position of every row's
   * diagonal entry (host; sh_full: every row has one), kept for the pattern upload sh_gen; the map of a SUBSET_NONZERO_PATTERN update
   * into this matrix, xtoy[k] = position in this matrix of entry k of X (host and device), kept for the pair of pattern uploads
   * (xtoy_xgen of X, xtoy_ygen of this matrix; 0: built for one call -- a matrix never sent to the device has no serial number, and
   * its map is built again by every update); the pair a same-pattern claim was last verified for */
  PetscInt *sh_diag; PetscBool sh_full; unsigned long long sh_gen;
  PetscInt *xtoy_h, *xtoy_d, xtoy_nz; unsigned long long xtoy_xgen, xtoy_ygen; void *xtoy_from;
  unsigned long long same_xgen, same_ygen;
  /* MatZeroRows / MatZeroRowsColumns with the pattern kept (host/aijhip.c, "MatZeroRows and MatZeroRowsColumns"): the list of the last
   * call as it was passed (host copy, zr_n entries; zr_have: there is one, possibly empty), the same list and its bitmap -- one bit per
   * row, zr_words words -- on the device.  A call with a list of the same length and content reuses them.  The counts outlive them:
   * uploads of a list to the device, updates that ran on the device copy */
  PetscInt *zr_rows_h, *zr_rows_d, zr_n, zr_words; unsigned int *zr_mask_h, *zr_mask_d; PetscBool zr_have;
  PetscInt zr_list_uploads, zr_device_updates;
  /* MatSOR (host/aijhip.c, "MatSOR"): the level plan of the pattern upload plan_gen (csrc/sor.hip), and with the matrix the work vector t
   * and the inverted / plain diagonal -- on the device as built for the values of upload state idiag_state with (omega, fshift), on the
   * host (the host route) for the object state h_state.  The counts outlive the arrays: diagonal builds (either route), plan builds,
   * applications on the device */
  struct {
    mi355x_sor_plan_t plan; unsigned long long plan_gen;
    PetscScalar *d_idiag, *d_mdiag, *d_t; int idiag_state; PetscReal omega, fshift; PetscBool have;
    PetscScalar *h_idiag, *h_mdiag, *h_t; int h_state; PetscReal h_omega, h_fshift; PetscBool h_have; PetscInt h_m;
    PetscInt idiag_builds, plan_builds, device_applications;
  } sor;
  HipMatProduct *prod;       /* the matrix is the result of a product (NULL: an ordinary matrix) */
  /* MatNorm / MatGetRowMaxAbs / Max / Min / MatGetColumnNorms (host/aijhip.c, "Norms and row / column reductions"): the device work array
   * the row results and their locations go to before the finishing pass or the copy to the caller's host array (red_cap bytes; goes
   * with the pattern) */
  void *red_work; size_t red_cap;
  PetscInt residual_fused, residual_calls;   /* "MatResidual_C" (host/aijhip.c): residuals that took the fused kernel / the product and VecAYPX */
  /* "MatCoarsenAggregate_C" (host/aijhip.c): coarsenings of this matrix per route so far and the rounds of the last one on the device */
  PetscInt coarsen_device, coarsen_host, coarsen_rounds;
  PetscInt opt[HOPT_N]; PetscBool opt_set[HOPT_N];   /* the integer options as MatSetFromOptions read them under the matrix's prefix */
  /* the route options (the table hroute[] in host/aijhip.c states each one's rule): route[k] is 1 or 2 for the option's first or second
   * word (device / host, fused / calls) as MatSetFromOptions read it under the matrix's prefix -- or, for an option whose global answer
   * is kept (sor, reductions), as the matrix's first use resolved it -- and 0 while neither has happened.  residual_global: what the
   * global database said to -mat_hipmi355x_residual when the device copy was last built for a new pattern (0: nothing) */
  int route[HROUTE_N], residual_global;
  /* per-launch device timing for bench.py (hipEvent pairs on the compute stream) */
  PetscBool timing; PetscInt time_n, time_cap; mi355x_event_t *time_ev;
#if defined(PETSCHIPMI355X_WITH_PETSC)
  HipAIJ view;               /* of the parent's Mat_SeqAIJ (or Mat_SeqBAIJ: baij_parent) */
  PetscBool baij_parent;
#else
  HipTriFactors *tri;        /* a factored matrix (A->factortype != MAT_FACTOR_NONE): its triangular factors on the device */
  HipBlockFactors *btri;     /* ... of a BAIJ operator: its block triangular factors (host/bilu.c); at most one of the two is set */
#endif
} Mat_SeqAIJHIP;
/* where a factored matrix keeps its device-side factors: inside PETSc the factor is the PARENT's matrix (MATSEQAIJ for ILU, MATSEQSBAIJ
 * for ICC, from MatGetFactor_seqaij_petsc) whose spptr is free; on the harness it is a matrix of this type */
#if defined(PETSCHIPMI355X_WITH_PETSC)
#define HipTriGet(F) ((HipTriFactors *)(F)->spptr)
#else
#define HipTriGet(F) (((Mat_SeqAIJHIP *)(F)->spptr)->tri)
#define HipBlockGet(F) (((Mat_SeqAIJHIP *)(F)->spptr)->btri)
#endif
#if defined(PETSCHIPMI355X_WITH_PETSC)
#define HipAIJGet(A) (&((Mat_SeqAIJHIP *)(A)->spptr)->view)
#else
#define HipAIJGet(A) ((HipAIJ *)(A)->data)
#endif

/* the members of Mat_MPIAIJ the path needs (src/mat/impls/aij/mpi/mpiaij.h:35-77), same names, with the plugin's scatter
 * in place of Mvctx.  On the harness it IS the container (A->data); inside a PETSc tree the parent MATMPIAIJ owns the
 * container and this struct hangs off A->spptr with A, B, garray aliasing the parent's after each assembly. */
typedef struct {
  Mat A, B;                 /* diagonal / off-diagonal blocks (SeqAIJHIPMI355X) */
  PetscInt *garray, ec;
  Vec lvec;
  HipScatter hscat;
  PetscInt rstart, rend, cstart, cend;
  HipStash stash;           /* off-process MatSetValues (harness flavour) */
  PetscBool keepnonzeropattern;   /* MAT_KEEP_NONZERO_PATTERN for blocks that are made later (harness flavour; the blocks hold their own) */
  Vec sor_bb1;              /* MatSOR: b + B lvec of the outer steps; made by the first call that needs it */
} HipMPIAIJ;
#if defined(PETSCHIPMI355X_WITH_PETSC)
#define HipMPIAIJGet(A) ((HipMPIAIJ *)(A)->spptr)
#else
#define HipMPIAIJGet(A) ((HipMPIAIJ *)(A)->data)
#endif

PetscErrorCode MatCreate_SeqAIJHIPMI355X(Mat);
PetscErrorCode MatCreate_MPIAIJHIPMI355X(Mat);
PetscErrorCode MatCreate_AIJHIPMI355X(Mat);
PetscErrorCode MatCreate_SeqBAIJHIPMI355X(Mat);
PetscErrorCode MatSeqAIJHIPUpload(Mat A);
PetscErrorCode MatSeqAIJHIPGetInodes(Mat A, PetscInt *count, const PetscInt **sizes);
PetscErrorCode MatSeqAIJHIPSetCompressedRow(Mat A, PetscBool flg);
/* Y += a X and B <- A between sequential matrices of this type whose columns are numbered through xcols / ycols (NULL: as stored; the
 * off-diagonal blocks of two MPIAIJ matrices, each compacted through its own garray); ...Check: the errors these would return, nothing
 * changed; checked: the caller has just made that check for this pair and nothing happened since */
PetscErrorCode MatAXPY_SeqAIJHIP_Cols(Mat Y, PetscScalar a, Mat X, MatStructure str, const PetscInt *xcols, const PetscInt *ycols, PetscBool checked);
PetscErrorCode MatCopy_SeqAIJHIP_Cols(Mat A, Mat B, MatStructure str, const PetscInt *acols, const PetscInt *bcols, PetscBool checked);
PetscErrorCode MatValueOpsCheck_SeqAIJHIP(Mat Y, Mat X, MatStructure str, const PetscInt *xcols, const PetscInt *ycols, PetscBool copy);
/* the reductions over one block of an MPIAIJ matrix (host/aijhip.c, "Norms and row / column reductions"); route: 1 device, 2 host */
PetscErrorCode MatReductionsRoute_SeqAIJHIP(Mat A, int *route);
PetscErrorCode MatBlockRowReduce_SeqAIJHIP(Mat A, int route, int op, PetscInt ncols, PetscBool add, PetscScalar *out, PetscInt *idx);
PetscErrorCode MatBlockColReduce_SeqAIJHIP(Mat A, int route, int op, PetscScalar *out_host);
PetscErrorCode MatBlockSquareSum_SeqAIJHIP(Mat A, int route, PetscReal *s);
PetscErrorCode HipDeviceMaxOf(const PetscScalar *x_dev, PetscInt n, PetscReal *val);
PetscErrorCode MatSetUpMultiply_MPIAIJ(Mat mat);
PetscErrorCode MatTimingBegin(Mat A, mi355x_handle_t h);
PetscErrorCode MatTimingEnd(Mat A, mi355x_handle_t h);
PetscErrorCode MatGetVecs_HIPMI355X(Mat A, Vec *right, Vec *left);
PetscErrorCode PCCreate_PBJacobi_HIPMI355X(PC);
/* "VecSplitReductionOps_C" on a Vec: the three phases of a split reduction as the type provides them (host/vechip.c composes it, the
 * object model's VecDotBegin / VecNormBegin / VecDotEnd / VecNormEnd / PetscCommSplitReductionBegin look it up, and so does
 * host/kspfused.c, which takes none of those five names from the object model's library) */
typedef struct {
  PetscErrorCode (*dot_begin)(Vec, Vec, PetscScalar *);
  PetscErrorCode (*dot_end)(Vec, Vec, PetscScalar *);
  PetscErrorCode (*norm_begin)(Vec, NormType, PetscReal *);
  PetscErrorCode (*norm_end)(Vec, NormType, PetscReal *);
  PetscErrorCode (*comm_begin)(MPI_Comm);
} VecSplitReductionOps;
PetscErrorCode KSPCreate_CGHIPMI355X(KSP);
PetscErrorCode KSPCreate_GMRESHIPMI355X(KSP);
PetscErrorCode KSPCreate_BCGSHIPMI355X(KSP);
PetscErrorCode KSPCreate_ChebychevHIPMI355X(KSP);
PetscErrorCode KSPCreate_RichardsonHIPMI355X(KSP);
PetscErrorCode KSPCreate_PIPECGHIPMI355X(KSP);
PetscErrorCode KSPCreate_MINRESHIPMI355X(KSP);
PetscErrorCode KSPCreate_TFQMRHIPMI355X(KSP);
PetscErrorCode KSPCreate_CGSHIPMI355X(KSP);
PetscErrorCode KSPCreate_BICGHIPMI355X(KSP);
PetscErrorCode KSPCreate_LSQRHIPMI355X(KSP);
PetscErrorCode KSPCreate_FGMRESHIPMI355X(KSP);

#endif
