/* Factored matrices of MATSEQAIJHIPMI355X, ILU(0) part, behind the reference's own factorisation interface:
 *
 *   MatGetFactor(A, "petsc", MAT_FACTOR_ILU | MAT_FACTOR_ICC, &F)      "MatGetFactor_petsc_C" composed on every matrix of the type
 *   MatILUFactorSymbolic(F, A, ...) / MatICCFactorSymbolic(F, A, ...)   F->ops->ilufactorsymbolic / iccfactorsymbolic
 *   MatLUFactorNumeric(F, A, info) / MatCholeskyFactorNumeric(F, A, info)
 *   MatSolve(F, b, x)                                                   F->ops->solve  = the device triangular solves
 *
 * so that an UNCHANGED PCILU / PCICC / PCBJACOBI (PETSc's own inside a PETSc tree, the harness's pcfactor.c on a box without
 * PETSc) reaches the device solves -- how the reference's GPU back end does it (MatGetFactor_seqaij_cusparse,
 * MatLUFactorNumeric_SeqAIJCUSPARSE installing MatSolve_SeqAIJCUSPARSE, src/mat/impls/aij/seq/seqcusparse/aijcusparse.cu:57-75,
 * 175-200,358-445), and like it the factorisation itself runs on the host copy of the matrix.
 *
 *   numeric : MatILUFactorSymbolic_SeqAIJ_ilu0 + MatLUFactorNumeric_SeqAIJ (src/mat/impls/aij/seq/aijfact.c:1628, :461), natural
 *             ordering.  Inside a PETSc tree those routines themselves (the parent class's); on the harness their restatement
 *             below.  Then a dependency-level analysis of L and U and one upload.
 *   solve   : MatSolve_SeqAIJ_NaturalOrdering (aijfact.c:3126) on the device, one lane per row in column order (same bits): by
 *             default two launches, one per triangular solve, with point-to-point hand-off of the solution values between
 *             wavefronts (mi355x_trisolve_*, csrc/trisolve.hip); -pc_factor_hipmi355x_trisolve level selects the level-scheduled
 *             kernels, one launch per dependency level (replayed from a hipGraph), which also serve systems with few levels.
 *             -pc_factor_hipmi355x_trisolve sweeps:<k> (opt-in, an APPROXIMATE application): k Jacobi sweeps per triangle, each one
 *             SpMV-shaped product with the negated strict triangle (ilu0_sweeps_* below). */
#include "hipmi355ximpl.h"
#include <pthread.h>
#include <sched.h>
#include <time.h>
#include <unistd.h>
#if defined(PETSCHIPMI355X_WITH_PETSC)
#include <../src/mat/impls/aij/seq/aij.h>
EXTERN_C_BEGIN
extern PetscErrorCode MatGetFactor_seqaij_petsc(Mat, MatFactorType, Mat *);
EXTERN_C_END
#endif

/* ---------------------------------------------------------------- sync-free solves that gave up: noticed at the next host wait
 * A dependency wait of the sync-free kernels is bounded; a lane that gives up raises a flag in pinned host memory and the
 * application's result is unusable.  The flag cannot be read before the kernels have run, so every factored matrix with
 * sync-free plans is on a watch list, and every host wait the solvers already perform (reduction results, VecGetArray:
 * HipTriWatchCheck, called from vechip.c) looks at the flags: the first wait after an abort returns PETSC_ERR_LIB instead of
 * numbers computed from a poisoned vector, and the factor is switched to the level-by-level form of the same plans for every
 * later application (MatSolve below), ILU(0) and ICC(0) alike. */
static HipTriFactors **tri_watch = NULL;
static int tri_watch_cap = 0;
static PetscInt tri_live = 0;   /* factors MatGetFactor made and HipTriFactorsDestroy has not released yet (HIPMI355XGetLiveFactors) */
/* the list grows with the number of live factors (multigrid levels, fieldsplit blocks, many KSPs); a factor that cannot be put on
 * it (out of memory) never runs the sync-free kernels unwatched: it takes the level launches */
void HipTriWatchAdd(HipTriFactors *f) {
  for (int i = 0; i < tri_watch_cap; i++) if (tri_watch[i] == f) return;
  for (int i = 0; i < tri_watch_cap; i++) if (!tri_watch[i]) { tri_watch[i] = f; return; }
  const int ncap = tri_watch_cap ? 2 * tri_watch_cap : 64;
  HipTriFactors **nw = (HipTriFactors **)realloc(tri_watch, sizeof(*nw) * (size_t)ncap);
  if (!nw) { f->syncfree.use_levels = 1; return; }
  memset(nw + tri_watch_cap, 0, sizeof(*nw) * (size_t)(ncap - tri_watch_cap));
  nw[tri_watch_cap] = f;
  tri_watch = nw; tri_watch_cap = ncap;
}
static void tri_watch_remove(HipTriFactors *f) { for (int i = 0; i < tri_watch_cap; i++) if (tri_watch[i] == f) tri_watch[i] = NULL; }
PetscErrorCode HipTriWatchCheck(void) {
  for (int i = 0; i < tri_watch_cap; i++) {
    HipTriFactors *f = tri_watch[i];
    int a = 0, b = 0;
    if (!f || !f->syncfree.tri_lo || f->syncfree.use_levels) continue;
    mi355x_trisolve_aborted(f->syncfree.tri_lo, &a); mi355x_trisolve_aborted(f->syncfree.tri_up, &b);
    if (a || b) {
      f->syncfree.use_levels = 1; f->aborted = 1;
      SETERRQ(PETSC_COMM_SELF, PETSC_ERR_LIB, "a sync-free triangular solve gave up waiting for a dependency: results computed since that MatSolve are invalid; "
                                              "later applications of this factor use one launch per dependency level");
    }
  }
  return 0;
}

/* ---------------------------------------------------------------- releasing a factor: one function per form (hipmi355ximpl.h) */
static void tri_free_host(HipTriFactors *f) {
  if (f->host.owns) { HipFree(f->host.bi); HipFree(f->host.bj); HipFree(f->host.bdiag); HipFree(f->host.ba); }
  memset(&f->host, 0, sizeof(f->host));
}
static void tri_free_lev(HipTriFactors *f) {
  HipFree(f->lev.rlevL); HipFree(f->lev.rlevU);
  memset(&f->lev, 0, sizeof(f->lev));
}
static void tri_free_launch(HipTriFactors *f) {
  if (f->launch.graph) mi355x_graph_destroy(f->launch.graph);
  if (f->launch.borrowed) f->launch.d_bi = f->launch.d_bj = f->launch.d_bdiag = f->launch.d_rowsL = NULL;   /* the context's: forgotten, not freed */
  void *dev[] = {f->launch.d_bi, f->launch.d_bj, f->launch.d_bdiag, f->launch.d_ba, f->launch.d_rowsL, f->launch.d_rowsU, f->launch.d_work};
  for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); i++) if (dev[i]) mi355x_free(dev[i]);
  HipFree(f->launch.levptrL); HipFree(f->launch.levptrU);
  memset(&f->launch, 0, sizeof(f->launch));
}
static void tri_free_syncfree(HipTriFactors *f) {
  if (f->syncfree.tri_lo) mi355x_trisolve_plan_destroy(f->syncfree.tri_lo);
  if (f->syncfree.tri_up) mi355x_trisolve_plan_destroy(f->syncfree.tri_up);
  memset(&f->syncfree, 0, sizeof(f->syncfree));
}
/* the device form of -pc_factor_hipmi355x_trisolve sweeps:<k> */
static void tri_free_sweeps(HipTriFactors *f) {
  void *dev[] = {f->sw.iL, f->sw.jL, f->sw.iU, f->sw.jU, f->sw.aL, f->sw.aU, f->sw.dinv, f->sw.work[0], f->sw.work[1]};
  for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); i++) if (dev[i]) mi355x_free(dev[i]);
  if (f->sw.planL) mi355x_spmv_plan_destroy(f->sw.planL);
  if (f->sw.planU) mi355x_spmv_plan_destroy(f->sw.planU);
  HipFree(f->sw.bi); HipFree(f->sw.bj); HipFree(f->sw.bdiag);
  memset(&f->sw, 0, sizeof(f->sw));
}
/* the device route's context of one pattern (-pc_factor_hipmi355x_numeric device) */
static void tri_free_dev(HipTriFactors *f) {
  if (f->dev.dfac) mi355x_ilu0_factor_destroy(f->dev.dfac);
  HipFree(f->dev.blk);
  memset(&f->dev, 0, sizeof(f->dev));
}
/* the transposed factor (MatSolveTranspose).  whole == 0: its values are those of a factorisation that is being forgotten -- the
 * value array itself stays, the captured graph names it and the next build refills it in place when the pattern is the same */
static void tri_free_transpose(HipTriFactors *f, int whole) {
  const PetscInt pb = f->tr.pattern_builds, vr = f->tr.value_refreshes;
  f->tr.fresh = 0;
  if (!whole) return;
  if (f->tr.graph) mi355x_graph_destroy(f->tr.graph);
  void *dev[] = {f->tr.d_ti, f->tr.d_tj, f->tr.d_si, f->tr.d_sj, f->tr.d_perm, f->tr.d_val, f->tr.d_rows1, f->tr.d_rows2, f->tr.d_work};
  for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); i++) if (dev[i]) mi355x_free(dev[i]);
  HipFree(f->tr.bi); HipFree(f->tr.bj); HipFree(f->tr.bdiag); HipFree(f->tr.perm); HipFree(f->tr.levptr1); HipFree(f->tr.levptr2);
  memset(&f->tr, 0, sizeof(f->tr));
  f->tr.pattern_builds = pb; f->tr.value_refreshes = vr;
}
/* forget one numeric factorisation (ILU(0) and ICC(0) alike); the symbolic choices, the block list and the watch slot stay, and so
 * do the sweep form's device arrays: the next factorisation may only have new values.  The one order that matters: the level-launch
 * form goes BEFORE the device route's context -- its captured graph names the context's arrays, and the pointers it borrowed from the
 * context are forgotten (tri_free_launch) while the context still owns them, never freed twice. */
void HipTriFactorsResetNumeric(HipTriFactors *f) {
  tri_free_transpose(f, 0);
  tri_free_launch(f); tri_free_dev(f);
  tri_free_host(f); tri_free_lev(f); tri_free_syncfree(f);
  f->sw.sweeps = 0; f->nshift = 0;
  f->factored_state = -1;
}
PetscErrorCode HipTriFactorsDestroy(HipTriFactors **pf) {
  HipTriFactors *f = *pf;
  if (!f) return 0;
  tri_watch_remove(f);
  HipTriFactorsResetNumeric(f);
  tri_free_sweeps(f);
  tri_free_transpose(f, 1);
  HipFree(f->blk);
  HipFree(f);
  tri_live--;
  *pf = NULL;
  return 0;
}
/* life-cycle tests: ILU / ICC factors of the AIJ type alive in this process, and how many of them sit on the watch list */
PetscErrorCode HIPMI355XGetLiveFactors(PetscInt *live, PetscInt *watched) {
  if (live) *live = tri_live;
  if (watched) { *watched = 0; for (int i = 0; i < tri_watch_cap; i++) if (tri_watch[i]) (*watched)++; }
  return 0;
}

/* the list "MatFactorSetIndependentBlocks_C" left when it covers the matrix, else the whole matrix as one block (kept in whole) */
PetscInt HipTriFactorsBlocks(const HipTriFactors *f, PetscInt n, PetscInt whole[2], const PetscInt **blk) {
  if (f->nblk > 0 && f->blk[f->nblk] == n) { *blk = f->blk; return f->nblk; }
  whole[0] = 0; whole[1] = n; *blk = whole;
  return 1;
}

/* block Jacobi solving all its ILU(0) / ICC(0) blocks as one block-diagonal system ("MatFactorSetIndependentBlocks_C", asked for
 * by the harness's PCILU / PCICC): every block is factored as the reference factors a matrix of its own (its own shift loop), so
 * the result is the blocks' factors side by side also when one block needs a shift */
static PetscErrorCode MatFactorSetIndependentBlocks_SeqAIJHIP(Mat F, PetscInt nblk, const PetscInt *starts) {
  HipTriFactors *f = HipTriGet(F);
  PetscErrorCode ierr;
  if (f->nblk == nblk && (!nblk || !memcmp(f->blk, starts, sizeof(PetscInt) * (size_t)(nblk + 1)))) return 0;
  HipFree(f->blk); f->blk = NULL; f->nblk = 0;
  if (nblk > 0) {
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nblk + 1), &f->blk);CHKERRQ(ierr);
    memcpy(f->blk, starts, sizeof(PetscInt) * (size_t)(nblk + 1));
    f->nblk = nblk;
  }
  f->factored_state = -1;
  return 0;
}

/* rows sorted by dependency level (stable: ascending row inside a level) */
static PetscErrorCode level_order(PetscInt n, const PetscInt *lev, PetscInt nlev, PetscInt **ptr_out, PetscInt **rows_out) {
  PetscErrorCode ierr;
  PetscInt *ptr, *rows, *next;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nlev + 1), &ptr);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &rows);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nlev + 1), &next);CHKERRQ(ierr);
  memset(ptr, 0, sizeof(PetscInt) * (size_t)(nlev + 1));
  for (PetscInt i = 0; i < n; i++) ptr[lev[i] + 1]++;
  for (PetscInt l = 0; l < nlev; l++) ptr[l + 1] += ptr[l];
  memcpy(next, ptr, sizeof(PetscInt) * (size_t)(nlev + 1));
  for (PetscInt i = 0; i < n; i++) rows[next[lev[i]]++] = i;
  HipFree(next);
  *ptr_out = ptr; *rows_out = rows;
  return 0;
}

static PetscErrorCode natural_ordering_only(Mat A, IS row, IS col, const MatFactorInfo *info, const char *what) {
  if (info->levels != 0.0 && strcmp(what, "ILU")) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "%s(%d): only zero fill is on the ported path", what, (int)info->levels);   /* ILU(k): ilu_symbolic_host below */
  if (info->levels < 0.0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Levels of fill negative %d", (int)info->levels);
#if defined(PETSCHIPMI355X_WITH_PETSC)
  { PetscErrorCode ierr; PetscBool id = PETSC_TRUE;
    if (row) { ierr = ISIdentity(row, &id);CHKERRQ(ierr); if (!id) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "%s on the device: natural ordering only (-pc_factor_mat_ordering_type natural)", what); }
    if (col) { ierr = ISIdentity(col, &id);CHKERRQ(ierr); if (!id) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "%s on the device: natural ordering only (-pc_factor_mat_ordering_type natural)", what); } }
#else
  if (row || col) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "%s: natural ordering only", what);
#endif
  return 0;
}

double HipWallSeconds(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

/* the host factorisation hands its work arrays to a thread that returns them to the system; at most one such thread: it is joined before the next one starts and by PetscHIPMI355XFinalize (never left running behind the library) */
static pthread_t release_th; static int release_running = 0;
void HipFactorJoinHelpers(void) { if (release_running) { pthread_join(release_th, NULL); release_running = 0; } }
/* dependency levels of the rows of L (a row may start once the rows its L part names are done) and of U (backwards), from the
 * factor's pattern in the reference's layout; each is a sequential recurrence, the two run side by side */
typedef struct { PetscInt n; const PetscInt *bi, *bj, *bdiag; PetscInt *lev, nlev; } RowLevArg;
static void *row_levels_L(void *a_) {
  RowLevArg *a = (RowLevArg *)a_; const PetscInt *bi = a->bi, *bj = a->bj; PetscInt *lev = a->lev, nlev = 0;
  for (PetscInt i = 0; i < a->n; i++) {
    PetscInt l = 0;
    for (PetscInt q = bi[i]; q < bi[i + 1]; q++) l = PetscMax(l, lev[bj[q]] + 1);
    lev[i] = l; nlev = PetscMax(nlev, l + 1);
  }
  a->nlev = nlev;
  return NULL;
}
static void *row_levels_U(void *a_) {
  RowLevArg *a = (RowLevArg *)a_; const PetscInt *bj = a->bj, *bdiag = a->bdiag; PetscInt *lev = a->lev, nlev = 0;
  for (PetscInt i = a->n - 1; i >= 0; i--) {
    PetscInt l = 0; const PetscInt s0 = bdiag[i + 1] + 1, nz = bdiag[i] - bdiag[i + 1] - 1;
    for (PetscInt q = 0; q < nz; q++) l = PetscMax(l, lev[bj[s0 + q]] + 1);
    lev[i] = l; nlev = PetscMax(nlev, l + 1);
  }
  a->nlev = nlev;
  return NULL;
}
static PetscErrorCode ilu0_row_levels(PetscInt n, const PetscInt *bi, const PetscInt *bj, const PetscInt *bdiag, PetscInt **levL, PetscInt *nlevL, PetscInt **levU, PetscInt *nlevU) {
  PetscErrorCode ierr;
  RowLevArg aL = {n, bi, bj, bdiag, NULL, 0}, aU = {n, bi, bj, bdiag, NULL, 0};
  pthread_t th; int side = 0;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &aL.lev);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &aU.lev);CHKERRQ(ierr);
  if (n >= 200000) side = !pthread_create(&th, NULL, row_levels_L, &aL);
  if (!side) row_levels_L(&aL);
  row_levels_U(&aU);
  if (side) pthread_join(th, NULL);
  *levL = aL.lev; *nlevL = aL.nlev; *levU = aU.lev; *nlevU = aU.nlev;
  return 0;
}

#if !defined(PETSCHIPMI355X_WITH_PETSC)
/* one pass of the numeric ILU(0) over the rows [r0, r1) of an independent block with a given diagonal shift, rows taken level by
 * level (dependency levels of L) and a level's rows dealt to the threads */
typedef struct {
  const PetscInt *ai, *aj; const PetscScalar *aa;
  const PetscInt *bi, *bj, *bdiag; PetscScalar *ba;
  PetscInt n, r0, r1, nlev, *levptr, *rows;
  PetscReal zeropivot, shift_amount;
  int nth;
  PetscScalar **rtmp;                 /* a dense work row per thread */
  volatile PetscInt fail_row, fail_level; volatile PetscReal fail_value;
  volatile int go;                    /* the gate the threads start at: 1 go, -1 leave (not all of them could be created) */
  int oversubscribed;                 /* more threads than cores of this rank */
  volatile int bar_count, bar_sense;  /* sense-reversing barrier: the levels are short (tens of microseconds), a futex sleep per level costs more */
  pthread_mutex_t mtx;
} IluPass;
typedef struct { IluPass *p; int tid; } IluArg;

/* row i of MatLUFactorNumeric_SeqAIJ (aijfact.c:505-570): dense work row, multipliers in column order, the pivot stored inverted;
 * returns 1 when the pivot fails MatPivotCheck_nz (matimpl.h:512-528) */
static int ilu0_factor_row(const IluPass *p, PetscScalar *rtmp, PetscInt i, PetscReal *badval) {
  const PetscInt *ai = p->ai, *aj = p->aj, *bi = p->bi, *bj = p->bj, *bdiag = p->bdiag; const PetscScalar *aa = p->aa; PetscScalar *ba = p->ba;
  PetscInt nzl = bi[i + 1] - bi[i], nzu = bdiag[i] - bdiag[i + 1];
  PetscReal rs = 0.0;
  for (PetscInt j = 0; j < nzl; j++) rtmp[bj[bi[i] + j]] = 0.0;
  for (PetscInt j = 0; j < nzu; j++) rtmp[bj[bdiag[i + 1] + 1 + j]] = 0.0;
  for (PetscInt q = ai[i]; q < ai[i + 1]; q++) rtmp[aj[q]] = aa[q];
  rtmp[i] += p->shift_amount;
  for (PetscInt kk = 0; kk < nzl; kk++) {
    const PetscInt row = bj[bi[i] + kk];
    PetscScalar *pc_ = rtmp + row;
    if (*pc_ != 0.0) {
      const PetscScalar multiplier = *pc_ * ba[bdiag[row]];
      *pc_ = multiplier;
      const PetscInt *pj = bj + bdiag[row + 1] + 1;
      const PetscScalar *pv = ba + bdiag[row + 1] + 1;
      const PetscInt nz = bdiag[row] - bdiag[row + 1] - 1;
      for (PetscInt j = 0; j < nz; j++) rtmp[pj[j]] -= multiplier * pv[j];
    }
  }
  for (PetscInt j = 0; j < nzl; j++) { ba[bi[i] + j] = rtmp[bj[bi[i] + j]]; rs += PetscAbsScalar(ba[bi[i] + j]); }
  for (PetscInt j = 0; j < nzu - 1; j++) { ba[bdiag[i + 1] + 1 + j] = rtmp[bj[bdiag[i + 1] + 1 + j]]; rs += PetscAbsScalar(ba[bdiag[i + 1] + 1 + j]); }
  if (PetscAbsScalar(rtmp[i]) <= p->zeropivot * rs) { *badval = PetscAbsScalar(rtmp[i]); return 1; }
  ba[bdiag[i]] = 1.0 / rtmp[i];
  return 0;
}
static void ilu0_barrier(IluPass *p, int *sense) {
  *sense = !*sense;
  if (__sync_add_and_fetch(&p->bar_count, 1) == p->nth) { p->bar_count = 0; __sync_synchronize(); p->bar_sense = *sense; }
  else {   /* more threads than this rank's cores (an explicit -mat_factor_hipmi355x_threads): give the core away at once instead of spinning */
    const int limit = p->oversubscribed ? 1 : 4000;
    int spins = 0; while (p->bar_sense != *sense) { if (++spins > limit) { sched_yield(); spins = 0; } } }
  __sync_synchronize();
}
static void *ilu0_worker(void *arg_) {
  IluArg *arg = (IluArg *)arg_;
  IluPass *p = arg->p;
  PetscScalar *rtmp = p->rtmp[arg->tid];
  int sense = 0;
  if (p->nth > 1 && arg->tid > 0) { while (p->go == 0) sched_yield(); if (p->go < 0) return NULL; }
  for (PetscInt l = 0; l < p->nlev; l++) {
    const PetscInt a = p->levptr[l], b = p->levptr[l + 1], cnt = b - a;
    const PetscInt lo = a + (PetscInt)((long)cnt * arg->tid / p->nth), hi = a + (PetscInt)((long)cnt * (arg->tid + 1) / p->nth);
    for (PetscInt t = lo; t < hi; t++) {
      const PetscInt i = p->rows[t];
      PetscReal bad;
      if (i < p->r0 || i >= p->r1) continue;
      if (ilu0_factor_row(p, rtmp, i, &bad)) {
        pthread_mutex_lock(&p->mtx);
        if (p->fail_row < 0 || i < p->fail_row) { p->fail_row = i; p->fail_value = bad; }
        if (p->fail_level < 0 || l < p->fail_level) p->fail_level = l;
        pthread_mutex_unlock(&p->mtx);
        break;
      }
    }
    if (p->nth > 1) ilu0_barrier(p, &sense);
    /* one barrier per level: a thread that is already in level l + 1 may record a failure there before a slower thread has looked
     * at level l's outcome; that thread goes on to level l + 1 like everybody else and they all leave after ITS barrier */
    if (p->fail_level >= 0 && p->fail_level <= l) break;
  }
  return NULL;
}
static PetscErrorCode ilu0_run_pass(IluPass *p) {
  IluArg args[64]; pthread_t th[64];
  for (int t = 0; t < p->nth; t++) { args[t].p = p; args[t].tid = t; }
  pthread_mutex_init(&p->mtx, NULL);
  if (p->nth == 1) { ilu0_worker(&args[0]); pthread_mutex_destroy(&p->mtx); return 0; }
  p->bar_count = 0; p->bar_sense = 0; p->go = 0;
  int started = 0;
  for (int t = 1; t < p->nth; t++) { if (pthread_create(&th[t], NULL, ilu0_worker, &args[t])) break; started = t; }
  if (started != p->nth - 1) {            /* could not start them all: the ones that did are still at the gate and leave from there */
    p->go = -1;
    for (int t = 1; t <= started; t++) pthread_join(th[t], NULL);
    pthread_mutex_destroy(&p->mtx);
    return PETSC_ERR_LIB;
  }
  p->go = 1;
  ilu0_worker(&args[0]);
  for (int t = 1; t < p->nth; t++) pthread_join(th[t], NULL);
  pthread_mutex_destroy(&p->mtx);
  return 0;
}
#endif

/* every block of an independent-blocks factorisation is a matrix of its own: no row may name a column outside its block */
static PetscErrorCode ilu0_check_blocks(Mat A, const PetscInt *ai, const PetscInt *aj, PetscInt nblk, const PetscInt *blk) {
  for (PetscInt bb = 0; bb < nblk; bb++)
    for (PetscInt i = blk[bb]; i < blk[bb + 1]; i++)
      if (ai[i] < ai[i + 1] && (aj[ai[i]] < blk[bb] || aj[ai[i + 1] - 1] >= blk[bb + 1])) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "row %d couples to a column outside its independent block", i);
  return 0;
}
/* MAT_SHIFT_NONZERO, PCILU's default on a SeqAIJ matrix (ilu.c:387): a pivot that fails MatPivotCheck_nz (matimpl.h:512-528) restarts the
 * factorisation with the diagonal shifted by shiftamount, then by twice that, ... at most 80 times (aijfact.c:507-592).  The next
 * shift after a failed pass; non-zero: give up */
static PetscErrorCode ilu0_next_shift(const MatFactorInfo *info, PetscReal *shift, PetscInt *nshift) {
  if (info->shifttype != (PetscReal)MAT_SHIFT_NONZERO) return PETSC_ERR_ARG_WRONG;
  *shift = *nshift ? *shift * 2.0 : info->shiftamount;
  return ++*nshift > 80 ? PETSC_ERR_ARG_WRONG : 0;
}
static PetscErrorCode ilu0_zero_pivot(Mat A, const MatFactorInfo *info, PetscInt row, PetscReal value) {
  SETERRQ(HipObjComm(A), 71 /* PETSC_ERR_MAT_LU_ZRPVT */, "Zero pivot row %d value %g%s", row, value, info->shifttype == (PetscReal)MAT_SHIFT_NONZERO ? ": still there after 80 diagonal shifts" : "");
}

#if !defined(PETSCHIPMI355X_WITH_PETSC)
static void *ilu0_release_thread(void *a_) { void **a = (void **)a_; for (int i = 0; a[i]; i++) free(a[i]); free(a); return NULL; }
typedef struct { const PetscInt *ai, *aj; PetscInt *adiag, *bi, *bj, *bdiag; volatile PetscInt missing; } IluSym;
static void ilu0_sym_diag(void *c_, PetscInt lo, PetscInt hi) {
  IluSym *c = (IluSym *)c_;
  for (PetscInt i = lo; i < hi; i++) {
    PetscInt d = -1;
    for (PetscInt q = c->ai[i]; q < c->ai[i + 1]; q++) if (c->aj[q] == i) { d = q; break; }
    c->adiag[i] = d;
    if (d < 0) c->missing = i;             /* (the caller looks for the first such row) */
  }
}
/* the pattern of A, L part forward, U part from the last row backwards with the diagonal at each row's end (aijfact.c:1660-1685) */
static void ilu0_sym_pattern(void *c_, PetscInt lo, PetscInt hi) {
  IluSym *c = (IluSym *)c_;
  for (PetscInt i = lo; i < hi; i++) {
    const PetscInt nzl = c->adiag[i] - c->ai[i], nzu = c->ai[i + 1] - c->adiag[i] - 1;
    PetscInt *l = c->bj + c->bi[i], *u = c->bj + c->bdiag[i + 1] + 1;
    for (PetscInt j = 0; j < nzl; j++) l[j] = c->aj[c->ai[i] + j];
    for (PetscInt j = 0; j < nzu; j++) u[j] = c->aj[c->adiag[i] + 1 + j];
    u[nzu] = i;
  }
}
/* MatILUFactorSymbolic_SeqAIJ_ilu0 restated for the harness: f->host.bi / bj / bdiag (ours) from the pattern of A.  adiag_out: for a caller
 * with a use for the diagonal positions in A (NULL: freed here); diag_phase: the set-up clock's label for the first half (NULL: none) */
static PetscErrorCode ilu0_symbolic_host(Mat A, PetscInt n, const PetscInt *ai, const PetscInt *aj, HipTriFactors *f, PetscInt **adiag_out, const char *diag_phase, double *clock) {
  PetscErrorCode ierr;
  PetscInt *adiag, *bi, *bdiag;
  f->host.owns = PETSC_TRUE;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &adiag);CHKERRQ(ierr);
  IluSym sy = {ai, aj, adiag, NULL, NULL, NULL, -1};
  HipParallelRanges(n, ilu0_sym_diag, &sy);
  if (sy.missing >= 0) {
    PetscInt first = 0;
    while (first < n && adiag[first] >= 0) first++;
    HipFree(adiag);
    SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry %d", first);
  }
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(n + 1), &f->host.bi);
  if (!ierr) ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(ai[n] + 1), &f->host.bj);
  if (!ierr) ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(n + 1), &f->host.bdiag);
  if (ierr) { HipFree(adiag); CHKERRQ(ierr); }
  if (diag_phase) HipSetupTick(*clock, diag_phase);
  /* the two pointer arrays are running sums (one light sequential pass each); the column copies are per row, on host threads */
  bi = f->host.bi; bdiag = f->host.bdiag;
  bi[0] = 0;
  for (PetscInt i = 0; i < n; i++) bi[i + 1] = bi[i] + (adiag[i] - ai[i]);
  bdiag[n] = bi[n] - 1;
  for (PetscInt i = n - 1; i >= 0; i--) bdiag[i] = bdiag[i + 1] + (ai[i + 1] - adiag[i] - 1) + 1;
  sy.bi = bi; sy.bj = f->host.bj; sy.bdiag = bdiag;
  HipParallelRanges(n, ilu0_sym_pattern, &sy);
  if (adiag_out) *adiag_out = adiag; else HipFree(adiag);
  return 0;
}
/* MatILUFactorSymbolic_SeqAIJ (levels of fill, natural ordering) for the harness: f->host.bi / bj / bdiag (ours) in the same layout,
 * from the kernel library's host routine (mi355x_iluk_symbolic_host: one thread, the rows depend on each other in sequence) */
static PetscErrorCode iluk_symbolic_host(Mat A, PetscInt n, const PetscInt *ai, const PetscInt *aj, PetscInt levels, HipTriFactors *f) {
  PetscErrorCode ierr;
  int bad = -1, rc;
  f->host.owns = PETSC_TRUE;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(n + 1), &f->host.bi);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(n + 1), &f->host.bdiag);CHKERRQ(ierr);
  rc = mi355x_iluk_symbolic_host(n, ai, aj, levels, f->host.bi, f->host.bdiag, NULL, NULL, &bad);
  if (!rc) {
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(f->host.bdiag[0] + 2), &f->host.bj);CHKERRQ(ierr);
    f->host.bj[f->host.bdiag[0] + 1] = 0;                      /* (the slot past the last column: compared with the sweep form's copy, never read as a column) */
    rc = mi355x_iluk_symbolic_host(n, ai, aj, levels, f->host.bi, f->host.bdiag, f->host.bj, NULL, &bad);
  }
  if (rc == 1 && bad >= 0 && bad < n) {                        /* hipErrorInvalidValue: the row at fault */
    PetscBool diag = PETSC_FALSE;
    for (PetscInt q = ai[bad]; q < ai[bad + 1]; q++) if (aj[q] == bad) diag = PETSC_TRUE;
    if (!diag) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry %d", bad);
    SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "ILU(%d): the columns of row %d are not sorted inside the matrix", levels, bad);
  }
  CHKHIP(rc);
  return 0;
}
/* the factor's pattern for the level of fill asked for.  Zero fill is ilu0_symbolic_host as it always was */
static PetscErrorCode ilu_symbolic_host(Mat A, PetscInt n, const PetscInt *ai, const PetscInt *aj, PetscInt levels, HipTriFactors *f, PetscInt **adiag_out, const char *diag_phase, double *clock) {
  PetscErrorCode ierr;
  f->levels = levels; f->nzA = ai[n];
  if (!levels) {
    ierr = ilu0_symbolic_host(A, n, ai, aj, f, adiag_out, diag_phase, clock);CHKERRQ(ierr);
    f->nz = ai[n];
  } else {
    if (adiag_out) *adiag_out = NULL;
    ierr = iluk_symbolic_host(A, n, ai, aj, levels, f);CHKERRQ(ierr);
    f->nz = f->host.bdiag[0] + 1;
  }
  return 0;
}
/* MatILUFactorSymbolic_SeqAIJ_ilu0 + MatLUFactorNumeric_SeqAIJ restated for the harness (inside a PETSc tree the parent's
 * routines run instead): the pattern (ilu0_symbolic_host); row by row with a dense work row, pivots stored inverted
 * (aijfact.c:505-570); MatPivotCheck_nz's restarts (ilu0_next_shift) */
static PetscErrorCode ilu0_factor_host(Mat F, Mat A, const MatFactorInfo *info) {
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  PetscInt n, *adiag, whole[2]; const PetscInt *ai, *aj, *blk; const PetscScalar *aa;
  double tick0 = HipWallSeconds();
  ierr = MatSeqAIJGetArrays(A, &n, &ai, &aj, &aa);CHKERRQ(ierr);
  f->n = n;
  ierr = ilu_symbolic_host(A, n, ai, aj, (PetscInt)info->levels, f, &adiag, "factor: diagonal positions", &tick0);CHKERRQ(ierr);   /* f->nz: the factor's entries */
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)(f->nz + 1), &f->host.ba);
  if (ierr) { HipFree(adiag); CHKERRQ(ierr); }
  f->host.ba[f->nz] = 0.0;                 /* (every other entry is written by the numeric pass) */
  HipSetupTick(tick0, "factor: pattern of L and U");
  f->nshift = 0;
  const PetscInt nblk = HipTriFactorsBlocks(f, n, whole, &blk);
  ierr = ilu0_check_blocks(A, ai, aj, nblk, blk);
  if (ierr) { HipFree(adiag); return ierr; }
  /* Rows of one dependency level of L do not read each other: a level's rows are factored by several host threads, one barrier per
   * level.  Every row's own arithmetic is the sequential loop's (ilu0_factor_row), so the factor carries the same bits whatever
   * the thread count; a pivot that fails MatPivotCheck_nz anywhere ends the pass for everybody and the block restarts shifted. */
  IluPass ps;
  memset(&ps, 0, sizeof(ps));
  ps.ai = ai; ps.aj = aj; ps.aa = aa; ps.bi = f->host.bi; ps.bj = f->host.bj; ps.bdiag = f->host.bdiag; ps.ba = f->host.ba; ps.zeropivot = info->zeropivot; ps.n = n;
  { PetscInt nth = 1; PetscBool set;
    if (n >= 200000) nth = (PetscInt)HipHostThreads(16);
    ierr = PetscOptionsGetInt(NULL, "-mat_factor_hipmi355x_threads", &nth, &set);CHKERRQ(ierr);
    if (nth < 1) nth = 1;
    if (nth > 64) nth = 64;
    ps.nth = (int)nth; ps.oversubscribed = nth > (PetscInt)HipHostThreads(64); }
  /* levels of L (the threaded passes below take a level's rows together) and of U, kept for the solves' analysis */
  tri_free_lev(f);
  ierr = ilu0_row_levels(n, ps.bi, ps.bj, ps.bdiag, &f->lev.rlevL, &f->lev.nlevL, &f->lev.rlevU, &f->lev.nlevU);
  if (!ierr) { ps.nlev = f->lev.nlevL; ierr = level_order(n, f->lev.rlevL, f->lev.nlevL, &ps.levptr, &ps.rows); }
  if (ierr) { HipFree(adiag); CHKERRQ(ierr); }
  HipSetupTick(tick0, "factor: levels of L and U");
  ierr = PetscMalloc(sizeof(PetscScalar *) * (size_t)ps.nth, &ps.rtmp);CHKERRQ(ierr);
  for (int t = 0; t < ps.nth; t++) { ps.rtmp[t] = (PetscScalar *)calloc((size_t)n + 1, sizeof(PetscScalar)); if (!ps.rtmp[t]) SETERRQ(HipObjComm(A), PETSC_ERR_MEM, "out of memory"); }
  for (PetscInt bb = 0; bb < nblk && !ierr; bb++) {   /* every block is a matrix of its own: its own sequence of shifts */
    PetscInt nshift = 0;
    ps.r0 = blk[bb]; ps.r1 = blk[bb + 1]; ps.shift_amount = 0.0;
    for (;;) {
      ps.fail_row = -1; ps.fail_level = -1;
      ierr = ilu0_run_pass(&ps);
      if (ierr || ps.fail_row < 0) break;
      ierr = ilu0_next_shift(info, &ps.shift_amount, &nshift);
      if (ierr) break;
    }
    if (!ierr) f->nshift = PetscMax(f->nshift, nshift);
  }
  HipSetupTick(tick0, "factor: numeric passes");
  /* returning 16 dense work rows (2 GB of touched pages at 16.7 M rows) to the system takes 0.12 s: off the caller's path */
  { void **junk = (void **)malloc(sizeof(void *) * (size_t)(ps.nth + 4)); int k = 0;
    if (junk) {
      for (int t = 0; t < ps.nth; t++) junk[k++] = ps.rtmp[t];
      junk[k++] = ps.levptr; junk[k++] = ps.rows; junk[k++] = adiag; junk[k] = NULL;
      HipFactorJoinHelpers();
      if (n < 200000 || pthread_create(&release_th, NULL, ilu0_release_thread, junk)) ilu0_release_thread(junk);
      else release_running = 1;
    } else { for (int t = 0; t < ps.nth; t++) free(ps.rtmp[t]); HipFree(ps.levptr); HipFree(ps.rows); HipFree(adiag); }
    HipFree(ps.rtmp); }
  HipSetupTick(tick0, "factor: work arrays released");
  if (ierr) return ilu0_zero_pivot(A, info, ps.fail_row, ps.fail_value);
  return 0;
}
#endif

typedef struct { const PetscInt *bi, *bdiag; const PetscScalar *ba; PetscInt *rlL, *rpU, *rlU; PetscScalar *dinv; } RowArr;
static void ilu0_row_arrays(void *c_, PetscInt lo, PetscInt hi) {
  RowArr *c = (RowArr *)c_;
  for (PetscInt i = lo; i < hi; i++) {
    c->rlL[i] = c->bi[i + 1] - c->bi[i];
    c->rpU[i] = c->bdiag[i + 1] + 1; c->rlU[i] = c->bdiag[i] - c->bdiag[i + 1] - 1; c->dinv[i] = c->ba[c->bdiag[i]];
  }
}
/* -pc_factor_hipmi355x_trisolve sweeps:<k>.  With L = I + Ls and U = D + Us (dinv = D^-1 as the factor stores it),
 *     lower:  y^0 = b             y^j = b - Ls y^(j-1)               j = 1..k
 *     upper:  x^0 = dinv .* y^k   x^j = dinv .* (y^k - Us x^(j-1))   j = 1..k
 * every step a product with a strict triangle that reads the previous iterate and writes the next one (two buffers, never in
 * place: the same bits whatever the scheduling).  A row of dependency level l is final from sweep l on, so k >= levels - 1 IS the
 * solve -- bit for bit where a row is summed by one lane, because s = b_i; s = s + (-l_ij) y_j in column order is the loop of
 * MatSolve_SeqAIJ_NaturalOrdering.  Fewer sweeps: an approximate application, 2k SpMV-shaped passes instead of a chain of levels.
 * Here: the negated strict triangles as CSR (the upper one taken out of the reference's backwards layout), their row-block
 * plans, dinv and the two work vectors.  A factorisation with the pattern of the last one sends the values only. */
typedef struct { const PetscInt *bi, *bj, *bdiag, *iU; const PetscScalar *ba; PetscInt *jU; PetscScalar *aL, *aU, *dinv; } SweepArr;
static void ilu0_sweeps_rows(void *c_, PetscInt lo, PetscInt hi) {   /* the columns of the upper triangle's CSR (jU set) or the host factor's values for both triangles (aL set) */
  SweepArr *c = (SweepArr *)c_;
  for (PetscInt i = lo; i < hi; i++) {
    const PetscInt u0 = c->bdiag[i + 1] + 1, nu = c->iU[i + 1] - c->iU[i];
    if (c->jU) memcpy(c->jU + c->iU[i], c->bj + u0, sizeof(PetscInt) * (size_t)nu);
    if (!c->aL) continue;
    for (PetscInt q = c->bi[i]; q < c->bi[i + 1]; q++) c->aL[q] = -c->ba[q];
    for (PetscInt q = 0; q < nu; q++) c->aU[c->iU[i] + q] = -c->ba[u0 + q];
    c->dinv[i] = c->ba[c->bdiag[i]];
  }
}
/* the pattern side, once per pattern: index arrays and plans of the two triangles (iU: the upper one's row pointer, host), the
 * device arrays the values go to, and what the form was built for */
static PetscErrorCode ilu0_sweeps_pattern(HipTriFactors *f, PetscDeviceCtx *dc, const PetscInt *iU, int from_device) {
  PetscErrorCode ierr = 0;
  const PetscInt n = f->n, nz = f->nz, *bi = f->host.bi, *bj = f->host.bj, *bdiag = f->host.bdiag;
  const PetscInt nzL = bi[n], nzU = nz - nzL - n;
  const size_t ni = sizeof(PetscInt) * (size_t)(n + 1), nj = sizeof(PetscInt) * (size_t)(nz + 1), nv = sizeof(PetscScalar) * (size_t)PetscMax(n, 1);
  /* (value and index arrays carry the 16 bytes of slack past their end that the row-block kernels' paired loads ask for) */
  struct { void *p; size_t bytes; } dev[] = {{&f->sw.iL, ni}, {&f->sw.iU, ni}, {&f->sw.jL, sizeof(PetscInt) * (size_t)nzL + 16}, {&f->sw.jU, sizeof(PetscInt) * (size_t)nzU + 16},
    {&f->sw.aL, sizeof(PetscScalar) * (size_t)nzL + 16}, {&f->sw.aU, sizeof(PetscScalar) * (size_t)nzU + 16}, {&f->sw.dinv, nv}, {&f->sw.work[0], nv}, {&f->sw.work[1], nv}};
  PetscInt *jU; int rc = 0;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nzU, 1), &jU);CHKERRQ(ierr);
  { SweepArr sa = {bi, bj, bdiag, iU, NULL, jU, NULL, NULL, NULL};
    HipParallelRanges(n, ilu0_sweeps_rows, &sa); }
  for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]) && !rc; i++) rc = mi355x_malloc((void **)dev[i].p, dev[i].bytes);
  if (!rc) rc = mi355x_memcpy_h2d(dc->h, f->sw.iL, bi, ni);
  if (!rc) rc = mi355x_memcpy_h2d(dc->h, f->sw.iU, iU, ni);
  if (!rc && nzL) rc = mi355x_memcpy_h2d(dc->h, f->sw.jL, bj, sizeof(PetscInt) * (size_t)nzL);
  if (!rc && nzU) rc = mi355x_memcpy_h2d(dc->h, f->sw.jU, jU, sizeof(PetscInt) * (size_t)nzU);
  if (!rc) rc = mi355x_spmv_plan_create(dc->h, n, bi, NULL, &f->sw.planL);
  if (!rc) rc = mi355x_spmv_plan_create(dc->h, n, iU, NULL, &f->sw.planU);
  if (!rc) rc = mi355x_handle_synchronize(dc->h);      /* jU goes away below */
  HipFree(jU);
  CHKHIP(rc);
  f->sw.n = n; f->sw.nz = nz; f->sw.from_device = from_device;
  if (!from_device) {   /* the host route recognises its pattern by comparing */
    ierr = PetscMalloc(ni, &f->sw.bi); if (!ierr) ierr = PetscMalloc(ni, &f->sw.bdiag); if (!ierr) ierr = PetscMalloc(nj, &f->sw.bj);CHKERRQ(ierr);
    memcpy(f->sw.bi, bi, ni); memcpy(f->sw.bdiag, bdiag, ni); memcpy(f->sw.bj, bj, nj);
  }
  return 0;
}
/* the values of a factor that is on the host: negated, copied, with the inverted pivots */
static PetscErrorCode ilu0_sweeps_values_host(HipTriFactors *f, PetscDeviceCtx *dc, const PetscInt *iU) {
  PetscErrorCode ierr;
  const PetscInt n = f->n, nzL = f->host.bi[n], nzU = f->nz - nzL - n;
  PetscScalar *aL; int rc = 0;
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)(nzL + nzU + n + 1), &aL);CHKERRQ(ierr);   /* one array for the three */
  PetscScalar *aU = aL + nzL, *dinv = aU + nzU;
  { SweepArr sa = {f->host.bi, f->host.bj, f->host.bdiag, iU, f->host.ba, NULL, aL, aU, dinv};
    HipParallelRanges(n, ilu0_sweeps_rows, &sa);
    if (nzL) rc = mi355x_memcpy_h2d(dc->h, f->sw.aL, aL, sizeof(PetscScalar) * (size_t)nzL);
    if (!rc && nzU) rc = mi355x_memcpy_h2d(dc->h, f->sw.aU, aU, sizeof(PetscScalar) * (size_t)nzU);
    if (!rc && n) rc = mi355x_memcpy_h2d(dc->h, f->sw.dinv, dinv, sizeof(PetscScalar) * (size_t)n);
    if (!rc) rc = mi355x_handle_synchronize(dc->h);      /* the host arrays go away below */
  }
  HipFree(aL);
  CHKHIP(rc);
  return 0;
}
/* the sweep form of the factor just computed: the one an earlier factorisation of this route and this pattern left (hipmi355ximpl.h on
 * how each route tells), or a new one; then the values, from the host factor or by two small kernels from launch.d_ba */
static PetscErrorCode ilu0_sweeps_setup(HipTriFactors *f, PetscDeviceCtx *dc, int from_device) {
  PetscErrorCode ierr = 0;
  const PetscInt n = f->n, nz = f->nz, *bi = f->host.bi, *bj = f->host.bj, *bdiag = f->host.bdiag;
  const size_t ni = sizeof(PetscInt) * (size_t)(n + 1), nj = sizeof(PetscInt) * (size_t)(nz + 1);
  PetscInt *iU = NULL; int rc = 0;
  if (f->sw.planL && (f->sw.from_device != from_device || f->sw.n != n || f->sw.nz != nz ||
                      (!from_device && (memcmp(f->sw.bi, bi, ni) || memcmp(f->sw.bdiag, bdiag, ni) || memcmp(f->sw.bj, bj, nj))))) tri_free_sweeps(f);
  const int fresh = !f->sw.planL;
  if (fresh || !from_device) {   /* the upper triangle's row pointer, out of the reference's backwards layout */
    ierr = PetscMalloc(ni, &iU);CHKERRQ(ierr);
    iU[0] = 0;
    for (PetscInt i = 0; i < n; i++) iU[i + 1] = iU[i] + (bdiag[i] - bdiag[i + 1] - 1);
  }
  if (fresh) ierr = ilu0_sweeps_pattern(f, dc, iU, from_device);
  if (!ierr && !from_device) ierr = ilu0_sweeps_values_host(f, dc, iU);
  if (!ierr && from_device) rc = mi355x_ilu0_factor_to_sweeps(dc->h, f->dev.dfac, f->sw.iU, f->launch.d_ba, f->sw.aL, f->sw.aU, f->sw.dinv);
  HipFree(iU);
  if (ierr || rc) tri_free_sweeps(f);
  CHKERRQ(ierr);
  CHKHIP(rc);
  return 0;
}

/* x = (approximately) U^-1 L^-1 b: 2k products and one pointwise multiply on the compute stream, no host wait.  b is read by the
 * lower sweeps only and x is first written after them, so b and x may be the same vector; the last upper step lands in x. */
static PetscErrorCode ilu0_sweeps_apply(HipTriFactors *f, Vec b, Vec x) {
  PetscErrorCode ierr;
  const PetscScalar *db; PetscScalar *dx; PetscDeviceCtx *dc;
  const PetscInt k = f->sw.sweeps;
  int rc = 0;
  if (!f->n) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = VecHIPGetRead(b, &db);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(x, &dx);CHKERRQ(ierr);
  const PetscScalar *prev = db;
  for (PetscInt j = 0; j < k && !rc; j++) {
    PetscScalar *out = f->sw.work[j & 1];
    rc = mi355x_spmv_csr_add(dc->h, f->sw.planL, f->sw.iL, f->sw.jL, f->sw.aL, prev, db, out);
    prev = out;
  }
  const PetscScalar *yk = prev;
  PetscScalar *spare = f->sw.work[k & 1], *cur = (k & 1) ? spare : dx;   /* x^0 where k steps of alternation end in dx */
  if (!rc) rc = mi355x_vec_pointwise_mult(dc->h, (size_t)f->n, f->sw.dinv, yk, cur);
  for (PetscInt j = 0; j < k && !rc; j++) {
    PetscScalar *out = (cur == dx) ? spare : dx;
    rc = mi355x_spmv_csr_add_scaled(dc->h, f->sw.planU, f->sw.iU, f->sw.jU, f->sw.aU, cur, yk, f->sw.dinv, out);
    cur = out;
  }
  ierr = VecHIPRestoreWrite(x);CHKERRQ(ierr);
  HipStateIncrease(x);
  CHKHIP(rc);
  ierr = PetscLogFlops((PetscLogDouble)k * (2.0 * f->nz - f->n));CHKERRQ(ierr);
  return 0;
}

/* the device factor's values on the host (the sync-free plans' creators read them there; inside PETSc the parent's b->a) */
static PetscErrorCode ilu0_fetch_host_ba(HipTriFactors *f, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  if (!f->host.ba) { ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)(f->nz + 1), &f->host.ba);CHKERRQ(ierr); }
  CHKHIP(mi355x_memcpy_d2h(dc->h, f->host.ba, f->launch.d_ba, sizeof(PetscScalar) * (size_t)(f->nz + 1)));
  CHKHIP(mi355x_handle_synchronize(dc->h));
  return 0;
}

/* -pc_factor_hipmi355x_trisolve <syncfree|level|sweeps:<k>>: how MatSolve applies the factor.  sweeps: k >= 1 (there is no default
 * count), 0 for the exact solves; syncfree: the sync-free solves are wanted (set: by the user, not by default) */
static PetscErrorCode ilu0_trisolve_mode(Mat F, PetscInt *sweeps, int *syncfree, PetscBool *set) {
  PetscErrorCode ierr;
  char mode[32] = "syncfree";
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_trisolve", mode, sizeof(mode), set);CHKERRQ(ierr);
  *sweeps = 0; *syncfree = !strcmp(mode, "syncfree");
  if (!strncmp(mode, "sweeps", 6)) {
    char *end = mode + 7; long k = 0;
    if (mode[6] == ':' && mode[7] >= '0' && mode[7] <= '9') k = strtol(mode + 7, &end, 10);
    if (k < 1 || k > 1000000 || *end) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_WRONG, "-pc_factor_hipmi355x_trisolve sweeps:<k> needs an integer k >= 1, got %s", mode);
    *sweeps = (PetscInt)k;
  } else if (!*syncfree && strcmp(mode, "level")) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_WRONG, "-pc_factor_hipmi355x_trisolve <syncfree|level|sweeps:<k>>, got %s", mode);
  return 0;
}

/* The factor of a matrix with inodes: the reference solves it node by node (MatSolve_SeqAIJ_Inode, inode.c:2327-2760;
 * MatLUFactorNumeric_SeqAIJ_Inode installs it), and so does the device: one lane per NODE, dependency levels over nodes
 * (a node's rows were consecutive levels of the row-granular analysis), the shared column list walked once per node, two
 * columns at a time as the reference routine does.  -pc_factor_hipmi355x_trisolve_order column: in column order -- the
 * reference routine's bits; level (the default for such factors, as for the row-granular plans): oldest dependency
 * first -- agreement to rounding, 1.6x faster on the FEM stand-in (profiles/r03_ilu_fem_nodes.log).
 * On request first with whole dependency nodes as columns (a fixed number of dofs per node: one gather per dependency node;
 * measured no faster, so not the default), then the general node plans.  *made: 0 when the factor is of neither shape (the
 * caller goes on row by row). */
static PetscErrorCode ilu0_node_plans(Mat F, HipTriFactors *f, PetscDeviceCtx *dc, PetscInt nodes, const PetscInt *nsizes, int by_level, const RowArr *ra, double ta0, int *made) {
  PetscErrorCode ierr;
  const PetscInt n = f->n, *bi = f->host.bi, *bj = f->host.bj;
  PetscInt *nstart, nlL = 0, nlU = 0, bc = 0; PetscBool bset;
  *made = 0;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(3 * nodes + 1 + n), &nstart);CHKERRQ(ierr);   /* one work array: node starts, node of a row, node levels */
  PetscInt *nodeof = nstart + nodes + 1, *nlevL = nodeof + n, *nlevU = nlevL + nodes;
  nstart[0] = 0;
  for (PetscInt u = 0; u < nodes; u++) { nstart[u + 1] = nstart[u] + nsizes[u]; for (PetscInt r = nstart[u]; r < nstart[u + 1] && r < n; r++) nodeof[r] = u; }
  if (nstart[nodes] == n) {
    for (PetscInt u = 0; u < nodes; u++) {                     /* a node may start once the nodes its FIRST row references are done */
      PetscInt l = 0; const PetscInt r0 = nstart[u];
      for (PetscInt q = bi[r0]; q < bi[r0 + 1]; q++) l = PetscMax(l, nlevL[nodeof[bj[q]]] + 1);
      nlevL[u] = l; nlL = PetscMax(nlL, l + 1);
    }
    for (PetscInt u = nodes - 1; u >= 0; u--) {                /* upper: the columns of the node's LAST row */
      PetscInt l = 0; const PetscInt rL = nstart[u + 1] - 1;
      for (PetscInt q = 0; q < ra->rlU[rL]; q++) l = PetscMax(l, nlevU[nodeof[bj[ra->rpU[rL] + q]]] + 1);
      nlevU[u] = l; nlU = PetscMax(nlU, l + 1);
    }
    HipSetupNote("ILU(0): ... node levels at %.3f s\n", HipWallSeconds() - ta0);
    ierr = PetscOptionsGetInt(HipObjPrefix(F), "-pc_factor_hipmi355x_trisolve_block_columns", &bc, &bset);
    for (int blk = bc ? 1 : 0; blk >= 0 && !ierr && !*made; blk--) {
      if (!mi355x_trisolve_plan_create_nodes_pair(dc->h, n, nodes, nstart, by_level, blk, nlL, nlevL, bi, ra->rlL, nlU, nlevU, ra->rpU, ra->rlU, bj, ra->ba, ra->dinv, &f->syncfree.tri_lo, &f->syncfree.tri_up)) {
        f->syncfree.nodes = nodes; f->syncfree.nlevL_nodes = nlL; f->syncfree.nlevU_nodes = nlU; f->syncfree.by_level = by_level; f->syncfree.block_columns = blk;
        *made = 1;
      } else tri_free_syncfree(f);                             /* not of that shape: the next, more general form */
    }
  }
  HipFree(nstart);
  CHKERRQ(ierr);
  return 0;
}

/* the sync-free plans: node by node for the factor of a matrix with inodes, else row by row.  A factor they cannot hold (e.g. one
 * too large for 32-bit sliced-ELL offsets) is left without plans: the level kernels serve */
static PetscErrorCode ilu0_syncfree_plans(Mat F, Mat A, HipTriFactors *f, PetscDeviceCtx *dc, double ta0) {
  PetscErrorCode ierr;
  const PetscInt n = f->n;
  /* -pc_factor_hipmi355x_trisolve_order <column|level>.  column: every row is summed in column order, the bits of
   * MatSolve_SeqAIJ_NaturalOrdering.  level: in the order of its dependencies' levels (a row then waits on its last
   * entries only) -- the default where the reference does not run the natural-ordering routine either: a matrix with
   * inodes, whose factor it solves with MatSolve_SeqAIJ_Inode (inode.c; MatLUFactorNumeric_SeqAIJ_Inode installs it),
   * in yet another order.  There the two agree to rounding.
   * -pc_factor_hipmi355x_trisolve_nodes 0 keeps the row-granular plans for such a factor. */
  char ord[32] = "", nodeopt[16] = ""; PetscInt nodes = 0; const PetscInt *nsizes = NULL; int made = 0, rc = 0; PetscBool set, nset;
  RowArr ra = {f->host.bi, f->host.bdiag, NULL, NULL, NULL, NULL, NULL};
  if (f->dev.dfac) {   /* the plans' creators take the values from the host: the factor's one copy back */
    const double tf0 = HipWallSeconds();
    if (f->host.owns) { ierr = ilu0_fetch_host_ba(f, dc);CHKERRQ(ierr); }   /* (inside PETSc the parent's array already holds it) */
    HipSetupNote("ILU(0): ... factor values back on the host %.3f s\n", HipWallSeconds() - tf0);
  }
  ra.ba = f->host.ba;
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_trisolve_order", ord, sizeof(ord), &set);CHKERRQ(ierr);
  if (set && strcmp(ord, "column") && strcmp(ord, "level")) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_WRONG, "-pc_factor_hipmi355x_trisolve_order <column|level>, got %s", ord);
  ierr = MatSeqAIJHIPGetInodes(A, &nodes, &nsizes);CHKERRQ(ierr);
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_trisolve_nodes", nodeopt, sizeof(nodeopt), &nset);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * 3 * (size_t)n, &ra.rlL);            /* (one array for the three per-row index arrays) */
  if (!ierr) ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)n, &ra.dinv);
  if (!ierr) {
    ra.rpU = ra.rlL + n; ra.rlU = ra.rpU + n;
    HipParallelRanges(n, ilu0_row_arrays, &ra);
    HipSetupNote("ILU(0): ... row arrays + inode query at %.3f s\n", HipWallSeconds() - ta0);
    /* ILU(k): the node plans take a node's shared column list from A's inodes, which says nothing about the factor's rows once
     * there is fill, so they stay ILU(0)-only: the factor gets the row-granular plans, in column order unless the option asks otherwise -- the bits of MatSolve_SeqAIJ_NaturalOrdering; where the
     * reference would install its inode routines the two agree to rounding */
    if (nodes > 0 && !f->levels && !(nset && (!strcmp(nodeopt, "0") || !strcmp(nodeopt, "false")))) ierr = ilu0_node_plans(F, f, dc, nodes, nsizes, set ? !strcmp(ord, "level") : 1, &ra, ta0, &made);
  }
  if (!ierr && !made) {
    f->syncfree.by_level = set ? !strcmp(ord, "level") : (nodes > 0 && !f->levels);
    rc = mi355x_trisolve_plan_create_pair(dc->h, n, f->syncfree.by_level, f->lev.nlevL, f->lev.rlevL, ra.bi, ra.rlL, f->host.bj, ra.ba, f->lev.nlevU, f->lev.rlevU, ra.rpU, ra.rlU, f->host.bj, ra.ba, ra.dinv, NULL, &f->syncfree.tri_lo, &f->syncfree.tri_up);
  }
  HipFree(ra.rlL); HipFree(ra.dinv);
  CHKERRQ(ierr);
  HipSetupNote("ILU(0): ... plans made at %.3f s\n", HipWallSeconds() - ta0);
  if (rc) tri_free_syncfree(f);
  else HipTriWatchAdd(f);
  return 0;
}

/* the level-scheduled kernels work on the reference's layout itself, rows listed level by level.  The host routes upload all of it.
 * On the device route the launches read launch.d_ba itself, the index arrays and the rows of L are borrowed from the context, the rows
 * of U uploaded -- and a factorisation with the pattern of the last one finds all of it in place, the captured graph included */
static PetscErrorCode ilu0_level_form(HipTriFactors *f, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  const PetscInt n = f->n;
  const size_t ni = sizeof(PetscInt) * (size_t)(n + 1), nj = sizeof(PetscInt) * (size_t)(f->nz + 1), na = sizeof(PetscScalar) * (size_t)(f->nz + 1), nr = sizeof(PetscInt) * (size_t)n;
  PetscInt *rowsL = NULL, *rowsU = NULL; int rc = 0;
  if (f->dev.dfac && f->launch.d_rowsU) return 0;
  HipFree(f->launch.levptrL); HipFree(f->launch.levptrU); f->launch.levptrL = f->launch.levptrU = NULL;
  ierr = level_order(n, f->lev.rlevL, f->lev.nlevL, &f->launch.levptrL, &rowsL);   /* where each level starts: kept; its rows: uploaded */
  if (!ierr) ierr = level_order(n, f->lev.rlevU, f->lev.nlevU, &f->launch.levptrU, &rowsU);
  if (!ierr && f->dev.dfac) {
    const int *cbi, *cbj, *cbd, *crows;
    rc = mi355x_ilu0_factor_arrays(f->dev.dfac, &cbi, &cbj, &cbd, &crows);
    if (!rc) { f->launch.d_bi = (PetscInt *)cbi; f->launch.d_bj = (PetscInt *)cbj; f->launch.d_bdiag = (PetscInt *)cbd; f->launch.d_rowsL = (PetscInt *)crows; f->launch.borrowed = 1; }
  } else if (!ierr) {
    struct { void *p; const void *from; size_t bytes; } up[] = {{&f->launch.d_bi, f->host.bi, ni}, {&f->launch.d_bj, f->host.bj, nj}, {&f->launch.d_bdiag, f->host.bdiag, ni}, {&f->launch.d_ba, f->host.ba, na}, {&f->launch.d_rowsL, rowsL, nr}};
    for (size_t i = 0; i < sizeof(up) / sizeof(up[0]) && !rc; i++) {
      rc = mi355x_malloc((void **)up[i].p, PetscMax(up[i].bytes, sizeof(PetscInt)));
      if (!rc) rc = mi355x_memcpy_h2d(dc->h, *(void **)up[i].p, up[i].from, up[i].bytes);
    }
  }
  if (!ierr && !rc) rc = mi355x_malloc((void **)&f->launch.d_rowsU, PetscMax(nr, sizeof(PetscInt)));
  if (!ierr && !rc) rc = mi355x_memcpy_h2d(dc->h, f->launch.d_rowsU, rowsU, nr);
  if (!ierr && !rc) rc = mi355x_handle_synchronize(dc->h);   /* the rows' host copies go away below */
  HipFree(rowsL); HipFree(rowsU);
  CHKERRQ(ierr);
  CHKHIP(rc);
  return 0;
}

/* everything MatSolve needs, in the form -pc_factor_hipmi355x_trisolve asks for, from the host factor in f->host (the reference's
 * layout, whoever computed it) or, on the device route, the values in launch.d_ba.  The row levels are the factor's (lev.rlevL / rlevU)
 * for the time of the analysis: the harness's host factorisation left them, the device route kept them from the last factorisation of
 * this pattern (which then analyses nothing), else they are computed here; only the device route keeps them afterwards */
static PetscErrorCode ilu0_analyse_and_upload(Mat F, Mat A) {
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  PetscDeviceCtx *dc;
  PetscInt sweeps = 0; int syncfree = 0; PetscBool set;
  const double ta0 = HipWallSeconds();
  const int from_device = f->dev.dfac != NULL;
  if (!f->lev.rlevL || !f->lev.rlevU) { ierr = ilu0_row_levels(f->n, f->host.bi, f->host.bj, f->host.bdiag, &f->lev.rlevL, &f->lev.nlevL, &f->lev.rlevU, &f->lev.nlevU);CHKERRQ(ierr); }
  HipSetupNote("ILU(0): row levels %.3f s\n", HipWallSeconds() - ta0);
  ierr = PetscDeviceGet(&dc);
  if (!ierr) ierr = ilu0_trisolve_mode(F, &sweeps, &syncfree, &set);
  if (!ierr && sweeps) {   /* no sync-free plans, no level lists, not on the watch list: the level counts are all the analysis this mode keeps */
    ierr = ilu0_sweeps_setup(f, dc, from_device);
    if (!ierr) f->sw.sweeps = sweeps;
  } else if (!ierr) {
    tri_free_sweeps(f);
    /* sync-free solves: worth it as soon as the level launches would be a launch-bound chain */
    if (syncfree && f->n > 0 && (f->lev.nlevL + f->lev.nlevU > 16 || set)) ierr = ilu0_syncfree_plans(F, A, f, dc, ta0);
    if (!ierr && !f->syncfree.tri_lo) ierr = ilu0_level_form(f, dc);
  }
  if (!from_device) { HipFree(f->lev.rlevL); HipFree(f->lev.rlevU); f->lev.rlevL = f->lev.rlevU = NULL; }
  CHKERRQ(ierr);
  return 0;
}

/* the device route's symbolic side, once per pattern: pattern and row levels on the host (kept), the context, the array of the values */
static PetscErrorCode ilu0_device_symbolic(Mat F, Mat A, PetscDeviceCtx *dc, PetscInt levels, PetscInt nblk, const PetscInt *blk, double *clock) {
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  PetscInt n, *levptr = NULL, *rows = NULL; const PetscInt *ai, *aj;
  ierr = MatSeqAIJGetArrays(A, &n, &ai, &aj, NULL);CHKERRQ(ierr);
  HipTriFactorsResetNumeric(f);
  tri_free_sweeps(f);
  f->n = n; f->nz = ai[n];
#if defined(PETSCHIPMI355X_WITH_PETSC)
  { Mat_SeqAIJ *b = (Mat_SeqAIJ *)F->data;   /* the parent's symbolic arrays (MatILUFactorSymbolic_SeqAIJ_ilu0, or MatILUFactorSymbolic_SeqAIJ with levels of fill) */
    f->nz = b->nz; f->host.bi = b->i; f->host.bj = b->j; f->host.bdiag = b->diag; f->host.ba = b->a; f->host.owns = PETSC_FALSE;
    f->levels = levels; f->nzA = ai[n]; }
#else
  ierr = ilu_symbolic_host(A, n, ai, aj, levels, f, NULL, NULL, NULL);CHKERRQ(ierr);
#endif
  HipSetupTick(*clock, "factor (device): pattern of L and U");
  ierr = ilu0_check_blocks(A, ai, aj, nblk, blk);CHKERRQ(ierr);
  ierr = ilu0_row_levels(n, f->host.bi, f->host.bj, f->host.bdiag, &f->lev.rlevL, &f->lev.nlevL, &f->lev.rlevU, &f->lev.nlevU);CHKERRQ(ierr);
  ierr = level_order(n, f->lev.rlevL, f->lev.nlevL, &levptr, &rows);CHKERRQ(ierr);
  HipSetupTick(*clock, "factor (device): levels of L and U");
  /* zero fill: position p of A's row IS position p of the factor's row, the ILU(0) kernel; with fill the kernel that finds A's entries by column */
  int rc = levels ? mi355x_ilu0_factor_create_fill(dc->h, n, ai, aj, f->host.bi, f->host.bj, f->host.bdiag, f->lev.nlevL, levptr, rows, nblk, blk, &f->dev.dfac)
                  : mi355x_ilu0_factor_create(dc->h, n, f->host.bi, f->host.bj, f->host.bdiag, f->lev.nlevL, levptr, rows, nblk, blk, &f->dev.dfac);
  HipFree(levptr); HipFree(rows);
  if (!rc) rc = mi355x_malloc((void **)&f->launch.d_ba, sizeof(PetscScalar) * (size_t)(f->nz + 1));
  if (!rc) rc = mi355x_memset(dc->h, f->launch.d_ba, 0, sizeof(PetscScalar) * (size_t)(f->nz + 1));   /* (the slot past the last value is never written) */
  CHKHIP(rc);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nblk + 1), &f->dev.blk);CHKERRQ(ierr);
  memcpy(f->dev.blk, blk, sizeof(PetscInt) * (size_t)(nblk + 1));
  f->dev.gen = ((Mat_SeqAIJHIP *)A->spptr)->pattern_gen; f->dev.n = n; f->dev.nz = ai[n]; f->dev.levels = levels; f->dev.nblk = nblk; f->dev.stale = 0;
  f->symbolic_builds++;
  HipSetupTick(*clock, "factor (device): context and index upload");
  return 0;
}
/* the numeric passes on the device.  The shift rule is ilu0_factor_host's (ilu0_next_shift), per independent block, all blocks in
 * one pass: a block whose pass reports a failing pivot runs again shifted, the other blocks' rows skip their work in those passes */
static PetscErrorCode ilu0_device_numeric(Mat A, HipTriFactors *f, PetscDeviceCtx *dc, PetscInt nblk, const MatFactorInfo *info, double *clock) {
  PetscErrorCode ierr;
  Mat_SeqAIJHIP *d = (Mat_SeqAIJHIP *)A->spptr;
  PetscReal *shifts = NULL, badval = 0.0; PetscInt *nsh = NULL, badrow = -1; int rc = 0, any = 1;
  ierr = PetscMalloc(sizeof(PetscReal) * 2 * (size_t)nblk, &shifts);       /* per block: the shift and the failing pivot's size; */
  if (!ierr) ierr = PetscMalloc(sizeof(PetscInt) * 2 * (size_t)nblk, &nsh);   /* the shifts taken and the failing row */
  if (ierr) { HipFree(shifts); CHKERRQ(ierr); }
  PetscReal *fabsv = shifts + nblk; PetscInt *frow = nsh + nblk;
  for (PetscInt bb = 0; bb < nblk; bb++) { shifts[bb] = 0.0; nsh[bb] = 0; }
  mi355x_ilu0_factor_reset(f->dev.dfac);
  while (any && !ierr && !rc) {
    any = 0;
    rc = mi355x_ilu0_factor_run(dc->h, f->dev.dfac, d->mat.i, d->mat.j, d->mat.a, info->zeropivot, shifts, f->launch.d_ba, frow, fabsv);
    for (PetscInt bb = 0; bb < nblk && !ierr && !rc; bb++) {
      if (frow[bb] < 0) continue;
      if (!any) { badrow = frow[bb]; badval = fabsv[bb]; }
      any = 1;
      ierr = ilu0_next_shift(info, &shifts[bb], &nsh[bb]);
    }
  }
  f->nshift = 0;
  for (PetscInt bb = 0; bb < nblk; bb++) f->nshift = PetscMax(f->nshift, nsh[bb]);
  HipFree(shifts); HipFree(nsh);
  HipSetupTick(*clock, "factor (device): numeric passes");
  CHKHIP(rc);
  if (ierr) return ilu0_zero_pivot(A, info, badrow, badval);
  f->numeric_runs++;
  return 0;
}
/* -pc_factor_hipmi355x_numeric device: the numeric ILU(0) on the device, one launch per dependency level of L
 * (mi355x_ilu0_factor_*, csrc/ilu_factor.hip), reading A's device copy in place and writing the factor's values to launch.d_ba.  The
 * symbolic work -- diagonal positions, pattern of L and U, row levels -- stays on the host and is kept with the factor: a
 * factorisation whose A has the pattern of the last one (the same upload of the operator's pattern, Mat_SeqAIJHIP.pattern_gen -- a serial number no other matrix or
 * later pattern shares -- with the same sizes and the same independent blocks) runs the numeric kernels only. */
static PetscErrorCode ilu0_factor_device(Mat F, Mat A, const MatFactorInfo *info) {
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  Mat_SeqAIJHIP *d = (Mat_SeqAIJHIP *)A->spptr;
  PetscDeviceCtx *dc;
  PetscInt n, whole[2]; const PetscInt *ai, *aj, *blk;
  double tick0 = HipWallSeconds();
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJGetArrays(A, &n, &ai, &aj, NULL);CHKERRQ(ierr);          /* (the values are read on the device) */
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (d->cprow || d->mat.bs != 1 || (n > 0 && !d->mat.a)) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "-pc_factor_hipmi355x_numeric device needs the operator's plain CSR copy on the device");
  HipSetupTick(tick0, "factor (device): operator current");
  const PetscInt nblk = HipTriFactorsBlocks(f, n, whole, &blk);
  const int same = f->dev.dfac && !f->dev.stale && d->pattern_gen && f->dev.gen == d->pattern_gen && f->dev.n == n && f->dev.nz == ai[n] &&
                   f->dev.levels == (PetscInt)info->levels && f->dev.nblk == nblk && !memcmp(f->dev.blk, blk, sizeof(PetscInt) * (size_t)(nblk + 1));
  f->factored_state = -1;
  if (same) {   /* values only: the plans that carry values go, everything built from the pattern stays */
    tri_free_syncfree(f);
    tri_free_transpose(f, 0);
    f->nshift = 0; f->sw.sweeps = 0;
  } else { ierr = ilu0_device_symbolic(F, A, dc, (PetscInt)info->levels, nblk, blk, &tick0);CHKERRQ(ierr); }
  ierr = ilu0_device_numeric(A, f, dc, nblk, info, &tick0);CHKERRQ(ierr);
#if defined(PETSCHIPMI355X_WITH_PETSC)
  ierr = ilu0_fetch_host_ba(f, dc);CHKERRQ(ierr);                        /* the parent's b->a holds the factor, as after its own routine */
  F->assembled = PETSC_TRUE; F->preallocated = PETSC_TRUE;
  HipSetupTick(tick0, "factor (device): values to the parent's array");
#endif
  return 0;
}

static PetscErrorCode MatSolve_SeqAIJHIP_ILU(Mat F, Vec b, Vec x);
static PetscErrorCode MatSolveTranspose_SeqAIJHIP_ILU(Mat F, Vec b, Vec x);
static PetscErrorCode MatLUFactorNumeric_SeqAIJHIP(Mat F, Mat A, const MatFactorInfo *info) {   /* MatLUFactorNumeric_SeqAIJCUSPARSE, aijcusparse.cu:358-376 */
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  const double t0 = HipWallSeconds();
  int on_device = 0;
  if (A->rmap->n != A->cmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "Must be square matrix, rows %d columns %d", A->rmap->n, A->cmap->n);
  if (f->factored_state == HipObjState(A) && f->factored_of == (void *)A && (f->syncfree.tri_lo || f->launch.d_ba || f->sw.sweeps)) return 0;   /* same operator, same values: nothing to redo */
  { char where[16] = "host"; PetscBool set;   /* -pc_factor_hipmi355x_numeric <host|device>, an opt-in */
    ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_numeric", where, sizeof(where), &set);CHKERRQ(ierr);
    if (strcmp(where, "host") && strcmp(where, "device")) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_WRONG, "-pc_factor_hipmi355x_numeric <host|device>, got %s", where);
    on_device = !strcmp(where, "device"); }
  if (on_device) { ierr = ilu0_factor_device(F, A, info);CHKERRQ(ierr); }
  else {
    HipTriFactorsResetNumeric(f);
#if defined(PETSCHIPMI355X_WITH_PETSC)
    ierr = MatLUFactorNumeric_SeqAIJ(F, A, info);CHKERRQ(ierr);            /* the parent's factorisation into F's own Mat_SeqAIJ */
    { Mat_SeqAIJ *b = (Mat_SeqAIJ *)F->data;
      f->n = A->rmap->n; f->nz = b->nz; f->host.bi = b->i; f->host.bj = b->j; f->host.bdiag = b->diag; f->host.ba = b->a; f->host.owns = PETSC_FALSE;
      f->levels = (PetscInt)info->levels; f->nzA = ((Mat_SeqAIJ *)A->data)->nz; }
#else
    ierr = ilu0_factor_host(F, A, info);CHKERRQ(ierr);
#endif
    f->symbolic_builds++; f->numeric_runs++;
  }
  const double t1 = HipWallSeconds();
  ierr = ilu0_analyse_and_upload(F, A);CHKERRQ(ierr);
  HipSetupNote("ILU(0) n=%d: %s factorisation %.3f s, level analysis + plans + upload %.3f s\n", (int)f->n, on_device ? "device" : "host", t1 - t0, HipWallSeconds() - t1);
  F->ops->solve = MatSolve_SeqAIJHIP_ILU;                                 /* aijcusparse.cu:372-373 */
  F->ops->solvetranspose = MatSolveTranspose_SeqAIJHIP_ILU;
  f->factored_state = HipObjState(A); f->factored_of = (void *)A;
  return 0;
}

static PetscErrorCode MatILUFactorSymbolic_SeqAIJHIP(Mat F, Mat A, IS row, IS col, const MatFactorInfo *info) {   /* aijcusparse.cu:175-186 */
  PetscErrorCode ierr = natural_ordering_only(A, row, col, info, "ILU");CHKERRQ(ierr);
  if (strcmp(HipObjTypeName(A), MATSEQAIJHIPMI355X)) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "ILU on the device needs a sequential AIJ matrix of this type (use -pc_type bjacobi -sub_pc_type ilu in parallel); got %s", HipObjTypeName(A));
#if defined(PETSCHIPMI355X_WITH_PETSC)
  ierr = MatILUFactorSymbolic_SeqAIJ(F, A, row, col, info);CHKERRQ(ierr);
#endif
  HipTriGet(F)->factored_state = -1;
  HipTriGet(F)->dev.stale = 1;                                            /* a new symbolic phase: the device route's context is of the old pattern */
  F->ops->lufactornumeric = MatLUFactorNumeric_SeqAIJHIP;
  return 0;
}

/* y = U^-1 L^-1 b through whatever the analysis prepared.  After a sync-free application gave up (HipTriWatchCheck), the same
 * plans run level by level. */
PetscErrorCode HipTriFactorsApply(Mat F, HipTriFactors *f, Vec b, Vec x, PetscLogDouble flops) {
  PetscErrorCode ierr;
  const PetscScalar *db; PetscScalar *dx; PetscDeviceCtx *dc;
  int rc;
  if (!f->n) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = VecHIPGetRead(b, &db);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(x, &dx);CHKERRQ(ierr);
  if (f->syncfree.use_levels) rc = mi355x_trisolve_apply_levels(dc->h, f->syncfree.tri_lo, f->syncfree.tri_up, db, dx);
  else {
    rc = mi355x_trisolve_apply(dc->h, f->syncfree.tri_lo, f->syncfree.tri_up, db, dx);
    if (rc == 719) {   /* hipErrorLaunchFailure: an earlier application gave up and no host wait has noticed yet: this one runs level by level */
      f->syncfree.use_levels = 1; f->aborted = 1;
      rc = mi355x_trisolve_apply_levels(dc->h, f->syncfree.tri_lo, f->syncfree.tri_up, db, dx);
    } else if (rc == 1 || rc == 701 || rc == 720) {   /* hipErrorInvalidValue / LaunchOutOfResources / cooperative too large: the sync-free kernels could not be launched on this
                                                        * device (LDS, registers): nothing ran, so the same plans serve one launch per level from now on */
      f->syncfree.use_levels = 1;
      rc = mi355x_trisolve_apply_levels(dc->h, f->syncfree.tri_lo, f->syncfree.tri_up, db, dx);
    }
  }
  ierr = VecHIPRestoreWrite(x);CHKERRQ(ierr);      /* also on the error path: x is not left in write state */
  HipStateIncrease(x);
  CHKHIP(rc);
  ierr = PetscLogFlops(flops);CHKERRQ(ierr);
  (void)F;
  return 0;
}

/* the level launches: L's levels forward from in to out, then U's backwards in place on out (in == out: in place throughout) */
static int ilu0_launch_levels(PetscDeviceCtx *dc, const HipTriFactors *f, const PetscScalar *in, PetscScalar *out) {
  int rc = 0;
  for (PetscInt l = 0; l < f->lev.nlevL && !rc; l++)
    rc = mi355x_ilu0_lower_level(dc->h, f->launch.levptrL[l + 1] - f->launch.levptrL[l], f->launch.d_rowsL + f->launch.levptrL[l], f->launch.d_bi, f->launch.d_bj, f->launch.d_ba, in, out);
  for (PetscInt l = 0; l < f->lev.nlevU && !rc; l++)
    rc = mi355x_ilu0_upper_level(dc->h, f->launch.levptrU[l + 1] - f->launch.levptrU[l], f->launch.d_rowsU + f->launch.levptrU[l], f->launch.d_bj, f->launch.d_ba, f->launch.d_bdiag, out);
  return rc;
}
static PetscErrorCode MatSolve_SeqAIJHIP_ILU(Mat F, Vec b, Vec x) {   /* MatSolve_SeqAIJCUSPARSE_NaturalOrdering, aijcusparse.cu:419-445 */
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  const PetscScalar *db; PetscScalar *dx; PetscDeviceCtx *dc;
  if (f->sw.sweeps) return ilu0_sweeps_apply(f, b, x);
  if (f->syncfree.tri_lo) return HipTriFactorsApply(F, f, b, x, 2.0 * f->nz - f->n);
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = VecHIPGetRead(b, &db);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(x, &dx);CHKERRQ(ierr);
  /* The level launches are a launch-bound inner loop (766 + 766 kernels for P7(256)): with more than a handful of levels they
   * are captured once into a hipGraph that works in place on a fixed buffer and replayed per application (copy in, one graph
   * launch, copy out).  Same kernels, same order, same bits. */
  if (!f->launch.graph_tried && f->lev.nlevL + f->lev.nlevU > 16) {
    f->launch.graph_tried = 1;
    if (!mi355x_malloc((void **)&f->launch.d_work, sizeof(PetscScalar) * (size_t)PetscMax(f->n, 1)) && !mi355x_graph_capture_begin(dc->h)) {
      const int bad = ilu0_launch_levels(dc, f, f->launch.d_work, f->launch.d_work);
      void *g = NULL;
      if (mi355x_graph_capture_end(dc->h, &g) || bad) g = NULL;   /* capture failed: stay with plain launches */
      f->launch.graph = g;
    }
  }
  int rc = 0;
  if (f->launch.graph) {
    rc = mi355x_vec_copy(dc->h, (size_t)f->n, db, f->launch.d_work);
    if (!rc) rc = mi355x_graph_launch(dc->h, f->launch.graph);
    if (!rc) rc = mi355x_vec_copy(dc->h, (size_t)f->n, f->launch.d_work, dx);
  } else rc = ilu0_launch_levels(dc, f, db, dx);
  ierr = VecHIPRestoreWrite(x);CHKERRQ(ierr);
  HipStateIncrease(x);
  CHKHIP(rc);
  ierr = PetscLogFlops(2.0 * f->nz - f->n);CHKERRQ(ierr);
  return 0;
}

/* ---------------------------------------------------------------- the transposed factor: MatSolveTranspose
 * MatSolveTranspose_SeqAIJ (aijfact.c) with the natural ordering -- t = b; forward with U^T: s = t[i] * inverted diagonal, t[j] -= s u(i,j)
 * over U's strict row i, t[i] = s; backward with L^T: t[j] -= t[i] l(i,j) over L's row i -- run as a gather over the two transposed
 * triangles (csrc/trisolve_transpose.hip: the same bits, no atomics), one launch per dependency level, replayed from a hipGraph when
 * there are more than a handful.  It serves ILU(0) and ILU(k) whatever -pc_factor_hipmi355x_trisolve chose for the forward application,
 * except sweeps:<k>: that application is approximate and has no transposed counterpart.  Row-granular also for the factor of a matrix
 * with inodes.  The form is built at the first transposed solve after a factorisation: pattern work (transposed patterns, levels, row
 * lists, index upload) once per pattern of the FACTOR, told by comparing the host pattern (bi / bj / bdiag are on the host on every
 * route today -- the symbolic phase runs there also under -pc_factor_hipmi355x_numeric device, which has no host VALUES only; a route
 * without a host pattern would have to key this form like f->dev, by pattern_gen, n, nz and the levels of fill; the comparison costs one
 * pass over nz ints per factorisation and does not depend on the operator having been uploaded); the values by one gather from the factor's
 * device values (launch.d_ba) when they are there, else gathered on the host and uploaded. */
static PetscErrorCode ilut_pattern(HipTriFactors *f, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  const PetscInt n = f->n, nz = f->nz, *bi = f->host.bi, *bj = f->host.bj, *bdiag = f->host.bdiag;
  const PetscInt nzL = bi[n], nzU = nz - nzL - n;
  const size_t ni = sizeof(PetscInt) * (size_t)(n + 1), nj = sizeof(PetscInt) * (size_t)PetscMax(nz, 1);
  PetscInt *hw, *rows1 = NULL, *rows2 = NULL; int rc;
  tri_free_transpose(f, 1);
  /* one host work array: ti, si (n + 1 each), tj, sj, then perm = tperm | sperm | bdiag[0 .. n), then the two level arrays */
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(2 * (n + 1) + 2 * (nzU + nzL) + 3 * n + 1), &hw);CHKERRQ(ierr);
  PetscInt *ti = hw, *si = ti + n + 1, *tj = si + n + 1, *sj = tj + nzU, *perm = sj + nzL, *lev1 = perm + nzU + nzL + n, *lev2 = lev1 + n;
  int nlev1 = 0, nlev2 = 0;
  rc = mi355x_ilut_build_host(n, bi, bj, bdiag, ti, tj, perm, si, sj, perm + nzU, lev1, &nlev1, lev2, &nlev2);
  if (rc) { HipFree(hw); CHKHIP(rc); }
  memcpy(perm + nzU + nzL, bdiag, sizeof(PetscInt) * (size_t)n);
  f->tr.nlev1 = nlev1; f->tr.nlev2 = nlev2;
  ierr = level_order(n, lev1, nlev1, &f->tr.levptr1, &rows1);
  if (!ierr) ierr = level_order(n, lev2, nlev2, &f->tr.levptr2, &rows2);
  if (!ierr) {
    struct { void *p; const void *from; size_t bytes; } up[] = {{&f->tr.d_ti, ti, ni}, {&f->tr.d_si, si, ni}, {&f->tr.d_tj, tj, sizeof(PetscInt) * (size_t)nzU},
      {&f->tr.d_sj, sj, sizeof(PetscInt) * (size_t)nzL}, {&f->tr.d_perm, perm, sizeof(PetscInt) * (size_t)(nzU + nzL + n)},
      {&f->tr.d_rows1, rows1, sizeof(PetscInt) * (size_t)n}, {&f->tr.d_rows2, rows2, sizeof(PetscInt) * (size_t)n}};
    for (size_t i = 0; i < sizeof(up) / sizeof(up[0]) && !rc; i++) {
      rc = mi355x_malloc((void **)up[i].p, PetscMax(up[i].bytes, sizeof(PetscInt)));
      if (!rc && up[i].bytes) rc = mi355x_memcpy_h2d(dc->h, *(void **)up[i].p, up[i].from, up[i].bytes);
    }
    if (!rc) rc = mi355x_malloc((void **)&f->tr.d_val, sizeof(PetscScalar) * (size_t)PetscMax(nzU + nzL + n, 1));
    if (!rc) rc = mi355x_handle_synchronize(dc->h);   /* the host arrays go away below */
  }
  if (!ierr && !rc) {   /* what the form was built for */
    ierr = PetscMalloc(ni, &f->tr.bi); if (!ierr) ierr = PetscMalloc(ni, &f->tr.bdiag); if (!ierr) ierr = PetscMalloc(nj, &f->tr.bj);
    if (!ierr) ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nzU + nzL + n, 1), &f->tr.perm);
    if (!ierr) { memcpy(f->tr.bi, bi, ni); memcpy(f->tr.bdiag, bdiag, ni); memcpy(f->tr.bj, bj, sizeof(PetscInt) * (size_t)nz); memcpy(f->tr.perm, perm, sizeof(PetscInt) * (size_t)(nzU + nzL + n)); }
  }
  HipFree(hw); HipFree(rows1); HipFree(rows2);
  if (ierr || rc) tri_free_transpose(f, 1);
  CHKERRQ(ierr);
  CHKHIP(rc);
  f->tr.n = n; f->tr.nz = nz; f->tr.levels = f->levels; f->tr.nzU = nzU; f->tr.nzL = nzL; f->tr.built = 1;
  f->tr.pattern_builds++;
  return 0;
}
static PetscErrorCode ilut_values(HipTriFactors *f, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  const PetscInt nv = f->tr.nzU + f->tr.nzL + f->tr.n;
  int rc = 0;
  if (f->launch.d_ba) rc = mi355x_pack(dc->h, (size_t)nv, f->tr.d_perm, f->launch.d_ba, f->tr.d_val);
  else {   /* the factor's values are on the host only (the sync-free plans took them from there) */
    const PetscScalar *ba = f->host.ba; PetscScalar *val;
    if (!ba) SETERRQ(PETSC_COMM_SELF, PETSC_ERR_PLIB, "the factor's values are neither on the device nor on the host");
    ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(nv, 1), &val);CHKERRQ(ierr);
    for (PetscInt k = 0; k < nv; k++) val[k] = ba[f->tr.perm[k]];
    if (nv) rc = mi355x_memcpy_h2d(dc->h, f->tr.d_val, val, sizeof(PetscScalar) * (size_t)nv);
    if (!rc) rc = mi355x_handle_synchronize(dc->h);      /* val goes away below */
    HipFree(val);
  }
  CHKHIP(rc);
  f->tr.fresh = 1;
  return 0;
}
static PetscErrorCode ilut_form(HipTriFactors *f, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  const PetscInt n = f->n, nz = f->nz;
  const size_t ni = sizeof(PetscInt) * (size_t)(n + 1);
  if (f->tr.built && f->tr.fresh) return 0;
  if (!f->host.bi || !f->host.bj || !f->host.bdiag) SETERRQ(PETSC_COMM_SELF, PETSC_ERR_ARG_WRONGSTATE, "MatSolveTranspose: the matrix holds no numeric factorisation");
  const int same = f->tr.built && f->tr.n == n && f->tr.nz == nz && f->tr.levels == f->levels &&
                   !memcmp(f->tr.bi, f->host.bi, ni) && !memcmp(f->tr.bdiag, f->host.bdiag, ni) && !memcmp(f->tr.bj, f->host.bj, sizeof(PetscInt) * (size_t)nz);
  if (!same) { ierr = ilut_pattern(f, dc);CHKERRQ(ierr); }
  ierr = ilut_values(f, dc);CHKERRQ(ierr);
  if (same) f->tr.value_refreshes++;
  return 0;
}
/* U^T's levels forward from in to out, then L^T's in place on out (in == out: in place throughout) */
static int ilut_launch_levels(PetscDeviceCtx *dc, const HipTriFactors *f, const PetscScalar *in, PetscScalar *out) {
  const PetscScalar *ta = f->tr.d_val, *sa = ta + f->tr.nzU, *dinv = sa + f->tr.nzL;
  int rc = 0;
  for (PetscInt l = 0; l < f->tr.nlev1 && !rc; l++)
    rc = mi355x_ilut_first_level(dc->h, f->tr.levptr1[l + 1] - f->tr.levptr1[l], f->tr.d_rows1 + f->tr.levptr1[l], f->tr.d_ti, f->tr.d_tj, ta, dinv, in, out);
  for (PetscInt l = 0; l < f->tr.nlev2 && !rc; l++)
    rc = mi355x_ilut_second_level(dc->h, f->tr.levptr2[l + 1] - f->tr.levptr2[l], f->tr.d_rows2 + f->tr.levptr2[l], f->tr.d_si, f->tr.d_sj, sa, out);
  return rc;
}
static PetscErrorCode MatSolveTranspose_SeqAIJHIP_ILU(Mat F, Vec b, Vec x) {
  PetscErrorCode ierr;
  HipTriFactors *f = HipTriGet(F);
  const PetscScalar *db; PetscScalar *dx; PetscDeviceCtx *dc;
  if (b == x) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_IDN, "x and b must be different vectors");
  if (f->sw.sweeps) SETERRQ(HipObjComm(F), PETSC_ERR_SUP, "MatSolveTranspose with -pc_factor_hipmi355x_trisolve sweeps:<k>: the sweeps apply the factor approximately and no transposed counterpart is defined");
  if (!f->n) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = ilut_form(f, dc);CHKERRQ(ierr);
  ierr = VecHIPGetRead(b, &db);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(x, &dx);CHKERRQ(ierr);
  /* as MatSolve's level launches: a single chain of kernels, captured once per pattern in place on a fixed buffer (the value array it
   * names is refilled in place by a later factorisation of the same pattern) */
  if (!f->tr.graph_tried && f->tr.nlev1 + f->tr.nlev2 > 16) {
    f->tr.graph_tried = 1;
    if (!mi355x_malloc((void **)&f->tr.d_work, sizeof(PetscScalar) * (size_t)PetscMax(f->n, 1)) && !mi355x_graph_capture_begin(dc->h)) {
      const int bad = ilut_launch_levels(dc, f, f->tr.d_work, f->tr.d_work);
      void *g = NULL;
      if (mi355x_graph_capture_end(dc->h, &g)) g = NULL;
      else if (bad) { mi355x_graph_destroy(g); g = NULL; }        /* a launch failed inside the capture: the graph is of no use */
      f->tr.graph = g;
    }
    if (!f->tr.graph && f->tr.d_work) { mi355x_free(f->tr.d_work); f->tr.d_work = NULL; }   /* capture failed: plain launches, no buffer kept */
  }
  int rc = 0;
  if (f->tr.graph) {
    rc = mi355x_vec_copy(dc->h, (size_t)f->n, db, f->tr.d_work);
    if (!rc) rc = mi355x_graph_launch(dc->h, f->tr.graph);
    if (!rc) rc = mi355x_vec_copy(dc->h, (size_t)f->n, f->tr.d_work, dx);
  } else rc = ilut_launch_levels(dc, f, db, dx);
  ierr = VecHIPRestoreWrite(x);CHKERRQ(ierr);
  HipStateIncrease(x);
  CHKHIP(rc);
  ierr = PetscLogFlops(2.0 * f->nz - f->n);CHKERRQ(ierr);
  return 0;
}

/* ---------------------------------------------------------------- MatGetFactor */
#if defined(PETSCHIPMI355X_WITH_PETSC)
static PetscErrorCode MatDestroy_Factor_SeqAIJHIP(Mat F) {   /* the factor's device state first, spptr zeroed, then the parent's destroy (aijcusp.cu:584-586) */
  HipTriFactors *f = HipTriGet(F);
  PetscErrorCode (*parent)(Mat) = f ? f->parent_destroy : NULL;
  PetscErrorCode ierr = HipTriFactorsDestroy(&f);CHKERRQ(ierr);
  F->spptr = 0;
  if (parent) { ierr = (*parent)(F);CHKERRQ(ierr); }
  return 0;
}
#endif

PetscErrorCode MatGetFactor_seqaijhipmi355x_petsc(Mat A, MatFactorType ftype, Mat *B) {   /* MatGetFactor_seqaij_cusparse, aijcusparse.cu:57-75 */
  PetscErrorCode ierr;
  HipTriFactors *f;
  if (ftype != MAT_FACTOR_ILU && ftype != MAT_FACTOR_ICC) SETERRQ(PETSC_COMM_SELF, PETSC_ERR_SUP, "Factor type not supported for HIPMI355X matrix types (ILU(k) and ICC(0) are)");
  ierr = PetscMalloc(sizeof(*f), &f);CHKERRQ(ierr);
  memset(f, 0, sizeof(*f));
  f->kind = ftype; f->factored_state = -1;
  tri_live++;
#if defined(PETSCHIPMI355X_WITH_PETSC)
  ierr = MatGetFactor_seqaij_petsc(A, ftype, B);CHKERRQ(ierr);           /* the parent's factor matrix (MATSEQAIJ / MATSEQSBAIJ) with its host routines */
  f->parent_destroy = (*B)->ops->destroy;
  (*B)->spptr = f;
  (*B)->ops->destroy = MatDestroy_Factor_SeqAIJHIP;
#else
  { const PetscInt n = A->rmap->n;
    ierr = MatCreate(HipObjComm(A), B);CHKERRQ(ierr);
    ierr = MatSetSizes(*B, n, n, n, n);CHKERRQ(ierr);
    ierr = MatSetType(*B, MATSEQAIJHIPMI355X);CHKERRQ(ierr);
    ((Mat_SeqAIJHIP *)(*B)->spptr)->tri = f; }
#endif
  (*B)->ops->ilufactorsymbolic = MatILUFactorSymbolic_SeqAIJHIP;
  (*B)->ops->iccfactorsymbolic = MatICCFactorSymbolic_SeqAIJHIP;
  (*B)->factortype = ftype;
  ierr = PetscObjectComposeFunction((PetscObject)*B, "MatFactorSetIndependentBlocks_C", "MatFactorSetIndependentBlocks_SeqAIJHIP", (PetscVoidFunction)MatFactorSetIndependentBlocks_SeqAIJHIP);CHKERRQ(ierr);
  return 0;
}
PetscErrorCode MatGetFactorAvailable_seqaijhipmi355x_petsc(Mat A, MatFactorType ftype, PetscBool *flg) {   /* MatGetFactorAvailable_seqaij_petsc, aijfact.c:97 */
  (void)A;
  *flg = (PetscBool)(ftype == MAT_FACTOR_ILU || ftype == MAT_FACTOR_ICC);
  return 0;
}

/* ---------------------------------------------------------------- introspection (tests / DESIGN.md), through the PC's public face */
static PetscErrorCode pc_factors(PC pc, MatFactorType kind, HipTriFactors **f) {
  PetscErrorCode ierr;
  Mat F = NULL;
  ierr = PCFactorGetMatrix(pc, &F);CHKERRQ(ierr);
  if (!F || !F->factortype || !HipTriGet(F) || HipTriGet(F)->kind != kind) SETERRQ(HipObjComm(pc), PETSC_ERR_ARG_WRONG, "not a set-up %s over a HIPMI355X factored matrix", kind == MAT_FACTOR_ILU ? "PCILU" : "PCICC");
  *f = HipTriGet(F);
  return 0;
}
/* 1 when MatSolve runs the sync-free solves (two launches), 0 for the level-scheduled kernels; *aborted: a dependency wait gave up */
PetscErrorCode PCILUGetSolver_HIPMI355X(PC pc, PetscInt *syncfree, PetscInt *aborted) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  int a = 0, b = 0;
  if (syncfree) *syncfree = (f->syncfree.tri_lo && !f->syncfree.use_levels) ? 1 : 0;
  if (f->syncfree.tri_lo) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    CHKHIP(mi355x_handle_synchronize(dc->h));      /* the flag of everything queued so far */
    mi355x_trisolve_aborted(f->syncfree.tri_lo, &a); mi355x_trisolve_aborted(f->syncfree.tri_up, &b);
  }
  if (aborted) *aborted = a || b || f->aborted;
  return 0;
}
/* Jacobi sweeps per triangular solve (-pc_factor_hipmi355x_trisolve sweeps:<k>); 0: the factor solves exactly */
PetscErrorCode PCILUGetSweeps_HIPMI355X(PC pc, PetscInt *k) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  *k = f->sw.sweeps;
  return 0;
}
/* on_device: the last numeric factorisation ran on the device (-pc_factor_hipmi355x_numeric device); host symbolic passes (pattern,
 * levels, context) and numeric factorisations of this factor so far */
PetscErrorCode PCILUGetNumeric_HIPMI355X(PC pc, PetscInt *on_device, PetscInt *symbolic_builds, PetscInt *numeric_runs) {
  HipTriFactors *f;
  PetscErrorCode ierr;
#if !defined(PETSCHIPMI355X_WITH_PETSC)
  { Mat F = NULL;   /* the block factor of a BAIJ operator (host/bilu.c) keeps the same two counts; it is always factored on the host */
    ierr = PCFactorGetMatrix(pc, &F);CHKERRQ(ierr);
    if (F && F->factortype && F->spptr && HipBlockGet(F)) {
      if (on_device) *on_device = 0;
      if (symbolic_builds) *symbolic_builds = HipBlockGet(F)->symbolic_builds;
      if (numeric_runs) *numeric_runs = HipBlockGet(F)->numeric_runs;
      return 0;
    } }
#endif
  ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (on_device) *on_device = f->dev.dfac ? 1 : 0;
  if (symbolic_builds) *symbolic_builds = f->symbolic_builds;
  if (numeric_runs) *numeric_runs = f->numeric_runs;
  return 0;
}
/* the transposed factor (MatSolveTranspose): builds of its pattern side, and refills of its values on a pattern that was already there */
PetscErrorCode PCILUGetTransposeBuilds_HIPMI355X(PC pc, PetscInt *pattern_builds, PetscInt *value_refreshes) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (pattern_builds) *pattern_builds = f->tr.pattern_builds;
  if (value_refreshes) *value_refreshes = f->tr.value_refreshes;
  return 0;
}
/* ILU(k): the levels of fill of the last factorisation (-pc_factor_levels / PCFactorSetLevels), the stored entries of the factor (L, the
 * diagonal and U) and those of the operator it was made from */
PetscErrorCode PCILUGetFill_HIPMI355X(PC pc, PetscInt *levels, PetscInt *nz_factor, PetscInt *nz_A) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (levels) *levels = f->levels;
  if (nz_factor) *nz_factor = f->nz;
  if (nz_A) *nz_A = f->nzA;
  return 0;
}
/* v <- the factor's application to v, input and result in ONE vector.  PCApply and MatSolve refuse identical vectors as the
 * reference's do (precon.c:380, matrix.c:3205); the sweep form is written to work in place (its iterates live in work vectors)
 * and this is the way to it.  The exact solves are not offered in place. */
PetscErrorCode PCILUApplyInPlace_HIPMI355X(PC pc, Vec v) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (!f->sw.sweeps) SETERRQ(HipObjComm(pc), PETSC_ERR_SUP, "in place only with -pc_factor_hipmi355x_trisolve sweeps:<k>");
  ierr = ilu0_sweeps_apply(f, v, v);CHKERRQ(ierr);
  return 0;
}
/* restarts of the factorisation with a larger diagonal shift (MAT_SHIFT_NONZERO); 0 for every matrix whose pivots pass */
PetscErrorCode PCILUGetShiftCount_HIPMI355X(PC pc, PetscInt *nshift) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  *nshift = f->nshift;
  return 0;
}
/* node-blocked solves: the number of nodes the plans hold (0: row-granular) and the dependency levels over nodes */
PetscErrorCode PCILUGetNodeInfo_HIPMI355X(PC pc, PetscInt *nodes, PetscInt *nlevL, PetscInt *nlevU) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (nodes) *nodes = f->syncfree.nodes ? (f->syncfree.block_columns ? -f->syncfree.nodes : f->syncfree.nodes) : 0;   /* negative: block-column plans */
  if (nlevL) *nlevL = f->syncfree.nlevL_nodes;
  if (nlevU) *nlevU = f->syncfree.nlevU_nodes;
  return 0;
}
/* levels of the two triangular solves */
PetscErrorCode PCILUGetLevels_HIPMI355X(PC pc, PetscInt *nlevL, PetscInt *nlevU) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ILU, &f);CHKERRQ(ierr);
  if (nlevL) *nlevL = f->lev.nlevL;
  if (nlevU) *nlevU = f->lev.nlevU;
  return 0;
}
/* dependency levels of the two sweeps and the number of positive-definite shifts the factorisation took */
PetscErrorCode PCICCGetInfo_HIPMI355X(PC pc, PetscInt *nlevL, PetscInt *nlevU, PetscInt *nshift) {
  HipTriFactors *f;
  PetscErrorCode ierr = pc_factors(pc, MAT_FACTOR_ICC, &f);CHKERRQ(ierr);
  if (nlevL) *nlevL = f->lev.nlevL;
  if (nlevU) *nlevU = f->lev.nlevU;
  if (nshift) *nshift = f->nshift;
  return 0;
}
/* tests: make the next host wait see an aborted sync-free solve on this PC's factor */
PetscErrorCode PCFactorDebugSetAborted_HIPMI355X(PC pc) {
  PetscErrorCode ierr;
  Mat F = NULL;
  ierr = PCFactorGetMatrix(pc, &F);CHKERRQ(ierr);
  if (!F || !HipTriGet(F) || !HipTriGet(F)->syncfree.tri_lo) SETERRQ(HipObjComm(pc), PETSC_ERR_ARG_WRONGSTATE, "no sync-free plans");
  CHKHIP(mi355x_trisolve_debug_set_aborted(HipTriGet(F)->syncfree.tri_lo, 1));
  return 0;
}
