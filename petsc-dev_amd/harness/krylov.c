/* HARNESS file: the Krylov drivers of the test harness (libpetscharness.so), for boxes without PETSc -- what an UNCHANGED PETSc program
 * asks of the plug-in's Vec / Mat types, call by call.  In a PETSc tree this file is NOT used: the reference's own
 * KSPSolve_CG / _GMRES / _BCGS take its place.  It is not part of the product library (libpetschipmi355x.so), links against nothing
 * device-specific and knows no fused kernel; the plug-in's own solvers are separate KSP types (host/kspfused.c).
 *
 * The CONTRACT of every solver below is the reference's sequence of Vec / Mat / PC calls and of convergence checkpoints, nothing else:
 * with the same sequence the iteration counts, the residual histories and (on one rank) the bits are the reference's.  The sequences
 * were read from
 *   CG            src/ksp/ksp/impls/cg/cg.c:92-286        (-ksp_cg_single_reduction: cg.c:116-122,166-169,200-203,263-270)
 *   Gropp CG      src/ksp/ksp/impls/cg/groppcg/groppcg.c:40-175
 *   pipelined CG  src/ksp/ksp/impls/cg/pipecg/pipecg.c:49-205
 *   GMRES(m)      src/ksp/ksp/impls/gmres/gmres.c:118-409, classical Gram-Schmidt src/ksp/ksp/impls/gmres/borthog2.c:35-119
 *   BiCGStab      src/ksp/ksp/impls/bcgs/bcgs.c:43-160
 *   Chebyshev     src/ksp/ksp/impls/cheby/cheby.c (KSPSolve_Chebychev; eigenvalue bounds from the user, no estimation)
 *   Richardson    src/ksp/ksp/impls/rich/rich.c (KSPSolve_Richardson; fixed scale, no self-scaling), PCApplyRichardson precon.c, sor.c
 *   MINRES        src/ksp/ksp/impls/minres/minres.c (KSPSolve_MINRES)
 *   TFQMR         src/ksp/ksp/impls/tfqmr/tfqmr.c (KSPSolve_TFQMR)
 *   CGS           src/ksp/ksp/impls/cgs/cgs.c (KSPSolve_CGS)
 *   BiCG          src/ksp/ksp/impls/bicg/bicg.c (KSPSolve_BiCG)
 *   LSQR          src/ksp/ksp/impls/lsqr/lsqr.c (KSPSolve_LSQR; the contract is the sequence stated in DESIGN.md section 4)
 *   FGMRES(m)     src/ksp/ksp/impls/gmres/fgmres/fgmres.c (the contract is the sequence stated in DESIGN.md section 4, restated without the source)
 * and are written here over a few shared pieces: one checkpoint routine (history, monitor, convergence test), one start-residual
 * routine for the CG family, index-addressed Hessenberg columns for GMRES. */
#include "petscimpl.h"

#define OK(call) do { PetscErrorCode e_ = (call); CHKERRQ(e_); } while (0)
#define FINITE(ksp, v) do { if (PetscIsInfOrNanScalar(v)) SETERRQ((ksp)->comm, PETSC_ERR_FP, "Infinite or not-a-number generated in dot product"); } while (0)

/* ------------------------------------------------------------------ shared pieces */

/* a convergence checkpoint: the norm goes to the history and the monitor, then the test decides ksp->reason */
static PetscErrorCode checkpoint(KSP ksp, PetscInt it, PetscReal rn) {
  ksp->rnorm = rn;
  KSPLogResidualHistory(ksp, rn);
  OK(KSPMonitor(ksp, it, rn));
  return (*ksp->converged)(ksp, it, rn, &ksp->reason, ksp->cnvP);
}

/* the CG family starts from res = rhs - A x, or from a copy of rhs when x is known to be zero */
static PetscErrorCode cg_family_start(KSP ksp, Mat A, Vec x, Vec rhs, Vec res) {
  if (ksp->guess_zero) return VecCopy(rhs, res);
  OK(KSP_MatMult(ksp, A, x, res));
  return VecAYPX(res, -1.0, rhs);
}

/* norm types the CG family accepts, with the priority of the preconditioned one (cg.c:439-442, groppcg.c:170-173, pipecg.c:199-202) */
static void cg_family_norm_table(KSP ksp, PetscInt preconditioned_priority) {
  static const KSPNormType all[] = {KSP_NORM_UNPRECONDITIONED, KSP_NORM_NATURAL, KSP_NORM_NONE};
  for (size_t k = 0; k < sizeof(all) / sizeof(all[0]); k++) ksp->normsupporttable[all[k]][PC_LEFT] = 1;
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = preconditioned_priority;
}

static PetscBool option_is_on(const char *text) { return (PetscBool)(strcmp(text, "0") != 0 && strcmp(text, "false") != 0); }

/* ================================================================== CG
 * Work vectors: res, z = B res, dir; with -ksp_cg_single_reduction two more (Az = A z, Adir), and then A dir and dir' A dir come from
 * recurrences after the first iteration, and z'Az, z'res from ONE VecMDot. */
typedef struct { PetscBool one_reduction; } CgData;
#define CGD(ksp) ((CgData *)(ksp)->data)

static PetscErrorCode KSPSetUp_CG(KSP ksp) { return KSPDefaultGetWork(ksp, CGD(ksp)->one_reduction ? 5 : 3); }   /* cg.c:50-80, no eigenvalue work */
static PetscErrorCode KSPDestroy_CG(KSP ksp) { free(ksp->data); ksp->data = NULL; return 0; }
static PetscErrorCode KSPSetFromOptions_CG(KSP ksp) {   /* cg.c:330-345 */
  char text[16]; PetscBool given;
  OK(PetscOptionsGetString(ksp->prefix, "-ksp_cg_single_reduction", text, sizeof(text), &given));
  if (given) CGD(ksp)->one_reduction = option_is_on(text);
  return 0;
}

/* z <- B res and, in the one-reduction form, Az <- A z right behind it */
static PetscErrorCode cg_precondition(KSP ksp, PetscBool one_red, Mat A, Vec res, Vec z, Vec Az) {
  OK(KSP_PCApply(ksp, res, z));
  if (one_red) OK(KSP_MatMult(ksp, A, z, Az));
  return 0;
}
/* the products the next direction needs: z'res, and z'Az with it in the same reduction when the one-reduction form runs */
static PetscErrorCode cg_products(KSP ksp, PetscBool one_red, Vec z, Vec res, Vec Az, PetscScalar *zAz, PetscScalar *rz) {
  if (one_red) {
    Vec against[2] = {Az, res}; PetscScalar both[2];
    OK(VecMDot(z, 2, against, both));
    *zAz = both[0]; *rz = both[1];
  } else OK(VecTDot(z, res, rz));
  FINITE(ksp, *rz);
  return 0;
}
/* before the first iteration the same two products are two separate dots, the product A z between the norm and them */
static PetscErrorCode cg_first_products(KSP ksp, PetscBool one_red, Mat A, Vec z, Vec res, Vec Az, PetscScalar *zAz, PetscScalar *rz) {
  if (one_red) { OK(KSP_MatMult(ksp, A, z, Az)); OK(VecTDot(z, Az, zAz)); }
  OK(VecTDot(z, res, rz));
  FINITE(ksp, *rz);
  return 0;
}

static PetscErrorCode KSPSolve_CG(KSP ksp) {
  const PetscBool one_red = CGD(ksp)->one_reduction;
  const KSPNormType norm = ksp->normtype;
  const PetscBool norm_has_z = (PetscBool)(norm == KSP_NORM_PRECONDITIONED || norm == KSP_NORM_NATURAL);   /* the norm's own work leaves z = B res behind */
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, res = ksp->work[0], z = ksp->work[1], dir = ksp->work[2];
  Vec Az = one_red ? ksp->work[3] : NULL, Adir = one_red ? ksp->work[4] : z;   /* without the extra vectors A dir borrows z (dead until the next B res) */
  Mat A = ksp->pc->mat;
  PetscScalar rz = 0.0, rz_last = 1.0, pAp = 0.0, pAp_last, zAz = 0.0, step;
  PetscReal rn = 0.0;
  PetscInt k = 0;

  ksp->its = 0;
  OK(cg_family_start(ksp, A, x, rhs, res));
  switch (norm) {                                                   /* iteration 0's checkpoint */
  case KSP_NORM_PRECONDITIONED: OK(KSP_PCApply(ksp, res, z)); OK(VecNorm(z, NORM_2, &rn)); break;
  case KSP_NORM_UNPRECONDITIONED: OK(VecNorm(res, NORM_2, &rn)); break;
  case KSP_NORM_NATURAL:                                             /* sqrt |z'res|: the recurrence's first product serves */
    OK(KSP_PCApply(ksp, res, z));
    OK(cg_first_products(ksp, one_red, A, z, res, Az, &zAz, &rz));
    rn = PetscSqrtReal(PetscAbsScalar(rz));
    break;
  case KSP_NORM_NONE: break;
  default: SETERRQ(ksp->comm, PETSC_ERR_SUP, "norm type %d", (int)norm);
  }
  OK(checkpoint(ksp, 0, rn));
  if (ksp->reason) return 0;
  if (!norm_has_z) OK(KSP_PCApply(ksp, res, z));
  if (norm != KSP_NORM_NATURAL) OK(cg_first_products(ksp, one_red, A, z, res, Az, &zAz, &rz));

  for (;;) {
    ksp->its = k + 1;
    if (rz == 0.0) { ksp->reason = KSP_CONVERGED_ATOL; break; }
    if (k > 0 && rz * rz_last < 0.0) { ksp->reason = KSP_DIVERGED_INDEFINITE_PC; break; }
    if (k == 0) OK(VecCopy(z, dir));
    else OK(VecAYPX(dir, rz / rz_last, z));                         /* dir <- z + (rz / rz_last) dir */
    pAp_last = pAp;
    if (!one_red || k == 0) {
      OK(KSP_MatMult(ksp, A, dir, Adir));
      OK(VecTDot(dir, Adir, &pAp));
    } else {                                                         /* the same two by recurrence */
      OK(VecAYPX(Adir, rz / rz_last, Az));
      pAp = zAz - rz * rz * pAp_last / (rz_last * rz_last);
    }
    rz_last = rz;
    FINITE(ksp, pAp);
    if (pAp == 0.0 || (k > 0 && pAp * pAp_last <= 0.0)) { ksp->reason = KSP_DIVERGED_INDEFINITE_MAT; break; }
    step = rz / pAp;
    OK(VecAXPY(x, step, dir));
    OK(VecAXPY(res, -step, Adir));
    /* this iteration's checkpoint; a norm that needs z produces it (and A z) now, the others after the test */
    if (norm_has_z) OK(cg_precondition(ksp, one_red, A, res, z, Az));
    if (norm == KSP_NORM_PRECONDITIONED) OK(VecNorm(z, NORM_2, &rn));
    else if (norm == KSP_NORM_UNPRECONDITIONED) OK(VecNorm(res, NORM_2, &rn));
    else if (norm == KSP_NORM_NATURAL) { OK(cg_products(ksp, one_red, z, res, Az, &zAz, &rz)); rn = PetscSqrtReal(PetscAbsScalar(rz)); }
    else rn = 0.0;
    OK(checkpoint(ksp, k + 1, rn));
    if (ksp->reason) break;
    if (!norm_has_z) OK(cg_precondition(ksp, one_red, A, res, z, Az));
    if (norm != KSP_NORM_NATURAL) OK(cg_products(ksp, one_red, z, res, Az, &zAz, &rz));
    if (++k >= ksp->max_it) break;
  }
  if (k >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

PetscErrorCode KSPCreate_CG(KSP ksp) {
  CgData *data;
  OK(PetscMalloc(sizeof(*data), &data));
  data->one_reduction = PETSC_FALSE;
  ksp->data = data;
  cg_family_norm_table(ksp, 2);
  ksp->ops->setup = KSPSetUp_CG;
  ksp->ops->solve = KSPSolve_CG;
  ksp->ops->setfromoptions = KSPSetFromOptions_CG;
  ksp->ops->destroy = KSPDestroy_CG;
  return 0;
}

/* ================================================================== Gropp's CG
 * Two reductions per iteration, both split-phase (VecDotBegin / PetscCommSplitReductionBegin / VecDotEnd) with independent work between
 * the halves: dir'Adir travels while B Adir is applied, {the norm, res'z} while A z is formed -- on several GPUs the all-reduce is
 * on the halo stream while the compute stream runs that work.  The preconditioned residual and A z are updated by recurrence, which
 * costs three more vectors than CG (six in all). */
static PetscErrorCode KSPSetUp_GROPPCG(KSP ksp) { return KSPDefaultGetWork(ksp, 6); }

static PetscErrorCode KSPSolve_GROPPCG(KSP ksp) {
  const KSPNormType norm = ksp->normtype;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs;
  Vec res = ksp->work[0], dir = ksp->work[1], Adir = ksp->work[2], BAdir = ksp->work[3], z = ksp->work[4], Az = ksp->work[5];
  Vec normed = norm == KSP_NORM_UNPRECONDITIONED ? res : norm == KSP_NORM_PRECONDITIONED ? z : NULL;   /* whose 2-norm the test sees, if any vector's */
  Mat A = ksp->pc->mat;
  PetscScalar rz, rz_new, pAp, step;
  PetscReal rn = 0.0;
  PetscInt k = 0;

  ksp->its = 0;
  OK(cg_family_start(ksp, A, x, rhs, res));
  OK(KSP_PCApply(ksp, res, z));
  OK(VecCopy(z, dir));
  OK(VecDotBegin(res, z, &rz));                                     /* res'z in flight over Adir <- A dir */
  OK(PetscCommSplitReductionBegin(res->comm));
  OK(KSP_MatMult(ksp, A, dir, Adir));
  OK(VecDotEnd(res, z, &rz));
  if (norm != KSP_NORM_PRECONDITIONED && norm != KSP_NORM_UNPRECONDITIONED && norm != KSP_NORM_NATURAL && norm != KSP_NORM_NONE) SETERRQ(ksp->comm, PETSC_ERR_SUP, "norm type %d", (int)norm);
  if (normed) OK(VecNorm(normed, NORM_2, &rn));
  else if (norm == KSP_NORM_NATURAL) { FINITE(ksp, rz); rn = PetscSqrtReal(PetscAbsScalar(rz)); }
  OK(checkpoint(ksp, 0, rn));
  if (ksp->reason) return 0;

  do {
    ksp->its = ++k;
    OK(VecDotBegin(dir, Adir, &pAp));                               /* dir'Adir in flight over BAdir <- B Adir */
    OK(PetscCommSplitReductionBegin(dir->comm));
    OK(KSP_PCApply(ksp, Adir, BAdir));
    OK(VecDotEnd(dir, Adir, &pAp));
    step = rz / pAp;
    OK(VecAXPY(x, step, dir));
    OK(VecAXPY(res, -step, Adir));
    OK(VecAXPY(z, -step, BAdir));                                   /* z stays B res without another application */
    if (normed) OK(VecNormBegin(normed, NORM_2, &rn));
    OK(VecDotBegin(res, z, &rz_new));                               /* {norm, res'z} in flight over Az <- A z */
    OK(PetscCommSplitReductionBegin(res->comm));
    OK(KSP_MatMult(ksp, A, z, Az));
    if (normed) OK(VecNormEnd(normed, NORM_2, &rn));
    OK(VecDotEnd(res, z, &rz_new));
    if (norm == KSP_NORM_NATURAL) { FINITE(ksp, rz_new); rn = PetscSqrtReal(PetscAbsScalar(rz_new)); }
    else if (norm == KSP_NORM_NONE) rn = 0.0;
    OK(checkpoint(ksp, k, rn));
    if (ksp->reason) break;
    OK(VecAYPX(dir, rz_new / rz, z));
    OK(VecAYPX(Adir, rz_new / rz, Az));                             /* A dir by the same recurrence */
    rz = rz_new;
  } while (k < ksp->max_it);
  if (k >= ksp->max_it && !ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_GROPPCG(KSP ksp) {
  cg_family_norm_table(ksp, 1);
  ksp->ops->setup = KSPSetUp_GROPPCG;
  ksp->ops->solve = KSPSolve_GROPPCG;
  return 0;
}

/* ================================================================== pipelined CG (Ghysels & Vanroose)
 * ONE split-phase reduction per iteration -- {a norm or res'u, w'u} -- in flight over m <- B w and n <- A m; nine work vectors, four
 * of them recurrences of products.  Restated as this snapshot of the reference has it, including which quantity each iteration
 * reduces (pipecg.c:124-131,138-145): with the preconditioned or the unpreconditioned norm res'u is reduced in iteration 0 only and
 * the direction recurrence then runs with ratio 1; the natural norm and KSP_NORM_NONE refresh it every iteration and are the forms
 * that converge like KSPCG. */
static PetscErrorCode KSPSetUp_PIPECG(KSP ksp) { return KSPDefaultGetWork(ksp, 9); }

enum { PIPE_NOTHING, PIPE_NORM, PIPE_RU };                          /* what rides with w'u in an iteration's reduction */

static PetscErrorCode KSPSolve_PIPECG(KSP ksp) {
  const KSPNormType norm = ksp->normtype;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs;
  Vec m = ksp->work[0], ABs_rec = ksp->work[1], dir = ksp->work[2], n = ksp->work[3], w = ksp->work[4];
  Vec Bs_rec = ksp->work[5], u = ksp->work[6], res = ksp->work[7], s = ksp->work[8];
  Vec normed = norm == KSP_NORM_UNPRECONDITIONED ? res : norm == KSP_NORM_PRECONDITIONED ? u : NULL;
  Mat A = ksp->pc->mat;
  PetscScalar step = 0.0, ratio, ru = 0.0, ru_last = 0.0, wu = 0.0;
  PetscReal rn = 0.0;
  PetscInt k = 0;

  ksp->its = 0;
  OK(cg_family_start(ksp, A, x, rhs, res));
  OK(KSP_PCApply(ksp, res, u));
  /* iteration 0's norm, its reduction in flight over w <- A u */
  if (norm != KSP_NORM_PRECONDITIONED && norm != KSP_NORM_UNPRECONDITIONED && norm != KSP_NORM_NATURAL && norm != KSP_NORM_NONE) SETERRQ(ksp->comm, PETSC_ERR_SUP, "norm type %d", (int)norm);
  if (normed) { OK(VecNormBegin(normed, NORM_2, &rn)); OK(PetscCommSplitReductionBegin(normed->comm)); }
  else if (norm == KSP_NORM_NATURAL) { OK(VecDotBegin(res, u, &ru)); OK(PetscCommSplitReductionBegin(res->comm)); }
  OK(KSP_MatMult(ksp, A, u, w));
  if (normed) OK(VecNormEnd(normed, NORM_2, &rn));
  else if (norm == KSP_NORM_NATURAL) { OK(VecDotEnd(res, u, &ru)); FINITE(ksp, ru); rn = PetscSqrtReal(PetscAbsScalar(ru)); }
  OK(checkpoint(ksp, 0, rn));
  if (ksp->reason) return 0;

  do {
    int rides;
    if (k > 0 && normed) rides = PIPE_NORM;
    else if (k == 0 && norm == KSP_NORM_NATURAL) rides = PIPE_NOTHING;   /* res'u is iteration 0's norm already */
    else rides = PIPE_RU;
    if (rides == PIPE_NORM) OK(VecNormBegin(normed, NORM_2, &rn));
    else if (rides == PIPE_RU) OK(VecDotBegin(res, u, &ru));
    OK(VecDotBegin(w, u, &wu));
    OK(PetscCommSplitReductionBegin(res->comm));
    OK(KSP_PCApply(ksp, w, m));                                      /* the work the reduction hides behind */
    OK(KSP_MatMult(ksp, A, m, n));
    if (rides == PIPE_NORM) OK(VecNormEnd(normed, NORM_2, &rn));
    else if (rides == PIPE_RU) OK(VecDotEnd(res, u, &ru));
    OK(VecDotEnd(w, u, &wu));
    if (k > 0) {
      if (norm == KSP_NORM_NATURAL) rn = PetscSqrtReal(PetscAbsScalar(ru));
      else if (norm == KSP_NORM_NONE) rn = 0.0;
      OK(checkpoint(ksp, k, rn));
      if (ksp->reason) break;
      ratio = ru / ru_last;
      step = ru / (wu - ratio / step * ru);
      OK(VecAYPX(ABs_rec, ratio, n));
      OK(VecAYPX(Bs_rec, ratio, m));
      OK(VecAYPX(dir, ratio, u));
      OK(VecAYPX(s, ratio, w));
    } else {
      step = ru / wu;
      OK(VecCopy(n, ABs_rec));
      OK(VecCopy(m, Bs_rec));
      OK(VecCopy(u, dir));
      OK(VecCopy(w, s));
    }
    OK(VecAXPY(x, step, dir));
    OK(VecAXPY(u, -step, Bs_rec));
    OK(VecAXPY(w, -step, ABs_rec));
    OK(VecAXPY(res, -step, s));
    ru_last = ru;
    ksp->its = ++k;
  } while (k < ksp->max_it);
  if (k >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_PIPECG(KSP ksp) {
  cg_family_norm_table(ksp, 1);
  ksp->ops->setup = KSPSetUp_PIPECG;
  ksp->ops->solve = KSPSolve_PIPECG;
  return 0;
}

/* ================================================================== GMRES(m), left or right preconditioning, classical Gram-Schmidt
 * Host state: the rotated Hessenberg matrix, one column per Arnoldi step, column k holding k + 2 numbers at H[k * ld ...]; the Givens
 * pairs; the rotated right-hand side.  Device state: a pool of restart + 4 vectors -- the update, a scratch for the two-step operator,
 * and the basis. */
typedef struct {
  PetscInt restart, ld;
  PetscReal happy_tol;
  KSPGMRESCGSRefinementType refinement;
  PetscScalar *H, *giv_c, *giv_s, *rot_rhs, *coef, *y;
  Vec *pool;
  PetscInt npool, nscratch;           /* vectors of the pool in front of the basis: GMRES 2 (update, scratch), FGMRES 1 (update) */
  /* FGMRES only: the preconditioned directions Z[k] = B_k V[k] and the routine that may change B before every application */
  Vec *Z;
  PetscErrorCode (*modifypc)(KSP, PetscInt, PetscInt, PetscReal, void *);
  void *modifyctx;
  PetscErrorCode (*modifydestroy)(void *);
} GmresData;
#define GMD(ksp) ((GmresData *)(ksp)->data)
#define UPDATE(g) ((g)->pool[0])
#define SCRATCH(g) ((g)->pool[1])
#define BASIS(g) ((g)->pool + (g)->nscratch)

static PetscErrorCode KSPGMRESSetRestart_GMRES(KSP ksp, PetscInt restart) {   /* gmres.c:752-770 */
  if (restart < 1) SETERRQ(ksp->comm, PETSC_ERR_ARG_OUTOFRANGE, "Restart must be positive");
  if (ksp->setupcalled) SETERRQ(ksp->comm, PETSC_ERR_ORDER, "Must call KSPGMRESSetRestart() before KSPSetUp()");
  GMD(ksp)->restart = restart;
  return 0;
}
static PetscErrorCode KSPGMRESSetCGSRefinementType_GMRES(KSP ksp, KSPGMRESCGSRefinementType type) { GMD(ksp)->refinement = type; return 0; }

static PetscErrorCode KSPSetFromOptions_GMRES(KSP ksp) {
  static const struct { const char *name; KSPGMRESCGSRefinementType type; } known[] = {
    {"refine_never", KSP_GMRES_CGS_REFINE_NEVER}, {"refine_ifneeded", KSP_GMRES_CGS_REFINE_IFNEEDED}, {"refine_always", KSP_GMRES_CGS_REFINE_ALWAYS}};
  PetscInt m; PetscBool given; char text[64];
  OK(PetscOptionsGetInt(ksp->prefix, "-ksp_gmres_restart", &m, &given));
  if (given) OK(KSPGMRESSetRestart(ksp, m));
  OK(PetscOptionsGetString(ksp->prefix, "-ksp_gmres_cgs_refinement_type", text, sizeof(text), &given));
  if (given) {
    size_t k = 0;
    while (k < 3 && strcmp(text, known[k].name)) k++;
    if (k == 3) SETERRQ(ksp->comm, PETSC_ERR_ARG_UNKNOWN_TYPE, "Unknown refinement type %s", text);
    GMD(ksp)->refinement = known[k].type;
  }
  return 0;
}

static PetscErrorCode KSPSetUp_GMRES(KSP ksp) {   /* gmres.c:36-96; the whole basis is allocated up front */
  GmresData *g = GMD(ksp);
  const size_t m = (size_t)g->restart;
  PetscScalar *host = (PetscScalar *)calloc((m + 2) * (m + 1) + 5 * (m + 2), sizeof(PetscScalar));   /* one block: H, then five vectors of m + 2 */
  if (!host) SETERRQ(ksp->comm, PETSC_ERR_MEM, "out of memory");
  g->ld = g->restart + 2;
  g->H = host; host += (m + 2) * (m + 1);
  g->giv_c = host; host += m + 2;
  g->giv_s = host; host += m + 2;
  g->rot_rhs = host; host += m + 2;
  g->coef = host; host += m + 2;
  g->y = host;
  g->npool = g->restart + 1 + g->nscratch;
  if (ksp->vec_sol) return VecDuplicateVecs(ksp->vec_sol, g->npool, &g->pool);
  Vec like;
  OK(MatGetVecs(ksp->pc->mat, &like, NULL));
  OK(VecDuplicateVecs(like, g->npool, &g->pool));
  return VecDestroy(&like);
}

/* classical Gram-Schmidt of basis vector k + 1 against 0..k (borthog2.c:35-119): all k + 1 dots in one VecMDot, all subtractions in one
 * VecMAXPY; a second pass always, never, or when the first one cancelled too much (Daniel et al.'s 1 / sqrt 2 criterion in the
 * reference's constant).  Column k of H accumulates the coefficients. */
static PetscErrorCode gmres_orthogonalize(KSP ksp, PetscInt k) {
  GmresData *g = GMD(ksp);
  PetscScalar *h = g->H + (size_t)k * (size_t)g->ld, *coef = g->coef;
  Vec *V = BASIS(g), fresh = V[k + 1];
  PetscBool again = (PetscBool)(g->refinement == KSP_GMRES_CGS_REFINE_ALWAYS);
  for (PetscInt j = 0; j <= k; j++) h[j] = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    OK(VecMDot(fresh, k + 1, V, coef));
    for (PetscInt j = 0; j <= k; j++) coef[j] = -coef[j];
    OK(VecMAXPY(fresh, k + 1, coef, V));
    for (PetscInt j = 0; j <= k; j++) h[j] -= coef[j];
    if (pass == 0 && g->refinement == KSP_GMRES_CGS_REFINE_IFNEEDED) {
      PetscReal removed = 0.0, left;
      for (PetscInt j = 0; j <= k; j++) removed += coef[j] * coef[j];
      removed = PetscSqrtReal(removed);
      OK(VecNorm(fresh, NORM_2, &left));
      if (left < 1.0286 * removed) again = PETSC_TRUE;
    }
    if (!again) break;
  }
  return 0;
}

/* the earlier rotations applied to column k of H, then (unless the happy breakdown ended the cycle) the new one that clears H(k+1, k)
 * (KSPGMRESUpdateHessenberg, gmres.c:360-409); *rn: the residual norm the rotated right-hand side now implies */
static PetscErrorCode gmres_rotate(KSP ksp, PetscInt k, PetscBool happy, PetscReal *rn) {
  GmresData *g = GMD(ksp);
  PetscScalar *h = g->H + (size_t)k * (size_t)g->ld, *c = g->giv_c, *s = g->giv_s, *rhs = g->rot_rhs;
  for (PetscInt j = 0; j < k; j++) {
    const PetscScalar upper = h[j];
    h[j] = c[j] * upper + s[j] * h[j + 1];
    h[j + 1] = c[j] * h[j + 1] - (s[j] * upper);
  }
  if (happy) { *rn = 0.0; return 0; }
  const PetscScalar len = sqrt(h[k] * h[k] + h[k + 1] * h[k + 1]);
  if (len == 0.0) { ksp->reason = KSP_DIVERGED_NULL; return 0; }
  c[k] = h[k] / len;
  s[k] = h[k + 1] / len;
  rhs[k + 1] = -(s[k] * rhs[k]);
  rhs[k] = c[k] * rhs[k];
  h[k] = c[k] * h[k] + s[k] * h[k + 1];
  *rn = PetscAbsScalar(rhs[k + 1]);
  return 0;
}

/* x <- x + [B] V y with R y = rotated right-hand side, R the leading (last + 1)^2 triangle of H (KSPGMRESBuildSoln, gmres.c:309-354) */
static PetscErrorCode gmres_update_solution(KSP ksp, PetscInt last) {
  GmresData *g = GMD(ksp);
  const size_t ld = (size_t)g->ld;
  PetscScalar *y = g->y;
  if (last < 0) return 0;
  for (PetscInt r = last; r >= 0; r--) {
    PetscScalar acc = g->rot_rhs[r];
    for (PetscInt j = r + 1; j <= last; j++) acc = acc - g->H[(size_t)j * ld + r] * y[j];
    if (g->H[(size_t)r * ld + r] == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; return 0; }
    y[r] = acc / g->H[(size_t)r * ld + r];
  }
  OK(VecSet(UPDATE(g), 0.0));
  OK(VecMAXPY(UPDATE(g), last + 1, y, BASIS(g)));
  if (ksp->pc_side == PC_RIGHT) {                                   /* KSPUnwindPreconditioner */
    OK(KSP_PCApply(ksp, UPDATE(g), SCRATCH(g)));
    OK(VecCopy(SCRATCH(g), UPDATE(g)));
  }
  return VecAXPY(ksp->vec_sol, 1.0, UPDATE(g));
}

/* one restart cycle from the residual in basis vector 0 (KSPGMRESCycle, gmres.c:118-209).  The history and the monitor see a step's
 * norm when the NEXT step starts (or when the cycle ends for good), the convergence test sees it at once. */
static PetscErrorCode gmres_cycle(KSP ksp, PetscInt *steps) {
  GmresData *g = GMD(ksp);
  Vec *V = BASIS(g);
  PetscReal rn, beta, hnext, happy_bound;
  PetscBool happy = PETSC_FALSE;
  PetscInt k = 0;

  *steps = 0;
  OK(VecNormalize(V[0], &beta));
  g->rot_rhs[0] = beta;
  ksp->rnorm = rn = beta;
  KSPLogResidualHistory(ksp, rn);
  OK(KSPMonitor(ksp, ksp->its, rn));
  if (!rn) { ksp->reason = KSP_CONVERGED_ATOL; return 0; }
  OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
  while (!ksp->reason && k < g->restart && ksp->its < ksp->max_it) {
    if (k) { KSPLogResidualHistory(ksp, rn); OK(KSPMonitor(ksp, ksp->its, rn)); }
    OK(KSP_PCApplyBAorAB(ksp, V[k], V[k + 1], SCRATCH(g)));
    OK(gmres_orthogonalize(ksp, k));
    OK(VecNormalize(V[k + 1], &hnext));
    g->H[(size_t)k * (size_t)g->ld + k + 1] = hnext;
    happy_bound = PetscAbsScalar(hnext / g->rot_rhs[k]);          /* the happy breakdown: the new vector vanished relative to the residual */
    if (happy_bound > g->happy_tol) happy_bound = g->happy_tol;
    if (hnext < happy_bound) happy = PETSC_TRUE;
    OK(gmres_rotate(ksp, k, happy, &rn));
    k++;
    ksp->its++;
    ksp->rnorm = rn;
    if (ksp->reason) break;
    OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
    if (happy) {
      if (!ksp->reason) SETERRQ(ksp->comm, PETSC_ERR_PLIB, "You reached the happy break down, but convergence was not indicated. Residual norm = %g", rn);
      break;
    }
  }
  if (k && (ksp->reason || ksp->its >= ksp->max_it)) { KSPLogResidualHistory(ksp, rn); OK(KSPMonitor(ksp, ksp->its, rn)); }
  *steps = k;
  return gmres_update_solution(ksp, k - 1);
}

static PetscErrorCode KSPSolve_GMRES(KSP ksp) {   /* gmres.c:213-243: cycles until a reason turns up or the iteration budget is spent */
  GmresData *g = GMD(ksp);
  const PetscBool caller_guess_zero = ksp->guess_zero;
  PetscInt total = 0, steps = 0;
  ksp->its = 0;
  ksp->reason = KSP_CONVERGED_ITERATING;
  while (!ksp->reason) {
    OK(KSPInitialResidual(ksp, ksp->vec_sol, UPDATE(g), SCRATCH(g), BASIS(g)[0], ksp->vec_rhs));
    OK(gmres_cycle(ksp, &steps));
    total += steps;
    if (total >= ksp->max_it) { if (!ksp->reason) ksp->reason = KSP_DIVERGED_ITS; break; }
    ksp->guess_zero = PETSC_FALSE;                                  /* x holds a cycle's update from here on */
  }
  ksp->guess_zero = caller_guess_zero;
  return 0;
}

static PetscErrorCode KSPDestroy_GMRES(KSP ksp) {
  GmresData *g = GMD(ksp);
  if (!g) return 0;
  free(g->H);                                                        /* the one host block */
  if (g->pool) OK(VecDestroyVecs(g->npool, &g->pool));
  free(g);
  ksp->data = NULL;
  (void)PetscObjectComposeFunction((PetscObject)ksp, "KSPGMRESSetRestart_C", "", (PetscVoidFunction)NULL);   /* gmres.c:288-291 */
  (void)PetscObjectComposeFunction((PetscObject)ksp, "KSPGMRESSetCGSRefinementType_C", "", (PetscVoidFunction)NULL);
  return 0;
}

PetscErrorCode KSPCreate_GMRES(KSP ksp) {   /* defaults of the reference's constructor: restart 30, happy-breakdown tolerance 1e-30, no refinement */
  GmresData *g;
  OK(PetscMalloc(sizeof(*g), &g));
  memset(g, 0, sizeof(*g));
  g->restart = 30;
  g->happy_tol = 1.0e-30;
  g->refinement = KSP_GMRES_CGS_REFINE_NEVER;
  g->nscratch = 2;
  ksp->data = g;
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;      /* gmres.c:909-910 */
  ksp->normsupporttable[KSP_NORM_UNPRECONDITIONED][PC_RIGHT] = 1;
  ksp->ops->setup = KSPSetUp_GMRES;
  ksp->ops->solve = KSPSolve_GMRES;
  ksp->ops->destroy = KSPDestroy_GMRES;
  ksp->ops->setfromoptions = KSPSetFromOptions_GMRES;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPGMRESSetRestart_C", "KSPGMRESSetRestart_GMRES", (PetscVoidFunction)KSPGMRESSetRestart_GMRES));   /* gmres.c:931-942 */
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPGMRESSetCGSRefinementType_C", "KSPGMRESSetCGSRefinementType_GMRES", (PetscVoidFunction)KSPGMRESSetCGSRefinementType_GMRES));
  return 0;
}

/* ================================================================== flexible GMRES(m): right preconditioning with a preconditioner that
 * may change from step to step (fgmres.c).  The sequence is the one DESIGN.md section 4 states -- it was restated without the reference's
 * source at hand.  GMRES's state with one scratch vector fewer and, beside the basis V[0..m], the preconditioned directions Z[0..m-1]:
 * Z[k] = B_k V[k] is kept, so the update is x += Z y and nothing is unwound through a preconditioner that may have changed meanwhile.
 * Gram-Schmidt and the rotations are GMRES's own routines; the norm is the true residual's. */
PetscErrorCode KSPFGMRESModifyPCNoChange(KSP ksp, PetscInt total_its, PetscInt loc_its, PetscReal res_norm, void *ctx) {
  (void)ksp; (void)total_its; (void)loc_its; (void)res_norm; (void)ctx;
  return 0;
}
static PetscErrorCode KSPFGMRESSetModifyPC_FGMRES(KSP ksp, PetscErrorCode (*fcn)(KSP, PetscInt, PetscInt, PetscReal, void *), void *ctx, PetscErrorCode (*d)(void *)) {
  GmresData *g = GMD(ksp);
  if (g->modifydestroy) OK((*g->modifydestroy)(g->modifyctx));
  g->modifypc = fcn ? fcn : KSPFGMRESModifyPCNoChange;
  g->modifyctx = ctx;
  g->modifydestroy = d;
  return 0;
}

static PetscErrorCode KSPSetUp_FGMRES(KSP ksp) {   /* V[0..m], Z[0..m-1] and the update vector, all up front */
  GmresData *g = GMD(ksp);
  OK(KSPSetUp_GMRES(ksp));
  return VecDuplicateVecs(UPDATE(g), g->restart, &g->Z);
}

/* V[0] = b - A x: the true residual, nothing preconditioned */
static PetscErrorCode fgmres_residual(KSP ksp) {
  Vec v0 = BASIS(GMD(ksp))[0];
  OK(KSP_MatMult(ksp, ksp->pc->mat, ksp->vec_sol, v0));
  return VecAYPX(v0, -1.0, ksp->vec_rhs);
}

/* x += Z y with R y = rotated right-hand side over the first n columns; a zero last pivot gives y[n-1] = 0 instead of a break-down */
static PetscErrorCode fgmres_update_solution(KSP ksp, PetscInt n) {
  GmresData *g = GMD(ksp);
  const size_t ld = (size_t)g->ld;
  PetscScalar *y = g->y;
  if (n < 1) return 0;
  y[n - 1] = g->H[(size_t)(n - 1) * ld + (size_t)(n - 1)] != 0.0 ? g->rot_rhs[n - 1] / g->H[(size_t)(n - 1) * ld + (size_t)(n - 1)] : 0.0;
  for (PetscInt r = n - 2; r >= 0; r--) {
    PetscScalar acc = g->rot_rhs[r];
    for (PetscInt j = r + 1; j < n; j++) acc = acc - g->H[(size_t)j * ld + r] * y[j];
    y[r] = acc / g->H[(size_t)r * ld + r];
  }
  OK(VecSet(UPDATE(g), 0.0));
  OK(VecMAXPY(UPDATE(g), n, y, g->Z));
  return VecAXPY(ksp->vec_sol, 1.0, UPDATE(g));
}

/* one restart cycle from the residual in V[0].  The history sees a step's norm when the next step starts and once more when the
 * cycle ends; the monitor runs at the head of every step and once after the last one of the solve. */
static PetscErrorCode fgmres_cycle(KSP ksp) {
  GmresData *g = GMD(ksp);
  Vec *V = BASIS(g), *Z = g->Z;
  PetscReal rn, tt, hapbnd;
  PetscBool hapend = PETSC_FALSE;
  PetscInt k = 0;

  OK(VecNorm(V[0], NORM_2, &rn));
  g->rot_rhs[0] = rn;
  ksp->rnorm = rn;
  KSPLogResidualHistory(ksp, rn);
  OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
  if (ksp->reason) return 0;                                         /* no step, no monitor call, x as it is */
  OK(VecScale(V[0], 1.0 / rn));
  while (!ksp->reason && k < g->restart && ksp->its < ksp->max_it) {
    if (k) KSPLogResidualHistory(ksp, rn);
    OK(KSPMonitor(ksp, ksp->its, rn));
    OK((*g->modifypc)(ksp, ksp->its, k, rn, g->modifyctx));
    OK(KSP_PCApply(ksp, V[k], Z[k]));
    OK(KSP_MatMult(ksp, ksp->pc->mat, Z[k], V[k + 1]));
    OK(gmres_orthogonalize(ksp, k));
    OK(VecNorm(V[k + 1], NORM_2, &tt));
    g->H[(size_t)k * (size_t)g->ld + k + 1] = tt;
    hapbnd = PetscAbsScalar(tt / g->rot_rhs[k]);
    if (hapbnd > g->happy_tol) hapbnd = g->happy_tol;
    if (tt > hapbnd) OK(VecScale(V[k + 1], 1.0 / tt));
    else hapend = PETSC_TRUE;
    OK(gmres_rotate(ksp, k, hapend, &rn));
    if (ksp->reason) break;                                          /* a rotation of length 0: the column does not count */
    k++;
    ksp->its++;
    ksp->rnorm = rn;
    OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
    if (hapend) {
      if (!ksp->reason) SETERRQ(ksp->comm, PETSC_ERR_PLIB, "You reached the happy break down, but convergence was not indicated. Residual norm = %g", rn);
      break;
    }
  }
  KSPLogResidualHistory(ksp, rn);
  if (ksp->reason || ksp->its >= ksp->max_it) OK(KSPMonitor(ksp, ksp->its, rn));
  return fgmres_update_solution(ksp, k);
}

static PetscErrorCode KSPSolve_FGMRES(KSP ksp) {
  ksp->its = 0;
  ksp->reason = KSP_CONVERGED_ITERATING;
  if (ksp->guess_zero) OK(VecCopy(ksp->vec_rhs, BASIS(GMD(ksp))[0]));
  else OK(fgmres_residual(ksp));
  OK(fgmres_cycle(ksp));
  while (!ksp->reason) {
    OK(fgmres_residual(ksp));
    if (ksp->its >= ksp->max_it) break;
    OK(fgmres_cycle(ksp));
  }
  if (ksp->its >= ksp->max_it && !ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

static PetscErrorCode KSPDestroy_FGMRES(KSP ksp) {
  GmresData *g = GMD(ksp);
  if (!g) return 0;
  if (g->Z) OK(VecDestroyVecs(g->restart, &g->Z));
  if (g->modifydestroy) OK((*g->modifydestroy)(g->modifyctx));
  (void)PetscObjectComposeFunction((PetscObject)ksp, "KSPFGMRESSetModifyPC_C", "", (PetscVoidFunction)NULL);
  return KSPDestroy_GMRES(ksp);
}

PetscErrorCode KSPCreate_FGMRES(KSP ksp) {   /* GMRES's defaults; right preconditioning only, the norm of the true residual or none */
  OK(KSPCreate_GMRES(ksp));
  GMD(ksp)->nscratch = 1;
  GMD(ksp)->modifypc = KSPFGMRESModifyPCNoChange;
  memset(ksp->normsupporttable, 0, sizeof(ksp->normsupporttable));
  ksp->normsupporttable[KSP_NORM_UNPRECONDITIONED][PC_RIGHT] = 2;
  ksp->normsupporttable[KSP_NORM_NONE][PC_RIGHT] = 1;
  ksp->ops->setup = KSPSetUp_FGMRES;
  ksp->ops->solve = KSPSolve_FGMRES;
  ksp->ops->destroy = KSPDestroy_FGMRES;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPFGMRESSetModifyPC_C", "KSPFGMRESSetModifyPC_FGMRES", (PetscVoidFunction)KSPFGMRESSetModifyPC_FGMRES));
  return 0;
}

/* ================================================================== BiCGStab (left preconditioning)
 * Six work vectors: res, the shadow residual, v = K dir, t = K s, s, dir, with K the preconditioned operator applied in one
 * KSP_PCApplyBAorAB.  KSP_NORM_NONE (smoother use, bcgs.c:76,131) skips the two norms and nothing else. */
static PetscErrorCode KSPSetUp_BCGS(KSP ksp) { return KSPDefaultGetWork(ksp, 6); }   /* bcgs.c:13 */

static PetscErrorCode KSPSolve_BCGS(KSP ksp) {
  const PetscBool want_norm = (PetscBool)(ksp->normtype != KSP_NORM_NONE);
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs;
  Vec res = ksp->work[0], shadow = ksp->work[1], v = ksp->work[2], t = ksp->work[3], s = ksp->work[4], dir = ksp->work[5];
  PetscScalar rho = 0.0, rho_last = 1.0, alpha = 1.0, omega, omega_last = 1.0, beta, dot;
  PetscReal rn = 0.0, tt;
  PetscInt k = 0;

  OK(KSPInitialResidual(ksp, x, v, t, res, rhs));
  if (want_norm) OK(VecNorm(res, NORM_2, &rn));
  ksp->its = 0;
  OK(checkpoint(ksp, 0, rn));
  if (ksp->reason) return 0;
  OK(VecCopy(res, shadow));
  OK(VecSet(dir, 0.0));
  OK(VecSet(v, 0.0));
  do {
    OK(VecDot(res, shadow, &rho));
    beta = (rho / rho_last) * (alpha / omega_last);
    OK(VecAXPBYPCZ(dir, 1.0, -omega_last * beta, beta, res, v));    /* dir <- res + beta (dir - omega v) */
    OK(KSP_PCApplyBAorAB(ksp, dir, v, t));
    OK(VecDot(v, shadow, &dot));
    if (dot == 0.0) SETERRQ(ksp->comm, PETSC_ERR_PLIB, "Divide by zero");
    alpha = rho / dot;
    OK(VecWAXPY(s, -alpha, v, res));
    OK(KSP_PCApplyBAorAB(ksp, s, t, res));                          /* (res is free: s replaced it) */
    OK(VecDotNorm2(s, t, &dot, &tt));                               /* s't and t't in one sweep */
    if (tt == 0.0) {                                                 /* K s vanished: with s = 0 as well, x + alpha dir is the solution */
      OK(VecDot(s, s, &dot));
      if (dot != 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
      OK(VecAXPY(x, alpha, dir));
      ksp->its++;
      ksp->rnorm = 0.0;
      ksp->reason = KSP_CONVERGED_RTOL;
      KSPLogResidualHistory(ksp, rn);                               /* (the reference logs the previous norm here, bcgs.c:118) */
      OK(KSPMonitor(ksp, k + 1, 0.0));
      break;
    }
    omega = dot / tt;
    OK(VecAXPBYPCZ(x, alpha, omega, 1.0, dir, s));
    OK(VecWAXPY(res, -omega, t, s));
    if (want_norm) OK(VecNorm(res, NORM_2, &rn));
    rho_last = rho;
    omega_last = omega;
    ksp->its++;
    OK(checkpoint(ksp, k + 1, rn));
    if (ksp->reason) break;
    if (rho == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }   /* bcgs.c:146 */
  } while (++k < ksp->max_it);
  if (k >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_BCGS(KSP ksp) {   /* bcgs.c:246 (left preconditioning only on this path) */
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->ops->setup = KSPSetUp_BCGS;
  ksp->ops->solve = KSPSolve_BCGS;
  return 0;
}

/* the norms the two stationary-type solvers accept (cheby.c, rich.c KSPCreate_*): preconditioned first, left preconditioning only */
static void stationary_norm_table(KSP ksp) {
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->normsupporttable[KSP_NORM_UNPRECONDITIONED][PC_LEFT] = 1;
}
/* "-name <real>[,<real>]" read as text; returns how many numbers were given */
static PetscErrorCode option_reals(KSP ksp, const char *name, PetscReal v[2], int *count) {
  char text[96], *end; PetscBool given;
  *count = 0;
  OK(PetscOptionsGetString(ksp->prefix, name, text, sizeof(text), &given));
  if (!given) return 0;
  v[0] = strtod(text, &end);
  if (end == text) SETERRQ(ksp->comm, PETSC_ERR_ARG_WRONG, "%s needs a number, got \"%s\"", name, text);
  *count = 1;
  if (*end == ',') { char *second = end + 1; v[1] = strtod(second, &end); if (end != second) *count = 2; }
  return 0;
}

/* ================================================================== Chebyshev (cheby.c KSPSolve_Chebychev), eigenvalue bounds from the user
 * The three-term recurrence over x itself and two work vectors, rotated after every update; a third work vector takes the residual.
 * Without a norm an iteration is one product, one preconditioner application and the update. */
typedef struct { PetscReal emin, emax; } ChebyData;
#define CHD(ksp) ((ChebyData *)(ksp)->data)

static PetscErrorCode KSPChebychevSetEigenvalues_Chebychev(KSP ksp, PetscReal emax, PetscReal emin) {   /* cheby.c:27-39 */
  if (emax <= emin) SETERRQ(ksp->comm, PETSC_ERR_ARG_INCOMP, "Maximum eigenvalue must be larger than minimum: max %g min %g", emax, emin);
  if (emax * emin <= 0.0) SETERRQ(ksp->comm, PETSC_ERR_ARG_INCOMP, "Both eigenvalues must be of the same sign: max %g min %g", emax, emin);
  CHD(ksp)->emax = emax; CHD(ksp)->emin = emin;
  return 0;
}
static PetscErrorCode KSPSetUp_Chebychev(KSP ksp) { return KSPDefaultGetWork(ksp, 3); }
static PetscErrorCode KSPSetFromOptions_Chebychev(KSP ksp) {   /* -ksp_chebychev_eigenvalues <emin,emax> */
  PetscReal v[2]; int count;
  OK(option_reals(ksp, "-ksp_chebychev_eigenvalues", v, &count));
  if (count == 1) SETERRQ(ksp->comm, PETSC_ERR_ARG_INCOMP, "-ksp_chebychev_eigenvalues: must specify 2 parameters, min and max eigenvalues");
  if (count == 2) OK(KSPChebychevSetEigenvalues(ksp, v[1], v[0]));
  return 0;
}
static PetscErrorCode KSPDestroy_Chebychev(KSP ksp) {
  free(ksp->data); ksp->data = NULL;
  (void)PetscObjectComposeFunction((PetscObject)ksp, "KSPChebychevSetEigenvalues_C", "", (PetscVoidFunction)NULL);
  return 0;
}

static PetscErrorCode KSPSolve_Chebychev(KSP ksp) {
  const KSPNormType norm = ksp->normtype;
  const PetscReal emin = CHD(ksp)->emin, emax = CHD(ksp)->emax;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, res = ksp->work[2];
  Vec p[3] = {x, ksp->work[0], ksp->work[1]};
  Mat A = ksp->pc->mat;
  PetscScalar c[3], scale, mu, omegaprod, omega, Gamma = 1.0;
  PetscReal rn = 0.0;
  PetscInt km1 = 0, k = 1, kp1 = 2, i;

  ksp->its = 0;
  scale = 2.0 / (emax + emin);
  mu = 1.0 / (1.0 - scale * emin);
  omegaprod = 2.0 / (1.0 - scale * emin);
  c[km1] = 1.0; c[k] = mu;
  OK(cg_family_start(ksp, A, x, rhs, res));
  OK(KSP_PCApply(ksp, res, p[k]));
  OK(VecAYPX(p[k], scale, x));                                      /* p[k] <- x + scale B res */
  for (i = 0; i < ksp->max_it; i++) {
    ksp->its++;
    c[kp1] = 2.0 * mu * c[k] - c[km1];
    omega = omegaprod * c[k] / c[kp1];
    OK(KSP_MatMult(ksp, A, p[k], res));
    OK(VecAYPX(res, -1.0, rhs));
    OK(KSP_PCApply(ksp, res, p[kp1]));
    if (norm != KSP_NORM_NONE) {                                    /* the checkpoint sees p[k]'s residual; p[kp1] holds B res only */
      OK(VecNorm(norm == KSP_NORM_UNPRECONDITIONED ? res : p[kp1], NORM_2, &rn));
      ksp->vec_sol = p[k];
      OK(checkpoint(ksp, i, rn));
      if (ksp->reason) break;
    }
    OK(VecScale(p[kp1], omega * Gamma * scale));                    /* p[kp1] <- omega Gamma scale B res + (1 - omega) p[km1] + omega p[k] */
    OK(VecAXPY(p[kp1], 1.0 - omega, p[km1]));
    OK(VecAXPY(p[kp1], omega, p[k]));
    { const PetscInt was = km1; km1 = k; k = kp1; kp1 = was; }
  }
  if (!ksp->reason) {
    if (norm != KSP_NORM_NONE) {
      OK(KSP_MatMult(ksp, A, p[k], res));
      OK(VecAYPX(res, -1.0, rhs));
      if (norm == KSP_NORM_UNPRECONDITIONED) OK(VecNorm(res, NORM_2, &rn));
      else { OK(KSP_PCApply(ksp, res, p[kp1])); OK(VecNorm(p[kp1], NORM_2, &rn)); }
      ksp->vec_sol = p[k];
      ksp->rnorm = rn;
      KSPLogResidualHistory(ksp, rn);
      OK(KSPMonitor(ksp, ksp->its, rn));
    }
    if (ksp->its >= ksp->max_it) {
      if (norm != KSP_NORM_NONE) {
        OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
        if (!ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
      } else ksp->reason = KSP_CONVERGED_ITS;
    }
  }
  ksp->vec_sol = x;
  if (p[k] != x) OK(VecCopy(p[k], x));
  return 0;
}
PetscErrorCode KSPCreate_Chebychev(KSP ksp) {   /* cheby.c KSPCreate_Chebychev: emin 1e-2, emax 1e+2 */
  ChebyData *data;
  OK(PetscMalloc(sizeof(*data), &data));
  data->emin = 1.0e-2; data->emax = 1.0e+2;
  ksp->data = data;
  stationary_norm_table(ksp);
  ksp->ops->setup = KSPSetUp_Chebychev;
  ksp->ops->solve = KSPSolve_Chebychev;
  ksp->ops->setfromoptions = KSPSetFromOptions_Chebychev;
  ksp->ops->destroy = KSPDestroy_Chebychev;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPChebychevSetEigenvalues_C", "KSPChebychevSetEigenvalues_Chebychev", (PetscVoidFunction)KSPChebychevSetEigenvalues_Chebychev));
  return 0;
}

/* ================================================================== Richardson (rich.c KSPSolve_Richardson), fixed damping
 * x <- x + scale B (rhs - A x).  A preconditioner that can run the whole iteration itself (PCApplyRichardson: PCSOR) does, when nobody
 * watches the residuals: -pc_type sor then costs ONE MatSOR call of max_it sweeps. */
typedef struct { PetscReal scale; } RichData;
#define RID(ksp) ((RichData *)(ksp)->data)

static PetscErrorCode KSPRichardsonSetScale_Richardson(KSP ksp, PetscReal scale) { RID(ksp)->scale = scale; return 0; }
static PetscErrorCode KSPSetUp_Richardson(KSP ksp) { return KSPDefaultGetWork(ksp, 2); }
static PetscErrorCode KSPSetFromOptions_Richardson(KSP ksp) {   /* -ksp_richardson_scale <s> */
  PetscReal v[2]; int count;
  OK(option_reals(ksp, "-ksp_richardson_scale", v, &count));
  if (count) OK(KSPRichardsonSetScale(ksp, v[0]));
  return 0;
}
static PetscErrorCode KSPDestroy_Richardson(KSP ksp) {
  free(ksp->data); ksp->data = NULL;
  (void)PetscObjectComposeFunction((PetscObject)ksp, "KSPRichardsonSetScale_C", "", (PetscVoidFunction)NULL);
  return 0;
}

static PetscErrorCode KSPSolve_Richardson(KSP ksp) {
  const KSPNormType norm = ksp->normtype;
  const PetscReal scale = RID(ksp)->scale;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, res = ksp->work[0], z = ksp->work[1];
  Mat A = ksp->pc->mat;
  PetscReal rn = 0.0;
  PetscBool whole;
  PetscInt i;

  OK(PCApplyRichardsonExists(ksp->pc, &whole));
  if (whole && !ksp->monitor && !ksp->nullsp) {                     /* rich.c:47-56 */
    PCRichardsonConvergedReason why;
    OK(PCApplyRichardson(ksp->pc, rhs, x, res, ksp->rtol, ksp->abstol, ksp->divtol, ksp->max_it, ksp->guess_zero, &ksp->its, &why));
    ksp->reason = (KSPConvergedReason)why;
    return 0;
  }
  OK(cg_family_start(ksp, A, x, rhs, res));
  ksp->its = 0;
  for (i = 0; i < ksp->max_it; i++) {
    if (norm == KSP_NORM_UNPRECONDITIONED) {
      OK(VecNorm(res, NORM_2, &rn));
      OK(checkpoint(ksp, i, rn));
      if (ksp->reason) break;
    }
    OK(KSP_PCApply(ksp, res, z));
    if (norm == KSP_NORM_PRECONDITIONED) {
      OK(VecNorm(z, NORM_2, &rn));
      OK(checkpoint(ksp, i, rn));
      if (ksp->reason) break;
    }
    OK(VecAXPY(x, scale, z));
    ksp->its++;
    if (i + 1 < ksp->max_it || norm != KSP_NORM_NONE) {
      OK(KSP_MatMult(ksp, A, x, res));
      OK(VecAYPX(res, -1.0, rhs));
    }
  }
  if (!ksp->reason) {
    if (norm != KSP_NORM_NONE) {
      if (norm == KSP_NORM_UNPRECONDITIONED) OK(VecNorm(res, NORM_2, &rn));
      else { OK(KSP_PCApply(ksp, res, z)); OK(VecNorm(z, NORM_2, &rn)); }
      ksp->rnorm = rn;
      KSPLogResidualHistory(ksp, rn);
      OK(KSPMonitor(ksp, ksp->its, rn));
    }
    if (ksp->its >= ksp->max_it) {
      if (norm == KSP_NORM_NONE) ksp->reason = KSP_CONVERGED_ITS;
      else {
        OK((*ksp->converged)(ksp, ksp->its, rn, &ksp->reason, ksp->cnvP));
        if (!ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
      }
    }
  }
  return 0;
}
PetscErrorCode KSPCreate_Richardson(KSP ksp) {   /* rich.c KSPCreate_Richardson: scale 1.0 */
  RichData *data;
  OK(PetscMalloc(sizeof(*data), &data));
  data->scale = 1.0;
  ksp->data = data;
  stationary_norm_table(ksp);
  ksp->ops->setup = KSPSetUp_Richardson;
  ksp->ops->solve = KSPSolve_Richardson;
  ksp->ops->setfromoptions = KSPSetFromOptions_Richardson;
  ksp->ops->destroy = KSPDestroy_Richardson;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPRichardsonSetScale_C", "KSPRichardsonSetScale_Richardson", (PetscVoidFunction)KSPRichardsonSetScale_Richardson));
  return 0;
}

/* ================================================================== MINRES (minres.c KSPSolve_MINRES), symmetric indefinite operators
 * The preconditioned Lanczos recurrence over (R, Z) with the two previous pairs (V, U), (VOLD, UOLD), one Givens rotation per step
 * applied to the last column of the tridiagonal matrix, and the three-term recurrence of the search direction W.  Left preconditioning
 * with the preconditioned norm only; the preconditioner must be positive definite.  The residual norm is the recurrence's estimate
 * rnorm |s|, never recomputed.  dp = r'z below 1e-18 ends the solve (at the start: KSP_DIVERGED_INDEFINITE_MAT; in the loop, before x
 * is updated: KSP_DIVERGED_INDEFINITE_PC) -- also on a lucky breakdown, when the Krylov space is exhausted and x is already exact:
 * the reference does the same. */
static PetscErrorCode KSPSetUp_MINRES(KSP ksp) { return KSPDefaultGetWork(ksp, 9); }

static PetscErrorCode KSPSolve_MINRES(KSP ksp) {
  const PetscReal haptol = 1.e-18;
  Vec X = ksp->vec_sol, B = ksp->vec_rhs;
  Vec R = ksp->work[0], Z = ksp->work[1], U = ksp->work[2], V = ksp->work[3], W = ksp->work[4];
  Vec UOLD = ksp->work[5], VOLD = ksp->work[6], WOLD = ksp->work[7], WOOLD = ksp->work[8];
  Mat A = ksp->pc->mat;
  PetscScalar alpha, beta, betaold, eta, c = 1.0, cold = 1.0, coold, s = 0.0, sold = 0.0, soold, rho0, rho1, rho2, rho3, dp = 0.0;
  PetscReal np;
  PetscInt i;

  ksp->its = 0;
  OK(VecSet(UOLD, 0.0));
  OK(VecCopy(UOLD, VOLD));
  OK(VecCopy(UOLD, W));
  OK(VecCopy(UOLD, WOLD));
  OK(cg_family_start(ksp, A, X, B, R));                             /* R <- B - A X */
  OK(KSP_PCApply(ksp, R, Z));
  OK(VecNorm(Z, NORM_2, &np));
  OK(VecDot(R, Z, &dp));
  if (dp < haptol) { ksp->reason = KSP_DIVERGED_INDEFINITE_MAT; return 0; }
  dp = PetscAbsScalar(dp);
  dp = PetscSqrtReal(dp);
  beta = dp;
  eta = beta;
  OK(VecCopy(R, V));
  OK(VecCopy(Z, U));
  OK(VecScale(V, 1.0 / beta));
  OK(VecScale(U, 1.0 / beta));
  OK(checkpoint(ksp, 0, np));
  if (ksp->reason) return 0;

  for (i = 0; i < ksp->max_it; i++) {
    ksp->its = i + 1;
    /* Lanczos */
    OK(KSP_MatMult(ksp, A, U, R));
    OK(VecDot(U, R, &alpha));
    OK(KSP_PCApply(ksp, R, Z));
    OK(VecAXPY(R, -alpha, V));
    OK(VecAXPY(Z, -alpha, U));
    OK(VecAXPY(R, -beta, VOLD));
    OK(VecAXPY(Z, -beta, UOLD));
    betaold = beta;
    OK(VecDot(R, Z, &dp));
    if (dp < haptol) { ksp->reason = KSP_DIVERGED_INDEFINITE_PC; break; }
    dp = PetscAbsScalar(dp);
    beta = PetscSqrtReal(dp);
    /* QR factorisation */
    coold = cold; cold = c; soold = sold; sold = s;
    rho0 = cold * alpha - coold * sold * betaold;
    rho1 = PetscSqrtReal(rho0 * rho0 + beta * beta);
    rho2 = sold * alpha + coold * cold * betaold;
    rho3 = soold * betaold;
    c = rho0 / rho1;
    s = beta / rho1;
    /* search direction and solution */
    OK(VecCopy(WOLD, WOOLD));
    OK(VecCopy(W, WOLD));
    OK(VecCopy(U, W));
    OK(VecAXPY(W, -rho2, WOLD));
    OK(VecAXPY(W, -rho3, WOOLD));
    OK(VecScale(W, 1.0 / rho1));
    OK(VecAXPY(X, c * eta, W));
    eta = -s * eta;
    OK(VecCopy(V, VOLD));
    OK(VecCopy(U, UOLD));
    OK(VecCopy(R, V));
    OK(VecCopy(Z, U));
    OK(VecScale(V, 1.0 / beta));
    OK(VecScale(U, 1.0 / beta));
    np = ksp->rnorm * PetscAbsScalar(s);
    OK(checkpoint(ksp, i + 1, np));
    if (ksp->reason) break;
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_MINRES(KSP ksp) {   /* minres.c KSPCreate_MINRES */
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->ops->setup = KSPSetUp_MINRES;
  ksp->ops->solve = KSPSolve_MINRES;
  return 0;
}

/* ================================================================== TFQMR (tfqmr.c KSPSolve_TFQMR) and CGS (cgs.c KSPSolve_CGS)
 * The two transpose-free short-recurrence methods for nonsymmetric operators.  They share the CGS recurrence over (R, U, P, Q) with the
 * shadow residual RP and two applications of K = B A per iteration (V = K P, AUQ = K T; AUQ lives in V's buffer).  CGS takes x and the
 * residual norm from the recurrence itself; TFQMR smooths it: two half steps per iteration over the direction D, a residual ESTIMATE
 * sqrt(m + 1) tau per half step (two history entries per iteration), and ksp->its counts the iterations completed, so an exit inside
 * the half steps of iteration i leaves its = i.  Left preconditioning with the preconditioned norm only.
 * s = V'RP == 0 sets KSP_DIVERGED_BREAKDOWN where the reference divides by it. */
enum { TQ_R = 0, TQ_RP, TQ_V, TQ_T, TQ_Q, TQ_P, TQ_U, TQ_T1, TQ_D };
static PetscErrorCode KSPSetUp_TFQMR(KSP ksp) { return KSPDefaultGetWork(ksp, 9); }
static PetscErrorCode KSPSetUp_CGS(KSP ksp) { return KSPDefaultGetWork(ksp, 8); }      /* the same vectors without D */

/* the solve start both share: the residual, the checkpoint of iteration 0, RP, rhoold, U, P and V = K P */
static PetscErrorCode cgs_family_start(KSP ksp, PetscReal *dp, PetscScalar *rhoold) {
  Vec X = ksp->vec_sol, B = ksp->vec_rhs, *w = ksp->work;
  if (ksp->pc_side == PC_RIGHT) SETERRQ(ksp->comm, PETSC_ERR_SUP, "KSP %s does not support right preconditioning", ksp->type_name);
  ksp->its = 0;
  OK(KSPInitialResidual(ksp, X, w[TQ_V], w[TQ_T], w[TQ_R], B));
  OK(VecNorm(w[TQ_R], NORM_2, dp));
  OK(checkpoint(ksp, 0, *dp));
  if (ksp->reason) return 0;
  OK(VecCopy(w[TQ_R], w[TQ_RP]));
  OK(VecDot(w[TQ_R], w[TQ_RP], rhoold));
  OK(VecCopy(w[TQ_R], w[TQ_U]));
  OK(VecCopy(w[TQ_R], w[TQ_P]));
  OK(KSP_PCApplyBAorAB(ksp, w[TQ_P], w[TQ_V], w[TQ_T1]));
  return 0;
}

static PetscErrorCode KSPSolve_TFQMR(KSP ksp) {
  Vec X = ksp->vec_sol, *w = ksp->work;
  Vec R = w[TQ_R], RP = w[TQ_RP], V = w[TQ_V], T = w[TQ_T], Q = w[TQ_Q], P = w[TQ_P], U = w[TQ_U], T1 = w[TQ_T1], D = w[TQ_D], AUQ = V;
  PetscScalar rho, rhoold, a, s, b, eta, etaold = 0.0, psiold = 0.0, cf;
  PetscReal dp, dpold, wt, dpest, tau, psi, cm;
  PetscInt i, m;

  OK(cgs_family_start(ksp, &dp, &rhoold));
  if (ksp->reason) return 0;
  OK(VecSet(D, 0.0));
  tau = dp; dpold = dp;
  for (i = 0; i < ksp->max_it; i++) {
    OK(VecDot(V, RP, &s));
    if (s == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
    a = rhoold / s;
    OK(VecWAXPY(Q, -a, V, U));
    OK(VecWAXPY(T, 1.0, U, Q));
    OK(KSP_PCApplyBAorAB(ksp, T, AUQ, T1));
    OK(VecAXPY(R, -a, AUQ));
    OK(VecNorm(R, NORM_2, &dp));
    for (m = 0; m < 2; m++) {
      wt = m ? dp : PetscSqrtReal(dp * dpold);
      psi = wt / tau;
      cm = 1.0 / PetscSqrtReal(1.0 + psi * psi);
      tau = tau * psi * cm;
      eta = cm * cm * a;
      cf = psiold * psiold * etaold / a;
      OK(VecAYPX(D, cf, m ? Q : U));
      OK(VecAXPY(X, eta, D));
      dpest = PetscSqrtReal(m + 1.0) * tau;
      OK(checkpoint(ksp, i + 1, dpest));
      if (ksp->reason) break;
      etaold = eta;
      psiold = psi;
    }
    if (ksp->reason) break;
    ksp->its = i + 1;
    OK(VecDot(R, RP, &rho));
    b = rho / rhoold;
    OK(VecWAXPY(U, b, Q, R));
    OK(VecAXPY(Q, b, P));
    OK(VecWAXPY(P, b, Q, U));
    OK(KSP_PCApplyBAorAB(ksp, P, V, T1));
    rhoold = rho;
    dpold = dp;
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

static PetscErrorCode KSPSolve_CGS(KSP ksp) {
  Vec X = ksp->vec_sol, *w = ksp->work;
  Vec R = w[TQ_R], RP = w[TQ_RP], V = w[TQ_V], T = w[TQ_T], Q = w[TQ_Q], P = w[TQ_P], U = w[TQ_U], T1 = w[TQ_T1], AUQ = V;
  PetscScalar rho, rhoold, a, s, b;
  PetscReal dp;
  PetscInt i;

  OK(cgs_family_start(ksp, &dp, &rhoold));
  if (ksp->reason) return 0;
  for (i = 0; i < ksp->max_it; i++) {
    OK(VecDot(V, RP, &s));
    if (s == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
    a = rhoold / s;
    OK(VecWAXPY(Q, -a, V, U));
    OK(VecWAXPY(T, 1.0, U, Q));
    OK(VecAXPY(X, a, T));
    OK(KSP_PCApplyBAorAB(ksp, T, AUQ, T1));
    OK(VecAXPY(R, -a, AUQ));
    OK(VecDot(R, RP, &rho));
    OK(VecNorm(R, NORM_2, &dp));
    ksp->its = i + 1;
    OK(checkpoint(ksp, i + 1, dp));
    if (ksp->reason) break;
    b = rho / rhoold;
    OK(VecWAXPY(U, b, Q, R));
    OK(VecAXPY(Q, b, P));
    OK(VecWAXPY(P, b, Q, U));
    OK(KSP_PCApplyBAorAB(ksp, P, V, T1));
    rhoold = rho;
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_TFQMR(KSP ksp) {   /* tfqmr.c KSPCreate_TFQMR */
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->ops->setup = KSPSetUp_TFQMR;
  ksp->ops->solve = KSPSolve_TFQMR;
  return 0;
}
PetscErrorCode KSPCreate_CGS(KSP ksp) {   /* cgs.c KSPCreate_CGS */
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->ops->setup = KSPSetUp_CGS;
  ksp->ops->solve = KSPSolve_CGS;
  return 0;
}

/* ================================================================== BiCG (bicg.c KSPSolve_BiCG)
 * The biconjugate-gradient method: the residual Rr with its directions Pr runs under A and B, the shadow residual Rl with Pl under A^T
 * and B^T (KSP_MatMultTranspose, KSP_PCApplyTranspose).  Work vectors Rr, Rl, Zr, Zl, Pr, Pl; Zr / Zl hold B Rr / B^T Rl between the
 * iterations and A Pr / A^T Pl inside one.  Real scalars: the reference's conjugations are no-ops and are not restated.  Left
 * preconditioning; the preconditioned norm ||B r|| by default, the unpreconditioned one on request -- then the two preconditioner
 * applications follow the checkpoint instead of preceding it.  There is no transposed null-space removal in the reference, so a
 * null space is refused at set-up.  beta == 0 in the first iteration is the reference's breakdown exit; dpi = Zr'Pl == 0 sets
 * KSP_DIVERGED_BREAKDOWN where the reference divides by it. */
enum { BG_RR = 0, BG_RL, BG_ZR, BG_ZL, BG_PR, BG_PL };
static PetscErrorCode KSPSetUp_BICG(KSP ksp) {
  if (ksp->pc_side == PC_RIGHT) SETERRQ(ksp->comm, PETSC_ERR_SUP, "no right preconditioning for KSPBiCG");
  if (ksp->pc_side == PC_SYMMETRIC) SETERRQ(ksp->comm, PETSC_ERR_SUP, "no symmetric preconditioning for KSPBiCG");
  if (ksp->nullsp) SETERRQ(ksp->comm, PETSC_ERR_SUP, "KSPBiCG with a null space: there is no removal behind the transposed preconditioner application");
  return KSPDefaultGetWork(ksp, 6);
}
static PetscErrorCode bicg_precondition(KSP ksp, Vec Rr, Vec Rl, Vec Zr, Vec Zl) {
  OK(KSP_PCApply(ksp, Rr, Zr));
  return KSP_PCApplyTranspose(ksp, Rl, Zl);
}
static PetscErrorCode KSPSolve_BICG(KSP ksp) {
  Vec X = ksp->vec_sol, B = ksp->vec_rhs, *w = ksp->work;
  Vec Rr = w[BG_RR], Rl = w[BG_RL], Zr = w[BG_ZR], Zl = w[BG_ZL], Pr = w[BG_PR], Pl = w[BG_PL];
  Mat A = ksp->pc->mat;
  const PetscBool pnorm = (PetscBool)(ksp->normtype == KSP_NORM_PRECONDITIONED);
  PetscScalar dpi, a, beta, betaold = 1.0;
  PetscReal dp;
  PetscInt i;

  if (ksp->nullsp) SETERRQ(ksp->comm, PETSC_ERR_SUP, "KSPBiCG with a null space: there is no removal behind the transposed preconditioner application");
  ksp->its = 0;
  OK(cg_family_start(ksp, A, X, B, Rr));
  OK(VecCopy(Rr, Rl));
  OK(bicg_precondition(ksp, Rr, Rl, Zr, Zl));
  OK(VecNorm(pnorm ? Zr : Rr, NORM_2, &dp));
  OK(checkpoint(ksp, 0, dp));
  if (ksp->reason) return 0;
  for (i = 0; i < ksp->max_it; i++) {
    OK(VecDot(Zr, Rl, &beta));
    if (!i) {
      if (beta == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; return 0; }
      OK(VecCopy(Zr, Pr));
      OK(VecCopy(Zl, Pl));
    } else {
      const PetscScalar b = beta / betaold;
      OK(VecAYPX(Pr, b, Zr));
      OK(VecAYPX(Pl, b, Zl));
    }
    betaold = beta;
    OK(KSP_MatMult(ksp, A, Pr, Zr));
    OK(KSP_MatMultTranspose(ksp, A, Pl, Zl));
    OK(VecDot(Zr, Pl, &dpi));
    if (dpi == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
    a = beta / dpi;
    OK(VecAXPY(X, a, Pr));
    OK(VecAXPY(Rr, -a, Zr));
    OK(VecAXPY(Rl, -a, Zl));
    if (pnorm) OK(bicg_precondition(ksp, Rr, Rl, Zr, Zl));
    OK(VecNorm(pnorm ? Zr : Rr, NORM_2, &dp));
    ksp->its = i + 1;
    OK(checkpoint(ksp, i + 1, dp));
    if (ksp->reason) break;
    if (!pnorm) OK(bicg_precondition(ksp, Rr, Rl, Zr, Zl));
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_BICG(KSP ksp) {   /* bicg.c KSPCreate_BiCG */
  ksp->normsupporttable[KSP_NORM_PRECONDITIONED][PC_LEFT] = 2;
  ksp->normsupporttable[KSP_NORM_UNPRECONDITIONED][PC_LEFT] = 1;
  ksp->ops->setup = KSPSetUp_BICG;
  ksp->ops->solve = KSPSolve_BICG;
  return 0;
}

/* ================================================================== LSQR (lsqr.c KSPSolve_LSQR), rectangular operators
 * Paige and Saunders' least-squares method: the Golub-Kahan bidiagonalisation of the m x n operator A started from the residual of the
 * guess -- U, U1 in the row space (length m), V, V1 in the column space (length n) -- one Givens rotation per step, the search direction
 * W and the update of x.  min ||b - A x||; for a wide consistent system the minimum-norm solution.  The work vectors come from
 * MatGetVecs(A), never from vec_sol.  A preconditioner acts on the normal equations (its matrix is n x n): Z = B V, alpha = sqrt(V'Z), and
 * Z takes V's place in the product and in W.  The norm is the recurrence's estimate phibar of ||b - A x||; arnorm = alpha |s phi|
 * estimates ||A^T r|| and anorm the Frobenius norm of A (KSPLSQRGetArnorm, KSPLSQRDefaultConverged).  With KSPLSQRSetStandardErrorVec the
 * running sum of (W .* W) / rho^2 is kept.  A null space and a side other than left are refused at set-up.
 * Deviations from the reference: beta == 0 or alpha == 0 in the loop finishes the step -- x takes the update that
 * makes it exact -- and ends with KSP_CONVERGED_HAPPY_BREAKDOWN where the reference leaves with KSP_DIVERGED_BREAKDOWN before the update;
 * alpha == 0 at the start is KSP_CONVERGED_ATOL_NORMAL; the standard-error vector is left as the running sum. */
typedef struct { Vec se; PetscBool se_flg; PetscReal arnorm, anorm, rhs_norm; Vec U, U1, V, V1, W, Z, Z1, W2; } LsqrData;
#define LSQRD(ksp) ((LsqrData *)(ksp)->data)

static PetscBool lsqr_no_pc(KSP ksp) { return (PetscBool)(!strcmp(ksp->pc->type_name, PCNONE)); }
/* the vectors this configuration needs and does not have yet; set-up and solve both ask */
static PetscErrorCode lsqr_get_work(KSP ksp) {
  LsqrData *ld = LSQRD(ksp);
  const PetscBool nopc = lsqr_no_pc(ksp);
  Vec right = NULL, left = NULL;
  Vec *m_side[] = {&ld->U, &ld->U1}, *n_side[] = {&ld->V, &ld->V1, &ld->W, &ld->Z, &ld->Z1, &ld->W2, &ld->se};
  const PetscBool n_needed[] = {PETSC_TRUE, PETSC_TRUE, PETSC_TRUE, (PetscBool)!nopc, (PetscBool)!nopc, (PetscBool)(ld->se || ld->se_flg), ld->se_flg};
  OK(MatGetVecs(ksp->pc->mat, &right, &left));
  for (int k = 0; k < 2; k++) if (!*m_side[k]) OK(VecDuplicate(left, m_side[k]));
  for (int k = 0; k < 7; k++) if (n_needed[k] && !*n_side[k]) OK(VecDuplicate(right, n_side[k]));
  OK(VecDestroy(&right));
  return VecDestroy(&left);
}
static PetscErrorCode lsqr_check(KSP ksp) {
  if (ksp->nullsp) SETERRQ(ksp->comm, PETSC_ERR_SUP, "KSPLSQR with a null space: there is no removal behind the transposed product");
  if (ksp->pc_side == PC_RIGHT || ksp->pc_side == PC_SYMMETRIC) SETERRQ(ksp->comm, PETSC_ERR_SUP, "KSPLSQR: left preconditioning (of the normal equations) only");
  if (!lsqr_no_pc(ksp)) {
    Mat A = ksp->pc->mat, Pm = ksp->pc->pmat;
    if (Pm->rmap->N != A->cmap->N || Pm->cmap->N != A->cmap->N) SETERRQ(ksp->comm, PETSC_ERR_ARG_SIZ, "KSPLSQR preconditions the normal equations: the preconditioner matrix must be %d x %d, it is %d x %d", A->cmap->N, A->cmap->N, Pm->rmap->N, Pm->cmap->N);
  }
  return 0;
}
static PetscErrorCode KSPSetUp_LSQR(KSP ksp) {
  OK(lsqr_check(ksp));
  return lsqr_get_work(ksp);
}
static PetscErrorCode KSPSetFromOptions_LSQR(KSP ksp) {   /* lsqr.c: -ksp_lsqr_set_standard_error */
  char text[16]; PetscBool given;
  OK(PetscOptionsGetString(ksp->prefix, "-ksp_lsqr_set_standard_error", text, sizeof(text), &given));
  if (given) LSQRD(ksp)->se_flg = option_is_on(text);
  return 0;
}
static PetscErrorCode KSPLSQRSetStandardErrorVec_LSQR(KSP ksp, Vec se) {
  LsqrData *ld = LSQRD(ksp);
  if (se == ld->se) return 0;
  OK(VecDestroy(&ld->se));
  ld->se = se;
  return 0;
}
static PetscErrorCode KSPLSQRGetStandardErrorVec_LSQR(KSP ksp, Vec *se) { *se = LSQRD(ksp)->se; return 0; }
static PetscErrorCode KSPLSQRGetArnorm_LSQR(KSP ksp, PetscReal *arnorm, PetscReal *rhs_norm, PetscReal *anorm) {
  *arnorm = LSQRD(ksp)->arnorm; *rhs_norm = LSQRD(ksp)->rhs_norm; *anorm = LSQRD(ksp)->anorm;
  return 0;
}
static PetscErrorCode KSPDestroy_LSQR(KSP ksp) {
  LsqrData *ld = LSQRD(ksp);
  if (!ld) return 0;
  Vec *all[] = {&ld->U, &ld->U1, &ld->V, &ld->V1, &ld->W, &ld->Z, &ld->Z1, &ld->W2, &ld->se};
  for (int k = 0; k < 9; k++) OK(VecDestroy(all[k]));
  free(ld); ksp->data = NULL;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRSetStandardErrorVec_C", "", (PetscVoidFunction)NULL));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRGetStandardErrorVec_C", "", (PetscVoidFunction)NULL));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRGetArnorm_C", "", (PetscVoidFunction)NULL));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPDefaultPCNone_C", "", (PetscVoidFunction)NULL));
  return 0;
}

static PetscErrorCode KSPSolve_LSQR(KSP ksp) {
  LsqrData *ld = LSQRD(ksp);
  Vec X = ksp->vec_sol, B = ksp->vec_rhs, U, U1, V, V1, W, Z, Z1, SE, W2, t;
  Mat A = ksp->pc->mat;
  const PetscBool nopc = lsqr_no_pc(ksp);
  PetscScalar alpha, beta, rho, rhobar, phi, phibar, theta, c, s, dot;
  PetscReal anorm2;
  PetscInt i;

  OK(lsqr_check(ksp));
  OK(lsqr_get_work(ksp));
  U = ld->U; U1 = ld->U1; V = ld->V; V1 = ld->V1; W = ld->W; Z = ld->Z; Z1 = ld->Z1; SE = ld->se; W2 = ld->W2;
  ksp->its = 0;
  OK(cg_family_start(ksp, A, X, B, U));                               /* U <- B - A X: the method iterates on the correction */
  OK(VecNorm(U, NORM_2, &beta));
  ld->rhs_norm = beta; ld->arnorm = 0.0; ld->anorm = 0.0;
  OK(checkpoint(ksp, 0, beta));
  if (ksp->reason) return 0;
  if (beta != 0.0) OK(VecScale(U, 1.0 / beta));
  OK(KSP_MatMultTranspose(ksp, A, U, V));
  if (nopc) OK(VecNorm(V, NORM_2, &alpha));
  else {
    OK(KSP_PCApply(ksp, V, Z));
    OK(VecDot(V, Z, &dot));
    alpha = PetscSqrtReal(dot);
    if (alpha != 0.0) OK(VecScale(Z, 1.0 / alpha));
  }
  if (alpha == 0.0) { ksp->reason = KSP_CONVERGED_ATOL_NORMAL; return 0; }   /* A^T r0 = 0: x already is a least-squares solution */
  OK(VecScale(V, 1.0 / alpha));
  OK(VecCopy(nopc ? V : Z, W));
  if (SE) OK(VecSet(SE, 0.0));
  phibar = beta; rhobar = alpha; anorm2 = alpha * alpha;
  ld->arnorm = alpha * beta; ld->anorm = PetscSqrtReal(anorm2);

  for (i = 0; i < ksp->max_it; i++) {
    PetscBool broke;
    OK(KSP_MatMult(ksp, A, nopc ? V : Z, U1));
    OK(VecAXPY(U1, -alpha, U));
    OK(VecNorm(U1, NORM_2, &beta));
    if (beta != 0.0) OK(VecScale(U1, 1.0 / beta));
    OK(KSP_MatMultTranspose(ksp, A, U1, V1));
    OK(VecAXPY(V1, -beta, V));
    if (nopc) OK(VecNorm(V1, NORM_2, &alpha));
    else {
      OK(KSP_PCApply(ksp, V1, Z1));
      OK(VecDot(V1, Z1, &dot));
      alpha = PetscSqrtReal(dot);
      if (alpha != 0.0) OK(VecScale(Z1, 1.0 / alpha));
    }
    if (alpha != 0.0) OK(VecScale(V1, 1.0 / alpha));
    broke = (PetscBool)(beta == 0.0 || alpha == 0.0);
    rho = PetscSqrtReal(rhobar * rhobar + beta * beta);
    c = rhobar / rho; s = beta / rho;
    theta = s * alpha; rhobar = -c * alpha;
    phi = c * phibar; phibar = s * phibar;
    OK(VecAXPY(X, phi / rho, W));
    if (SE) {
      OK(VecCopy(W, W2));
      OK(VecPointwiseMult(W2, W2, W2));
      OK(VecScale(W2, 1.0 / (rho * rho)));
      OK(VecAXPY(SE, 1.0, W2));
    }
    if (!broke) OK(VecAYPX(W, -theta / rho, nopc ? V1 : Z1));
    ld->arnorm = alpha * PetscAbsScalar(s * phi);
    anorm2 += alpha * alpha + beta * beta;
    ld->anorm = PetscSqrtReal(anorm2);
    ksp->its = i + 1;
    OK(checkpoint(ksp, i + 1, phibar));
    if (broke && !ksp->reason) ksp->reason = KSP_CONVERGED_HAPPY_BREAKDOWN;
    if (ksp->reason) break;
    t = U; U = U1; U1 = t; t = V; V = V1; V1 = t; t = Z; Z = Z1; Z1 = t;
  }
  if (i >= ksp->max_it && !ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
static PetscErrorCode KSPDefaultPCNone_LSQR(KSP ksp) { (void)ksp; return 0; }   /* its presence is the message: see KSPSetUp */
PetscErrorCode KSPCreate_LSQR(KSP ksp) {   /* lsqr.c KSPCreate_LSQR */
  LsqrData *ld = (LsqrData *)calloc(1, sizeof(*ld));
  if (!ld) SETERRQ(ksp->comm, PETSC_ERR_MEM, "out of memory");
  ksp->data = ld;
  ksp->normsupporttable[KSP_NORM_UNPRECONDITIONED][PC_LEFT] = 2;
  ksp->ops->setup = KSPSetUp_LSQR;
  ksp->ops->solve = KSPSolve_LSQR;
  ksp->ops->setfromoptions = KSPSetFromOptions_LSQR;
  ksp->ops->destroy = KSPDestroy_LSQR;
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRSetStandardErrorVec_C", "KSPLSQRSetStandardErrorVec_LSQR", (PetscVoidFunction)KSPLSQRSetStandardErrorVec_LSQR));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRGetStandardErrorVec_C", "KSPLSQRGetStandardErrorVec_LSQR", (PetscVoidFunction)KSPLSQRGetStandardErrorVec_LSQR));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPLSQRGetArnorm_C", "KSPLSQRGetArnorm_LSQR", (PetscVoidFunction)KSPLSQRGetArnorm_LSQR));
  OK(PetscObjectComposeFunction((PetscObject)ksp, "KSPDefaultPCNone_C", "KSPDefaultPCNone_LSQR", (PetscVoidFunction)KSPDefaultPCNone_LSQR));
  return 0;
}
