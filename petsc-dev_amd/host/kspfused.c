/* The plug-in's own Krylov solvers, shipped the way the reference ships a solver: as KSP types registered with KSPRegister
 * (include/petscksp.h:83-123) and selected with -ksp_type:
 *
 *     KSPCGHIPMI355X    "cghipmi355x"      CG        (the recurrence of KSPCG,    src/ksp/ksp/impls/cg/cg.c:92-286)
 *     KSPGMRESHIPMI355X "gmreshipmi355x"   GMRES(m)  (the cycle of KSPGMRES,      src/ksp/ksp/impls/gmres/gmres.c:118-409, borthog2.c:35-119)
 *     KSPBCGSHIPMI355X  "bcgshipmi355x"    BiCGStab  (the recurrence of KSPBCGS,  src/ksp/ksp/impls/bcgs/bcgs.c:43-160)
 *     KSPCHEBYCHEVHIPMI355X  "chebychevhipmi355x"   Chebyshev  (the sequence of KSPCHEBYCHEV,  src/ksp/ksp/impls/cheby/cheby.c)
 *     KSPRICHARDSONHIPMI355X "richardsonhipmi355x"  Richardson (the sequence of KSPRICHARDSON, src/ksp/ksp/impls/rich/rich.c)
 *     KSPPIPECGHIPMI355X     "pipecghipmi355x"      pipelined CG (the sequence of KSPPIPECG, src/ksp/ksp/impls/cg/pipecg/pipecg.c:49-205)
 *     KSPMINRESHIPMI355X     "minreshipmi355x"      MINRES     (the sequence of KSPMINRES,  src/ksp/ksp/impls/minres/minres.c)
 *     KSPTFQMRHIPMI355X      "tfqmrhipmi355x"       TFQMR      (the sequence of KSPTFQMR,   src/ksp/ksp/impls/tfqmr/tfqmr.c)
 *     KSPCGSHIPMI355X        "cgshipmi355x"         CGS        (the sequence of KSPCGS,     src/ksp/ksp/impls/cgs/cgs.c)
 *     KSPBICGHIPMI355X       "bicghipmi355x"        BiCG       (the sequence of KSPBICG,    src/ksp/ksp/impls/bicg/bicg.c)
 *     KSPLSQRHIPMI355X       "lsqrhipmi355x"        LSQR       (the sequence of KSPLSQR,    src/ksp/ksp/impls/lsqr/lsqr.c; rectangular operators)
 *     KSPFGMRESHIPMI355X     "fgmreshipmi355x"      FGMRES(m)  (the cycle of KSPFGMRES,     src/ksp/ksp/impls/gmres/fgmres/fgmres.c; a varying preconditioner)
 *
 * They compute what the reference's solvers compute -- same iterates, same residual history, same exits, bit for bit against
 * the op-by-op sequences (tests/test_host_gpu.py) -- but group the vector work between two reductions into the fused sweeps a
 * Vec / Mat type may offer by name ("VecKrylovFusedOps_C", "MatMultTDotBegin_C", "MatMultDiagonalScale_C";
 * include/petsckrylovfused.h), keep scalars that only the device needs on the device, and queue the front half of the next
 * iteration before the host has looked at the residual norm.  On vectors of a type without those methods every step falls
 * back to the public Vec / Mat / PC calls, so the types work on any PETSc objects -- with THREE exceptions: minreshipmi355x, lsqrhipmi355x (see there) and chebychevhipmi355x.  The
 * three-term Chebyshev update needs VecScale, which is not among the calls this library takes from PETSc, so there is nothing to fall
 * back to: KSPSetUp of that type returns PETSC_ERR_SUP on vectors whose type lacks "cheby_step" and names -ksp_type chebychev.
 *
 * Written against the public API and the KSP implementation header only (petsc-private/kspimpl.h inside a PETSc tree, the
 * harness's petscimpl.h on a box without PETSc): nothing here reaches into a Vec, a Mat or a PC.  An unchanged PETSc program
 * gets these solvers with -ksp_type cghipmi355x etc.; with its own -ksp_type cg it gets PETSc's KSPSolve_CG over the same
 * Vec/Mat ops, one kernel per call.
 *
 * What the types share is written once, and a new type is added by filling it in.  Every type's data struct starts with a KSPHipCommon
 * (the diagonal of a PCJACOBI, the type's -ksp_<type>_fused switch, the two counters KSPHIPMI355XGetFusedStepCounts reports; a type
 * without one of them leaves it at zero) and states the methods it composes on its KSP ONCE, in a static KSPHipMethod table.
 * KSPCreate_* calls ksp_create_data with the struct's size and that table, sets its defaults and its ops; KSPDestroy_* releases what
 * only the type owns and ends in ksp_destroy_data with the same table, so what create composed is what destroy takes away.  The
 * solves themselves share helpers (the tables a Vec type offers, the diagonal form of the PC, K = B A with the dots that follow,
 * the start residual), never a loop: each recurrence is read against its reference. */
#include "hipmi355ximpl.h"

/* ------------------------------------------------------------------------------------------------ what the types offer */
/* fn(x): the table the type of x offers under name, or NULL when it offers none or one without the members `complete` asks of T */
#define VEC_TABLE(fn, Table, name, complete) \
  static const Table *fn(Vec x) { \
    PetscVoidFunction f = NULL; \
    const Table *T; \
    if (PetscObjectQueryFunction((PetscObject)x, name, &f) || !f) return NULL; \
    T = ((const Table *(*)(void))f)(); \
    return (T && (complete)) ? T : NULL; \
  }
VEC_TABLE(vec_fused_ops, VecKrylovFusedOps, "VecKrylovFusedOps_C", PETSC_TRUE)
VEC_TABLE(vec_fgmres_ops, VecFgmresFusedOps, "VecFgmresFusedOps_C", T->fgmres_orthog_normalize_pc)
VEC_TABLE(vec_pipelined_ops, VecPipelinedCGFusedOps, "VecPipelinedCGFusedOps_C", PETSC_TRUE)
VEC_TABLE(vec_split_ops, VecSplitReductionOps, "VecSplitReductionOps_C", PETSC_TRUE)
VEC_TABLE(vec_minres_ops, VecMinresFusedOps, "VecMinresFusedOps_C", T->minres_lanczos && T->minres_update)
VEC_TABLE(vec_tfqmr_ops, VecTfqmrFusedOps, "VecTfqmrFusedOps_C", T->tfqmr_qt && T->tfqmr_resid && T->tfqmr_update)
VEC_TABLE(vec_bicg_ops, VecBicgFusedOps, "VecBicgFusedOps_C", T->bicg_dirs && T->bicg_update)
VEC_TABLE(vec_lsqr_ops, VecLsqrFusedOps, "VecLsqrFusedOps_C", T->lsqr_bidiag && T->lsqr_update)
/* the three types without an op-by-op route (chebychevhipmi355x, minreshipmi355x, lsqrhipmi355x) refuse other vectors at set-up and at solve */
static PetscErrorCode needs_table(KSP ksp, PetscBool offered, const char *type, const char *sweeps, const char *table, const char *plain) {
  if (!offered) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s needs vectors whose type offers the fused %s (\"%s\"); use -ksp_type %s on these vectors", type, sweeps, table, plain);
  return 0;
}
static PetscErrorCode mat_mult_scaled(Mat A, Vec d, Vec x, Vec y, PetscBool *ok) {        /* y = d .* (A x) in one kernel */
  PetscVoidFunction f = NULL;
  PetscErrorCode ierr;
  *ok = PETSC_FALSE;
  ierr = PetscObjectQueryFunction((PetscObject)A, "MatMultDiagonalScale_C", &f);CHKERRQ(ierr);
  if (f) { ierr = ((MatMultDiagonalScaleFn)f)(A, d, x, y, ok);CHKERRQ(ierr); }
  return 0;
}
static PetscErrorCode mat_mult_with_dot(Mat A, Vec x, Vec y, PetscBool *ok) {             /* y = A x, x'y left on the device */
  PetscVoidFunction f = NULL;
  PetscErrorCode ierr;
  *ok = PETSC_FALSE;
  ierr = PetscObjectQueryFunction((PetscObject)A, "MatMultTDotBegin_C", &f);CHKERRQ(ierr);
  if (f) { ierr = ((MatMultTDotBeginFn)f)(A, x, y, ok);CHKERRQ(ierr); }
  return 0;
}
static PetscErrorCode option_level(KSP ksp, const char *name, PetscInt lo, PetscInt hi, PetscInt *level) {   /* "-name <int|true|false>" */
  char t[16]; PetscBool set;
  PetscErrorCode ierr = PetscOptionsGetString(HipObjPrefix(ksp), name, t, sizeof(t), &set);CHKERRQ(ierr);
  if (!set) return 0;
  if (!strcmp(t, "false")) *level = lo;
  else if (!strcmp(t, "true") || !t[0]) *level = hi;
  else { PetscInt v = (PetscInt)atoi(t); *level = v < lo ? lo : (v > hi ? hi : v); }
  return 0;
}
static PetscErrorCode option_bool(KSP ksp, const char *name, PetscBool *flag) {                                /* "-name <bool>", as a level 0..1 */
  PetscInt iv = *flag;
  PetscErrorCode ierr = option_level(ksp, name, 0, 1, &iv);CHKERRQ(ierr);
  *flag = (PetscBool)iv;
  return 0;
}

/* ------------------------------------------------------------------------------------------------ what the types share */
/* the head of every type's data struct: 1 / diagonal of a PCJACOBI (pc_diagonal_form), the -ksp_<type>_fused switch, the two counters of
 * KSPHIPMI355XGetFusedStepCounts.  A type without a switch or without counters leaves them at zero */
typedef struct { Vec dinv; PetscBool fused; PetscInt count[2]; } KSPHipCommon;
#define COMMON(ksp) ((KSPHipCommon *)(ksp)->data)
/* a method a type composes on its KSP; a type's table ends with a NULL name */
typedef struct { const char *name, *fname; PetscVoidFunction fn; } KSPHipMethod;

static PetscErrorCode ksp_compose(KSP ksp, const KSPHipMethod *m, PetscBool on) {
  for (; m && m->name; m++) {
    PetscErrorCode ierr = PetscObjectComposeFunction((PetscObject)ksp, m->name, on ? m->fname : "", on ? m->fn : (PetscVoidFunction)NULL);CHKERRQ(ierr);
  }
  return 0;
}
/* ksp->data: `size` zeroed bytes that start with a KSPHipCommon; the type's methods composed */
static PetscErrorCode ksp_create_data(KSP ksp, size_t size, const KSPHipMethod *methods) {
  void *data;
  PetscErrorCode ierr = PetscMalloc(size, &data);CHKERRQ(ierr);
  memset(data, 0, size);
  ksp->data = data;
  return ksp_compose(ksp, methods, PETSC_TRUE);
}
/* the end of every KSPDestroy_*: the common part and the struct released, the methods of create taken away */
static PetscErrorCode ksp_destroy_data(KSP ksp, const KSPHipMethod *methods) {
  PetscErrorCode ierr;
  if (!ksp->data) return 0;
  ierr = VecDestroy(&COMMON(ksp)->dinv);CHKERRQ(ierr);
  HipFree(ksp->data); ksp->data = NULL;
  return ksp_compose(ksp, methods, PETSC_FALSE);
}
/* the one getter behind KSPHIPMI355XGetFusedStepCounts, composed by the types that count (COUNTS_METHOD in their table); what the two counters mean is the type's (see each type) */
static PetscErrorCode KSPGetFusedStepCounts_Common(KSP ksp, PetscInt *first, PetscInt *second) {
  *first = COMMON(ksp)->count[0]; *second = COMMON(ksp)->count[1];
  return 0;
}
#define COUNTS_METHOD {"KSPHIPMI355XGetFusedStepCounts_C", "KSPGetFusedStepCounts_Common", (PetscVoidFunction)KSPGetFusedStepCounts_Common}
static const KSPHipMethod counts_only[] = {COUNTS_METHOD, {NULL, NULL, NULL}};   /* the types that compose nothing else */
PetscErrorCode KSPHIPMI355XGetFusedStepCounts(KSP ksp, PetscInt *fused, PetscInt *opbyop) {
  PetscVoidFunction f = NULL;
  PetscErrorCode ierr = PetscObjectQueryFunction((PetscObject)ksp, "KSPHIPMI355XGetFusedStepCounts_C", &f);CHKERRQ(ierr);
  *fused = 0; *opbyop = 0;
  if (f) { ierr = ((PetscErrorCode (*)(KSP, PetscInt *, PetscInt *))f)(ksp, fused, opbyop);CHKERRQ(ierr); }
  return 0;
}

/* A null space (KSPSetNullSpace) is projected out of every preconditioned vector by KSP_PCApply / KSP_PCApplyBAorAB (kspimpl.h
 * KSP_RemoveNullSpace).  A sweep that folds the preconditioner into a product or takes the dots of z in the pass that forms z has no
 * place for that projection: with a null space every preconditioner counts as PCKIND_GENERAL and goes through those two calls. */
static PetscBool has_null_space(KSP ksp) { return (PetscBool)(ksp->nullsp != NULL); }   /* kspimpl.h: what KSPGetNullSpace returns */
/* A preconditioner that is a diagonal scaling can ride along in a fused sweep.  Which diagonal: asked of the PC itself through
 * its public face -- PCApply to a vector of ones returns exactly the numbers PCApply_Jacobi multiplies by (1.0 * d is d), for
 * every variant of PCJACOBI (-pc_jacobi_rowmax, ...) and without knowing the PC's data structure.  Every solve opens with this:
 * `wanted` is the solve's own condition for looking at all; not wanted, or a null space: PCKIND_GENERAL, nothing asked of the PC.
 * *d: the diagonal (kept in the common header) of a PCKIND_DIAGONAL, NULL otherwise. */
typedef enum { PCKIND_GENERAL = 0, PCKIND_IDENTITY, PCKIND_DIAGONAL } HipPCKind;
static PetscErrorCode pc_diagonal_form(KSP ksp, PetscBool wanted, Vec like, HipPCKind *kind, Vec *d) {
  PetscErrorCode ierr;
  PCType t = NULL;
  Vec *dinv = &COMMON(ksp)->dinv;
  *kind = PCKIND_GENERAL; *d = NULL;
  if (!wanted || has_null_space(ksp)) return 0;
  ierr = PCGetType(ksp->pc, &t);CHKERRQ(ierr);
  if (t && !strcmp(t, PCNONE)) *kind = PCKIND_IDENTITY;
  else if (t && !strcmp(t, PCJACOBI)) {
    Vec ones;
    if (!*dinv) { ierr = VecDuplicate(like, dinv);CHKERRQ(ierr); }
    ierr = VecDuplicate(like, &ones);CHKERRQ(ierr);
    ierr = VecSet(ones, 1.0);CHKERRQ(ierr);
    ierr = PCApply(ksp->pc, ones, *dinv);CHKERRQ(ierr);
    ierr = VecDestroy(&ones);CHKERRQ(ierr);
    *kind = PCKIND_DIAGONAL; *d = *dinv;
  }
  return 0;
}
#define KSPCheckDot(ksp, v) do { if (PetscIsInfOrNanScalar(v)) SETERRQ(HipObjComm(ksp), PETSC_ERR_FP, "Infinite or not-a-number generated in dot product"); } while (0)
#define KSPTestConvergence(ksp, it, rn) (*(ksp)->converged)((ksp), (it), (rn), &(ksp)->reason, (ksp)->cnvP)
static PetscErrorCode report(KSP ksp, PetscInt it, PetscReal rn) {   /* what every solver does with a new residual norm */
  PetscErrorCode ierr;
  ksp->rnorm = rn;
  KSPLogResidualHistory(ksp, rn);
  ierr = KSPMonitor(ksp, it, rn);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode start_residual(KSP ksp, Mat A, Vec x, Vec rhs, Vec r) {   /* r = rhs - A x; a zero guess: the copy */
  PetscErrorCode ierr;
  if (ksp->guess_zero) { ierr = VecCopy(rhs, r);CHKERRQ(ierr); }
  else { ierr = KSP_MatMult(ksp, A, x, r);CHKERRQ(ierr); ierr = VecAYPX(r, -1.0, rhs);CHKERRQ(ierr); }
  return 0;
}
/* out = K in (K = B A, left preconditioning) and, when the types can, the reduction(s) that follow in the same pass: PCJACOBI on a
 * matrix that offers it: d .* (A in) in the product's own kernel; PCJACOBI / PCNONE otherwise: PCApply fused with the dot(s)
 * ("pmult_dot", "pmult_dotnorm2"); any other PC, a null space, or no table F: KSP_PCApplyBAorAB and the public dots.
 * which = 0: nothing is reduced; which = 1: *s1 = (out, other); which = 2: *s1 = (other, out), *s2 = (out, out).  scratch: a vector for A in. */
static PetscErrorCode apply_operator(KSP ksp, Mat A, const VecKrylovFusedOps *F, HipPCKind pck, Vec d, Vec in, Vec out, Vec scratch, int which, Vec other,
                                     PetscScalar *s1, PetscReal *s2) {
  PetscErrorCode ierr;
  PetscBool done = PETSC_FALSE, scaled = PETSC_FALSE;
  if (F && pck != PCKIND_GENERAL) {
    if (d) { ierr = mat_mult_scaled(A, d, in, out, &scaled);CHKERRQ(ierr); }
    if (!scaled) {
      ierr = KSP_MatMult(ksp, A, in, scratch);CHKERRQ(ierr);
      if (which == 1) { ierr = F->pmult_dot(out, scratch, d, other, s1, &done);CHKERRQ(ierr); }
      else if (which == 2) { ierr = F->pmult_dotnorm2(out, scratch, d, other, s1, s2, &done);CHKERRQ(ierr); }
      if (!done) { ierr = KSP_PCApply(ksp, scratch, out);CHKERRQ(ierr); }
    }
  } else { ierr = KSP_PCApplyBAorAB(ksp, in, out, scratch);CHKERRQ(ierr); }
  if (!done) {
    if (which == 1) { ierr = VecDot(out, other, s1);CHKERRQ(ierr); }
    else if (which == 2) { ierr = VecDotNorm2(other, out, s1, s2);CHKERRQ(ierr); }
  }
  return 0;
}

/* ================================================================================================ CG
 * -ksp_cg_fused <0..4> (default 4); iterates and history carry the same bits at levels 0..3:
 *  0  every step through the public Vec / Mat / PC calls (what KSPCG does);
 *  1  with PCJACOBI or PCNONE the five calls between the two reductions of an iteration -- x += a p, r -= a w, z = B r, |z|,
 *     z'r (cg.c:206-232) -- are ONE sweep returning z'z, z'r and r'r; any other PC: norm and dot share one VecDotNorm2;
 *  2  as 1, and p'w never leaves the device: the sweep forms a = beta / (p'w) itself and applies the reference's break-down
 *     tests before touching anything; p'w comes back with the sums, so the host takes the same exits one kernel later;
 *  3  as 2, and while the host waits for the sums of iteration i the device already runs p = z + b p (b formed on the device),
 *     w = A p and p'w of iteration i+1.  If the convergence test ends the solve only work vectors have been touched.  Not done
 *     for the last permitted iteration nor within 10x of the target;
 *  4  as 3 with p'w produced by the SpMV pass itself (another summation tree: agrees with the other levels to rounding, not bit for
 *     bit; deterministic).  Sequential AIJ matrices whose product kernel leaves per-block sums ("MatMultTDotBegin_C"); level 3 otherwise.
 * -ksp_cg_x_with_p <bool> (default true), levels 3 and 4: when the front half of iteration i+1 is queued, x += a p of iteration i
 * moves from the update sweep into the AYPX that reads p anyway (the same a, the same x + a*p): 12 vector passes per iteration
 * instead of 13, same bits.  Iterations that queue nothing keep x in the update sweep. */
typedef struct { KSPHipCommon common; PetscInt level; PetscBool x_with_p; } KSP_CGHIP;   /* the switch is `level`: common.fused stays unused */

static PetscErrorCode KSPSetUp_CGHIP(KSP ksp) { return KSPDefaultGetWork(ksp, 3); }
static PetscErrorCode KSPSetFromOptions_CGHIP(KSP ksp) {
  KSP_CGHIP *cg = (KSP_CGHIP *)ksp->data;
  PetscErrorCode ierr = option_level(ksp, "-ksp_cg_fused", 0, 4, &cg->level);CHKERRQ(ierr);
  return option_bool(ksp, "-ksp_cg_x_with_p", &cg->x_with_p);
}
static PetscErrorCode KSPDestroy_CGHIP(KSP ksp) { return ksp_destroy_data(ksp, NULL); }

static PetscReal cg_norm_from_sums(KSPNormType nt, PetscScalar zz, PetscScalar zr, PetscScalar rr) {
  switch (nt) {                                          /* the square is reduced, then rooted (pvec2.c:62-64) */
  case KSP_NORM_PRECONDITIONED:   return PetscSqrtReal(zz);
  case KSP_NORM_UNPRECONDITIONED: return PetscSqrtReal(rr);
  case KSP_NORM_NATURAL:          return PetscSqrtReal(PetscAbsScalar(zr));
  default:                        return 0.0;
  }
}

static PetscErrorCode KSPSolve_CGHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_CGHIP *cg = (KSP_CGHIP *)ksp->data;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, r = ksp->work[0], z = ksp->work[1], p = ksp->work[2], w = z;   /* w = A p shares z's storage, as cg.c:122 */
  Mat A;
  const KSPNormType nt = ksp->normtype;
  const VecKrylovFusedOps *F = vec_fused_ops(x);
  const PetscInt level = F ? cg->level : 0;
  HipPCKind pck = PCKIND_GENERAL;
  Vec d = NULL;
  PetscBool sweep = PETSC_FALSE;          /* the one-sweep update is available for these vectors and this PC */
  PetscBool ahead = PETSC_FALSE;          /* p, w = A p and p'w of the coming iteration are already queued */
  PetscScalar pw = 0.0, pw_prev, rz, rz_prev = 1.0, step;
  PetscReal rn = 0.0;
  PetscInt it;

  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(level > 0), x, &pck, &d);CHKERRQ(ierr);   /* with a null space: pck stays general, sweep stays off, every z from KSP_PCApply */
  if (pck != PCKIND_GENERAL) { ierr = F->cg_update_check(x, r, z, p, w, d, &sweep);CHKERRQ(ierr); }
  const PetscBool on_device = (PetscBool)(sweep && level > 1);

  /* ---- residual of the initial guess, its norm in the flavour the test wants, the first z'r ---- */
  ksp->its = 0;
  ierr = start_residual(ksp, A, x, rhs, r);CHKERRQ(ierr);
  if (nt == KSP_NORM_PRECONDITIONED) { ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr); ierr = VecNorm(z, NORM_2, &rn);CHKERRQ(ierr); }
  else if (nt == KSP_NORM_UNPRECONDITIONED) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
  else if (nt == KSP_NORM_NATURAL) {
    ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr);
    ierr = VecTDot(z, r, &rz);CHKERRQ(ierr);
    KSPCheckDot(ksp, rz);
    rn = PetscSqrtReal(PetscAbsScalar(rz));
  } else if (nt != KSP_NORM_NONE) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "norm type %d", (int)nt);
  ierr = report(ksp, 0, rn);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, rn);CHKERRQ(ierr);
  if (ksp->reason) return 0;
  if (nt == KSP_NORM_UNPRECONDITIONED || nt == KSP_NORM_NONE) { ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr); }
  if (nt != KSP_NORM_NATURAL) { ierr = VecTDot(z, r, &rz);CHKERRQ(ierr); KSPCheckDot(ksp, rz); }

  it = 0;
  do {
    PetscBool pw_on_device = PETSC_FALSE, have_sums = PETSC_FALSE;
    PetscScalar zz = 0.0, zr = 0.0, rr = 0.0;
    ksp->its = it + 1;
    if (rz == 0.0) { ksp->reason = KSP_CONVERGED_ATOL; break; }
    if (it > 0 && rz * rz_prev < 0.0) { ksp->reason = KSP_DIVERGED_INDEFINITE_PC; break; }
    pw_prev = pw;
    if (ahead) { pw_on_device = PETSC_TRUE; ahead = PETSC_FALSE; }       /* queued behind the previous sweep */
    else {
      if (it == 0) { ierr = VecCopy(z, p);CHKERRQ(ierr); }                /* p <- z */
      else { ierr = VecAYPX(p, rz / rz_prev, z);CHKERRQ(ierr); }          /* p <- z + b p */
      if (on_device && level > 3) { ierr = mat_mult_with_dot(A, p, w, &pw_on_device);CHKERRQ(ierr); }
      if (!pw_on_device) {
        ierr = KSP_MatMult(ksp, A, p, w);CHKERRQ(ierr);                   /* w <- A p */
        if (on_device) { ierr = F->tdot_begin(p, w, &pw_on_device);CHKERRQ(ierr); }
        if (!pw_on_device) { ierr = VecTDot(p, w, &pw);CHKERRQ(ierr); }
      }
    }
    rz_prev = rz;
    if (pw_on_device) {
      const PetscBool queue = (PetscBool)(level > 2 && it + 1 < ksp->max_it && (nt == KSP_NORM_NONE || rn > 10.0 * ksp->ttol));
      const PetscBool x_in_aypx = (PetscBool)(queue && cg->x_with_p && F->cg_update_dev_begin_nox && F->aypx_dev_x);
      if (x_in_aypx) { ierr = F->cg_update_dev_begin_nox(r, z, w, d, rz, pw_prev, (PetscBool)(it > 0));CHKERRQ(ierr); }
      else { ierr = F->cg_update_dev_begin(x, r, z, p, w, d, rz, pw_prev, (PetscBool)(it > 0));CHKERRQ(ierr); }
      if (queue) {
        PetscBool ok = PETSC_FALSE;                                        /* front half of iteration it+1 */
        if (x_in_aypx) { ierr = F->aypx_dev_x(p, rz, z, x, rz, pw_prev, (PetscBool)(it > 0));CHKERRQ(ierr); }   /* x += a p, then p <- z + b p */
        else { ierr = F->aypx_dev(p, rz, z);CHKERRQ(ierr); }
        if (level > 3) { ierr = mat_mult_with_dot(A, p, w, &ok);CHKERRQ(ierr); }
        if (!ok) {
          ierr = KSP_MatMult(ksp, A, p, w);CHKERRQ(ierr);
          ierr = F->tdot_begin(p, w, &ok);CHKERRQ(ierr);
          if (!ok) SETERRQ(HipObjComm(ksp), PETSC_ERR_PLIB, "split dot refused after it had been accepted");
        }
        ahead = PETSC_TRUE;
      }
      ierr = F->cg_update_dev_end(x, &zz, &zr, &rr, &pw);CHKERRQ(ierr);
      have_sums = PETSC_TRUE;
    }
    KSPCheckDot(ksp, pw);
    if (pw == 0.0 || (it > 0 && pw * pw_prev <= 0.0)) { ksp->reason = KSP_DIVERGED_INDEFINITE_MAT; break; }
    step = rz / pw;
    if (!have_sums && sweep) { ierr = F->cg_update(x, r, z, p, w, d, step, &zz, &zr, &rr, &have_sums);CHKERRQ(ierr); }
    if (have_sums) {
      if (nt == KSP_NORM_NATURAL) KSPCheckDot(ksp, zr);
      rn = cg_norm_from_sums(nt, zz, zr, rr);
    } else {
      ierr = VecAXPY(x, step, p);CHKERRQ(ierr);
      ierr = VecAXPY(r, -step, w);CHKERRQ(ierr);
      if (nt == KSP_NORM_PRECONDITIONED) {
        ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr);
        if (level > 0) { PetscReal n2; ierr = VecDotNorm2(r, z, &zr, &n2);CHKERRQ(ierr); rn = PetscSqrtReal(n2); have_sums = PETSC_TRUE; }
        else { ierr = VecNorm(z, NORM_2, &rn);CHKERRQ(ierr); }
      } else if (nt == KSP_NORM_UNPRECONDITIONED) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
      else if (nt == KSP_NORM_NATURAL) {
        ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr);
        ierr = VecTDot(z, r, &rz);CHKERRQ(ierr);
        KSPCheckDot(ksp, rz);
        rn = PetscSqrtReal(PetscAbsScalar(rz));
      } else rn = 0.0;
    }
    ierr = report(ksp, it + 1, rn);CHKERRQ(ierr);
    ierr = KSPTestConvergence(ksp, it + 1, rn);CHKERRQ(ierr);
    if (ksp->reason) break;
    if (have_sums) rz = zr;
    else {
      if (nt == KSP_NORM_UNPRECONDITIONED || nt == KSP_NORM_NONE) { ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr); }
      if (nt != KSP_NORM_NATURAL) { ierr = VecTDot(z, r, &rz);CHKERRQ(ierr); }
    }
    KSPCheckDot(ksp, rz);
    it++;
  } while (it < ksp->max_it);
  if (it >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

PetscErrorCode KSPCreate_CGHIPMI355X(KSP ksp) {
  KSP_CGHIP *cg;
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(*cg), NULL);CHKERRQ(ierr);
  cg = (KSP_CGHIP *)ksp->data;
  cg->level = 4; cg->x_with_p = PETSC_TRUE;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);    /* the four of KSPCG, cg.c:439-442 */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NATURAL, PC_LEFT, 1);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NONE, PC_LEFT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_CGHIP; ksp->ops->solve = KSPSolve_CGHIP; ksp->ops->setfromoptions = KSPSetFromOptions_CGHIP; ksp->ops->destroy = KSPDestroy_CGHIP;
  return 0;
}

/* ================================================================================================ GMRES(m)
 * -ksp_gmres_fused <bool> (default true).  Left PCJACOBI: the product writes d .* (A v) itself.  Without refinement the
 * Gram-Schmidt step is MDot (coefficients stay on the device) -> ONE sweep w -= V h with |w|^2 -> w *= 1/|w| off the
 * device-resident norm, one host wait instead of three ("gmres_orthog_normalize").  Same bits as the separate calls.
 * Options of KSPGMRES kept: -ksp_gmres_restart, -ksp_gmres_cgs_refinement_type, KSPGMRESSetRestart / SetCGSRefinementType. */
typedef struct {
  KSPHipCommon common;              /* count: fgmreshipmi355x only */
  PetscInt m;                       /* restart length */
  PetscReal haptol;
  KSPGMRESCGSRefinementType refine;
  PetscScalar *H;                   /* Hessenberg matrix after the rotations, column j at H + j (m + 2) */
  PetscScalar *g, *cs, *sn, *coef, *y;   /* rotated right-hand side, rotations, Gram-Schmidt coefficients, triangular solve */
  Vec *V; PetscInt nV, nscr;        /* V[0 .. nscr - 1]: scratch (GMRES 2, FGMRES 1); V[nscr + k]: k-th basis vector */
  /* fgmreshipmi355x only: Z[k] = B_k V[k], the routine that may change B before every application, the form of B */
  PetscBool flexible;
  Vec *Z;
  PetscErrorCode (*modifypc)(KSP, PetscInt, PetscInt, PetscReal, void *);
  void *modifyctx;
  PetscErrorCode (*modifydestroy)(void *);
  HipPCKind pckind;
} KSP_GMRESHIP;
#define GH(ksp) ((KSP_GMRESHIP *)(ksp)->data)
#define Hcol(gm, j) ((gm)->H + (size_t)(j) * (size_t)((gm)->m + 2))
#define BASIS(gm, k) ((gm)->V[(gm)->nscr + (k)])

static PetscErrorCode KSPGMRESSetRestart_GMRESHIP(KSP ksp, PetscInt restart) {
  if (restart < 1) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_OUTOFRANGE, "Restart must be positive");
  if (GH(ksp)->V) SETERRQ(HipObjComm(ksp), PETSC_ERR_ORDER, "Must call KSPGMRESSetRestart() before KSPSetUp()");
  GH(ksp)->m = restart;
  return 0;
}
static PetscErrorCode KSPGMRESSetCGSRefinementType_GMRESHIP(KSP ksp, KSPGMRESCGSRefinementType type) { GH(ksp)->refine = type; return 0; }

static PetscErrorCode KSPSetFromOptions_GMRESHIP(KSP ksp) {
  PetscErrorCode ierr; PetscInt iv; PetscBool set; char t[64];
  ierr = PetscOptionsGetInt(HipObjPrefix(ksp), "-ksp_gmres_restart", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = KSPGMRESSetRestart_GMRESHIP(ksp, iv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetString(HipObjPrefix(ksp), "-ksp_gmres_cgs_refinement_type", t, sizeof(t), &set);CHKERRQ(ierr);
  if (set) {
    if (!strcmp(t, "refine_never")) GH(ksp)->refine = KSP_GMRES_CGS_REFINE_NEVER;
    else if (!strcmp(t, "refine_ifneeded")) GH(ksp)->refine = KSP_GMRES_CGS_REFINE_IFNEEDED;
    else if (!strcmp(t, "refine_always")) GH(ksp)->refine = KSP_GMRES_CGS_REFINE_ALWAYS;
    else SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_UNKNOWN_TYPE, "Unknown refinement type %s", t);
  }
  return option_bool(ksp, GH(ksp)->flexible ? "-ksp_fgmres_fused" : "-ksp_gmres_fused", &COMMON(ksp)->fused);
}

static PetscErrorCode KSPSetUp_GMRESHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  const size_t m = (size_t)gm->m;
  Vec like = ksp->vec_sol, made = NULL;
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2) * (m + 1), &gm->H);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2), &gm->g);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2), &gm->cs);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2), &gm->sn);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2), &gm->coef);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (m + 2), &gm->y);CHKERRQ(ierr);
  memset(gm->H, 0, sizeof(PetscScalar) * (m + 2) * (m + 1));
  memset(gm->g, 0, sizeof(PetscScalar) * (m + 2)); memset(gm->cs, 0, sizeof(PetscScalar) * (m + 2)); memset(gm->sn, 0, sizeof(PetscScalar) * (m + 2));
  if (!like) { Mat A; ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr); ierr = MatGetVecs(A, &made, NULL);CHKERRQ(ierr); like = made; }
  gm->nV = gm->flexible ? gm->m + 2 : gm->m + 4;        /* all basis vectors up front (gmres.c:36-96 allocates them in chunks) */
  ierr = VecDuplicateVecs(like, gm->nV, &gm->V);CHKERRQ(ierr);
  if (gm->flexible) { ierr = VecDuplicateVecs(like, gm->m, &gm->Z);CHKERRQ(ierr); }
  if (made) { ierr = VecDestroy(&made);CHKERRQ(ierr); }
  return 0;
}

/* classical Gram-Schmidt against BASIS(0..k) through the public calls (borthog2.c:35-119), optionally twice */
static PetscErrorCode gmres_orthogonalize(KSP ksp, PetscInt k, PetscScalar *hcol) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  PetscScalar *c = gm->coef;
  Vec w = BASIS(gm, k + 1);
  PetscBool again = (PetscBool)(gm->refine == KSP_GMRES_CGS_REFINE_ALWAYS);
  for (PetscInt j = 0; j <= k; j++) hcol[j] = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    ierr = VecMDot(w, k + 1, &BASIS(gm, 0), c);CHKERRQ(ierr);
    for (PetscInt j = 0; j <= k; j++) c[j] = -c[j];
    ierr = VecMAXPY(w, k + 1, c, &BASIS(gm, 0));CHKERRQ(ierr);
    for (PetscInt j = 0; j <= k; j++) hcol[j] -= c[j];
    if (pass == 0 && gm->refine == KSP_GMRES_CGS_REFINE_IFNEEDED) {          /* borthog2.c:77-98 */
      PetscReal hn = 0.0, wn;
      for (PetscInt j = 0; j <= k; j++) hn += c[j] * c[j];
      hn = PetscSqrtReal(hn);
      ierr = VecNorm(w, NORM_2, &wn);CHKERRQ(ierr);
      if (wn < 1.0286 * hn) again = PETSC_TRUE;
    }
    if (!again) break;
  }
  return 0;
}

/* apply the k earlier rotations to column k, then the new one that annihilates H(k+1,k) (gmres.c:360-409) */
static void gmres_rotate(KSP ksp, PetscInt k, PetscBool happy, PetscReal *res) {
  KSP_GMRESHIP *gm = GH(ksp);
  PetscScalar *h = Hcol(gm, k);
  for (PetscInt j = 0; j < k; j++) {
    const PetscScalar t = h[j];
    h[j] = gm->cs[j] * t + gm->sn[j] * h[j + 1];
    h[j + 1] = gm->cs[j] * h[j + 1] - gm->sn[j] * t;
  }
  if (happy) { *res = 0.0; return; }
  const PetscScalar t = PetscSqrtReal(h[k] * h[k] + h[k + 1] * h[k + 1]);
  if (t == 0.0) { ksp->reason = KSP_DIVERGED_NULL; return; }
  gm->cs[k] = h[k] / t;
  gm->sn[k] = h[k + 1] / t;
  gm->g[k + 1] = -(gm->sn[k] * gm->g[k]);
  gm->g[k] = gm->cs[k] * gm->g[k];
  h[k] = gm->cs[k] * h[k] + gm->sn[k] * h[k + 1];
  *res = PetscAbsScalar(gm->g[k + 1]);
}

/* x += [M^-1] V y with R y = g over the first n columns (gmres.c:309-354) */
static PetscErrorCode gmres_update_solution(KSP ksp, PetscInt n) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  PetscScalar *y = gm->y;
  if (n < 1) return 0;
  for (PetscInt k = n - 1; k >= 0; k--) {
    PetscScalar t = gm->g[k];
    for (PetscInt j = k + 1; j < n; j++) t = t - Hcol(gm, j)[k] * y[j];
    if (Hcol(gm, k)[k] == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; return 0; }
    y[k] = t / Hcol(gm, k)[k];
  }
  ierr = VecSet(gm->V[0], 0.0);CHKERRQ(ierr);
  ierr = VecMAXPY(gm->V[0], n, y, &BASIS(gm, 0));CHKERRQ(ierr);
  if (ksp->pc_side == PC_RIGHT) {                                   /* KSPUnwindPreconditioner */
    ierr = KSP_PCApply(ksp, gm->V[0], gm->V[1]);CHKERRQ(ierr);
    ierr = VecCopy(gm->V[1], gm->V[0]);CHKERRQ(ierr);
  }
  ierr = VecAXPY(ksp->vec_sol, 1.0, gm->V[0]);CHKERRQ(ierr);
  return 0;
}

/* one restart cycle starting from the residual in BASIS(0) */
static PetscErrorCode gmres_cycle(KSP ksp, PetscInt *steps) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  const VecKrylovFusedOps *F = gm->common.fused ? vec_fused_ops(BASIS(gm, 0)) : NULL;
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscReal res, wnorm;
  PetscInt k = 0;
  PetscBool happy = PETSC_FALSE, done;

  if (F && !F->gmres_orthog_normalize) F = NULL;
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(gm->common.fused && ksp->pc_side == PC_LEFT), BASIS(gm, 0), &pck, &d);CHKERRQ(ierr);
  ierr = VecNormalize(BASIS(gm, 0), &res);CHKERRQ(ierr);
  gm->g[0] = res;
  ierr = report(ksp, ksp->its, res);CHKERRQ(ierr);
  *steps = 0;
  if (!res) { ksp->reason = KSP_CONVERGED_ATOL; return 0; }
  ierr = KSPTestConvergence(ksp, ksp->its, res);CHKERRQ(ierr);
  while (!ksp->reason && k < gm->m && ksp->its < ksp->max_it) {
    PetscScalar *hcol = Hcol(gm, k);
    if (k) { ierr = report(ksp, ksp->its, res);CHKERRQ(ierr); }
    done = PETSC_FALSE;                                                        /* BASIS(k+1) = [M^-1] A [M^-1] BASIS(k) */
    if (d) { ierr = mat_mult_scaled(A, d, BASIS(gm, k), BASIS(gm, k + 1), &done);CHKERRQ(ierr); }
    if (!done) { ierr = KSP_PCApplyBAorAB(ksp, BASIS(gm, k), BASIS(gm, k + 1), gm->V[1]);CHKERRQ(ierr); }
    done = PETSC_FALSE;
    if (F && gm->refine == KSP_GMRES_CGS_REFINE_NEVER) {
      ierr = F->gmres_orthog_normalize(BASIS(gm, k + 1), k + 1, &BASIS(gm, 0), gm->coef, &wnorm, &done);CHKERRQ(ierr);
      if (done) for (PetscInt j = 0; j <= k; j++) { const PetscScalar c = -gm->coef[j]; hcol[j] = 0.0; hcol[j] -= c; }   /* borthog2.c:52-66 */
    }
    if (!done) {
      ierr = gmres_orthogonalize(ksp, k, hcol);CHKERRQ(ierr);
      ierr = VecNormalize(BASIS(gm, k + 1), &wnorm);CHKERRQ(ierr);
    }
    hcol[k + 1] = wnorm;
    {                                                                          /* happy breakdown test (gmres.c:171-178) */
      PetscReal bound = PetscAbsScalar(wnorm / gm->g[k]);
      if (bound > gm->haptol) bound = gm->haptol;
      if (wnorm < bound) happy = PETSC_TRUE;
    }
    gmres_rotate(ksp, k, happy, &res);
    k++;
    ksp->its++;
    ksp->rnorm = res;
    if (ksp->reason) break;
    ierr = KSPTestConvergence(ksp, ksp->its, res);CHKERRQ(ierr);
    if (happy) {
      if (!ksp->reason) SETERRQ(HipObjComm(ksp), PETSC_ERR_PLIB, "You reached the happy break down, but convergence was not indicated. Residual norm = %g", (double)res);
      break;
    }
  }
  if (k && (ksp->reason || ksp->its >= ksp->max_it)) { ierr = report(ksp, ksp->its, res);CHKERRQ(ierr); }
  *steps = k;
  ierr = gmres_update_solution(ksp, k);CHKERRQ(ierr);
  return 0;
}

static PetscErrorCode KSPSolve_GMRESHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  const PetscBool guess_zero = ksp->guess_zero;
  PetscInt total = 0, steps = 0;
  ksp->its = 0;
  ksp->reason = KSP_CONVERGED_ITERATING;
  while (!ksp->reason) {
    ierr = KSPInitialResidual(ksp, ksp->vec_sol, gm->V[0], gm->V[1], BASIS(gm, 0), ksp->vec_rhs);CHKERRQ(ierr);
    ierr = gmres_cycle(ksp, &steps);CHKERRQ(ierr);
    total += steps;
    if (total >= ksp->max_it) { if (!ksp->reason) ksp->reason = KSP_DIVERGED_ITS; break; }
    ksp->guess_zero = PETSC_FALSE;                    /* the next cycle starts from the iterate (gmres.c:236) */
  }
  ksp->guess_zero = guess_zero;
  return 0;
}

static const KSPHipMethod gmres_methods[] = {
  {"KSPGMRESSetRestart_C", "KSPGMRESSetRestart_GMRESHIP", (PetscVoidFunction)KSPGMRESSetRestart_GMRESHIP},
  {"KSPGMRESSetCGSRefinementType_C", "KSPGMRESSetCGSRefinementType_GMRESHIP", (PetscVoidFunction)KSPGMRESSetCGSRefinementType_GMRESHIP},
  {NULL, NULL, NULL}};
static PetscErrorCode KSPDestroy_GMRESHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  if (!gm) return 0;
  HipFree(gm->H); HipFree(gm->g); HipFree(gm->cs); HipFree(gm->sn); HipFree(gm->coef); HipFree(gm->y);
  if (gm->V) { ierr = VecDestroyVecs(gm->nV, &gm->V);CHKERRQ(ierr); }
  if (gm->Z) { ierr = VecDestroyVecs(gm->m, &gm->Z);CHKERRQ(ierr); }
  if (gm->modifydestroy) { ierr = (*gm->modifydestroy)(gm->modifyctx);CHKERRQ(ierr); }
  return ksp_destroy_data(ksp, gmres_methods);
}

PetscErrorCode KSPCreate_GMRESHIPMI355X(KSP ksp) {
  KSP_GMRESHIP *gm;
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(*gm), gmres_methods);CHKERRQ(ierr);
  gm = GH(ksp);
  gm->m = 30; gm->haptol = 1.0e-30; gm->refine = KSP_GMRES_CGS_REFINE_NEVER; gm->common.fused = PETSC_TRUE;   /* KSPGMRES's defaults, gmres.c:944-958 */
  gm->nscr = 2;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);       /* gmres.c:909-910 */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_RIGHT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_GMRESHIP; ksp->ops->solve = KSPSolve_GMRESHIP; ksp->ops->setfromoptions = KSPSetFromOptions_GMRESHIP; ksp->ops->destroy = KSPDestroy_GMRESHIP;
  return 0;
}

/* ================================================================================================ flexible GMRES(m)
 * The cycle of KSPFGMRES (fgmres.c; the sequence DESIGN.md section 4 states): right preconditioning with a preconditioner that may
 * differ from step to step, Z[k] = B_k V[k] kept, x += Z y.  GMRES's state, Gram-Schmidt and rotations above are shared.
 * Without refinement the Gram-Schmidt step is "gmres_orthog_normalize": one host wait per step with ANY preconditioner, PCKSP included.
 * -ksp_fgmres_fused <bool> (default false: measured no faster, profiles/fgmres_rate.log): with PCNONE or PCJACOBI, no null space, no KSPFGMRESSetModifyPC routine and at most 32
 * basis vectors the normalising sweep of step k also writes Z[k+1] = B V[k+1] ("fgmres_orthog_normalize_pc" of "VecFgmresFusedOps_C"),
 * and step k + 1 skips its KSP_PCApply: 2 nv + 7 vector passes instead of 2 nv + 8 with Jacobi, one launch fewer, same bits.  The
 * last step of a restart cycle has no Z[m] to write and takes the plain call.  After a happy breakdown V[k+1] and Z[k+1] are
 * unspecified (the sweep scales what the reference leaves unscaled); x, the history, the iteration count and the reason are not.
 * The start of a cycle normalises with VecNormalize: this library takes a fixed list of calls from PETSc (tests/test_host_cpu.py keeps
 * it; VecScale is not on it, see the Chebyshev type above).  VecNormalize leaves a zero residual alone where VecScale(1 / 0) would fill
 * the work vector with NaN: only seen with KSP_NORM_NONE, where no test stops the cycle.
 * KSPHIPMI355XGetFusedStepCounts: (steps that wrote the next Z in the sweep, all other steps), summed over all solves since the type was set.  On vectors without the tables every
 * step runs through the public calls.  Options of KSPGMRES kept: -ksp_gmres_restart, -ksp_gmres_cgs_refinement_type. */
static PetscErrorCode KSPFGMRESSetModifyPC_FGMRESHIP(KSP ksp, PetscErrorCode (*fcn)(KSP, PetscInt, PetscInt, PetscReal, void *), void *ctx, PetscErrorCode (*d)(void *)) {
  KSP_GMRESHIP *gm = GH(ksp);
  if (gm->modifydestroy) { PetscErrorCode ierr = (*gm->modifydestroy)(gm->modifyctx);CHKERRQ(ierr); }
  gm->modifypc = fcn; gm->modifyctx = ctx; gm->modifydestroy = d;          /* NULL: the preconditioner is left alone (KSPFGMRESModifyPCNoChange) */
  return 0;
}

static PetscErrorCode fgmres_residual(KSP ksp) {                        /* V[0] = b - A x, the true residual */
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  Mat A;
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = KSP_MatMult(ksp, A, ksp->vec_sol, BASIS(gm, 0));CHKERRQ(ierr);
  ierr = VecAYPX(BASIS(gm, 0), -1.0, ksp->vec_rhs);CHKERRQ(ierr);
  return 0;
}

/* x += Z y with R y = g over the first n columns; a zero last pivot gives y[n-1] = 0, not a break-down */
static PetscErrorCode fgmres_update_solution(KSP ksp, PetscInt n) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  PetscScalar *y = gm->y;
  if (n < 1) return 0;
  y[n - 1] = Hcol(gm, n - 1)[n - 1] != 0.0 ? gm->g[n - 1] / Hcol(gm, n - 1)[n - 1] : 0.0;
  for (PetscInt k = n - 2; k >= 0; k--) {
    PetscScalar t = gm->g[k];
    for (PetscInt j = k + 1; j < n; j++) t = t - Hcol(gm, j)[k] * y[j];
    y[k] = t / Hcol(gm, k)[k];
  }
  ierr = VecSet(gm->V[0], 0.0);CHKERRQ(ierr);
  ierr = VecMAXPY(gm->V[0], n, y, gm->Z);CHKERRQ(ierr);
  ierr = VecAXPY(ksp->vec_sol, 1.0, gm->V[0]);CHKERRQ(ierr);
  return 0;
}

static PetscErrorCode fgmres_cycle(KSP ksp) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  const VecKrylovFusedOps *F = vec_fused_ops(BASIS(gm, 0));
  const VecFgmresFusedOps *P = (gm->common.fused && gm->pckind != PCKIND_GENERAL) ? vec_fgmres_ops(BASIS(gm, 0)) : NULL;
  Mat A;
  PetscReal res, tt, hapbnd;
  PetscInt k = 0;
  PetscBool hapend = PETSC_FALSE, have_z = PETSC_FALSE, done;

  if (F && !F->gmres_orthog_normalize) F = NULL;
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = VecNormalize(BASIS(gm, 0), &res);CHKERRQ(ierr);
  gm->g[0] = res;
  ksp->rnorm = res;
  KSPLogResidualHistory(ksp, res);
  ierr = KSPTestConvergence(ksp, ksp->its, res);CHKERRQ(ierr);
  if (ksp->reason) return 0;                                             /* no step, no monitor call, x as it is */
  while (!ksp->reason && k < gm->m && ksp->its < ksp->max_it) {
    PetscScalar *hcol = Hcol(gm, k);
    if (k) KSPLogResidualHistory(ksp, res);
    ierr = KSPMonitor(ksp, ksp->its, res);CHKERRQ(ierr);
    if (gm->modifypc) { ierr = (*gm->modifypc)(ksp, ksp->its, k, res, gm->modifyctx);CHKERRQ(ierr); }
    if (!have_z) { ierr = KSP_PCApply(ksp, BASIS(gm, k), gm->Z[k]);CHKERRQ(ierr); }      /* else the sweep of step k - 1 wrote Z[k] */
    have_z = PETSC_FALSE;
    ierr = KSP_MatMult(ksp, A, gm->Z[k], BASIS(gm, k + 1));CHKERRQ(ierr);
    done = PETSC_FALSE;
    if (gm->refine == KSP_GMRES_CGS_REFINE_NEVER) {
      if (P && k + 1 < gm->m) {
        ierr = P->fgmres_orthog_normalize_pc(BASIS(gm, k + 1), k + 1, &BASIS(gm, 0), gm->common.dinv, (PetscBool)(gm->pckind == PCKIND_IDENTITY), gm->Z[k + 1], gm->coef, &tt, &done);CHKERRQ(ierr);
        have_z = done;
      }
      if (!done && F) { ierr = F->gmres_orthog_normalize(BASIS(gm, k + 1), k + 1, &BASIS(gm, 0), gm->coef, &tt, &done);CHKERRQ(ierr); }
      if (done) for (PetscInt j = 0; j <= k; j++) { const PetscScalar c = -gm->coef[j]; hcol[j] = 0.0; hcol[j] -= c; }   /* borthog2.c:52-66 */
    }
    if (!done) {
      ierr = gmres_orthogonalize(ksp, k, hcol);CHKERRQ(ierr);
      ierr = VecNormalize(BASIS(gm, k + 1), &tt);CHKERRQ(ierr);
    }
    gm->common.count[have_z ? 0 : 1]++;                                  /* (steps that wrote the next Z in the sweep, all other steps) */
    hcol[k + 1] = tt;
    hapbnd = PetscAbsScalar(tt / gm->g[k]);
    if (hapbnd > gm->haptol) hapbnd = gm->haptol;
    if (!(tt > hapbnd)) hapend = PETSC_TRUE;
    gmres_rotate(ksp, k, hapend, &res);
    if (ksp->reason) break;                                              /* a rotation of length 0: the column does not count */
    k++;
    ksp->its++;
    ksp->rnorm = res;
    ierr = KSPTestConvergence(ksp, ksp->its, res);CHKERRQ(ierr);
    if (hapend) {
      if (!ksp->reason) SETERRQ(HipObjComm(ksp), PETSC_ERR_PLIB, "You reached the happy break down, but convergence was not indicated. Residual norm = %g", (double)res);
      break;
    }
  }
  KSPLogResidualHistory(ksp, res);
  if (ksp->reason || ksp->its >= ksp->max_it) { ierr = KSPMonitor(ksp, ksp->its, res);CHKERRQ(ierr); }
  ierr = fgmres_update_solution(ksp, k);CHKERRQ(ierr);
  return 0;
}

static PetscErrorCode KSPSolve_FGMRESHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_GMRESHIP *gm = GH(ksp);
  Vec d;                                                                 /* the cycle takes the diagonal from the common header */
  ksp->its = 0;
  ksp->reason = KSP_CONVERGED_ITERATING;
  /* what the sweep may apply itself: a PC nobody changes, nothing projected behind it */
  ierr = pc_diagonal_form(ksp, (PetscBool)(gm->common.fused && !gm->modifypc), BASIS(gm, 0), &gm->pckind, &d);CHKERRQ(ierr);
  if (ksp->guess_zero) { ierr = VecCopy(ksp->vec_rhs, BASIS(gm, 0));CHKERRQ(ierr); }
  else { ierr = fgmres_residual(ksp);CHKERRQ(ierr); }
  ierr = fgmres_cycle(ksp);CHKERRQ(ierr);
  while (!ksp->reason) {
    ierr = fgmres_residual(ksp);CHKERRQ(ierr);
    if (ksp->its >= ksp->max_it) break;
    ierr = fgmres_cycle(ksp);CHKERRQ(ierr);
  }
  if (ksp->its >= ksp->max_it && !ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

static const KSPHipMethod fgmres_methods[] = {   /* on top of gmres_methods */
  {"KSPFGMRESSetModifyPC_C", "KSPFGMRESSetModifyPC_FGMRESHIP", (PetscVoidFunction)KSPFGMRESSetModifyPC_FGMRESHIP},
  COUNTS_METHOD,
  {NULL, NULL, NULL}};
static PetscErrorCode KSPDestroy_FGMRESHIP(KSP ksp) {
  PetscErrorCode ierr;
  if (!ksp->data) return 0;
  ierr = KSPDestroy_GMRESHIP(ksp);CHKERRQ(ierr);
  return ksp_compose(ksp, fgmres_methods, PETSC_FALSE);
}

PetscErrorCode KSPCreate_FGMRESHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = KSPCreate_GMRESHIPMI355X(ksp);CHKERRQ(ierr);
  GH(ksp)->flexible = PETSC_TRUE; GH(ksp)->nscr = 1; COMMON(ksp)->fused = PETSC_FALSE;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 0);CHKERRQ(ierr);      /* right preconditioning only: the true residual's norm, or none */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NONE, PC_LEFT, 0);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_RIGHT, 2);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NONE, PC_RIGHT, 1);CHKERRQ(ierr);
  ksp->ops->solve = KSPSolve_FGMRESHIP; ksp->ops->destroy = KSPDestroy_FGMRESHIP;
  return ksp_compose(ksp, fgmres_methods, PETSC_TRUE);
}

/* ================================================================================================ BiCGStab
 * -ksp_bcgs_fused <bool> (default true), left preconditioning.  PCJACOBI: both products write d .* (A x) themselves; PCJACOBI /
 * PCNONE on types without that method: PCApply fused with the dot(s) that follow it; the x / r update, |r| and the NEXT
 * iteration's rho are one sweep: 22 vector passes and 3 reductions per iteration instead of 27 and 4, identical bits. */
static PetscErrorCode KSPSetUp_BCGSHIP(KSP ksp) { return KSPDefaultGetWork(ksp, 6); }
static PetscErrorCode KSPSetFromOptions_BCGSHIP(KSP ksp) { return option_bool(ksp, "-ksp_bcgs_fused", &COMMON(ksp)->fused); }
static PetscErrorCode KSPDestroy_BCGSHIP(KSP ksp) { return ksp_destroy_data(ksp, NULL); }

static PetscErrorCode KSPSolve_BCGSHIP(KSP ksp) {
  PetscErrorCode ierr;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, r = ksp->work[0], rshadow = ksp->work[1], v = ksp->work[2], t = ksp->work[3], s = ksp->work[4], p = ksp->work[5];
  Mat A;
  const VecKrylovFusedOps *F = COMMON(ksp)->fused ? vec_fused_ops(x) : NULL;
  HipPCKind pck;
  Vec d;
  const PetscBool nonorm = (PetscBool)(ksp->normtype == KSP_NORM_NONE);
  PetscScalar rho = 0.0, rho_used, rho_prev = 1.0, alpha = 1.0, omega, omega_prev = 1.0, beta, sv;
  PetscReal rn = 0.0, tt;
  PetscBool have_rho = PETSC_FALSE;
  PetscInt it;

  if (ksp->pc_side == PC_RIGHT) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "right-preconditioned BiCGStab is outside the ported path");
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(F != NULL), x, &pck, &d);CHKERRQ(ierr);
  ierr = KSPInitialResidual(ksp, x, v, t, r, rhs);CHKERRQ(ierr);
  if (!nonorm) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
  ksp->its = 0;
  ierr = report(ksp, 0, rn);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, rn);CHKERRQ(ierr);
  if (ksp->reason) return 0;
  ierr = VecCopy(r, rshadow);CHKERRQ(ierr);
  ierr = VecSet(p, 0.0);CHKERRQ(ierr);
  ierr = VecSet(v, 0.0);CHKERRQ(ierr);
  it = 0;
  do {
    PetscBool done = PETSC_FALSE;
    if (!have_rho) { ierr = VecDot(r, rshadow, &rho);CHKERRQ(ierr); }
    have_rho = PETSC_FALSE;
    rho_used = rho;
    beta = (rho / rho_prev) * (alpha / omega_prev);
    ierr = VecAXPBYPCZ(p, 1.0, -omega_prev * beta, beta, r, v);CHKERRQ(ierr);          /* p <- r - omega beta v + beta p */
    ierr = apply_operator(ksp, A, F, pck, d, p, v, t, 1, rshadow, &sv, NULL);CHKERRQ(ierr);   /* v <- K p, (v, r~) */
    if (sv == 0.0) SETERRQ(HipObjComm(ksp), PETSC_ERR_PLIB, "Divide by zero");
    alpha = rho / sv;
    ierr = VecWAXPY(s, -alpha, v, r);CHKERRQ(ierr);                                    /* s <- r - alpha v */
    ierr = apply_operator(ksp, A, F, pck, d, s, t, r, 2, s, &sv, &tt);CHKERRQ(ierr);    /* t <- K s, (s, t), (t, t) */
    if (tt == 0.0) {                                                                    /* t = 0: if s = 0 too, alpha p may be the solution */
      ierr = VecDot(s, s, &sv);CHKERRQ(ierr);
      if (sv != 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
      ierr = VecAXPY(x, alpha, p);CHKERRQ(ierr);
      ksp->its++;
      ksp->rnorm = 0.0;
      ksp->reason = KSP_CONVERGED_RTOL;
      KSPLogResidualHistory(ksp, rn);
      ierr = KSPMonitor(ksp, it + 1, 0.0);CHKERRQ(ierr);
      break;
    }
    omega = sv / tt;
    if (F && pck != PCKIND_GENERAL) {                                                   /* x, r, (r, r) and the next (r, r~) in one sweep */
      PetscScalar rr, rho_next;
      ierr = F->bcgs_update(x, r, p, s, t, rshadow, alpha, omega, &rr, &rho_next, &done);CHKERRQ(ierr);
      if (done) { rn = nonorm ? 0.0 : PetscSqrtReal(rr); rho = rho_next; have_rho = PETSC_TRUE; }
    }
    if (!done) {
      ierr = VecAXPBYPCZ(x, alpha, omega, 1.0, p, s);CHKERRQ(ierr);                    /* x <- x + alpha p + omega s */
      ierr = VecWAXPY(r, -omega, t, s);CHKERRQ(ierr);                                  /* r <- s - omega t */
      if (!nonorm) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
    }
    rho_prev = rho_used;
    omega_prev = omega;
    ksp->its++;
    ierr = report(ksp, it + 1, rn);CHKERRQ(ierr);
    ierr = KSPTestConvergence(ksp, it + 1, rn);CHKERRQ(ierr);
    if (ksp->reason) break;
    if (rho_used == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }              /* bcgs.c:146: the rho this iteration used */
    it++;
  } while (it < ksp->max_it);
  if (it >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

PetscErrorCode KSPCreate_BCGSHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSPHipCommon), NULL);CHKERRQ(ierr);   /* the common header is all this type keeps */
  COMMON(ksp)->fused = PETSC_TRUE;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_BCGSHIP; ksp->ops->solve = KSPSolve_BCGSHIP; ksp->ops->setfromoptions = KSPSetFromOptions_BCGSHIP; ksp->ops->destroy = KSPDestroy_BCGSHIP;
  return 0;
}

/* ================================================================================================ Chebyshev and Richardson
 * The sequences of KSPSolve_Chebychev (src/ksp/ksp/impls/cheby/cheby.c; eigenvalue bounds from the user: KSPChebychevSetEigenvalues,
 * -ksp_chebychev_eigenvalues <emin,emax>) and KSPSolve_Richardson (src/ksp/ksp/impls/rich/rich.c; KSPRichardsonSetScale,
 * -ksp_richardson_scale <s>; never PCApplyRichardson), same iterates, histories and exits as those.  What follows the product of an
 * iteration -- residual, PCJACOBI / PCNONE, update, and for Chebyshev the norm's sums -- is ONE sweep ("cheby_step", "rich_step" of
 * include/petsckrylovfused.h): with KSP_NORM_NONE an iteration is a product and an element-wise pass, nothing is reduced and the host
 * never waits.  Any other PC, or a null space: the public calls, and for Chebyshev the three-term update alone in the sweep. */
static PetscErrorCode option_reals(KSP ksp, const char *name, PetscReal v[2], int *count) {   /* "-name <real>[,<real>]" */
  char t[96], *comma; PetscBool set;
  PetscErrorCode ierr = PetscOptionsGetString(HipObjPrefix(ksp), name, t, sizeof(t), &set);CHKERRQ(ierr);
  *count = 0;
  if (!set || !t[0]) return 0;
  comma = strchr(t, ',');
  if (comma) { *comma = 0; v[1] = atof(comma + 1); }
  v[0] = atof(t);
  *count = comma ? 2 : 1;
  return 0;
}
/* the exit both solvers share once the loop has ended without a reason (cheby.c, rich.c): the budget is spent */
static PetscErrorCode stationary_out_of_iterations(KSP ksp, PetscReal rn) {
  PetscErrorCode ierr;
  if (ksp->its < ksp->max_it) return 0;
  if (ksp->normtype == KSP_NORM_NONE) { ksp->reason = KSP_CONVERGED_ITS; return 0; }
  ierr = KSPTestConvergence(ksp, ksp->its, rn);CHKERRQ(ierr);
  if (!ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

typedef struct { KSPHipCommon common; PetscReal emin, emax; } KSP_ChebyHIP;

static PetscErrorCode KSPChebychevSetEigenvalues_ChebyHIP(KSP ksp, PetscReal emax, PetscReal emin) {
  KSP_ChebyHIP *ch = (KSP_ChebyHIP *)ksp->data;
  if (emax <= emin) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_INCOMP, "Maximum eigenvalue must be larger than minimum: max %g min %g", (double)emax, (double)emin);
  if (emax * emin <= 0.0) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_INCOMP, "Both eigenvalues must be of the same sign: max %g min %g", (double)emax, (double)emin);
  ch->emax = emax; ch->emin = emin;
  return 0;
}
/* the three-term update cannot be written with the public calls this library may use (no VecScale): the vectors' type must offer it */
static PetscErrorCode cheby_ops(KSP ksp, Vec x, const VecKrylovFusedOps **F) {
  *F = vec_fused_ops(x);
  return needs_table(ksp, (PetscBool)(*F && (*F)->cheby_step), KSPCHEBYCHEVHIPMI355X, "Chebyshev step", "VecKrylovFusedOps_C", "chebychev");
}
static PetscErrorCode KSPSetUp_ChebyHIP(KSP ksp) {
  const VecKrylovFusedOps *F;
  PetscErrorCode ierr = KSPDefaultGetWork(ksp, 3);CHKERRQ(ierr);
  return cheby_ops(ksp, ksp->vec_sol ? ksp->vec_sol : ksp->work[0], &F);   /* the vectors the solve will run on */
}
static PetscErrorCode KSPSetFromOptions_ChebyHIP(KSP ksp) {
  PetscReal v[2]; int count;
  PetscErrorCode ierr = option_reals(ksp, "-ksp_chebychev_eigenvalues", v, &count);CHKERRQ(ierr);
  if (count == 1) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_INCOMP, "-ksp_chebychev_eigenvalues: must specify 2 parameters, min and max eigenvalues");
  if (count == 2) { ierr = KSPChebychevSetEigenvalues_ChebyHIP(ksp, v[1], v[0]);CHKERRQ(ierr); }
  return 0;
}
static const KSPHipMethod cheby_methods[] = {
  {"KSPChebychevSetEigenvalues_C", "KSPChebychevSetEigenvalues_ChebyHIP", (PetscVoidFunction)KSPChebychevSetEigenvalues_ChebyHIP},
  {NULL, NULL, NULL}};
static PetscErrorCode KSPDestroy_ChebyHIP(KSP ksp) { return ksp_destroy_data(ksp, cheby_methods); }

static PetscErrorCode KSPSolve_ChebyHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_ChebyHIP *ch = (KSP_ChebyHIP *)ksp->data;
  const KSPNormType nt = ksp->normtype;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, r = ksp->work[2];
  Vec p[3] = {x, ksp->work[0], ksp->work[1]};
  const VecKrylovFusedOps *F;
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscScalar c[3], scale, mu, omegaprod, omega, Gamma = 1.0, zz = 0.0, rr = 0.0;
  PetscReal rn = 0.0;
  PetscInt km1 = 0, k = 1, kp1 = 2, i;
  PetscBool done;

  ierr = cheby_ops(ksp, x, &F);CHKERRQ(ierr);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, PETSC_TRUE, x, &pck, &d);CHKERRQ(ierr);
  ksp->its = 0;
  scale = 2.0 / (ch->emax + ch->emin);
  mu = 1.0 / (1.0 - scale * ch->emin);
  omegaprod = 2.0 / (1.0 - scale * ch->emin);
  c[km1] = 1.0; c[k] = mu;
  ierr = start_residual(ksp, A, x, rhs, r);CHKERRQ(ierr);
  ierr = KSP_PCApply(ksp, r, p[k]);CHKERRQ(ierr);
  ierr = VecAYPX(p[k], scale, x);CHKERRQ(ierr);                                         /* p[k] = x + scale B r */
  for (i = 0; i < ksp->max_it; i++) {
    ksp->its++;
    c[kp1] = 2.0 * mu * c[k] - c[km1];
    omega = omegaprod * c[k] / c[kp1];
    ierr = KSP_MatMult(ksp, A, p[k], r);CHKERRQ(ierr);
    if (pck != PCKIND_GENERAL) {
      /* residual, B, the norm's sums and p[kp1] in one sweep.  p[kp1] is a work vector (the iterate the test sees is p[k]), so a
       * solve that stops at this checkpoint has lost nothing; r itself is not stored, nobody reads it */
      const PetscBool sums = (PetscBool)(nt != KSP_NORM_NONE);
      ierr = F->cheby_step(p[kp1], NULL, r, rhs, d, p[km1], p[k], omega * Gamma * scale, 1.0 - omega, omega, sums ? &zz : NULL, sums ? &rr : NULL, &done);CHKERRQ(ierr);
      if (!done) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused Chebyshev step refused these vectors; use -ksp_type chebychev");
      if (sums) {
        rn = PetscSqrtReal(nt == KSP_NORM_UNPRECONDITIONED ? rr : zz);                  /* the square is reduced, then rooted (pvec2.c:62-64) */
        ksp->vec_sol = p[k];
        ierr = report(ksp, i, rn);CHKERRQ(ierr);
        ierr = KSPTestConvergence(ksp, i, rn);CHKERRQ(ierr);
        if (ksp->reason) break;
      }
    } else {
      ierr = VecAYPX(r, -1.0, rhs);CHKERRQ(ierr);
      ierr = KSP_PCApply(ksp, r, p[kp1]);CHKERRQ(ierr);
      if (nt != KSP_NORM_NONE) {
        ierr = VecNorm(nt == KSP_NORM_UNPRECONDITIONED ? r : p[kp1], NORM_2, &rn);CHKERRQ(ierr);
        ksp->vec_sol = p[k];
        ierr = report(ksp, i, rn);CHKERRQ(ierr);
        ierr = KSPTestConvergence(ksp, i, rn);CHKERRQ(ierr);
        if (ksp->reason) break;
      }
      /* p[kp1] holds B r as KSP_PCApply left it: the update alone, in place */
      ierr = F->cheby_step(p[kp1], NULL, p[kp1], NULL, NULL, p[km1], p[k], omega * Gamma * scale, 1.0 - omega, omega, NULL, NULL, &done);CHKERRQ(ierr);
      if (!done) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused Chebyshev step refused these vectors; use -ksp_type chebychev");
    }
    { const PetscInt was = km1; km1 = k; k = kp1; kp1 = was; }
  }
  if (!ksp->reason) {
    if (nt != KSP_NORM_NONE) {
      ierr = KSP_MatMult(ksp, A, p[k], r);CHKERRQ(ierr);
      ierr = VecAYPX(r, -1.0, rhs);CHKERRQ(ierr);
      if (nt == KSP_NORM_UNPRECONDITIONED) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
      else { ierr = KSP_PCApply(ksp, r, p[kp1]);CHKERRQ(ierr); ierr = VecNorm(p[kp1], NORM_2, &rn);CHKERRQ(ierr); }
      ksp->vec_sol = p[k];
      ierr = report(ksp, ksp->its, rn);CHKERRQ(ierr);
    }
    ierr = stationary_out_of_iterations(ksp, rn);CHKERRQ(ierr);
  }
  ksp->vec_sol = x;
  if (p[k] != x) { ierr = VecCopy(p[k], x);CHKERRQ(ierr); }
  return 0;
}

PetscErrorCode KSPCreate_ChebychevHIPMI355X(KSP ksp) {
  KSP_ChebyHIP *ch;
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(*ch), cheby_methods);CHKERRQ(ierr);
  ch = (KSP_ChebyHIP *)ksp->data;
  ch->emin = 1.0e-2; ch->emax = 1.0e+2;                                                  /* KSPCreate_Chebychev's defaults */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_ChebyHIP; ksp->ops->solve = KSPSolve_ChebyHIP; ksp->ops->setfromoptions = KSPSetFromOptions_ChebyHIP; ksp->ops->destroy = KSPDestroy_ChebyHIP;
  return 0;
}

/* ================================================================================================ pipelined CG
 * The sequence of KSPSolve_PIPECG (src/ksp/ksp/impls/cg/pipecg/pipecg.c:49-205): nine work vectors, the norm table of KSPPIPECG, ONE
 * split-phase reduction per iteration in flight over m = B w and n = A m, the same quantity riding with w'u in each iteration (with the
 * preconditioned or the unpreconditioned norm res'u is reduced in iteration 0 only), same iterates, histories and exits.  The solve
 * start and iteration 0 are the public calls.  From then on what follows the End calls of iteration k -- four VecAYPX (VecCopy), four
 * VecAXPY, with PCJACOBI / PCNONE and no null space iteration k+1's m = B w, and iteration k+1's VecNormBegin / VecDotBegin pair -- is
 * ONE sweep ("pipecg_step" of "VecPipelinedCGFusedOps_C", include/petsckrylovfused.h) that leaves the sums pending; the driver goes on
 * with the communicator-wide Begin, the product, and the End calls (all of them through the type's "VecSplitReductionOps_C").  The sweep of the last permitted iteration queues no sums, so no
 * exit leaves a split phase pending.  Vectors without the table, a sweep that refuses, or -ksp_pipecg_fused false: the public calls
 * of that step.  KSPHIPMI355XGetFusedStepCounts: steps taken by each route. */
/* The split-phase reductions as the vectors' type provides them ("VecSplitReductionOps_C", what VecDotBegin / VecNormBegin / VecDotEnd /
 * VecNormEnd / PetscCommSplitReductionBegin of the object model dispatch to for these vectors).  A type without the table: Begin is
 * the whole reduction (VecDot / VecNorm), nothing is in flight and End has nothing left to do -- the vectors do not change between the
 * two, so the value is the one End would have delivered. */
static PetscErrorCode split_dot_begin(const VecSplitReductionOps *S, Vec x, Vec y, PetscScalar *v) { return S ? S->dot_begin(x, y, v) : VecDot(x, y, v); }
static PetscErrorCode split_dot_end(const VecSplitReductionOps *S, Vec x, Vec y, PetscScalar *v) { return S ? S->dot_end(x, y, v) : 0; }
static PetscErrorCode split_norm_begin(const VecSplitReductionOps *S, Vec x, PetscReal *v) { return S ? S->norm_begin(x, NORM_2, v) : VecNorm(x, NORM_2, v); }
static PetscErrorCode split_norm_end(const VecSplitReductionOps *S, Vec x, PetscReal *v) { return S ? S->norm_end(x, NORM_2, v) : 0; }
static PetscErrorCode split_comm_begin(const VecSplitReductionOps *S, Vec x) { return S && S->comm_begin ? S->comm_begin(HipObjComm(x)) : 0; }

static PetscErrorCode KSPSetUp_PipeCGHIP(KSP ksp) { return KSPDefaultGetWork(ksp, 9); }
static PetscErrorCode KSPSetFromOptions_PipeCGHIP(KSP ksp) { return option_bool(ksp, "-ksp_pipecg_fused", &COMMON(ksp)->fused); }
static PetscErrorCode KSPDestroy_PipeCGHIP(KSP ksp) { return ksp_destroy_data(ksp, counts_only); }

enum { PIPE_NOTHING = 0, PIPE_RR = 1, PIPE_UU = 2, PIPE_RU = 3 };   /* what rides with w'u in an iteration's reduction: "rides" of pipecg_step */
static int pipecg_rides(KSPNormType norm, PetscInt k) {             /* pipecg.c:124-131,138-145 */
  const PetscBool normed = (PetscBool)(norm == KSP_NORM_UNPRECONDITIONED || norm == KSP_NORM_PRECONDITIONED);
  if (k > 0 && normed) return norm == KSP_NORM_UNPRECONDITIONED ? PIPE_RR : PIPE_UU;
  if (k == 0 && norm == KSP_NORM_NATURAL) return PIPE_NOTHING;      /* res'u is iteration 0's norm already */
  return PIPE_RU;
}

static PetscErrorCode KSPSolve_PipeCGHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSPHipCommon *pd = COMMON(ksp);      /* all this type keeps; count: (steps taken by the sweep, steps taken by the public calls) */
  const KSPNormType norm = ksp->normtype;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs;
  Vec m = ksp->work[0], ABs_rec = ksp->work[1], dir = ksp->work[2], n = ksp->work[3], w = ksp->work[4];
  Vec Bs_rec = ksp->work[5], u = ksp->work[6], res = ksp->work[7], s = ksp->work[8];
  Vec normed = norm == KSP_NORM_UNPRECONDITIONED ? res : norm == KSP_NORM_PRECONDITIONED ? u : NULL;
  const VecSplitReductionOps *S = vec_split_ops(x);
  const VecPipelinedCGFusedOps *P = pd->fused && S ? vec_pipelined_ops(x) : NULL;   /* a sweep leaves its sums pending in the type's split phase */
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscScalar step = 0.0, ratio = 0.0, ru = 0.0, ru_last = 0.0, wu = 0.0;
  PetscReal rn = 0.0;
  PetscInt k = 0;
  PetscBool pending = PETSC_FALSE;    /* the sweep of the iteration before has queued this iteration's sums ... */
  PetscBool m_formed = PETSC_FALSE;   /* ... and formed m = B w */

  if (norm != KSP_NORM_PRECONDITIONED && norm != KSP_NORM_UNPRECONDITIONED && norm != KSP_NORM_NATURAL && norm != KSP_NORM_NONE) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "norm type %d", (int)norm);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(P && P->pipecg_step), x, &pck, &d);CHKERRQ(ierr);
  ksp->its = 0;
  ierr = start_residual(ksp, A, x, rhs, res);CHKERRQ(ierr);
  ierr = KSP_PCApply(ksp, res, u);CHKERRQ(ierr);
  /* iteration 0's norm, its reduction in flight over w <- A u */
  if (normed) { ierr = split_norm_begin(S, normed, &rn);CHKERRQ(ierr); ierr = split_comm_begin(S, normed);CHKERRQ(ierr); }
  else if (norm == KSP_NORM_NATURAL) { ierr = split_dot_begin(S, res, u, &ru);CHKERRQ(ierr); ierr = split_comm_begin(S, res);CHKERRQ(ierr); }
  ierr = KSP_MatMult(ksp, A, u, w);CHKERRQ(ierr);
  if (normed) { ierr = split_norm_end(S, normed, &rn);CHKERRQ(ierr); }
  else if (norm == KSP_NORM_NATURAL) { ierr = split_dot_end(S, res, u, &ru);CHKERRQ(ierr); KSPCheckDot(ksp, ru); rn = PetscSqrtReal(PetscAbsScalar(ru)); }
  ierr = report(ksp, 0, rn);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, rn);CHKERRQ(ierr);
  if (ksp->reason) return 0;

  do {
    const int rides = pipecg_rides(norm, k);
    PetscBool done = PETSC_FALSE;
    if (!pending) {
      if (rides == PIPE_RR || rides == PIPE_UU) { ierr = split_norm_begin(S, normed, &rn);CHKERRQ(ierr); }
      else if (rides == PIPE_RU) { ierr = split_dot_begin(S, res, u, &ru);CHKERRQ(ierr); }
      ierr = split_dot_begin(S, w, u, &wu);CHKERRQ(ierr);
    }
    ierr = split_comm_begin(S, res);CHKERRQ(ierr);
    if (!m_formed) { ierr = KSP_PCApply(ksp, w, m);CHKERRQ(ierr); }                     /* the work the reduction hides behind */
    ierr = KSP_MatMult(ksp, A, m, n);CHKERRQ(ierr);
    if (rides == PIPE_RR || rides == PIPE_UU) { ierr = split_norm_end(S, normed, &rn);CHKERRQ(ierr); }
    else if (rides == PIPE_RU) { ierr = split_dot_end(S, res, u, &ru);CHKERRQ(ierr); }
    ierr = split_dot_end(S, w, u, &wu);CHKERRQ(ierr);
    pending = PETSC_FALSE; m_formed = PETSC_FALSE;
    if (k > 0) {
      if (norm == KSP_NORM_NATURAL) rn = PetscSqrtReal(PetscAbsScalar(ru));
      else if (norm == KSP_NORM_NONE) rn = 0.0;
      ierr = report(ksp, k, rn);CHKERRQ(ierr);
      ierr = KSPTestConvergence(ksp, k, rn);CHKERRQ(ierr);
      if (ksp->reason) break;
      ratio = ru / ru_last;
      step = ru / (wu - ratio / step * ru);
    } else step = ru / wu;
    if (P && P->pipecg_step) {
      /* the whole update, iteration k+1's m and its sums in one sweep; the last permitted iteration has no successor to reduce for */
      const int next = k + 1 < ksp->max_it ? pipecg_rides(norm, k + 1) : PIPE_NOTHING;
      ierr = P->pipecg_step(x, u, w, res, ABs_rec, Bs_rec, dir, s, n, m, d, pck != PCKIND_GENERAL ? m : NULL, (PetscBool)(k == 0), k == 0 ? 0.0 : ratio, step, next, &done);CHKERRQ(ierr);
      if (done) { pending = (PetscBool)(next != PIPE_NOTHING); m_formed = (PetscBool)(pck != PCKIND_GENERAL); pd->count[0]++; }
    }
    if (!done) {
      if (k > 0) {
        ierr = VecAYPX(ABs_rec, ratio, n);CHKERRQ(ierr);
        ierr = VecAYPX(Bs_rec, ratio, m);CHKERRQ(ierr);
        ierr = VecAYPX(dir, ratio, u);CHKERRQ(ierr);
        ierr = VecAYPX(s, ratio, w);CHKERRQ(ierr);
      } else {
        ierr = VecCopy(n, ABs_rec);CHKERRQ(ierr);
        ierr = VecCopy(m, Bs_rec);CHKERRQ(ierr);
        ierr = VecCopy(u, dir);CHKERRQ(ierr);
        ierr = VecCopy(w, s);CHKERRQ(ierr);
      }
      ierr = VecAXPY(x, step, dir);CHKERRQ(ierr);
      ierr = VecAXPY(u, -step, Bs_rec);CHKERRQ(ierr);
      ierr = VecAXPY(w, -step, ABs_rec);CHKERRQ(ierr);
      ierr = VecAXPY(res, -step, s);CHKERRQ(ierr);
      pd->count[1]++;
    }
    ru_last = ru;
    ksp->its = ++k;
  } while (k < ksp->max_it);
  if (k >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

PetscErrorCode KSPCreate_PIPECGHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSPHipCommon), counts_only);CHKERRQ(ierr);
  COMMON(ksp)->fused = PETSC_TRUE;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);    /* the four of KSPPIPECG, pipecg.c:199-202 */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NATURAL, PC_LEFT, 1);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_NONE, PC_LEFT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_PipeCGHIP; ksp->ops->solve = KSPSolve_PipeCGHIP; ksp->ops->setfromoptions = KSPSetFromOptions_PipeCGHIP; ksp->ops->destroy = KSPDestroy_PipeCGHIP;
  return 0;
}

/* ================================================================================================ MINRES
 * The sequence of KSPSolve_MINRES (src/ksp/ksp/impls/minres/minres.c): left preconditioning, the preconditioned norm, the residual
 * estimate rnorm |s| of the recurrence, the exits at r'z < 1e-18 (also taken on a lucky breakdown, as the reference takes them); same
 * iterates, histories and exits as the op-by-op type, bit for bit.  Behind the product an iteration is TWO sweeps of
 * "VecMinresFusedOps_C" (include/petsckrylovfused.h) instead of 2 dots, 7 VecAXPY, 7 VecCopy, 3 VecScale and PCApply_Jacobi:
 *   - alpha = u'r through tdot_begin where the vectors accept it: VecDot's bits, left on the device, no wait (VecDot otherwise);
 *   - the Lanczos sweep: Jacobi, the four AXPYs and r'z, which comes home with alpha in the iteration's one wait;
 *   - the Givens scalars on the host;
 *   - the update sweep: the new search direction, x, and the next Lanczos pair scaled into the buffers of the pair that drops out.
 * The copies of the reference are pointer rotations here: (V, VOLD), (U, UOLD) and (W, WOLD) swap after every update, and WOOLD is
 * never needed (the update reads the old WOLD in place before it stores the new W over it).  Any PC but Jacobi, or a null space:
 * KSP_PCApply forms z and the Lanczos sweep takes it as given.  The solve start is the public calls but for its two VecScale, which
 * are the `first` form of the update sweep: VecScale is not among the calls this library takes from PETSc, so like chebychevhipmi355x
 * the type has no op-by-op route and KSPSetUp returns PETSC_ERR_SUP on vectors without the table (-ksp_type minres is that route).
 * KSPHIPMI355XGetFusedStepCounts: (Lanczos sweeps run, 0). */
static PetscErrorCode minres_ops(KSP ksp, Vec x, const VecMinresFusedOps **M) {
  *M = vec_minres_ops(x);
  return needs_table(ksp, (PetscBool)(*M != NULL), KSPMINRESHIPMI355X, "MINRES sweeps", "VecMinresFusedOps_C", "minres");
}
static PetscErrorCode KSPSetUp_MinresHIP(KSP ksp) {
  const VecMinresFusedOps *M;
  PetscErrorCode ierr = KSPDefaultGetWork(ksp, 8);CHKERRQ(ierr);
  return minres_ops(ksp, ksp->vec_sol ? ksp->vec_sol : ksp->work[0], &M);   /* the vectors the solve will run on */
}
static PetscErrorCode KSPDestroy_MinresHIP(KSP ksp) { return ksp_destroy_data(ksp, counts_only); }

static PetscErrorCode KSPSolve_MinresHIP(KSP ksp) {
  PetscErrorCode ierr;
  const PetscReal haptol = 1.e-18;
  Vec X = ksp->vec_sol, B = ksp->vec_rhs;
  Vec R = ksp->work[0], Z = ksp->work[1], U = ksp->work[2], V = ksp->work[3], W = ksp->work[4], UOLD = ksp->work[5], VOLD = ksp->work[6], WOLD = ksp->work[7];
  const VecMinresFusedOps *M;
  const VecKrylovFusedOps *F = vec_fused_ops(X);
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscScalar alpha = 0.0, beta, betaold, eta, c = 1.0, cold = 1.0, coold, s = 0.0, sold = 0.0, soold, rho0, rho1, rho2, rho3, dp = 0.0;
  PetscReal np;
  PetscInt i;
  PetscBool done;

  ierr = minres_ops(ksp, X, &M);CHKERRQ(ierr);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, PETSC_TRUE, X, &pck, &d);CHKERRQ(ierr);
  ksp->its = 0;
  ierr = VecSet(UOLD, 0.0);CHKERRQ(ierr);
  ierr = VecCopy(UOLD, VOLD);CHKERRQ(ierr);
  ierr = VecCopy(UOLD, W);CHKERRQ(ierr);
  ierr = VecCopy(UOLD, WOLD);CHKERRQ(ierr);
  ierr = start_residual(ksp, A, X, B, R);CHKERRQ(ierr);
  ierr = KSP_PCApply(ksp, R, Z);CHKERRQ(ierr);
  ierr = VecNorm(Z, NORM_2, &np);CHKERRQ(ierr);
  ierr = VecDot(R, Z, &dp);CHKERRQ(ierr);
  if (dp < haptol) { ksp->reason = KSP_DIVERGED_INDEFINITE_MAT; return 0; }
  beta = PetscSqrtReal(PetscAbsScalar(dp));
  eta = beta;
  ierr = M->minres_update(NULL, NULL, NULL, NULL, R, Z, V, U, PETSC_TRUE, 0.0, 0.0, 0.0, 0.0, 1.0 / beta, &done);CHKERRQ(ierr);   /* V = R / beta, U = Z / beta */
  if (!done) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused MINRES sweep refused these vectors; use -ksp_type minres");
  ierr = report(ksp, 0, np);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, np);CHKERRQ(ierr);
  if (ksp->reason) return 0;

  for (i = 0; i < ksp->max_it; i++) {
    PetscBool on_device = PETSC_FALSE;
    ksp->its = i + 1;
    ierr = KSP_MatMult(ksp, A, U, R);CHKERRQ(ierr);
    if (F && F->tdot_begin) { ierr = F->tdot_begin(U, R, &on_device);CHKERRQ(ierr); }
    if (!on_device) { ierr = VecDot(U, R, &alpha);CHKERRQ(ierr); }
    if (!d) { ierr = KSP_PCApply(ksp, R, Z);CHKERRQ(ierr); }
    ierr = M->minres_lanczos(R, Z, V, U, VOLD, UOLD, d, alpha, on_device, beta, &dp, &alpha, &done);CHKERRQ(ierr);
    if (!done) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused MINRES sweep refused these vectors; use -ksp_type minres");
    COMMON(ksp)->count[0]++;                                             /* (Lanczos sweeps run, 0) */
    betaold = beta;
    if (dp < haptol) { ksp->reason = KSP_DIVERGED_INDEFINITE_PC; break; }
    beta = PetscSqrtReal(PetscAbsScalar(dp));
    coold = cold; cold = c; soold = sold; sold = s;
    rho0 = cold * alpha - coold * sold * betaold;
    rho1 = PetscSqrtReal(rho0 * rho0 + beta * beta);
    rho2 = sold * alpha + coold * cold * betaold;
    rho3 = soold * betaold;
    c = rho0 / rho1;
    s = beta / rho1;
    /* the new W over the old WOLD, x, and the new (V, U) into the buffers of (VOLD, UOLD); then the names rotate */
    ierr = M->minres_update(X, U, W, WOLD, R, Z, VOLD, UOLD, PETSC_FALSE, rho2, rho3, 1.0 / rho1, c * eta, 1.0 / beta, &done);CHKERRQ(ierr);
    if (!done) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused MINRES sweep refused these vectors; use -ksp_type minres");
    { Vec t = W; W = WOLD; WOLD = t; t = V; V = VOLD; VOLD = t; t = U; U = UOLD; UOLD = t; }
    eta = -s * eta;
    np = ksp->rnorm * PetscAbsScalar(s);
    ierr = report(ksp, i + 1, np);CHKERRQ(ierr);
    ierr = KSPTestConvergence(ksp, i + 1, np);CHKERRQ(ierr);
    if (ksp->reason) break;
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

PetscErrorCode KSPCreate_MINRESHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSPHipCommon), counts_only);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);    /* the one of KSPMINRES */
  ksp->ops->setup = KSPSetUp_MinresHIP; ksp->ops->solve = KSPSolve_MinresHIP; ksp->ops->destroy = KSPDestroy_MinresHIP;
  return 0;
}

/* ================================================================================================ TFQMR and CGS
 * The sequences of KSPSolve_TFQMR (src/ksp/ksp/impls/tfqmr/tfqmr.c) and KSPSolve_CGS (src/ksp/ksp/impls/cgs/cgs.c), one function for
 * both (they share the recurrence over R, U, P, Q and the shadow residual RP): left preconditioning, the preconditioned norm; same
 * iterates, histories and exits as the op-by-op types, bit for bit.  -ksp_tfqmr_fused / -ksp_cgs_fused <bool> (default true).  Around
 * the two applications of K = B A an iteration is THREE sweeps of "VecTfqmrFusedOps_C" (include/petsckrylovfused.h):
 *   - tfqmr_qt:     q = u - a v, t = u + q (CGS: and x += a t);
 *   - tfqmr_resid:  r -= a K t with r'r and r'rp, which come home together: the host waits twice per iteration (s = v'rp, then
 *                   these two) where the call-by-call sequence waits three times;
 *   - tfqmr_update: TFQMR's two half steps on d and x, then the new u, q, p.  The half steps' residual estimates depend on scalars only,
 *                   so the host runs both checkpoints FIRST and then launches the one sweep with the half steps that were taken (an
 *                   exit inside them: without the tail).  A monitor that looks at x therefore sees the x of before this iteration's
 *                   half steps; the history, the exits and the x returned are those of the call-by-call sequence.
 * K goes through apply_operator, as in bcgshipmi355x: PCJACOBI on a matrix that offers it: d .* (A x) in the product's own kernel; PCJACOBI / PCNONE
 * otherwise: PCApply fused with s = v'rp ("pmult_dot"); any other PC, or a null space: KSP_PCApplyBAorAB.  The three sweeps do not
 * involve the PC.  Like bcgshipmi355x -- and unlike minreshipmi355x -- the types work on any vectors: without the table, with the option
 * off, or when a sweep answers done = PETSC_FALSE, the same function makes the public calls of the sequence.
 * s == 0 sets KSP_DIVERGED_BREAKDOWN where the reference divides.
 * KSPHIPMI355XGetFusedStepCounts: (fused sweeps run, iterations in which a step ran through the public calls). */
typedef struct { KSPHipCommon common; PetscBool cgs; } KSP_TfqmrHIP;   /* count: (fused sweeps run, iterations with a step through the public calls) */

static PetscErrorCode KSPSetUp_TfqmrHIP(KSP ksp) { return KSPDefaultGetWork(ksp, ((KSP_TfqmrHIP *)ksp->data)->cgs ? 8 : 9); }   /* CGS: no D */
static PetscErrorCode KSPSetFromOptions_TfqmrHIP(KSP ksp) {
  return option_bool(ksp, ((KSP_TfqmrHIP *)ksp->data)->cgs ? "-ksp_cgs_fused" : "-ksp_tfqmr_fused", &COMMON(ksp)->fused);
}
static PetscErrorCode KSPDestroy_TfqmrHIP(KSP ksp) { return ksp_destroy_data(ksp, counts_only); }

static PetscErrorCode KSPSolve_TfqmrHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_TfqmrHIP *td = (KSP_TfqmrHIP *)ksp->data;
  const PetscBool cgs = td->cgs;
  Vec X = ksp->vec_sol, B = ksp->vec_rhs;
  Vec R = ksp->work[0], RP = ksp->work[1], V = ksp->work[2], T = ksp->work[3], Q = ksp->work[4], P = ksp->work[5], U = ksp->work[6], T1 = ksp->work[7];
  Vec D = cgs ? NULL : ksp->work[8], AUQ = V;
  const VecTfqmrFusedOps *M = td->common.fused ? vec_tfqmr_ops(X) : NULL;
  const VecKrylovFusedOps *F = td->common.fused ? vec_fused_ops(X) : NULL;
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscScalar rho = 0.0, rhoold, a, s, b, rr, etaold = 0.0, psiold = 0.0;
  PetscReal dp, dpold, tau;
  PetscInt i;

  if (ksp->pc_side == PC_RIGHT) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s does not support right preconditioning", cgs ? KSPCGSHIPMI355X : KSPTFQMRHIPMI355X);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(F != NULL), X, &pck, &d);CHKERRQ(ierr);
  ksp->its = 0;
  ierr = KSPInitialResidual(ksp, X, V, T, R, B);CHKERRQ(ierr);
  ierr = VecNorm(R, NORM_2, &dp);CHKERRQ(ierr);
  ierr = report(ksp, 0, dp);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, dp);CHKERRQ(ierr);
  if (ksp->reason) return 0;
  ierr = VecCopy(R, RP);CHKERRQ(ierr);
  ierr = VecDot(R, RP, &rhoold);CHKERRQ(ierr);
  ierr = VecCopy(R, U);CHKERRQ(ierr);
  ierr = VecCopy(R, P);CHKERRQ(ierr);
  ierr = apply_operator(ksp, A, F, pck, d, P, V, T1, 1, RP, &s, NULL);CHKERRQ(ierr);    /* V <- K P and s = V'RP of iteration 0 */
  if (!cgs) { ierr = VecSet(D, 0.0);CHKERRQ(ierr); }
  tau = dp; dpold = dp;

  for (i = 0; i < ksp->max_it; i++) {
    PetscBool done = PETSC_FALSE, have_rho = PETSC_FALSE, all_fused = PETSC_TRUE;
    PetscScalar cfm[2] = {0.0, 0.0}, etam[2] = {0.0, 0.0};
    PetscInt nhalves = 0, m;
    if (s == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; break; }
    a = rhoold / s;
    if (M) { ierr = M->tfqmr_qt(U, V, Q, T, cgs ? X : NULL, a, &done);CHKERRQ(ierr); }
    if (done) td->common.count[0]++;
    else {
      all_fused = PETSC_FALSE;
      ierr = VecWAXPY(Q, -a, V, U);CHKERRQ(ierr);
      ierr = VecWAXPY(T, 1.0, U, Q);CHKERRQ(ierr);
      if (cgs) { ierr = VecAXPY(X, a, T);CHKERRQ(ierr); }
    }
    ierr = apply_operator(ksp, A, F, pck, d, T, AUQ, T1, 0, NULL, NULL, NULL);CHKERRQ(ierr);   /* AUQ <- K T */
    done = PETSC_FALSE;
    if (M) { ierr = M->tfqmr_resid(R, AUQ, RP, a, &rr, &rho, &done);CHKERRQ(ierr); }
    if (done) { td->common.count[0]++; dp = PetscSqrtReal(rr); have_rho = PETSC_TRUE; }
    else {
      all_fused = PETSC_FALSE;
      ierr = VecAXPY(R, -a, AUQ);CHKERRQ(ierr);
      if (cgs) { ierr = VecDot(R, RP, &rho);CHKERRQ(ierr); have_rho = PETSC_TRUE; }
      ierr = VecNorm(R, NORM_2, &dp);CHKERRQ(ierr);
    }
    if (cgs) {
      ksp->its = i + 1;
      ierr = report(ksp, i + 1, dp);CHKERRQ(ierr);
      ierr = KSPTestConvergence(ksp, i + 1, dp);CHKERRQ(ierr);
    } else {
      /* the two half steps: scalars and checkpoints now, their vector work in the sweep below */
      for (m = 0; m < 2; m++) {
        const PetscReal w = m ? dp : PetscSqrtReal(dp * dpold), psi = w / tau, cm = 1.0 / PetscSqrtReal(1.0 + psi * psi);
        PetscReal dpest;
        tau = tau * psi * cm;
        etam[m] = cm * cm * a;
        cfm[m] = psiold * psiold * etaold / a;
        nhalves = m + 1;
        dpest = PetscSqrtReal(m + 1.0) * tau;
        ierr = report(ksp, i + 1, dpest);CHKERRQ(ierr);
        ierr = KSPTestConvergence(ksp, i + 1, dpest);CHKERRQ(ierr);
        if (ksp->reason) break;
        etaold = etam[m]; psiold = psi;
      }
      if (!ksp->reason) ksp->its = i + 1;
    }
    if (cgs && ksp->reason) { if (!all_fused) td->common.count[1]++; break; }
    b = 0.0;
    if (!ksp->reason) {
      if (!have_rho) { ierr = VecDot(R, RP, &rho);CHKERRQ(ierr); }
      b = rho / rhoold;
    }
    done = PETSC_FALSE;
    if (M) { ierr = M->tfqmr_update(D, X, U, Q, R, P, nhalves, cfm[0], etam[0], cfm[1], etam[1], (PetscBool)!ksp->reason, b, &done);CHKERRQ(ierr); }
    if (done) td->common.count[0]++;
    else {
      all_fused = PETSC_FALSE;
      for (m = 0; m < nhalves; m++) {
        ierr = VecAYPX(D, cfm[m], m ? Q : U);CHKERRQ(ierr);
        ierr = VecAXPY(X, etam[m], D);CHKERRQ(ierr);
      }
      if (!ksp->reason) {
        ierr = VecWAXPY(U, b, Q, R);CHKERRQ(ierr);
        ierr = VecAXPY(Q, b, P);CHKERRQ(ierr);
        ierr = VecWAXPY(P, b, Q, U);CHKERRQ(ierr);
      }
    }
    if (!all_fused) td->common.count[1]++;
    if (ksp->reason) break;
    ierr = apply_operator(ksp, A, F, pck, d, P, V, T1, 1, RP, &s, NULL);CHKERRQ(ierr);  /* V <- K P and the next s = V'RP */
    rhoold = rho; dpold = dp;
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}

static PetscErrorCode tfqmr_create(KSP ksp, PetscBool cgs) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSP_TfqmrHIP), counts_only);CHKERRQ(ierr);
  COMMON(ksp)->fused = PETSC_TRUE; ((KSP_TfqmrHIP *)ksp->data)->cgs = cgs;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);    /* the one of KSPTFQMR and KSPCGS */
  ksp->ops->setup = KSPSetUp_TfqmrHIP; ksp->ops->solve = KSPSolve_TfqmrHIP; ksp->ops->setfromoptions = KSPSetFromOptions_TfqmrHIP; ksp->ops->destroy = KSPDestroy_TfqmrHIP;
  return 0;
}
PetscErrorCode KSPCreate_TFQMRHIPMI355X(KSP ksp) { return tfqmr_create(ksp, PETSC_FALSE); }
PetscErrorCode KSPCreate_CGSHIPMI355X(KSP ksp) { return tfqmr_create(ksp, PETSC_TRUE); }

/* ================================================================================================ BiCG
 * The sequence of KSPSolve_BiCG (src/ksp/ksp/impls/bicg/bicg.c) as the harness's KSPBICG restates it -- same iterates, histories and exits,
 * bit for bit -- with the vector work of an iteration in the TWO sweeps of "VecBicgFusedOps_C" (include/petsckrylovfused.h) around the
 * products A pr and A^T pl.  -ksp_bicg_fused <bool> (default true).
 *   - bicg_dirs:    pr = zr + b pr, pl = zl + b pl (the copies in the first iteration); no host wait;
 *   - bicg_update:  x += a pr, rr -= a zr, rl -= a zl; with PCJACOBI or PCNONE also zr = B rr, zl = B^T rl, the next beta = zr'rl and the
 *                   norm's sum in the same pass -- the host waits twice per iteration (dpi = zr'pl, then these sums).  Any other PC: the
 *                   sweep returns rr'rr, KSP_PCApply / PCApplyTranspose follow, then VecNorm(Zr) (preconditioned norm) and VecDot(Zr, Rl).
 * With the unpreconditioned norm the reference applies the preconditioner after the checkpoint; the folded form has zr and zl already
 * (work vectors only: an exit at that checkpoint leaves x and the history as they are).
 * Without the table, with the option off, or when a sweep answers done = PETSC_FALSE, the same function makes the public calls.
 * Left preconditioning; a null space is PETSC_ERR_SUP at set-up; beta == 0 in the first iteration and dpi == 0 set KSP_DIVERGED_BREAKDOWN.
 * KSPHIPMI355XGetFusedStepCounts: (fused sweeps run, iterations in which a step ran through the public calls).  bicg_dirs runs once per
 * iteration entered, bicg_update once per iteration that gets past dpi: 2 its sweeps, and 2 its + 1 after a breakdown at dpi == 0. */
/* KSP_MatMultTranspose / KSP_PCApplyTranspose of kspimpl.h.  On the harness the plug-in dispatches through the function tables it can see,
 * as an implementation does (the library exports the two for the harness's own KSPBICG) */
static PetscErrorCode bicg_mult_transpose(KSP ksp, Mat A, Vec x, Vec y) {
#if defined(PETSCHIPMI355X_WITH_PETSC)
  return KSP_MatMultTranspose(ksp, A, x, y);
#else
  PetscErrorCode ierr;
  if (x == y) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_IDN, "x and y must be different vectors");
  if (!A->ops->multtranspose) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "This matrix type does not have a multiply tranpose defined");
  ierr = (*A->ops->multtranspose)(A, x, y);CHKERRQ(ierr);
  HipStateIncrease(y);
  return 0;
#endif
}
static PetscErrorCode bicg_pc_apply_transpose(KSP ksp, Vec x, Vec y) {
#if defined(PETSCHIPMI355X_WITH_PETSC)
  return KSP_PCApplyTranspose(ksp, x, y);
#else
  PetscErrorCode ierr;
  if (x == y) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_IDN, "x and y must be different vectors");
  if (!ksp->pc->ops->applytranspose) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "PC does not have apply transpose");
  ierr = (*ksp->pc->ops->applytranspose)(ksp->pc, x, y);CHKERRQ(ierr);
  return 0;
#endif
}
static PetscErrorCode KSPSetUp_BicgHIP(KSP ksp) {
  if (ksp->pc_side == PC_RIGHT || ksp->pc_side == PC_SYMMETRIC) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s: left preconditioning only", KSPBICGHIPMI355X);
  if (has_null_space(ksp)) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s with a null space: there is no removal behind the transposed preconditioner application", KSPBICGHIPMI355X);
  return KSPDefaultGetWork(ksp, 6);
}
static PetscErrorCode KSPSetFromOptions_BicgHIP(KSP ksp) { return option_bool(ksp, "-ksp_bicg_fused", &COMMON(ksp)->fused); }
static PetscErrorCode KSPDestroy_BicgHIP(KSP ksp) { return ksp_destroy_data(ksp, counts_only); }
static PetscErrorCode bicg_precondition(KSP ksp, Vec Rr, Vec Rl, Vec Zr, Vec Zl) {
  PetscErrorCode ierr = KSP_PCApply(ksp, Rr, Zr);CHKERRQ(ierr);
  return bicg_pc_apply_transpose(ksp, Rl, Zl);
}
static PetscErrorCode KSPSolve_BicgHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSPHipCommon *bd = COMMON(ksp);      /* all this type keeps; count: (fused sweeps run, iterations with a step through the public calls) */
  Vec X = ksp->vec_sol, B = ksp->vec_rhs;
  Vec Rr = ksp->work[0], Rl = ksp->work[1], Zr = ksp->work[2], Zl = ksp->work[3], Pr = ksp->work[4], Pl = ksp->work[5];
  const VecBicgFusedOps *M = bd->fused ? vec_bicg_ops(X) : NULL;
  const PetscBool pnorm = (PetscBool)(ksp->normtype == KSP_NORM_PRECONDITIONED);
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscScalar dpi, a, beta = 0.0, betaold = 1.0, nrm2 = 0.0;
  PetscBool have_beta = PETSC_FALSE;
  PetscReal dp;
  PetscInt i;

  if (has_null_space(ksp)) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s with a null space: there is no removal behind the transposed preconditioner application", KSPBICGHIPMI355X);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(M != NULL), X, &pck, &d);CHKERRQ(ierr);     /* (no null space here: refused above) */
  ksp->its = 0;
  ierr = start_residual(ksp, A, X, B, Rr);CHKERRQ(ierr);
  ierr = VecCopy(Rr, Rl);CHKERRQ(ierr);
  ierr = bicg_precondition(ksp, Rr, Rl, Zr, Zl);CHKERRQ(ierr);
  ierr = VecNorm(pnorm ? Zr : Rr, NORM_2, &dp);CHKERRQ(ierr);
  ierr = report(ksp, 0, dp);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, dp);CHKERRQ(ierr);
  if (ksp->reason) return 0;

  for (i = 0; i < ksp->max_it; i++) {
    PetscBool done = PETSC_FALSE, all_fused = PETSC_TRUE, folded = PETSC_FALSE;
    PetscScalar b;
    if (!have_beta) { ierr = VecDot(Zr, Rl, &beta);CHKERRQ(ierr); }
    if (!i && beta == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; return 0; }
    b = i ? beta / betaold : 0.0;
    if (M) { ierr = M->bicg_dirs(Pr, Pl, Zr, Zl, b, (PetscBool)!i, &done);CHKERRQ(ierr); }
    if (done) bd->count[0]++;
    else {
      all_fused = PETSC_FALSE;
      if (!i) { ierr = VecCopy(Zr, Pr);CHKERRQ(ierr); ierr = VecCopy(Zl, Pl);CHKERRQ(ierr); }
      else { ierr = VecAYPX(Pr, b, Zr);CHKERRQ(ierr); ierr = VecAYPX(Pl, b, Zl);CHKERRQ(ierr); }
    }
    betaold = beta; have_beta = PETSC_FALSE;
    ierr = KSP_MatMult(ksp, A, Pr, Zr);CHKERRQ(ierr);
    ierr = bicg_mult_transpose(ksp, A, Pl, Zl);CHKERRQ(ierr);
    ierr = VecDot(Zr, Pl, &dpi);CHKERRQ(ierr);
    if (dpi == 0.0) { ksp->reason = KSP_DIVERGED_BREAKDOWN; if (!all_fused) bd->count[1]++; break; }
    a = beta / dpi;
    done = PETSC_FALSE;
    if (M) { ierr = M->bicg_update(X, Rr, Rl, Pr, Zr, Zl, d, (PetscBool)(pck == PCKIND_IDENTITY), a, pnorm ? 0 : 1, &beta, &nrm2, &done);CHKERRQ(ierr); }
    if (done) {
      bd->count[0]++;
      folded = (PetscBool)(pck != PCKIND_GENERAL);
      if (folded) { have_beta = PETSC_TRUE; dp = PetscSqrtReal(nrm2); }
      else if (pnorm) { ierr = bicg_precondition(ksp, Rr, Rl, Zr, Zl);CHKERRQ(ierr); ierr = VecNorm(Zr, NORM_2, &dp);CHKERRQ(ierr); }
      else dp = PetscSqrtReal(nrm2);
    } else {
      all_fused = PETSC_FALSE;
      ierr = VecAXPY(X, a, Pr);CHKERRQ(ierr);
      ierr = VecAXPY(Rr, -a, Zr);CHKERRQ(ierr);
      ierr = VecAXPY(Rl, -a, Zl);CHKERRQ(ierr);
      if (pnorm) { ierr = bicg_precondition(ksp, Rr, Rl, Zr, Zl);CHKERRQ(ierr); }
      ierr = VecNorm(pnorm ? Zr : Rr, NORM_2, &dp);CHKERRQ(ierr);
    }
    if (!all_fused) bd->count[1]++;
    ksp->its = i + 1;
    ierr = report(ksp, i + 1, dp);CHKERRQ(ierr);
    ierr = KSPTestConvergence(ksp, i + 1, dp);CHKERRQ(ierr);
    if (ksp->reason) break;
    if (!pnorm && !folded) { ierr = bicg_precondition(ksp, Rr, Rl, Zr, Zl);CHKERRQ(ierr); }
  }
  if (i >= ksp->max_it) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_BICGHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSPHipCommon), counts_only);CHKERRQ(ierr);
  COMMON(ksp)->fused = PETSC_TRUE;
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);      /* the two of KSPBICG */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_BicgHIP; ksp->ops->solve = KSPSolve_BicgHIP; ksp->ops->setfromoptions = KSPSetFromOptions_BicgHIP; ksp->ops->destroy = KSPDestroy_BicgHIP;
  return 0;
}

/* ================================================================================================ LSQR
 * The sequence of KSPSolve_LSQR (src/ksp/ksp/impls/lsqr/lsqr.c) as the harness's KSPLSQR restates it -- rectangular operators, work vectors
 * from MatGetVecs(A), the unpreconditioned norm (the recurrence's estimate of ||b - A x||), a preconditioner on the normal equations, the
 * same exits (the happy-breakdown one included) -- same iterates, histories and estimates, bit for bit.  Behind the two
 * products an iteration's vector work is the two sweeps of "VecLsqrFusedOps_C" (include/petsckrylovfused.h):
 *   PCNONE:   u1 = A v ; lsqr_bidiag QUEUE (u1 -= alpha u, |u1|^2 into a device slot, u1 normalised from the slot) ; v1 = A^T u1, queued
 *             without a wait ; lsqr_bidiag FINISH (v1 -= beta v with beta rooted from the slot on the device, |v1|^2) -- beta^2 and alpha^2
 *             come home together, the iteration's ONE wait ; the Givens scalars on the host ; lsqr_update (v1 /= alpha, x, the standard-error
 *             sum, w).  5 launches besides the products: the two sweeps, the scaling, the publish kernel, the update.  A beta == 0 found at that wait has cost one product on work
 *             vectors and nothing in x.
 *   other PC: the row-space side through lsqr_bidiag WAIT (beta comes home), steps 6-7 through VecAXPY, KSP_PCApply and VecDot, and the
 *             update sweep takes Z1 with its scaling.  Two waits.
 * VecScale is not among the calls this library takes from PETSc: the scalings outside the sweeps (the solve start, u1 and v1 in the mixed
 * route) are the update sweep's scaling form, so like minreshipmi355x the type has no op-by-op route and KSPSetUp returns PETSC_ERR_SUP on
 * vectors without the table (-ksp_type lsqr is that route).  On several ranks the Vec type refuses the slot routes (the slot would hold a
 * local partial sum): both sweeps take the WAIT route, the sums are all-reduced, step 6 takes beta from the host -- two waits.
 * KSPHIPMI355XGetFusedStepCounts: (bidiagonalisation sweeps run, update sweeps run; the scaling forms are not counted). */
typedef struct { KSPHipCommon common; Vec se; PetscBool se_flg; PetscReal arnorm, anorm, rhs_norm; Vec U, U1, V, V1, W, Z, Z1; } KSP_LsqrHIP;   /* dinv, fused: unused */

static PetscErrorCode lsqr_no_pc(KSP ksp, PetscBool *nopc) {
  PCType t = NULL;
  PetscErrorCode ierr = PCGetType(ksp->pc, &t);CHKERRQ(ierr);
  *nopc = (PetscBool)(t && !strcmp(t, PCNONE));
  return 0;
}
static PetscErrorCode lsqr_get_work(KSP ksp) {   /* what this configuration needs and does not have yet; set-up and solve both ask */
  KSP_LsqrHIP *ld = (KSP_LsqrHIP *)ksp->data;
  PetscErrorCode ierr;
  PetscBool nopc;
  Mat A;
  Vec right = NULL, left = NULL;
  Vec *m_side[] = {&ld->U, &ld->U1}, *n_side[] = {&ld->V, &ld->V1, &ld->W, &ld->Z, &ld->Z1, &ld->se};
  ierr = lsqr_no_pc(ksp, &nopc);CHKERRQ(ierr);
  const PetscBool n_needed[] = {PETSC_TRUE, PETSC_TRUE, PETSC_TRUE, (PetscBool)!nopc, (PetscBool)!nopc, ld->se_flg};
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = MatGetVecs(A, &right, &left);CHKERRQ(ierr);
  for (int k = 0; k < 2; k++) if (!*m_side[k]) { ierr = VecDuplicate(left, m_side[k]);CHKERRQ(ierr); }
  for (int k = 0; k < 6; k++) if (n_needed[k] && !*n_side[k]) { ierr = VecDuplicate(right, n_side[k]);CHKERRQ(ierr); }
  ierr = VecDestroy(&right);CHKERRQ(ierr);
  ierr = VecDestroy(&left);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode lsqr_check(KSP ksp) {
  PetscErrorCode ierr;
  PetscBool nopc;
  Mat A, Pm;
  if (has_null_space(ksp)) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s with a null space: there is no removal behind the transposed product", KSPLSQRHIPMI355X);
  if (ksp->pc_side == PC_RIGHT || ksp->pc_side == PC_SYMMETRIC) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "KSP type %s: left preconditioning (of the normal equations) only", KSPLSQRHIPMI355X);
  ierr = lsqr_no_pc(ksp, &nopc);CHKERRQ(ierr);
  ierr = PCGetOperators(ksp->pc, &A, &Pm, NULL);CHKERRQ(ierr);
  if (!nopc && (Pm->rmap->N != A->cmap->N || Pm->cmap->N != A->cmap->N)) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_SIZ, "KSP type %s preconditions the normal equations: the preconditioner matrix must be %d x %d, it is %d x %d", KSPLSQRHIPMI355X, (int)A->cmap->N, (int)A->cmap->N, (int)Pm->rmap->N, (int)Pm->cmap->N);
  return 0;
}
static PetscErrorCode lsqr_needs_table(KSP ksp) {
  const KSP_LsqrHIP *ld = (const KSP_LsqrHIP *)ksp->data;
  const PetscBool offered = (PetscBool)(vec_lsqr_ops(ld->V) && vec_lsqr_ops(ld->U) && (!ksp->vec_sol || vec_lsqr_ops(ksp->vec_sol)) && (!ksp->vec_rhs || vec_lsqr_ops(ksp->vec_rhs)));
  return needs_table(ksp, offered, KSPLSQRHIPMI355X, "LSQR sweeps", "VecLsqrFusedOps_C", "lsqr");
}
static PetscErrorCode KSPSetUp_LsqrHIP(KSP ksp) {
  PetscErrorCode ierr = lsqr_check(ksp);CHKERRQ(ierr);
  ierr = lsqr_get_work(ksp);CHKERRQ(ierr);
  return lsqr_needs_table(ksp);
}
static PetscErrorCode KSPSetFromOptions_LsqrHIP(KSP ksp) { return option_bool(ksp, "-ksp_lsqr_set_standard_error", &((KSP_LsqrHIP *)ksp->data)->se_flg); }
static PetscErrorCode KSPLSQRSetStandardErrorVec_LsqrHIP(KSP ksp, Vec se) {
  KSP_LsqrHIP *ld = (KSP_LsqrHIP *)ksp->data;
  if (se == ld->se) return 0;
  PetscErrorCode ierr = VecDestroy(&ld->se);CHKERRQ(ierr);
  ld->se = se;
  return 0;
}
static PetscErrorCode KSPLSQRGetStandardErrorVec_LsqrHIP(KSP ksp, Vec *se) { *se = ((KSP_LsqrHIP *)ksp->data)->se; return 0; }
static PetscErrorCode KSPLSQRGetArnorm_LsqrHIP(KSP ksp, PetscReal *arnorm, PetscReal *rhs_norm, PetscReal *anorm) {
  const KSP_LsqrHIP *ld = (const KSP_LsqrHIP *)ksp->data;
  *arnorm = ld->arnorm; *rhs_norm = ld->rhs_norm; *anorm = ld->anorm;
  return 0;
}
static PetscErrorCode KSPDefaultPCNone_LsqrHIP(KSP ksp) { (void)ksp; return 0; }   /* its presence is the message: see the harness's KSPSetUp */
static const KSPHipMethod lsqr_methods[] = {
  {"KSPLSQRSetStandardErrorVec_C", "KSPLSQRSetStandardErrorVec_LsqrHIP", (PetscVoidFunction)KSPLSQRSetStandardErrorVec_LsqrHIP},
  {"KSPLSQRGetStandardErrorVec_C", "KSPLSQRGetStandardErrorVec_LsqrHIP", (PetscVoidFunction)KSPLSQRGetStandardErrorVec_LsqrHIP},
  {"KSPLSQRGetArnorm_C", "KSPLSQRGetArnorm_LsqrHIP", (PetscVoidFunction)KSPLSQRGetArnorm_LsqrHIP},
  COUNTS_METHOD,                                                                    /* count: (bidiagonalisation sweeps run, update sweeps run) */
  {"KSPDefaultPCNone_C", "KSPDefaultPCNone_LsqrHIP", (PetscVoidFunction)KSPDefaultPCNone_LsqrHIP},
  {NULL, NULL, NULL}};
static PetscErrorCode KSPDestroy_LsqrHIP(KSP ksp) {
  KSP_LsqrHIP *ld = (KSP_LsqrHIP *)ksp->data;
  PetscErrorCode ierr;
  if (!ld) return 0;
  Vec *all[] = {&ld->U, &ld->U1, &ld->V, &ld->V1, &ld->W, &ld->Z, &ld->Z1, &ld->se};
  for (int k = 0; k < 8; k++) { ierr = VecDestroy(all[k]);CHKERRQ(ierr); }
  return ksp_destroy_data(ksp, lsqr_methods);
}
#define LSQR_REFUSED(ksp) SETERRQ(HipObjComm(ksp), PETSC_ERR_SUP, "the fused LSQR sweep refused these vectors; use -ksp_type lsqr")
/* v = a v through the update sweep's scaling form (a == 1: nothing) */
static PetscErrorCode lsqr_scale(KSP ksp, const VecLsqrFusedOps *L, Vec v, PetscScalar a) {
  PetscBool done;
  PetscErrorCode ierr = L->lsqr_update(v, NULL, NULL, NULL, a, 0.0, 0.0, 0.0, PETSC_TRUE, &done);CHKERRQ(ierr);
  if (!done) LSQR_REFUSED(ksp);
  return 0;
}
static PetscErrorCode KSPSolve_LsqrHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_LsqrHIP *ld = (KSP_LsqrHIP *)ksp->data;
  Vec X = ksp->vec_sol, B = ksp->vec_rhs, U, U1, V, V1, W, Z, Z1, SE, t;
  const VecLsqrFusedOps *L;
  Mat A;
  PetscBool nopc, done, one_wait = PETSC_TRUE;                       /* until the Vec type refuses the slot route (several ranks) */
  PetscScalar alpha, beta, rho, rhobar, phi, phibar, theta, c, s, dot, sums[2];
  PetscReal anorm2;
  PetscInt i;

  ierr = lsqr_check(ksp);CHKERRQ(ierr);
  ierr = lsqr_get_work(ksp);CHKERRQ(ierr);
  ierr = lsqr_needs_table(ksp);CHKERRQ(ierr);
  ierr = lsqr_no_pc(ksp, &nopc);CHKERRQ(ierr);
  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  if (B->map->n != A->rmap->n || X->map->n != A->cmap->n) SETERRQ(HipObjComm(ksp), PETSC_ERR_ARG_SIZ, "KSP type %s: b must have the rows of A (%d, it has %d) and x its columns (%d, it has %d)", KSPLSQRHIPMI355X, (int)A->rmap->n, (int)B->map->n, (int)A->cmap->n, (int)X->map->n);
  U = ld->U; U1 = ld->U1; V = ld->V; V1 = ld->V1; W = ld->W; Z = ld->Z; Z1 = ld->Z1; SE = ld->se;
  L = vec_lsqr_ops(X);
  ksp->its = 0;
  ierr = start_residual(ksp, A, X, B, U);CHKERRQ(ierr);
  ierr = VecNorm(U, NORM_2, &beta);CHKERRQ(ierr);
  ld->rhs_norm = beta; ld->arnorm = 0.0; ld->anorm = 0.0;
  ierr = report(ksp, 0, beta);CHKERRQ(ierr);
  ierr = KSPTestConvergence(ksp, 0, beta);CHKERRQ(ierr);
  if (ksp->reason) return 0;
  ierr = lsqr_scale(ksp, L, U, beta != 0.0 ? 1.0 / beta : 1.0);CHKERRQ(ierr);
  ierr = bicg_mult_transpose(ksp, A, U, V);CHKERRQ(ierr);
  if (nopc) { ierr = VecNorm(V, NORM_2, &alpha);CHKERRQ(ierr); }
  else {
    ierr = KSP_PCApply(ksp, V, Z);CHKERRQ(ierr);
    ierr = VecDot(V, Z, &dot);CHKERRQ(ierr);
    alpha = PetscSqrtReal(dot);
    ierr = lsqr_scale(ksp, L, Z, alpha != 0.0 ? 1.0 / alpha : 1.0);CHKERRQ(ierr);
  }
  if (alpha == 0.0) { ksp->reason = KSP_CONVERGED_ATOL_NORMAL; return 0; }
  ierr = lsqr_scale(ksp, L, V, 1.0 / alpha);CHKERRQ(ierr);
  ierr = VecCopy(nopc ? V : Z, W);CHKERRQ(ierr);
  if (SE) { ierr = VecSet(SE, 0.0);CHKERRQ(ierr); }
  phibar = beta; rhobar = alpha; anorm2 = alpha * alpha;
  ld->arnorm = alpha * beta; ld->anorm = PetscSqrtReal(anorm2);

  for (i = 0; i < ksp->max_it; i++) {
    PetscBool broke;
    ierr = KSP_MatMult(ksp, A, nopc ? V : Z, U1);CHKERRQ(ierr);
    done = PETSC_FALSE;
    if (nopc && one_wait) { ierr = L->lsqr_bidiag(U, U1, alpha, LSQR_BIDIAG_QUEUE, sums, &done);CHKERRQ(ierr); one_wait = done; }
    if (nopc && one_wait) {
      ierr = bicg_mult_transpose(ksp, A, U1, V1);CHKERRQ(ierr);
      ierr = L->lsqr_bidiag(V, V1, 0.0, LSQR_BIDIAG_FINISH, sums, &done);CHKERRQ(ierr);
      if (!done) LSQR_REFUSED(ksp);
      ld->common.count[0] += 2;
      beta = PetscSqrtReal(sums[0]); alpha = PetscSqrtReal(sums[1]);
    } else if (nopc) {                                               /* several ranks: both sums all-reduced, beta and alpha come home one by one */
      ierr = L->lsqr_bidiag(U, U1, alpha, LSQR_BIDIAG_WAIT, sums, &done);CHKERRQ(ierr);
      if (!done) LSQR_REFUSED(ksp);
      beta = PetscSqrtReal(sums[0]);
      ierr = lsqr_scale(ksp, L, U1, beta != 0.0 ? 1.0 / beta : 1.0);CHKERRQ(ierr);
      ierr = bicg_mult_transpose(ksp, A, U1, V1);CHKERRQ(ierr);
      ierr = L->lsqr_bidiag(V, V1, beta, LSQR_BIDIAG_WAIT, sums, &done);CHKERRQ(ierr);
      if (!done) LSQR_REFUSED(ksp);
      ld->common.count[0] += 2;
      alpha = PetscSqrtReal(sums[0]);
    } else {
      ierr = L->lsqr_bidiag(U, U1, alpha, LSQR_BIDIAG_WAIT, sums, &done);CHKERRQ(ierr);
      if (!done) LSQR_REFUSED(ksp);
      ld->common.count[0]++;
      beta = PetscSqrtReal(sums[0]);
      ierr = lsqr_scale(ksp, L, U1, beta != 0.0 ? 1.0 / beta : 1.0);CHKERRQ(ierr);
      ierr = bicg_mult_transpose(ksp, A, U1, V1);CHKERRQ(ierr);
      ierr = VecAXPY(V1, -beta, V);CHKERRQ(ierr);
      ierr = KSP_PCApply(ksp, V1, Z1);CHKERRQ(ierr);
      ierr = VecDot(V1, Z1, &dot);CHKERRQ(ierr);
      alpha = PetscSqrtReal(dot);
      ierr = lsqr_scale(ksp, L, V1, alpha != 0.0 ? 1.0 / alpha : 1.0);CHKERRQ(ierr);
    }
    broke = (PetscBool)(beta == 0.0 || alpha == 0.0);
    rho = PetscSqrtReal(rhobar * rhobar + beta * beta);
    c = rhobar / rho; s = beta / rho;
    theta = s * alpha; rhobar = -c * alpha;
    phi = c * phibar; phibar = s * phibar;
    ierr = L->lsqr_update(nopc ? V1 : Z1, X, W, SE, alpha != 0.0 ? 1.0 / alpha : 1.0, phi / rho, -theta / rho, 1.0 / (rho * rho), broke, &done);CHKERRQ(ierr);
    if (!done) LSQR_REFUSED(ksp);
    ld->common.count[1]++;
    ld->arnorm = alpha * PetscAbsScalar(s * phi);
    anorm2 += alpha * alpha + beta * beta;
    ld->anorm = PetscSqrtReal(anorm2);
    ksp->its = i + 1;
    ierr = report(ksp, i + 1, phibar);CHKERRQ(ierr);
    ierr = KSPTestConvergence(ksp, i + 1, phibar);CHKERRQ(ierr);
    if (broke && !ksp->reason) ksp->reason = KSP_CONVERGED_HAPPY_BREAKDOWN;
    if (ksp->reason) break;
    t = U; U = U1; U1 = t; t = V; V = V1; V1 = t; t = Z; Z = Z1; Z1 = t;
  }
  if (i >= ksp->max_it && !ksp->reason) ksp->reason = KSP_DIVERGED_ITS;
  return 0;
}
PetscErrorCode KSPCreate_LSQRHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSP_LsqrHIP), lsqr_methods);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);    /* the one of KSPLSQR */
  ksp->ops->setup = KSPSetUp_LsqrHIP; ksp->ops->solve = KSPSolve_LsqrHIP; ksp->ops->setfromoptions = KSPSetFromOptions_LsqrHIP; ksp->ops->destroy = KSPDestroy_LsqrHIP;
  return 0;
}

typedef struct { KSPHipCommon common; PetscReal scale; } KSP_RichHIP;

static PetscErrorCode KSPRichardsonSetScale_RichHIP(KSP ksp, PetscReal scale) { ((KSP_RichHIP *)ksp->data)->scale = scale; return 0; }
static PetscErrorCode KSPSetUp_RichHIP(KSP ksp) { return KSPDefaultGetWork(ksp, 2); }
static PetscErrorCode KSPSetFromOptions_RichHIP(KSP ksp) {
  PetscReal v[2]; int count;
  PetscErrorCode ierr = option_reals(ksp, "-ksp_richardson_scale", v, &count);CHKERRQ(ierr);
  if (count) ((KSP_RichHIP *)ksp->data)->scale = v[0];
  return 0;
}
static const KSPHipMethod rich_methods[] = {
  {"KSPRichardsonSetScale_C", "KSPRichardsonSetScale_RichHIP", (PetscVoidFunction)KSPRichardsonSetScale_RichHIP},
  {NULL, NULL, NULL}};
static PetscErrorCode KSPDestroy_RichHIP(KSP ksp) { return ksp_destroy_data(ksp, rich_methods); }

static PetscErrorCode KSPSolve_RichHIP(KSP ksp) {
  PetscErrorCode ierr;
  KSP_RichHIP *ri = (KSP_RichHIP *)ksp->data;
  const KSPNormType nt = ksp->normtype;
  Vec x = ksp->vec_sol, rhs = ksp->vec_rhs, r = ksp->work[0], z = ksp->work[1];
  const VecKrylovFusedOps *F = vec_fused_ops(x);
  HipPCKind pck;
  Vec d;
  Mat A;
  PetscReal rn = 0.0;
  PetscBool product_only = PETSC_FALSE;   /* r holds A x, not yet rhs - A x: the sweep of the coming iteration forms the residual itself */
  PetscInt i;

  ierr = PCGetOperators(ksp->pc, &A, NULL, NULL);CHKERRQ(ierr);
  ierr = pc_diagonal_form(ksp, (PetscBool)(nt == KSP_NORM_NONE && F && F->rich_step), x, &pck, &d);CHKERRQ(ierr);
  ierr = start_residual(ksp, A, x, rhs, r);CHKERRQ(ierr);
  ksp->its = 0;
  for (i = 0; i < ksp->max_it; i++) {
    PetscBool done = PETSC_FALSE;
    if (nt == KSP_NORM_UNPRECONDITIONED) {
      ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr);
      ierr = report(ksp, i, rn);CHKERRQ(ierr);
      ierr = KSPTestConvergence(ksp, i, rn);CHKERRQ(ierr);
      if (ksp->reason) break;
    }
    if (product_only) {                                                                  /* r = rhs - r, z = B r, x += scale z in one sweep */
      ierr = F->rich_step(x, NULL, NULL, r, rhs, d, ri->scale, &done);CHKERRQ(ierr);
      if (!done) { ierr = VecAYPX(r, -1.0, rhs);CHKERRQ(ierr); }
    }
    if (!done) {
      ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr);
      if (nt == KSP_NORM_PRECONDITIONED) {
        ierr = VecNorm(z, NORM_2, &rn);CHKERRQ(ierr);
        ierr = report(ksp, i, rn);CHKERRQ(ierr);
        ierr = KSPTestConvergence(ksp, i, rn);CHKERRQ(ierr);
        if (ksp->reason) break;
      }
      ierr = VecAXPY(x, ri->scale, z);CHKERRQ(ierr);
    }
    ksp->its++;
    product_only = PETSC_FALSE;
    if (i + 1 < ksp->max_it || nt != KSP_NORM_NONE) {
      ierr = KSP_MatMult(ksp, A, x, r);CHKERRQ(ierr);
      if (pck != PCKIND_GENERAL) product_only = PETSC_TRUE;                              /* (KSP_NORM_NONE: another iteration follows) */
      else { ierr = VecAYPX(r, -1.0, rhs);CHKERRQ(ierr); }
    }
  }
  if (!ksp->reason) {
    if (nt != KSP_NORM_NONE) {
      if (nt == KSP_NORM_UNPRECONDITIONED) { ierr = VecNorm(r, NORM_2, &rn);CHKERRQ(ierr); }
      else { ierr = KSP_PCApply(ksp, r, z);CHKERRQ(ierr); ierr = VecNorm(z, NORM_2, &rn);CHKERRQ(ierr); }
      ierr = report(ksp, ksp->its, rn);CHKERRQ(ierr);
    }
    ierr = stationary_out_of_iterations(ksp, rn);CHKERRQ(ierr);
  }
  return 0;
}

PetscErrorCode KSPCreate_RichardsonHIPMI355X(KSP ksp) {
  PetscErrorCode ierr = ksp_create_data(ksp, sizeof(KSP_RichHIP), rich_methods);CHKERRQ(ierr);
  ((KSP_RichHIP *)ksp->data)->scale = 1.0;                                               /* KSPCreate_Richardson's default */
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_PRECONDITIONED, PC_LEFT, 2);CHKERRQ(ierr);
  ierr = KSPSetSupportedNorm(ksp, KSP_NORM_UNPRECONDITIONED, PC_LEFT, 1);CHKERRQ(ierr);
  ksp->ops->setup = KSPSetUp_RichHIP; ksp->ops->solve = KSPSolve_RichHIP; ksp->ops->setfromoptions = KSPSetFromOptions_RichHIP; ksp->ops->destroy = KSPDestroy_RichHIP;
  return 0;
}
