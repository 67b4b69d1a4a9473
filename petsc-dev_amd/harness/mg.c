/* PCMG (src/ksp/pc/impls/mg/mg.c, mgfunc.c, smg.c, fmg.c): multigrid cycles over level KSPs.  Level 0 is the coarsest, level n-1 the PC's
 * own operator (pc->mat for the residual, pc->pmat for the smoother).  Control flow only: every step of a cycle is a public call of this
 * library -- KSPSolve, MatResidual, MatRestrict, VecSet, MatInterpolateAdd -- so a cycle equals that sequence of calls bit for bit
 * whatever Vec / Mat types run underneath.  The sequence ("PCMG"):
 *
 *   cycle(l):  KSPSolve(down_l, b_l, x_l);  l == 0: return                     the coarse solve
 *              residual_l(A_l, b_l, x_l, r_l);  MatRestrict(R_l, r_l, b_{l-1});  VecSet(x_{l-1}, 0)
 *              cycle(l-1), once for a V cycle or when l-1 == 0, twice for a W cycle
 *              MatInterpolateAdd(P_l, x_{l-1}, x_l, x_l);  KSPSolve(up_l, b_l, x_l)
 *   multiplicative:  b_{n-1} = b, x_{n-1} = 0, `cycles` times cycle(n-1), y = x_{n-1}
 *   additive:        b restricted down through all levels, every level solved by its down solver from x_l = 0, interpolate-add upwards
 *   full:            b restricted down, coarse solve, then for l = 1 .. n-1: MatInterpolate(P_l, x_{l-1}, x_l), cycle(l)
 *
 * Smoothers default to KSPRICHARDSON + PCSOR without a norm, one step, nonzero initial guess: one smoothing step is one MatSOR through
 * PCApplyRichardson_SOR.  The coarse solver defaults to KSPPREONLY + the PC default from a zero guess (there is no LU here: ILU(0) is exact
 * on a tridiagonal coarse matrix, -mg_coarse_pc_factor_levels k >= the coarse size is a complete LU).  Every solve below the top starts from
 * x = 0, so the preconditioner is a fixed linear map whenever the level solvers are.  No applytranspose, no applyrichardson, no Kaskade. */
#include "petscimpl.h"

typedef struct {
  KSP smoothd, smoothu;        /* smoothu == smoothd until a second one is asked for */
  Vec b, x, r;
  Mat interpolate, restrct;    /* the user's, each with a reference of the PC's own; NULL: the other one serves (mg_interp, mg_restr) */
  PetscBool optd, optu;        /* the options of smoothd / smoothu were read (at the solver's first set-up, never again) */
  Mat A;                       /* level < n-1 with Galerkin: P^T A P, the PC's own */
  PetscBool Aready;            /* A was handed over just computed (PCMGAdoptGalerkin_Private): the next set-up takes it as it is */
  PCMGResidualFn residual; Mat resmat;   /* PCMGSetResidual; NULL: MatResidual on the level's operator */
} PC_MG_Level;
typedef struct {
  PetscInt n;
  PC_MG_Level *lev;
  PCMGType am;
  PCMGCycleType cycle;
  PetscInt cycles;             /* multiplicative cycles per application */
  PetscBool galerkin;
  void *layer;                 /* the data of a type built on this one (PCGAMG, gamg.c); NULL for a plain PCMG */
} PC_MG;
static PetscErrorCode PCApply_MG(PC pc, Vec b, Vec y);

#define PCMGValid(pc, mg) do { \
  if (!(pc)) SETERRQ(0, PETSC_ERR_ARG_NULL, "Null PC"); \
  if (strcmp((pc)->type_name, PCMG) && (pc)->ops->apply != PCApply_MG) SETERRQ((pc)->comm, PETSC_ERR_ARG_WRONG, "PC of type %s is not a PCMG", (pc)->type_name); \
  (mg) = (PC_MG *)(pc)->data; } while (0)
#define PCMGLevel(pc, mg, l) do { \
  if (!(mg)->n) SETERRQ((pc)->comm, PETSC_ERR_ORDER, "PCMGSetLevels() first"); \
  if ((l) < 0 || (l) >= (mg)->n) SETERRQ((pc)->comm, PETSC_ERR_ARG_OUTOFRANGE, "level %d of %d", (int)(l), (int)(mg)->n); } while (0)

PetscErrorCode PCMGDefaultResidual(Mat A, Vec b, Vec x, Vec r) { return MatResidual(A, b, x, r); }
/* each transfer defaults to the other at the time of use, so setting either one later changes exactly what it names */
static Mat mg_interp(const PC_MG_Level *v) { return v->interpolate ? v->interpolate : v->restrct; }
static Mat mg_restr(const PC_MG_Level *v) { return v->restrct ? v->restrct : v->interpolate; }
static PetscErrorCode mg_hold(Mat *slot, Mat mat) {   /* PetscObjectReference on the new one, MatDestroy on the one it replaces */
  PetscErrorCode ierr;
  if (mat) mat->xrefs++;
  ierr = MatDestroy(slot);CHKERRQ(ierr);
  *slot = mat;
  return 0;
}

static PetscErrorCode mg_level_prefix(PC pc, PetscInt l, PetscBool generic, char out[], size_t len) {
  if (strlen(pc->prefix) + sizeof("mg_levels_000_") > sizeof(pc->prefix)) SETERRQ(pc->comm, PETSC_ERR_ARG_SIZ, "The options prefix %s leaves no room for the level solvers' mg_levels_<l>_", pc->prefix);
  if (l == 0) snprintf(out, len, "%smg_coarse_", pc->prefix);
  else if (generic) snprintf(out, len, "%smg_levels_", pc->prefix);
  else snprintf(out, len, "%smg_levels_%d_", pc->prefix, (int)l);
  return 0;
}
static PetscErrorCode mg_smoother_defaults(KSP ksp, PetscInt its) {
  PC sub;
  PetscErrorCode ierr = KSPSetType(ksp, KSPRICHARDSON);CHKERRQ(ierr);
  ierr = KSPGetPC(ksp, &sub);CHKERRQ(ierr);
  ierr = PCSetType(sub, PCSOR);CHKERRQ(ierr);
  ierr = KSPSetNormType(ksp, KSP_NORM_NONE);CHKERRQ(ierr);
  ierr = KSPSetTolerances(ksp, PETSC_DEFAULT, PETSC_DEFAULT, PETSC_DEFAULT, its);CHKERRQ(ierr);
  ierr = KSPSetInitialGuessNonzero(ksp, PETSC_TRUE);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode mg_free_levels(PC_MG *mg) {
  PetscErrorCode ierr;
  for (PetscInt l = 0; l < mg->n; l++) {
    PC_MG_Level *v = &mg->lev[l];
    if (v->smoothu != v->smoothd) { ierr = KSPDestroy(&v->smoothu);CHKERRQ(ierr); }
    ierr = KSPDestroy(&v->smoothd);CHKERRQ(ierr);
    ierr = VecDestroy(&v->b);CHKERRQ(ierr);
    ierr = VecDestroy(&v->x);CHKERRQ(ierr);
    ierr = VecDestroy(&v->r);CHKERRQ(ierr);
    if (v->A) { ierr = MatDestroy(&v->A);CHKERRQ(ierr); }
    ierr = MatDestroy(&v->interpolate);CHKERRQ(ierr);   /* the PC's references; the caller's own destroy frees the matrices */
    ierr = MatDestroy(&v->restrct);CHKERRQ(ierr);
  }
  free(mg->lev); mg->lev = NULL; mg->n = 0;
  return 0;
}

PetscErrorCode PCMGSetLevels(PC pc, PetscInt levels, PetscComm *comms) {
  PC_MG *mg; PetscErrorCode ierr; char prefix[80];
  PCMGValid(pc, mg);
  (void)comms;   /* one communicator for all levels */
  if (pc->setupcalled) SETERRQ(pc->comm, PETSC_ERR_ORDER, "PCMGSetLevels() after the PC was set up");
  if (levels < 1 || levels > 999) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d levels", (int)levels);
  ierr = mg_level_prefix(pc, 1, PETSC_FALSE, prefix, sizeof(prefix));CHKERRQ(ierr);
  ierr = mg_free_levels(mg);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PC_MG_Level) * (size_t)levels, &mg->lev);CHKERRQ(ierr);
  memset(mg->lev, 0, sizeof(PC_MG_Level) * (size_t)levels);
  mg->n = levels;
  for (PetscInt l = 0; l < levels; l++) {
    KSP ksp;
    ierr = KSPCreate(pc->comm, &ksp);CHKERRQ(ierr);
    mg->lev[l].smoothd = mg->lev[l].smoothu = ksp;
    ierr = mg_level_prefix(pc, l, PETSC_FALSE, prefix, sizeof(prefix));CHKERRQ(ierr);
    ierr = KSPSetOptionsPrefix(ksp, prefix);CHKERRQ(ierr);
    if (l) { ierr = mg_smoother_defaults(ksp, 1);CHKERRQ(ierr); }
    else { ierr = KSPSetType(ksp, KSPPREONLY);CHKERRQ(ierr); }   /* the PC's type stays unset: PCSetUp picks the default */
  }
  return 0;
}
PetscErrorCode PCMGGetLevels(PC pc, PetscInt *levels) { PC_MG *mg; PCMGValid(pc, mg); *levels = mg->n; return 0; }
PetscErrorCode PCMGSetType(PC pc, PCMGType form) {
  PC_MG *mg; PCMGValid(pc, mg);
  if (form == PC_MG_KASKADE) SETERRQ(pc->comm, PETSC_ERR_SUP, "PC_MG_KASKADE is outside the ported path");
  if (form != PC_MG_MULTIPLICATIVE && form != PC_MG_ADDITIVE && form != PC_MG_FULL) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "Unknown multigrid type %d", (int)form);
  mg->am = form;
  return 0;
}
PetscErrorCode PCMGSetCycleType(PC pc, PCMGCycleType c) {
  PC_MG *mg; PCMGValid(pc, mg);
  if (c != PC_MG_CYCLE_V && c != PC_MG_CYCLE_W) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "Unknown cycle type %d", (int)c);
  mg->cycle = c;
  return 0;
}
PetscErrorCode PCMGMultiplicativeSetCycles(PC pc, PetscInt n) {
  PC_MG *mg; PCMGValid(pc, mg);
  if (n < 1) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d cycles per application", (int)n);
  mg->cycles = n;
  return 0;
}
PetscErrorCode PCMGSetGalerkin(PC pc, PetscBool use) { PC_MG *mg; PCMGValid(pc, mg); mg->galerkin = use; return 0; }

/* the second smoother of a level: the same type, PC type, prefix and step count as the first, which stays the down smoother */
static PetscErrorCode mg_split_smoother(PC pc, PC_MG *mg, PetscInt l) {
  PetscErrorCode ierr;
  PC_MG_Level *v = &mg->lev[l];
  KSP up; PC dpc, upc;
  if (v->smoothu != v->smoothd) return 0;
  ierr = KSPCreate(pc->comm, &up);CHKERRQ(ierr);
  ierr = KSPSetOptionsPrefix(up, v->smoothd->prefix);CHKERRQ(ierr);
  ierr = mg_smoother_defaults(up, v->smoothd->max_it);CHKERRQ(ierr);
  ierr = KSPSetType(up, v->smoothd->type_name);CHKERRQ(ierr);
  ierr = KSPGetPC(v->smoothd, &dpc);CHKERRQ(ierr);
  ierr = KSPGetPC(up, &upc);CHKERRQ(ierr);
  if (dpc->type_name[0]) { ierr = PCSetType(upc, dpc->type_name);CHKERRQ(ierr); }
  if (dpc->mat) { ierr = KSPSetOperators(up, dpc->mat, dpc->pmat, SAME_NONZERO_PATTERN);CHKERRQ(ierr); }
  v->smoothu = up;
  if (pc->setupcalled == 2) pc->setupcalled = 1;   /* the new solver is set up with the others */
  return 0;
}
PetscErrorCode PCMGGetSmoother(PC pc, PetscInt l, KSP *ksp) { PC_MG *mg; PCMGValid(pc, mg); PCMGLevel(pc, mg, l); *ksp = mg->lev[l].smoothd; return 0; }
PetscErrorCode PCMGGetSmootherDown(PC pc, PetscInt l, KSP *ksp) { return PCMGGetSmoother(pc, l, ksp); }
PetscErrorCode PCMGGetSmootherUp(PC pc, PetscInt l, KSP *ksp) {
  PC_MG *mg; PCMGValid(pc, mg); PCMGLevel(pc, mg, l);
  if (!l) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "There is no such thing as a up smoother on the coarse grid");
  PetscErrorCode ierr = mg_split_smoother(pc, mg, l);CHKERRQ(ierr);
  *ksp = mg->lev[l].smoothu;
  return 0;
}
PetscErrorCode PCMGGetCoarseSolve(PC pc, KSP *ksp) { return PCMGGetSmoother(pc, 0, ksp); }
PetscErrorCode PCMGSetNumberSmoothDown(PC pc, PetscInt n) {
  PC_MG *mg; PetscErrorCode ierr; PCMGValid(pc, mg); PCMGLevel(pc, mg, 0);
  if (n < 0) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d smoothing steps", (int)n);
  for (PetscInt l = 1; l < mg->n; l++) {
    if (mg->lev[l].smoothd->max_it == n) continue;
    ierr = mg_split_smoother(pc, mg, l);CHKERRQ(ierr);       /* unequal counts: the up smoother keeps its own */
    ierr = KSPSetTolerances(mg->lev[l].smoothd, PETSC_DEFAULT, PETSC_DEFAULT, PETSC_DEFAULT, n);CHKERRQ(ierr);
  }
  return 0;
}
PetscErrorCode PCMGSetNumberSmoothUp(PC pc, PetscInt n) {
  PC_MG *mg; PetscErrorCode ierr; PCMGValid(pc, mg); PCMGLevel(pc, mg, 0);
  if (n < 0) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d smoothing steps", (int)n);
  for (PetscInt l = 1; l < mg->n; l++) {
    if (mg->lev[l].smoothu->max_it == n) continue;
    ierr = mg_split_smoother(pc, mg, l);CHKERRQ(ierr);
    ierr = KSPSetTolerances(mg->lev[l].smoothu, PETSC_DEFAULT, PETSC_DEFAULT, PETSC_DEFAULT, n);CHKERRQ(ierr);
  }
  return 0;
}
PetscErrorCode PCMGSetInterpolation(PC pc, PetscInt l, Mat mat) {
  PC_MG *mg; PCMGValid(pc, mg); PCMGLevel(pc, mg, l);
  if (!l) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "Do not set interpolation routine for coarsest level");
  return mg_hold(&mg->lev[l].interpolate, mat);
}
PetscErrorCode PCMGSetRestriction(PC pc, PetscInt l, Mat mat) {
  PC_MG *mg; PCMGValid(pc, mg); PCMGLevel(pc, mg, l);
  if (!l) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "Do not set restriction routine for coarsest level");
  return mg_hold(&mg->lev[l].restrct, mat);
}
PetscErrorCode PCMGSetResidual(PC pc, PetscInt l, PCMGResidualFn residual, Mat mat) {
  PC_MG *mg; PCMGValid(pc, mg); PCMGLevel(pc, mg, l);
  mg->lev[l].residual = residual;
  mg->lev[l].resmat = mat;
  return 0;
}

/* a level solver's options are read once, at its first set-up (mg.c reads them only while !pc->setupcalled): what the caller sets on a
 * borrowed smoother between two set-ups stays */
static PetscErrorCode mg_solver_setup(PC pc, KSP ksp, PetscInt l, PetscBool *optread) {
  PetscErrorCode ierr; char prefix[80];
  if (*optread) return KSPSetUp(ksp);
  *optread = PETSC_TRUE;
  if (l) {   /* an option under mg_levels_ reaches every smoothed level; the same option under mg_levels_<l>_ is read after it and wins */
    ierr = mg_level_prefix(pc, l, PETSC_TRUE, prefix, sizeof(prefix));CHKERRQ(ierr);
    ierr = KSPSetOptionsPrefix(ksp, prefix);CHKERRQ(ierr);
    ierr = KSPSetFromOptions(ksp);CHKERRQ(ierr);
  }
  ierr = mg_level_prefix(pc, l, PETSC_FALSE, prefix, sizeof(prefix));CHKERRQ(ierr);
  ierr = KSPSetOptionsPrefix(ksp, prefix);CHKERRQ(ierr);
  ierr = KSPSetFromOptions(ksp);CHKERRQ(ierr);
  ierr = KSPSetUp(ksp);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode PCSetUp_MG(PC pc) {
  PetscErrorCode ierr;
  PC_MG *mg = (PC_MG *)pc->data;
  const PetscInt n = mg->n;
  if (!n) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "PCMGSetLevels() or -pc_mg_levels must come before the set-up");
  for (PetscInt l = 1; l < n; l++) {
    PC_MG_Level *v = &mg->lev[l];
    if (!v->interpolate && !v->restrct) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "level %d has neither interpolation nor restriction", (int)l);
  }
  ierr = KSPSetOperators(mg->lev[n - 1].smoothd, pc->mat, pc->pmat, SAME_NONZERO_PATTERN);CHKERRQ(ierr);
  for (PetscInt l = n - 1; l > 0; l--) {
    PC_MG_Level *c = &mg->lev[l - 1];
    if (mg->galerkin) {   /* A_{l-1} = P_l^T A_l P_l: symbolic and numeric the first time, numeric only from then on */
      Mat Af = l == n - 1 ? pc->pmat : mg->lev[l].A, P = mg_interp(&mg->lev[l]);
      if (P->rmap->N != Af->cmap->N) SETERRQ(pc->comm, PETSC_ERR_SUP, "Galerkin operators need the transfer of level %d stored as the interpolation (%d rows), got %d x %d", (int)l, Af->cmap->N, P->rmap->N, P->cmap->N);
      if (c->A && c->Aready) c->Aready = PETSC_FALSE;
      else { ierr = MatPtAP(Af, P, c->A ? MAT_REUSE_MATRIX : MAT_INITIAL_MATRIX, (PetscReal)PETSC_DEFAULT, &c->A);CHKERRQ(ierr); }
      ierr = KSPSetOperators(c->smoothd, c->A, c->A, SAME_NONZERO_PATTERN);CHKERRQ(ierr);
    } else {
      if (!c->smoothd->pc || !c->smoothd->pc->mat) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "level %d has no operators: KSPSetOperators() on its smoother, or PCMGSetGalerkin()", (int)(l - 1));
      ierr = KSPSetOperators(c->smoothd, c->smoothd->pc->mat, c->smoothd->pc->pmat, SAME_NONZERO_PATTERN);CHKERRQ(ierr);   /* values may have changed */
    }
  }
  for (PetscInt l = 0; l < n; l++) {
    PC_MG_Level *v = &mg->lev[l];
    Mat A = v->smoothd->pc->mat, T = l ? mg_interp(v) : NULL;
    if (v->b && (v->b->map->n != A->rmap->n || v->x->map->n != A->cmap->n)) {   /* the level's operator changed its size: new level vectors */
      ierr = VecDestroy(&v->b);CHKERRQ(ierr);
      ierr = VecDestroy(&v->x);CHKERRQ(ierr);
      ierr = VecDestroy(&v->r);CHKERRQ(ierr);
    }
    if (!v->b) {
      ierr = MatGetVecs(A, &v->x, &v->b);CHKERRQ(ierr);
      ierr = VecDuplicate(v->b, &v->r);CHKERRQ(ierr);
    }
    if (T && T->rmap->N != A->cmap->N && T->cmap->N != A->cmap->N) SETERRQ(pc->comm, PETSC_ERR_ARG_SIZ, "the interpolation of level %d is %d x %d, the level has %d unknowns", (int)l, T->rmap->N, T->cmap->N, A->cmap->N);
    ierr = mg_solver_setup(pc, v->smoothd, l, &v->optd);CHKERRQ(ierr);
    if (v->smoothu != v->smoothd) {
      ierr = KSPSetOperators(v->smoothu, A, v->smoothd->pc->pmat, SAME_NONZERO_PATTERN);CHKERRQ(ierr);
      ierr = mg_solver_setup(pc, v->smoothu, l, &v->optu);CHKERRQ(ierr);
    }
  }
  return 0;
}

static PetscErrorCode mg_residual(PC_MG *mg, PetscInt l) {
  PC_MG_Level *v = &mg->lev[l];
  Mat A = v->resmat ? v->resmat : v->smoothd->pc->mat;
  return (*(v->residual ? v->residual : PCMGDefaultResidual))(A, v->b, v->x, v->r);
}
static PetscErrorCode mg_cycle(PC_MG *mg, PetscInt l) {   /* PCMGMCycle_Private, mg.c:8-40 */
  PetscErrorCode ierr;
  PC_MG_Level *v = &mg->lev[l], *c;
  ierr = KSPSolve(v->smoothd, v->b, v->x);CHKERRQ(ierr);
  if (!l) return 0;
  c = &mg->lev[l - 1];
  ierr = mg_residual(mg, l);CHKERRQ(ierr);
  ierr = MatRestrict(mg_restr(v), v->r, c->b);CHKERRQ(ierr);
  ierr = VecSet(c->x, 0.0);CHKERRQ(ierr);
  for (PetscInt k = (l - 1 == 0 || mg->cycle == PC_MG_CYCLE_V) ? 1 : 2; k > 0; k--) { ierr = mg_cycle(mg, l - 1);CHKERRQ(ierr); }
  ierr = MatInterpolateAdd(mg_interp(v), c->x, v->x, v->x);CHKERRQ(ierr);
  ierr = KSPSolve(v->smoothu, v->b, v->x);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode PCApply_MG(PC pc, Vec b, Vec y) {
  PetscErrorCode ierr;
  PC_MG *mg = (PC_MG *)pc->data;
  const PetscInt n = mg->n;
  PC_MG_Level *top = &mg->lev[n - 1];
  ierr = VecCopy(b, top->b);CHKERRQ(ierr);
  if (mg->am == PC_MG_MULTIPLICATIVE) {
    ierr = VecSet(top->x, 0.0);CHKERRQ(ierr);
    for (PetscInt k = 0; k < mg->cycles; k++) { ierr = mg_cycle(mg, n - 1);CHKERRQ(ierr); }
  } else {
    for (PetscInt l = n - 1; l > 0; l--) { ierr = MatRestrict(mg_restr(&mg->lev[l]), mg->lev[l].b, mg->lev[l - 1].b);CHKERRQ(ierr); }
    if (mg->am == PC_MG_ADDITIVE) {   /* PCMGACycle_Private, smg.c */
      for (PetscInt l = 0; l < n; l++) {
        ierr = VecSet(mg->lev[l].x, 0.0);CHKERRQ(ierr);
        ierr = KSPSolve(mg->lev[l].smoothd, mg->lev[l].b, mg->lev[l].x);CHKERRQ(ierr);
      }
      for (PetscInt l = 1; l < n; l++) { ierr = MatInterpolateAdd(mg_interp(&mg->lev[l]), mg->lev[l - 1].x, mg->lev[l].x, mg->lev[l].x);CHKERRQ(ierr); }
    } else {                          /* PCMGFCycle_Private, fmg.c */
      ierr = VecSet(mg->lev[0].x, 0.0);CHKERRQ(ierr);
      ierr = KSPSolve(mg->lev[0].smoothd, mg->lev[0].b, mg->lev[0].x);CHKERRQ(ierr);
      for (PetscInt l = 1; l < n; l++) {
        ierr = MatInterpolate(mg_interp(&mg->lev[l]), mg->lev[l - 1].x, mg->lev[l].x);CHKERRQ(ierr);
        ierr = mg_cycle(mg, l);CHKERRQ(ierr);
      }
    }
  }
  ierr = VecCopy(top->x, y);CHKERRQ(ierr);
  return 0;
}

/* -pc_mg_type, -pc_mg_cycle_type, -pc_mg_multiplicative_cycles: what needs no levels */
PetscErrorCode PCMGCycleOptions_Private(PC pc) {
  PetscErrorCode ierr;
  PC_MG *mg = (PC_MG *)pc->data;
  PetscInt iv; PetscBool set; char t[32];
  ierr = PetscOptionsGetString(pc->prefix, "-pc_mg_type", t, sizeof(t), &set);CHKERRQ(ierr);
  if (set) {
    static const char *const names[] = {"multiplicative", "additive", "full", "kaskade"};
    int k = 0;
    while (k < 4 && strcmp(t, names[k])) k++;
    if (k == 4) SETERRQ(pc->comm, PETSC_ERR_ARG_UNKNOWN_TYPE, "Unknown multigrid type %s", t);
    ierr = PCMGSetType(pc, (PCMGType)k);CHKERRQ(ierr);
  }
  ierr = PetscOptionsGetString(pc->prefix, "-pc_mg_cycle_type", t, sizeof(t), &set);CHKERRQ(ierr);
  if (set) {
    if (!strcmp(t, "v")) mg->cycle = PC_MG_CYCLE_V;
    else if (!strcmp(t, "w")) mg->cycle = PC_MG_CYCLE_W;
    else SETERRQ(pc->comm, PETSC_ERR_ARG_UNKNOWN_TYPE, "-pc_mg_cycle_type <v|w>, got %s", t);
  }
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_mg_multiplicative_cycles", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCMGMultiplicativeSetCycles(pc, iv);CHKERRQ(ierr); }
  return 0;
}
static PetscErrorCode PCSetFromOptions_MG(PC pc) {
  PetscErrorCode ierr;
  PC_MG *mg = (PC_MG *)pc->data;
  PetscInt iv; PetscBool set; char t[32];
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_mg_levels", &iv, &set);CHKERRQ(ierr);
  if (set && iv != mg->n) { ierr = PCMGSetLevels(pc, iv, NULL);CHKERRQ(ierr); }
  ierr = PCMGCycleOptions_Private(pc);CHKERRQ(ierr);
  ierr = PetscOptionsGetString(pc->prefix, "-pc_mg_galerkin", t, sizeof(t), &set);CHKERRQ(ierr);
  if (set) mg->galerkin = (PetscBool)(strcmp(t, "0") && strcmp(t, "false"));
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_mg_smoothdown", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCMGSetNumberSmoothDown(pc, iv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_mg_smoothup", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCMGSetNumberSmoothUp(pc, iv);CHKERRQ(ierr); }
  return 0;
}
static PetscErrorCode PCDestroy_MG(PC pc) {
  PC_MG *mg = (PC_MG *)pc->data;
  if (!mg) return 0;
  PetscErrorCode ierr = mg_free_levels(mg);CHKERRQ(ierr);
  free(mg); pc->data = NULL;
  return 0;
}
/* ---- for the types built on this one (gamg.c) ---- */
void **PCMGLayerData_Private(PC pc) { return &((PC_MG *)pc->data)->layer; }
PetscErrorCode PCMGReset_Private(PC pc) {   /* back to "no levels, never set up": the level solvers, vectors, operators and transfers go */
  PetscErrorCode ierr = mg_free_levels((PC_MG *)pc->data);CHKERRQ(ierr);
  pc->setupcalled = 0;
  return 0;
}
PetscErrorCode PCMGAdoptGalerkin_Private(PC pc, PetscInt l, Mat A) {   /* A = MatPtAP(A_{l+1}, P_{l+1}, MAT_INITIAL_MATRIX): the PC's own from here on */
  PC_MG *mg = (PC_MG *)pc->data;
  PCMGLevel(pc, mg, l);
  if (mg->lev[l].A) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "level %d has a Galerkin operator", (int)l);
  mg->lev[l].A = A; mg->lev[l].Aready = PETSC_TRUE;
  return 0;
}
PetscErrorCode PCSetUp_MG_Private(PC pc) { return PCSetUp_MG(pc); }
PetscErrorCode PCDestroy_MG_Private(PC pc) { return PCDestroy_MG(pc); }
PetscErrorCode PCCreate_MG(PC pc) {
  PC_MG *mg;
  PetscErrorCode ierr = PetscMalloc(sizeof(*mg), &mg);CHKERRQ(ierr);
  memset(mg, 0, sizeof(*mg));
  mg->am = PC_MG_MULTIPLICATIVE; mg->cycle = PC_MG_CYCLE_V; mg->cycles = 1;
  pc->data = mg;
  pc->ops->setup = PCSetUp_MG; pc->ops->apply = PCApply_MG; pc->ops->setfromoptions = PCSetFromOptions_MG; pc->ops->destroy = PCDestroy_MG;
  return 0;
}
