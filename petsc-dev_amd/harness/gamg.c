/* PCGAMG (src/ksp/pc/impls/gamg/gamg.c, agg.c): smoothed aggregation for sequential AIJ operators with the constant as near-null
 * space.  A thin layer that fills a PC_MG (mg.c) and then is one: apply, cycle types, the PCMG calls and the level solvers' prefixes
 * mg_coarse_ / mg_levels_<l>_ are mg.c's own.  Control flow only: every step of the set-up is a public call of this library, so an
 * application equals, bit for bit, that of a PCMG given the same prolongators by hand.  The set-up ("PCGAMG"), on level
 * operator A_l, A_0 = the PC's pmat (levels counted from the fine one here; PCMG counts from the coarse one):
 *
 *   d = MatGetDiagonal(A_l)                       a zero entry: PETSC_ERR_ARG_WRONGSTATE naming the row
 *   agg, nagg = MatCoarsenAggregate(A_l, threshold)
 *   stop when  n_l <= coarse_eq_limit,  l + 1 == the level cap,  nagg == n_l or nagg == 0:  A_l is the coarsest
 *   T  n_l x nagg, T(i, agg[i]) = 1 / sqrt(|aggregate agg[i]|)
 *   S = D^-1 A_l (MatDuplicate, MatDiagonalScale), rho_l = MatNorm(S, NORM_INFINITY)
 *   nsmooths == 1:  P = T - (4 / (3 rho_l)) S T   (MatMatMult, MatScale, MatAXPY with SUBSET_NONZERO_PATTERN: A_l stores its diagonal,
 *                   so T's pattern lies inside S T's);   nsmooths == 0:  P = T
 *   A_{l+1} = MatPtAP(A_l, P), handed to the PCMG as the Galerkin operator of that level (later set-ups refill it there)
 *
 * Smoothers default to chebychev + jacobi, two steps, no norm, eigenvalue bounds (rho_l / 10, rho_l); options under mg_levels_ are
 * read after that and win.  The coarsest level: preonly + ILU with as many levels of fill as it has rows -- a complete LU. */
#include "petscimpl.h"

typedef struct {
  PetscReal threshold;
  PetscInt coarse_eq_limit, nlevels, nsmooths;
  PetscBool reuse;
  PetscBool built;
  PetscInt n, sizes[1000];       /* the hierarchy of the last set-up, fine level first */
} PC_GAMG;

#define PCGAMGValid(pc, g) do { \
  if (!(pc)) SETERRQ(0, PETSC_ERR_ARG_NULL, "Null PC"); \
  if (strcmp((pc)->type_name, PCGAMG)) SETERRQ((pc)->comm, PETSC_ERR_ARG_WRONG, "PC of type %s is not a PCGAMG", (pc)->type_name); \
  (g) = (PC_GAMG *)*PCMGLayerData_Private(pc); } while (0)

PetscErrorCode PCGAMGSetThreshold(PC pc, PetscReal threshold) {
  PC_GAMG *g; PCGAMGValid(pc, g);
  if (!(threshold >= 0.0)) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "threshold %g must be >= 0", (double)threshold);
  g->threshold = threshold;
  return 0;
}
PetscErrorCode PCGAMGSetCoarseEqLimit(PC pc, PetscInt n) {
  PC_GAMG *g; PCGAMGValid(pc, g);
  if (n < 1) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "coarse limit %d must be >= 1", (int)n);
  g->coarse_eq_limit = n;
  return 0;
}
PetscErrorCode PCGAMGSetNlevels(PC pc, PetscInt n) {
  PC_GAMG *g; PCGAMGValid(pc, g);
  if (n < 1 || n > 999) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d levels", (int)n);
  g->nlevels = n;
  return 0;
}
PetscErrorCode PCGAMGSetNSmooths(PC pc, PetscInt n) {
  PC_GAMG *g; PCGAMGValid(pc, g);
  if (n != 0 && n != 1) SETERRQ(pc->comm, PETSC_ERR_ARG_OUTOFRANGE, "%d smoothing steps of the prolongator: 0 or 1", (int)n);
  g->nsmooths = n;
  return 0;
}
PetscErrorCode PCGAMGSetReuseInterpolation(PC pc, PetscBool reuse) { PC_GAMG *g; PCGAMGValid(pc, g); g->reuse = reuse; return 0; }
PetscErrorCode PCGAMGGetLevelSizes(PC pc, PetscInt maxn, PetscInt *nlevels, PetscInt sizes[]) {
  PC_GAMG *g; PCGAMGValid(pc, g);
  if (nlevels) *nlevels = g->n;
  for (PetscInt l = 0; sizes && l < g->n && l < maxn; l++) sizes[l] = g->sizes[l];
  return 0;
}

/* T of a level: n x nagg, one entry 1 / sqrt(|aggregate|) per row, a matrix of A's type */
static PetscErrorCode gamg_tentative(Mat A, PetscInt n, PetscInt nagg, const PetscInt agg[], Mat *T) {
  PetscErrorCode ierr;
  PetscInt *ti, *cnt; PetscScalar *ta;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(n + 1), &ti);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)nagg, &cnt);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)n, &ta);CHKERRQ(ierr);
  memset(cnt, 0, sizeof(PetscInt) * (size_t)nagg);
  for (PetscInt i = 0; i < n; i++) cnt[agg[i]]++;
  for (PetscInt i = 0; i < n; i++) { ti[i] = i; ta[i] = 1.0 / sqrt((PetscReal)cnt[agg[i]]); }
  ti[n] = n;
  ierr = MatCreate(A->comm, T);CHKERRQ(ierr);
  ierr = MatSetSizes(*T, n, nagg, n, nagg);CHKERRQ(ierr);
  ierr = MatSetType(*T, A->type_name);CHKERRQ(ierr);
  ierr = MatSeqAIJSetPreallocationCSR(*T, ti, agg, ta);CHKERRQ(ierr);
  free(ti); free(cnt); free(ta);
  return 0;
}
/* rho = |D^-1 A|_inf and, with nsmooths, P = T - (4 / (3 rho)) D^-1 A T (T is consumed: P is T itself without smoothing) */
static PetscErrorCode gamg_prolongator(PC pc, Mat A, Vec dinv, PetscInt nsmooths, Mat T, PetscReal *rho, Mat *P) {
  PetscErrorCode ierr;
  Mat S;
  ierr = MatDuplicate(A, MAT_COPY_VALUES, &S);CHKERRQ(ierr);
  ierr = MatDiagonalScale(S, dinv, NULL);CHKERRQ(ierr);
  ierr = MatNorm(S, NORM_INFINITY, rho);CHKERRQ(ierr);
  if (!(*rho > 0.0) || *rho - *rho != 0.0) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "the row sums of D^-1 A give the bound %g", (double)*rho);
  if (nsmooths) {
    ierr = MatMatMult(S, T, MAT_INITIAL_MATRIX, (PetscReal)PETSC_DEFAULT, P);CHKERRQ(ierr);
    ierr = MatScale(*P, -(4.0 / (3.0 * *rho)));CHKERRQ(ierr);
    ierr = MatAXPY(*P, 1.0, T, SUBSET_NONZERO_PATTERN);CHKERRQ(ierr);
    ierr = MatDestroy(&T);CHKERRQ(ierr);
  } else *P = T;
  return MatDestroy(&S);
}

static PetscErrorCode gamg_build(PC pc, PC_GAMG *g) {
  PetscErrorCode ierr;
  Mat A = pc->pmat, *Ps = NULL, *As = NULL;
  PetscReal *rho = NULL;
  PetscInt L = 0;                                   /* levels below the fine one so far */
  ierr = PetscMalloc(sizeof(Mat) * (size_t)g->nlevels, &Ps);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(Mat) * (size_t)g->nlevels, &As);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscReal) * (size_t)g->nlevels, &rho);CHKERRQ(ierr);
  for (;;) {
    const PetscInt n = A->rmap->N;
    PetscInt nagg = 0, *agg = NULL;
    Vec d = NULL; const PetscScalar *dv; Mat T = NULL;
    PetscBool last;
    if (A->rmap->N != A->cmap->N) SETERRQ(pc->comm, PETSC_ERR_ARG_SIZ, "Matrix must be square, %d != %d", A->rmap->N, A->cmap->N);
    g->sizes[L] = n;
    ierr = MatGetVecs(A, NULL, &d);CHKERRQ(ierr);
    ierr = MatGetDiagonal(A, d);CHKERRQ(ierr);
    ierr = VecGetArrayRead(d, &dv);CHKERRQ(ierr);
    for (PetscInt i = 0; i < n; i++) if (dv[i] == 0.0) SETERRQ(pc->comm, PETSC_ERR_ARG_WRONGSTATE, "Zero diagonal entry in row %d of the operator of level %d (0 is the fine level)", (int)i, (int)L);
    ierr = VecRestoreArrayRead(d, &dv);CHKERRQ(ierr);
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &agg);CHKERRQ(ierr);
    ierr = MatCoarsenAggregate(A, g->threshold, &nagg, agg);CHKERRQ(ierr);
    last = (PetscBool)(n <= g->coarse_eq_limit || L + 1 >= g->nlevels || nagg == n || nagg == 0);
    if (!last) {
      ierr = gamg_tentative(A, n, nagg, agg, &T);CHKERRQ(ierr);
      ierr = VecReciprocal(d);CHKERRQ(ierr);
      ierr = gamg_prolongator(pc, A, d, g->nsmooths, T, &rho[L], &Ps[L]);CHKERRQ(ierr);
      ierr = MatPtAP(A, Ps[L], MAT_INITIAL_MATRIX, (PetscReal)PETSC_DEFAULT, &As[L]);CHKERRQ(ierr);
    }
    free(agg);
    ierr = VecDestroy(&d);CHKERRQ(ierr);
    if (last) break;
    A = As[L++];
  }
  /* the PCMG: level L - k of it is level k here */
  g->n = L + 1;
  ierr = PCMGSetLevels(pc, g->n, NULL);CHKERRQ(ierr);
  ierr = PCMGSetGalerkin(pc, PETSC_TRUE);CHKERRQ(ierr);
  for (PetscInt k = 0; k < L; k++) {
    KSP smooth; PC sub;
    ierr = PCMGSetInterpolation(pc, L - k, Ps[k]);CHKERRQ(ierr);
    ierr = MatDestroy(&Ps[k]);CHKERRQ(ierr);        /* (the PCMG holds its own reference) */
    ierr = PCMGAdoptGalerkin_Private(pc, L - k - 1, As[k]);CHKERRQ(ierr);
    ierr = PCMGGetSmoother(pc, L - k, &smooth);CHKERRQ(ierr);
    ierr = KSPSetType(smooth, KSPCHEBYCHEV);CHKERRQ(ierr);
    ierr = KSPGetPC(smooth, &sub);CHKERRQ(ierr);
    ierr = PCSetType(sub, PCJACOBI);CHKERRQ(ierr);
    ierr = KSPSetNormType(smooth, KSP_NORM_NONE);CHKERRQ(ierr);
    ierr = KSPSetTolerances(smooth, PETSC_DEFAULT, PETSC_DEFAULT, PETSC_DEFAULT, 2);CHKERRQ(ierr);
    ierr = KSPChebychevSetEigenvalues(smooth, rho[k], rho[k] / 10.0);CHKERRQ(ierr);
  }
  {
    KSP coarse; PC sub;
    ierr = PCMGGetCoarseSolve(pc, &coarse);CHKERRQ(ierr);
    ierr = KSPGetPC(coarse, &sub);CHKERRQ(ierr);
    ierr = PCSetType(sub, PCILU);CHKERRQ(ierr);
    ierr = PCFactorSetLevels(sub, g->sizes[L]);CHKERRQ(ierr);
  }
  free(Ps); free(As); free(rho);
  g->built = PETSC_TRUE;
  return 0;
}

static PetscErrorCode PCSetUp_GAMG(PC pc) {
  PetscErrorCode ierr;
  PC_GAMG *g = (PC_GAMG *)*PCMGLayerData_Private(pc);
  if (!g->built || !g->reuse) {
    const int was = pc->setupcalled;
    if (g->built) { ierr = PCMGReset_Private(pc);CHKERRQ(ierr); g->built = PETSC_FALSE; g->n = 0; }
    ierr = gamg_build(pc, g);CHKERRQ(ierr);
    pc->setupcalled = was;
  }
  return PCSetUp_MG_Private(pc);   /* with the hierarchy kept: the Galerkin refill and the level solvers' set-up */
}
static PetscErrorCode PCSetFromOptions_GAMG(PC pc) {
  PetscErrorCode ierr;
  PetscReal rv; PetscInt iv; PetscBool set; char t[32];
  ierr = PetscOptionsGetReal(pc->prefix, "-pc_gamg_threshold", &rv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCGAMGSetThreshold(pc, rv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_gamg_coarse_eq_limit", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCGAMGSetCoarseEqLimit(pc, iv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_mg_levels", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCGAMGSetNlevels(pc, iv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetInt(pc->prefix, "-pc_gamg_agg_nsmooths", &iv, &set);CHKERRQ(ierr);
  if (set) { ierr = PCGAMGSetNSmooths(pc, iv);CHKERRQ(ierr); }
  ierr = PetscOptionsGetString(pc->prefix, "-pc_gamg_reuse_interpolation", t, sizeof(t), &set);CHKERRQ(ierr);
  if (set) { ierr = PCGAMGSetReuseInterpolation(pc, (PetscBool)(strcmp(t, "0") && strcmp(t, "false")));CHKERRQ(ierr); }
  return PCMGCycleOptions_Private(pc);
}
static PetscErrorCode PCDestroy_GAMG(PC pc) {
  if (pc->data) { void **slot = PCMGLayerData_Private(pc); free(*slot); *slot = NULL; }
  return PCDestroy_MG_Private(pc);
}
PetscErrorCode PCCreate_GAMG(PC pc) {
  PC_GAMG *g;
  PetscErrorCode ierr = PCCreate_MG(pc);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(*g), &g);CHKERRQ(ierr);
  memset(g, 0, sizeof(*g));
  g->threshold = 0.0; g->coarse_eq_limit = 50; g->nlevels = 25; g->nsmooths = 1; g->reuse = PETSC_FALSE;
  *PCMGLayerData_Private(pc) = g;
  pc->ops->setup = PCSetUp_GAMG; pc->ops->setfromoptions = PCSetFromOptions_GAMG; pc->ops->destroy = PCDestroy_GAMG;
  return 0;
}
