/* Factored matrices of MATSEQBAIJHIPMI355X: block ILU(k) behind the reference's factorisation interface, the BAIJ companion of
 * host/ilu.c --
 *
 *   MatGetFactor(A, "petsc", MAT_FACTOR_ILU, &F)         "MatGetFactor_petsc_C" composed on every matrix of the block type (bs > 1)
 *   MatILUFactorSymbolic(F, A, NULL, NULL, info)         natural ordering, info->levels levels of fill over BLOCKS
 *   MatLUFactorNumeric(F, A, info)                       MatLUFactorNumeric_SeqBAIJ_<bs>_NaturalOrdering on the host copy
 *   MatSolve(F, b, x)                                    MatSolve_SeqBAIJ_<bs>_NaturalOrdering (baijfact2.c) on the device
 *
 * so that an unchanged PCILU (-pc_type ilu, -pc_factor_levels k, PCFactorSetLevels) preconditions a BAIJ operator.
 *
 *   symbolic : mi355x_iluk_symbolic_host on the block pattern (a block pattern is a CSR pattern), the dependency levels of L and of U
 *              over block rows, the rows sorted by level; layout and row lists uploaded once per pattern;
 *   numeric  : mi355x_bilu_numeric_host (csrc/bilu.hip, one host thread) into the host copy of the values, one upload.  A factorisation
 *              whose operator has the pattern of the last one (Mat_SeqAIJHIP.pattern_gen, sizes, levels of fill) repeats these two only;
 *   solve    : mi355x_bilu_lower_level for L's levels in ascending order, then mi355x_bilu_upper_level for U's: one launch per level on
 *              the compute stream, no host wait.  A kernel boundary per level is the only synchronisation, so this route cannot hang.
 *              -pc_factor_hipmi355x_trisolve fused (opt-in; level is the default): every maximal run of consecutive levels of at most
 *              -pc_factor_hipmi355x_bilu_chain_rows <n> (default 128) block rows each is ONE launch of one workgroup (mi355x_bilu_lower_chain /
 *              _upper_chain: a barrier between levels, no hand-off between workgroups, so no hang either), wider levels keep their
 *              own launch; the plan (mi355x_bilu_chain_plan_host) is cut once per pattern and chain_rows.  Same bits as level.
 *
 * PETSC_ERR_SUP, before anything is changed: ICC and LU of a block matrix, a -pc_factor_shift_type other than none (PCILU's unset default
 * is taken as none here: the reference's BAIJ factorisation has no shift loop either), -pc_factor_hipmi355x_numeric device,
 * -pc_factor_hipmi355x_trisolve other than level or fused, 1 = bs or bs > 7, a non-square matrix, an ordering other than the natural one.
 * Inside a PETSc tree (PETSCHIPMI355X_WITH_PETSC) the block type composes no factor: PETSc's own MATSEQBAIJ factorisation is what
 * MatGetFactor finds there. */
#include "hipmi355ximpl.h"

#if !defined(PETSCHIPMI355X_WITH_PETSC)
/* ---------------------------------------------------------------- releasing a factor: one function per form */
static void bilu_free_values(HipBlockFactors *f) {
  HipFree(f->ba); f->ba = NULL;
  if (f->d_ba) mi355x_free(f->d_ba);
  f->d_ba = NULL;
  f->factored_state = -1;
}
static void bilu_free_pattern(HipBlockFactors *f) {
  void *dev[] = {f->pat.d_bi, f->pat.d_bj, f->pat.d_bdiag, f->pat.d_rowsL, f->pat.d_rowsU, f->pat.d_levptrL, f->pat.d_levptrU};
  for (size_t i = 0; i < sizeof(dev) / sizeof(dev[0]); i++) if (dev[i]) mi355x_free(dev[i]);
  HipFree(f->pat.bi); HipFree(f->pat.bj); HipFree(f->pat.bdiag); HipFree(f->pat.levptrL); HipFree(f->pat.levptrU);
  HipFree(f->pat.segL); HipFree(f->pat.segU);
  memset(&f->pat, 0, sizeof(f->pat));
}
PetscErrorCode HipBlockFactorsDestroy(HipBlockFactors **pf) {
  HipBlockFactors *f = *pf;
  if (!f) return 0;
  bilu_free_values(f); bilu_free_pattern(f);
  HipFree(f);
  *pf = NULL;
  return 0;
}

/* what this route does not offer, asked for under the factor's prefix: refused before anything is changed.  What it does offer, if the
 * caller wants it: *fused = -pc_factor_hipmi355x_trisolve fused, *chain_rows = -pc_factor_hipmi355x_bilu_chain_rows (-1: not given) */
static PetscErrorCode bilu_refuse_options(Mat F, int *fused, PetscInt *chain_rows) {
  PetscErrorCode ierr;
  char v[64]; PetscBool set;
  PetscInt n = -1;
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_shift_type", v, sizeof(v), &set);CHKERRQ(ierr);
  if (set && strcmp(v, "none") && strcmp(v, "NONE")) SETERRQ(HipObjComm(F), PETSC_ERR_SUP, "-pc_factor_shift_type %s: block ILU of a BAIJ matrix has no shifts (none only)", v);
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_numeric", v, sizeof(v), &set);CHKERRQ(ierr);
  if (set && strcmp(v, "host")) SETERRQ(HipObjComm(F), PETSC_ERR_SUP, "-pc_factor_hipmi355x_numeric %s: block ILU of a BAIJ matrix is factored on the host", v);
  ierr = PetscOptionsGetString(HipObjPrefix(F), "-pc_factor_hipmi355x_trisolve", v, sizeof(v), &set);CHKERRQ(ierr);
  if (set && strcmp(v, "level") && strcmp(v, "fused")) SETERRQ(HipObjComm(F), PETSC_ERR_SUP, "-pc_factor_hipmi355x_trisolve %s: block ILU of a BAIJ matrix solves level by level, one launch per level (level) or per run of narrow levels (fused)", v);
  if (fused) *fused = set && !strcmp(v, "fused");
  ierr = PetscOptionsGetInt(HipObjPrefix(F), "-pc_factor_hipmi355x_bilu_chain_rows", &n, &set);CHKERRQ(ierr);
  if (set && n < 0) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_OUTOFRANGE, "-pc_factor_hipmi355x_bilu_chain_rows %d: a number of block rows >= 0 (0: no level is chained)", n);
  if (chain_rows) *chain_rows = set ? n : -1;
  return 0;
}

/* the launches of one application under trisolve fused, from the host level lists: once per pattern and per max_rows */
static PetscErrorCode bilu_plan(HipBlockFactors *f, PetscInt max_rows) {
  PetscErrorCode ierr;
  struct { PetscInt nlev; const PetscInt *levptr; PetscInt **seg, *nseg; } tri[2] = {{f->pat.nlevL, f->pat.levptrL, &f->pat.segL, &f->pat.nsegL},
                                                                                    {f->pat.nlevU, f->pat.levptrU, &f->pat.segU, &f->pat.nsegU}};
  for (int t = 0; t < 2; t++) {
    int nseg = 0;
    HipFree(*tri[t].seg); *tri[t].seg = NULL; *tri[t].nseg = 0;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(2 * tri[t].nlev + 2), tri[t].seg);CHKERRQ(ierr);
    CHKHIP(mi355x_bilu_chain_plan_host((int)tri[t].nlev, tri[t].levptr, (int)max_rows, *tri[t].seg, *tri[t].seg + tri[t].nlev + 1, &nseg));
    *tri[t].nseg = nseg;
  }
  f->pat.plan_rows = max_rows;
  return 0;
}

/* the block rows sorted by dependency level (stable: ascending row inside a level) */
static PetscErrorCode bilu_level_order(PetscInt n, const PetscInt *lev, PetscInt nlev, PetscInt **ptr_out, PetscInt *rows) {
  PetscInt *ptr, *next;
  PetscErrorCode ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(2 * nlev + 2), &ptr);CHKERRQ(ierr);
  next = ptr + nlev + 1;
  memset(ptr, 0, sizeof(PetscInt) * (size_t)(nlev + 1));
  for (PetscInt i = 0; i < n; i++) ptr[lev[i] + 1]++;
  for (PetscInt l = 0; l < nlev; l++) ptr[l + 1] += ptr[l];
  memcpy(next, ptr, sizeof(PetscInt) * (size_t)(nlev + 1));
  for (PetscInt i = 0; i < n; i++) rows[next[lev[i]]++] = i;
  *ptr_out = ptr;
  return 0;
}

/* the pattern side, once per pattern: the level-of-fill layout over blocks, the levels of L and U, everything but the values uploaded */
static PetscErrorCode bilu_pattern(Mat A, HipBlockFactors *f, PetscDeviceCtx *dc, PetscInt mbs, PetscInt bs, const PetscInt *ai, const PetscInt *aj, PetscInt levels, PetscInt max_rows) {
  PetscErrorCode ierr = 0;
  PetscInt *lev = NULL, *rows = NULL;
  int bad = -1, rc;
  bilu_free_values(f); bilu_free_pattern(f);
  f->mbs = mbs; f->bs = bs; f->levels = levels; f->nzbA = ai[mbs];
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(mbs + 1), &f->pat.bi);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(mbs + 1), &f->pat.bdiag);CHKERRQ(ierr);
  rc = mi355x_iluk_symbolic_host(mbs, ai, aj, levels, f->pat.bi, f->pat.bdiag, NULL, NULL, &bad);
  if (!rc) {
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(f->pat.bdiag[0] + 2), &f->pat.bj);CHKERRQ(ierr);
    f->pat.bj[f->pat.bdiag[0] + 1] = 0;
    rc = mi355x_iluk_symbolic_host(mbs, ai, aj, levels, f->pat.bi, f->pat.bdiag, f->pat.bj, NULL, &bad);
  }
  if (rc == 1 && bad >= 0 && bad < mbs) {                        /* hipErrorInvalidValue: the block row at fault */
    PetscBool diag = PETSC_FALSE;
    for (PetscInt q = ai[bad]; q < ai[bad + 1]; q++) if (aj[q] == bad) diag = PETSC_TRUE;
    if (!diag) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal block %d", bad);
    SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "block ILU(%d): the block columns of block row %d are not sorted inside the matrix", levels, bad);
  }
  CHKHIP(rc);
  f->nzb = f->pat.bdiag[0] + 1;
  /* a block row of L may start once the block rows its L part names are done; U backwards */
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(2 * PetscMax(mbs, 1)), &lev);CHKERRQ(ierr);
  rows = lev + PetscMax(mbs, 1);
  { const PetscInt *bi = f->pat.bi, *bj = f->pat.bj, *bdiag = f->pat.bdiag;
    const size_t ni = sizeof(PetscInt) * (size_t)(mbs + 1), nj = sizeof(PetscInt) * (size_t)(f->nzb + 1), nr = sizeof(PetscInt) * (size_t)PetscMax(mbs, 1);
    PetscInt nlev = 0;
    for (PetscInt i = 0; i < mbs; i++) {
      PetscInt l = 0;
      for (PetscInt q = bi[i]; q < bi[i + 1]; q++) l = PetscMax(l, lev[bj[q]] + 1);
      lev[i] = l; nlev = PetscMax(nlev, l + 1);
    }
    f->pat.nlevL = nlev;
    ierr = bilu_level_order(mbs, lev, nlev, &f->pat.levptrL, rows);
    if (!ierr) { rc = mi355x_malloc((void **)&f->pat.d_rowsL, nr); if (!rc) rc = mi355x_memcpy_h2d(dc->h, f->pat.d_rowsL, rows, nr); if (!rc) rc = mi355x_handle_synchronize(dc->h); }
    nlev = 0;
    for (PetscInt i = mbs - 1; i >= 0 && !ierr && !rc; i--) {
      PetscInt l = 0;
      for (PetscInt q = bdiag[i + 1] + 1; q < bdiag[i]; q++) l = PetscMax(l, lev[bj[q]] + 1);
      lev[i] = l; nlev = PetscMax(nlev, l + 1);
    }
    f->pat.nlevU = nlev;
    if (!ierr && !rc) ierr = bilu_level_order(mbs, lev, nlev, &f->pat.levptrU, rows);
    if (!ierr && !rc) { rc = mi355x_malloc((void **)&f->pat.d_rowsU, nr); if (!rc) rc = mi355x_memcpy_h2d(dc->h, f->pat.d_rowsU, rows, nr); }
    struct { void *p; const void *from; size_t bytes; } up[] = {{&f->pat.d_bi, bi, ni}, {&f->pat.d_bj, bj, nj}, {&f->pat.d_bdiag, bdiag, ni},
                                                                {&f->pat.d_levptrL, f->pat.levptrL, sizeof(PetscInt) * (size_t)(f->pat.nlevL + 1)},
                                                                {&f->pat.d_levptrU, f->pat.levptrU, sizeof(PetscInt) * (size_t)(f->pat.nlevU + 1)}};
    for (size_t i = 0; i < sizeof(up) / sizeof(up[0]) && !ierr && !rc; i++) {
      rc = mi355x_malloc((void **)up[i].p, up[i].bytes);
      if (!rc) rc = mi355x_memcpy_h2d(dc->h, *(void **)up[i].p, up[i].from, up[i].bytes);
    }
    if (!ierr && !rc) rc = mi355x_handle_synchronize(dc->h);   /* the rows' host copy goes away below */
  }
  HipFree(lev);
  CHKERRQ(ierr);
  CHKHIP(rc);
  ierr = bilu_plan(f, max_rows);CHKERRQ(ierr);
  f->pat.gen = ((Mat_SeqAIJHIP *)A->spptr)->pattern_gen; f->pat.stale = 0;
  f->symbolic_builds++;
  return 0;
}

static PetscErrorCode MatSolve_SeqBAIJHIP_ILU(Mat F, Vec b, Vec x);
/* the transposed block solves are not ported: said here, not left to an empty slot, so that the message names what is missing */
static PetscErrorCode MatSolveTranspose_SeqBAIJHIP_ILU(Mat F, Vec b, Vec x) {
  (void)b; (void)x;
  SETERRQ(HipObjComm(F), PETSC_ERR_SUP, "MatSolveTranspose on a block ILU factor (SeqBAIJ) is outside the ported path");
}
static PetscErrorCode MatLUFactorNumeric_SeqBAIJHIP(Mat F, Mat A, const MatFactorInfo *info) {
  PetscErrorCode ierr;
  HipBlockFactors *f = HipBlockGet(F);
  Mat_SeqAIJHIP *d = (Mat_SeqAIJHIP *)A->spptr;
  PetscDeviceCtx *dc;
  PetscInt mbs; const PetscInt *ai, *aj; const PetscScalar *aa;
  int zrow = -1, rc, fused = 0;
  PetscInt chain_rows = -1;
  if (strcmp(HipObjTypeName(A), MATSEQBAIJHIPMI355X)) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU on the device needs a sequential BAIJ matrix of this type; got %s", HipObjTypeName(A));
  if (A->rmap->n != A->cmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU of a BAIJ matrix: square matrices only, rows %d columns %d", A->rmap->n, A->cmap->n);
  ierr = bilu_refuse_options(F, &fused, &chain_rows);CHKERRQ(ierr);
  if (f->factored_state == HipObjState(A) && f->factored_of == (void *)A && f->d_ba && !f->pat.stale) {   /* same operator, same values: nothing to redo ... */
    f->fused = fused;                                                                                      /* ... but the route of this set-up */
    if (chain_rows < 0) chain_rows = HIP_BILU_CHAIN_ROWS;
    if (chain_rows != f->pat.plan_rows) { ierr = bilu_plan(f, chain_rows);CHKERRQ(ierr); }
    return 0;
  }
  ierr = MatSeqAIJGetArrays(A, &mbs, &ai, &aj, &aa);CHKERRQ(ierr);
  const PetscInt bs = mbs ? A->rmap->n / mbs : HipAIJGet(A)->bs;
  if (bs < 2 || bs > 7) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU of a BAIJ matrix: block sizes 2 .. 7, got %d", bs);
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);                              /* (the operator's pattern has its serial number from here) */
  const int same = f->pat.bi && !f->pat.stale && d->pattern_gen && f->pat.gen == d->pattern_gen && f->mbs == mbs && f->bs == bs && f->nzbA == ai[mbs] &&
                   f->levels == (PetscInt)info->levels;
  f->factored_state = -1;
  if (chain_rows < 0) chain_rows = HIP_BILU_CHAIN_ROWS;
  if (!same) { ierr = bilu_pattern(A, f, dc, mbs, bs, ai, aj, (PetscInt)info->levels, chain_rows);CHKERRQ(ierr); }
  else if (chain_rows != f->pat.plan_rows) { ierr = bilu_plan(f, chain_rows);CHKERRQ(ierr); }
  f->fused = fused;
  const size_t na = sizeof(PetscScalar) * (size_t)(f->nzb + 1) * (size_t)(bs * bs);
  if (!f->ba) { ierr = PetscMalloc(na, &f->ba);CHKERRQ(ierr); memset(f->ba, 0, na); }
  rc = mi355x_bilu_numeric_host(mbs, bs, ai, aj, aa, f->pat.bi, f->pat.bj, f->pat.bdiag, f->ba, &zrow);
  if (rc && zrow >= 0) SETERRQ(HipObjComm(A), 71 /* PETSC_ERR_MAT_LU_ZRPVT */, "Zero pivot, row %d", zrow);
  CHKHIP(rc);
  if (!f->d_ba) CHKHIP(mi355x_malloc((void **)&f->d_ba, na));
  CHKHIP(mi355x_memcpy_h2d(dc->h, f->d_ba, f->ba, na));
  CHKHIP(mi355x_handle_synchronize(dc->h));
  f->numeric_runs++;
  F->ops->solve = MatSolve_SeqBAIJHIP_ILU;
  F->ops->solvetranspose = MatSolveTranspose_SeqBAIJHIP_ILU;
  f->factored_state = HipObjState(A); f->factored_of = (void *)A;
  return 0;
}

static PetscErrorCode MatILUFactorSymbolic_SeqBAIJHIP(Mat F, Mat A, IS row, IS col, const MatFactorInfo *info) {
  PetscErrorCode ierr;
  if (strcmp(HipObjTypeName(A), MATSEQBAIJHIPMI355X)) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU on the device needs a sequential BAIJ matrix of this type; got %s", HipObjTypeName(A));
  if (A->rmap->n != A->cmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU of a BAIJ matrix: square matrices only, rows %d columns %d", A->rmap->n, A->cmap->n);
  if (info->levels < 0.0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Levels of fill negative %d", (int)info->levels);
  if (row || col) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block ILU of a BAIJ matrix: natural ordering only");
  ierr = bilu_refuse_options(F, NULL, NULL);CHKERRQ(ierr);
  HipBlockGet(F)->factored_state = -1;
  HipBlockGet(F)->pat.stale = 1;                                           /* a new symbolic phase: the layout is of the old pattern or level */
  F->ops->lufactornumeric = MatLUFactorNumeric_SeqBAIJHIP;
  return 0;
}

static PetscErrorCode MatSolve_SeqBAIJHIP_ILU(Mat F, Vec b, Vec x) {   /* MatSolve_SeqBAIJ_N_NaturalOrdering, baijfact2.c */
  PetscErrorCode ierr;
  HipBlockFactors *f = HipBlockGet(F);
  const PetscScalar *db; PetscScalar *dx; PetscDeviceCtx *dc;
  int rc = 0;
  if (!f->d_ba) SETERRQ(HipObjComm(F), PETSC_ERR_ARG_WRONGSTATE, "block ILU factor without values");
  if (!f->mbs) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = VecHIPGetRead(b, &db);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(x, &dx);CHKERRQ(ierr);
  if (f->fused) {   /* segment by segment: a run of narrow levels in one chain launch, a wide level in its own */
    const PetscInt *seg = f->pat.segL, *chain = f->pat.segL + f->pat.nlevL + 1;
    for (PetscInt s = 0; s < f->pat.nsegL && !rc; s++) {
      const PetscInt l = seg[s];
      if (chain[s]) rc = mi355x_bilu_lower_chain(dc->h, (int)(seg[s + 1] - l), f->pat.d_levptrL + l, f->pat.d_rowsL, (int)f->bs, f->pat.d_bi, f->pat.d_bj, f->d_ba, db, dx);
      else rc = mi355x_bilu_lower_level(dc->h, f->pat.levptrL[l + 1] - f->pat.levptrL[l], f->pat.d_rowsL + f->pat.levptrL[l], (int)f->bs, f->pat.d_bi, f->pat.d_bj, f->d_ba, db, dx);
    }
    seg = f->pat.segU; chain = f->pat.segU + f->pat.nlevU + 1;
    for (PetscInt s = 0; s < f->pat.nsegU && !rc; s++) {
      const PetscInt l = seg[s];
      if (chain[s]) rc = mi355x_bilu_upper_chain(dc->h, (int)(seg[s + 1] - l), f->pat.d_levptrU + l, f->pat.d_rowsU, (int)f->bs, f->pat.d_bj, f->d_ba, f->pat.d_bdiag, dx);
      else rc = mi355x_bilu_upper_level(dc->h, f->pat.levptrU[l + 1] - f->pat.levptrU[l], f->pat.d_rowsU + f->pat.levptrU[l], (int)f->bs, f->pat.d_bj, f->d_ba, f->pat.d_bdiag, dx);
    }
  } else {
    for (PetscInt l = 0; l < f->pat.nlevL && !rc; l++)
      rc = mi355x_bilu_lower_level(dc->h, f->pat.levptrL[l + 1] - f->pat.levptrL[l], f->pat.d_rowsL + f->pat.levptrL[l], (int)f->bs, f->pat.d_bi, f->pat.d_bj, f->d_ba, db, dx);
    for (PetscInt l = 0; l < f->pat.nlevU && !rc; l++)
      rc = mi355x_bilu_upper_level(dc->h, f->pat.levptrU[l + 1] - f->pat.levptrU[l], f->pat.d_rowsU + f->pat.levptrU[l], (int)f->bs, f->pat.d_bj, f->d_ba, f->pat.d_bdiag, dx);
  }
  ierr = VecHIPRestoreWrite(x);CHKERRQ(ierr);
  HipStateIncrease(x);
  CHKHIP(rc);
  ierr = PetscLogFlops(2.0 * (PetscLogDouble)(f->bs * f->bs) * (PetscLogDouble)f->nzb - (PetscLogDouble)f->bs * (PetscLogDouble)(f->mbs * f->bs));CHKERRQ(ierr);   /* baijfact2.c: 2 bs2 nz - bs n */
  return 0;
}

/* ---------------------------------------------------------------- MatGetFactor */
PetscErrorCode MatGetFactor_seqbaijhipmi355x_petsc(Mat A, MatFactorType ftype, Mat *B) {
  PetscErrorCode ierr;
  HipBlockFactors *f;
  const PetscInt n = A->rmap->n;
  if (ftype != MAT_FACTOR_ILU) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "Factor type not supported for a BAIJ matrix of the HIPMI355X types: block ILU(k) is, ICC, LU and Cholesky are not");
  ierr = PetscMalloc(sizeof(*f), &f);CHKERRQ(ierr);
  memset(f, 0, sizeof(*f));
  f->factored_state = -1;
  ierr = MatCreate(HipObjComm(A), B);CHKERRQ(ierr);
  ierr = MatSetSizes(*B, n, A->cmap->n, n, A->cmap->n);CHKERRQ(ierr);
  ierr = MatSetType(*B, MATSEQAIJHIPMI355X);CHKERRQ(ierr);                /* the container of a factored matrix; the factor hangs off it */
  HipBlockGet(*B) = f;
  (*B)->ops->ilufactorsymbolic = MatILUFactorSymbolic_SeqBAIJHIP;
  (*B)->factortype = ftype;
  return 0;
}
PetscErrorCode MatGetFactorAvailable_seqbaijhipmi355x_petsc(Mat A, MatFactorType ftype, PetscBool *flg) {
  (void)A;
  *flg = (PetscBool)(ftype == MAT_FACTOR_ILU);
  return 0;
}
#endif

/* ---------------------------------------------------------------- introspection, through the PC's public face */
/* block size, dependency levels of the two block solves and stored blocks of the factor of a set-up PCILU over a BAIJ operator */
PetscErrorCode PCBILUGetInfo_HIPMI355X(PC pc, PetscInt *bs, PetscInt *levels_L, PetscInt *levels_U, PetscInt *nz_blocks) {
#if defined(PETSCHIPMI355X_WITH_PETSC)
  (void)bs; (void)levels_L; (void)levels_U; (void)nz_blocks;
  SETERRQ(HipObjComm(pc), PETSC_ERR_SUP, "inside a PETSc tree the BAIJ type composes no factor of its own");
#else
  PetscErrorCode ierr;
  Mat F = NULL;
  ierr = PCFactorGetMatrix(pc, &F);CHKERRQ(ierr);
  if (!F || !F->factortype || !F->spptr || !HipBlockGet(F) || !HipBlockGet(F)->d_ba) SETERRQ(HipObjComm(pc), PETSC_ERR_ARG_WRONG, "not a set-up PCILU over a HIPMI355X block factored matrix");
  const HipBlockFactors *f = HipBlockGet(F);
  if (bs) *bs = f->bs;
  if (levels_L) *levels_L = f->pat.nlevL;
  if (levels_U) *levels_U = f->pat.nlevU;
  if (nz_blocks) *nz_blocks = f->nzb;
  return 0;
#endif
}

/* how one application of the same factor is launched: *fused = 1 under -pc_factor_hipmi355x_trisolve fused, and the launches it makes for
 * L and for U (level route: one per dependency level; fused: one per segment of the plan, a chained run or a wide level) */
PetscErrorCode PCBILUGetSolvePlan_HIPMI355X(PC pc, PetscInt *fused, PetscInt *launches_L, PetscInt *launches_U) {
#if defined(PETSCHIPMI355X_WITH_PETSC)
  (void)fused; (void)launches_L; (void)launches_U;
  SETERRQ(HipObjComm(pc), PETSC_ERR_SUP, "inside a PETSc tree the BAIJ type composes no factor of its own");
#else
  PetscErrorCode ierr;
  Mat F = NULL;
  ierr = PCFactorGetMatrix(pc, &F);CHKERRQ(ierr);
  if (!F || !F->factortype || !F->spptr || !HipBlockGet(F) || !HipBlockGet(F)->d_ba) SETERRQ(HipObjComm(pc), PETSC_ERR_ARG_WRONG, "not a set-up PCILU over a HIPMI355X block factored matrix");
  const HipBlockFactors *f = HipBlockGet(F);
  if (fused) *fused = f->fused ? 1 : 0;
  if (launches_L) *launches_L = f->fused ? f->pat.nsegL : f->pat.nlevL;
  if (launches_U) *launches_U = f->fused ? f->pat.nsegU : f->pat.nlevU;
  return 0;
#endif
}
