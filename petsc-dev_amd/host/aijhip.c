/* MATSEQAIJHIPMI355X (and MATSEQBAIJHIPMI355X): host CSR container for assembly (the part of
 * HipAIJ the path needs: src/mat/impls/aij/seq/aij.h:10-39,99-115; MatSetValues_SeqAIJ aij.c:~330,
 * MatAssemblyEnd_SeqAIJ aij.c:~860) plus the device mirror and the ops the reference's GPU subclass
 * overrides (MatCreate_SeqAIJCUSP, src/mat/impls/aij/seq/seqcusp/aijcusp.cu:657-681): mult, multadd,
 * multtranspose[add], getdiagonal, assemblyend, getvecs, destroy. */
#include "hipmi355ximpl.h"
#include <time.h>

/* the host CSR container: this file's own on the harness, a view of the parent MATSEQAIJ's arrays inside a PETSc tree */
#define SA(A) HipAIJGet(A)
#define SD(A) ((Mat_SeqAIJHIP *)(A)->spptr)
PetscErrorCode MatSeqAIJGetArrays(Mat A, PetscInt *m, const PetscInt **i, const PetscInt **j, const PetscScalar **a);
static PetscErrorCode device_free(Mat A);
static PetscBool device_values_current(Mat A);
/* the device copy is to be built again from the host at its next use */
static unsigned long long pattern_serial = 0;   /* pattern uploads so far, over all matrices */
static void mirror_reset(Mat_SeqAIJHIP *d) { d->uploaded_state = -1; d->pattern_nz = -1; d->pattern_gen = 0; }
/* stored scalars of the container (BAIJ: bs^2 per block); where row r (BAIJ: block row) keeps its diagonal entry (block), -1: nowhere */
static size_t value_count(const HipAIJ *a) { return (size_t)a->nz * (size_t)(a->bs > 1 ? a->bs * a->bs : 1); }
static PetscInt diag_position(const PetscInt *ai, const PetscInt *aj, PetscInt r) {
  for (PetscInt k = ai[r]; k < ai[r + 1]; k++) if (aj[k] == r) return k;
  return -1;
}

#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* inside a PETSc tree the parent type MATSEQAIJ owns the container and its assembly (aij.c) */
/* ---------------------------------------------------------------- host container */
#define CHUNKSIZE 15   /* aij.h: rows grow by this many slots when preallocation is exceeded */
static PetscErrorCode seqaij_prealloc(Mat A, PetscInt nz, const PetscInt *nnz) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  PetscInt m = a->m;
  if (nz == PETSC_DEFAULT || nz == PETSC_DECIDE) nz = 5;   /* aij.c MatSeqAIJSetPreallocation_SeqAIJ */
  if (nz < 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "nz cannot be less than 0: value %d", nz);
  device_free(A);   /* a new pattern is coming: the mirror, plan, index dictionary, transpose and batch map go with the old one */
  HipFree(a->i); HipFree(a->j); HipFree(a->a); HipFree(a->ilen); HipFree(a->imax);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(m + 1), &a->i);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(m, 1), &a->ilen);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(m, 1), &a->imax);CHKERRQ(ierr);
  a->i[0] = 0;
  for (PetscInt r = 0; r < m; r++) {
    PetscInt c = nnz ? nnz[r] : nz;
    if (c < 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "nnz cannot be less than 0: local row %d value %d", r, c);
    a->imax[r] = c; a->ilen[r] = 0; a->i[r + 1] = a->i[r] + c;
  }
  a->maxnz = a->i[m];
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(a->maxnz, 1), &a->j);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(a->maxnz, 1), &a->a);CHKERRQ(ierr);
  a->nz = 0; a->compact = PETSC_FALSE;
  A->preallocated = PETSC_TRUE;
  return 0;
}

/* grow row r by CHUNKSIZE slots (MatSeqXAIJReallocateAIJ, aij.h) */
static PetscErrorCode seqaij_grow(HipAIJ *a, PetscInt r) {
  PetscErrorCode ierr;
  PetscInt m = a->m, add = CHUNKSIZE, newmax = a->i[m] + add;
  PetscInt *nj; PetscScalar *na;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)newmax, &nj);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)newmax, &na);CHKERRQ(ierr);
  PetscInt upto = a->i[r] + a->ilen[r];
  memcpy(nj, a->j, sizeof(PetscInt) * (size_t)upto);
  memcpy(na, a->a, sizeof(PetscScalar) * (size_t)upto);
  PetscInt tail = a->i[m] - a->i[r + 1];
  memcpy(nj + a->i[r + 1] + add, a->j + a->i[r + 1], sizeof(PetscInt) * (size_t)tail);
  memcpy(na + a->i[r + 1] + add, a->a + a->i[r + 1], sizeof(PetscScalar) * (size_t)tail);
  for (PetscInt q = r + 1; q <= m; q++) a->i[q] += add;
  a->imax[r] += add;
  HipFree(a->j); HipFree(a->a);
  a->j = nj; a->a = na; a->maxnz = newmax;
  return 0;
}

/* one entry of MatSetValues_SeqAIJ: sorted insertion into the row, INSERT or ADD on a hit */
static PetscErrorCode seqaij_set(HipAIJ *a, PetscInt r, PetscInt c, PetscScalar v, InsertMode mode, PetscBool *newnz) {
  PetscErrorCode ierr;
  PetscInt *rp = a->j + a->i[r], n = a->ilen[r], lo = 0, hi = n;
  PetscScalar *ap = a->a + a->i[r];
  while (hi - lo > 5) { PetscInt t = (lo + hi) / 2; if (rp[t] > c) hi = t; else lo = t; }
  PetscInt k;
  for (k = lo; k < n; k++) {
    if (rp[k] > c) break;
    if (rp[k] == c) { if (mode == ADD_VALUES) ap[k] += v; else ap[k] = v; return 0; }
  }
  if (n >= a->imax[r]) {
    ierr = seqaij_grow(a, r);CHKERRQ(ierr);
    rp = a->j + a->i[r]; ap = a->a + a->i[r];
  }
  for (PetscInt q = n - 1; q >= k; q--) { rp[q + 1] = rp[q]; ap[q + 1] = ap[q]; }
  rp[k] = c; ap[k] = v;
  a->ilen[r] = n + 1;
  a->nz++;
  if (newnz) *newnz = PETSC_TRUE;
  return 0;
}

/* MatAssemblyEnd_SeqAIJ (aij.c:~860-930): squeeze out the unused slots of every row */
static PetscErrorCode seqaij_compact(HipAIJ *a) {
  PetscInt m = a->m, shift = 0;
  a->nonzerorows = 0;
  for (PetscInt r = 0; r < m; r++) {
    PetscInt start = a->i[r], n = a->ilen[r];
    if (shift) {
      memmove(a->j + start - shift, a->j + start, sizeof(PetscInt) * (size_t)n);
      memmove(a->a + start - shift, a->a + start, sizeof(PetscScalar) * (size_t)n);
    }
    PetscInt slack = a->imax[r] - n;
    a->i[r] = start - shift;
    shift += slack;
    a->imax[r] = n;
    a->nonzerorows += (n > 0);
  }
  a->i[m] -= shift;
  a->nz = a->i[m];
  a->compact = PETSC_TRUE;
  return 0;
}

#else
static PetscErrorCode device_free(Mat A);
#endif

/* Mat_CheckInode (src/mat/impls/aij/seq/inode.c:3964-4034): consecutive rows with identical column lists form a node of
 * at most `limit` rows (-mat_inode_limit, default 5, inode2.c:85-99); with more than 0.8 m nodes -- or -mat_no_inode -- the
 * matrix keeps the plain routines (inode_count = 0). */
typedef struct { const PetscInt *ii, *jj; unsigned char *same; PetscInt m; } InodeCmp;
static void inode_compare_rows(void *c_, PetscInt lo, PetscInt hi) {     /* same[r]: row r + 1 has row r's column list */
  InodeCmp *c = (InodeCmp *)c_;
  for (PetscInt r = lo; r < hi; r++) {
    const PetscInt nzx = c->ii[r + 1] - c->ii[r];
    c->same[r] = (unsigned char)(r + 1 < c->m && c->ii[r + 2] - c->ii[r + 1] == nzx && !memcmp(c->jj + c->ii[r], c->jj + c->ii[r + 1], sizeof(PetscInt) * (size_t)nzx));
  }
}
static PetscErrorCode seqaij_check_inode(Mat A) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  PetscInt m = a->m, limit = 5, i = 0, node_count = 0, *ns;
  PetscBool set; char buf[16];
  HipFree(a->inode_size); a->inode_size = NULL; a->inode_count = 0;
  ierr = PetscOptionsGetString(NULL, "-mat_no_inode", buf, sizeof(buf), &set);CHKERRQ(ierr);
  if (set || !m) return 0;
  ierr = PetscOptionsGetInt(NULL, "-mat_inode_limit", &limit, &set);CHKERRQ(ierr);
  if (limit < 1) limit = 1;
  if (limit > 5) limit = 5;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(m + 1), &ns);CHKERRQ(ierr);
  /* the comparisons (row r + 1 against row r: "the same list as the node's first row" is transitive) are the pass over the
   * column indices and run on host threads; the greedy grouping of the reference's loop then reads one byte per row */
  unsigned char *same;
  ierr = PetscMalloc((size_t)m + 1, &same);CHKERRQ(ierr);
  { InodeCmp ic = {a->i, a->j, same, m};
    HipParallelRanges(m, inode_compare_rows, &ic); }
  while (i < m) {
    PetscInt j, blk_size;
    for (j = i + 1, blk_size = 1; j < m && blk_size < limit; ++j, ++blk_size) if (!same[j - 1]) break;
    ns[node_count++] = blk_size;
    i = j;
  }
  HipFree(same);
  if (node_count > .8 * m) { HipFree(ns); return 0; }
  a->inode_size = ns; a->inode_count = node_count;
  return 0;
}

/* ---------------------------------------------------------------- the type's options
 * -mat_hipmi355x_index_compression, _row_patterns, _pattern_runs, _value_patterns, _tiled, _tiled_stage_min, _blocked, _update_on_device.  MatSetFromOptions (ops->setfromoptions,
 * slot 76, matimpl.h:110; gcreate.c:201-203) reads them under the matrix's own options prefix and keeps them with the matrix; a matrix
 * that was never asked falls back to the global database when its device copy is built (blocks of an MPIAIJ matrix, matrices created
 * by MatCreateSeqAIJWithArrays and used at once). */
static const char *const hopt_name[HOPT_N] = {"-mat_hipmi355x_index_compression", "-mat_hipmi355x_row_patterns", "-mat_hipmi355x_value_patterns",
                                              "-mat_hipmi355x_tiled", "-mat_hipmi355x_tiled_stage_min", "-mat_hipmi355x_blocked",
                                              "-mat_hipmi355x_update_on_device", "-mat_hipmi355x_pattern_runs"};
static PetscErrorCode hip_mat_option(Mat A, int which, PetscInt *val) {
  Mat_SeqAIJHIP *d = SD(A);
  PetscBool set;
  if (d->opt_set[which]) { *val = d->opt[which]; return 0; }
  return PetscOptionsGetInt(NULL, hopt_name[which], val, &set);
}
/* The route options: each picks one of two ways an operation of the matrix runs, by one of two words (route 1: the first, 2: the second).
 * Asked under the matrix's prefix (MatSetFromOptions, at any time) the answer stays with the matrix in route[]; a matrix never asked
 * there reads the global database -- `when` -- and takes the default -- `dflt` -- when the option is given nowhere.  DESIGN.md, "Route
 * options", has the same table in words. */
#ifndef HIPMI355X_RESIDUAL_DEFAULT
#define HIPMI355X_RESIDUAL_DEFAULT 1   /* 1 fused, 2 calls */
#endif
enum { ROUTE_EVERY_USE,    /* the global database is read at every use */
       ROUTE_ONCE,         /* ... at the matrix's first use; the answer, default included, is kept in route[] like one given under the prefix */
       ROUTE_AT_UPLOAD };  /* ... whenever the device copy is built for a new pattern, into residual_global (upload_pattern): the use reads fields only */
static const struct {
  const char *name, *word[2];
  int when;
  int dflt;                /* the route when the option is given nowhere; 0: the first with a device in the process, the second without */
  PetscBool inherited;     /* the result of a product starts with its operand's route[] entry (product_result) */
} hroute[HROUTE_N] = {
  [HROUTE_SOR]        = {"-mat_hipmi355x_sor",        {"device", "host"}, ROUTE_ONCE,      1,                          PETSC_TRUE},
  [HROUTE_PRODUCT]    = {"-mat_hipmi355x_product",    {"device", "host"}, ROUTE_EVERY_USE, 1,                          PETSC_TRUE},
  [HROUTE_REDUCTIONS] = {"-mat_hipmi355x_reductions", {"device", "host"}, ROUTE_ONCE,      0,                          PETSC_FALSE},
  [HROUTE_RESIDUAL]   = {"-mat_hipmi355x_residual",   {"fused", "calls"}, ROUTE_AT_UPLOAD, HIPMI355X_RESIDUAL_DEFAULT, PETSC_FALSE},
  [HROUTE_COARSEN]    = {"-mat_hipmi355x_coarsen",    {"device", "host"}, ROUTE_EVERY_USE, 0,                          PETSC_TRUE},
};
/* the option as given under `prefix` (NULL: the global database); 0: not given there */
static PetscErrorCode route_option(Mat A, int which, const char *prefix, int *route) {
  PetscErrorCode ierr;
  const char *name = hroute[which].name, *const *word = hroute[which].word;
  char kind[16] = ""; PetscBool set = PETSC_FALSE;
  *route = 0;
  ierr = PetscOptionsGetString(prefix, name, kind, sizeof(kind), &set);CHKERRQ(ierr);
  if (!set) return 0;
  if (strcmp(kind, word[0]) && strcmp(kind, word[1])) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "%s <%s|%s>, got %s", name, word[0], word[1], kind);
  *route = strcmp(kind, word[1]) ? 1 : 2;
  return 0;
}
/* the route of an operation that reads the global database when it runs (every entry but ROUTE_AT_UPLOAD's, which MatResidual reads
 * from the struct) */
static PetscErrorCode route_resolve(Mat A, int which, int *route) {
  PetscErrorCode ierr;
  *route = SD(A)->route[which];
  if (!*route) { ierr = route_option(A, which, NULL, route);CHKERRQ(ierr); }
  if (!*route) *route = hroute[which].dflt;
  if (!*route) { int n = 0; *route = (mi355x_device_count(&n) || n < 1) ? 2 : 1; }
  if (hroute[which].when == ROUTE_ONCE) SD(A)->route[which] = *route;
  return 0;
}
static PetscErrorCode MatSetFromOptions_SeqAIJHIP(Mat A) {
  PetscErrorCode ierr;
  Mat_SeqAIJHIP *d = SD(A);
  for (int k = 0; k < HOPT_N; k++) {
    PetscInt v = 0; PetscBool set = PETSC_FALSE;
    ierr = PetscOptionsGetInt(HipObjPrefix(A), hopt_name[k], &v, &set);CHKERRQ(ierr);
    if (set && (!d->opt_set[k] || d->opt[k] != v)) {
      d->opt[k] = v; d->opt_set[k] = PETSC_TRUE;
      if (k != HOPT_UPDATE_DEV) mirror_reset(d);             /* the analyses run again with the new choice */
    }
  }
  for (int k = 0; k < HROUTE_N; k++) {
    int route = 0;
    ierr = route_option(A, k, HipObjPrefix(A), &route);CHKERRQ(ierr);
    if (route) d->route[k] = route;
  }
  return 0;
}

/* ---------------------------------------------------------------- device mirror */
static void form_free(HipDevForm *f) {
  if (f->i) mi355x_free(f->i);
  if (f->j) mi355x_free(f->j);
  if (f->a) mi355x_free(f->a);
  if (f->perm) mi355x_free(f->perm);
  if (f->plan) mi355x_spmv_plan_destroy(f->plan);
  if (f->tiled) mi355x_spmv_tiled_destroy(f->tiled);
  memset(f, 0, sizeof(*f));
}
static void batch_map_free(Mat_SeqAIJHIP *d) {
  if (d->bm_order) mi355x_free(d->bm_order);
  if (d->bm_segptr) mi355x_free(d->bm_segptr);
  if (d->bm_segslot) mi355x_free(d->bm_segslot);
  d->bm_order = d->bm_segptr = d->bm_segslot = NULL;
}
static void value_maps_free(Mat_SeqAIJHIP *d) {   /* what MatShift / MatAXPY / MatCopy keep with the pattern */
  HipFree(d->sh_diag); d->sh_diag = NULL; d->sh_gen = 0;
  HipFree(d->xtoy_h); d->xtoy_h = NULL;
  if (d->xtoy_d) mi355x_free(d->xtoy_d);
  d->xtoy_d = NULL; d->xtoy_xgen = d->xtoy_ygen = 0; d->xtoy_from = NULL;
  d->same_xgen = d->same_ygen = 0;
  HipFree(d->zr_rows_h); HipFree(d->zr_mask_h); d->zr_rows_h = NULL; d->zr_mask_h = NULL;
  if (d->zr_rows_d) mi355x_free(d->zr_rows_d);
  if (d->zr_mask_d) mi355x_free(d->zr_mask_d);
  d->zr_rows_d = NULL; d->zr_mask_d = NULL; d->zr_n = d->zr_words = 0; d->zr_have = PETSC_FALSE;
  /* MatSOR: the level plan and the work arrays of both routes */
  if (d->sor.plan) mi355x_sor_plan_destroy(d->sor.plan);
  if (d->sor.d_idiag) mi355x_free(d->sor.d_idiag);
  if (d->sor.d_mdiag) mi355x_free(d->sor.d_mdiag);
  if (d->sor.d_t) mi355x_free(d->sor.d_t);
  HipFree(d->sor.h_idiag); HipFree(d->sor.h_mdiag); HipFree(d->sor.h_t);
  d->sor.plan = NULL; d->sor.plan_gen = 0; d->sor.d_idiag = d->sor.d_mdiag = d->sor.d_t = NULL; d->sor.have = PETSC_FALSE;
  d->sor.h_idiag = d->sor.h_mdiag = d->sor.h_t = NULL; d->sor.h_have = PETSC_FALSE; d->sor.h_m = 0;
}
/* the arrays of the old pattern go; counts, requests, options, timing and (harness) the triangular factors outlive them */
static PetscErrorCode device_free(Mat A) {
  Mat_SeqAIJHIP *d = SD(A);
  if (!d) return 0;
  { PetscErrorCode ierr = VecHIPProductMatrixChanges(A);CHKERRQ(ierr); }   /* a noted product of this matrix runs while its arrays exist */
  form_free(&d->mat); form_free(&d->t); form_free(&d->b); form_free(&d->tb);
  batch_map_free(d);
  value_maps_free(d);
  if (d->bm_v) mi355x_free(d->bm_v);
  d->bm_v = NULL; d->bm_vcap = 0;
  if (d->red_work) mi355x_free(d->red_work);
  d->red_work = NULL; d->red_cap = 0;
  d->baij4_mfma = PETSC_FALSE;
  mirror_reset(d);
  return 0;
}

/* a form's device arrays from host ones: i (nrows + 1), j (nblocks), perm (nblocks bs^2; optional) and a (optional: else left to the gather
 * through perm).  +16 B past j and a: the SpMV kernels read aligned pairs and the pair holding the last element may extend past it
 * (mi355x_kernels.h).  The row-block plan partitions the VALUE stream, i.e. the row pointer scaled by bs*bs. */
static PetscErrorCode form_upload(PetscDeviceCtx *dc, HipDevForm *f, PetscInt nrows, PetscInt bs, const PetscInt *i, const PetscInt *j,
                                  const PetscInt *perm, const PetscScalar *a) {
  PetscErrorCode ierr;
  const PetscInt nblocks = i[nrows], bs2 = bs * bs;
  const size_t nvals = (size_t)nblocks * (size_t)bs2, cap = (size_t)PetscMax(nblocks, 1) * (size_t)bs2;
  PetscInt *sc;
  CHKHIP(mi355x_malloc((void **)&f->i, sizeof(PetscInt) * (size_t)(nrows + 1)));
  CHKHIP(mi355x_malloc((void **)&f->j, sizeof(PetscInt) * (size_t)PetscMax(nblocks, 1) + 16));
  CHKHIP(mi355x_malloc((void **)&f->a, sizeof(PetscScalar) * cap + 16));
  CHKHIP(mi355x_memcpy_h2d(dc->h, f->i, i, sizeof(PetscInt) * (size_t)(nrows + 1)));
  CHKHIP(mi355x_memcpy_h2d(dc->h, f->j, j, sizeof(PetscInt) * (size_t)nblocks));
  if (perm) {
    CHKHIP(mi355x_malloc((void **)&f->perm, sizeof(PetscInt) * cap));
    CHKHIP(mi355x_memcpy_h2d(dc->h, f->perm, perm, sizeof(PetscInt) * nvals));
  }
  if (a) CHKHIP(mi355x_memcpy_h2d(dc->h, f->a, a, sizeof(PetscScalar) * nvals));
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nrows + 1), &sc);CHKERRQ(ierr);
  for (PetscInt r = 0; r <= nrows; r++) sc[r] = i[r] * bs2;
  CHKHIP(mi355x_spmv_plan_create(dc->h, nrows, sc, NULL, &f->plan));
  CHKHIP(mi355x_handle_synchronize(dc->h));       /* the host arrays are pageable and the caller's to free */
  HipFree(sc);
  f->bs = bs; f->nblocks = nblocks; f->fresh = (PetscBool)(a != NULL);
  return 0;
}
/* after a change of the device values d_a: a derived form's values by one gather through its perm, a tiled layout's copy by its refresh */
static PetscErrorCode form_current(PetscDeviceCtx *dc, HipDevForm *f, const PetscScalar *d_a) {
  if (!f->plan || f->fresh) return 0;
  if (f->perm) CHKHIP(mi355x_pack(dc->h, (size_t)f->nblocks * (size_t)(f->bs * f->bs), f->perm, d_a, f->a));
  if (f->tiled) CHKHIP(mi355x_spmv_tiled_refresh_values(dc->h, f->tiled, f->a));
  f->fresh = PETSC_TRUE;
  return 0;
}
static void forms_stale(Mat_SeqAIJHIP *d) { d->mat.fresh = d->t.fresh = d->b.fresh = d->tb.fresh = PETSC_FALSE; }
/* called just before the device values change in place (MatScale, MatZeroEntries, MatDiagonalScale, MatSetValuesBatch): a noted product
 * of the old values runs first, the derived forms follow by a gather when next used, the value-pattern dictionary no longer describes the
 * values, and the device copy is stamped with the state the wrapper's bump after the op gives the matrix */
static PetscErrorCode device_values_changed(Mat A) {
  PetscErrorCode ierr;
  Mat_SeqAIJHIP *d = SD(A);
  ierr = VecHIPProductMatrixChanges(A);CHKERRQ(ierr);
  forms_stale(d);
  CHKHIP(mi355x_spmv_plan_drop_value_patterns(d->mat.plan));
  d->uploaded_state = HipObjState(A) + 1;
  return 0;
}

/* the transpose of a BCSR pattern (bs = 1: CSR) of nbrows x nbcols blocks by a stable counting sort: each row of the transpose lists its
 * entries in increasing original (block) row, the order MatMultTransposeAdd_SeqAIJ's scatter loop adds them in (aij.c:1100-1112; baij2.c:1740),
 * every bs x bs block transposed (column-major, baij.h:13-30).  map: for each stored value of the pattern, its position in the matrix's value
 * array (NULL: the identity); tperm: the same for each value of the transpose. */
static PetscErrorCode transpose_pattern(PetscInt nbrows, PetscInt nbcols, const PetscInt *bi, const PetscInt *bj, PetscInt bs, const PetscInt *map,
                                        PetscInt **ti_, PetscInt **tj_, PetscInt **tperm_) {
  PetscErrorCode ierr;
  const PetscInt nb = bi[nbrows], bs2 = bs * bs;
  PetscInt *ti, *tj, *tperm, *next;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nbcols + 1), &ti);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nb, 1), &tj);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nb, 1) * (size_t)bs2, &tperm);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nbcols, 1), &next);CHKERRQ(ierr);
  memset(ti, 0, sizeof(PetscInt) * (size_t)(nbcols + 1));
  for (PetscInt k = 0; k < nb; k++) ti[bj[k] + 1]++;
  for (PetscInt c = 0; c < nbcols; c++) ti[c + 1] += ti[c];
  for (PetscInt c = 0; c < nbcols; c++) next[c] = ti[c];
  for (PetscInt r = 0; r < nbrows; r++)
    for (PetscInt k = bi[r]; k < bi[r + 1]; k++) {
      const PetscInt p = next[bj[k]]++;
      tj[p] = r;
      /* entry (row q, column c) of the transposed block is entry (row c, column q) of the block */
      for (PetscInt c = 0; c < bs; c++) for (PetscInt q = 0; q < bs; q++) {
        const size_t src = (size_t)k * bs2 + q * bs + c;
        tperm[(size_t)p * bs2 + c * bs + q] = map ? map[src] : (PetscInt)src;
      }
    }
  HipFree(next);
  *ti_ = ti; *tj_ = tj; *tperm_ = tperm;
  return 0;
}

/* -mat_hipmi355x_tiled <-1|0|1> (default -1 = decide), tl: the column-tiled product (csrc/spmv_tiled.hip) of an m x n pattern, or NULL.
 * Built when asked for, or when `probe` is set and a sample of its 32-row groups shows the gathers landing on lines of x of their own
 * (> 0.5 line per nonzero: rows that share no columns with their neighbours -- the irregular matrices of BASELINE configs[3]) on a matrix
 * large enough for x to leave the L2 (>= 2^17 columns); the transpose (probe not set) builds it whenever the matrix took it.  Kept when asked
 * for, or if at least half of the nonzeros fall into pairs worth staging.  A failed build is an error when the matrix asked for it, else the
 * row-block kernels serve (e.g. no host memory for the layout).  -mat_hipmi355x_tiled_stage_min <n> (default 1024): entries a (panel, tile)
 * pair needs to be staged. */
static PetscErrorCode tiled_decide(Mat A, PetscInt tl, PetscBool probe, PetscInt m, PetscInt n, const PetscInt *ai, const PetscInt *aj,
                                   mi355x_spmv_tiled_t *tiled) {
  PetscErrorCode ierr;
  PetscInt smin = 0; long staged = 0, rest = 0;
  *tiled = NULL;
  ierr = hip_mat_option(A, HOPT_TILED_SMIN, &smin);CHKERRQ(ierr);
  if (probe && tl < 0) {
    double lpn = 0.0;
    if (n < (1 << 17) || ai[m] < (1 << 22)) return 0;
    CHKHIP(mi355x_spmv_tiled_probe(m, ai, aj, &lpn));
    if (!(lpn > 0.5)) return 0;
  }
  const int rc = mi355x_spmv_tiled_build(m, n, ai, aj, (int)smin, tiled);
  if (rc) {
    *tiled = NULL;
    if (probe && tl > 0) CHKHIP(rc);
    return 0;
  }
  CHKHIP(mi355x_spmv_tiled_info(*tiled, &staged, &rest, NULL, NULL, NULL));
  if (tl < 0 && 2 * staged < (long)ai[m]) { mi355x_spmv_tiled_destroy(*tiled); *tiled = NULL; }
  return 0;
}

/* MatCUSPCopyToGPU (aijcusp.cu:126-253): H2D of i, j, a when the host copy is newer.  Unlike the
 * reference, a value-only change (same pattern) re-sends only `a`. */
#if defined(PETSCHIPMI355X_WITH_PETSC)
static PetscErrorCode hipaij_refresh_view_if_stale(Mat A);   /* integration/petsc-3.3/aijhipmi355x_ctor.h */
#endif
/* the blocked companion (see upload_pattern): an AIJ matrix whose nodes are complete bs x bs blocks.  Its block size (0: not of that shape)
 * and number of blocks */
static PetscInt companion_shape(const HipAIJ *a, PetscInt *nblocks) {
  const PetscInt m = a->m, n = a->n, nn = a->inode_count;
  *nblocks = 0;
  if (nn <= 0 || !a->inode_size) return 0;
  const PetscInt bs = a->inode_size[0];
  if (bs < 2 || bs > 5 || nn * bs != m || n % bs) return 0;
  for (PetscInt i = 0; i < nn; i++) if (a->inode_size[i] != bs) return 0;
  /* every node's column list: whole aligned groups of bs consecutive columns (the rows of a node share the list: check its first row) */
  PetscInt nblk = 0;
  for (PetscInt i = 0; i < nn; i++) {
    const PetscInt r = i * bs, k0 = a->i[r], len = a->i[r + 1] - k0;
    if (len % bs) return 0;
    for (PetscInt g = 0; g < len; g += bs) {
      const PetscInt c0 = a->j[k0 + g];
      if (c0 % bs) return 0;
      for (PetscInt q = 1; q < bs; q++) if (a->j[k0 + g + q] != c0 + q) return 0;
    }
    for (PetscInt q = 1; q < bs; q++) if (a->i[r + q + 1] - a->i[r + q] != len) return 0;     /* (Mat_CheckInode compared the lists themselves) */
    nblk += len / bs;
  }
  if ((double)nblk * bs * bs > 2147483000.0) return 0;
  *nblocks = nblk;
  return bs;
}
/* the companion's BCSR pattern on the host: bi, bj and perm, the position in the CSR value array of every block value (column-major) */
static PetscErrorCode companion_pattern(const HipAIJ *a, PetscInt bs, PetscInt nblk, PetscInt **bi_, PetscInt **bj_, PetscInt **perm_) {
  PetscErrorCode ierr;
  const PetscInt nn = a->m / bs, bs2 = bs * bs;
  PetscInt *bi, *bj, *perm;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nn + 1), &bi);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nblk, 1), &bj);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nblk, 1) * (size_t)bs2, &perm);CHKERRQ(ierr);
  bi[0] = 0;
  for (PetscInt i = 0, b = 0; i < nn; i++) {
    const PetscInt r = i * bs, len = a->i[r + 1] - a->i[r];
    for (PetscInt g = 0; g < len; g += bs, b++) {
      bj[b] = a->j[a->i[r] + g] / bs;
      for (PetscInt c = 0; c < bs; c++) for (PetscInt q = 0; q < bs; q++) perm[(size_t)b * bs2 + c * bs + q] = a->i[r + q] + g + c;   /* value (row q, column c) of the block */
    }
    bi[i + 1] = bi[i] + len / bs;
  }
  *bi_ = bi; *bj_ = bj; *perm_ = perm;
  return 0;
}
static PetscErrorCode blocked_companion_build(Mat A, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  PetscInt nblk, *bi, *bj, *perm;
  const PetscInt bs = companion_shape(a, &nblk);
  if (!bs) return 0;
  ierr = companion_pattern(a, bs, nblk, &bi, &bj, &perm);CHKERRQ(ierr);
  ierr = form_upload(dc, &d->b, a->m / bs, bs, bi, bj, perm, NULL);CHKERRQ(ierr);
  HipFree(bi); HipFree(bj); HipFree(perm);
  return 0;
}

/* PETSC_HIPMI355X_SETUP_TIMING=1: the upload's phases on stderr */
typedef struct { int on; double t0; } UpTick;
static void up_tick(UpTick *tk, PetscDeviceCtx *dc, const char *what) {
  struct timespec ts;
  if (!tk->on) return;
  (void)mi355x_handle_synchronize(dc->h);
  clock_gettime(CLOCK_MONOTONIC, &ts);
  const double t = (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
  if (tk->t0 > 0.0) fprintf(stderr, "[hipmi355x]   upload: %-30s %.3f s\n", what, t - tk->t0);
  tk->t0 = t;
}
/* the device forms for the matrix's pattern: the arrays, the plan and the analyses on it */
static PetscErrorCode upload_pattern(Mat A, PetscDeviceCtx *dc, UpTick *tk) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  Mat_SeqAIJHIP *d = SD(A);
  ierr = route_option(A, HROUTE_RESIDUAL, NULL, &d->residual_global);CHKERRQ(ierr);   /* ROUTE_AT_UPLOAD: MatResidual searches no table */
  device_free(A);
  if (a->bs > 1) {   /* BAIJ */
    if (a->bs == 4) {   /* -mat_hipmi355x_baij4 <mfma|fma>: the matrix cores (v_mfma_f64_4x4x4, 16-byte loads: 1.22-1.28 ms at 128^3 nodes, 27
                         * blocks per row; the default -- BASELINE configs[4]'s "MFMA 4x4 tile path") or the row-block FMA kernel with x staged
                         * in LDS (1.25-1.32 ms in the same processes, three boxes: profiles/r03_cfg5.log) */
      char kind[16] = "mfma"; PetscBool set;
      ierr = PetscOptionsGetString(NULL, "-mat_hipmi355x_baij4", kind, sizeof(kind), &set);CHKERRQ(ierr);
      if (strcmp(kind, "mfma") && strcmp(kind, "fma")) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "-mat_hipmi355x_baij4 <mfma|fma>, got %s", kind);
      d->baij4_mfma = (PetscBool)!strcmp(kind, "mfma");
    }
    if ((double)a->nz * a->bs * a->bs > 2147483000.0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "BAIJ matrix too large for 32-bit value offsets");
    ierr = form_upload(dc, &d->mat, a->m, a->bs, a->i, a->j, NULL, NULL);CHKERRQ(ierr);
    up_tick(tk, dc, "row pointer and columns up");
    d->pattern_nz = a->nz; d->pattern_gen = ++pattern_serial; d->cprow = PETSC_FALSE;
    return 0;
  }
  PetscInt m = a->m, nrows = m;
  const PetscInt *ip = a->i; PetscInt *ci = NULL, *ridx = NULL;
  /* compressed rows when >= 60% of the rows are empty (Mat_CheckCompressedRow ratio, compressedrow.c:28;
   * the reference forces it off for B, mpiaij.c:705, because its CPU loop gains little -- on the GPU the
   * off-diagonal block is >99% empty rows and visiting them costs a full pass over y) */
  PetscBool use_cprow = PETSC_FALSE;
  if (d->cprow && m > 0 && (double)(m - a->nonzerorows) > 0.6 * m) {
    use_cprow = PETSC_TRUE;
    nrows = a->nonzerorows;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nrows + 1), &ci);CHKERRQ(ierr);
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nrows, 1), &ridx);CHKERRQ(ierr);
    PetscInt k = 0; ci[0] = 0;
    for (PetscInt r = 0; r < m; r++) if (a->i[r + 1] > a->i[r]) { ridx[k] = r; ci[++k] = a->i[r + 1]; }
    ip = ci;
  }
  CHKHIP(mi355x_malloc((void **)&d->mat.i, sizeof(PetscInt) * (size_t)(nrows + 1)));
  /* +16 B: the SpMV kernels read aligned pairs and the pair holding the last element may extend past it (mi355x_kernels.h) */
  CHKHIP(mi355x_malloc((void **)&d->mat.j, sizeof(PetscInt) * (size_t)PetscMax(a->nz, 1) + 16));
  CHKHIP(mi355x_malloc((void **)&d->mat.a, sizeof(PetscScalar) * (size_t)PetscMax(a->nz, 1) + 16));
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->mat.i, ip, sizeof(PetscInt) * (size_t)(nrows + 1)));
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->mat.j, a->j, sizeof(PetscInt) * (size_t)a->nz));
  d->mat.bs = 1; d->mat.nblocks = a->nz;
  up_tick(tk, dc, "row pointer and columns up");
  PetscInt ic = 1;
  CHKHIP(mi355x_spmv_plan_create(dc->h, nrows, ip, use_cprow ? ridx : NULL, &d->mat.plan));
  up_tick(tk, dc, "row-block plan");
  /* -mat_hipmi355x_index_compression <0|1> (default 1): one byte per nonzero instead of a 4-byte column index
   * when the matrix uses <= 256 distinct (col - row) offsets; plain CSR otherwise */
  ierr = hip_mat_option(A, HOPT_IC, &ic);CHKERRQ(ierr);
  if (ic && !use_cprow) {
    PetscInt rp = 1, pr = 1;
    CHKHIP(mi355x_spmv_plan_compress_indices(dc->h, d->mat.plan, a->i, a->j));
    /* -mat_hipmi355x_row_patterns <0|1> (default 1): stencil matrices whose rows' offset lists come from a small dictionary
     * stream 4 bytes per ROW instead of 1 byte per nonzero + the row pointer (spmv_csr_rowblock_pat_kernel); same bits */
    ierr = hip_mat_option(A, HOPT_RP, &rp);CHKERRQ(ierr);
    CHKHIP(mi355x_spmv_plan_use_patterns(d->mat.plan, rp ? 1 : 0, NULL));
    /* -mat_hipmi355x_pattern_runs <0|1> (default 1): row blocks whose rows form a few runs of equal patterns (grid lines) read one
     * 32-byte descriptor instead of 4 bytes per row; same bits */
    ierr = hip_mat_option(A, HOPT_PR, &pr);CHKERRQ(ierr);
    CHKHIP(mi355x_spmv_plan_use_pattern_runs(d->mat.plan, pr ? 1 : 0, NULL));
    up_tick(tk, dc, "offset / row-pattern dictionaries");
  }
  /* inodes: when the reference's Mat_CheckInode would switch this matrix to MatMult_SeqAIJ_Inode, the row sums take
   * that routine's two-at-a-time order (same bits), and -- unless the 1-byte index dictionary already applies --
   * the rows of a node share one stored column list (mi355x_spmv_plan_group_rows) */
  ierr = seqaij_check_inode(A);CHKERRQ(ierr);
  up_tick(tk, dc, "inode check");
  if (a->inode_count) {
    int ntab = 0;
    CHKHIP(mi355x_spmv_plan_set_pairsum(d->mat.plan, 1));
    CHKHIP(mi355x_spmv_plan_is_compressed(d->mat.plan, &ntab));
    if (!ntab && !use_cprow) CHKHIP(mi355x_spmv_plan_group_rows(dc->h, d->mat.plan, a->i, a->j, a->inode_count, a->inode_size));
  }
  /* -mat_hipmi355x_blocked <-1|0|1> (default -1 = decide): the blocked companion.  When every node Mat_CheckInode found has the same
   * size bs (2..5) and its shared column list is made of whole aligned groups of bs columns -- the 3-dof matrices of FEM codes
   * assembled into AIJ: every coupling a complete bs x bs block -- the matrix IS a BAIJ matrix, and MatMult_SeqBAIJ_bs's kernel
   * reads 8 bs^2 + 4 bytes per block where the grouped-row kernel reads 8 bs^2 + 4 bs: BCSR arrays are laid out beside the CSR ones
   * (block values column-major, baij.h:13-30, as a permutation of d_a kept on the device) and the products take the BCSR row-block
   * kernel: FEM stand-in 0.245 -> 0.197 ms, the same sums bit for bit (profiles/r04_fem_as_baij.log).  Decided here only for rows
   * long enough that the grouped-row kernel does not carry the reference's bits anyway (more than 16 nonzeros per row). */
  if (a->inode_count && !use_cprow) {
    PetscInt bl = -1;
    ierr = hip_mat_option(A, HOPT_BLOCKED, &bl);CHKERRQ(ierr);
    if (bl != 0 && (bl > 0 || (double)a->nz > 16.0 * (double)a->m)) { ierr = blocked_companion_build(A, dc);CHKERRQ(ierr); }
    up_tick(tk, dc, "blocked companion");
  }
  /* the column-tiled product for a matrix that got neither an offset dictionary nor grouped rows: it gathers x once per nonzero */
  {
    PetscInt tl = -1; int ntab = 0, ng = 0; long ngj = 0;
    ierr = hip_mat_option(A, HOPT_TILED, &tl);CHKERRQ(ierr);
    CHKHIP(mi355x_spmv_plan_is_compressed(d->mat.plan, &ntab));
    CHKHIP(mi355x_spmv_plan_group_info(d->mat.plan, &ng, &ngj, NULL));
    if (tl != 0 && !use_cprow && !ntab && !ng && a->nz > 0) {
      ierr = tiled_decide(A, tl, PETSC_TRUE, a->m, a->n, a->i, a->j, &d->mat.tiled);CHKERRQ(ierr);
      up_tick(tk, dc, "column-tiled layout");
    }
  }
  CHKHIP(mi355x_handle_synchronize(dc->h));
  HipFree(ci); HipFree(ridx);
  d->pattern_nz = a->nz; d->pattern_gen = ++pattern_serial;
  if (!use_cprow) d->cprow = PETSC_FALSE;
  return 0;
}
/* the values, into the device copy and the forms that carry them */
static PetscErrorCode upload_values(Mat A, PetscDeviceCtx *dc, PetscBool new_pattern, UpTick *tk) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  Mat_SeqAIJHIP *d = SD(A);
  up_tick(tk, dc, "(grouped rows, bookkeeping)");
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->mat.a, a->a, sizeof(PetscScalar) * (size_t)a->nz * (size_t)(d->mat.bs * d->mat.bs)));
  up_tick(tk, dc, "values up");
  forms_stale(d);
  if (d->b.plan) {
    ierr = form_current(dc, &d->b, d->mat.a);CHKERRQ(ierr);
    up_tick(tk, dc, "blocked companion's values");
  }
  if (d->mat.tiled) {
    if (new_pattern) { CHKHIP(mi355x_spmv_tiled_upload(dc->h, d->mat.tiled, d->mat.a)); CHKHIP(mi355x_spmv_tiled_drop_host(d->mat.tiled)); d->mat.fresh = PETSC_TRUE; }
    else { ierr = form_current(dc, &d->mat, d->mat.a);CHKERRQ(ierr); }
    up_tick(tk, dc, "column-tiled values");
  }
  if (a->bs <= 1 && d->mat.plan) {
    /* -mat_hipmi355x_value_patterns <0|1> (default 1): constant-coefficient operators -- whole rows, offsets and values,
     * from a dictionary of <= 512 entries -- run a kernel that reads 2 bytes per row and no values (spmv_csr_valpat_kernel);
     * same bits.  The dictionary belongs to THESE values: derived again on every upload, dropped by every device-side change. */
    PetscInt vp = 1;
    ierr = hip_mat_option(A, HOPT_VP, &vp);CHKERRQ(ierr);
    CHKHIP(mi355x_spmv_plan_use_value_patterns(d->mat.plan, vp ? 1 : 0, NULL));
    if (vp) CHKHIP(mi355x_spmv_plan_value_patterns(dc->h, d->mat.plan, a->i, a->j, a->a, NULL));
  }
  CHKHIP(mi355x_handle_synchronize(dc->h));
  up_tick(tk, dc, "value-pattern analysis");
  return 0;
}
PetscErrorCode MatSeqAIJHIPUpload(Mat A) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  Mat_SeqAIJHIP *d = SD(A);
  PetscDeviceCtx *dc;
#if defined(PETSCHIPMI355X_WITH_PETSC)
  /* the parent class fills or replaces its arrays on paths that never pass this type's MatAssemblyEnd (MatDuplicate_SeqAIJ,
   * MatCopy, MatConvert set assembled = TRUE themselves): the view of them is checked before every use */
  ierr = hipaij_refresh_view_if_stale(A);CHKERRQ(ierr);
#endif
  if (d->uploaded_state == HipObjState(A) && d->mat.a) return 0;
  ierr = VecHIPProductMatrixChanges(A);CHKERRQ(ierr);      /* (the device copy still holds the values the noted product was asked with) */
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  UpTick tk = {getenv("PETSC_HIPMI355X_SETUP_TIMING") != NULL, 0.0};
  up_tick(&tk, dc, "");
  if (!a->compact) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "matrix must be assembled before it is sent to the GPU");
  const PetscBool new_pattern = (PetscBool)!(d->mat.a && d->mat.plan && d->pattern_nz == a->nz);   /* entries are never removed: same nz == same pattern */
  if (new_pattern) { ierr = upload_pattern(A, dc, &tk);CHKERRQ(ierr); }
  ierr = upload_values(A, dc, new_pattern, &tk);CHKERRQ(ierr);
  d->n_uploads++;
  d->uploaded_state = HipObjState(A);
  return 0;
}

PetscErrorCode MatSeqAIJHIPSetCompressedRow(Mat A, PetscBool flg) { SD(A)->cprow = flg; mirror_reset(SD(A)); return 0; }

/* the transpose products' form, built when missing and with its values current: the blocked companion's block transpose (its values a
 * gather of d_a like the companion's own), else the explicit transpose, built on the host once per pattern -- for BAIJ whenever the
 * matrix moved -- and refreshed on the device when only the values changed */
static PetscErrorCode transpose_current(Mat A, PetscDeviceCtx *dc) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  Mat_SeqAIJHIP *d = SD(A);
  PetscInt *ti, *tj, *tperm;
  /* the device copy of A first: building it discards everything that belonged to an older pattern, the transposes included (device_free) */
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (d->b.plan) {
    if (!d->tb.plan) {
      const PetscInt bs = d->b.bs;
      PetscInt *bi, *bj, *perm;
      ierr = companion_pattern(a, bs, d->b.nblocks, &bi, &bj, &perm);CHKERRQ(ierr);
      ierr = transpose_pattern(a->m / bs, a->n / bs, bi, bj, bs, perm, &ti, &tj, &tperm);CHKERRQ(ierr);
      ierr = form_upload(dc, &d->tb, a->n / bs, bs, ti, tj, tperm, NULL);CHKERRQ(ierr);
      HipFree(bi); HipFree(bj); HipFree(perm); HipFree(ti); HipFree(tj); HipFree(tperm);
    }
    return form_current(dc, &d->tb, d->mat.a);
  }
  if (d->t.plan && d->t.fresh) return 0;
  if (d->t.plan && d->t.perm) {
    /* only the VALUES changed since the transpose was built (a time step, a Newton iteration, MatScale / MatDiagonalScale /
     * MatSetValuesBatch on the device copy): A^T's values are the matrix's values in another order, and that order is on the device.
     * One gather kernel over the current device values; nothing is rebuilt on the host, nothing crosses PCIe beyond what
     * MatSeqAIJHIPUpload needed for the matrix itself. */
    d->t_refreshes++;
    return form_current(dc, &d->t, d->mat.a);
  }
  /* BAIJ (MatMultTranspose_SeqBAIJ / MatMultTransposeAdd_SeqBAIJ, baij2.c:1579, 1740): the block transpose, its values placed on the host
   * (a->m counts block rows, a->n scalar columns) */
  const PetscInt bs = a->bs > 1 ? a->bs : 1, nbc = a->n / bs;
  const size_t nvals = value_count(a);
  PetscScalar *ta;
  form_free(&d->t);
  ierr = transpose_pattern(a->m, nbc, a->i, a->j, bs, NULL, &ti, &tj, &tperm);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * PetscMax(nvals, 1), &ta);CHKERRQ(ierr);
  for (size_t k = 0; k < nvals; k++) ta[k] = a->a[tperm[k]];
  ierr = form_upload(dc, &d->t, nbc, bs, ti, tj, bs > 1 ? NULL : tperm, ta);CHKERRQ(ierr);
  if (bs == 1) {
    /* the transpose of a stencil matrix is a stencil matrix: same index compression / row patterns as the matrix itself */
    PetscInt ic = 1, rp = 1, pr = 1;
    ierr = hip_mat_option(A, HOPT_IC, &ic);CHKERRQ(ierr);
    ierr = hip_mat_option(A, HOPT_RP, &rp);CHKERRQ(ierr);
    ierr = hip_mat_option(A, HOPT_PR, &pr);CHKERRQ(ierr);
    if (ic) {
      CHKHIP(mi355x_spmv_plan_compress_indices(dc->h, d->t.plan, ti, tj));
      CHKHIP(mi355x_spmv_plan_use_patterns(d->t.plan, rp ? 1 : 0, NULL));
      CHKHIP(mi355x_spmv_plan_use_pattern_runs(d->t.plan, pr ? 1 : 0, NULL));
    }
    CHKHIP(mi355x_handle_synchronize(dc->h));
  }
  if (d->mat.tiled) {
    /* the matrix took the column-tiled product (its gathers miss the caches): so do its transpose's, whose rows pick their columns
     * from the same wide windows */
    PetscInt tl = -1;
    ierr = hip_mat_option(A, HOPT_TILED, &tl);CHKERRQ(ierr);
    ierr = tiled_decide(A, tl, PETSC_FALSE, nbc, a->m, ti, tj, &d->t.tiled);CHKERRQ(ierr);
    if (d->t.tiled) { CHKHIP(mi355x_spmv_tiled_upload(dc->h, d->t.tiled, d->t.a)); CHKHIP(mi355x_spmv_tiled_drop_host(d->t.tiled)); }
  }
  HipFree(ti); HipFree(tj); HipFree(tperm); HipFree(ta);
  d->t_builds++;
  return 0;
}

/* ---------------------------------------------------------------- ops */
#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* the parent MATSEQAIJ's job inside a PETSc tree */
static PetscErrorCode MatSetUp_SeqAIJHIP(Mat A) { return seqaij_prealloc(A, PETSC_DEFAULT, NULL); }

static PetscErrorCode MatSetValues_SeqAIJHIP(Mat A, PetscInt m, const PetscInt im[], PetscInt n, const PetscInt in[], const PetscScalar v[], InsertMode is) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  /* a host-side insertion: whatever the device-side updates stamped (MatSetValuesBatch, MatScale, ... look one state
   * bump ahead), the device copy is stale from here on */
  SD(A)->uploaded_state = -1;
  for (PetscInt k = 0; k < m; k++) {
    PetscInt row = im[k];
    if (row < 0) continue;
    if (row >= a->m) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Row too large: row %d max %d", row, a->m - 1);
    for (PetscInt l = 0; l < n; l++) {
      if (in[l] < 0) continue;
      if (in[l] >= a->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Column too large: col %d max %d", in[l], a->n - 1);
      ierr = seqaij_set(a, row, in[l], v[k * n + l], is, NULL);CHKERRQ(ierr);   /* row-oriented values, aij.c roworiented */
    }
  }
  return 0;
}

#endif
/* MatSetValuesBatch (matrix.c:1698; the reference's GPU version aijAssemble.cu:157 sorts and reduces a COO list on every
 * call): nb square blocks of bs x bs values, rows[] = their row = column indices, ADD_VALUES.  With an assembled matrix
 * whose pattern already holds every (row, col) pair -- the re-assembly of a time step or Newton iteration -- the values
 * are assembled ON THE DEVICE through a map built once per connectivity: contributions grouped by nonzero, kept in call
 * order, one lane per nonzero adds them one after the other (mi355x_csr_assemble), so the result carries the bits of the
 * reference's loop of MatSetValues.  The host copy is refreshed from the device afterwards.  Anything else (first
 * assembly, new nonzeros, BAIJ) takes that loop itself. */
static unsigned long long fnv1a(const void *p, size_t nbytes) {
  const unsigned char *c = (const unsigned char *)p; unsigned long long h = 1469598103934665603ULL;
  for (size_t k = 0; k < nbytes; k++) { h ^= c[k]; h *= 1099511628211ULL; }
  return h;
}
static PetscErrorCode batch_map_build(Mat A, PetscInt nb, PetscInt bs, const PetscInt rows[], PetscBool *ok) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  PetscDeviceCtx *dc;
  const size_t T = (size_t)nb * (size_t)bs * (size_t)bs;
  PetscInt *slot = NULL, *count = NULL, *order = NULL, *segptr = NULL, *segslot = NULL;
  *ok = PETSC_FALSE;
  if (T == 0 || T > 2147483000UL) return 0;
  ierr = PetscMalloc(sizeof(PetscInt) * T, &slot);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(a->nz + 1), &count);CHKERRQ(ierr);
  memset(count, 0, sizeof(PetscInt) * (size_t)(a->nz + 1));
  size_t used = 0;
  for (PetscInt b = 0; b < nb; b++) {
    const PetscInt *rb = rows + (size_t)b * bs;
    for (PetscInt i = 0; i < bs; i++) {
      const PetscInt row = rb[i];
      if (row >= a->m) { HipFree(slot); HipFree(count); SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Row too large: row %d max %d", row, a->m - 1); }
      for (PetscInt j = 0; j < bs; j++) {
        const size_t t = ((size_t)b * bs + i) * bs + j;
        const PetscInt col = rb[j];
        slot[t] = -1;
        if (row < 0 || col < 0) continue;                     /* MatSetValues ignores negative indices */
        if (col >= a->n) { HipFree(slot); HipFree(count); SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Column too large: col %d max %d", col, a->n - 1); }
        PetscInt k = a->i[row];
        for (; k < a->i[row + 1]; k++) if (a->j[k] == col) break;
        if (k == a->i[row + 1]) { HipFree(slot); HipFree(count); return 0; }   /* a new nonzero: not a pure value re-assembly */
        slot[t] = k; count[k + 1]++; used++;
      }
    }
  }
  /* counting sort by nonzero, stable in t: the order of the reference's loop */
  PetscInt nseg = 0;
  for (PetscInt k = 0; k < a->nz; k++) if (count[k + 1]) nseg++;
  ierr = PetscMalloc(sizeof(PetscInt) * PetscMax(used, 1), &order);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nseg + 1), &segptr);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nseg, 1), &segslot);CHKERRQ(ierr);
  { PetscInt s = 0, run = 0;
    for (PetscInt k = 0; k < a->nz; k++) { const PetscInt c = count[k + 1]; count[k + 1] = run; if (c) { segptr[s] = run; segslot[s] = k; s++; } run += c; }
    segptr[nseg] = run; }
  for (size_t t = 0; t < T; t++) if (slot[t] >= 0) order[count[slot[t] + 1]++] = (PetscInt)t;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  batch_map_free(d);
  CHKHIP(mi355x_malloc((void **)&d->bm_order, sizeof(PetscInt) * PetscMax(used, 1)));
  CHKHIP(mi355x_malloc((void **)&d->bm_segptr, sizeof(PetscInt) * (size_t)(nseg + 1)));
  CHKHIP(mi355x_malloc((void **)&d->bm_segslot, sizeof(PetscInt) * (size_t)PetscMax(nseg, 1)));
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->bm_order, order, sizeof(PetscInt) * used));
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->bm_segptr, segptr, sizeof(PetscInt) * (size_t)(nseg + 1)));
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->bm_segslot, segslot, sizeof(PetscInt) * (size_t)nseg));
  CHKHIP(mi355x_handle_synchronize(dc->h));
  HipFree(slot); HipFree(count); HipFree(order); HipFree(segptr); HipFree(segslot);
  d->bm_nb = nb; d->bm_bs = bs; d->bm_nseg = nseg; d->bm_T = T;
  d->bm_hash = fnv1a(rows, sizeof(PetscInt) * (size_t)nb * (size_t)bs);
  *ok = PETSC_TRUE;
  return 0;
}
static PetscErrorCode MatSetValuesBatch_SeqAIJHIP(Mat A, PetscInt nb, PetscInt bs, PetscInt rows[], const PetscScalar v[]) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  PetscBool ok = PETSC_FALSE;
  if (a->bs <= 1 && a->compact && A->assembled && nb > 0 && bs > 0 && !d->cprow) {
    ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);               /* device values current before they are added to */
    ok = (PetscBool)(d->bm_order && d->bm_nb == nb && d->bm_bs == bs && d->pattern_nz == a->nz &&
                     d->bm_hash == fnv1a(rows, sizeof(PetscInt) * (size_t)nb * (size_t)bs));
    if (!ok) { ierr = batch_map_build(A, nb, bs, rows, &ok);CHKERRQ(ierr); }
  }
  if (!ok) {                                                   /* the reference's default (matrix.c:1715-1718) */
    for (PetscInt b = 0; b < nb; b++) { ierr = MatSetValues(A, bs, &rows[(size_t)b * bs], bs, &rows[(size_t)b * bs], &v[(size_t)b * bs * bs], ADD_VALUES);CHKERRQ(ierr); }
    return 0;
  }
  PetscDeviceCtx *dc;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  if (d->bm_vcap < d->bm_T) {
    if (d->bm_v) mi355x_free(d->bm_v);
    d->bm_v = NULL;
    CHKHIP(mi355x_malloc((void **)&d->bm_v, sizeof(PetscScalar) * d->bm_T));
    d->bm_vcap = d->bm_T;
  }
  CHKHIP(mi355x_memcpy_h2d(dc->h, d->bm_v, v, sizeof(PetscScalar) * d->bm_T));
  /* MatSetValuesBatch's wrapper leaves the state alone and the MatAssemblyEnd that has to follow bumps it once: the
   * device copy is stamped with that state, so the assembly does not trigger an upload */
  ierr = device_values_changed(A);CHKERRQ(ierr);
  CHKHIP(mi355x_csr_assemble(dc->h, d->bm_nseg, d->bm_segptr, d->bm_segslot, d->bm_order, d->bm_v, d->mat.a));
  CHKHIP(mi355x_memcpy_d2h(dc->h, a->a, d->mat.a, sizeof(PetscScalar) * (size_t)a->nz));   /* host mirror follows */
  CHKHIP(mi355x_handle_synchronize(dc->h));                    /* v and a->a are pageable host memory */
  ierr = PetscLogFlops((PetscLogDouble)d->bm_T);CHKERRQ(ierr);
  return 0;
}

#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* the parent MATSEQAIJ's job inside a PETSc tree */
static PetscErrorCode MatAssemblyEnd_SeqAIJHIP(Mat A, MatAssemblyType mode) {
  if (mode == MAT_FLUSH_ASSEMBLY) return 0;
  /* (the reference re-installs ops->mult here because the inode check may have replaced it,
   *  aijcusp.cu:462-466; this container has no inode variant) */
  return seqaij_compact(SA(A));
}

#endif
static PetscErrorCode MatMult_SeqAIJHIP_device(Mat A, Vec xx, Vec yy);
PetscErrorCode MatMultDiagonalScale_HIPMI355X(Mat A, Vec dd, Vec xx, Vec yy, PetscBool *ok);
/* what the product of A (transpose: of A^T) runs on: the blocked companion or the device copy itself, their transposes for A^T.  The
 * transpose forms are built here when missing and brought up to date; a forward product takes the device copy as it is (its caller
 * uploads) and the forward forms' values are brought up to date in product()'s timed window */
static PetscErrorCode product_form(Mat A, PetscBool transpose, PetscDeviceCtx *dc, HipDevForm **f) {
  Mat_SeqAIJHIP *d = SD(A);
  if (transpose) { PetscErrorCode ierr = transpose_current(A, dc);CHKERRQ(ierr); }
  if (d->b.plan) *f = transpose ? &d->tb : &d->b;
  else *f = transpose ? &d->t : &d->mat;
  return 0;
}
/* z = op(A) x (yy NULL) or z = y + op(A) x (zz may be yy), op(A) = A or A^T (MatMultTranspose: 0 + p1 + p2 ... == p1 + p2 ... bit for bit,
 * so the plain product kernel serves).  The one place that picks the kernel: MatMult_SeqBAIJ_4 on the matrix cores (16-byte stores of y;
 * a vector borrowing storage at an odd offset takes the FMA kernel), the BCSR row-block kernel (BAIJ, the blocked companion and their
 * block transposes), the column-tiled kernel (with the row-block CSR kernel for an x it cannot take), the row-block CSR kernel.  The
 * forward products are timed (MatTimingBegin/End). */
static PetscErrorCode product(Mat A, PetscBool transpose, Vec xx, Vec yy, Vec zz) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscScalar *x, *y = NULL; PetscScalar *z; PetscDeviceCtx *dc; HipDevForm *f = NULL;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = product_form(A, transpose, dc, &f);CHKERRQ(ierr);
  const PetscBool cprow = (PetscBool)(f == &d->mat && f->bs == 1 && d->cprow);   /* rows without entries are not visited */
  ierr = VecHIPGetRead(xx, &x);CHKERRQ(ierr);
  if (!yy) { ierr = VecHIPGetWrite(zz, &z);CHKERRQ(ierr); }
  else if (zz == yy) { ierr = VecHIPGetReadWrite(zz, &z);CHKERRQ(ierr); y = z; }
  else {
    ierr = VecHIPGetRead(yy, &y);CHKERRQ(ierr);
    ierr = VecHIPGetWrite(zz, &z);CHKERRQ(ierr);
    if (cprow) { CHKHIP(mi355x_vec_copy(dc->h, (size_t)a->m, y, z)); y = z; }   /* aij.c:1314-1316 */
  }
  if (!transpose) { ierr = MatTimingBegin(A, dc->h);CHKERRQ(ierr); }
  ierr = form_current(dc, f, d->mat.a);CHKERRQ(ierr);
  if (f == &d->mat && f->bs == 4 && d->baij4_mfma && !y && !(((size_t)z) & 15)) CHKHIP(mi355x_spmv_bsr4_mfma(dc->h, a->m, 0, f->i, f->j, f->a, x, z));
  else if (f->bs > 1 && y) CHKHIP(mi355x_spmv_bsr_planned_add(dc->h, f->plan, (int)f->bs, f->i, f->j, f->a, x, y, z));
  else if (f->bs > 1) CHKHIP(mi355x_spmv_bsr_planned(dc->h, f->plan, (int)f->bs, f->i, f->j, f->a, x, z));
  else {
    int rc = 801;
    if (f->tiled) { rc = mi355x_spmv_tiled(dc->h, f->tiled, x, y, z); if (rc && rc != 801) CHKHIP(rc); }
    if (rc && y) CHKHIP(mi355x_spmv_csr_add(dc->h, f->plan, f->i, f->j, f->a, x, y, z));
    else if (rc) {                                                       /* no tiled form, or an x it cannot take (storage borrowed at an odd offset) */
      if (cprow) CHKHIP(mi355x_vec_set(dc->h, (size_t)a->m, 0.0, z));
      CHKHIP(mi355x_spmv_csr(dc->h, f->plan, f->i, f->j, f->a, x, z));
    }
  }
  if (!transpose) { ierr = MatTimingEnd(A, dc->h);CHKERRQ(ierr); }
  ierr = VecHIPRestoreWrite(zz);CHKERRQ(ierr);
  const PetscInt bs = a->bs > 1 ? a->bs : 1;                           /* aij.c:1281, 1324; baij2.c: 2 bs^2 nz (- bs nonzero block rows) */
  if (transpose) return PetscLogFlops(2.0 * a->nz);
  if (yy) return PetscLogFlops(2.0 * bs * bs * a->nz);
  return PetscLogFlops(2.0 * bs * bs * a->nz - (double)bs * a->nonzerorows);
}
static PetscErrorCode MatMult_SeqAIJHIP(Mat A, Vec xx, Vec yy) {   /* MatMult_SeqAIJCUSP aijcusp.cu:349 */
  PetscErrorCode ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);       /* from here on the device copy holds the values of THIS call */
  /* a point-wise AIJ matrix on one rank: the product is noted with the Vec type (host/vechip.c, "a noted product"): if PCApply_Jacobi
   * follows, the two become one kernel and the work vector in between is never written; anything else runs the product as it is.
   * Whatever changes the device copy afterwards (a new upload, MatScale / MatDiagonalScale / assembly on the device, the matrix going
   * away) first lets a noted product of this matrix run (VecHIPProductMatrixChanges). */
  if (SA(A)->bs <= 1 && !SD(A)->cprow) {
    PetscBool noted = PETSC_FALSE;
    ierr = VecHIPNoteProduct(A, xx, yy, MatMult_SeqAIJHIP_device, MatMultDiagonalScale_HIPMI355X, &noted);CHKERRQ(ierr);
    if (noted) return 0;
  }
  return MatMult_SeqAIJHIP_device(A, xx, yy);
}
static PetscErrorCode MatMult_SeqAIJHIP_device(Mat A, Vec xx, Vec yy) { return product(A, PETSC_FALSE, xx, NULL, yy); }   /* y = A x with the device copy as it is */
static PetscErrorCode MatMultAdd_SeqAIJHIP(Mat A, Vec xx, Vec yy, Vec zz) {   /* MatMultAdd_SeqAIJCUSP aijcusp.cu:405; MatMultAdd_SeqBAIJ_N baij2.c:1168-1480 */
  PetscErrorCode ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  return product(A, PETSC_FALSE, xx, yy, zz);
}
static PetscErrorCode MatMultTranspose_SeqAIJHIP(Mat A, Vec xx, Vec yy) { return product(A, PETSC_TRUE, xx, NULL, yy); }   /* aij.c:1124: VecSet(yy,0); Add */
static PetscErrorCode MatMultTransposeAdd_SeqAIJHIP(Mat A, Vec xx, Vec zz, Vec yy) { return product(A, PETSC_TRUE, xx, zz, yy); }   /* aij.c:1078: yy = zz + A^T xx */

/* "Is this my matrix": a sequential matrix of this type (AIJ or BAIJ: they share the constructor), NULL included in the answer.  What
 * an entry point does with a no is its own: PETSC_ERR_ARG_WRONG with its text (seq_hip_check), zeros, or the diagonal block (seq_block) */
static PetscBool is_seq_hip(Mat A) { return (PetscBool)(A && A->spptr && A->ops->mult == MatMult_SeqAIJHIP); }
static PetscErrorCode seq_hip_check(Mat A, const char *text) {
  if (!is_seq_hip(A)) SETERRQ(A ? HipObjComm(A) : 0, PETSC_ERR_ARG_WRONG, "%s", text);
  return 0;
}
/* the sequential matrix of this type an info call answers for: A itself, or the diagonal block of an MPIAIJ matrix of this type; else NULL */
static PetscErrorCode seq_block(Mat A, Mat *S) {
  PetscErrorCode ierr;
  Mat Ad = NULL;
  *S = NULL;
  if (!A) return 0;
  if (is_seq_hip(A)) { *S = A; return 0; }
  if (!strcmp(HipObjTypeName(A), MATMPIAIJHIPMI355X)) { ierr = MatMPIAIJGetSeqAIJ(A, &Ad, NULL, NULL);CHKERRQ(ierr); }
  if (is_seq_hip(Ad)) *S = Ad;
  return 0;
}
#define CHK_ASSEMBLED(A) do { if (!SA(A)->compact) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "matrix must be assembled"); } while (0)

/* how many times the values of a sequential matrix of this type have crossed to the device (tests: value updates with an
 * unchanged pattern must not add to it) */
PetscErrorCode MatHIPMI355XGetUploadCount(Mat A, PetscInt *n) {
  *n = 0;
  { PetscErrorCode ierr = seq_hip_check(A, "sequential HIPMI355X matrix expected");CHKERRQ(ierr); }
  *n = SD(A)->n_uploads;
  return 0;
}
/* number of distinct (col - row) offsets of the index-compressed SpMV plan, 0 when the matrix streams plain 4-byte
 * column indices (bench.py labels its roofline kernel with it; an MPIAIJ matrix answers for its diagonal block) */
PetscErrorCode MatHIPMI355XGetIndexCompression(Mat A, PetscInt *noffsets) {
  PetscErrorCode ierr; int ntab = 0;
  *noffsets = 0;
  ierr = seq_block(A, &A);CHKERRQ(ierr);
  if (!A) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->mat.plan && SA(A)->bs <= 1) CHKHIP(mi355x_spmv_plan_is_compressed(SD(A)->mat.plan, &ntab));
  *noffsets = ntab;
  return 0;
}

/* the blocked companion of a sequential matrix, if the analysis chose it: block size and number of blocks (0, 0: none) */
PetscErrorCode MatHIPMI355XGetBlockedInfo(Mat A, PetscInt *bs, PetscInt *nblocks) {
  *bs = 0; *nblocks = 0;
  { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }
  if (SD(A)->b.plan) { *bs = SD(A)->b.bs; *nblocks = SD(A)->b.nblocks; }
  return 0;
}

/* the column-tiled form of a sequential matrix's product, if the analysis chose it: nonzeros that gather from LDS tiles / that stay in
 * the CSR remainder (both 0: the row-block kernels run) */
PetscErrorCode MatHIPMI355XGetTiledInfo(Mat A, PetscInt *staged, PetscInt *remainder) {
  PetscErrorCode ierr; long s_ = 0, r_ = 0;
  *staged = 0; *remainder = 0;
  if (!is_seq_hip(A)) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->mat.tiled) CHKHIP(mi355x_spmv_tiled_info(SD(A)->mat.tiled, &s_, &r_, NULL, NULL, NULL));
  *staged = (PetscInt)s_; *remainder = (PetscInt)r_;
  return 0;
}

/* size of the row-pattern dictionary the SpMV plan runs with (0: none, or switched off) */
PetscErrorCode MatHIPMI355XGetRowPatterns(Mat A, PetscInt *npat) {
  PetscErrorCode ierr; int np_ = 0;
  *npat = 0;
  ierr = seq_block(A, &A);CHKERRQ(ierr);
  if (!A) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->mat.plan && SA(A)->bs <= 1) {
    PetscInt rp = 1;
    CHKHIP(mi355x_spmv_plan_use_patterns(SD(A)->mat.plan, -1, &np_));
    ierr = hip_mat_option(A, HOPT_RP, &rp);CHKERRQ(ierr);
    if (!rp) np_ = 0;
  }
  *npat = np_;
  return 0;
}

/* size of the value-pattern dictionary the SpMV runs with right now (0: none -- varying coefficients, switched off, or
 * dropped by a device-side change of the values since the last upload) */
PetscErrorCode MatHIPMI355XGetValuePatterns(Mat A, PetscInt *nvpat) {
  PetscErrorCode ierr; int nv = 0;
  *nvpat = 0;
  ierr = seq_block(A, &A);CHKERRQ(ierr);
  if (!A) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->mat.plan && SA(A)->bs <= 1) CHKHIP(mi355x_spmv_plan_use_value_patterns(SD(A)->mat.plan, -1, &nv));
  *nvpat = nv;
  return 0;
}

/* A/B switch for one matrix (the option -mat_hipmi355x_value_patterns is read at every upload; this overrides it until
 * the next upload): off -> the SpMV streams the value array again; on -> the dictionary is derived from the host copy now */
PetscErrorCode MatHIPMI355XSetValuePatterns(Mat A, PetscBool on) {
  PetscErrorCode ierr; PetscDeviceCtx *dc; Mat S;
  if (!A) return 0;
  ierr = seq_block(A, &S);CHKERRQ(ierr);
  if (!S) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "HIPMI355X AIJ matrix expected");
  A = S;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (!SD(A)->mat.plan || SA(A)->bs > 1) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  CHKHIP(mi355x_spmv_plan_use_value_patterns(SD(A)->mat.plan, on ? 1 : 0, NULL));
  if (on && device_values_current(A)) CHKHIP(mi355x_spmv_plan_value_patterns(dc->h, SD(A)->mat.plan, SA(A)->i, SA(A)->j, SA(A)->a, NULL));
  return 0;
}

/* host builds of the explicit transpose / device-side value refreshes of it so far (tests: a time-stepping caller of
 * MatMultTranspose must not go back to the host for A^T) */
PetscErrorCode MatHIPMI355XGetTransposeCounts(Mat A, PetscInt *builds, PetscInt *refreshes) {
  { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }
  if (builds) *builds = SD(A)->t_builds;
  if (refreshes) *refreshes = SD(A)->t_refreshes;
  return 0;
}

/* the nodes Mat_CheckInode finds (consecutive rows with identical column lists): count and sizes, NULL / 0 when the matrix keeps the
 * plain routines.  For the factorisations (host/ilu.c): the reference solves the factor of such a matrix node by node */
PetscErrorCode MatSeqAIJHIPGetInodes(Mat A, PetscInt *count, const PetscInt **sizes) {
  PetscErrorCode ierr;
  *count = 0; *sizes = NULL;
  if (!is_seq_hip(A)) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);          /* runs Mat_CheckInode's restatement on the current pattern */
  *count = SA(A)->inode_count; *sizes = SA(A)->inode_size;
  return 0;
}

/* row grouping of the SpMV plan: number of nodes Mat_CheckInode found (0: plain routines), groups the device plan stores
 * one column list for (0: the plan streams per-nonzero indices), and the shared indices stored */
PetscErrorCode MatHIPMI355XGetInodeInfo(Mat A, PetscInt *nodes, PetscInt *groups, PetscInt *shared_indices) {
  PetscErrorCode ierr; int ng = 0; long ngj = 0;
  if (nodes) *nodes = 0;
  if (groups) *groups = 0;
  if (shared_indices) *shared_indices = 0;
  ierr = seq_block(A, &A);CHKERRQ(ierr);
  if (!A) return 0;
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->mat.plan && SA(A)->bs <= 1) CHKHIP(mi355x_spmv_plan_group_info(SD(A)->mat.plan, &ng, &ngj, NULL));
  if (nodes) *nodes = SA(A)->inode_count;
  if (groups) *groups = ng;
  if (shared_indices) *shared_indices = (PetscInt)ngj;
  return 0;
}

/* w = A p with dpi = p'w as a by-product of the same pass (KSPSolve_CG cg.c:190-191); dpi is left in the device
 * scratch slot the fused CG update reads (all-reduced there when the vectors' communicator has an RCCL communicator).
 * *ok = PETSC_FALSE and nothing done unless A is a square, sequential AIJ matrix of this type whose product kernel is one of the
 * row-block kernels that also leave the per-block sums (value patterns, row patterns, 8-bit column offsets). */
PetscErrorCode MatMultTDotBegin_HIPMI355X(Mat A, Vec xx, Vec yy, PetscBool *ok) {
  PetscErrorCode ierr;
  *ok = PETSC_FALSE;
  if (!is_seq_hip(A)) return 0;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscScalar *x; PetscScalar *y; PetscDeviceCtx *dc; int ntab = 0;
  if (a->bs > 1 || d->cprow || a->m != a->n || xx == yy) return 0;
  if (xx->map->n != a->n || yy->map->n != a->m || (HipCommSize(HipObjComm(xx)) > 1 && !HipCommDevice(HipObjComm(xx)))) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (!d->mat.plan) return 0;
  CHKHIP(mi355x_spmv_plan_dot_available(d->mat.plan, d->mat.a, &ntab));   /* a plan whose kernel also leaves the per-block sums: patterns or 8-bit offsets */
  if (!ntab) return 0;
  ierr = VecHIPGetRead(xx, &x);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(yy, &y);CHKERRQ(ierr);
  ierr = MatTimingBegin(A, dc->h);CHKERRQ(ierr);
  CHKHIP(mi355x_spmv_csr_dot(dc->h, d->mat.plan, d->mat.i, d->mat.j, d->mat.a, x, y));
  ierr = MatTimingEnd(A, dc->h);CHKERRQ(ierr);
  double *slot = mi355x_handle_device_scratch(dc->h) + PETSC_HIP_DPI_SLOT;
  CHKHIP(mi355x_spmv_dot_finish(dc->h, d->mat.plan, slot));
  if (HipCommDevice(HipObjComm(xx))) CHKHIP(mi355x_comm_allreduce_sum(HipCommDevice(HipObjComm(xx)), dc->h, slot, 1));
  ierr = VecHIPRestoreWrite(yy);CHKERRQ(ierr);
  HipStateIncrease(yy);
  ierr = PetscLogFlops(2.0 * a->nz - a->nonzerorows + 2.0 * a->m - 1);CHKERRQ(ierr);
  *ok = PETSC_TRUE;
  return 0;
}

/* "MatMultDiagonalScale_C": y = d .* (A x), i.e. MatMult followed by PCApply_Jacobi's VecPointwiseMult(y, w, d) (jacobi.c:266)
 * with the scaling in the product's epilogue: the intermediate vector is neither written nor read.  Same bits as the two calls. */
PetscErrorCode MatMultDiagonalScale_HIPMI355X(Mat A, Vec dd, Vec xx, Vec yy, PetscBool *ok) {
  PetscErrorCode ierr;
  *ok = PETSC_FALSE;
  if (!is_seq_hip(A)) return 0;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscScalar *x, *dg; PetscScalar *y; PetscDeviceCtx *dc;
  if (a->bs > 1 || xx == yy || dd == yy || xx->map->n != a->n || yy->map->n != a->m || dd->map->n != a->m) return 0;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (!d->mat.plan || d->cprow || d->mat.tiled || d->b.plan) return 0;         /* (the column-tiled and the blocked product have no scaling epilogue: the two calls stay two) */
  ierr = VecHIPGetRead(xx, &x);CHKERRQ(ierr);
  ierr = VecHIPGetRead(dd, &dg);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(yy, &y);CHKERRQ(ierr);
  ierr = MatTimingBegin(A, dc->h);CHKERRQ(ierr);
  CHKHIP(mi355x_spmv_csr_scaled(dc->h, d->mat.plan, d->mat.i, d->mat.j, d->mat.a, x, dg, y));
  ierr = MatTimingEnd(A, dc->h);CHKERRQ(ierr);
  ierr = VecHIPRestoreWrite(yy);CHKERRQ(ierr);
  HipStateIncrease(yy);
  ierr = PetscLogFlops(2.0 * a->nz - a->nonzerorows + a->m);CHKERRQ(ierr);
  *ok = PETSC_TRUE;
  return 0;
}

/* "MatResidual_C": r = b - A x.  Fused: the product's row sum and one subtraction from b_r in the product's own launch
 * (mi355x_spmv_csr_residual, every row-block form), where MatMult + VecAYPX write the work vector, read it again and read b: the same
 * bits, two vector passes fewer.  The column-tiled product, the blocked companion and a compressed-row plan have no such epilogue, and
 * vectors of another type have no device array: MatMult and VecAYPX(r, -1, b) run as they are.  Pending deferred Vec work and stale
 * device values are settled as in MatMult_SeqAIJHIP: the upload first, the deferred queue by the vectors' accessors.
 * -mat_hipmi355x_residual (the route table's ROUTE_AT_UPLOAD entry): two fields of the struct are read per residual, no options table
 * is searched.  README "Multigrid" has the measurement behind the default. */
static int vec_on_device(Vec v) { return v && v->data && strstr(HipObjTypeName(v), "hipmi355x") != NULL; }   /* a vector of the HIPMI355X types */
static PetscErrorCode MatResidual_SeqAIJHIP(Mat A, Vec bb, Vec xx, Vec rr) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  int route;
  if (rr == xx || rr == bb) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_IDN, "r must differ from b and from x");
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);   /* (builds the device copy if need be, and with it reads the global option) */
  route = d->route[HROUTE_RESIDUAL] ? d->route[HROUTE_RESIDUAL] : d->residual_global ? d->residual_global : HIPMI355X_RESIDUAL_DEFAULT;
  if (route == 1 && a->bs <= 1 && vec_on_device(bb) && vec_on_device(xx) && vec_on_device(rr) &&
      xx->map->n == a->n && bb->map->n == a->m && rr->map->n == a->m) {
    if (d->mat.plan && !d->cprow && !d->mat.tiled && !d->b.plan) {
      const PetscScalar *x, *b; PetscScalar *r; PetscDeviceCtx *dc;
      ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
      ierr = VecHIPGetRead(xx, &x);CHKERRQ(ierr);
      ierr = VecHIPGetRead(bb, &b);CHKERRQ(ierr);
      ierr = VecHIPGetWrite(rr, &r);CHKERRQ(ierr);
      ierr = MatTimingBegin(A, dc->h);CHKERRQ(ierr);
      CHKHIP(mi355x_spmv_csr_residual(dc->h, d->mat.plan, d->mat.i, d->mat.j, d->mat.a, x, b, r));
      ierr = MatTimingEnd(A, dc->h);CHKERRQ(ierr);
      ierr = VecHIPRestoreWrite(rr);CHKERRQ(ierr);
      HipStateIncrease(rr);
      ierr = PetscLogFlops(2.0 * a->nz - a->nonzerorows + a->m);CHKERRQ(ierr);
      d->residual_fused++;
      return 0;
    }
  }
  ierr = MatMult_SeqAIJHIP(A, xx, rr);CHKERRQ(ierr);   /* (MatMult's own slot: sizes were checked by the caller) */
  HipStateIncrease(rr);
  ierr = VecAYPX(rr, -1.0, bb);CHKERRQ(ierr);
  d->residual_calls++;
  return 0;
}
PetscErrorCode MatHIPMI355XGetResidualCounts(Mat A, PetscInt *fused, PetscInt *calls) {
  { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }
  if (fused) *fused = SD(A)->residual_fused;
  if (calls) *calls = SD(A)->residual_calls;
  return 0;
}

static PetscErrorCode MatGetDiagonal_SeqAIJHIP(Mat A, Vec v) {   /* aij.c:1040 */
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  PetscScalar *dv; PetscDeviceCtx *dc;
  if (v->map->n != A->rmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Nonconforming matrix and vector");
  if (a->bs > 1 || d->cprow) {   /* host route for the rarely used shapes */
    PetscScalar *h;
    ierr = VecGetArray(v, &h);CHKERRQ(ierr);
    if (a->bs > 1) {
      PetscInt bs = a->bs, mbs = a->m;                 /* BAIJ: a->m counts block rows */
      for (PetscInt r = 0; r < mbs * bs; r++) h[r] = 0.0;
      for (PetscInt br = 0; br < mbs; br++) {
        const PetscInt k = diag_position(a->i, a->j, br);
        if (k >= 0) for (PetscInt q = 0; q < bs; q++) h[br * bs + q] = a->a[(size_t)k * bs * bs + q * bs + q];
      }
    } else {
      for (PetscInt r = 0; r < a->m; r++) { const PetscInt k = diag_position(a->i, a->j, r); h[r] = k >= 0 ? a->a[k] : 0.0; }
    }
    return VecRestoreArray(v, &h);
  }
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  ierr = VecHIPGetWrite(v, &dv);CHKERRQ(ierr);
  CHKHIP(mi355x_csr_get_diagonal(dc->h, a->m, d->mat.i, d->mat.j, d->mat.a, dv));
  return VecHIPRestoreWrite(v);
}

/* Value updates with an unchanged pattern: the host copy and the device copy are updated side by side, so
 * the next MatMult finds the device values current and nothing crosses PCIe (the reference's GPU back end re-sent the
 * whole matrix after every such call, aijcusp.cu:138-152).  The wrappers in mat.c bump the object state AFTER the op:
 * the device copy is stamped with that future state (device_values_changed); the derived forms follow by a gather. */
static PetscBool device_values_current(Mat A) {
  Mat_SeqAIJHIP *d = SD(A);
  return (PetscBool)(d->mat.a && d->uploaded_state == HipObjState(A) && SA(A)->bs <= 1);
}
static PetscBool update_on_device(Mat A) {   /* -mat_hipmi355x_update_on_device <1|0>, with MatShift below */
  PetscInt v = 1;
  if (hip_mat_option(A, HOPT_UPDATE_DEV, &v)) return PETSC_TRUE;
  return (PetscBool)(v != 0);
}
/* The device-side step of a value update.  updates_device: the update of the host copy also runs on the device copy -- its values are
 * current, and, where they apply to the operation, by_option: -mat_hipmi355x_update_on_device says so; no_cprow: the device copy is not
 * a compressed-row form.  Then one of: device_update_begin just before the kernels that change the values (dc: the stream to queue them
 * on); device_update_skipped when the host copy alone was changed (the values travel at the next use); device_update_none when
 * neither copy changes (a current device copy stays current over the wrapper's bump) */
static PetscBool updates_device(Mat A, PetscBool by_option, PetscBool no_cprow) {
  if (!device_values_current(A) || (no_cprow && SD(A)->cprow)) return PETSC_FALSE;
  return (PetscBool)(!by_option || update_on_device(A));
}
static PetscErrorCode device_update_begin(Mat A, PetscDeviceCtx **dc) {
  PetscErrorCode ierr = PetscDeviceGet(dc);CHKERRQ(ierr);
  return device_values_changed(A);
}
static void device_update_skipped(Mat A) { SD(A)->uploaded_state = -1; }
static void device_update_none(Mat A) { if (device_values_current(A)) SD(A)->uploaded_state = HipObjState(A) + 1; }
static PetscErrorCode MatScale_SeqAIJHIP(Mat A, PetscScalar alpha) {   /* MatScale_SeqAIJ: dscal on a->a */
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const size_t vals = value_count(a);
  const PetscBool on_device = (PetscBool)(updates_device(A, PETSC_FALSE, PETSC_FALSE) && alpha != 0.0);   /* alpha == 0: signs of zero, take the upload */
  for (size_t k = 0; k < vals; k++) a->a[k] = alpha * a->a[k];
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(A, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_vec_scale(dc->h, vals, alpha, d->mat.a));
  } else device_update_skipped(A);
  return PetscLogFlops((PetscLogDouble)vals);
}
static PetscErrorCode MatZeroEntries_SeqAIJHIP(Mat A) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  size_t vals = (size_t)(a->compact ? a->nz : a->maxnz) * (size_t)(a->bs > 1 ? a->bs * a->bs : 1);
  const PetscBool on_device = (PetscBool)(updates_device(A, PETSC_FALSE, PETSC_FALSE) && a->compact);
  memset(a->a, 0, sizeof(PetscScalar) * vals);
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(A, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_memset(dc->h, d->mat.a, 0, sizeof(PetscScalar) * vals));
  } else device_update_skipped(A);
  return 0;
}
/* MatDiagonalScale_SeqAIJ, aij.c:2055-2092: left scaling pass, then right scaling pass ((a*l)*r) */
static PetscErrorCode MatDiagonalScale_SeqAIJHIP(Mat A, Vec ll, Vec rr) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscScalar *l = NULL, *r = NULL;
  CHK_ASSEMBLED(A);
  if (a->bs > 1) {   /* MatDiagonalScale_SeqBAIJ, baij2.c:2026-2084: blocks column-major, v[r + c bs] *= l[row bs + r], then *= r[col bs + c]; on the
                      * host copy (a set-up operation of this type); the wrapper's state bump sends the values to the device at the next use */
    const PetscInt bs = a->bs, bs2 = bs * bs, mbs = a->m;
    if (ll && ll->map->n != mbs * bs) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Left scaling vector wrong length");
    if (rr && rr->map->n != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Right scaling vector wrong length");
    if (ll) {
      ierr = VecGetArrayRead(ll, &l);CHKERRQ(ierr);
      for (PetscInt i = 0; i < mbs; i++) {
        const PetscScalar *li = l + (size_t)i * bs;
        PetscScalar *v = a->a + (size_t)bs2 * a->i[i];
        for (PetscInt j = a->i[i]; j < a->i[i + 1]; j++) for (PetscInt k = 0; k < bs2; k++) (*v++) *= li[k % bs];
      }
      ierr = VecRestoreArrayRead(ll, &l);CHKERRQ(ierr);
      ierr = PetscLogFlops((PetscLogDouble)a->nz);CHKERRQ(ierr);       /* (the reference logs the block count, baij2.c:2060) */
    }
    if (rr) {
      ierr = VecGetArrayRead(rr, &r);CHKERRQ(ierr);
      for (PetscInt i = 0; i < mbs; i++) {
        PetscScalar *v = a->a + (size_t)bs2 * a->i[i];
        for (PetscInt j = a->i[i]; j < a->i[i + 1]; j++) {
          const PetscScalar *ri = r + (size_t)bs * a->j[j];
          for (PetscInt k = 0; k < bs; k++) { const PetscScalar x = ri[k]; for (PetscInt t = 0; t < bs; t++) v[t] *= x; v += bs; }
        }
      }
      ierr = VecRestoreArrayRead(rr, &r);CHKERRQ(ierr);
      ierr = PetscLogFlops((PetscLogDouble)a->nz);CHKERRQ(ierr);
    }
    device_update_skipped(A);
    return 0;
  }
  if (ll && ll->map->n != a->m) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Left scaling vector wrong length");
  if (rr && rr->map->n != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Right scaling vector wrong length");
  if (updates_device(A, PETSC_FALSE, PETSC_TRUE)) {   /* device pointers first: fetching the host arrays below must not be what makes them stale */
    const PetscScalar *dl = NULL, *dr = NULL; PetscDeviceCtx *dc;
    if (ll) { ierr = VecHIPGetRead(ll, &dl);CHKERRQ(ierr); }
    if (rr) { ierr = VecHIPGetRead(rr, &dr);CHKERRQ(ierr); }
    ierr = device_update_begin(A, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_csr_diagonal_scale(dc->h, a->m, d->mat.i, d->mat.j, d->mat.a, dl, dr));
  } else device_update_skipped(A);
  if (ll) {
    ierr = VecGetArrayRead(ll, &l);CHKERRQ(ierr);
    for (PetscInt i = 0; i < a->m; i++) for (PetscInt k = a->i[i]; k < a->i[i + 1]; k++) a->a[k] *= l[i];
    ierr = VecRestoreArrayRead(ll, &l);CHKERRQ(ierr);
    ierr = PetscLogFlops((PetscLogDouble)a->nz);CHKERRQ(ierr);
  }
  if (rr) {
    ierr = VecGetArrayRead(rr, &r);CHKERRQ(ierr);
    for (PetscInt k = 0; k < a->nz; k++) a->a[k] *= r[a->j[k]];
    ierr = VecRestoreArrayRead(rr, &r);CHKERRQ(ierr);
    ierr = PetscLogFlops((PetscLogDouble)a->nz);CHKERRQ(ierr);
  }
  return 0;
}

/* MatShift, MatAXPY and MatCopy (axpy.c:170 MatShift; aij.c:2600-2660 MatAXPY_SeqAIJ, 2663-2690 MatCopy_SeqAIJ) on the same model: the
 * host copy by loops on host threads, and -- when the device copy is current -- the same update queued on the device, no host wait.
 * -mat_hipmi355x_update_on_device <1|0> (default 1; per matrix, for these three only): 0 updates the host copy alone and the values
 * travel at the next use, the route a program took before these slots existed.  BAIJ, compressed-row forms: host copy only. */
/* the serial number of A's pattern upload while the host pattern still is that pattern (entries are never removed: same nz), else 0 */
static unsigned long long host_pattern_gen(Mat A) {
  Mat_SeqAIJHIP *d = SD(A);
  return (d->pattern_gen && SA(A)->compact && d->pattern_nz == SA(A)->nz) ? d->pattern_gen : 0;
}
static PetscErrorCode value_op_view(Mat A) {   /* inside a PETSc tree the parent may have replaced its arrays since the view was taken */
#if defined(PETSCHIPMI355X_WITH_PETSC)
  PetscErrorCode ierr = hipaij_refresh_view_if_stale(A);CHKERRQ(ierr);
#endif
  (void)A;
  return 0;
}
typedef struct { PetscScalar *a; const PetscInt *pos, *ai, *aj; const PetscScalar *x; PetscScalar alpha; PetscInt *out; } ValUpd;
static void upd_find_diag(void *c_, PetscInt lo, PetscInt hi) {
  ValUpd *c = (ValUpd *)c_;
  for (PetscInt r = lo; r < hi; r++) c->out[r] = diag_position(c->ai, c->aj, r);
}
static void upd_shift(void *c_, PetscInt lo, PetscInt hi) { ValUpd *c = (ValUpd *)c_; for (PetscInt r = lo; r < hi; r++) c->a[c->pos[r]] = c->a[c->pos[r]] + c->alpha; }
static void upd_axpy(void *c_, PetscInt lo, PetscInt hi) { ValUpd *c = (ValUpd *)c_; for (PetscInt k = lo; k < hi; k++) c->a[k] = c->a[k] + c->alpha * c->x[k]; }
static void upd_copy(void *c_, PetscInt lo, PetscInt hi) { ValUpd *c = (ValUpd *)c_; memcpy(c->a + lo, c->x + lo, sizeof(PetscScalar) * (size_t)(hi - lo)); }
static void upd_axpy_map(void *c_, PetscInt lo, PetscInt hi) {
  ValUpd *c = (ValUpd *)c_;
  for (PetscInt k = lo; k < hi; k++) { const PetscInt t = c->pos[k]; c->a[t] = c->a[t] + c->alpha * c->x[k]; }
}
/* where every row's diagonal entry is; full: a square matrix every row of which has one -- decided once per pattern upload */
static PetscErrorCode shift_diag_positions(Mat A, const PetscInt **pos, PetscBool *full) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const unsigned long long gen = host_pattern_gen(A);
  *pos = NULL; *full = PETSC_FALSE;
  if (!(d->sh_diag && gen && d->sh_gen == gen)) {
    PetscInt *p;
    HipFree(d->sh_diag); d->sh_diag = NULL; d->sh_gen = 0; d->sh_full = PETSC_FALSE;
    if (a->m != a->n) return 0;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(a->m, 1), &p);CHKERRQ(ierr);
    { ValUpd u = {NULL, NULL, a->i, a->j, NULL, 0.0, p};
      HipParallelRanges(a->m, upd_find_diag, &u); }
    d->sh_full = PETSC_TRUE;
    for (PetscInt r = 0; r < a->m; r++) if (p[r] < 0) { d->sh_full = PETSC_FALSE; break; }
    d->sh_diag = p; d->sh_gen = gen;
  }
  *pos = d->sh_diag; *full = d->sh_full;
  return 0;
}
static PetscErrorCode MatShift_SeqAIJHIP(Mat A, PetscScalar alpha) {
  PetscErrorCode ierr;
  HipAIJ *a; Mat_SeqAIJHIP *d = SD(A);
  const PetscInt *pos; PetscBool full;
  ierr = value_op_view(A);CHKERRQ(ierr);
  a = SA(A);
  CHK_ASSEMBLED(A);
  if (a->bs > 1) {   /* BAIJ: the diagonal of every diagonal block (column-major blocks), on the host copy; the values travel at the next use */
    const PetscInt bs = a->bs, bs2 = bs * bs;
    for (PetscInt br = 0; br < a->m; br++) if (diag_position(a->i, a->j, br) < 0) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "block row %d has no diagonal block", br);
    for (PetscInt br = 0; br < a->m; br++) {
      const PetscInt k = diag_position(a->i, a->j, br);
      for (PetscInt q = 0; q < bs; q++) a->a[(size_t)k * bs2 + q * bs + q] = a->a[(size_t)k * bs2 + q * bs + q] + alpha;
    }
    device_update_skipped(A);
    return PetscLogFlops((PetscLogDouble)a->m * bs);
  }
  ierr = shift_diag_positions(A, &pos, &full);CHKERRQ(ierr);
  if (!full) {   /* the reference's default (axpy.c:185-192): new entries may appear -- today's pattern-change route */
    PetscInt rs = A->rmap->rstart, re = A->rmap->rend;
    for (PetscInt i = rs; i < re; i++) { ierr = MatSetValues(A, 1, &i, 1, &i, &alpha, ADD_VALUES);CHKERRQ(ierr); }
    ierr = MatAssemblyBegin(A, MAT_FINAL_ASSEMBLY);CHKERRQ(ierr);
    ierr = MatAssemblyEnd(A, MAT_FINAL_ASSEMBLY);CHKERRQ(ierr);
    return PetscLogFlops((PetscLogDouble)a->m);
  }
  const PetscBool on_device = updates_device(A, PETSC_TRUE, PETSC_TRUE);
  { ValUpd u = {a->a, pos, NULL, NULL, NULL, alpha, NULL};
    HipParallelRanges(a->m, upd_shift, &u); }
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(A, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_csr_shift(dc->h, a->m, d->mat.i, d->mat.j, alpha, d->mat.a, NULL));
  } else device_update_skipped(A);
#if defined(PETSCHIPMI355X_WITH_PETSC)
  HipStateIncrease(A);   /* MatShift of 3.3 leaves the state to the assembly of its default loop: what device_values_changed stamped is this bump */
#endif
  return PetscLogFlops((PetscLogDouble)a->m);
}

/* SAME_NONZERO_PATTERN claimed for X and Y: sizes and nz always, the arrays by one memcmp per pair of pattern uploads */
static PetscErrorCode same_pattern(Mat Y, Mat X, const PetscInt *xcols, const PetscInt *ycols, PetscBool *same) {
  HipAIJ *x = SA(X), *y = SA(Y); Mat_SeqAIJHIP *dy = SD(Y);
  *same = PETSC_FALSE;
  if (x->m != y->m || x->n != y->n || x->nz != y->nz) return 0;
  if (X == Y) { *same = PETSC_TRUE; return 0; }
  const unsigned long long gx = host_pattern_gen(X), gy = host_pattern_gen(Y);
  if (!xcols && !ycols && gx && gy && dy->same_xgen == gx && dy->same_ygen == gy) { *same = PETSC_TRUE; return 0; }
  if (memcmp(x->i, y->i, sizeof(PetscInt) * (size_t)(x->m + 1)) || memcmp(x->j, y->j, sizeof(PetscInt) * (size_t)x->nz)) return 0;
  if ((xcols || ycols) && (!xcols || !ycols || memcmp(xcols, ycols, sizeof(PetscInt) * (size_t)(x->bs > 1 ? x->n / x->bs : x->n)))) return 0;
  if (!xcols && !ycols && gx && gy) { dy->same_xgen = gx; dy->same_ygen = gy; }
  *same = PETSC_TRUE;
  return 0;
}
/* the map of a subset update of Y by X, kept with Y: on the host, and on the device when asked.  *bad_row >= 0: X has an entry in that
 * row that Y lacks, no map */
static PetscErrorCode subset_map_get(Mat Y, Mat X, const PetscInt *xcols, const PetscInt *ycols, PetscBool fresh, PetscBool want_dev, PetscInt *bad_row) {
  PetscErrorCode ierr;
  HipAIJ *x = SA(X), *y = SA(Y); Mat_SeqAIJHIP *dy = SD(Y);
  const unsigned long long gx = host_pattern_gen(X), gy = host_pattern_gen(Y);
  /* (the column translations of two off-diagonal blocks change only with their patterns, which then lose their serial numbers);
   * fresh: the caller has just had the map built for this very pair (MatValueOpsCheck_SeqAIJHIP) and nothing happened since */
  const PetscBool keyed = (PetscBool)(gx && gy && dy->xtoy_xgen == gx && dy->xtoy_ygen == gy);
  *bad_row = -1;
  if (!(dy->xtoy_h && dy->xtoy_from == (void *)X && dy->xtoy_nz == x->nz && (keyed || fresh))) {
    PetscInt *map; int bad = -1;
    HipFree(dy->xtoy_h); dy->xtoy_h = NULL;
    if (dy->xtoy_d) mi355x_free(dy->xtoy_d);
    dy->xtoy_d = NULL; dy->xtoy_xgen = dy->xtoy_ygen = 0; dy->xtoy_from = NULL;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(x->nz, 1), &map);CHKERRQ(ierr);
    const int rc = mi355x_csr_subset_map(x->m, x->i, x->j, xcols, y->i, y->j, ycols, map, &bad);
    if (rc) {
      HipFree(map);
      if (bad < 0) CHKHIP(rc);
      *bad_row = bad;
      return 0;
    }
    dy->xtoy_h = map; dy->xtoy_nz = x->nz; dy->xtoy_from = (void *)X;
    dy->xtoy_xgen = gx; dy->xtoy_ygen = gy;
  }
  if (want_dev && !dy->xtoy_d && x->nz > 0) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    CHKHIP(mi355x_malloc((void **)&dy->xtoy_d, sizeof(PetscInt) * (size_t)x->nz));
    CHKHIP(mi355x_memcpy_h2d(dc->h, dy->xtoy_d, dy->xtoy_h, sizeof(PetscInt) * (size_t)x->nz));
    CHKHIP(mi355x_handle_synchronize(dc->h));       /* once per map: the host array is pageable */
  }
  return 0;
}
static PetscErrorCode value_op_pair(Mat Y, Mat X, PetscBool cols) {   /* what MatAXPY and MatCopy ask of their two matrices */
  PetscErrorCode ierr;
  if (!is_seq_hip(X) || !is_seq_hip(Y)) SETERRQ(Y ? HipObjComm(Y) : 0, PETSC_ERR_SUP, "both matrices must be sequential HIPMI355X matrices");
  ierr = value_op_view(X);CHKERRQ(ierr);
  ierr = value_op_view(Y);CHKERRQ(ierr);
  HipAIJ *x = SA(X), *y = SA(Y);
  if (!x->compact || !y->compact) SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_WRONGSTATE, "both matrices must be assembled");
  if (x->m != y->m || (!cols && x->n != y->n) || (x->bs > 1 ? x->bs : 1) != (y->bs > 1 ? y->bs : 1)) SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_SIZ, "Non conforming matrices: %d x %d and %d x %d", x->m, x->n, y->m, y->n);
  return 0;
}
/* Y's update by an AXPY (or a basic copy into it) runs on the device copy too */
static PetscBool axpy_on_device(Mat Y) { return updates_device(Y, PETSC_TRUE, PETSC_TRUE); }
/* the errors MatAXPY (copy: MatCopy) of this pair would return, with nothing changed.  When Y's device copy will take the update, a source
 * that is not current is sent first (reading it is a use; its pattern upload keys the map); a map built here serves the call that follows
 * (its `checked` argument) */
PetscErrorCode MatValueOpsCheck_SeqAIJHIP(Mat Y, Mat X, MatStructure str, const PetscInt *xcols, const PetscInt *ycols, PetscBool copy) {
  PetscErrorCode ierr;
  PetscBool same = PETSC_FALSE; PetscInt bad;
  ierr = value_op_pair(Y, X, (PetscBool)(xcols || ycols));CHKERRQ(ierr);
  if (X != Y && axpy_on_device(Y)) { ierr = MatSeqAIJHIPUpload(X);CHKERRQ(ierr); }
  if (str == SAME_NONZERO_PATTERN) {
    ierr = same_pattern(Y, X, xcols, ycols, &same);CHKERRQ(ierr);
    if (same) return 0;
    if (!copy) SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_WRONG, "SAME_NONZERO_PATTERN given, but the nonzero patterns of X and Y differ");
  }
  if (SA(Y)->bs > 1) SETERRQ(HipObjComm(Y), PETSC_ERR_SUP, "block matrices: SAME_NONZERO_PATTERN with equal patterns only");
  ierr = subset_map_get(Y, X, xcols, ycols, PETSC_FALSE, PETSC_FALSE, &bad);CHKERRQ(ierr);
  if (bad >= 0) {
    if (str == DIFFERENT_NONZERO_PATTERN && !copy) SETERRQ(HipObjComm(Y), PETSC_ERR_SUP, "X has an entry in local row %d that Y lacks: an update that changes Y's nonzero pattern is not supported", bad);
    SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_WRONG, "the nonzero pattern of X is not a subset of Y's: X has an entry in local row %d that Y lacks", bad);
  }
  return 0;
}
/* ya[xtoy[k]] += alpha xa[k] on the host copy and, when Y's device copy is current, on the device; zero_first: Y's values zeroed before
 * (MatCopy_Basic: MatZeroEntries, then every entry of the source set) */
static PetscErrorCode axpy_subset(Mat Y, PetscScalar alpha, Mat X, const PetscInt *xcols, const PetscInt *ycols, PetscBool zero_first) {
  PetscErrorCode ierr;
  HipAIJ *x = SA(X), *y = SA(Y); Mat_SeqAIJHIP *dx = SD(X), *dy = SD(Y);
  PetscInt bad;
  if (zero_first) {   /* the existing operator; its stamp looks one state bump ahead */
    ierr = MatZeroEntries_SeqAIJHIP(Y);CHKERRQ(ierr);
    HipStateIncrease(Y);
  }
  const PetscBool on_device = axpy_on_device(Y);
  if (on_device && X != Y) { ierr = MatSeqAIJHIPUpload(X);CHKERRQ(ierr); }   /* (the check has sent a source that was not current) */
  ierr = subset_map_get(Y, X, xcols, ycols, PETSC_TRUE, on_device, &bad);CHKERRQ(ierr);
  if (bad >= 0) SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_WRONG, "the nonzero pattern of X is not a subset of Y's (local row %d)", bad);
  { ValUpd u = {y->a, dy->xtoy_h, NULL, NULL, x->a, alpha, NULL};
    HipParallelRanges(x->nz, upd_axpy_map, &u); }
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(Y, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_csr_axpy_map(dc->h, x->nz, dy->xtoy_d, alpha, dx->mat.a, dy->mat.a));
  } else device_update_skipped(Y);
  return 0;
}
PetscErrorCode MatAXPY_SeqAIJHIP_Cols(Mat Y, PetscScalar alpha, Mat X, MatStructure str, const PetscInt *xcols, const PetscInt *ycols, PetscBool checked) {
  PetscErrorCode ierr;
  if (!checked) { ierr = MatValueOpsCheck_SeqAIJHIP(Y, X, str, xcols, ycols, PETSC_FALSE);CHKERRQ(ierr); }
  HipAIJ *x = SA(X), *y = SA(Y); Mat_SeqAIJHIP *dx = SD(X), *dy = SD(Y);
  if (str == SAME_NONZERO_PATTERN) {   /* daxpy on the value arrays: alpha == 0 returns at once (so does mi355x_vec_axpy) */
    const size_t vals = value_count(y);
    const PetscBool on_device = axpy_on_device(Y);
    if (alpha == 0.0) {
      device_update_none(Y);
      return PetscLogFlops(2.0 * (PetscLogDouble)value_count(x));
    }
    if (on_device && X != Y) { ierr = MatSeqAIJHIPUpload(X);CHKERRQ(ierr); }
    { ValUpd u = {y->a, NULL, NULL, NULL, x->a, alpha, NULL};
      HipParallelRanges((PetscInt)vals, upd_axpy, &u); }
    if (on_device) {
      PetscDeviceCtx *dc;
      ierr = device_update_begin(Y, &dc);CHKERRQ(ierr);
      CHKHIP(mi355x_vec_axpy(dc->h, vals, alpha, dx->mat.a, dy->mat.a));
    } else device_update_skipped(Y);
  } else {
    ierr = axpy_subset(Y, alpha, X, xcols, ycols, PETSC_FALSE);CHKERRQ(ierr);
  }
  return PetscLogFlops(2.0 * (PetscLogDouble)value_count(x));
}
static PetscErrorCode MatAXPY_SeqAIJHIP(Mat Y, PetscScalar alpha, Mat X, MatStructure str) {
  PetscErrorCode ierr = MatAXPY_SeqAIJHIP_Cols(Y, alpha, X, str, NULL, NULL, PETSC_FALSE);CHKERRQ(ierr);
#if defined(PETSCHIPMI355X_WITH_PETSC)
  HipStateIncrease(Y);   /* MatAXPY of 3.3 (axpy.c:26-56) does not bump the state after the slot: what device_values_changed stamped is this bump */
#endif
  return 0;
}
PetscErrorCode MatCopy_SeqAIJHIP_Cols(Mat A, Mat B, MatStructure str, const PetscInt *acols, const PetscInt *bcols, PetscBool checked) {
  PetscErrorCode ierr;
  PetscBool same = PETSC_FALSE;
  if (A == B) return 0;
  if (!checked) { ierr = MatValueOpsCheck_SeqAIJHIP(B, A, str, acols, bcols, PETSC_TRUE);CHKERRQ(ierr); }
  HipAIJ *a = SA(A), *b = SA(B); Mat_SeqAIJHIP *da = SD(A), *db = SD(B);
  if (str == SAME_NONZERO_PATTERN) { ierr = same_pattern(B, A, acols, bcols, &same);CHKERRQ(ierr); }
  if (!same) return axpy_subset(B, 1.0, A, acols, bcols, PETSC_TRUE);   /* any other structure: MatCopy_Basic */
  const size_t vals = value_count(a);
  /* B's own values do not matter: its device arrays for this pattern do.  B becomes current when A is (A is sent first when it is not) */
  const PetscBool on_device = (PetscBool)(update_on_device(B) && b->bs <= 1 && !da->cprow && !db->cprow && db->mat.a && db->mat.plan && host_pattern_gen(B));
  if (on_device) { ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr); }
  { ValUpd u = {b->a, NULL, NULL, NULL, a->a, 0.0, NULL};
    HipParallelRanges((PetscInt)vals, upd_copy, &u); }
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(B, &dc);CHKERRQ(ierr);
    CHKHIP(mi355x_memcpy_d2d(dc->h, db->mat.a, da->mat.a, sizeof(PetscScalar) * vals));
  } else device_update_skipped(B);
  return 0;
}
static PetscErrorCode MatCopy_SeqAIJHIP(Mat A, Mat B, MatStructure str) { return MatCopy_SeqAIJHIP_Cols(A, B, str, NULL, NULL, PETSC_FALSE); }

/* MatZeroRows and MatZeroRowsColumns (MatZeroRows_SeqAIJ, MatZeroRowsColumns_SeqAIJ, aij.c) on the same model when the pattern is kept --
 * MatZeroRowsColumns always, MatZeroRows with MAT_KEEP_NONZERO_PATTERN: the host copy by a loop over the rows on host threads and, when the
 * device copy is current, the same update queued on the device (mi355x_csr_zero_columns, mi355x_csr_zero_rows), b with it, no host wait.
 * The list and its bitmap stay with the matrix: a loop that fixes the same boundary every step sends them once.
 * MatZeroRows without the option (the reference's default) removes the rows' entries from the pattern: host copy only, then the type's
 * pattern-change route -- the device forms go and the next use builds them again.
 * BAIJ: PETSC_ERR_SUP; a compressed-row form: host copy only.  Every error is raised before anything is changed. */
#define ZR_LISTED(mask, c) (((mask)[(c) >> 5] >> ((c) & 31)) & 1u)
typedef struct { const PetscInt *ai, *aj; PetscScalar *a; const unsigned int *mask; PetscScalar diag; const PetscScalar *x; PetscScalar *b; PetscBool cols; } ZeroUpd;
static void upd_zero_rows(void *c_, PetscInt lo, PetscInt hi) {
  ZeroUpd *c = (ZeroUpd *)c_;
  const PetscBool set = (PetscBool)(c->diag != 0.0);
  for (PetscInt r = lo; r < hi; r++) {
    if (ZR_LISTED(c->mask, r)) {   /* each entry written once: +0.0, or diag on the diagonal */
      for (PetscInt k = c->ai[r]; k < c->ai[r + 1]; k++) c->a[k] = (set && c->aj[k] == r) ? c->diag : 0.0;
      if (c->b) c->b[r] = c->diag * c->x[r];
    } else if (c->cols) {
      for (PetscInt k = c->ai[r]; k < c->ai[r + 1]; k++) if (ZR_LISTED(c->mask, c->aj[k])) {
        if (c->b) c->b[r] = c->b[r] - c->a[k] * c->x[c->aj[k]];
        c->a[k] = 0.0;
      }
    }
  }
}
/* the list of this call with the matrix: kept when it is the list of the last call, else built again; on the device when asked */
static PetscErrorCode zero_rows_list(Mat A, PetscInt n, const PetscInt rows[], PetscBool want_dev) {
  PetscErrorCode ierr;
  Mat_SeqAIJHIP *d = SD(A);
  const PetscInt m = SA(A)->m, words = PetscMax((m + 31) / 32, 1);
  if (!(d->zr_have && d->zr_n == n && d->zr_words == words && (!n || !memcmp(d->zr_rows_h, rows, sizeof(PetscInt) * (size_t)n)))) {
    HipFree(d->zr_rows_h); HipFree(d->zr_mask_h); d->zr_rows_h = NULL; d->zr_mask_h = NULL; d->zr_have = PETSC_FALSE;
    if (d->zr_rows_d) mi355x_free(d->zr_rows_d);
    if (d->zr_mask_d) mi355x_free(d->zr_mask_d);
    d->zr_rows_d = NULL; d->zr_mask_d = NULL;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(n, 1), &d->zr_rows_h);CHKERRQ(ierr);
    ierr = PetscMalloc(sizeof(unsigned int) * (size_t)words, &d->zr_mask_h);CHKERRQ(ierr);
    memset(d->zr_mask_h, 0, sizeof(unsigned int) * (size_t)words);
    for (PetscInt q = 0; q < n; q++) { d->zr_rows_h[q] = rows[q]; d->zr_mask_h[rows[q] >> 5] |= 1u << (rows[q] & 31); }
    d->zr_n = n; d->zr_words = words; d->zr_have = PETSC_TRUE;
  }
  if (want_dev && !d->zr_rows_d) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    CHKHIP(mi355x_malloc((void **)&d->zr_rows_d, sizeof(PetscInt) * (size_t)PetscMax(n, 1)));
    CHKHIP(mi355x_malloc((void **)&d->zr_mask_d, sizeof(unsigned int) * (size_t)words));
    CHKHIP(mi355x_memcpy_h2d(dc->h, d->zr_rows_d, d->zr_rows_h, sizeof(PetscInt) * (size_t)n));
    CHKHIP(mi355x_memcpy_h2d(dc->h, d->zr_mask_d, d->zr_mask_h, sizeof(unsigned int) * (size_t)words));
    CHKHIP(mi355x_handle_synchronize(dc->h));       /* once per list: the host arrays are pageable */
    d->zr_list_uploads++;
  }
  return 0;
}
/* what both operations ask of the matrix and the list, and the diagonal rules of the forms that keep the pattern */
static PetscErrorCode zero_rows_check(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, PetscBool keep, PetscBool cols) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  CHK_ASSEMBLED(A);
  if (a->bs > 1) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "MatZeroRows / MatZeroRowsColumns on scalar rows of a block matrix");
  for (PetscInt q = 0; q < n; q++) if (rows[q] < 0 || rows[q] >= a->m) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "row %d out of range [0,%d)", rows[q], a->m);
  if (cols && a->m != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Only works for square matrices: %d x %d", a->m, a->n);
  if (diag != 0.0) {
    if (a->m != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "a nonzero diagonal value on a matrix that is not square: %d x %d", a->m, a->n);
    if (keep) {   /* MatMissingDiagonal_SeqAIJ on the whole matrix, as the reference asks it */
      const PetscInt *pos; PetscBool full;
      ierr = shift_diag_positions(A, &pos, &full);CHKERRQ(ierr);
      if (!full) for (PetscInt r = 0; r < a->m; r++) if (pos[r] < 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry in row %d", r);
    }
  }
  return 0;
}
static PetscErrorCode zero_rows_keep_pattern(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb, PetscBool cols) {
  PetscErrorCode ierr;
  HipAIJ *a; Mat_SeqAIJHIP *d = SD(A);
  ierr = value_op_view(A);CHKERRQ(ierr);
  a = SA(A);
  ierr = zero_rows_check(A, n, rows, diag, PETSC_TRUE, cols);CHKERRQ(ierr);
  if (!n) { device_update_none(A); return 0; }
  const PetscBool on_device = updates_device(A, PETSC_TRUE, PETSC_TRUE);
  const PetscScalar *x = NULL, *dx = NULL; PetscScalar *b = NULL, *db = NULL;
  ierr = zero_rows_list(A, n, rows, on_device);CHKERRQ(ierr);
  if (xx && on_device) {   /* the vectors stay on the device: b is updated there */
    ierr = VecHIPGetRead(xx, &dx);CHKERRQ(ierr);
    ierr = VecHIPGetReadWrite(bb, &db);CHKERRQ(ierr);
  } else if (xx) {
    ierr = VecGetArrayRead(xx, &x);CHKERRQ(ierr);
    ierr = VecGetArray(bb, &b);CHKERRQ(ierr);
  }
  { ZeroUpd u = {a->i, a->j, a->a, d->zr_mask_h, diag, x, b, cols};
    HipParallelRanges(a->m, upd_zero_rows, &u); }
  if (xx && !on_device) {
    ierr = VecRestoreArrayRead(xx, &x);CHKERRQ(ierr);
    ierr = VecRestoreArray(bb, &b);CHKERRQ(ierr);
  }
  if (on_device) {
    PetscDeviceCtx *dc;
    ierr = device_update_begin(A, &dc);CHKERRQ(ierr);
    /* the two kernels write disjoint entries and disjoint rows of b: the columns of the rows that are not listed, then the listed rows */
    if (cols) CHKHIP(mi355x_csr_zero_columns(dc->h, d->mat.plan, d->mat.i, d->mat.j, d->mat.a, d->zr_mask_d, dx, db));
    CHKHIP(mi355x_csr_zero_rows(dc->h, (int)n, d->zr_rows_d, d->mat.i, d->mat.j, d->mat.a, diag, dx, db));
    if (xx) { ierr = VecHIPRestoreWrite(bb);CHKERRQ(ierr); HipStateIncrease(bb); }   /* as the host route's VecRestoreArray does */
    d->zr_device_updates++;
  } else device_update_skipped(A);
  return 0;
}
static PetscErrorCode zero_rows_new_pattern(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb);   /* per flavour, below */
static PetscBool keep_nonzero_pattern(Mat A);
static PetscErrorCode MatZeroRows_SeqAIJHIP(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb) {
  if (keep_nonzero_pattern(A)) return zero_rows_keep_pattern(A, n, rows, diag, xx, bb, PETSC_FALSE);
  return zero_rows_new_pattern(A, n, rows, diag, xx, bb);
}
static PetscErrorCode MatZeroRowsColumns_SeqAIJHIP(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb) {
  return zero_rows_keep_pattern(A, n, rows, diag, xx, bb, PETSC_TRUE);
}
/* uploads of a row list to the device / updates that ran on the device copy so far (tests: the same list given again is not sent again) */
PetscErrorCode MatHIPMI355XGetZeroRowsCounts(Mat A, PetscInt *list_uploads, PetscInt *device_updates) {
  { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }
  if (list_uploads) *list_uploads = SD(A)->zr_list_uploads;
  if (device_updates) *device_updates = SD(A)->zr_device_updates;
  return 0;
}
#if !defined(PETSCHIPMI355X_WITH_PETSC)
static PetscBool keep_nonzero_pattern(Mat A) { return SA(A)->keepnonzeropattern; }
static PetscErrorCode MatSetOption_SeqAIJHIP(Mat A, MatOption op, PetscBool flg) {   /* MatSetOption_SeqAIJ, aij.c: the one option this container acts on */
  if (op == MAT_KEEP_NONZERO_PATTERN) SA(A)->keepnonzeropattern = flg;
  return 0;
}
/* the else branch of MatZeroRows_SeqAIJ: a listed row keeps (r, r) = diag in its first slot (diag != 0; a row without a slot gets one
 * inserted) or nothing, the rows are squeezed as after an assembly, and the device forms of the old pattern go */
static PetscErrorCode zero_rows_new_pattern(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  ierr = zero_rows_check(A, n, rows, diag, PETSC_FALSE, PETSC_FALSE);CHKERRQ(ierr);
  if (xx) {
    const PetscScalar *x; PetscScalar *b;
    ierr = VecGetArrayRead(xx, &x);CHKERRQ(ierr);
    ierr = VecGetArray(bb, &b);CHKERRQ(ierr);
    for (PetscInt q = 0; q < n; q++) b[rows[q]] = diag * x[rows[q]];
    ierr = VecRestoreArrayRead(xx, &x);CHKERRQ(ierr);
    ierr = VecRestoreArray(bb, &b);CHKERRQ(ierr);
  }
  if (!n) { device_update_none(A); return 0; }
  ierr = device_free(A);CHKERRQ(ierr);
  for (PetscInt q = 0; q < n; q++) {
    const PetscInt r = rows[q];
    if (diag != 0.0) {
      if (a->ilen[r] > 0) { a->ilen[r] = 1; a->a[a->i[r]] = diag; a->j[a->i[r]] = r; }
      else { ierr = seqaij_set(a, r, r, diag, INSERT_VALUES, NULL);CHKERRQ(ierr); }
    } else a->ilen[r] = 0;
  }
  return seqaij_compact(a);
}
#endif

/* MatSOR (MatSOR_SeqAIJ, aij.c:1463; the inverted diagonal of MatInvertDiagonal_SeqAIJ): its * lits point sweeps of the enabled directions,
 * the first one in the zero-guess form when SOR_ZERO_INITIAL_GUESS is set.  A matrix with inodes takes the point sweeps too (the reference
 * under -mat_no_inode).
 * Device route: the matrix's own device arrays (sent first when the host copy is newer, as for a product), the vectors on the device, the
 * sweeps level by level (csrc/sor.hip); t, the two diagonals and the level plan stay with the matrix -- the plan for one pattern upload,
 * the diagonals for one upload state and one (omega, fshift).  No host wait per call.
 * Host route: the same loops on the host copy -- a compressed-row form, or -mat_hipmi355x_sor host (the route table).  Same bits: one
 * product and one difference per entry, in storage order, on both.
 * Every error is raised before anything is written. */
enum { SOR_FWD_BITS = SOR_FORWARD_SWEEP | SOR_LOCAL_FORWARD_SWEEP, SOR_BWD_BITS = SOR_BACKWARD_SWEEP | SOR_LOCAL_BACKWARD_SWEEP };
#define SOR_MINUS_DOT(sum, k0, k1) do { for (PetscInt k_ = (k0); k_ < (k1); k_++) (sum) -= aa[k_] * x[aj[k_]]; } while (0)
static void sor_host_sweeps(const HipAIJ *a, const PetscInt *pos, const PetscScalar *idiag, const PetscScalar *mdiag, PetscReal omega, int flag,
                            PetscInt its, const PetscScalar *b, PetscScalar *t, PetscScalar *x) {
  const PetscInt m = a->m, *ai = a->i, *aj = a->j; const PetscScalar *aa = a->a;
  const PetscBool fwd = (PetscBool)((flag & SOR_FWD_BITS) != 0), bwd = (PetscBool)((flag & SOR_BWD_BITS) != 0);
  if (flag & SOR_ZERO_INITIAL_GUESS) {
    const PetscScalar *xb = b;
    if (fwd) {
      for (PetscInt i = 0; i < m; i++) { PetscScalar sum = b[i]; SOR_MINUS_DOT(sum, ai[i], pos[i]); t[i] = sum; x[i] = sum * idiag[i]; }
      xb = t;
    }
    if (bwd) for (PetscInt i = m - 1; i >= 0; i--) {
      PetscScalar sum = xb[i];
      SOR_MINUS_DOT(sum, pos[i] + 1, ai[i + 1]);
      if (xb == b) x[i] = sum * idiag[i];
      else x[i] = (1. - omega) * x[i] + sum * idiag[i];
    }
    its--;
  }
  while (its--) {
    if (fwd) for (PetscInt i = 0; i < m; i++) {
      PetscScalar sum = b[i];
      SOR_MINUS_DOT(sum, ai[i], ai[i + 1]);
      x[i] = (1. - omega) * x[i] + (sum + mdiag[i] * x[i]) * idiag[i];
    }
    if (bwd) for (PetscInt i = m - 1; i >= 0; i--) {
      PetscScalar sum = b[i];
      SOR_MINUS_DOT(sum, ai[i], ai[i + 1]);
      x[i] = (1. - omega) * x[i] + (sum + mdiag[i] * x[i]) * idiag[i];
    }
  }
}
/* what MatInvertDiagonal_SeqAIJ refuses, on the host copy: a row without a diagonal entry; a stored zero that would be inverted as it is */
static PetscErrorCode sor_diag_check(Mat A, PetscReal omega, PetscReal fshift, const PetscInt **pos_) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  const PetscInt *pos; PetscBool full;
  ierr = shift_diag_positions(A, &pos, &full);CHKERRQ(ierr);
  if (!full) for (PetscInt r = 0; r < a->m; r++) if (pos[r] < 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Matrix is missing diagonal entry in row %d", r);
  if (omega == 1.0 && fshift == 0.0) for (PetscInt r = 0; r < a->m; r++) if (a->a[pos[r]] == 0.0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_INCOMP, "Zero diagonal on row %d", r);
  *pos_ = pos;
  return 0;
}
static PetscErrorCode sor_on_host(Mat A, Vec bb, PetscReal omega, int flag, PetscReal fshift, PetscInt its, Vec xx) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscInt m = a->m, *pos = NULL;
  const PetscScalar *b; PetscScalar *x;
  const PetscBool fresh = (PetscBool)(d->sor.h_have && d->sor.h_m == m && d->sor.h_state == HipObjState(A) && d->sor.h_omega == omega && d->sor.h_fshift == fshift);
  ierr = sor_diag_check(A, omega, fshift, &pos);CHKERRQ(ierr);
  if (!fresh) {
    if (d->sor.h_m != m || !d->sor.h_idiag) {
      HipFree(d->sor.h_idiag); HipFree(d->sor.h_mdiag); HipFree(d->sor.h_t); d->sor.h_idiag = d->sor.h_mdiag = d->sor.h_t = NULL; d->sor.h_have = PETSC_FALSE;
      ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(m, 1), &d->sor.h_idiag);CHKERRQ(ierr);
      ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(m, 1), &d->sor.h_mdiag);CHKERRQ(ierr);
      ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(m, 1), &d->sor.h_t);CHKERRQ(ierr);
      d->sor.h_m = m;
    }
    for (PetscInt i = 0; i < m; i++) {
      const PetscScalar v = a->a[pos[i]];
      d->sor.h_mdiag[i] = v;
      d->sor.h_idiag[i] = (omega == 1.0 && fshift == 0.0) ? 1.0 / v : omega / (fshift + v);
    }
    d->sor.h_state = HipObjState(A); d->sor.h_omega = omega; d->sor.h_fshift = fshift; d->sor.h_have = PETSC_TRUE;
    d->sor.idiag_builds++;
  }
  ierr = VecGetArrayRead(bb, &b);CHKERRQ(ierr);
  ierr = VecGetArray(xx, &x);CHKERRQ(ierr);
  sor_host_sweeps(a, pos, d->sor.h_idiag, d->sor.h_mdiag, omega, flag, its, b, d->sor.h_t, x);
  ierr = VecRestoreArrayRead(bb, &b);CHKERRQ(ierr);
  ierr = VecRestoreArray(xx, &x);CHKERRQ(ierr);
  ierr = VecHIPFlushBorrowed(xx);CHKERRQ(ierr);              /* a block-Jacobi block's slice of the parallel vector */
  return 0;
}
static PetscErrorCode MatSOR_SeqAIJHIP(Mat A, Vec bb, PetscReal omega, MatSORType flag_, PetscReal fshift, PetscInt its, PetscInt lits, Vec xx) {
  PetscErrorCode ierr;
  HipAIJ *a; Mat_SeqAIJHIP *d = SD(A);
  const int flag = (int)flag_;
  int route;
  ierr = value_op_view(A);CHKERRQ(ierr);
  a = SA(A);
  CHK_ASSEMBLED(A);
  if (a->bs > 1) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "MatSOR on a block matrix");
  if (flag & SOR_EISENSTAT) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "No support yet for Eisenstat");
  if (flag & (SOR_APPLY_UPPER | SOR_APPLY_LOWER)) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "SOR_APPLY_UPPER or SOR_APPLY_LOWER is not implemented");
  if (a->m != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "MatSOR on a matrix that is not square: %d x %d", a->m, a->n);
  if (its <= 0 || lits <= 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "Relaxation requires global its %d and local its %d both positive", its, lits);
  if (bb == xx) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_IDN, "b and x vector cannot be the same");
  its *= lits;
  ierr = route_resolve(A, HROUTE_SOR, &route);CHKERRQ(ierr);
  if (route != 2) {
    PetscDeviceCtx *dc;
    const PetscScalar *db; PetscScalar *dx;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);               /* the device values current, as before a product */
    if (!d->cprow) {
      const PetscBool rebuilt = (PetscBool)(!d->sor.plan || d->sor.plan_gen != d->pattern_gen);
      if (rebuilt || !d->sor.have || d->sor.idiag_state != d->uploaded_state || d->sor.omega != omega || d->sor.fshift != fshift) {
        const PetscInt *pos;
        ierr = sor_diag_check(A, omega, fshift, &pos);CHKERRQ(ierr);
        if (rebuilt) {
          const size_t bytes = sizeof(PetscScalar) * (size_t)PetscMax(a->m, 1);
          int bad = -1, rc;
          if (d->sor.plan) mi355x_sor_plan_destroy(d->sor.plan);
          d->sor.plan = NULL; d->sor.have = PETSC_FALSE;
          rc = mi355x_sor_plan_create(dc->h, (int)a->m, a->i, a->j, 0, &d->sor.plan, &bad);
          if (rc && bad >= 0) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "MatSOR: the columns of row %d are not sorted and distinct", bad);
          CHKHIP(rc);
          d->sor.plan_gen = d->pattern_gen; d->sor.plan_builds++;
          if (!d->sor.d_t) {
            CHKHIP(mi355x_malloc((void **)&d->sor.d_t, bytes));
            CHKHIP(mi355x_malloc((void **)&d->sor.d_idiag, bytes));
            CHKHIP(mi355x_malloc((void **)&d->sor.d_mdiag, bytes));
          }
        }
        CHKHIP(mi355x_sor_idiag(dc->h, d->sor.plan, d->mat.a, omega, fshift, d->sor.d_idiag, d->sor.d_mdiag));
        d->sor.idiag_state = d->uploaded_state; d->sor.omega = omega; d->sor.fshift = fshift; d->sor.have = PETSC_TRUE;
        d->sor.idiag_builds++;
      }
      ierr = VecHIPGetRead(bb, &db);CHKERRQ(ierr);
      if ((flag & SOR_ZERO_INITIAL_GUESS) && (flag & (SOR_FWD_BITS | SOR_BWD_BITS))) { ierr = VecHIPGetWrite(xx, &dx);CHKERRQ(ierr); }   /* every entry is written before it is read */
      else { ierr = VecHIPGetReadWrite(xx, &dx);CHKERRQ(ierr); }
      CHKHIP(mi355x_sor_apply(dc->h, d->sor.plan, d->mat.i, d->mat.j, d->mat.a, d->sor.d_idiag, d->sor.d_mdiag, omega,
                              flag & (SOR_FWD_BITS | SOR_BWD_BITS | SOR_ZERO_INITIAL_GUESS), (int)its, db, d->sor.d_t, dx));
      ierr = VecHIPRestoreWrite(xx);CHKERRQ(ierr);
      d->sor.device_applications++;
      return PetscLogFlops(2.0 * (PetscLogDouble)a->nz * (PetscLogDouble)its);
    }
  }
  ierr = sor_on_host(A, bb, omega, flag, fshift, its, xx);CHKERRQ(ierr);
  return PetscLogFlops(2.0 * (PetscLogDouble)a->nz * (PetscLogDouble)its);
}
PetscErrorCode MatHIPMI355XGetSORInfo(Mat A, PetscInt *levels, PetscInt *launches_per_sweep, PetscInt *idiag_builds, PetscInt *plan_builds, PetscInt *device_applications) {
  { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }
  int nlev = 0, launches = 0;
  if (SD(A)->sor.plan) CHKHIP(mi355x_sor_plan_info(SD(A)->sor.plan, &nlev, &launches, NULL));
  if (levels) *levels = nlev;
  if (launches_per_sweep) *launches_per_sweep = launches;
  if (idiag_builds) *idiag_builds = SD(A)->sor.idiag_builds;
  if (plan_builds) *plan_builds = SD(A)->sor.plan_builds;
  if (device_applications) *device_applications = SD(A)->sor.device_applications;
  return 0;
}

/* ---------------------------------------------------------------- Sparse matrix products: MatMatMult, MatTranspose, MatPtAP
 * C = A B (MatMatMult_SeqAIJ_SeqAIJ), B = A^T (MatTranspose_SeqAIJ) and C = P^T A P = MatMatMult(MatTranspose(P), MatMatMult(A, P)) for
 * sequential AIJ matrices of this type, on the model of the device ILU(0): the host does the symbolic work once (MAT_INITIAL_MATRIX:
 * the pattern of the result, its upload, the kernel plan), the device reproduces the sequential loop's arithmetic bit for bit
 * (csrc/spgemm.hip; the transpose's values are the a = d_a[perm] gather of the derived forms), and MAT_REUSE_MATRIX on unchanged patterns
 * launches kernels only.  The operands' device values follow the ordinary upload rule -- an operand changed on the device by MatScale,
 * MatShift, MatAXPY is not sent again.  The result's host values are brought back with one copy, its device copy is stamped current and
 * its derived forms go stale through device_values_changed like after every other device-side value change.
 * -mat_hipmi355x_product (the route table; A's, read at the symbolic phase and kept with the result): the host route is the sequential
 * loop over host threads followed by the ordinary upload at the result's next use.
 * A product ends in the result's own state bump (the reference's numeric phases end in MatAssemblyEnd). */
static void product_free(Mat C) {
  Mat_SeqAIJHIP *d = SD(C);
  HipMatProduct *p = d ? d->prod : NULL;
  if (!p) return;
  if (p->plan) mi355x_spgemm_plan_destroy(p->plan);
  HipFree(p->perm_h);
  if (p->perm_d) mi355x_free(p->perm_d);
  (void)MatDestroy(&p->Pt); (void)MatDestroy(&p->AP);
  HipFree(p); d->prod = NULL;
}
/* operands of a product: assembled sequential AIJ matrices of this type (BAIJ has the constructor in common) */
static PetscErrorCode product_operand(Mat X) {
  PetscErrorCode ierr;
  if (!is_seq_hip(X)) SETERRQ(HipObjComm(X), PETSC_ERR_SUP, "Matrix products of Mat type %s", HipObjTypeName(X));
  ierr = value_op_view(X);CHKERRQ(ierr);
  if (SA(X)->bs > 1) SETERRQ(HipObjComm(X), PETSC_ERR_SUP, "Matrix products of block matrices (%s)", HipObjTypeName(X));
  CHK_ASSEMBLED(X);
  return 0;
}
/* the device copies of the operands current; compressed rows (an off-diagonal block's form) are not the CSR the kernel reads: host route */
static PetscErrorCode product_operands_up(Mat X, Mat Y, int *route) {
  PetscErrorCode ierr;
  if (*route != 1) return 0;
  ierr = MatSeqAIJHIPUpload(X);CHKERRQ(ierr);
  if (Y) { ierr = MatSeqAIJHIPUpload(Y);CHKERRQ(ierr); }
  if (SD(X)->cprow || (Y && SD(Y)->cprow)) *route = 2;
  return 0;
}
static void product_note(HipMatProduct *p, int k, Mat X) { p->op[k] = X; p->op_nz[k] = SA(X)->nz; p->op_gen[k] = SD(X)->pattern_gen; }
static PetscBool product_noted(const HipMatProduct *p, int k, Mat X) {
  return (PetscBool)(p->op[k] == (void *)X && p->op_nz[k] == SA(X)->nz && (!p->op_gen[k] || p->op_gen[k] == SD(X)->pattern_gen));
}
/* MAT_REUSE_MATRIX: C came from this operation on these operands, and no pattern was uploaded anew since */
static PetscErrorCode product_reuse_check(Mat C, int kind, Mat X, Mat Y, HipMatProduct **p_) {
  PetscErrorCode ierr;
  HipMatProduct *p;
  if (!is_seq_hip(C) || !SD(C)->prod || SD(C)->prod->kind != kind)
    SETERRQ(HipObjComm(X), PETSC_ERR_ARG_WRONG, "MAT_REUSE_MATRIX: the matrix is not the result of this operation");
  p = SD(C)->prod;
  { int route = p->route; ierr = product_operands_up(X, Y, &route);CHKERRQ(ierr);
    if (route != p->route) SETERRQ(HipObjComm(X), PETSC_ERR_ARG_WRONG, "MAT_REUSE_MATRIX: an operand changed its device form since the symbolic phase"); }
  if (!product_noted(p, 0, X) || (Y && !product_noted(p, 1, Y)))
    SETERRQ(HipObjComm(X), PETSC_ERR_ARG_WRONG, "MAT_REUSE_MATRIX: not the operands, or not the operand patterns, of the symbolic phase");
  *p_ = p;
  return 0;
}
/* the result as a matrix of the operands' type with the given pattern and zero values; the type's options go along (as MatDuplicate), and
 * of the routes those the table marks inherited -- as they stand in A: asked under its prefix, or kept from its first use */
static PetscErrorCode product_result(Mat A, PetscInt m, PetscInt n, const PetscInt *ci, const PetscInt *cj, int kind, int route, Mat *C_, HipMatProduct **p_) {
  PetscErrorCode ierr;
  Mat C; HipMatProduct *p; PetscScalar *ca;
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(ci[m], 1), &ca);CHKERRQ(ierr);
  memset(ca, 0, sizeof(PetscScalar) * (size_t)PetscMax(ci[m], 1));
  ierr = MatCreate(HipObjComm(A), &C);CHKERRQ(ierr);
  ierr = MatSetSizes(C, m, n, m, n);CHKERRQ(ierr);
  ierr = MatSetType(C, MATSEQAIJHIPMI355X);CHKERRQ(ierr);
  ierr = MatSeqAIJSetPreallocationCSR(C, ci, cj, ca);CHKERRQ(ierr);
  HipFree(ca);
  ierr = value_op_view(C);CHKERRQ(ierr);
  memcpy(SD(C)->opt, SD(A)->opt, sizeof(SD(A)->opt)); memcpy(SD(C)->opt_set, SD(A)->opt_set, sizeof(SD(A)->opt_set));
  for (int k = 0; k < HROUTE_N; k++) if (hroute[k].inherited) SD(C)->route[k] = SD(A)->route[k];
  ierr = PetscMalloc(sizeof(*p), &p);CHKERRQ(ierr);
  memset(p, 0, sizeof(*p));
  p->kind = kind; p->route = route; p->symbolic_builds = 1;
  SD(C)->prod = p;
  if (route == 1) { ierr = MatSeqAIJHIPUpload(C);CHKERRQ(ierr); }   /* the one pattern upload */
  *C_ = C; *p_ = p;
  return 0;
}
/* after the device numeric phase: the host copy by one device-to-host copy; both routes: the result's state */
static PetscErrorCode product_values_back(Mat C, PetscDeviceCtx *dc) {
  const size_t bytes = sizeof(PetscScalar) * (size_t)SA(C)->nz;
  if (bytes) CHKHIP(mi355x_memcpy_d2h(dc->h, SA(C)->a, SD(C)->mat.a, bytes));
  CHKHIP(mi355x_handle_synchronize(dc->h));
  return 0;
}

/* C = A B.  The host route's loop: MatMatMultNumeric_SeqAIJ_SeqAIJ's, a row of C at a time, both column lists ascending */
typedef struct { const HipAIJ *a, *b, *c; } ProdHost;
static void product_host_rows(void *c_, PetscInt lo, PetscInt hi) {
  const ProdHost *h = (const ProdHost *)c_;
  const HipAIJ *a = h->a, *b = h->b, *c = h->c;
  for (PetscInt i = lo; i < hi; i++) {
    const PetscInt *cc = c->j + c->i[i]; PetscScalar *cr = c->a + c->i[i];
    for (PetscInt p = 0; p < c->i[i + 1] - c->i[i]; p++) cr[p] = 0.0;
    for (PetscInt t = a->i[i]; t < a->i[i + 1]; t++) {
      const PetscScalar av = a->a[t]; const PetscInt r = a->j[t];
      PetscInt p = 0;
      for (PetscInt q = b->i[r]; q < b->i[r + 1]; q++) {
        while (cc[p] != b->j[q]) p++;
        cr[p] = cr[p] + av * b->a[q];
        p++;
      }
    }
  }
}
static PetscErrorCode matmult_symbolic(Mat A, Mat B, int route, Mat *C_) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A), *b = SA(B);
  const PetscInt m = a->m, n = b->n;
  PetscInt *ci, *cj; HipMatProduct *p;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(m + 1), &ci);CHKERRQ(ierr);
  CHKHIP(mi355x_spgemm_symbolic_host((int)m, (int)n, a->i, a->j, b->i, b->j, ci, NULL, 0));
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(ci[m], 1), &cj);CHKERRQ(ierr);
  CHKHIP(mi355x_spgemm_symbolic_host((int)m, (int)n, a->i, a->j, b->i, b->j, ci, cj, 0));
  ierr = product_result(A, m, n, ci, cj, 1, route, C_, &p);CHKERRQ(ierr);
  product_note(p, 0, A); product_note(p, 1, B);
  if (route == 1) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    CHKHIP(mi355x_spgemm_plan_create(dc->h, (int)m, (int)a->n, (int)n, a->i, a->j, b->i, b->j, ci, cj, &p->plan));
  }
  HipFree(ci); HipFree(cj);
  return 0;
}
static PetscErrorCode matmult_numeric(Mat A, Mat B, Mat C) {
  PetscErrorCode ierr;
  HipMatProduct *p = SD(C)->prod;
  if (SA(C)->nz != SA(C)->i[SA(C)->m] || !SA(C)->compact) SETERRQ(HipObjComm(C), PETSC_ERR_ARG_WRONGSTATE, "the product's pattern was changed");
  if (p->route == 1) {
    PetscDeviceCtx *dc;
    Mat_SeqAIJHIP *da = SD(A), *db = SD(B), *dd = SD(C);
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    ierr = MatSeqAIJHIPUpload(C);CHKERRQ(ierr);                   /* (its arrays exist; nothing moves unless someone changed C) */
    ierr = device_values_changed(C);CHKERRQ(ierr);
    CHKHIP(mi355x_spgemm_numeric(dc->h, p->plan, da->mat.i, da->mat.j, da->mat.a, db->mat.i, db->mat.j, db->mat.a, dd->mat.i, dd->mat.j, dd->mat.a));
    ierr = product_values_back(C, dc);CHKERRQ(ierr);
    p->device_numerics++;
  } else {
    ProdHost h = {SA(A), SA(B), SA(C)};
    HipParallelRanges(SA(A)->m, product_host_rows, &h);
    p->host_numerics++;
  }
  HipStateIncrease(C);
  return 0;
}
/* B = A^T: the stable counting sort behind the cached transpose (transpose_pattern), the values by the gather through its permutation */
typedef struct { const PetscInt *perm; const PetscScalar *src; PetscScalar *dst; } GatherHost;
static void product_gather_host(void *c_, PetscInt lo, PetscInt hi) { const GatherHost *g = (const GatherHost *)c_; for (PetscInt k = lo; k < hi; k++) g->dst[k] = g->src[g->perm[k]]; }
static PetscErrorCode transpose_symbolic(Mat A, int route, Mat *B_) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  PetscInt *ti, *tj, *tperm; HipMatProduct *p;
  ierr = transpose_pattern(a->m, a->n, a->i, a->j, 1, NULL, &ti, &tj, &tperm);CHKERRQ(ierr);
  ierr = product_result(A, a->n, a->m, ti, tj, 2, route, B_, &p);CHKERRQ(ierr);
  product_note(p, 0, A);
  p->perm_h = tperm;
  if (route == 1) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    CHKHIP(mi355x_malloc((void **)&p->perm_d, sizeof(PetscInt) * (size_t)PetscMax(a->nz, 1)));
    CHKHIP(mi355x_memcpy_h2d(dc->h, p->perm_d, tperm, sizeof(PetscInt) * (size_t)a->nz));
    CHKHIP(mi355x_handle_synchronize(dc->h));
  }
  HipFree(ti); HipFree(tj);
  return 0;
}
static PetscErrorCode transpose_numeric(Mat A, Mat B) {
  PetscErrorCode ierr;
  HipMatProduct *p = SD(B)->prod;
  if (SA(B)->nz != SA(A)->nz || !SA(B)->compact) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_WRONGSTATE, "the transpose's pattern was changed");
  if (p->route == 1) {
    PetscDeviceCtx *dc;
    ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
    ierr = MatSeqAIJHIPUpload(B);CHKERRQ(ierr);
    ierr = device_values_changed(B);CHKERRQ(ierr);
    if (SA(A)->nz) CHKHIP(mi355x_pack(dc->h, (size_t)SA(A)->nz, p->perm_d, SD(A)->mat.a, SD(B)->mat.a));
    ierr = product_values_back(B, dc);CHKERRQ(ierr);
    p->device_numerics++;
  } else {
    GatherHost g = {p->perm_h, SA(A)->a, SA(B)->a};
    HipParallelRanges(SA(A)->nz, product_gather_host, &g);
    p->host_numerics++;
  }
  HipStateIncrease(B);
  return 0;
}

static PetscErrorCode MatMatMultSymbolic_SeqAIJHIP(Mat A, Mat B, PetscReal fill, Mat *C) {
  PetscErrorCode ierr;
  int route;
  (void)fill;
  ierr = product_operand(A);CHKERRQ(ierr);
  ierr = product_operand(B);CHKERRQ(ierr);
  if (SA(A)->n != SA(B)->m) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Matrix dimensions are incompatible, %d != %d", SA(A)->n, SA(B)->m);
  ierr = route_resolve(A, HROUTE_PRODUCT, &route);CHKERRQ(ierr);
  ierr = product_operands_up(A, B, &route);CHKERRQ(ierr);
  ierr = matmult_symbolic(A, B, route, C);CHKERRQ(ierr);      /* (the new matrix's first state is its constructor's: the device copy just made stays current) */
  return 0;
}
static PetscErrorCode MatMatMultNumeric_SeqAIJHIP(Mat A, Mat B, Mat C) {
  PetscErrorCode ierr;
  HipMatProduct *p;
  ierr = product_operand(A);CHKERRQ(ierr);
  ierr = product_operand(B);CHKERRQ(ierr);
  ierr = product_reuse_check(C, 1, A, B, &p);CHKERRQ(ierr);
  return matmult_numeric(A, B, C);
}
static PetscErrorCode MatMatMult_SeqAIJHIP(Mat A, Mat B, MatReuse scall, PetscReal fill, Mat *C) {
  PetscErrorCode ierr;
  if (scall == MAT_INITIAL_MATRIX) { ierr = MatMatMultSymbolic_SeqAIJHIP(A, B, fill, C);CHKERRQ(ierr); }
  return MatMatMultNumeric_SeqAIJHIP(A, B, *C);
}
static PetscErrorCode MatTranspose_SeqAIJHIP(Mat A, MatReuse reuse, Mat *B) {
  PetscErrorCode ierr;
  HipMatProduct *p;
  ierr = product_operand(A);CHKERRQ(ierr);
  if (reuse == MAT_INITIAL_MATRIX || !*B) {
    int route;
    ierr = route_resolve(A, HROUTE_PRODUCT, &route);CHKERRQ(ierr);
    ierr = product_operands_up(A, NULL, &route);CHKERRQ(ierr);
    ierr = transpose_symbolic(A, route, B);CHKERRQ(ierr);
  }
  ierr = product_reuse_check(*B, 2, A, NULL, &p);CHKERRQ(ierr);
  return transpose_numeric(A, *B);
}
static PetscErrorCode MatPtAP_SeqAIJHIP(Mat A, Mat P, MatReuse scall, PetscReal fill, Mat *C) {
  PetscErrorCode ierr;
  HipMatProduct *p;
  (void)fill;
  ierr = product_operand(A);CHKERRQ(ierr);
  ierr = product_operand(P);CHKERRQ(ierr);
  if (SA(A)->m != SA(A)->n || SA(A)->n != SA(P)->m) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Matrix dimensions are incompatible, A %d x %d, P %d x %d", SA(A)->m, SA(A)->n, SA(P)->m, SA(P)->n);
  if (scall == MAT_INITIAL_MATRIX) {
    int route;
    Mat Pt = NULL, AP = NULL;
    ierr = route_resolve(A, HROUTE_PRODUCT, &route);CHKERRQ(ierr);
    ierr = product_operands_up(A, P, &route);CHKERRQ(ierr);
    ierr = transpose_symbolic(P, route, &Pt);CHKERRQ(ierr);
    ierr = transpose_numeric(P, Pt);CHKERRQ(ierr);             /* (the symbolic phase of Pt (A P) reads patterns only; the inner results are complete matrices all the same) */
    ierr = matmult_symbolic(A, P, route, &AP);CHKERRQ(ierr);
    ierr = matmult_numeric(A, P, AP);CHKERRQ(ierr);
    ierr = matmult_symbolic(Pt, AP, route, C);CHKERRQ(ierr);
    p = SD(*C)->prod;
    p->kind = 3; p->Pt = Pt; p->AP = AP;
    product_note(p, 0, A); product_note(p, 1, P);
    p->device_numerics = p->host_numerics = 0;
  } else {
    HipMatProduct *q;
    ierr = product_reuse_check(*C, 3, A, P, &p);CHKERRQ(ierr);
    ierr = product_reuse_check(p->Pt, 2, P, NULL, &q);CHKERRQ(ierr);
    ierr = product_reuse_check(p->AP, 1, A, P, &q);CHKERRQ(ierr);
    ierr = transpose_numeric(P, p->Pt);CHKERRQ(ierr);
    ierr = matmult_numeric(A, P, p->AP);CHKERRQ(ierr);
  }
  return matmult_numeric(p->Pt, p->AP, *C);
}
PetscErrorCode MatHIPMI355XGetProductCounts(Mat C, PetscInt *symbolic_builds, PetscInt *device_numerics, PetscInt *host_numerics) {
  if (!is_seq_hip(C) || !SD(C)->prod) SETERRQ(C ? HipObjComm(C) : 0, PETSC_ERR_ARG_WRONG, "not the result of MatMatMult, MatTranspose or MatPtAP");
  if (symbolic_builds) *symbolic_builds = SD(C)->prod->symbolic_builds;
  if (device_numerics) *device_numerics = SD(C)->prod->device_numerics;
  if (host_numerics) *host_numerics = SD(C)->prod->host_numerics;
  return 0;
}

/* ---------------------------------------------------------------- Norms and row / column reductions
 * MatNorm (MatNorm_SeqAIJ aij.c, MatNorm_SeqBAIJ baij.c), MatGetRowMaxAbs / MatGetRowMax / MatGetRowMin (aij.c), MatGetColumnNorms
 * (MatGetColumnNorms_SeqAIJ aij.c) of the two sequential types.  A point row's entries are taken in storage order (BAIJ: block after
 * block, a block's columns left to right), one at a time:
 *   NORM_INFINITY   the row sums of |a|, then their maximum as VecMax takes it (0.0 for a matrix without rows)
 *   NORM_1          the same over the columns; a column's entries are added in ascending row order.  On the device the rows of the cached
 *                   transpose -- the one MatMultTranspose builds and refreshes -- whose rows list their entries in exactly that order
 *   NORM_FROBENIUS  the root of the sum of squares of the stored value array: on the device VecNorm's tree over that array (the bits of
 *                   mi355x_vec_norm), on the host the sequential sum; the two differ by at most (nnz - 1) 2^-53 sum a^2 before the root
 *   NORM_2          PETSC_ERR_SUP, as in the reference
 *   row max-abs     starts at (0.0, column 0), replaced on cur < |a| only
 *   row max / min   a row with fewer stored entries than the matrix has columns starts at the implicit (0.0, its smallest missing
 *                   column), a full row at its first entry, a row without entries gives (0.0, 0); replaced on cur < a (a < cur) only
 *   column norms    NORM_1 / NORM_2 / NORM_INFINITY: the sums of |a|, the roots of the sums of a * a, the max-abs of the columns
 * -mat_hipmi355x_reductions (the route table): the device route runs the row
 * reductions of csrc/mat_reduce.hip over the plain device value array -- the one every device-side value update writes, current after
 * MatSeqAIJHIPUpload whatever form the products take -- and its transposed form; the host route is the loops below over the host
 * copy.  Except for NORM_FROBENIUS the two give the same bits. */
/* entry j of point row I bs + r (block row I starts at block a0) and its scalar column */
#define RED_VALUE(m_, bs_, a0_, r_, e_) ((m_)->a[(size_t)(a0_) * (size_t)((bs_) * (bs_)) + (size_t)(e_) * (size_t)(bs_) + (size_t)(r_)])
#define RED_COLUMN(m_, bs_, a0_, e_) ((m_)->j[(a0_) + (e_) / (bs_)] * (bs_) + (e_) % (bs_))
static PetscScalar red_term(int op, PetscScalar v) { return (op == MI355X_ROW_ABSSUM || op == MI355X_ROW_MAXABS) ? fabs(v) : (op == MI355X_ROW_SQSUM ? v * v : v); }
/* the host route of mi355x_mat_row_reduce: out[i] (and idx[i], extrema only, may be NULL) for every point row of a matrix of ncols
 * columns; add: a sum continues from out[i] */
static void host_row_reduce(const HipAIJ *a, int op, PetscInt ncols, PetscBool add, PetscScalar *out, PetscInt *idx) {
  const PetscInt bs = a->bs > 1 ? a->bs : 1;
  for (PetscInt I = 0; I < a->m; I++) for (PetscInt r = 0; r < bs; r++) {
    const PetscInt a0 = a->i[I], n = (a->i[I + 1] - a0) * bs, row = I * bs + r;
    PetscScalar cur = (add && op <= MI355X_ROW_SQSUM) ? out[row] : 0.0; PetscInt best = -1;
    if (op <= MI355X_ROW_SQSUM) { for (PetscInt j = 0; j < n; j++) cur = cur + red_term(op, RED_VALUE(a, bs, a0, r, j)); }
    else {
      const PetscBool full = (PetscBool)(n > 0 && n == ncols);
      for (PetscInt j = 0; j < n; j++) {
        const PetscScalar v = red_term(op, RED_VALUE(a, bs, a0, r, j));
        if ((op != MI355X_ROW_MAXABS && j == 0 && full) || (op == MI355X_ROW_MIN ? v < cur : cur < v)) { cur = v; best = j; }
      }
    }
    out[row] = cur;
    if (idx && op > MI355X_ROW_SQSUM) {
      PetscInt col = 0;
      if (best >= 0) col = RED_COLUMN(a, bs, a0, best);
      else if (op != MI355X_ROW_MAXABS && n > 0) { while (col < n && RED_COLUMN(a, bs, a0, col) == col) col++; }
      idx[row] = col;
    }
  }
}
/* the same per column (op: MI355X_ROW_ABSSUM, _SQSUM or _MAXABS), a column's entries taken in ascending row order */
static void host_col_reduce(const HipAIJ *a, int op, PetscScalar *out) {
  const PetscInt bs = a->bs > 1 ? a->bs : 1;
  for (PetscInt c = 0; c < a->n; c++) out[c] = 0.0;
  for (PetscInt I = 0; I < a->m; I++) for (PetscInt r = 0; r < bs; r++) {
    const PetscInt a0 = a->i[I], n = (a->i[I + 1] - a0) * bs;
    for (PetscInt j = 0; j < n; j++) {
      const PetscScalar v = red_term(op, RED_VALUE(a, bs, a0, r, j));
      const PetscInt c = RED_COLUMN(a, bs, a0, j);
      if (op == MI355X_ROW_MAXABS) { if (out[c] < v) out[c] = v; }
      else out[c] = out[c] + v;
    }
  }
}
/* VecMax_Seq's loop (dvec2.c): what mi355x_vec_max gives; 0.0 for no elements */
static PetscReal host_max_of(const PetscScalar *x, PetscInt n) {
  if (n <= 0) return 0.0;
  PetscReal m = x[0];
  for (PetscInt k = 1; k < n; k++) if (x[k] > m) m = x[k];
  return m;
}
static PetscErrorCode device_max_of(PetscDeviceCtx *dc, const PetscScalar *x, PetscInt n, PetscReal *val) {
  *val = 0.0;
  if (n <= 0) return 0;
  CHKHIP(mi355x_vec_max(dc->h, (size_t)n, x, mi355x_handle_host_scratch(dc->h)));
  CHKHIP(mi355x_handle_wait_result(dc->h)); { PetscErrorCode e_ = HipTriWatchCheck();CHKERRQ(e_); }
  *val = mi355x_handle_host_scratch(dc->h)[0];
  return 0;
}
static PetscErrorCode red_work_get(Mat A, size_t bytes, void **w) {
  Mat_SeqAIJHIP *d = SD(A);
  if (d->red_cap < bytes || !d->red_work) {
    if (d->red_work) mi355x_free(d->red_work);
    d->red_work = NULL; d->red_cap = 0;
    CHKHIP(mi355x_malloc(&d->red_work, PetscMax(bytes, 16)));
    d->red_cap = PetscMax(bytes, 16);
  }
  *w = d->red_work;
  return 0;
}
/* the device copy current, for the device route; the compressed-row form of an MPIAIJ matrix's off-diagonal block is not a matrix a
 * user holds, and its rows are not the matrix's */
static PetscErrorCode red_device_copy(Mat A, PetscDeviceCtx **dc) {
  PetscErrorCode ierr;
  CHK_ASSEMBLED(A);
  ierr = PetscDeviceGet(dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (SD(A)->cprow) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "reductions over a compressed-row device copy");
  return 0;
}
/* out_dev[c] for every column c through the rows of the transposed form (the blocked companion's block transpose when there is one) */
static PetscErrorCode device_col_reduce(Mat A, PetscDeviceCtx *dc, int op, PetscScalar *out_dev) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); HipDevForm *f = NULL;
  const PetscInt bs = a->bs > 1 ? a->bs : 1;
  ierr = product_form(A, PETSC_TRUE, dc, &f);CHKERRQ(ierr);
  CHKHIP(mi355x_mat_row_reduce(dc->h, op, (int)(a->n / f->bs), (int)f->bs, (int)(a->m * bs), f->i, f->j, f->a, NULL, NULL, out_dev, NULL));
  return 0;
}
static PetscErrorCode MatNorm_SeqAIJHIP(Mat A, NormType type, PetscReal *nrm) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscInt bs = a->bs > 1 ? a->bs : 1, mrows = a->m * bs;
  const size_t nvals = value_count(a);
  int route;
  if (type == NORM_2) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "No support for two norm");
  if (type != NORM_1 && type != NORM_FROBENIUS && type != NORM_INFINITY) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Unknown NormType %d", (int)type);
  CHK_ASSEMBLED(A);
  ierr = route_resolve(A, HROUTE_REDUCTIONS, &route);CHKERRQ(ierr);
  if (route == 2) {
    if (type == NORM_FROBENIUS) {
      PetscReal s = 0.0;
      for (size_t k = 0; k < nvals; k++) s = s + a->a[k] * a->a[k];
      *nrm = sqrt(s);
    } else {
      const PetscInt len = type == NORM_1 ? a->n : mrows;
      PetscScalar *w;
      ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(len, 1), &w);CHKERRQ(ierr);
      if (type == NORM_1) host_col_reduce(a, MI355X_ROW_ABSSUM, w); else host_row_reduce(a, MI355X_ROW_ABSSUM, a->n, PETSC_FALSE, w, NULL);
      *nrm = host_max_of(w, len);
      HipFree(w);
    }
  } else {
    PetscDeviceCtx *dc; void *w;
    ierr = red_device_copy(A, &dc);CHKERRQ(ierr);
    if (type == NORM_FROBENIUS) {
      *nrm = 0.0;
      if (nvals) {
        CHKHIP(mi355x_vec_norm(dc->h, nvals, 2, d->mat.a, mi355x_handle_host_scratch(dc->h)));
        CHKHIP(mi355x_handle_wait_result(dc->h)); { PetscErrorCode e_ = HipTriWatchCheck();CHKERRQ(e_); }
        *nrm = sqrt(mi355x_handle_host_scratch(dc->h)[0]);
      }
    } else if (type == NORM_1) {
      ierr = red_work_get(A, sizeof(PetscScalar) * (size_t)a->n, &w);CHKERRQ(ierr);
      ierr = device_col_reduce(A, dc, MI355X_ROW_ABSSUM, (PetscScalar *)w);CHKERRQ(ierr);
      ierr = device_max_of(dc, (const PetscScalar *)w, a->n, nrm);CHKERRQ(ierr);
    } else {
      ierr = red_work_get(A, sizeof(PetscScalar) * (size_t)mrows, &w);CHKERRQ(ierr);
      CHKHIP(mi355x_mat_row_reduce(dc->h, MI355X_ROW_ABSSUM, (int)a->m, (int)bs, (int)a->n, d->mat.i, d->mat.j, d->mat.a, NULL, NULL, (PetscScalar *)w, NULL));
      ierr = device_max_of(dc, (const PetscScalar *)w, mrows, nrm);CHKERRQ(ierr);
    }
  }
  return PetscLogFlops(type == NORM_FROBENIUS ? 2.0 * (double)nvals : (double)nvals);
}
static PetscErrorCode row_extremum(Mat A, int op, Vec v, PetscInt idx[]) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  const PetscInt bs = a->bs > 1 ? a->bs : 1, mrows = a->m * bs;
  int route;
  if (!vec_on_device(v)) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "the result must be a HIPMI355X vector");
  if (v->map->n != A->rmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Nonconforming matrix and vector");
  CHK_ASSEMBLED(A);
  ierr = route_resolve(A, HROUTE_REDUCTIONS, &route);CHKERRQ(ierr);
  if (route == 2) {
    PetscScalar *h;
    ierr = VecGetArray(v, &h);CHKERRQ(ierr);
    host_row_reduce(a, op, a->n, PETSC_FALSE, h, idx);
    return VecRestoreArray(v, &h);
  }
  PetscDeviceCtx *dc; PetscScalar *dv; void *w = NULL;
  ierr = red_device_copy(A, &dc);CHKERRQ(ierr);
  if (idx) { ierr = red_work_get(A, sizeof(PetscInt) * (size_t)mrows, &w);CHKERRQ(ierr); }
  ierr = VecHIPGetWrite(v, &dv);CHKERRQ(ierr);
  CHKHIP(mi355x_mat_row_reduce(dc->h, op, (int)a->m, (int)bs, (int)a->n, d->mat.i, d->mat.j, d->mat.a, NULL, NULL, dv, (int *)w));
  ierr = VecHIPRestoreWrite(v);CHKERRQ(ierr);
  if (idx && mrows > 0) {
    CHKHIP(mi355x_memcpy_d2h(dc->h, idx, w, sizeof(PetscInt) * (size_t)mrows));
    CHKHIP(mi355x_handle_synchronize(dc->h));
  }
  return 0;
}
static PetscErrorCode MatGetRowMaxAbs_SeqAIJHIP(Mat A, Vec v, PetscInt idx[]) { return row_extremum(A, MI355X_ROW_MAXABS, v, idx); }
static PetscErrorCode MatGetRowMax_SeqAIJHIP(Mat A, Vec v, PetscInt idx[]) { return row_extremum(A, MI355X_ROW_MAX, v, idx); }
static PetscErrorCode MatGetRowMin_SeqAIJHIP(Mat A, Vec v, PetscInt idx[]) { return row_extremum(A, MI355X_ROW_MIN, v, idx); }
static PetscErrorCode MatGetColumnNorms_SeqAIJHIP(Mat A, NormType type, PetscReal *norms) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  int route;
  const int op = type == NORM_1 ? MI355X_ROW_ABSSUM : (type == NORM_2 ? MI355X_ROW_SQSUM : MI355X_ROW_MAXABS);
  if (type != NORM_1 && type != NORM_2 && type != NORM_INFINITY) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONG, "Unknown NormType %d", (int)type);
  CHK_ASSEMBLED(A);
  ierr = route_resolve(A, HROUTE_REDUCTIONS, &route);CHKERRQ(ierr);
  if (route == 2) host_col_reduce(a, op, norms);
  else if (a->n > 0) {
    PetscDeviceCtx *dc; void *w;
    ierr = red_device_copy(A, &dc);CHKERRQ(ierr);
    ierr = red_work_get(A, sizeof(PetscScalar) * (size_t)a->n, &w);CHKERRQ(ierr);
    ierr = device_col_reduce(A, dc, op, (PetscScalar *)w);CHKERRQ(ierr);
    CHKHIP(mi355x_memcpy_d2h(dc->h, norms, w, sizeof(PetscScalar) * (size_t)a->n));
    CHKHIP(mi355x_handle_synchronize(dc->h));
  }
  if (type == NORM_2) for (PetscInt c = 0; c < a->n; c++) norms[c] = sqrt(norms[c]);
  return 0;
}

/* ---------------------------------------------------------------- Coarsening ("MatCoarsenAggregate_C", what PCGAMG asks of a level operator)
 * Aggregates of a square sequential AIJ matrix: d = its diagonal, the strength mask |a_ij| > threshold sqrt(|d_i| |d_j|), and the
 * distance-2 MIS aggregation of the strong graph (csrc/coarsen.hip; include/mi355x_kernels.h states the contract).  agg[i] in
 * [0, *nagg) for every row, a host array.  -mat_hipmi355x_coarsen (the route table): the device route works on the device copy of the
 * pattern and the values, uploaded under the ordinary rule, and brings back the m numbers; the host route is the host twins over the
 * host copy.  The same integers. */
static PetscInt coarsen_total_device = 0, coarsen_total_host = 0, coarsen_total_rounds = 0;
static PetscErrorCode MatCoarsenAggregate_SeqAIJHIP(Mat A, PetscReal threshold, PetscInt *nagg, PetscInt agg[]) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  int route, n = 0, rounds = 0;
  if (strcmp(HipObjTypeName(A), MATSEQAIJHIPMI355X) || a->bs > 1) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "MatCoarsenAggregate for Mat type %s", HipObjTypeName(A));
  CHK_ASSEMBLED(A);
  if (a->m != a->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Matrix must be square, %d != %d", (int)a->m, (int)a->n);
  ierr = route_resolve(A, HROUTE_COARSEN, &route);CHKERRQ(ierr);
  *nagg = 0;
  if (route == 2) {
    PetscScalar *diag; unsigned char *strong;
    ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(a->m, 1), &diag);CHKERRQ(ierr);
    ierr = PetscMalloc((size_t)PetscMax(a->nz, 1), &strong);CHKERRQ(ierr);
    for (PetscInt r = 0; r < a->m; r++) { const PetscInt k = diag_position(a->i, a->j, r); diag[r] = k >= 0 ? a->a[k] : 0.0; }
    int rc = mi355x_csr_strength_host((int)a->m, a->i, a->j, a->a, diag, threshold, strong);
    if (!rc) rc = mi355x_coarsen_mis2_host((int)a->m, a->i, a->j, strong, agg, &n);
    HipFree(diag); HipFree(strong);
    CHKHIP(rc);
    d->coarsen_host++; coarsen_total_host++;
  } else {
    PetscDeviceCtx *dc; void *w = NULL;
    ierr = red_device_copy(A, &dc);CHKERRQ(ierr);
    if (a->m > 0) {
      /* the diagonal, the aggregate numbers, the mask: one work array */
      const size_t off_agg = sizeof(PetscScalar) * (size_t)a->m, off_strong = off_agg + ((sizeof(int) * (size_t)a->m + 7) & ~(size_t)7);
      CHKHIP(mi355x_malloc(&w, off_strong + (size_t)PetscMax(a->nz, 1)));
      int rc = mi355x_csr_get_diagonal(dc->h, (int)a->m, d->mat.i, d->mat.j, d->mat.a, (double *)w);
      if (!rc) rc = mi355x_csr_strength(dc->h, (int)a->m, d->mat.i, d->mat.j, d->mat.a, (const double *)w, threshold, (unsigned char *)w + off_strong);
      if (!rc) rc = mi355x_coarsen_mis2(dc->h, (int)a->m, d->mat.i, d->mat.j, (const unsigned char *)w + off_strong, (int *)((char *)w + off_agg), &n, &rounds);
      if (!rc) rc = mi355x_memcpy_d2h(dc->h, agg, (char *)w + off_agg, sizeof(int) * (size_t)a->m);
      if (!rc) rc = mi355x_handle_synchronize(dc->h);
      mi355x_free(w);
      CHKHIP(rc);
    }
    d->coarsen_device++; coarsen_total_device++;
    d->coarsen_rounds = coarsen_total_rounds = rounds;
  }
  *nagg = n;
  return 0;
}
PetscErrorCode MatHIPMI355XGetCoarsenCounts(Mat A, PetscInt *device, PetscInt *host, PetscInt *rounds) {
  if (A) { PetscErrorCode ierr = seq_hip_check(A, "not a sequential HIPMI355X AIJ matrix");CHKERRQ(ierr); }   /* (NULL: the totals of the process) */
  if (device) *device = A ? SD(A)->coarsen_device : coarsen_total_device;
  if (host) *host = A ? SD(A)->coarsen_host : coarsen_total_host;
  if (rounds) *rounds = A ? SD(A)->coarsen_rounds : coarsen_total_rounds;
  return 0;
}

/* The same reductions over ONE BLOCK of an MPIAIJ matrix (host/mpiaijhip.c), on the route the parent chose (1 device, 2 host).
 * Route 1: out / idx are device arrays of the block's rows; the off-diagonal block's compressed-row device copy is walked through
 * its plan's row list, and the rows it does not list keep what out / idx hold (add) or get (0.0, 0), an empty row's result.
 * Route 2: host arrays.  ncols: the columns of the matrix the block is a part of (a row is full only with that many entries). */
PetscErrorCode MatReductionsRoute_SeqAIJHIP(Mat A, int *route) { return route_resolve(A, HROUTE_REDUCTIONS, route); }
PetscErrorCode MatBlockRowReduce_SeqAIJHIP(Mat A, int route, int op, PetscInt ncols, PetscBool add, PetscScalar *out, PetscInt *idx) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A); Mat_SeqAIJHIP *d = SD(A);
  CHK_ASSEMBLED(A);
  if (a->bs > 1) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "blocks of an MPIAIJ matrix are point matrices");
  if (route == 2) { host_row_reduce(a, op, ncols, add, out, idx); return 0; }
  PetscDeviceCtx *dc; const int *rows = NULL; int nrows = (int)a->m;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  if (d->cprow) {
    CHKHIP(mi355x_spmv_plan_rows(d->mat.plan, &rows, &nrows));
    if (!add && a->m > 0) {
      CHKHIP(mi355x_memset(dc->h, out, 0, sizeof(PetscScalar) * (size_t)a->m));
      if (idx) CHKHIP(mi355x_memset(dc->h, idx, 0, sizeof(PetscInt) * (size_t)a->m));
    }
  }
  CHKHIP(mi355x_mat_row_reduce(dc->h, op, nrows, 1, (int)ncols, d->mat.i, d->mat.j, d->mat.a, rows, add ? out : NULL, out, (int *)idx));
  return 0;
}
/* per column of the block (host array of the block's columns), either route */
PetscErrorCode MatBlockColReduce_SeqAIJHIP(Mat A, int route, int op, PetscScalar *out_host) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  CHK_ASSEMBLED(A);
  if (route == 2) { host_col_reduce(a, op, out_host); return 0; }
  if (a->n <= 0) return 0;
  PetscDeviceCtx *dc; void *w;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  ierr = red_work_get(A, sizeof(PetscScalar) * (size_t)a->n, &w);CHKERRQ(ierr);
  ierr = device_col_reduce(A, dc, op, (PetscScalar *)w);CHKERRQ(ierr);
  CHKHIP(mi355x_memcpy_d2h(dc->h, out_host, w, sizeof(PetscScalar) * (size_t)a->n));
  CHKHIP(mi355x_handle_synchronize(dc->h));
  return 0;
}
/* the sum of squares of the block's stored values: VecNorm's tree over the device value array, or the sequential sum */
PetscErrorCode MatBlockSquareSum_SeqAIJHIP(Mat A, int route, PetscReal *s) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  *s = 0.0;
  CHK_ASSEMBLED(A);
  if (route == 2) { for (PetscInt k = 0; k < a->nz; k++) *s = *s + a->a[k] * a->a[k]; return 0; }
  if (a->nz <= 0) return 0;
  PetscDeviceCtx *dc;
  ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  ierr = MatSeqAIJHIPUpload(A);CHKERRQ(ierr);
  CHKHIP(mi355x_vec_norm(dc->h, (size_t)a->nz, 2, SD(A)->mat.a, mi355x_handle_host_scratch(dc->h)));
  CHKHIP(mi355x_handle_wait_result(dc->h)); { PetscErrorCode e_ = HipTriWatchCheck();CHKERRQ(e_); }
  *s = mi355x_handle_host_scratch(dc->h)[0];
  return 0;
}
PetscErrorCode HipDeviceMaxOf(const PetscScalar *x_dev, PetscInt n, PetscReal *val) {
  PetscDeviceCtx *dc;
  PetscErrorCode ierr = PetscDeviceGet(&dc);CHKERRQ(ierr);
  return device_max_of(dc, x_dev, n, val);
}

static PetscErrorCode MatGetVecs_HIP(Mat A, Vec *right, Vec *left) {   /* MatGetVecs_SeqAIJCUSP aijcusp.cu:324-345 */
  PetscErrorCode ierr;
  if (right) {
    ierr = VecCreate(HipObjComm(A), right);CHKERRQ(ierr);
    ierr = VecSetSizes(*right, A->cmap->n, A->cmap->N);CHKERRQ(ierr);
    ierr = VecSetType(*right, VECHIPMI355X);CHKERRQ(ierr);
  }
  if (left) {
    ierr = VecCreate(HipObjComm(A), left);CHKERRQ(ierr);
    ierr = VecSetSizes(*left, A->rmap->n, A->rmap->N);CHKERRQ(ierr);
    ierr = VecSetType(*left, VECHIPMI355X);CHKERRQ(ierr);
  }
  return 0;
}
PetscErrorCode MatGetVecs_HIPMI355X(Mat A, Vec *right, Vec *left) { return MatGetVecs_HIP(A, right, left); }

#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* the parent MATSEQAIJ's job inside a PETSc tree */
static PetscErrorCode MatDestroy_SeqAIJHIP(Mat A) {   /* free the mirror and zero spptr first, aijcusp.cu:584-586 */
  HipAIJ *a = SA(A);
  if (SD(A)) {
    Mat_SeqAIJHIP *d = SD(A);
    (void)HipTriFactorsDestroy(&d->tri);    /* a factored matrix: its triangular factors */
    (void)HipBlockFactorsDestroy(&d->btri); /* ... of a BAIJ operator: its block triangular factors (host/bilu.c) */
    product_free(A);                        /* the result of a product: its plan and inner results */
    device_free(A);
    if (d->time_ev) { for (PetscInt k = 0; k < 2 * d->time_cap; k++) mi355x_event_destroy(d->time_ev[k]); HipFree(d->time_ev); }
    HipFree(A->spptr); A->spptr = NULL;
  }
  if (a) { HipFree(a->i); HipFree(a->j); HipFree(a->a); HipFree(a->ilen); HipFree(a->imax); HipFree(a->inode_size); HipFree(a); A->data = NULL; }
  return 0;
}

#endif
#if defined(PETSCHIPMI355X_WITH_PETSC)
#include "aijhipmi355x_ctor.h"    /* integration/petsc-3.3/: the constructor as a subclass of the reference's MATSEQAIJ */
#include "baijhipmi355x_ctor.h"   /* ... and MATSEQBAIJHIPMI355X as a subclass of MATSEQBAIJ */
#else
static PetscErrorCode MatSeqAIJSetPreallocation_SeqAIJHIP(Mat A, PetscInt nz, const PetscInt nnz[]) { return seqaij_prealloc(A, nz, nnz); }
static PetscErrorCode MatSeqAIJSetPreallocationCSR_SeqAIJHIP(Mat B, const PetscInt *i, const PetscInt *j, const PetscScalar *a);
static PetscErrorCode MatSeqBAIJSetPreallocationCSR_SeqBAIJHIP(Mat B, PetscInt bs, const PetscInt *i, const PetscInt *j, const PetscScalar *a);
static PetscErrorCode MatDuplicate_SeqAIJHIP(Mat A, MatDuplicateOption op, Mat *M);

/* MatCreate_SeqAIJCUSP (aijcusp.cu:657-681) fills, after the parent constructor, the slots mult, multadd, multtranspose,
 * multtransposeadd, assemblyend, destroy, getvecs, setvaluesbatch; the container and its assembly are this file's too
 * (host/aijhip.c) on the harness, the parent MATSEQAIJ's inside a PETSc tree. */
static PetscErrorCode create_common(Mat B, const char *tname, PetscInt bs) {
  PetscErrorCode ierr;
  HipAIJ *a; Mat_SeqAIJHIP *d;
  if (HipCommSize(HipObjComm(B)) > 1) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_WRONG, "Comm must be of size 1");
  ierr = PetscMalloc(sizeof(*a), &a);CHKERRQ(ierr);
  memset(a, 0, sizeof(*a));
  ierr = PetscMalloc(sizeof(*d), &d);CHKERRQ(ierr);
  memset(d, 0, sizeof(*d));
  mirror_reset(d);
  a->m = B->rmap->n; a->n = B->cmap->n; a->bs = bs;
  B->data = a; B->spptr = d;
  ierr = PetscObjectChangeTypeName((PetscObject)B, tname);CHKERRQ(ierr);
  B->ops->setvalues = MatSetValues_SeqAIJHIP;
  B->ops->mult = MatMult_SeqAIJHIP;
  B->ops->multadd = MatMultAdd_SeqAIJHIP;
  B->ops->multtranspose = MatMultTranspose_SeqAIJHIP;
  B->ops->multtransposeadd = MatMultTransposeAdd_SeqAIJHIP;
  B->ops->getdiagonal = MatGetDiagonal_SeqAIJHIP;
  B->ops->assemblyend = MatAssemblyEnd_SeqAIJHIP;
  B->ops->zeroentries = MatZeroEntries_SeqAIJHIP;
  B->ops->setup = MatSetUp_SeqAIJHIP;
  B->ops->scale = MatScale_SeqAIJHIP;
  B->ops->shift = MatShift_SeqAIJHIP;
  B->ops->axpy = MatAXPY_SeqAIJHIP;
  B->ops->copy = MatCopy_SeqAIJHIP;
  B->ops->zerorows = MatZeroRows_SeqAIJHIP;
  B->ops->zerorowscolumns = MatZeroRowsColumns_SeqAIJHIP;
  B->ops->setoption = MatSetOption_SeqAIJHIP;
  B->ops->sor = MatSOR_SeqAIJHIP;
  B->ops->diagonalscale = MatDiagonalScale_SeqAIJHIP;
  B->ops->setvaluesbatch = MatSetValuesBatch_SeqAIJHIP;
  B->ops->norm = MatNorm_SeqAIJHIP;
  B->ops->getrowmaxabs = MatGetRowMaxAbs_SeqAIJHIP;
  B->ops->getrowmax = MatGetRowMax_SeqAIJHIP;
  B->ops->getrowmin = MatGetRowMin_SeqAIJHIP;
  B->ops->getcolumnnorms = MatGetColumnNorms_SeqAIJHIP;
  B->ops->duplicate = MatDuplicate_SeqAIJHIP;
  B->ops->matmult = MatMatMult_SeqAIJHIP;                     /* sequential AIJ operands; the block type answers PETSC_ERR_SUP */
  B->ops->matmultsymbolic = MatMatMultSymbolic_SeqAIJHIP;
  B->ops->matmultnumeric = MatMatMultNumeric_SeqAIJHIP;
  B->ops->transpose = MatTranspose_SeqAIJHIP;
  B->ops->ptap = MatPtAP_SeqAIJHIP;
  B->ops->setfromoptions = MatSetFromOptions_SeqAIJHIP;
  B->ops->destroy = MatDestroy_SeqAIJHIP;
  B->ops->getvecs = MatGetVecs_HIP;
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatSeqAIJGetArrays_C", "MatSeqAIJGetArrays", (PetscVoidFunction)MatSeqAIJGetArrays);CHKERRQ(ierr);
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatMultTDotBegin_C", "MatMultTDotBegin_HIPMI355X", (PetscVoidFunction)MatMultTDotBegin_HIPMI355X);CHKERRQ(ierr);
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatMultDiagonalScale_C", "MatMultDiagonalScale_HIPMI355X", (PetscVoidFunction)MatMultDiagonalScale_HIPMI355X);CHKERRQ(ierr);
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatCoarsenAggregate_C", "MatCoarsenAggregate_SeqAIJHIP", (PetscVoidFunction)MatCoarsenAggregate_SeqAIJHIP);CHKERRQ(ierr);   /* (the block type: PETSC_ERR_SUP) */
  if (bs == 1) {
    /* ILU(0) / ICC(0) of this type: the factored matrix carries the device triangular solves behind ops->solve (host/ilu.c), as
     * MatCreate_SeqAIJCUSPARSE overloads "MatGetFactor_petsc_C" (aijcusparse.cu:837-840) */
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatGetFactor_petsc_C", "MatGetFactor_seqaijhipmi355x_petsc", (PetscVoidFunction)MatGetFactor_seqaijhipmi355x_petsc);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatGetFactorAvailable_petsc_C", "MatGetFactorAvailable_seqaijhipmi355x_petsc", (PetscVoidFunction)MatGetFactorAvailable_seqaijhipmi355x_petsc);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatSeqAIJSetPreallocation_C", "MatSeqAIJSetPreallocation_SeqAIJHIP", (PetscVoidFunction)MatSeqAIJSetPreallocation_SeqAIJHIP);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatSeqAIJSetPreallocationCSR_C", "MatSeqAIJSetPreallocationCSR_SeqAIJHIP", (PetscVoidFunction)MatSeqAIJSetPreallocationCSR_SeqAIJHIP);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatResidual_C", "MatResidual_SeqAIJHIP", (PetscVoidFunction)MatResidual_SeqAIJHIP);CHKERRQ(ierr);   /* (the block type composes none: MatResidual takes the two calls) */
  } else {
    /* block ILU(k) of the block type (host/bilu.c): ILU only; ICC and LU answer PETSC_ERR_SUP */
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatGetFactor_petsc_C", "MatGetFactor_seqbaijhipmi355x_petsc", (PetscVoidFunction)MatGetFactor_seqbaijhipmi355x_petsc);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatGetFactorAvailable_petsc_C", "MatGetFactorAvailable_seqbaijhipmi355x_petsc", (PetscVoidFunction)MatGetFactorAvailable_seqbaijhipmi355x_petsc);CHKERRQ(ierr);
    ierr = PetscObjectComposeFunction((PetscObject)B, "MatSeqBAIJSetPreallocationCSR_C", "MatSeqBAIJSetPreallocationCSR_SeqBAIJHIP", (PetscVoidFunction)MatSeqBAIJSetPreallocationCSR_SeqBAIJHIP);CHKERRQ(ierr);
  }
  return 0;
}
/* MatDuplicate_SeqAIJ (aij.c:3964) / MatDuplicate_SeqBAIJ (baij.c:2874): same type, same layouts, the pattern copied, the values copied
 * (MAT_COPY_VALUES) or zero; MAT_SHARE_NONZERO_PATTERN copies the pattern as well (the harness container has no shared arrays).  The
 * type's options go along. */
static PetscErrorCode adopt_csr(Mat B, PetscInt nrows, PetscInt bs, const PetscInt *i, const PetscInt *j, const PetscScalar *a);
static PetscErrorCode MatDuplicate_SeqAIJHIP(Mat A, MatDuplicateOption op, Mat *M) {
  PetscErrorCode ierr;
  HipAIJ *a = SA(A);
  Mat B;
  if (!a->compact) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_WRONGSTATE, "Not for unassembled matrix");
  ierr = MatCreate(HipObjComm(A), &B);CHKERRQ(ierr);
  ierr = MatSetSizes(B, A->rmap->n, A->cmap->n, A->rmap->n, A->cmap->n);CHKERRQ(ierr);
  ierr = MatSetType(B, HipObjTypeName(A));CHKERRQ(ierr);
  ierr = adopt_csr(B, a->m, a->bs > 1 ? a->bs : 1, a->i, a->j, a->a);CHKERRQ(ierr);
  if (op != MAT_COPY_VALUES) memset(SA(B)->a, 0, sizeof(PetscScalar) * value_count(a));
  memcpy(SD(B)->opt, SD(A)->opt, sizeof(SD(A)->opt)); memcpy(SD(B)->opt_set, SD(A)->opt_set, sizeof(SD(A)->opt_set));
  SD(B)->cprow = SD(A)->cprow; memcpy(SD(B)->route, SD(A)->route, sizeof(SD(A)->route));
  SA(B)->keepnonzeropattern = a->keepnonzeropattern;
  *M = B;
  return 0;
}
PetscErrorCode MatCreate_SeqAIJHIPMI355X(Mat B) { return create_common(B, MATSEQAIJHIPMI355X, 1); }
PetscErrorCode MatCreate_SeqBAIJHIPMI355X(Mat B) { return create_common(B, MATSEQBAIJHIPMI355X, 0); }

/* MatCreateSeqAIJWithArrays (aij.c): the arrays are copied (the reference aliases them); i, j, a may be the matrix's own (MatDuplicate) */
static PetscErrorCode adopt_csr(Mat B, PetscInt nrows, PetscInt bs, const PetscInt *i, const PetscInt *j, const PetscScalar *a) {
  PetscErrorCode ierr;
  HipAIJ *s = SA(B);
  PetscInt nz = i[nrows];
  size_t vals = (size_t)nz * (size_t)(bs > 1 ? bs * bs : 1);
  if (i[0] != 0) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_OUTOFRANGE, "i (row indices) must start with 0");
  for (PetscInt r = 0; r < nrows; r++) if (i[r + 1] < i[r]) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_OUTOFRANGE, "Negative row length in i (row indices) row = %d length = %d", r, i[r + 1] - i[r]);
  {   /* column indices in range and ascending within each row (the kernels gather x[col] unchecked) */
    const PetscInt ncols = bs > 1 ? s->n / bs : s->n;
    for (PetscInt r = 0; r < nrows; r++) for (PetscInt k = i[r]; k < i[r + 1]; k++) {
      if (j[k] < 0 || j[k] >= ncols) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_OUTOFRANGE, "Column index %d out of range [0,%d) in row %d", j[k], ncols, r);
      if (k > i[r] && j[k] <= j[k - 1]) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_WRONG, "Column indices of row %d are not sorted and unique", r);
    }
  }
  device_free(B);   /* the matrix may have been used before (MatLoad into a used Mat): nothing of the old pattern survives */
  HipFree(s->i); HipFree(s->j); HipFree(s->a); HipFree(s->ilen); HipFree(s->imax);
  s->i = s->j = s->ilen = s->imax = NULL; s->a = NULL;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(nrows + 1), &s->i);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nz, 1), &s->j);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * PetscMax(vals, 1), &s->a);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nrows, 1), &s->ilen);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nrows, 1), &s->imax);CHKERRQ(ierr);
  memcpy(s->i, i, sizeof(PetscInt) * (size_t)(nrows + 1));
  memcpy(s->j, j, sizeof(PetscInt) * (size_t)nz);
  memcpy(s->a, a, sizeof(PetscScalar) * vals);
  s->nonzerorows = 0;
  for (PetscInt r = 0; r < nrows; r++) {
    s->ilen[r] = s->imax[r] = i[r + 1] - i[r];
    s->nonzerorows += (s->ilen[r] > 0);
  }
  s->nz = s->maxnz = nz; s->compact = PETSC_TRUE;
  if (bs > 1) { s->m = nrows; s->bs = bs; }
  B->preallocated = PETSC_TRUE; B->assembled = PETSC_TRUE; B->was_assembled = PETSC_TRUE; HipStateIncrease(B);
  return 0;
}
/* "MatSeqAIJSetPreallocationCSR_C" (aij.c:3795) and its BAIJ analogue (baij.c): m, n are point sizes; i, j index blocks */
static PetscErrorCode MatSeqAIJSetPreallocationCSR_SeqAIJHIP(Mat B, const PetscInt *i, const PetscInt *j, const PetscScalar *a) { return adopt_csr(B, B->rmap->n, 1, i, j, a); }
static PetscErrorCode MatSeqBAIJSetPreallocationCSR_SeqBAIJHIP(Mat B, PetscInt bs, const PetscInt *i, const PetscInt *j, const PetscScalar *a) {
  PetscErrorCode ierr;
  if (bs < 1 || B->rmap->n % bs || B->cmap->n % bs) SETERRQ(HipObjComm(B), PETSC_ERR_ARG_SIZ, "block size %d must divide the local sizes %d, %d", bs, B->rmap->n, B->cmap->n);
  SA(B)->bs = bs;                       /* the column check of adopt_csr counts block columns */
  ierr = adopt_csr(B, B->rmap->n / bs, bs, i, j, a);CHKERRQ(ierr);
  if (bs == 1) SA(B)->bs = 1;
  return 0;
}
#endif

PetscErrorCode MatSeqAIJGetArrays(Mat A, PetscInt *m, const PetscInt **i, const PetscInt **j, const PetscScalar **a) {
  if (!A || !A->data || (strcmp(HipObjTypeName(A), MATSEQAIJHIPMI355X) && strcmp(HipObjTypeName(A), MATSEQBAIJHIPMI355X))) SETERRQ(0, PETSC_ERR_ARG_WRONG, "not a SeqAIJHIPMI355X matrix");
  HipAIJ *s = SA(A);
  if (m) *m = s->m;
  if (i) *i = s->i;
  if (j) *j = s->j;
  if (a) *a = s->a;
  return 0;
}

/* ---- per-launch device timing used by bench.py (hipEvent pairs on the compute stream) ---- */
PetscErrorCode MatHIPMI355XSetTiming(Mat A, PetscBool on) {
  { PetscErrorCode ierr = seq_hip_check(A, "sequential HIPMI355X matrix expected");CHKERRQ(ierr); }
  Mat_SeqAIJHIP *d = SD(A);
  d->timing = on; d->time_n = 0;
  if (on && !d->time_ev) {
    d->time_cap = 4096;
    PetscErrorCode ierr = PetscMalloc(sizeof(mi355x_event_t) * 2 * (size_t)d->time_cap, &d->time_ev);CHKERRQ(ierr);
    for (PetscInt k = 0; k < 2 * d->time_cap; k++) CHKHIP(mi355x_event_create(&d->time_ev[k]));
  }
  return 0;
}
PetscErrorCode MatTimingBegin(Mat A, mi355x_handle_t h) {
  Mat_SeqAIJHIP *d = SD(A);
  if (d->timing && d->time_n < d->time_cap) CHKHIP(mi355x_event_record(d->time_ev[2 * d->time_n], h));
  return 0;
}
PetscErrorCode MatTimingEnd(Mat A, mi355x_handle_t h) {
  Mat_SeqAIJHIP *d = SD(A);
  if (d->timing && d->time_n < d->time_cap) { CHKHIP(mi355x_event_record(d->time_ev[2 * d->time_n + 1], h)); d->time_n++; }
  return 0;
}
PetscErrorCode MatHIPMI355XGetTiming(Mat A, PetscInt *nlaunches, PetscLogDouble *total_ms) {
  { PetscErrorCode ierr = seq_hip_check(A, "sequential HIPMI355X matrix expected");CHKERRQ(ierr); }
  Mat_SeqAIJHIP *d = SD(A);
  double tot = 0.0;
  for (PetscInt k = 0; k < d->time_n; k++) {
    float ms = 0.f;
    CHKHIP(mi355x_event_synchronize(d->time_ev[2 * k + 1]));
    CHKHIP(mi355x_event_elapsed_ms(d->time_ev[2 * k], d->time_ev[2 * k + 1], &ms));
    tot += ms;
  }
  if (nlaunches) *nlaunches = d->time_n;
  if (total_ms) *total_ms = tot;
  return 0;
}
