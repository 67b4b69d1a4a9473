/* MATMPIAIJHIPMI355X: row-block distributed CSR.  Mat_MPIAIJ layout and MatMult choreography of
 * src/mat/impls/aij/mpi/mpiaij.c:1102-1238 and mmaij.c:9-161; the GPU subclass role of
 * src/mat/impls/aij/mpi/mpicusp/mpiaijcusp.cu:85-112,204-235.  A (diagonal block, local columns)
 * and B (off-diagonal block, columns compacted through garray) are MATSEQAIJHIPMI355X. */
#include "hipmi355ximpl.h"

#define MA(A) HipMPIAIJGet(A)

#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* container, assembly and MatSetUpMultiply are the parent MATMPIAIJ's inside a PETSc tree */
static PetscErrorCode make_block(Mat parent, PetscInt m, PetscInt n, Mat *blk) {
  PetscErrorCode ierr;
  (void)parent;
  ierr = MatCreate(PETSC_COMM_SELF, blk);CHKERRQ(ierr);
  ierr = MatSetSizes(*blk, m, n, m, n);CHKERRQ(ierr);
  ierr = MatSetType(*blk, MATSEQAIJHIPMI355X);CHKERRQ(ierr);
  if (MA(parent)->keepnonzeropattern && (*blk)->ops->setoption) { ierr = (*(*blk)->ops->setoption)(*blk, MAT_KEEP_NONZERO_PATTERN, PETSC_TRUE);CHKERRQ(ierr); }   /* MatSetOption came first */
  return 0;
}

/* "MatMPIAIJSetPreallocation_C" (MatMPIAIJSetPreallocation_MPIAIJ, mpiaij.c; recomposed by the GPU subclass as in
 * mpiaijcusp.cu:36-46,213-215) */
static PetscErrorCode MatMPIAIJSetPreallocation_MPIAIJHIP(Mat A, PetscInt d_nz, const PetscInt d_nnz[], PetscInt o_nz, const PetscInt o_nnz[]) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (d_nz == PETSC_DEFAULT || d_nz == PETSC_DECIDE) d_nz = 5;     /* mpiaij.c MatMPIAIJSetPreallocation_MPIAIJ */
  if (o_nz == PETSC_DEFAULT || o_nz == PETSC_DECIDE) o_nz = 2;
  if (!a->A) {
    ierr = make_block(A, A->rmap->n, A->cmap->n, &a->A);CHKERRQ(ierr);
    ierr = make_block(A, A->rmap->n, A->cmap->N, &a->B);CHKERRQ(ierr);
  }
  ierr = MatSeqAIJSetPreallocation(a->A, d_nz, d_nnz);CHKERRQ(ierr);
  ierr = MatSeqAIJSetPreallocation(a->B, o_nz, o_nnz);CHKERRQ(ierr);
  A->preallocated = PETSC_TRUE;
  return 0;
}
static PetscErrorCode MatSetUp_MPIAIJHIP(Mat A) { return MatMPIAIJSetPreallocation_MPIAIJHIP(A, PETSC_DEFAULT, NULL, PETSC_DEFAULT, NULL); }

static int cmp_int(const void *a, const void *b) { PetscInt x = *(const PetscInt *)a, y = *(const PetscInt *)b; return (x > y) - (x < y); }

/* MatDisAssemble_MPIAIJ, mmaij.c:170-231: an entry in an off-diagonal column the assembled matrix does not have yet.  The
 * off-diagonal block goes back to GLOBAL column numbers (the reference builds a full-width B and re-inserts every row; garray is
 * increasing, so mapping the stored indices through it keeps every row sorted), the local work vector, the scatter and garray
 * are discarded; the next final assembly builds them again (MatSetUpMultiply_MPIAIJ) -- on every process, see MatAssemblyEnd */
static PetscErrorCode MatDisAssemble_MPIAIJHIP(Mat A) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (!a->garray) return 0;
  HipAIJ *B = HipAIJGet(a->B);
  for (PetscInt r = 0; r < B->m; r++)
    for (PetscInt k = B->i[r]; k < B->i[r] + B->ilen[r]; k++) B->j[k] = a->garray[B->j[k]];
  B->n = A->cmap->N;
  ierr = PetscLayoutDestroy(&a->B->cmap);CHKERRQ(ierr);
  ierr = PetscLayoutCreateSetUp(PETSC_COMM_SELF, A->cmap->N, A->cmap->N, &a->B->cmap);CHKERRQ(ierr);
  ierr = VecDestroy(&a->lvec);CHKERRQ(ierr);
  ierr = HipScatterDestroy(&a->hscat);CHKERRQ(ierr);
  HipFree(a->garray); a->garray = NULL; a->ec = 0;
  ierr = MatSeqAIJHIPSetCompressedRow(a->B, PETSC_FALSE);CHKERRQ(ierr);      /* (and: the device copy of B belongs to the old columns) */
  HipStateIncrease(a->B);
  return 0;
}

/* MatSetValues_MPIAIJ, mpiaij.c:517-560: locally owned rows go into A / B; rows of other processes are stashed until the
 * assembly (mpiaij.c:552-558, matstash.c), unless MAT_NO_OFF_PROC_ENTRIES-like behaviour is asked with nothing */
static PetscErrorCode MatSetValues_MPIAIJHIP(Mat A, PetscInt m, const PetscInt im[], PetscInt n, const PetscInt in[], const PetscScalar v[], InsertMode addv) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  for (PetscInt i = 0; i < m; i++) {
    if (im[i] < 0) continue;
    if (im[i] >= A->rmap->N) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Row too large: row %d max %d", im[i], A->rmap->N - 1);
    if (im[i] < a->rstart || im[i] >= a->rend) {
      for (PetscInt j = 0; j < n; j++) {
        if (in[j] < 0) continue;
        if (in[j] >= A->cmap->N) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Column too large: col %d max %d", in[j], A->cmap->N - 1);
        ierr = HipStashAdd(&a->stash, im[i], in[j], v[i * n + j], (int)addv);CHKERRQ(ierr);
      }
      continue;
    }
    PetscInt row = im[i] - a->rstart;
    for (PetscInt j = 0; j < n; j++) {
      PetscInt col = in[j];
      if (col < 0) continue;
      if (col >= A->cmap->N) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_OUTOFRANGE, "Column too large: col %d max %d", col, A->cmap->N - 1);
      if (col >= a->cstart && col < a->cend) {
        PetscInt lc = col - a->cstart;
        ierr = MatSetValues(a->A, 1, &row, 1, &lc, &v[i * n + j], addv);CHKERRQ(ierr);
      } else {
        PetscInt bc = col;
        if (a->garray) {   /* assembled before: B's columns are compacted (colmap lookup, mpiaij.c:540-550) */
          PetscInt *p = (PetscInt *)bsearch(&col, a->garray, (size_t)a->ec, sizeof(PetscInt), cmp_int);
          if (p) bc = (PetscInt)(p - a->garray);
          else { ierr = MatDisAssemble_MPIAIJHIP(A);CHKERRQ(ierr); }            /* mpiaij.c:545-549: from here on B takes global columns */
        }
        ierr = MatSetValues(a->B, 1, &row, 1, &bc, &v[i * n + j], addv);CHKERRQ(ierr);
      }
    }
  }
  return 0;
}

/* MatSetUpMultiply_MPIAIJ, mmaij.c:9-161 */
PetscErrorCode MatSetUpMultiply_MPIAIJ(Mat mat) {
  PetscErrorCode ierr;
  HipMPIAIJ *aij = MA(mat);
  HipAIJ *B = HipAIJGet(aij->B);
  PetscInt nzB = B->nz, ec = 0, *garray, *tmp;
  /* garray = sorted distinct global columns of B (mmaij.c:27-50) */
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nzB, 1), &tmp);CHKERRQ(ierr);
  memcpy(tmp, B->j, sizeof(PetscInt) * (size_t)nzB);
  qsort(tmp, (size_t)nzB, sizeof(PetscInt), cmp_int);
  for (PetscInt k = 0; k < nzB; k++) if (k == 0 || tmp[k] != tmp[k - 1]) tmp[ec++] = tmp[k];
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(ec + 1), &garray);CHKERRQ(ierr);
  memcpy(garray, tmp, sizeof(PetscInt) * (size_t)ec);
  HipFree(tmp);
  /* compact out the extra columns in B (mmaij.c:56-63) */
  for (PetscInt k = 0; k < nzB; k++) {
    PetscInt *p = (PetscInt *)bsearch(&B->j[k], garray, (size_t)ec, sizeof(PetscInt), cmp_int);
    B->j[k] = (PetscInt)(p - garray);
  }
  B->n = ec;
  ierr = PetscLayoutDestroy(&aij->B->cmap);CHKERRQ(ierr);
  ierr = PetscLayoutCreateSetUp(PETSC_COMM_SELF, ec, ec, &aij->B->cmap);CHKERRQ(ierr);
  HipStateIncrease(aij->B);
  /* local vector that is used to scatter into (mmaij.c:102) */
  ierr = VecCreateSeqHIPMI355X(PETSC_COMM_SELF, ec, &aij->lvec);CHKERRQ(ierr);
  /* generate the scatter context (mmaij.c:131-148) */
  ierr = HipScatterCreate_PtoS_MPIAIJ(HipObjComm(mat), mat->cmap, ec, garray, &aij->hscat);CHKERRQ(ierr);
  aij->garray = garray; aij->ec = ec;
  ierr = MatSeqAIJHIPSetCompressedRow(aij->B, PETSC_TRUE);CHKERRQ(ierr);
  return 0;
}

static PetscErrorCode MatAssemblyEnd_MPIAIJHIP(Mat A, MatAssemblyType mode) {   /* mpiaij.c:590-720 */
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  {   /* the stashed off-process entries reach their owners (MatAssemblyBegin/End_MPIAIJ: MatStashScatterBegin .. GetMesg),
       * rank after rank and in the order they were set */
    PetscInt nr, *ri, *rj; PetscScalar *rv; int smode;
    ierr = HipStashExchange(HipObjComm(A), &a->stash, &nr, &ri, &rj, &rv, &smode);CHKERRQ(ierr);
    for (PetscInt k = 0; k < nr; k++) {
      if (ri[k] < a->rstart || ri[k] >= a->rend) continue;
      ierr = MatSetValues_MPIAIJHIP(A, 1, &ri[k], 1, &rj[k], &rv[k], (InsertMode)smode);
      if (ierr) { HipFree(ri); HipFree(rj); HipFree(rv); CHKERRQ(ierr); }
    }
    HipFree(ri); HipFree(rj); HipFree(rv);
  }
  if (mode == MAT_FLUSH_ASSEMBLY) return 0;
  ierr = MatAssemblyBegin(a->A, mode);CHKERRQ(ierr);
  ierr = MatAssemblyEnd(a->A, mode);CHKERRQ(ierr);
  ierr = MatAssemblyBegin(a->B, mode);CHKERRQ(ierr);
  ierr = MatAssemblyEnd(a->B, mode);CHKERRQ(ierr);
  /* if one process has disassembled, all of them must (the scatter is rebuilt collectively): mpiaij.c:694-700 */
  if (A->was_assembled) {
    double dis = a->garray ? 0.0 : 1.0;
    if (HipCommAllreduce(HipObjComm(A), &dis, 1, 1, 0)) SETERRQ(HipObjComm(A), PETSC_ERR_LIB, "allreduce failed");
    if (dis > 0.0 && a->garray) { ierr = MatDisAssemble_MPIAIJHIP(A);CHKERRQ(ierr); }
  }
  if (!a->garray) { ierr = MatSetUpMultiply_MPIAIJ(A);CHKERRQ(ierr); }   /* mpiaij.c:701-703 */
  return 0;
}

#endif

static PetscErrorCode MatMult_MPIAIJHIP(Mat A, Vec xx, Vec yy) {   /* mpiaij.c:1102-1116 */
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (xx->map->n != A->cmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "Incompatible partition of A (%d) and xx (%d)", A->cmap->n, xx->map->n);
  /* Same dependences as the reference's Begin / mult / End sequence, but the diagonal-block SpMV is queued before
   * the host spends its ~tens of microseconds enqueueing the RCCL group: "x is final" is marked first. */
  ierr = HipScatterMarkReady(a->hscat, xx);CHKERRQ(ierr);
  ierr = (*a->A->ops->mult)(a->A, xx, yy);CHKERRQ(ierr);                                         /* compute stream */
  ierr = HipScatterBegin(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);   /* halo stream, overlaps */
  ierr = HipScatterEnd(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
  ierr = (*a->B->ops->multadd)(a->B, a->lvec, yy, yy);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode MatMultAdd_MPIAIJHIP(Mat A, Vec xx, Vec yy, Vec zz) {   /* mpiaij.c:1132-1143 */
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  ierr = HipScatterBegin(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
  ierr = (*a->A->ops->multadd)(a->A, xx, yy, zz);CHKERRQ(ierr);
  ierr = HipScatterEnd(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
  ierr = (*a->B->ops->multadd)(a->B, a->lvec, zz, zz);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode MatMultTranspose_MPIAIJHIP(Mat A, Vec xx, Vec yy) {   /* mpiaij.c:1147-1174, !merged branch */
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  ierr = (*a->B->ops->multtranspose)(a->B, xx, a->lvec);CHKERRQ(ierr);
  ierr = HipScatterBegin(a->hscat, a->lvec, yy, ADD_VALUES, SCATTER_REVERSE);CHKERRQ(ierr);
  ierr = (*a->A->ops->multtranspose)(a->A, xx, yy);CHKERRQ(ierr);
  ierr = HipScatterEnd(a->hscat, a->lvec, yy, ADD_VALUES, SCATTER_REVERSE);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode MatMultTransposeAdd_MPIAIJHIP(Mat A, Vec xx, Vec yy, Vec zz) {   /* mpiaij.c:1223-1238 */
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  ierr = (*a->B->ops->multtranspose)(a->B, xx, a->lvec);CHKERRQ(ierr);
  ierr = HipScatterBegin(a->hscat, a->lvec, zz, ADD_VALUES, SCATTER_REVERSE);CHKERRQ(ierr);
  ierr = (*a->A->ops->multtransposeadd)(a->A, xx, yy, zz);CHKERRQ(ierr);
  ierr = HipScatterEnd(a->hscat, a->lvec, zz, ADD_VALUES, SCATTER_REVERSE);CHKERRQ(ierr);
  return 0;
}
static PetscErrorCode MatGetDiagonal_MPIAIJHIP(Mat A, Vec v) {   /* mpiaij.c:1246-1256 */
  if (A->rmap->N != A->cmap->N) SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "Supports only square matrix where A->A is diag block");
  if (A->rmap->rstart != A->cmap->rstart || A->rmap->rend != A->cmap->rend) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "row partition must equal col partition");
  return (*MA(A)->A->ops->getdiagonal)(MA(A)->A, v);
}
static PetscErrorCode MatScale_MPIAIJHIP(Mat A, PetscScalar aa) {
  PetscErrorCode ierr;
  ierr = MatScale(MA(A)->A, aa);CHKERRQ(ierr);
  ierr = MatScale(MA(A)->B, aa);CHKERRQ(ierr);
  return 0;
}
/* MatDiagonalScale_MPIAIJ, mpiaij.c:2183-2213: the right vector's ghost values come through the MatMult scatter */
static PetscErrorCode MatDiagonalScale_MPIAIJHIP(Mat A, Vec ll, Vec rr) {
  PetscErrorCode ierr;
  HipMPIAIJ *aij = MA(A);
  if (rr) {
    if (rr->map->n != A->cmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "right vector non-conforming local size");
    ierr = HipScatterBegin(aij->hscat, rr, aij->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
  }
  if (ll) {
    if (ll->map->n != A->rmap->n) SETERRQ(HipObjComm(A), PETSC_ERR_ARG_SIZ, "left vector non-conforming local size");
    ierr = MatDiagonalScale(aij->B, ll, NULL);CHKERRQ(ierr);
  }
  ierr = MatDiagonalScale(aij->A, ll, rr);CHKERRQ(ierr);
  if (rr) {
    ierr = HipScatterEnd(aij->hscat, rr, aij->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
    ierr = MatDiagonalScale(aij->B, NULL, aij->lvec);CHKERRQ(ierr);
  }
  return 0;
}
static PetscErrorCode MatZeroEntries_MPIAIJHIP(Mat A) {
  PetscErrorCode ierr;
  ierr = MatZeroEntries(MA(A)->A);CHKERRQ(ierr);
  ierr = MatZeroEntries(MA(A)->B);CHKERRQ(ierr);
  return 0;
}
/* MatShift / MatAXPY / MatCopy (axpy.c:170, mpiaij.c:2470-2520 MatAXPY_MPIAIJ, 2290-2310 MatCopy_MPIAIJ): through the blocks, whose own
 * operators keep host and device copies side by side (host/aijhip.c).  The blocks' states are bumped here, as the public wrappers
 * would.  The off-diagonal blocks number their columns through each matrix's own garray. */
static PetscErrorCode MatShift_MPIAIJHIP(Mat A, PetscScalar alpha) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (a->A && a->A->ops->shift && A->rmap->rstart == A->cmap->rstart && A->rmap->rend == A->cmap->rend) {   /* the diagonal lies in the diagonal block */
    ierr = (*a->A->ops->shift)(a->A, alpha);CHKERRQ(ierr);
#if !defined(PETSCHIPMI355X_WITH_PETSC)   /* (inside a PETSc tree the block's own operator bumps its state: MatShift of 3.3 does not) */
    HipStateIncrease(a->A);
#endif
    return 0;
  }
  for (PetscInt i = A->rmap->rstart; i < A->rmap->rend; i++) { ierr = MatSetValues(A, 1, &i, 1, &i, &alpha, ADD_VALUES);CHKERRQ(ierr); }   /* the reference's default */
  ierr = MatAssemblyBegin(A, MAT_FINAL_ASSEMBLY);CHKERRQ(ierr);
  ierr = MatAssemblyEnd(A, MAT_FINAL_ASSEMBLY);CHKERRQ(ierr);
  return 0;
}
/* MatZeroRows_MPIAIJ (mpiaij.c): rows[] are global and may belong to any rank.  The lists of all ranks are gathered over the communicator's
 * host collective (the reference routes each row to its owner; a gather of a few boundary rows is the same information), every rank keeps
 * the rows it owns, and both blocks get them through their own zerorows slots -- whose host and device copies move side by side
 * (host/aijhip.c): the diagonal block with diag and the vectors (b[r] = diag x[r], once per owned row), the off-diagonal block with 0 and
 * none.  The blocks' states are bumped here, as the public wrapper would.  Without MAT_KEEP_NONZERO_PATTERN the blocks shrink their own
 * patterns; garray, the local vector and the scatter stay (they may then carry columns no entry uses, as in the reference).
 * Every rank sees every row: a row out of range is the same error everywhere.  n == 0 is a rank that only takes part. */
static PetscErrorCode MatZeroRows_MPIAIJHIP(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  MPI_Comm comm = HipObjComm(A);
  const int size = HipCommSize(comm);
  const PetscInt rs = A->rmap->rstart, re = A->rmap->rend;
  PetscInt *counts, *all = NULL, *lrows, maxn = 0, nl = 0, bad = 0; PetscBool isbad = PETSC_FALSE;
  if (!a->A || !a->B || !a->garray) SETERRQ(comm, PETSC_ERR_ARG_WRONGSTATE, "matrix must be assembled");
  if (!a->A->ops->zerorows || !a->B->ops->zerorows) SETERRQ(comm, PETSC_ERR_SUP, "the blocks have no MatZeroRows");
  double odd = (A->rmap->rstart == A->cmap->rstart && A->rmap->rend == A->cmap->rend) ? 0.0 : 1.0;   /* on any rank: the diagonal is not in the diagonal blocks */
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)size, &counts);CHKERRQ(ierr);
  counts[0] = n;
  if (size > 1) {
    if (HipCommAllgather(comm, &n, (int)sizeof(PetscInt), counts)) SETERRQ(comm, PETSC_ERR_LIB, "allgather failed");
    if (HipCommAllreduce(comm, &odd, 1, 1, 0)) SETERRQ(comm, PETSC_ERR_LIB, "allreduce failed");
  }
  for (int p = 0; p < size; p++) maxn = PetscMax(maxn, counts[p]);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(maxn, 1) * (size_t)size, &all);CHKERRQ(ierr);
  if (size > 1 && maxn > 0) {
    PetscInt *mine;
    ierr = PetscMalloc(sizeof(PetscInt) * (size_t)maxn, &mine);CHKERRQ(ierr);
    memset(mine, 0, sizeof(PetscInt) * (size_t)maxn);
    memcpy(mine, rows, sizeof(PetscInt) * (size_t)n);
    if (HipCommAllgather(comm, mine, (int)(sizeof(PetscInt) * (size_t)maxn), all)) SETERRQ(comm, PETSC_ERR_LIB, "allgather failed");
    HipFree(mine);
  } else if (n > 0) memcpy(all, rows, sizeof(PetscInt) * (size_t)n);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(maxn, 1) * (size_t)size, &lrows);CHKERRQ(ierr);
  for (int p = 0; p < size; p++) for (PetscInt q = 0; q < counts[p]; q++) {
    const PetscInt r = all[(size_t)p * (size_t)maxn + q];
    if (r < 0 || r >= A->rmap->N) { if (!isbad) { bad = r; isbad = PETSC_TRUE; } }
    else if (r >= rs && r < re) lrows[nl++] = r - rs;
  }
  HipFree(counts); HipFree(all);
  if (isbad) { HipFree(lrows); SETERRQ(comm, PETSC_ERR_ARG_OUTOFRANGE, "row %d out of range [0,%d)", bad, A->rmap->N); }
  if (odd > 0.0 && (diag != 0.0 || xx)) { HipFree(lrows); SETERRQ(comm, PETSC_ERR_SUP, "row and column ownership ranges differ: only diag == 0 without vectors"); }
  ierr = (*a->A->ops->zerorows)(a->A, nl, lrows, diag, xx, bb);
  if (!ierr) { HipStateIncrease(a->A); ierr = (*a->B->ops->zerorows)(a->B, nl, lrows, 0.0, NULL, NULL); }
  if (!ierr) HipStateIncrease(a->B);
  HipFree(lrows);
  CHKERRQ(ierr);
  return 0;
}
/* the columns of MatZeroRowsColumns belong to other ranks' rows as well: the mask and x have to travel through the halo scatter first.
 * Not written yet (sections 8 and 11) */
static PetscErrorCode MatZeroRowsColumns_MPIAIJHIP(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec xx, Vec bb) {
  (void)n; (void)rows; (void)diag; (void)xx; (void)bb;
  SETERRQ(HipObjComm(A), PETSC_ERR_SUP, "MatZeroRowsColumns of a parallel matrix is not supported: use MatZeroRows, or a sequential matrix");
}
/* MatSOR_MPIAIJ (mpiaij.c): the local sweeps only -- each process relaxes its diagonal block, the other processes' unknowns frozen for
 * the lits sweeps of one outer step.  From a zero guess the first step is the block's own MatSOR on b; every further step moves x into
 * the halo (the MatMult scatter), forms bb1 = b - B x_halo (lvec negated, then the off-diagonal block's multadd) and relaxes the block on
 * bb1 with the non-local twin of the sweep.  bb1 stays with the matrix and is made by the first call that takes such a step.  A sweep
 * over the whole parallel matrix (a non-local bit), Eisenstat's trick and the triangular applications are refused */
static PetscErrorCode MatSOR_MPIAIJHIP(Mat A, Vec bb, PetscReal omega, MatSORType flag_, PetscReal fshift, PetscInt its, PetscInt lits, Vec xx) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  MPI_Comm comm = HipObjComm(A);
  const int flag = (int)flag_;
  MatSORType twin;
  (void)comm;
  if (!a->A || !a->B || !a->garray) SETERRQ(comm, PETSC_ERR_ARG_WRONGSTATE, "matrix must be assembled");
  if (flag & (SOR_EISENSTAT | SOR_APPLY_UPPER | SOR_APPLY_LOWER)) SETERRQ(comm, PETSC_ERR_SUP, "Eisenstat and SOR_APPLY_UPPER / SOR_APPLY_LOWER are not supported on a parallel matrix");
  if (flag & SOR_SYMMETRIC_SWEEP) SETERRQ(comm, PETSC_ERR_SUP, "Parallel SOR not supported");
  if ((flag & SOR_LOCAL_SYMMETRIC_SWEEP) == SOR_LOCAL_SYMMETRIC_SWEEP) twin = SOR_SYMMETRIC_SWEEP;
  else if (flag & SOR_LOCAL_FORWARD_SWEEP) twin = SOR_FORWARD_SWEEP;
  else if (flag & SOR_LOCAL_BACKWARD_SWEEP) twin = SOR_BACKWARD_SWEEP;
  else SETERRQ(comm, PETSC_ERR_SUP, "Parallel SOR not supported");
  if (!a->A->ops->sor || !a->B->ops->multadd) SETERRQ(comm, PETSC_ERR_SUP, "the blocks have no MatSOR");
  if (its <= 0 || lits <= 0) SETERRQ(comm, PETSC_ERR_ARG_WRONG, "Relaxation requires global its %d and local its %d both positive", its, lits);
  if (bb == xx) SETERRQ(comm, PETSC_ERR_ARG_IDN, "b and x vector cannot be the same");
  if (flag & SOR_ZERO_INITIAL_GUESS) {
    ierr = (*a->A->ops->sor)(a->A, bb, omega, (MatSORType)flag, fshift, lits, 1, xx);CHKERRQ(ierr);
    its--;
  }
  if (its > 0 && !a->sor_bb1) { ierr = VecDuplicate(bb, &a->sor_bb1);CHKERRQ(ierr); }
  while (its-- > 0) {
    ierr = HipScatterBegin(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
    ierr = HipScatterEnd(a->hscat, xx, a->lvec, INSERT_VALUES, SCATTER_FORWARD);CHKERRQ(ierr);
    ierr = (*a->lvec->ops->scale)(a->lvec, -1.0);CHKERRQ(ierr);   /* the vector's own slot: the plug-in takes no VecScale from the object model */
    HipStateIncrease(a->lvec);
    ierr = (*a->B->ops->multadd)(a->B, a->lvec, bb, a->sor_bb1);CHKERRQ(ierr);
    ierr = (*a->A->ops->sor)(a->A, a->sor_bb1, omega, twin, fshift, lits, 1, xx);CHKERRQ(ierr);
  }
  return 0;
}
/* ---------------------------------------------------------------- Norms and row / column reductions (MatNorm_MPIAIJ, MatGetRowMaxAbs_MPIAIJ,
 * MatGetRowMax_MPIAIJ, MatGetRowMin_MPIAIJ mpiaij.c; MatGetColumnNorms_MPIAIJ): through the blocks' own reductions (host/aijhip.c, either
 * route as the diagonal block resolves -mat_hipmi355x_reductions) and the communicator's host collectives.
 *   NORM_INFINITY   a row's sum of |a| runs over its diagonal-block entries and continues, from that value, over its off-diagonal-block
 *                   entries (the ADD form; the compressed-row device copy of B through its row list); local maximum, one max all-reduce.
 *                   A local quantity per row: the bits do not depend on the number of ranks' reduction order
 *   NORM_FROBENIUS  the two blocks' sums of squares added, one sum all-reduce, the root
 *   NORM_1, column norms   local column results into an array of the N global columns -- the diagonal block's at cstart + c, the
 *                   off-diagonal block's at garray[c] --, one all-reduce of N doubles (sum; max for NORM_INFINITY), then the maximum / the roots
 *   row max-abs / max / min   both blocks are reduced as parts of a matrix of N columns (a block's row is full only with N entries) and
 *                   compete on the host: the larger (smaller) value wins, equal values go to the smaller global column; a row whose two
 *                   blocks both end at the implicit zero, and a row that stores all N columns, is scanned over its merged columns in
 *                   ascending global order -- the sequential contract itself.  Columns are global. */
static PetscReal mpi_host_max_of(const PetscScalar *x, PetscInt n) {
  if (n <= 0) return 0.0;
  PetscReal m = x[0];
  for (PetscInt k = 1; k < n; k++) if (x[k] > m) m = x[k];
  return m;
}
/* the local column results of both blocks in an array of the N global columns (zero elsewhere) */
static PetscErrorCode mpi_local_columns(Mat A, int route, int op, PetscScalar *glob) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  const PetscInt nd = A->cmap->n, ec = a->ec, N = A->cmap->N, cstart = A->cmap->rstart;
  PetscScalar *w;
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(PetscMax(nd, ec), 1), &w);CHKERRQ(ierr);
  for (PetscInt c = 0; c < N; c++) glob[c] = 0.0;
  ierr = MatBlockColReduce_SeqAIJHIP(a->A, route, op, w);
  if (!ierr) { for (PetscInt c = 0; c < nd; c++) glob[cstart + c] = w[c]; }
  if (!ierr && ec > 0) {
    ierr = MatBlockColReduce_SeqAIJHIP(a->B, route, op, w);
    if (!ierr) for (PetscInt c = 0; c < ec; c++) glob[a->garray[c]] = w[c];
  }
  HipFree(w);
  return ierr;
}
static PetscErrorCode MatNorm_MPIAIJHIP(Mat A, NormType type, PetscReal *nrm) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  MPI_Comm comm = HipObjComm(A);
  const PetscInt m = A->rmap->n, N = A->cmap->N;
  int route;
  if (type == NORM_2) SETERRQ(comm, PETSC_ERR_SUP, "No support for two norm");
  if (type != NORM_1 && type != NORM_FROBENIUS && type != NORM_INFINITY) SETERRQ(comm, PETSC_ERR_ARG_OUTOFRANGE, "Unknown NormType %d", (int)type);
  ierr = MatReductionsRoute_SeqAIJHIP(a->A, &route);CHKERRQ(ierr);
  if (type == NORM_FROBENIUS) {
    PetscReal s1, s2, s;
    ierr = MatBlockSquareSum_SeqAIJHIP(a->A, route, &s1);CHKERRQ(ierr);
    ierr = MatBlockSquareSum_SeqAIJHIP(a->B, route, &s2);CHKERRQ(ierr);
    s = s1 + s2;
    if (HipCommSize(comm) > 1 && HipCommAllreduce(comm, &s, 1, 1, 0)) SETERRQ(comm, PETSC_ERR_LIB, "allreduce failed");
    *nrm = sqrt(s);
  } else if (type == NORM_1) {
    PetscScalar *glob;
    ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(N, 1), &glob);CHKERRQ(ierr);
    ierr = mpi_local_columns(A, route, MI355X_ROW_ABSSUM, glob);
    if (!ierr && HipCommSize(comm) > 1 && N > 0 && HipCommAllreduce(comm, glob, (int)N, 1, 0)) { HipFree(glob); SETERRQ(comm, PETSC_ERR_LIB, "allreduce failed"); }
    if (!ierr) *nrm = mpi_host_max_of(glob, N);
    HipFree(glob);
    CHKERRQ(ierr);
  } else {
    PetscReal v = 0.0;
    if (route == 2) {
      PetscScalar *w;
      ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(m, 1), &w);CHKERRQ(ierr);
      ierr = MatBlockRowReduce_SeqAIJHIP(a->A, 2, MI355X_ROW_ABSSUM, N, PETSC_FALSE, w, NULL);
      if (!ierr) ierr = MatBlockRowReduce_SeqAIJHIP(a->B, 2, MI355X_ROW_ABSSUM, N, PETSC_TRUE, w, NULL);
      if (!ierr) v = mpi_host_max_of(w, m);
      HipFree(w);
      CHKERRQ(ierr);
    } else {
      void *w = NULL;
      CHKHIP(mi355x_malloc(&w, sizeof(PetscScalar) * (size_t)PetscMax(m, 2)));
      ierr = MatBlockRowReduce_SeqAIJHIP(a->A, 1, MI355X_ROW_ABSSUM, N, PETSC_FALSE, (PetscScalar *)w, NULL);
      if (!ierr) ierr = MatBlockRowReduce_SeqAIJHIP(a->B, 1, MI355X_ROW_ABSSUM, N, PETSC_TRUE, (PetscScalar *)w, NULL);
      if (!ierr) ierr = HipDeviceMaxOf((const PetscScalar *)w, m, &v);
      mi355x_free(w);
      CHKERRQ(ierr);
    }
    if (HipCommSize(comm) > 1 && HipCommAllreduce(comm, &v, 1, 1, 1)) SETERRQ(comm, PETSC_ERR_LIB, "allreduce failed");
    *nrm = v;
  }
  return 0;
}
static PetscErrorCode MatGetColumnNorms_MPIAIJHIP(Mat A, NormType type, PetscReal *norms) {
  PetscErrorCode ierr;
  MPI_Comm comm = HipObjComm(A);
  const PetscInt N = A->cmap->N;
  int route;
  const int op = type == NORM_1 ? MI355X_ROW_ABSSUM : (type == NORM_2 ? MI355X_ROW_SQSUM : MI355X_ROW_MAXABS);
  if (type != NORM_1 && type != NORM_2 && type != NORM_INFINITY) SETERRQ(comm, PETSC_ERR_ARG_WRONG, "Unknown NormType %d", (int)type);
  ierr = MatReductionsRoute_SeqAIJHIP(MA(A)->A, &route);CHKERRQ(ierr);
  ierr = mpi_local_columns(A, route, op, norms);CHKERRQ(ierr);
  if (HipCommSize(comm) > 1 && N > 0 && HipCommAllreduce(comm, norms, (int)N, 1, type == NORM_INFINITY ? 1 : 0)) SETERRQ(comm, PETSC_ERR_LIB, "allreduce failed");
  if (type == NORM_2) for (PetscInt c = 0; c < N; c++) norms[c] = sqrt(norms[c]);
  return 0;
}
/* row r of the parallel matrix by the sequential contract over its merged columns (ascending global column) */
static void mpi_row_scan(Mat A, int op, PetscInt r, PetscScalar *val, PetscInt *col) {
  HipMPIAIJ *a = MA(A);
  const HipAIJ *d = HipAIJGet(a->A), *o = HipAIJGet(a->B);
  const PetscInt cstart = A->cmap->rstart, N = A->cmap->N;
  PetscInt kd = d->i[r], ko = o->i[r];
  const PetscInt ed = d->i[r + 1], eo = o->i[r + 1], n = (ed - kd) + (eo - ko);
  const PetscBool full = (PetscBool)(n > 0 && n == N);
  PetscScalar cur = 0.0; PetscInt best = -1, missing = -1, expect = 0;
  for (PetscInt j = 0; j < n; j++) {
    const PetscBool from_d = (PetscBool)(kd < ed && (ko >= eo || cstart + d->j[kd] < a->garray[o->j[ko]]));
    const PetscInt c = from_d ? cstart + d->j[kd] : a->garray[o->j[ko]];
    PetscScalar v = from_d ? d->a[kd++] : o->a[ko++];
    if (op == MI355X_ROW_MAXABS) v = fabs(v);
    if (missing < 0 && c != expect) missing = expect;
    expect = c + 1;
    if ((op != MI355X_ROW_MAXABS && j == 0 && full) || (op == MI355X_ROW_MIN ? v < cur : cur < v)) { cur = v; best = c; }
  }
  if (missing < 0) missing = n;                       /* columns 0 .. n - 1 are stored: the next one is the first missing */
  *val = cur;
  *col = best >= 0 ? best : ((op == MI355X_ROW_MAXABS || n == 0) ? 0 : missing);
}
static PetscErrorCode mpi_row_extremum(Mat A, int op, Vec v, PetscInt idx[]) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  MPI_Comm comm = HipObjComm(A); (void)comm;
  const HipAIJ *hd = HipAIJGet(a->A), *ho = HipAIJGet(a->B);
  const PetscInt m = A->rmap->n, N = A->cmap->N, cstart = A->cmap->rstart;
  const size_t mm = (size_t)PetscMax(m, 2);
  PetscScalar *vd, *vo, *out; PetscInt *id, *io;
  int route;
  if (!v || !v->data || !strstr(HipObjTypeName(v), "hipmi355x")) SETERRQ(comm, PETSC_ERR_ARG_WRONG, "the result must be a HIPMI355X vector");
  if (v->map->n != m) SETERRQ(comm, PETSC_ERR_ARG_SIZ, "Nonconforming matrix and vector");
  ierr = MatReductionsRoute_SeqAIJHIP(a->A, &route);CHKERRQ(ierr);
  ierr = PetscMalloc(2 * sizeof(PetscScalar) * mm + 2 * sizeof(PetscInt) * mm, &vd);CHKERRQ(ierr);
  vo = vd + mm; id = (PetscInt *)(vo + mm); io = id + mm;
  if (route == 2) {
    ierr = MatBlockRowReduce_SeqAIJHIP(a->A, 2, op, N, PETSC_FALSE, vd, id);
    if (!ierr) ierr = MatBlockRowReduce_SeqAIJHIP(a->B, 2, op, N, PETSC_FALSE, vo, io);
  } else {
    PetscDeviceCtx *dc; void *w = NULL;
    ierr = PetscDeviceGet(&dc);
    if (!ierr) {
      int rc = mi355x_malloc(&w, 2 * sizeof(PetscScalar) * mm + 2 * sizeof(PetscInt) * mm);
      if (rc) { HipFree(vd); CHKHIP(rc); }
      PetscScalar *wd = (PetscScalar *)w, *wo = wd + mm; PetscInt *xd = (PetscInt *)(wo + mm), *xo = xd + mm;
      ierr = MatBlockRowReduce_SeqAIJHIP(a->A, 1, op, N, PETSC_FALSE, wd, xd);
      if (!ierr) ierr = MatBlockRowReduce_SeqAIJHIP(a->B, 1, op, N, PETSC_FALSE, wo, xo);
      if (!ierr && m > 0) {
        rc = mi355x_memcpy_d2h(dc->h, vd, w, 2 * sizeof(PetscScalar) * mm + 2 * sizeof(PetscInt) * mm);
        if (!rc) rc = mi355x_handle_synchronize(dc->h);
        if (rc) { mi355x_free(w); HipFree(vd); CHKHIP(rc); }
      }
      mi355x_free(w);
    }
  }
  if (ierr) { HipFree(vd); CHKERRQ(ierr); }
  ierr = VecGetArray(v, &out);
  if (ierr) { HipFree(vd); CHKERRQ(ierr); }
  for (PetscInt r = 0; r < m; r++) {
    const PetscInt nd = hd->i[r + 1] - hd->i[r], no = ho->i[r + 1] - ho->i[r];
    /* a block's value is 0.0 exactly when no stored entry of it won: max-abs 0.0 at column 0, max / min the implicit zero (a stored
     * +-0.0 never replaces the start, and no block row is full unless the whole row lies in it) */
    PetscScalar val; PetscInt col;
    if ((vd[r] == 0.0 && vo[r] == 0.0) || (nd + no == N && N > 0) || vd[r] != vd[r] || vo[r] != vo[r]) mpi_row_scan(A, op, r, &val, &col);
    else {
      const PetscInt cd = cstart + id[r], co = no > 0 ? a->garray[io[r]] : 0;
      PetscBool take_o;
      if (vd[r] == 0.0) take_o = PETSC_TRUE;               /* the diagonal block offers its start only: the other block's stored entry beat 0.0 */
      else if (vo[r] == 0.0) take_o = PETSC_FALSE;
      else if (vd[r] == vo[r]) take_o = (PetscBool)(co < cd);
      else take_o = (PetscBool)(op == MI355X_ROW_MIN ? vo[r] < vd[r] : vd[r] < vo[r]);
      val = take_o ? vo[r] : vd[r]; col = take_o ? co : cd;
    }
    out[r] = val;
    if (idx) idx[r] = col;
  }
  HipFree(vd);
  return VecRestoreArray(v, &out);
}
static PetscErrorCode MatGetRowMaxAbs_MPIAIJHIP(Mat A, Vec v, PetscInt idx[]) { return mpi_row_extremum(A, MI355X_ROW_MAXABS, v, idx); }
static PetscErrorCode MatGetRowMax_MPIAIJHIP(Mat A, Vec v, PetscInt idx[]) { return mpi_row_extremum(A, MI355X_ROW_MAX, v, idx); }
static PetscErrorCode MatGetRowMin_MPIAIJHIP(Mat A, Vec v, PetscInt idx[]) { return mpi_row_extremum(A, MI355X_ROW_MIN, v, idx); }

static PetscErrorCode mpi_value_op_pair(Mat Y, Mat X) {
  if (!X || strcmp(HipObjTypeName(X), MATMPIAIJHIPMI355X) || strcmp(HipObjTypeName(Y), MATMPIAIJHIPMI355X)) SETERRQ(HipObjComm(Y), PETSC_ERR_SUP, "both matrices must be MPIAIJHIPMI355X matrices");
  if (X->rmap->rstart != Y->rmap->rstart || X->rmap->rend != Y->rmap->rend || X->cmap->rstart != Y->cmap->rstart || X->cmap->rend != Y->cmap->rend)
    SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_SIZ, "the two matrices must have the same row and column layouts");
  if (!MA(X)->A || !MA(Y)->A || !MA(X)->garray || !MA(Y)->garray) SETERRQ(HipObjComm(Y), PETSC_ERR_ARG_WRONGSTATE, "both matrices must be assembled");
  return 0;
}
static PetscErrorCode MatAXPY_MPIAIJHIP(Mat Y, PetscScalar alpha, Mat X, MatStructure str) {
  PetscErrorCode ierr;
  ierr = mpi_value_op_pair(Y, X);CHKERRQ(ierr);
  HipMPIAIJ *x = MA(X), *y = MA(Y);
  /* both blocks are checked before either is changed: an error leaves Y as it was */
  ierr = MatValueOpsCheck_SeqAIJHIP(y->A, x->A, str, NULL, NULL, PETSC_FALSE);CHKERRQ(ierr);
  ierr = MatValueOpsCheck_SeqAIJHIP(y->B, x->B, str, x->garray, y->garray, PETSC_FALSE);CHKERRQ(ierr);
  ierr = MatAXPY_SeqAIJHIP_Cols(y->A, alpha, x->A, str, NULL, NULL, PETSC_TRUE);CHKERRQ(ierr);
  HipStateIncrease(y->A);
  ierr = MatAXPY_SeqAIJHIP_Cols(y->B, alpha, x->B, str, x->garray, y->garray, PETSC_TRUE);CHKERRQ(ierr);
  HipStateIncrease(y->B);
#if defined(PETSCHIPMI355X_WITH_PETSC)
  HipStateIncrease(Y);
#endif
  return 0;
}
static PetscErrorCode MatCopy_MPIAIJHIP(Mat A, Mat B, MatStructure str) {
  PetscErrorCode ierr;
  if (A == B) return 0;
  ierr = mpi_value_op_pair(B, A);CHKERRQ(ierr);
  HipMPIAIJ *a = MA(A), *b = MA(B);
  ierr = MatValueOpsCheck_SeqAIJHIP(b->A, a->A, str, NULL, NULL, PETSC_TRUE);CHKERRQ(ierr);
  ierr = MatValueOpsCheck_SeqAIJHIP(b->B, a->B, str, a->garray, b->garray, PETSC_TRUE);CHKERRQ(ierr);
  ierr = MatCopy_SeqAIJHIP_Cols(a->A, b->A, str, NULL, NULL, PETSC_TRUE);CHKERRQ(ierr);
  HipStateIncrease(b->A);
  ierr = MatCopy_SeqAIJHIP_Cols(a->B, b->B, str, a->garray, b->garray, PETSC_TRUE);CHKERRQ(ierr);
  HipStateIncrease(b->B);
  return 0;
}
#if defined(PETSCHIPMI355X_WITH_PETSC)
#include "mpiaijhipmi355x_ctor.h"   /* integration/petsc-3.3/: the constructor as a subclass of the reference's MATMPIAIJ */
#else
/* MatSetOption_MPIAIJ, mpiaij.c: MAT_KEEP_NONZERO_PATTERN goes to both blocks (now, or when they are made) */
static PetscErrorCode MatSetOption_MPIAIJHIP(Mat A, MatOption op, PetscBool flg) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (op != MAT_KEEP_NONZERO_PATTERN) return 0;
  a->keepnonzeropattern = flg;
  if (a->A && a->A->ops->setoption) { ierr = (*a->A->ops->setoption)(a->A, op, flg);CHKERRQ(ierr); }
  if (a->B && a->B->ops->setoption) { ierr = (*a->B->ops->setoption)(a->B, op, flg);CHKERRQ(ierr); }
  return 0;
}
static PetscErrorCode MatDestroy_MPIAIJHIP(Mat A) {
  PetscErrorCode ierr;
  HipMPIAIJ *a = MA(A);
  if (!a) return 0;
  ierr = MatDestroy(&a->A);CHKERRQ(ierr);
  ierr = MatDestroy(&a->B);CHKERRQ(ierr);
  ierr = VecDestroy(&a->lvec);CHKERRQ(ierr);
  ierr = VecDestroy(&a->sor_bb1);CHKERRQ(ierr);
  ierr = HipScatterDestroy(&a->hscat);CHKERRQ(ierr);
  HipFree(a->garray);
  HipStashFree(&a->stash);
  HipFree(a); A->data = NULL;
  return 0;
}

static PetscErrorCode MatMPIAIJSetPreallocationCSR_MPIAIJHIP(Mat A, const PetscInt i[], const PetscInt j[], const PetscScalar a[]);
static PetscErrorCode MatGetDiagonalBlock_MPIAIJHIP(Mat A, Mat *a) { *a = MA(A)->A; return 0; }   /* MatGetDiagonalBlock_MPIAIJ, mpiaij.c */

PetscErrorCode MatCreate_MPIAIJHIPMI355X(Mat B) {   /* MatCreate_MPIAIJCUSP, mpiaijcusp.cu:204-235 */
  PetscErrorCode ierr;
  HipMPIAIJ *a;
  ierr = PetscMalloc(sizeof(*a), &a);CHKERRQ(ierr);
  memset(a, 0, sizeof(*a));
  a->rstart = B->rmap->rstart; a->rend = B->rmap->rend; a->cstart = B->cmap->rstart; a->cend = B->cmap->rend;
  B->data = a;
  ierr = PetscObjectChangeTypeName((PetscObject)B, MATMPIAIJHIPMI355X);CHKERRQ(ierr);
  B->ops->setvalues = MatSetValues_MPIAIJHIP;
  B->ops->mult = MatMult_MPIAIJHIP;
  B->ops->multadd = MatMultAdd_MPIAIJHIP;
  B->ops->multtranspose = MatMultTranspose_MPIAIJHIP;
  B->ops->multtransposeadd = MatMultTransposeAdd_MPIAIJHIP;
  B->ops->getdiagonal = MatGetDiagonal_MPIAIJHIP;
  B->ops->assemblyend = MatAssemblyEnd_MPIAIJHIP;
  B->ops->zeroentries = MatZeroEntries_MPIAIJHIP;
  B->ops->setup = MatSetUp_MPIAIJHIP;
  B->ops->scale = MatScale_MPIAIJHIP;
  B->ops->shift = MatShift_MPIAIJHIP;
  B->ops->axpy = MatAXPY_MPIAIJHIP;
  B->ops->copy = MatCopy_MPIAIJHIP;
  B->ops->zerorows = MatZeroRows_MPIAIJHIP;
  B->ops->zerorowscolumns = MatZeroRowsColumns_MPIAIJHIP;
  B->ops->setoption = MatSetOption_MPIAIJHIP;
  B->ops->sor = MatSOR_MPIAIJHIP;
  B->ops->diagonalscale = MatDiagonalScale_MPIAIJHIP;
  B->ops->norm = MatNorm_MPIAIJHIP;
  B->ops->getrowmaxabs = MatGetRowMaxAbs_MPIAIJHIP;
  B->ops->getrowmax = MatGetRowMax_MPIAIJHIP;
  B->ops->getrowmin = MatGetRowMin_MPIAIJHIP;
  B->ops->getcolumnnorms = MatGetColumnNorms_MPIAIJHIP;
  B->ops->destroy = MatDestroy_MPIAIJHIP;
  B->ops->getvecs = MatGetVecs_HIPMI355X;
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatMPIAIJSetPreallocation_C", "MatMPIAIJSetPreallocation_MPIAIJHIP", (PetscVoidFunction)MatMPIAIJSetPreallocation_MPIAIJHIP);CHKERRQ(ierr);
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatMPIAIJSetPreallocationCSR_C", "MatMPIAIJSetPreallocationCSR_MPIAIJHIP", (PetscVoidFunction)MatMPIAIJSetPreallocationCSR_MPIAIJHIP);CHKERRQ(ierr);
  ierr = PetscObjectComposeFunction((PetscObject)B, "MatGetDiagonalBlock_C", "MatGetDiagonalBlock_MPIAIJHIP", (PetscVoidFunction)MatGetDiagonalBlock_MPIAIJHIP);CHKERRQ(ierr);
  return 0;
}
#endif

/* base name "aijhipmi355x" -> seq or mpi by communicator size (MatRegisterBaseName, matreg.c:161-180) */
PetscErrorCode MatCreate_AIJHIPMI355X(Mat B) {
  return (HipCommSize(HipObjComm(B)) == 1) ? MatCreate_SeqAIJHIPMI355X(B) : MatCreate_MPIAIJHIPMI355X(B);
}

#if !defined(PETSCHIPMI355X_WITH_PETSC)
/* "MatMPIAIJSetPreallocationCSR_C" (MatMPIAIJSetPreallocationCSR_MPIAIJ, mpiaij.c:3900-3960): fills the matrix from this
 * rank's rows in CSR form, global ascending column indices.  The split is the column test of MatSetValues_MPIAIJ in bulk. */
static PetscErrorCode MatMPIAIJSetPreallocationCSR_MPIAIJHIP(Mat A, const PetscInt i[], const PetscInt j[], const PetscScalar a[]) {
  PetscErrorCode ierr;
  const PetscInt m = A->rmap->n;
  MPI_Comm comm = HipObjComm(A);
  HipMPIAIJ *aij = MA(A);
  (void)comm;
  if (i[0]) SETERRQ(comm, PETSC_ERR_ARG_OUTOFRANGE, "i (row indices) must start with 0");
  if (aij->A) { ierr = MatDestroy(&aij->A);CHKERRQ(ierr); ierr = MatDestroy(&aij->B);CHKERRQ(ierr); }
  PetscInt cs = aij->cstart, ce = aij->cend, nd = 0, no = 0;
  for (PetscInt k = 0; k < i[m]; k++) { if (j[k] >= cs && j[k] < ce) nd++; else no++; }
  PetscInt *di, *dj, *oi, *oj; PetscScalar *da, *oa;
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(m + 1), &di);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)(m + 1), &oi);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(nd, 1), &dj);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscInt) * (size_t)PetscMax(no, 1), &oj);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(nd, 1), &da);CHKERRQ(ierr);
  ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)PetscMax(no, 1), &oa);CHKERRQ(ierr);
  nd = no = 0; di[0] = oi[0] = 0;
  for (PetscInt r = 0; r < m; r++) {
    for (PetscInt k = i[r]; k < i[r + 1]; k++) {
      if (j[k] < 0 || j[k] >= A->cmap->N) SETERRQ(comm, PETSC_ERR_ARG_OUTOFRANGE, "Column %d out of range [0,%d) in row %d", j[k], A->cmap->N, r);
      if (k > i[r] && j[k] <= j[k - 1]) SETERRQ(comm, PETSC_ERR_ARG_WRONG, "columns of row %d must be ascending and distinct", r);
      if (j[k] >= cs && j[k] < ce) { dj[nd] = j[k] - cs; da[nd++] = a[k]; }
      else { oj[no] = j[k]; oa[no++] = a[k]; }
    }
    di[r + 1] = nd; oi[r + 1] = no;
  }
  ierr = make_block(A, m, A->cmap->n, &aij->A);CHKERRQ(ierr);
  ierr = MatSeqAIJSetPreallocationCSR(aij->A, di, dj, da);CHKERRQ(ierr);
  ierr = make_block(A, m, A->cmap->N, &aij->B);CHKERRQ(ierr);
  ierr = MatSeqAIJSetPreallocationCSR(aij->B, oi, oj, oa);CHKERRQ(ierr);
  HipFree(di); HipFree(dj); HipFree(da); HipFree(oi); HipFree(oj); HipFree(oa);
  A->preallocated = PETSC_TRUE;
  ierr = MatSetUpMultiply_MPIAIJ(A);CHKERRQ(ierr);
  A->assembled = PETSC_TRUE; A->was_assembled = PETSC_TRUE; HipStateIncrease(A);
  return 0;
}

#endif

PetscErrorCode MatMPIAIJGetSeqAIJ(Mat A, Mat *Ad, Mat *Ao, const PetscInt **garray) {   /* mpiaij.c MatMPIAIJGetSeqAIJ */
  if (!A || strcmp(HipObjTypeName(A), MATMPIAIJHIPMI355X)) SETERRQ(0, PETSC_ERR_ARG_WRONG, "not an MPIAIJHIPMI355X matrix");
  if (Ad) *Ad = MA(A)->A;
  if (Ao) *Ao = MA(A)->B;
  if (garray) *garray = MA(A)->garray;
  return 0;
}
PetscErrorCode MatMPIAIJGetScatter(Mat A, VecScatter *ctx, Vec *lvec, PetscInt *ec) {
  if (!A || strcmp(HipObjTypeName(A), MATMPIAIJHIPMI355X)) SETERRQ(0, PETSC_ERR_ARG_WRONG, "not an MPIAIJHIPMI355X matrix");
  if (ctx) *ctx = (VecScatter)MA(A)->hscat;
  if (lvec) *lvec = MA(A)->lvec;
  if (ec) *ec = MA(A)->ec;
  return 0;
}

/* ---- bench.py: how the halo exchange of MatMult_MPIAIJ (mpiaij.c:1102-1116; VecScatterBegin_1/End_1, vpscat.h:14-233) sits beside the
 * diagonal-block product.  Event pairs: the diagonal product on the compute stream (MatHIPMI355XSetTiming of the diagonal block) and
 * the exchange on the halo stream (HipScatterSetTiming), one pair of each per MatMult.  Reported over the products timed so far:
 *   halo_ms     sum of the halo stream's busy spans (pack, grouped send/recv, unpack)
 *   overlap_ms  the part of those spans inside the diagonal product's span
 *   exposed_ms  what the compute stream waits for after its diagonal product has ended (halo end - product end, where positive)
 *   send_bytes  bytes this rank sends per product, neighbours: to how many ranks ---- */
PetscErrorCode MatMPIAIJHIPMI355XSetHaloTiming(Mat A, PetscBool on) {
  PetscErrorCode ierr;
  if (!A || strcmp(HipObjTypeName(A), MATMPIAIJHIPMI355X)) SETERRQ(0, PETSC_ERR_ARG_WRONG, "not an MPIAIJHIPMI355X matrix");
  ierr = MatHIPMI355XSetTiming(MA(A)->A, on);CHKERRQ(ierr);
  if (MA(A)->hscat) { ierr = HipScatterSetTiming(MA(A)->hscat, on);CHKERRQ(ierr); }
  return 0;
}
PetscErrorCode MatMPIAIJHIPMI355XGetHaloTiming(Mat A, PetscInt *nproducts, PetscLogDouble *halo_ms, PetscLogDouble *overlap_ms, PetscLogDouble *exposed_ms,
                                               PetscLogDouble *send_bytes, PetscInt *neighbours) {
  if (!A || strcmp(HipObjTypeName(A), MATMPIAIJHIPMI355X)) SETERRQ(0, PETSC_ERR_ARG_WRONG, "not an MPIAIJHIPMI355X matrix");
  HipScatter sc = MA(A)->hscat;
  Mat_SeqAIJHIP *d = (Mat_SeqAIJHIP *)MA(A)->A->spptr;
  double halo = 0.0, over = 0.0, expo = 0.0;
  PetscInt n = 0;
  if (sc && d && sc->time_ev && d->time_ev) {
    n = PetscMin(sc->time_n, d->time_n);
    for (PetscInt k = 0; k < n; k++) {
      mi355x_event_t s0 = d->time_ev[2 * k], s1 = d->time_ev[2 * k + 1], h0 = sc->time_ev[2 * k], h1 = sc->time_ev[2 * k + 1];
      float ts1 = 0.f, th0 = 0.f, th1 = 0.f;     /* all measured from the start of the diagonal product */
      CHKHIP(mi355x_event_synchronize(s1));
      CHKHIP(mi355x_event_synchronize(h1));
      CHKHIP(mi355x_event_elapsed_ms(s0, s1, &ts1));
      CHKHIP(mi355x_event_elapsed_ms(s0, h0, &th0));
      CHKHIP(mi355x_event_elapsed_ms(s0, h1, &th1));
      const double lo = th0 > 0.f ? th0 : 0.0, hi = th1 < ts1 ? th1 : ts1;
      halo += (double)th1 - (double)th0;
      if (hi > lo) over += hi - lo;
      if (th1 > ts1) expo += (double)th1 - (double)ts1;
    }
  }
  if (nproducts) *nproducts = n;
  if (halo_ms) *halo_ms = halo;
  if (overlap_ms) *overlap_ms = over;
  if (exposed_ms) *exposed_ms = expo;
  if (send_bytes) *send_bytes = sc ? (double)sizeof(PetscScalar) * (double)sc->to.starts[sc->to.n] : 0.0;
  if (neighbours) *neighbours = sc ? sc->to.n : 0;
  return 0;
}
