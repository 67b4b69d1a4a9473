/* MatNullSpace: the null space of a singular operator and its removal from a vector (src/mat/interface/matnull.c).  A KSP that has
 * one (KSPSetNullSpace) projects it out after every preconditioner application (kspimpl.h KSP_RemoveNullSpace; harness/ksp.c).
 * Host control flow only: the sums, shifts, dots and updates dispatch through the Vec function table. */
#include "petscimpl.h"

PetscErrorCode MatNullSpaceCreate(PetscComm comm, PetscBool has_cnst, PetscInt n, const Vec vecs[], MatNullSpace *SP) {   /* matnull.c MatNullSpaceCreate */
  PetscErrorCode ierr;
  MatNullSpace sp;
  if (n < 0) SETERRQ(comm, PETSC_ERR_ARG_OUTOFRANGE, "Number of basis vectors (given %d) cannot be negative", n);
  if (n && !vecs) SETERRQ(comm, PETSC_ERR_ARG_NULL, "Null Pointer: Parameter # 4");
  ierr = PetscMalloc(sizeof(*sp), &sp);CHKERRQ(ierr);
  memset(sp, 0, sizeof(*sp));
  sp->comm = comm; sp->has_cnst = has_cnst; sp->n = n; sp->refct = 1;
  if (n) {
    ierr = PetscMalloc(sizeof(Vec) * (size_t)n, &sp->vecs);CHKERRQ(ierr);
    ierr = PetscMalloc(sizeof(PetscScalar) * (size_t)n, &sp->alpha);CHKERRQ(ierr);
    for (PetscInt i = 0; i < n; i++) { vecs[i]->xrefs++; sp->vecs[i] = vecs[i]; }   /* PetscObjectReference */
  }
  *SP = sp;
  return 0;
}
PetscErrorCode MatNullSpaceDestroy(MatNullSpace *sp) {
  PetscErrorCode ierr;
  if (!*sp) return 0;
  if (--(*sp)->refct > 0) { *sp = NULL; return 0; }
  ierr = VecDestroy(&(*sp)->vec);CHKERRQ(ierr);
  for (PetscInt i = 0; i < (*sp)->n; i++) { ierr = VecDestroy(&(*sp)->vecs[i]);CHKERRQ(ierr); }
  free((*sp)->vecs); free((*sp)->alpha);
  free(*sp); *sp = NULL;
  return 0;
}
PetscErrorCode MatNullSpaceSetFunction(MatNullSpace sp, PetscErrorCode (*rem)(MatNullSpace, Vec, void *), void *ctx) {
  if (!sp) SETERRQ(0, PETSC_ERR_ARG_NULL, "Null Object: Parameter # 1");
  sp->remove = rem; sp->rmctx = ctx;
  return 0;
}

/* matnull.c MatNullSpaceRemove, in its order: the constant (VecSum; sum / (-1.0 * N); VecShift), the basis vectors (VecMDot, negate,
 * VecMAXPY), the user's function.  A vector type on one rank may offer the first step as one call whose sum stays on its side
 * ("VecShiftByMean_C": v += sum(v) / den, the same arithmetic). */
PetscErrorCode MatNullSpaceRemove(MatNullSpace sp, Vec vec, Vec *out) {
  PetscErrorCode ierr;
  PetscScalar sum;
  PetscInt N;
  if (!sp) SETERRQ(0, PETSC_ERR_ARG_NULL, "Null Object: Parameter # 1");
  if (!vec) SETERRQ(sp->comm, PETSC_ERR_ARG_NULL, "Null Object: Parameter # 2");
  if (out) {
    if (!sp->vec) { ierr = VecDuplicate(vec, &sp->vec);CHKERRQ(ierr); }
    ierr = VecCopy(vec, sp->vec);CHKERRQ(ierr);
    vec = *out = sp->vec;
  }
  if (sp->has_cnst) {
    ierr = VecGetSize(vec, &N);CHKERRQ(ierr);
    if (N > 0) {
      PetscVoidFunction f = NULL;
      ierr = PetscObjectQueryFunction((PetscObject)vec, "VecShiftByMean_C", &f);CHKERRQ(ierr);
      if (f && sp->comm->size == 1) { ierr = ((PetscErrorCode (*)(Vec, PetscScalar))f)(vec, -1.0 * N);CHKERRQ(ierr); }
      else {
        ierr = VecSum(vec, &sum);CHKERRQ(ierr);
        sum = sum / (-1.0 * N);
        ierr = VecShift(vec, sum);CHKERRQ(ierr);
      }
    }
  }
  if (sp->n) {
    ierr = VecMDot(vec, sp->n, sp->vecs, sp->alpha);CHKERRQ(ierr);
    for (PetscInt i = 0; i < sp->n; i++) sp->alpha[i] = -sp->alpha[i];
    ierr = VecMAXPY(vec, sp->n, sp->alpha, sp->vecs);CHKERRQ(ierr);
  }
  if (sp->remove) { ierr = (*sp->remove)(sp, vec, sp->rmctx);CHKERRQ(ierr); }
  return 0;
}

/* matnull.c MatNullSpaceTest: |A (1/N)|, |A v_j| and |A (removed copy)| against 1e-7 */
PetscErrorCode MatNullSpaceTest(MatNullSpace sp, Mat mat, PetscBool *isNull) {
  PetscErrorCode ierr;
  Vec l, r;
  PetscReal nrm;
  PetscInt N;
  PetscBool consistent = PETSC_TRUE;
  if (!sp) SETERRQ(0, PETSC_ERR_ARG_NULL, "Null Object: Parameter # 1");
  if (!sp->vec) {
    Vec right;
    ierr = MatGetVecs(mat, &right, NULL);CHKERRQ(ierr);
    sp->vec = right;
  }
  l = sp->vec;
  if (sp->has_cnst) {
    ierr = VecDuplicate(l, &r);CHKERRQ(ierr);
    ierr = VecGetSize(l, &N);CHKERRQ(ierr);
    ierr = VecSet(l, 1.0 / N);CHKERRQ(ierr);
    ierr = MatMult(mat, l, r);CHKERRQ(ierr);
    ierr = VecNorm(r, NORM_2, &nrm);CHKERRQ(ierr);
    if (nrm >= 1.e-7) consistent = PETSC_FALSE;
    ierr = VecDestroy(&r);CHKERRQ(ierr);
  }
  for (PetscInt j = 0; j < sp->n; j++) {
    ierr = MatMult(mat, sp->vecs[j], l);CHKERRQ(ierr);
    ierr = VecNorm(l, NORM_2, &nrm);CHKERRQ(ierr);
    if (nrm >= 1.e-7) consistent = PETSC_FALSE;
  }
  if (sp->remove) {
    Vec rem;
    ierr = VecGetSize(l, &N);CHKERRQ(ierr);
    ierr = VecSet(l, 1.0 / N);CHKERRQ(ierr);
    ierr = VecDuplicate(l, &rem);CHKERRQ(ierr);
    ierr = VecCopy(l, rem);CHKERRQ(ierr);                       /* the function works on a copy */
    ierr = (*sp->remove)(sp, rem, sp->rmctx);CHKERRQ(ierr);
    ierr = MatMult(mat, rem, l);CHKERRQ(ierr);
    ierr = VecNorm(l, NORM_2, &nrm);CHKERRQ(ierr);
    if (nrm >= 1.e-7) consistent = PETSC_FALSE;
    ierr = VecDestroy(&rem);CHKERRQ(ierr);
  }
  if (isNull) *isNull = consistent;
  return 0;
}
