/* The optional fused-kernel interface between a Krylov driver and the Vec / Mat types it runs on.  A type that has such
 * kernels composes them on its objects under the names below (PetscObjectComposeFunction, the reference's mechanism for
 * type-specific methods: e.g. "MatMPIAIJSetPreallocation_C", mpiaij.c:5421); a driver that knows them queries by name
 * (PetscObjectQueryFunction) and falls back to the reference's op-by-op sequence when the name is absent.  The reference's own
 * KSPSolve_CG / _GMRES / _BCGS never ask, and run op by op over the same types.  Every fused form is bit-identical to the calls it
 * replaces.  Included by the harness drivers and by the plug-in; needs Vec / Mat / PetscScalar declared before it. */
#if !defined(PETSCKRYLOVFUSED_H)
#define PETSCKRYLOVFUSED_H

/* ---- optional, type-specific methods the drivers look up by name (PetscObjectQueryFunction), never link against ----
 * "VecKrylovFusedOps_C" on a Vec returns a table of fused Krylov kernels (several BLAS-1 calls of KSPSolve_CG / _BCGS in
 * one sweep, results bit-identical to the separate calls); absent -> the drivers run the reference's op-by-op sequence.
 * "MatMultTDotBegin_C" on a Mat: y = A x with x'y left on the device for the fused CG update.
 * "MatMultDiagonalScale_C" on a Mat: y = d .* (A x), MatMult followed by PCApply_Jacobi, in one kernel. */
typedef struct {
  PetscErrorCode (*cg_update)(Vec x, Vec r, Vec z, Vec p, Vec w, Vec d, PetscScalar a, PetscScalar *zz, PetscScalar *zr, PetscScalar *rr, PetscBool *done);
  PetscErrorCode (*cg_update_check)(Vec x, Vec r, Vec z, Vec p, Vec w, Vec d, PetscBool *ok);
  PetscErrorCode (*tdot_begin)(Vec x, Vec y, PetscBool *ok);
  PetscErrorCode (*cg_update_dev_begin)(Vec x, Vec r, Vec z, Vec p, Vec w, Vec d, PetscScalar beta, PetscScalar dpiold, PetscBool check_sign);
  PetscErrorCode (*cg_update_dev_end)(Vec x, PetscScalar *zz, PetscScalar *zr, PetscScalar *rr, PetscScalar *dpi);
  PetscErrorCode (*aypx_dev)(Vec p, PetscScalar den, Vec z);
  PetscErrorCode (*pmult_dot)(Vec w, Vec x, Vec d, Vec y, PetscScalar *val, PetscBool *done);
  PetscErrorCode (*pmult_dotnorm2)(Vec w, Vec x, Vec d, Vec s, PetscScalar *dp, PetscReal *nm, PetscBool *done);
  PetscErrorCode (*bcgs_update)(Vec x, Vec r, Vec p, Vec s, Vec t, Vec rp, PetscScalar alpha, PetscScalar omega, PetscScalar *rr, PetscScalar *rho, PetscBool *done);
  /* KSPGMRESClassicalGramSchmidtOrthogonalization without refinement (borthog2.c:60-66) and the VecNormalize that follows it
   * (gmres.c:146): dots[j] = <w, V[j]>, w -= sum_j dots[j] V[j], *nrm = |w|, w /= |w|; one host wait instead of three */
  PetscErrorCode (*gmres_orthog_normalize)(Vec w, PetscInt nv, const Vec V[], PetscScalar *dots, PetscReal *nrm, PetscBool *done);
  /* cg_update_dev_begin without x += a p (r -= a w, z = B r and the sums only), and aypx_dev that applies that x += a p with
   * the p it is about to overwrite (a = beta / p'w with the same device-side tests; a refused step leaves x alone): the pair
   * computes what cg_update_dev_begin followed by aypx_dev computes, with one pass over p fewer */
  PetscErrorCode (*cg_update_dev_begin_nox)(Vec r, Vec z, Vec w, Vec d, PetscScalar beta, PetscScalar dpiold, PetscBool check_sign);
  PetscErrorCode (*aypx_dev_x)(Vec p, PetscScalar den, Vec z, Vec x, PetscScalar beta, PetscScalar dpiold, PetscBool check_sign);
  /* One step of KSPSolve_Chebychev (cheby.c) behind w = A p[k]: r = b - w (VecAYPX; stored only with r != NULL, r may be w),
   * z = d .* r (PCApply_Jacobi; d == NULL: identity), pn = s z (VecScale) + a pm (VecAXPY) + c pk (VecAXPY) with the special cases of
   * those calls, and with zz, rr != NULL *zz = z'z, *rr = r'r (the sums VecNorm roots) -- one sweep, the bits of the separate calls.
   * zz == rr == NULL: the pure element-wise form, nothing reduced, no host wait.  b == NULL: w is the preconditioned residual as
   * given (any PC applied it, a null space was removed): z = w, d and r must be NULL, no sums, and w may be pn itself.
   * pn overlaps no other operand.  *done = PETSC_FALSE and nothing touched otherwise. */
  PetscErrorCode (*cheby_step)(Vec pn, Vec r, Vec w, Vec b, Vec d, Vec pm, Vec pk, PetscScalar s, PetscScalar a, PetscScalar c, PetscScalar *zz, PetscScalar *rr, PetscBool *done);
  /* One step of KSPSolve_Richardson (rich.c) behind w = A x: r = b - w (stored with r != NULL, r may be w), z = d .* r (stored with
   * z != NULL), x += scale z (VecAXPY) */
  PetscErrorCode (*rich_step)(Vec x, Vec r, Vec z, Vec w, Vec b, Vec d, PetscScalar scale, PetscBool *done);
} VecKrylovFusedOps;
typedef const VecKrylovFusedOps *(*VecKrylovFusedOpsGetFn)(void);
/* "VecPipelinedCGFusedOps_C" on a Vec returns the sweeps of the pipelined CG family, a table of its own.  Their sums are not waited
 * for: a sweep leaves them PENDING as the VecNormBegin / VecDotBegin calls it replaces would have, same kinds in the same order, and
 * the driver's PetscCommSplitReductionBegin, VecNormEnd and VecDotEnd follow as in the op-by-op sequence.  A split phase already
 * begun: PETSC_ERR_ORDER.  *done = PETSC_FALSE and nothing touched when the sweep refuses its operands. */
typedef struct {
  /* The body of KSPSolve_PIPECG's loop (pipecg.c:138-175) behind mv = B w and nv = A mv:
   *   first: zrec = nv, qrec = mv, p = u, s = w (VecCopy x4); else zrec = nv + ratio zrec, .. , s = w + ratio s (VecAYPX x4);
   *   x += step p, u -= step qrec, w -= step zrec, r -= step s (VecAXPY x4);
   *   m_next != NULL: m_next = d .* w, the next iteration's PCApply_Jacobi (d == NULL: PCNONE's copy); m_next may be mv;
   *   rides 1 / 2 / 3: VecNormBegin(r) / VecNormBegin(u) / VecDotBegin(r, u), then VecDotBegin(w, u), on the updated vectors, pending;
   *   rides 0: nothing is reduced.
   * No written vector is another operand (but m_next == mv). */
  PetscErrorCode (*pipecg_step)(Vec x, Vec u, Vec w, Vec r, Vec zrec, Vec qrec, Vec p, Vec s, Vec nv, Vec mv, Vec d, Vec m_next,
                                PetscBool first, PetscScalar ratio, PetscScalar step, PetscInt rides, PetscBool *done);
} VecPipelinedCGFusedOps;
typedef const VecPipelinedCGFusedOps *(*VecPipelinedCGFusedOpsGetFn)(void);
/* "VecMinresFusedOps_C" on a Vec returns the two sweeps of a MINRES iteration (KSPSolve_MINRES, minres.c), a third table.  *done =
 * PETSC_FALSE and nothing touched when a sweep refuses its operands: a vector of another type, unequal local sizes, or a written
 * vector that is another operand of the call. */
typedef struct {
  /* Behind r = A u and alpha = u'r:  d != NULL: z = d .* r (PCApply_Jacobi; z is not read), d == NULL: z as KSP_PCApply left it;
   *   r -= alpha v ; z -= alpha u ; r -= beta vold ; z -= beta uold (VecAXPY x4 in this order) ; *dp = r'z (VecDot, all-reduced).
   * alpha_on_device: alpha is what tdot_begin(u, r) of "VecKrylovFusedOps_C" left on the device and the argument is ignored; either
   * way *alpha_out returns the value the sweep used, with the one wait that brings *dp. */
  PetscErrorCode (*minres_lanczos)(Vec r, Vec z, Vec v, Vec u, Vec vold, Vec uold, Vec d, PetscScalar alpha, PetscBool alpha_on_device, PetscScalar beta,
                                   PetscScalar *dp, PetscScalar *alpha_out, PetscBool *done);
  /* wold = (u - rho2 w - rho3 wold) irho1 (VecCopy, VecAXPY x2, VecScale: the new W, the caller rotates its three names) ;
   * x += ceta wold (VecAXPY) ; vnew = ibeta r ; unew = ibeta z (VecCopy + VecScale x2).  first: vnew and unew alone (the solve start;
   * x, u, w, wold may be NULL).  Nothing is reduced and the host does not wait. */
  PetscErrorCode (*minres_update)(Vec x, Vec u, Vec w, Vec wold, Vec r, Vec z, Vec vnew, Vec unew, PetscBool first,
                                  PetscScalar rho2, PetscScalar rho3, PetscScalar irho1, PetscScalar ceta, PetscScalar ibeta, PetscBool *done);
} VecMinresFusedOps;
typedef const VecMinresFusedOps *(*VecMinresFusedOpsGetFn)(void);
/* "VecTfqmrFusedOps_C" on a Vec returns the three sweeps of an iteration of KSPSolve_TFQMR (tfqmr.c) and KSPSolve_CGS (cgs.c), a fourth
 * table.  *done = PETSC_FALSE and nothing touched when a sweep refuses its operands: a vector of another type or on another device,
 * unequal local sizes, or a written vector that is another operand of the call. */
typedef struct {
  /* q = u - a v (VecWAXPY(Q, -a, V, U)) ; t = u + q (VecWAXPY(T, 1.0, U, Q)) ; x != NULL (CGS): x += a t (VecAXPY(X, a, T)).
   * Nothing is reduced and the host does not wait. */
  PetscErrorCode (*tfqmr_qt)(Vec u, Vec v, Vec q, Vec t, Vec x, PetscScalar a, PetscBool *done);
  /* r -= a auq (VecAXPY(R, -a, AUQ)) ; *rr = r'r (the sum VecNorm(R, NORM_2) takes the root of) ; *rrp = r'rp (VecDot(R, RP)), both over
   * the updated r and all-reduced, in one wait. */
  PetscErrorCode (*tfqmr_resid)(Vec r, Vec auq, Vec rp, PetscScalar a, PetscScalar *rr, PetscScalar *rrp, PetscBool *done);
  /* nhalves >= 1: d = u + cf0 d ; x += eta0 d.  nhalves == 2: then d = q + cf1 d ; x += eta1 d (VecAYPX + VecAXPY per half step of TFQMR;
   * the halves read the old u and q).  tail: u = r + b q ; q += b p ; p = u + b q (VecWAXPY, VecAXPY, VecWAXPY).  nhalves == 0 (CGS):
   * d and x are not touched and may be NULL; !tail (an exit inside the half steps): r and p likewise.  Nothing is reduced. */
  PetscErrorCode (*tfqmr_update)(Vec d, Vec x, Vec u, Vec q, Vec r, Vec p, PetscInt nhalves, PetscScalar cf0, PetscScalar eta0, PetscScalar cf1, PetscScalar eta1,
                                 PetscBool tail, PetscScalar b, PetscBool *done);
} VecTfqmrFusedOps;
typedef const VecTfqmrFusedOps *(*VecTfqmrFusedOpsGetFn)(void);
/* "VecBicgFusedOps_C" on a Vec returns the two sweeps of an iteration of KSPSolve_BiCG (bicg.c), a fifth table.  *done = PETSC_FALSE and
 * nothing touched when a sweep refuses its operands: a vector of another type or on another device, unequal local sizes, or a written
 * vector that is another operand of the call. */
typedef struct {
  /* first: pr = zr ; pl = zl (VecCopy x2).  Else pr = zr + b pr ; pl = zl + b pl (VecAYPX x2).  Nothing is reduced, no host wait. */
  PetscErrorCode (*bicg_dirs)(Vec pr, Vec pl, Vec zr, Vec zl, PetscScalar b, PetscBool first, PetscBool *done);
  /* x += a pr ; rr -= a zr ; rl -= a zl (VecAXPY x3 in this order).  d != NULL (PCJACOBI: PCApply and PCApplyTranspose alike) or identity
   * (PCNONE): zr = d .* rr and zl = d .* rl (or the copies) in the same pass, with *beta = zr'rl (VecDot(Zr, Rl)) and *nrm2 = zr'zr
   * (which == 0) or rr'rr (which == 1), the sum VecNorm(.., NORM_2) takes the root of.  Otherwise zr and zl are only read, *beta is not
   * set and *nrm2 = rr'rr.  The sums are over the updated vectors, all-reduced, and arrive in one wait. */
  PetscErrorCode (*bicg_update)(Vec x, Vec rr, Vec rl, Vec pr, Vec zr, Vec zl, Vec d, PetscBool identity, PetscScalar a, PetscInt which,
                                PetscScalar *beta, PetscScalar *nrm2, PetscBool *done);
} VecBicgFusedOps;
typedef const VecBicgFusedOps *(*VecBicgFusedOpsGetFn)(void);
/* "VecLsqrFusedOps_C" on a Vec returns the two sweeps of an iteration of KSPSolve_LSQR (lsqr.c), a sixth table.  *done = PETSC_FALSE and
 * nothing touched when a sweep refuses its operands: a vector of another type or on another device, unequal local sizes, a written
 * vector that is another operand of the call, or a route the communicator cannot take. */
typedef enum {
  LSQR_BIDIAG_WAIT = 0,   /* coef from the host; sums[0] = y'y, all-reduced, comes home in one wait */
  LSQR_BIDIAG_QUEUE = 1,  /* coef from the host; y'y stays in a device slot and y = y / sqrt(y'y) is queued behind the sweep (VecNormalize's rule:
                             a zero norm leaves y alone); the host does not wait and sums is not written.  One rank only: the slot would hold a
                             local partial sum */
  LSQR_BIDIAG_FINISH = 2  /* coef = sqrt of the sum the QUEUE call before it left in the slot, formed on the device, the argument ignored;
                             sums[0] = that sum, sums[1] = y'y: both in one wait.  One rank only, and only behind a QUEUE call */
} VecLsqrBidiagRoute;
typedef struct {
  /* y -= coef x (VecAXPY(Y, -coef, X)) ; y'y, the sum VecNorm(Y, NORM_2) takes the root of, over the updated y */
  PetscErrorCode (*lsqr_bidiag)(Vec x, Vec y, PetscScalar coef, VecLsqrBidiagRoute route, PetscScalar sums[2], PetscBool *done);
  /* v1 = ialpha v1 (VecScale) ; x += step w (VecAXPY) ; se != NULL: se += irho2 (w .* w) (VecCopy, VecPointwiseMult, VecScale, VecAXPY) ;
   * w = v1 + cf w (VecAYPX).  skip_w: w is not stored (the breakdown exit).  x == NULL with step == 0, and w == NULL with skip_w, step == 0
   * and se == NULL: that vector is not looked at; the last form is a plain scaling of v1.  Nothing is reduced, the host does not wait. */
  PetscErrorCode (*lsqr_update)(Vec v1, Vec x, Vec w, Vec se, PetscScalar ialpha, PetscScalar step, PetscScalar cf, PetscScalar irho2, PetscBool skip_w,
                                PetscBool *done);
} VecLsqrFusedOps;
typedef const VecLsqrFusedOps *(*VecLsqrFusedOpsGetFn)(void);
/* "VecFgmresFusedOps_C" on a Vec returns the Gram-Schmidt step of flexible GMRES (KSPFGMRESCycle, fgmres.c), a seventh table */
typedef struct {
  /* gmres_orthog_normalize of "VecKrylovFusedOps_C" (dots[j] = <w, V_j>, w -= sum_j dots[j] V_j, *nrm = |w|, w *= 1 / |w| under
   * VecNormalize's rules) whose last sweep also writes the next step's preconditioned direction from the values it holds:
   * z = d .* w_new (PCApply_Jacobi), or z = w_new with identity set (PCApply_None; d is not looked at).  The bits of the separate calls;
   * one host wait.  *done = PETSC_FALSE and nothing touched for vectors of another type, unequal local sizes, nv < 1 or nv > 32,
   * host-staged vectors, or a z or d that is w or one of the V_j.  On several ranks the sums are all-reduced on the device. */
  PetscErrorCode (*fgmres_orthog_normalize_pc)(Vec w, PetscInt nv, const Vec V[], Vec d, PetscBool identity, Vec z, PetscScalar *dots, PetscReal *nrm,
                                               PetscBool *done);
} VecFgmresFusedOps;
typedef const VecFgmresFusedOps *(*VecFgmresFusedOpsGetFn)(void);
typedef PetscErrorCode (*MatMultTDotBeginFn)(Mat A, Vec x, Vec y, PetscBool *ok);
typedef PetscErrorCode (*MatMultDiagonalScaleFn)(Mat A, Vec d, Vec x, Vec y, PetscBool *ok);

#endif
