/*
 * petscmini.h -- public interface of the HARNESS library (libpetscharness.so): a stand-in for the slice of PETSc's
 * object model the Krylov hot path runs through, for boxes where no PETSc exists (the GPU test box; the reference
 * cannot be built here).  It mirrors, name for name and argument for argument, erdc/petsc-dev 3.3.0-dev's
 * include/petscsys.h, petscvec.h, petscmat.h, petscpc.h, petscksp.h for the calls of
 * src/ksp/ksp/examples/tutorials/ex2.c-style programs: type registries keyed by strings, per-object function tables,
 * composed functions, options database, KSPSolve_CG/GMRES/BCGS, PCNONE/JACOBI/BJACOBI drivers.  It contains NO
 * device code and knows no HIPMI355X name: the Vec/Mat implementations come from the plugin
 * (include/petschipmi355x.h, libpetschipmi355x.so), which registers them here exactly as it registers them with a
 * real PETSc.  Inside a PETSc tree this header and this library are not used at all.
 *
 * Names: the communicator type is PetscComm (own name), so that this header can be included next to <mpi.h>;
 * petscmini_mpinames.h maps MPI_Comm / MPI_Comm_rank / MPI_Comm_size onto it for example programs written against
 * PETSc's spelling.
 */
#ifndef PETSCMINI_H
#define PETSCMINI_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef int    PetscErrorCode;   /* include/petscsys.h:123 */
typedef int    PetscInt;         /* 32-bit indices, include/petscsys.h:188 */
typedef double PetscScalar;      /* real double, include/petscmath.h:198 */
typedef double PetscReal;
typedef int    PetscBool;
typedef int    PetscMPIInt;
typedef double PetscLogDouble;
#define PETSC_TRUE 1
#define PETSC_FALSE 0
#define PETSC_DECIDE (-1)
#define PETSC_DETERMINE PETSC_DECIDE
#define PETSC_DEFAULT (-2)
#define PETSC_NULL 0

/* error codes: include/petscerror.h:41-84 */
#define PETSC_ERR_MEM 55
#define PETSC_ERR_SUP 56
#define PETSC_ERR_ORDER 58
#define PETSC_ERR_ARG_SIZ 60
#define PETSC_ERR_ARG_IDN 61
#define PETSC_ERR_ARG_WRONG 62
#define PETSC_ERR_ARG_OUTOFRANGE 63
#define PETSC_ERR_ARG_CORRUPT 64
#define PETSC_ERR_ARG_NOTSAMETYPE 69
#define PETSC_ERR_FP 72
#define PETSC_ERR_ARG_WRONGSTATE 73
#define PETSC_ERR_ARG_INCOMP 75
#define PETSC_ERR_LIB 76
#define PETSC_ERR_USER 83
#define PETSC_ERR_PLIB 77
#define PETSC_ERR_ARG_NULL 85
#define PETSC_ERR_ARG_UNKNOWN_TYPE 86
#define PETSC_ERR_ARG_TYPENOTSET 89
#define PETSC_ERR_NOT_CONVERGED 91

typedef enum { NOT_SET_VALUES, INSERT_VALUES, ADD_VALUES, MAX_VALUES } InsertMode;          /* petscsys.h */
typedef enum { SCATTER_FORWARD = 0, SCATTER_REVERSE = 1 } ScatterMode;                         /* petscvec.h:42 */
typedef enum { NORM_1 = 0, NORM_2 = 1, NORM_FROBENIUS = 2, NORM_INFINITY = 3, NORM_1_AND_2 = 4 } NormType; /* petscvec.h:155 */
typedef enum { MAT_FLUSH_ASSEMBLY = 1, MAT_FINAL_ASSEMBLY = 0 } MatAssemblyType;               /* petscmat.h:347 */
typedef enum { MAT_DO_NOT_COPY_VALUES, MAT_COPY_VALUES, MAT_SHARE_NONZERO_PATTERN } MatDuplicateOption;   /* petscmat.h:440 */
typedef enum { MAT_INITIAL_MATRIX, MAT_REUSE_MATRIX } MatReuse;   /* petscmat.h: a product builds its result, or fills the one an earlier call built */
typedef enum { DIFFERENT_NONZERO_PATTERN, SUBSET_NONZERO_PATTERN, SAME_NONZERO_PATTERN, SAME_PRECONDITIONER } MatStructure;
/* MatSetOption (include/petscmat.h, the list of 3.3 in its order).  The HIPMI355X types act on MAT_KEEP_NONZERO_PATTERN (MatZeroRows);
 * the others are accepted and have no effect here */
typedef enum { MAT_ROW_ORIENTED, MAT_NEW_NONZERO_LOCATIONS, MAT_SYMMETRIC, MAT_STRUCTURALLY_SYMMETRIC, MAT_NEW_DIAGONALS,
               MAT_IGNORE_OFF_PROC_ENTRIES, MAT_NEW_NONZERO_LOCATION_ERR, MAT_NEW_NONZERO_ALLOCATION_ERR, MAT_USE_HASH_TABLE,
               MAT_KEEP_NONZERO_PATTERN, MAT_IGNORE_ZERO_ENTRIES, MAT_USE_INODES, MAT_HERMITIAN, MAT_SYMMETRY_ETERNAL,
               MAT_CHECK_COMPRESSED_ROW, MAT_IGNORE_LOWER_TRIANGULAR, MAT_ERROR_LOWER_TRIANGULAR, MAT_GETROW_UPPERTRIANGULAR,
               MAT_UNUSED_NONZERO_LOCATION_ERR, MAT_SPD, MAT_NO_OFF_PROC_ENTRIES, MAT_NO_OFF_PROC_ZERO_ROWS, NUM_MAT_OPTIONS } MatOption;
/* MatSOR (include/petscmat.h MatSORType, the reference's values): which sweeps run, on the whole matrix or on each process's diagonal
 * block (LOCAL); ZERO_INITIAL_GUESS: x is not read; EISENSTAT, APPLY_UPPER, APPLY_LOWER are refused by the HIPMI355X types */
typedef enum { SOR_FORWARD_SWEEP = 1, SOR_BACKWARD_SWEEP = 2, SOR_SYMMETRIC_SWEEP = 3, SOR_LOCAL_FORWARD_SWEEP = 4, SOR_LOCAL_BACKWARD_SWEEP = 8,
               SOR_LOCAL_SYMMETRIC_SWEEP = 12, SOR_ZERO_INITIAL_GUESS = 16, SOR_EISENSTAT = 32, SOR_APPLY_UPPER = 64, SOR_APPLY_LOWER = 128 } MatSORType;
/* matrix factorisation interface (include/petscmat.h:100-131,1042-1088): the factored matrix is a Mat of its own, obtained from the
 * operator with MatGetFactor, filled by a symbolic and a numeric call, applied with MatSolve */
typedef enum { MAT_FACTOR_NONE, MAT_FACTOR_LU, MAT_FACTOR_CHOLESKY, MAT_FACTOR_ILU, MAT_FACTOR_ICC, MAT_FACTOR_ILUDT } MatFactorType;
typedef enum { MAT_SHIFT_NONE, MAT_SHIFT_NONZERO, MAT_SHIFT_POSITIVE_DEFINITE, MAT_SHIFT_INBLOCKS } MatFactorShiftType;
typedef struct {
  PetscReal diagonal_fill, usedt, dt, dtcol, dtcount;
  PetscReal fill;            /* expected fill */
  PetscReal levels;          /* ICC/ILU(levels) */
  PetscReal pivotinblocks;
  PetscReal zeropivot;       /* pivot is called zero if less than this */
  PetscReal shifttype;       /* MatFactorShiftType, stored as a real (petscmat.h:1072) */
  PetscReal shiftamount;
} MatFactorInfo;
#define MatSolverPackage char *
#define MATSOLVERPETSC "petsc"
typedef enum { PC_SIDE_DEFAULT = -1, PC_LEFT, PC_RIGHT, PC_SYMMETRIC } PCSide;
#define PC_SIDE_MAX 3    /* PC_SYMMETRIC + 1, petscpc.h:96 */
typedef enum { KSP_NORM_DEFAULT = -1, KSP_NORM_NONE = 0, KSP_NORM_PRECONDITIONED = 1, KSP_NORM_UNPRECONDITIONED = 2, KSP_NORM_NATURAL = 3 } KSPNormType;
#define KSP_NORM_MAX 4   /* KSP_NORM_NATURAL + 1, petscksp.h:349 */
typedef enum { KSP_GMRES_CGS_REFINE_NEVER, KSP_GMRES_CGS_REFINE_IFNEEDED, KSP_GMRES_CGS_REFINE_ALWAYS } KSPGMRESCGSRefinementType;
typedef enum { /* petscksp.h:403-430 */
  KSP_CONVERGED_RTOL_NORMAL = 1, KSP_CONVERGED_ATOL_NORMAL = 9, KSP_CONVERGED_RTOL = 2, KSP_CONVERGED_ATOL = 3,
  KSP_CONVERGED_ITS = 4, KSP_CONVERGED_HAPPY_BREAKDOWN = 8,
  KSP_DIVERGED_NULL = -2, KSP_DIVERGED_ITS = -3, KSP_DIVERGED_DTOL = -4, KSP_DIVERGED_BREAKDOWN = -5,
  KSP_DIVERGED_BREAKDOWN_BICG = -6, KSP_DIVERGED_NONSYMMETRIC = -7, KSP_DIVERGED_INDEFINITE_PC = -8,
  KSP_DIVERGED_NAN = -9, KSP_DIVERGED_INDEFINITE_MAT = -10, KSP_CONVERGED_ITERATING = 0
} KSPConvergedReason;

/* how PCApplyRichardson ended (include/petscpc.h); the values are those of the KSPConvergedReason of the same name */
typedef enum { PCRICHARDSON_CONVERGED_RTOL = 2, PCRICHARDSON_CONVERGED_ATOL = 3, PCRICHARDSON_CONVERGED_ITS = 4, PCRICHARDSON_DIVERGED_DTOL = -4 } PCRichardsonConvergedReason;

typedef struct _p_PetscComm  *PetscComm;    /* stands in for PetscComm (own name: coexists with <mpi.h>) */
typedef struct _p_Vec        *Vec;
typedef struct _p_Mat        *Mat;
typedef struct _p_VecScatter *VecScatter;
typedef struct _p_KSP        *KSP;
typedef struct _p_PC         *PC;
typedef struct _p_PetscViewer *PetscViewer;
typedef struct _p_MatNullSpace *MatNullSpace;
typedef struct _p_IS         *IS;           /* index set: only ever NULL here (the natural ordering) */
typedef enum { FILE_MODE_READ, FILE_MODE_WRITE } PetscFileMode;
typedef const char *VecType;
typedef const char *MatType;
typedef const char *KSPType;
typedef const char *PCType;

/* the reference's type names (include/petscvec.h:75-80, petscmat.h:33-62); WHICH implementation answers to them is up to
 * whoever registered it (VecRegister / MatRegister): this library has none of its own */
#define VECSEQ      "seq"
#define VECMPI      "mpi"
#define VECSTANDARD "standard"
#define MATSEQAIJ   "seqaij"
#define MATMPIAIJ   "mpiaij"
#define MATAIJ      "aij"
#define MATSEQBAIJ  "seqbaij"
#define KSPCG      "cg"
#define KSPGMRES   "gmres"
#define KSPBCGS    "bcgs"
#define KSPPREONLY "preonly"
#define KSPPIPECG  "pipecg"    /* pipelined CG (src/ksp/ksp/impls/cg/pipecg/pipecg.c), SURVEY 8f.4 */
#define KSPGROPPCG "groppcg"   /* Gropp's overlapped CG (src/ksp/ksp/impls/cg/groppcg/groppcg.c), SURVEY 8f.4 */
#define KSPCHEBYCHEV  "chebychev"    /* Chebyshev iteration with given eigenvalue bounds (src/ksp/ksp/impls/cheby/cheby.c) */
#define KSPRICHARDSON "richardson"   /* (damped) Richardson iteration (src/ksp/ksp/impls/rich/rich.c) */
#define KSPMINRES  "minres"    /* minimum residual method for symmetric indefinite operators (src/ksp/ksp/impls/minres/minres.c) */
#define KSPTFQMR   "tfqmr"     /* transpose-free QMR for nonsymmetric operators (src/ksp/ksp/impls/tfqmr/tfqmr.c) */
#define KSPCGS     "cgs"       /* conjugate gradient squared (src/ksp/ksp/impls/cgs/cgs.c) */
#define KSPLSQR    "lsqr"      /* least squares for rectangular operators: A v and A^T u per iteration (src/ksp/ksp/impls/lsqr/lsqr.c) */
#define KSPBICG    "bicg"      /* biconjugate gradients: A^T p and B^T r per iteration (src/ksp/ksp/impls/bicg/bicg.c) */
#define KSPFGMRES  "fgmres"    /* flexible GMRES: right preconditioning with a preconditioner that may change from step to step (src/ksp/ksp/impls/gmres/fgmres/fgmres.c) */
#define PCNONE     "none"
#define PCJACOBI   "jacobi"
#define PCBJACOBI  "bjacobi"
#define PCPBJACOBI "pbjacobi"  /* point-block Jacobi (src/ksp/pc/impls/pbjacobi/pbjacobi.c), SURVEY 8f.4 */
#define PCILU      "ilu"       /* ILU(0), natural ordering, sequential AIJ */
#define PCICC      "icc"       /* ICC(0), natural ordering, sequential AIJ */
#define PCSOR      "sor"       /* SOR / SSOR through the operator's MatSOR (src/ksp/pc/impls/sor/sor.c) */
#define PCKSP      "ksp"       /* a Krylov solver as the preconditioner: every application is a KSPSolve of the inner KSP (src/ksp/pc/impls/ksp/pcksp.c) */
#define PCGAMG     "gamg"      /* smoothed aggregation: builds the hierarchy of a PCMG from the operator (gamg.c) */
#define PCMG       "mg"        /* multigrid cycles over level KSPs, grid transfers given as matrices (src/ksp/pc/impls/mg/mg.c) */

/* ---- Sys ----------------------------------------------------------------------------------- */
extern PetscComm PETSC_COMM_SELF, PETSC_COMM_WORLD;
/* registers the harness's own KSP and PC types (idempotent; every Create calls it) */
PetscErrorCode PetscMiniInitialize(void);
/* last error message (PetscError traceback text, src/sys/error/err.c) */
const char    *PetscGetLastErrorMessage(void);
/* Host collectives supplied by the launcher (torch.distributed / MPI): the reference uses MPI for these */
typedef int (*PetscCommAllgatherFn)(void *ctx, const void *sendbuf, int nbytes, void *recvbuf);
typedef int (*PetscCommAllreduceFn)(void *ctx, void *buf, int count, int is_double, int op /*0 sum,1 max,2 min*/);
typedef int (*PetscCommBarrierFn)(void *ctx);
PetscErrorCode PetscCommCreate(int rank, int size, void *ctx, PetscCommAllgatherFn, PetscCommAllreduceFn, PetscCommBarrierFn, PetscComm *comm);
/* optional host-staged neighbour exchange (used only when no RCCL communicator is attached, e.g. several ranks
 * sharing one GPU): post every receive and send of one halo exchange, return when all have completed */
typedef int (*PetscCommExchangeFn)(void *ctx, int nsend, const int *speers, void *const *sbufs, const int *sbytes,
                                   int nrecv, const int *rpeers, void *const *rbufs, const int *rbytes);
PetscErrorCode PetscCommSetExchange(PetscComm comm, PetscCommExchangeFn fn);
PetscErrorCode PetscCommSetWorld(PetscComm comm);
/* two opaque slots a Vec/Mat plugin may hang communicator-wide data on (the HIPMI355X plugin: its RCCL communicators) */
PetscErrorCode PetscCommSetPluginData(PetscComm comm, int slot, void *data);
PetscErrorCode PetscCommGetPluginData(PetscComm comm, int slot, void **data);
PetscErrorCode PetscCommDestroy(PetscComm *comm);
PetscErrorCode PetscCommRank(PetscComm comm, PetscMPIInt *rank);
PetscErrorCode PetscCommSize(PetscComm comm, PetscMPIInt *size);
/* flop counter fed by PetscLogFlops with the reference's formulas (include/petsclog.h:294) */
PetscErrorCode PetscGetFlops(PetscLogDouble *flops);
PetscErrorCode PetscSplitOwnership(PetscComm comm, PetscInt *n, PetscInt *N);   /* src/sys/utils/psplit.c */
/* options database subset (src/sys/objects/options.c): "-ksp_type cg -pc_type jacobi ..." */
PetscErrorCode PetscOptionsInsertString(const char *str);
PetscErrorCode PetscOptionsSetValue(const char *name, const char *value);
PetscErrorCode PetscOptionsClear(void);

/* ---- registries and composed functions: what a Vec/Mat/PC plugin binds to ------------------------------------------
 * VecRegister (src/vec/vec/interface/vecreg.c:100), MatRegister (src/mat/interface/matreg.c:137), PCRegister
 * (src/ksp/pc/interface/pcregis.c), PetscObjectComposeFunction / PetscObjectQueryFunction (src/sys/objects/inherit.c):
 * type-specific methods such as "MatSeqAIJSetPreallocation_C" are looked up by name on the object. */
typedef struct _p_PetscObject *PetscObject;
typedef void (*PetscVoidFunction)(void);
/* signatures of the reference (petscvec.h:314, petscmat.h:176, petscpc.h, petscksp.h, petscsys.h:1360): `path` and the
 * function's own name serve dynamic loading there and are ignored here */
PetscErrorCode VecRegister(const char sname[], const char path[], const char name[], PetscErrorCode (*create)(Vec));
PetscErrorCode MatRegister(const char sname[], const char path[], const char name[], PetscErrorCode (*create)(Mat));
PetscErrorCode PCRegister(const char sname[], const char path[], const char name[], PetscErrorCode (*create)(PC));
PetscErrorCode KSPRegister(const char sname[], const char path[], const char name[], PetscErrorCode (*create)(KSP));
PetscErrorCode PetscObjectComposeFunction(PetscObject obj, const char name[], const char fname[], PetscVoidFunction fn);
PetscErrorCode PetscObjectQueryFunction(PetscObject obj, const char name[], PetscVoidFunction *fn);
PetscErrorCode PetscObjectChangeTypeName(PetscObject obj, const char type_name[]);

/* ---- Vec (include/petscvec.h; wrappers src/vec/vec/interface/rvector.c) ---------------------- */
PetscErrorCode VecCreate(PetscComm comm, Vec *vec);
PetscErrorCode VecSetSizes(Vec v, PetscInt n, PetscInt N);
PetscErrorCode VecSetType(Vec v, VecType type);
PetscErrorCode VecSetFromOptions(Vec v);                       /* -vec_type */
PetscErrorCode VecGetType(Vec v, VecType *type);
PetscErrorCode VecDuplicate(Vec v, Vec *newv);
PetscErrorCode VecDuplicateVecs(Vec v, PetscInt m, Vec **V);
PetscErrorCode VecDestroyVecs(PetscInt m, Vec **V);
PetscErrorCode VecDestroy(Vec *v);
PetscErrorCode VecGetSize(Vec v, PetscInt *N);
PetscErrorCode VecGetLocalSize(Vec v, PetscInt *n);
PetscErrorCode VecGetOwnershipRange(Vec v, PetscInt *low, PetscInt *high);
PetscErrorCode VecSetValues(Vec v, PetscInt ni, const PetscInt ix[], const PetscScalar y[], InsertMode mode);
PetscErrorCode VecAssemblyBegin(Vec v);
PetscErrorCode VecAssemblyEnd(Vec v);
PetscErrorCode VecGetArray(Vec v, PetscScalar **a);            /* host pointer; syncs device -> host */
PetscErrorCode VecRestoreArray(Vec v, PetscScalar **a);        /* marks host copy newer */
PetscErrorCode VecGetArrayRead(Vec v, const PetscScalar **a);
PetscErrorCode VecRestoreArrayRead(Vec v, const PetscScalar **a);
PetscErrorCode VecPlaceArray(Vec v, const PetscScalar *a);
PetscErrorCode VecResetArray(Vec v);
PetscErrorCode VecReplaceArray(Vec v, const PetscScalar *a);   /* rvector.c:1610: the vector takes ownership of a (allocated with PetscMalloc) */
PetscErrorCode VecSet(Vec x, PetscScalar alpha);
PetscErrorCode VecCopy(Vec x, Vec y);
PetscErrorCode VecSwap(Vec x, Vec y);
PetscErrorCode VecScale(Vec x, PetscScalar alpha);
PetscErrorCode VecAXPY(Vec y, PetscScalar alpha, Vec x);
PetscErrorCode VecAYPX(Vec y, PetscScalar alpha, Vec x);
PetscErrorCode VecAXPBY(Vec y, PetscScalar alpha, PetscScalar beta, Vec x);
PetscErrorCode VecWAXPY(Vec w, PetscScalar alpha, Vec x, Vec y);
PetscErrorCode VecAXPBYPCZ(Vec z, PetscScalar alpha, PetscScalar beta, PetscScalar gamma, Vec x, Vec y);
PetscErrorCode VecMAXPY(Vec y, PetscInt nv, const PetscScalar alpha[], Vec x[]);
PetscErrorCode VecPointwiseMult(Vec w, Vec x, Vec y);
PetscErrorCode VecPointwiseDivide(Vec w, Vec x, Vec y);
PetscErrorCode VecReciprocal(Vec x);
PetscErrorCode VecDot(Vec x, Vec y, PetscScalar *val);
PetscErrorCode VecTDot(Vec x, Vec y, PetscScalar *val);
PetscErrorCode VecMDot(Vec x, PetscInt nv, const Vec y[], PetscScalar val[]);
PetscErrorCode VecMTDot(Vec x, PetscInt nv, const Vec y[], PetscScalar val[]);
PetscErrorCode VecNorm(Vec x, NormType type, PetscReal *val);
PetscErrorCode VecNormalize(Vec x, PetscReal *val);
PetscErrorCode VecDotNorm2(Vec s, Vec t, PetscScalar *dp, PetscReal *nm);
PetscErrorCode VecSum(Vec v, PetscScalar *sum);                /* vinv.c VecSum */
PetscErrorCode VecShift(Vec v, PetscScalar shift);             /* rvector.c VecShift: v[i] += shift */
PetscErrorCode VecMax(Vec x, PetscInt *p, PetscReal *val);     /* rvector.c: the first location of the maximum (p may be NULL); no entries: PETSC_MIN_REAL, -1 */
PetscErrorCode VecMin(Vec x, PetscInt *p, PetscReal *val);
/* split-phase reductions (src/vec/vec/utils/comb.c:402-721) */
PetscErrorCode VecDotBegin(Vec x, Vec y, PetscScalar *result);
PetscErrorCode VecDotEnd(Vec x, Vec y, PetscScalar *result);
PetscErrorCode VecNormBegin(Vec x, NormType type, PetscReal *result);
PetscErrorCode VecNormEnd(Vec x, NormType type, PetscReal *result);
PetscErrorCode PetscCommSplitReductionBegin(PetscComm comm);
/* ---- Mat (include/petscmat.h; wrappers src/mat/interface/matrix.c) --------------------------- */
PetscErrorCode MatCreate(PetscComm comm, Mat *A);
PetscErrorCode MatSetSizes(Mat A, PetscInt m, PetscInt n, PetscInt M, PetscInt N);
PetscErrorCode MatSetType(Mat A, MatType type);
PetscErrorCode MatSetFromOptions(Mat A);                      /* -mat_type, then the type's own options (ops->setfromoptions, gcreate.c:167-205) */
PetscErrorCode MatDuplicate(Mat A, MatDuplicateOption op, Mat *B);   /* matrix.c:4023 */
PetscErrorCode MatGetType(Mat A, MatType *type);
PetscErrorCode MatSetUp(Mat A);
PetscErrorCode MatSeqAIJSetPreallocation(Mat A, PetscInt nz, const PetscInt nnz[]);
PetscErrorCode MatMPIAIJSetPreallocation(Mat A, PetscInt d_nz, const PetscInt d_nnz[], PetscInt o_nz, const PetscInt o_nnz[]);
PetscErrorCode MatSeqAIJSetPreallocationCSR(Mat A, const PetscInt i[], const PetscInt j[], const PetscScalar v[]);   /* aij.c:3795 */
PetscErrorCode MatMPIAIJSetPreallocationCSR(Mat A, const PetscInt i[], const PetscInt j[], const PetscScalar v[]);   /* mpiaij.c:3960 */
PetscErrorCode MatGetDiagonalBlock(Mat A, Mat *a);
PetscErrorCode MatSetValues(Mat A, PetscInt m, const PetscInt idxm[], PetscInt n, const PetscInt idxn[], const PetscScalar v[], InsertMode addv);
PetscErrorCode MatSetValuesBatch(Mat A, PetscInt nb, PetscInt bs, PetscInt rows[], const PetscScalar v[]);   /* matrix.c:1698; device-side value assembly when the pattern is unchanged */
PetscErrorCode MatAssemblyBegin(Mat A, MatAssemblyType type);
PetscErrorCode MatAssemblyEnd(Mat A, MatAssemblyType type);
/* bulk creation from CSR (MatCreateSeqAIJWithArrays src/mat/impls/aij/seq/aij.c, MatCreateMPIAIJWithArrays
 * src/mat/impls/aij/mpi/mpiaij.c; i/j/a are copied; j holds global column indices, ascending per row) */
PetscErrorCode MatCreateSeqAIJWithArrays(PetscComm comm, PetscInt m, PetscInt n, PetscInt i[], PetscInt j[], PetscScalar a[], Mat *mat);
PetscErrorCode MatCreateMPIAIJWithArrays(PetscComm comm, PetscInt m, PetscInt n, PetscInt M, PetscInt N, const PetscInt i[], const PetscInt j[], const PetscScalar a[], Mat *mat);
PetscErrorCode MatCreateSeqBAIJWithArrays(PetscComm comm, PetscInt bs, PetscInt m, PetscInt n, PetscInt i[], PetscInt j[], PetscScalar a[], Mat *mat);
PetscErrorCode MatDestroy(Mat *A);
PetscErrorCode MatGetSize(Mat A, PetscInt *M, PetscInt *N);
PetscErrorCode MatGetLocalSize(Mat A, PetscInt *m, PetscInt *n);
PetscErrorCode MatGetOwnershipRange(Mat A, PetscInt *rstart, PetscInt *rend);
PetscErrorCode MatGetVecs(Mat A, Vec *right, Vec *left);
PetscErrorCode MatMult(Mat A, Vec x, Vec y);
PetscErrorCode MatMultAdd(Mat A, Vec x, Vec y, Vec z);
PetscErrorCode MatMultTranspose(Mat A, Vec x, Vec y);
PetscErrorCode MatMultTransposeAdd(Mat A, Vec x, Vec y, Vec z);
PetscErrorCode MatGetDiagonal(Mat A, Vec d);
PetscErrorCode MatScale(Mat A, PetscScalar a);
PetscErrorCode MatZeroEntries(Mat A);
/* value updates of an assembled matrix (src/mat/utils/axpy.c, matrix.c MatCopy): on the device copy when the pattern allows */
PetscErrorCode MatShift(Mat Y, PetscScalar a);                           /* Y += a I */
PetscErrorCode MatAXPY(Mat Y, PetscScalar a, Mat X, MatStructure str);   /* Y += a X; X's pattern must lie inside Y's */
PetscErrorCode MatAYPX(Mat Y, PetscScalar a, Mat X, MatStructure str);   /* Y = a Y + X */
PetscErrorCode MatCopy(Mat A, Mat B, MatStructure str);                  /* B <- A */
/* Dirichlet rows (matrix.c MatZeroRows / MatZeroRowsColumns; aij.c, mpiaij.c): the listed rows -- local indices on a sequential matrix,
 * global ones owned by any rank on a parallel one, where the call is collective -- are zeroed and get diag on the diagonal (diag != 0);
 * MatZeroRowsColumns zeroes the listed columns too and keeps a symmetric operator symmetric.  x and b, both or neither:
 * b[r] = diag * x[r] on the listed rows, and (columns) b[i] -= a_ij x[j] for every eliminated entry.  MatZeroRows removes the rows' entries
 * from the nonzero pattern unless MatSetOption(A, MAT_KEEP_NONZERO_PATTERN, PETSC_TRUE) was given; MatZeroRowsColumns always keeps it */
PetscErrorCode MatZeroRows(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec x, Vec b);
PetscErrorCode MatZeroRowsColumns(Mat A, PetscInt n, const PetscInt rows[], PetscScalar diag, Vec x, Vec b);
PetscErrorCode MatSetOption(Mat A, MatOption op, PetscBool flg);
/* its * lits sweeps of (S)SOR on A x = b with relaxation omega and diagonal shift fshift (matrix.c MatSOR; MatSOR_SeqAIJ aij.c:1463,
 * MatSOR_MPIAIJ mpiaij.c: local sweeps only, its outer steps of lits local sweeps each).  b and x are different vectors, its, lits > 0 */
PetscErrorCode MatSOR(Mat A, Vec b, PetscReal omega, MatSORType flag, PetscReal fshift, PetscInt its, PetscInt lits, Vec x);
PetscErrorCode MatSetOptionsPrefix(Mat A, const char prefix[]);
/* sparse matrix products (matrix.c MatMatMult, MatTranspose, MatPtAP; MatMatMult_SeqAIJ_SeqAIJ matmatmult.c, MatPtAP_SeqAIJ_SeqAIJ
 * matptap.c): dispatch on A's type; operands of different types PETSC_ERR_SUP, inner dimensions that do not match PETSC_ERR_ARG_SIZ.
 * MAT_INITIAL_MATRIX builds *C (symbolic and numeric phase); MAT_REUSE_MATRIX fills the *C an earlier call built from the same
 * operands with unchanged patterns (else PETSC_ERR_ARG_WRONG).  fill, the expected nnz(C) / (nnz(A) + nnz(B)), is a hint the
 * HIPMI355X types do not need (PETSC_DEFAULT).  MatPtAP is MatMatMult(MatTranspose(P), MatMatMult(A, P)) with exactly those bits. */
PetscErrorCode MatMatMult(Mat A, Mat B, MatReuse scall, PetscReal fill, Mat *C);           /* C = A B */
PetscErrorCode MatMatMultSymbolic(Mat A, Mat B, PetscReal fill, Mat *C);                   /* C's pattern, values zero */
PetscErrorCode MatMatMultNumeric(Mat A, Mat B, Mat C);                                     /* the values of a C from MatMatMultSymbolic / MatMatMult */
PetscErrorCode MatTranspose(Mat A, MatReuse reuse, Mat *B);                                /* B = A^T, out of place */
PetscErrorCode MatPtAP(Mat A, Mat P, MatReuse scall, PetscReal fill, Mat *C);              /* C = P^T A P */
/* matrix.c:3937-4010 (MatGetFactor looks "MatGetFactor_<package>_C" up on the operator), 2766-3144 (symbolic / numeric), 3196 (MatSolve) */
PetscErrorCode MatFactorInfoInitialize(MatFactorInfo *info);
PetscErrorCode MatGetFactor(Mat mat, const MatSolverPackage type, MatFactorType ftype, Mat *f);
PetscErrorCode MatGetFactorAvailable(Mat mat, const MatSolverPackage type, MatFactorType ftype, PetscBool *flg);
PetscErrorCode MatILUFactorSymbolic(Mat fact, Mat mat, IS row, IS col, const MatFactorInfo *info);
PetscErrorCode MatLUFactorNumeric(Mat fact, Mat mat, const MatFactorInfo *info);
PetscErrorCode MatICCFactorSymbolic(Mat fact, Mat mat, IS perm, const MatFactorInfo *info);
PetscErrorCode MatCholeskyFactorNumeric(Mat fact, Mat mat, const MatFactorInfo *info);
PetscErrorCode MatSolve(Mat mat, Vec b, Vec x);
PetscErrorCode MatSolveTranspose(Mat mat, Vec b, Vec x);   /* matrix.c MatSolveTranspose: x = (factor)^-T b; PETSC_ERR_SUP without ops->solvetranspose */
PetscErrorCode MatDiagonalScale(Mat A, Vec l, Vec r);   /* A <- diag(l) A diag(r); l or r may be NULL (aij.c:2055, mpiaij.c:2183) */
/* queries about the stored values (matrix.c; MatNorm_SeqAIJ, MatGetRowMaxAbs_SeqAIJ, MatGetRowMax_SeqAIJ, MatGetRowMin_SeqAIJ,
 * MatGetColumnNorms_SeqAIJ aij.c).  MatNorm: NORM_1 (largest column sum of |a|), NORM_FROBENIUS, NORM_INFINITY (largest row sum);
 * NORM_2 is PETSC_ERR_SUP.  The row extrema go to v (the matrix's row layout), the column each one was found at to idx (a host array
 * of the local rows, or NULL): the first of equal entries, NaNs never chosen over a number; MatGetRowMax / MatGetRowMin let a row
 * that stores fewer entries than the matrix has columns compete with one implicit 0.0 at its smallest missing column.
 * MatGetRowSum is MatMult with a vector of ones.  MatGetColumnNorms: NORM_1, NORM_2 or NORM_INFINITY of every column into norms[N]. */
PetscErrorCode MatNorm(Mat A, NormType type, PetscReal *nrm);
/* aggregates for smoothed aggregation: agg[i] in [0, *nagg) for every row of a square matrix, by the strength mask
 * |a_ij| > threshold sqrt(|a_ii| |a_jj|) and a distance-2 maximal independent set (the type's "MatCoarsenAggregate_C"; a type
 * without one: PETSC_ERR_SUP) */
PetscErrorCode MatCoarsenAggregate(Mat A, PetscReal threshold, PetscInt *nagg, PetscInt agg[]);
PetscErrorCode MatGetRowMaxAbs(Mat A, Vec v, PetscInt idx[]);
PetscErrorCode MatGetRowMax(Mat A, Vec v, PetscInt idx[]);
PetscErrorCode MatGetRowMin(Mat A, Vec v, PetscInt idx[]);
PetscErrorCode MatGetRowSum(Mat A, Vec v);
PetscErrorCode MatGetColumnNorms(Mat A, NormType type, PetscReal norms[]);
/* null spaces of singular operators (src/mat/interface/matnull.c): the constant vector (has_cnst) and / or n orthonormal vectors, which
 * the null space keeps references to.  MatNullSpaceRemove: the constant first (VecSum, sum / (-N), VecShift), then the vectors (VecMDot,
 * VecMAXPY), then the function set with MatNullSpaceSetFunction; out != NULL: the result goes to an internal copy returned in *out */
/* grid transfers and the residual (matrix.c).  MatRestrict / MatInterpolate: y = A x when A's rows match y, y = A^T x when its columns do
 * (one matrix serves both directions); MatInterpolateAdd: w = y + (A or A^T) x, w may be y; sizes that fit neither way PETSC_ERR_ARG_SIZ.
 * MatResidual: r = b - A x by the type's own "MatResidual_C" (Mat, Vec b, Vec x, Vec r) if it composed one, else MatMult and
 * VecAYPX(r, -1, b); r must be neither b nor x. */
PetscErrorCode MatRestrict(Mat A, Vec x, Vec y);
PetscErrorCode MatInterpolate(Mat A, Vec x, Vec y);
PetscErrorCode MatInterpolateAdd(Mat A, Vec x, Vec y, Vec w);
PetscErrorCode MatResidual(Mat A, Vec b, Vec x, Vec r);
PetscErrorCode MatNullSpaceCreate(PetscComm comm, PetscBool has_cnst, PetscInt n, const Vec vecs[], MatNullSpace *SP);
PetscErrorCode MatNullSpaceDestroy(MatNullSpace *sp);
PetscErrorCode MatNullSpaceSetFunction(MatNullSpace sp, PetscErrorCode (*rem)(MatNullSpace, Vec, void *), void *ctx);
PetscErrorCode MatNullSpaceRemove(MatNullSpace sp, Vec vec, Vec *out);
PetscErrorCode MatNullSpaceTest(MatNullSpace sp, Mat mat, PetscBool *isNull);
/* ---- binary IO (PETSc binary format, big-endian; src/mat/impls/aij/seq/aij.c:4093-4157, src/vec/vec/utils/vecio.c) ---- */
PetscErrorCode PetscViewerBinaryOpen(PetscComm comm, const char name[], PetscFileMode mode, PetscViewer *viewer);
PetscErrorCode PetscViewerDestroy(PetscViewer *viewer);
PetscErrorCode MatLoad(Mat A, PetscViewer viewer);     /* AIJ types, sequential and parallel (each rank reads its rows) */
PetscErrorCode MatView(Mat A, PetscViewer viewer);     /* sequential AIJ */
PetscErrorCode VecLoad(Vec v, PetscViewer viewer);
PetscErrorCode VecView(Vec v, PetscViewer viewer);     /* sequential */

/* example-driver support: bulk assembly of the 3-D 7-point Poisson operator (rows [rstart,rend), global
 * ascending columns); the 3-D analogue of src/ksp/ksp/examples/tutorials/ex2.c:96-103 */
PetscErrorCode PetscMiniGenPoisson7(PetscInt nx, PetscInt ny, PetscInt nz, long rstart, long rend, PetscInt *ai, PetscInt *aj, PetscScalar *aa, long *nnz_out);

/* ---- PC (include/petscpc.h) ------------------------------------------------------------------ */
PetscErrorCode PCCreate(PetscComm comm, PC *pc);
PetscErrorCode PCSetType(PC pc, PCType type);
PetscErrorCode PCGetType(PC pc, PCType *type);
PetscErrorCode PCSetOperators(PC pc, Mat Amat, Mat Pmat, MatStructure flag);
PetscErrorCode PCGetOperators(PC pc, Mat *Amat, Mat *Pmat, MatStructure *flag);
PetscErrorCode PCSetUp(PC pc);
PetscErrorCode PCSetUpOnBlocks(PC pc);
PetscErrorCode PCApply(PC pc, Vec x, Vec y);
PetscErrorCode PCApplyTranspose(PC pc, Vec x, Vec y);           /* precon.c PCApplyTranspose: y = B^T x; PETSC_ERR_SUP for a type without ops->applytranspose */
PetscErrorCode PCApplyTransposeExists(PC pc, PetscBool *flg);
/* precon.c PCApplyRichardson: `its` steps of Richardson's iteration with this preconditioner on A y = b done by the PC itself (PCSOR:
 * ONE MatSOR call of its sweeps); w: a work vector; PETSC_ERR_SUP when the PC has no such method (KSPRICHARDSON asks first) */
PetscErrorCode PCApplyRichardson(PC pc, Vec b, Vec y, Vec w, PetscReal rtol, PetscReal abstol, PetscReal dtol, PetscInt its, PetscBool guesszero, PetscInt *outits, PCRichardsonConvergedReason *reason);
PetscErrorCode PCApplyRichardsonExists(PC pc, PetscBool *exists);
PetscErrorCode PCSetFromOptions(PC pc);
PetscErrorCode PCDestroy(PC *pc);
PetscErrorCode PCFactorSetLevels(PC pc, PetscInt levels);   /* levels of fill of a PCILU / PCICC (factor.c PCFactorSetLevels; -pc_factor_levels); a changed level after set-up has the next set-up redo the symbolic phase */
PetscErrorCode PCFactorGetMatrix(PC pc, Mat *mat);   /* the factored matrix of a PCILU / PCICC (precon.c PCFactorGetMatrix) */
PetscErrorCode PCBJacobiGetSubKSP(PC pc, PetscInt *n_local, PetscInt *first_local, KSP **ksp);
/* pcksp.c.  The inner solver of a PCKSP, created at the first call or at set-up on the PC's communicator with the options prefix
 * "<pc prefix>ksp_" (-ksp_ksp_type, -ksp_pc_type, -ksp_ksp_max_it ...); not owned by the caller.  GetTotalIterations: the inner iterations of
 * all applications so far.  Both return PETSC_ERR_ARG_WRONG for a PC of another type. */
PetscErrorCode PCKSPGetKSP(PC pc, KSP *ksp);
PetscErrorCode PCKSPGetTotalIterations(PC pc, PetscInt *n);
/* PCMG (include/petscpcmg.h; mg.c, mgfunc.c).  Level 0 is the coarsest, level n-1 the PC's own operators.  Level solvers: options prefix
 * "<pc prefix>mg_coarse_" for level 0, "<pc prefix>mg_levels_<l>_" above it; an option under "mg_levels_" reaches every smoothed level and
 * the same option under "mg_levels_<l>_" beats it.  Smoothers default to richardson + sor without a norm, one step, nonzero guess; the
 * coarse solver to preonly + the PC default.  The up smoother is the down smoother's KSP until PCMGGetSmootherUp or unequal
 * PCMGSetNumberSmoothDown / Up ask for a second one (same type, PC type and prefix).  The solvers are borrowed, not owned by the caller.
 * PCMGSetLevels: comms must be NULL; after set-up PETSC_ERR_ORDER.  PCMGSetType: PC_MG_KASKADE is PETSC_ERR_SUP.
 * PCMGSetInterpolation / SetRestriction (l >= 1): each defaults to the other; the direction is chosen from the sizes (MatRestrict).
 * PCMGSetGalerkin: A_{l-1} = MatPtAP(A_l, P_l), the PC's own matrices, rebuilt with MAT_REUSE_MATRIX at every later set-up; the transfer
 * must then be stored as the interpolation (fine x coarse).  Without it every level below the top needs KSPSetOperators on its smoother
 * (PETSC_ERR_ARG_WRONGSTATE names the level).  PCMGSetResidual: fn NULL is PCMGDefaultResidual = MatResidual; mat NULL the level's operator.
 * Options: -pc_mg_levels -pc_mg_type <multiplicative|additive|full> -pc_mg_cycle_type <v|w> -pc_mg_multiplicative_cycles -pc_mg_smoothdown
 * -pc_mg_smoothup -pc_mg_galerkin. */
typedef enum { PC_MG_MULTIPLICATIVE, PC_MG_ADDITIVE, PC_MG_FULL, PC_MG_KASKADE } PCMGType;
typedef enum { PC_MG_CYCLE_V = 1, PC_MG_CYCLE_W = 2 } PCMGCycleType;
typedef PetscErrorCode (*PCMGResidualFn)(Mat, Vec, Vec, Vec);
PetscErrorCode PCMGSetLevels(PC pc, PetscInt levels, PetscComm *comms);
PetscErrorCode PCMGGetLevels(PC pc, PetscInt *levels);
PetscErrorCode PCMGSetType(PC pc, PCMGType form);
PetscErrorCode PCMGSetCycleType(PC pc, PCMGCycleType c);
PetscErrorCode PCMGMultiplicativeSetCycles(PC pc, PetscInt n);
PetscErrorCode PCMGSetNumberSmoothDown(PC pc, PetscInt n);
PetscErrorCode PCMGSetNumberSmoothUp(PC pc, PetscInt n);
PetscErrorCode PCMGSetGalerkin(PC pc, PetscBool use);
PetscErrorCode PCMGSetInterpolation(PC pc, PetscInt l, Mat mat);
PetscErrorCode PCMGSetRestriction(PC pc, PetscInt l, Mat mat);
PetscErrorCode PCMGSetResidual(PC pc, PetscInt l, PCMGResidualFn residual, Mat mat);
PetscErrorCode PCMGDefaultResidual(Mat mat, Vec b, Vec x, Vec r);
PetscErrorCode PCMGGetSmoother(PC pc, PetscInt l, KSP *ksp);
PetscErrorCode PCMGGetSmootherDown(PC pc, PetscInt l, KSP *ksp);
PetscErrorCode PCMGGetSmootherUp(PC pc, PetscInt l, KSP *ksp);
PetscErrorCode PCMGGetCoarseSolve(PC pc, KSP *ksp);
/* PCGAMG (gamg.c; the reference's src/ksp/pc/impls/gamg/): smoothed aggregation that fills a PCMG and then is one -- cycle types, the
 * PCMG calls above and the level solvers' prefixes mg_coarse_ / mg_levels_<l>_ are PCMG's own.  Sequential AIJ operators with the
 * constant as near-null space.  Per level, from the PC's pmat: aggregates by MatCoarsenAggregate(A_l, threshold); the tentative
 * prolongator T with one entry 1/sqrt(|aggregate|) per row; with nsmooths == 1 P = T - (4 / (3 rho)) D^-1 A_l T, rho the infinity
 * norm of D^-1 A_l; A_{l+1} = MatPtAP(A_l, P).  Coarsening stops at n_l <= coarse_eq_limit, at the level cap (-pc_mg_levels), or when
 * an aggregation stalls.  Smoothers default to chebychev + jacobi, two steps, eigenvalue bounds (rho_l / 10, rho_l); the coarse level to
 * preonly + ILU with as many levels of fill as it has rows.  PCGAMGSetReuseInterpolation: a later set-up keeps aggregates and
 * prolongators and only refills the Galerkin operators.  PCGAMGGetLevelSizes: sizes[0] is the fine level; at most maxn are written. */
PetscErrorCode PCGAMGSetThreshold(PC pc, PetscReal threshold);          /* -pc_gamg_threshold, default 0 */
PetscErrorCode PCGAMGSetCoarseEqLimit(PC pc, PetscInt n);               /* -pc_gamg_coarse_eq_limit, default 50 */
PetscErrorCode PCGAMGSetNlevels(PC pc, PetscInt n);                     /* -pc_mg_levels, default 25 */
PetscErrorCode PCGAMGSetNSmooths(PC pc, PetscInt n);                    /* -pc_gamg_agg_nsmooths, 0 or 1, default 1 */
PetscErrorCode PCGAMGSetReuseInterpolation(PC pc, PetscBool reuse);     /* -pc_gamg_reuse_interpolation, default false */
PetscErrorCode PCGAMGGetLevelSizes(PC pc, PetscInt maxn, PetscInt *nlevels, PetscInt sizes[]);

/* ---- KSP (include/petscksp.h) ---------------------------------------------------------------- */
PetscErrorCode KSPCreate(PetscComm comm, KSP *ksp);
PetscErrorCode KSPSetType(KSP ksp, KSPType type);
PetscErrorCode KSPGetType(KSP ksp, KSPType *type);
PetscErrorCode KSPSetOperators(KSP ksp, Mat Amat, Mat Pmat, MatStructure flag);
PetscErrorCode KSPGetPC(KSP ksp, PC *pc);
PetscErrorCode KSPSetTolerances(KSP ksp, PetscReal rtol, PetscReal abstol, PetscReal dtol, PetscInt maxits);
PetscErrorCode KSPGetTolerances(KSP ksp, PetscReal *rtol, PetscReal *abstol, PetscReal *dtol, PetscInt *maxits);   /* any pointer may be NULL */
PetscErrorCode KSPSetInitialGuessNonzero(KSP ksp, PetscBool flg);
PetscErrorCode KSPSetNormType(KSP ksp, KSPNormType normtype);
PetscErrorCode KSPSetPCSide(KSP ksp, PCSide side);   /* -ksp_pc_side <left|right>; right: the GMRES types, and the only side of KSPFGMRES */
/* itfunc.c KSPSetNullSpace: removed from the result of every preconditioner application while the preconditioner is on the left
 * (kspimpl.h KSP_RemoveNullSpace); the KSP keeps a reference; NULL takes it away again */
PetscErrorCode KSPSetNullSpace(KSP ksp, MatNullSpace nullsp);
PetscErrorCode KSPGetNullSpace(KSP ksp, MatNullSpace *nullsp);
PetscErrorCode KSPSetOptionsPrefix(KSP ksp, const char prefix[]);
PetscErrorCode KSPSetFromOptions(KSP ksp);   /* -ksp_type -ksp_rtol -ksp_atol -ksp_max_it -ksp_gmres_restart -ksp_gmres_cgs_refinement_type -pc_type -sub_* */
PetscErrorCode KSPGMRESSetRestart(KSP ksp, PetscInt restart);
PetscErrorCode KSPGMRESSetCGSRefinementType(KSP ksp, KSPGMRESCGSRefinementType type);
/* fgmres.c.  PetscTryMethod on "KSPFGMRESSetModifyPC_C": fcn(ksp, total_its, loc_its, res_norm, ctx) runs before every preconditioner
 * application of the flexible GMRES types (total_its: iterations so far, loc_its: position in the restart cycle, res_norm: the current
 * residual norm) and may change the preconditioner; d (may be NULL) releases ctx when the routine is replaced or the KSP destroyed.
 * KSPFGMRESModifyPCNoChange, the default, does nothing.  Any other KSP type ignores the call. */
PetscErrorCode KSPFGMRESSetModifyPC(KSP ksp, PetscErrorCode (*fcn)(KSP, PetscInt, PetscInt, PetscReal, void *), void *ctx, PetscErrorCode (*d)(void *));
PetscErrorCode KSPFGMRESModifyPCNoChange(KSP ksp, PetscInt total_its, PetscInt loc_its, PetscReal res_norm, void *ctx);
/* cheby.c / rich.c: PetscTryMethod on "KSPChebychevSetEigenvalues_C" / "KSPRichardsonSetScale_C" -- a type that composed the method
 * answers, any other type ignores the call.  Options: -ksp_chebychev_eigenvalues <emin,emax>, -ksp_richardson_scale <s> */
PetscErrorCode KSPChebychevSetEigenvalues(KSP ksp, PetscReal emax, PetscReal emin);
PetscErrorCode KSPRichardsonSetScale(KSP ksp, PetscReal scale);
PetscErrorCode KSPSetUp(KSP ksp);
PetscErrorCode KSPSetUpOnBlocks(KSP ksp);
PetscErrorCode KSPSolve(KSP ksp, Vec b, Vec x);
PetscErrorCode KSPGetIterationNumber(KSP ksp, PetscInt *its);
PetscErrorCode KSPGetResidualNorm(KSP ksp, PetscReal *rnorm);
PetscErrorCode KSPGetConvergedReason(KSP ksp, KSPConvergedReason *reason);
PetscErrorCode KSPSetResidualHistory(KSP ksp, PetscReal a[], PetscInt na, PetscBool reset);
PetscErrorCode KSPGetResidualHistory(KSP ksp, PetscReal *a[], PetscInt *na);
/* the residual norms KSPMonitor would be called with (what -ksp_monitor_short prints) */
/* -ksp_monitor / -ksp_monitor_short (iterativ.c:178,484): the reference's text, on rank 0 */
PetscErrorCode KSPMonitorDefault(KSP ksp, PetscInt n, PetscReal rnorm, void *dummy);
PetscErrorCode KSPMonitorDefaultShort(KSP ksp, PetscInt n, PetscReal rnorm, void *dummy);
PetscErrorCode KSPMonitorSet(KSP ksp, PetscErrorCode (*monitor)(KSP, PetscInt, PetscReal, void *), void *mctx, PetscErrorCode (*destroy)(void **));
PetscErrorCode KSPDestroy(KSP *ksp);
/* itfunc.c KSPSetConvergenceTest: converge(ksp, it, rnorm, &reason, cctx) decides at every checkpoint; destroy (may be NULL) releases cctx
 * when the test is replaced or the KSP destroyed */
PetscErrorCode KSPSetConvergenceTest(KSP ksp, PetscErrorCode (*converge)(KSP, PetscInt, PetscReal, KSPConvergedReason *, void *), void *cctx, PetscErrorCode (*destroy)(void *));
PetscErrorCode KSPDefaultConverged(KSP ksp, PetscInt n, PetscReal rnorm, KSPConvergedReason *reason, void *ctx);
/* lsqr.c.  PetscTryMethod / PetscUseMethod on "KSPLSQRSetStandardErrorVec_C", "KSPLSQRGetStandardErrorVec_C", "KSPLSQRGetArnorm_C": the LSQR
 * types answer, any other type ignores the setter and returns NULL / zeros from the getters.
 *   SetStandardErrorVec: se (length: the columns of A) takes the running sum of (w .* w) / rho^2; the KSP takes over the caller's reference.
 *                        -ksp_lsqr_set_standard_error has KSPSetUp create the vector.
 *   GetArnorm:           the estimates ||A^T r||, ||b|| (of the start residual) and ||A||_F of the last solve; any pointer may be NULL.
 *   KSPLSQRDefaultConverged: KSPDefaultConverged, then arnorm <= abstol -> KSP_CONVERGED_ATOL_NORMAL and arnorm <= rtol * anorm * rnorm ->
 *                        KSP_CONVERGED_RTOL_NORMAL; installed with KSPSetConvergenceTest */
PetscErrorCode KSPLSQRSetStandardErrorVec(KSP ksp, Vec se);
PetscErrorCode KSPLSQRGetStandardErrorVec(KSP ksp, Vec *se);
PetscErrorCode KSPLSQRGetArnorm(KSP ksp, PetscReal *arnorm, PetscReal *rhs_norm, PetscReal *anorm);
PetscErrorCode KSPLSQRDefaultConverged(KSP ksp, PetscInt n, PetscReal rnorm, KSPConvergedReason *reason, void *ctx);

#ifdef __cplusplus
}
#endif
#endif
