"""Thin ctypes front end of the two C libraries above the kernel library -- harness/libpetscharness.so (the stand-in
PETSc object model, include/petscmini.h) and host/libpetschipmi355x.so (the HIPMI355X plugin, include/petschipmi355x.h)
-- for tests and bench.py.

No arithmetic happens here: every call goes straight to the C host library, which dispatches through
the Vec/Mat function tables to the HIP kernels.  Errors raise PetscError with the C traceback text."""
import ctypes as C

import numpy as np

from ._lib import load_host, load_harness, load_kernels

vp, i32, dbl = C.c_void_p, C.c_int, C.c_double
P = C.POINTER

# name -> argtypes; all return PetscErrorCode (int)
_SIG = {
    "PetscHIPMI355XInitialize": [i32], "PetscHIPMI355XFinalize": [], "PetscHIPMI355XRegisterAll": [],
    "PetscCommCreate": [i32, i32, vp, vp, vp, vp, P(vp)], "PetscCommSetWorld": [vp], "PetscCommSetExchange": [vp, vp], "PetscCommSetDeviceComm": [vp, vp], "PetscCommSetDeviceComms": [vp, vp, vp], "PetscCommGetDeviceTransport": [vp, P(i32), P(i32), P(i32)],
    "PetscCommDestroy": [P(vp)], "PetscGetFlops": [P(dbl)],
    "PetscOptionsInsertString": [C.c_char_p], "PetscOptionsSetValue": [C.c_char_p, C.c_char_p], "PetscOptionsClear": [],
    "VecCreate": [vp, P(vp)], "VecSetSizes": [vp, i32, i32], "VecSetType": [vp, C.c_char_p], "VecSetFromOptions": [vp],
    "VecGetType": [vp, P(C.c_char_p)], "VecDuplicate": [vp, P(vp)], "VecDestroy": [P(vp)], "VecGetSize": [vp, P(i32)],
    "VecGetLocalSize": [vp, P(i32)], "VecGetOwnershipRange": [vp, P(i32), P(i32)],
    "VecSetValues": [vp, i32, vp, vp, i32], "VecAssemblyBegin": [vp], "VecAssemblyEnd": [vp],
    "VecGetArray": [vp, P(vp)], "VecRestoreArray": [vp, P(vp)], "VecGetArrayRead": [vp, P(vp)], "VecRestoreArrayRead": [vp, P(vp)],
    "VecPlaceArray": [vp, vp], "VecResetArray": [vp], "VecReplaceArray": [vp, vp], "PetscMallocFn": [C.c_size_t, P(vp)],
    "VecHIPMI355XGetArray": [vp, P(vp)], "VecHIPMI355XRestoreArray": [vp, P(vp)], "VecHIPMI355XGetArrayRead": [vp, P(vp)],
    "VecSet": [vp, dbl], "VecCopy": [vp, vp], "VecSwap": [vp, vp], "VecScale": [vp, dbl], "VecAXPY": [vp, dbl, vp],
    "VecAYPX": [vp, dbl, vp], "VecAXPBY": [vp, dbl, dbl, vp], "VecWAXPY": [vp, dbl, vp, vp],
    "VecAXPBYPCZ": [vp, dbl, dbl, dbl, vp, vp], "VecMAXPY": [vp, i32, vp, vp], "VecPointwiseMult": [vp, vp, vp],
    "VecPointwiseDivide": [vp, vp, vp], "VecReciprocal": [vp], "VecDot": [vp, vp, P(dbl)], "VecDotBegin": [vp, vp, P(dbl)], "VecDotEnd": [vp, vp, P(dbl)], "VecNormBegin": [vp, i32, P(dbl)], "VecNormEnd": [vp, i32, P(dbl)], "PetscCommSplitReductionBegin": [vp], "VecTDot": [vp, vp, P(dbl)],
    "VecMDot": [vp, i32, vp, vp], "VecMTDot": [vp, i32, vp, vp], "VecNorm": [vp, i32, P(dbl)], "VecNormalize": [vp, P(dbl)],
    "VecDotNorm2": [vp, vp, P(dbl), P(dbl)],
    "VecSum": [vp, P(dbl)], "VecShift": [vp, dbl], "VecMax": [vp, P(i32), P(dbl)], "VecMin": [vp, P(i32), P(dbl)],
    "MatNullSpaceCreate": [vp, i32, i32, vp, P(vp)], "MatNullSpaceDestroy": [P(vp)], "MatNullSpaceSetFunction": [vp, vp, vp],
    "MatNullSpaceRemove": [vp, vp, P(vp)], "MatNullSpaceTest": [vp, vp, P(i32)], "MatNullSpaceRemoveConstantHIPMI355X": [vp, vp, vp],
    "KSPSetNullSpace": [vp, vp], "KSPGetNullSpace": [vp, P(vp)],
    "VecScatterBegin": [vp, vp, vp, i32, i32], "VecScatterEnd": [vp, vp, vp, i32, i32],
    "VecScatterGetLists": [vp, P(i32), P(vp), P(vp), P(vp), P(i32), P(vp), P(vp), P(vp), P(i32), P(vp), P(vp)],
    "MatCreate": [vp, P(vp)], "MatSetSizes": [vp, i32, i32, i32, i32], "MatSetType": [vp, C.c_char_p], "MatSetFromOptions": [vp],
    "MatGetType": [vp, P(C.c_char_p)], "MatSetUp": [vp], "MatSeqAIJSetPreallocation": [vp, i32, vp],
    "MatMPIAIJSetPreallocation": [vp, i32, vp, i32, vp], "MatSetValues": [vp, i32, vp, i32, vp, vp, i32],
    "MatAssemblyBegin": [vp, i32], "MatAssemblyEnd": [vp, i32],
    "MatCreateSeqAIJWithArrays": [vp, i32, i32, vp, vp, vp, P(vp)],
    "MatCreateMPIAIJWithArrays": [vp, i32, i32, i32, i32, vp, vp, vp, P(vp)],
    "MatCreateSeqBAIJWithArrays": [vp, i32, i32, i32, vp, vp, vp, P(vp)],
    "MatDestroy": [P(vp)], "MatGetSize": [vp, P(i32), P(i32)], "MatGetLocalSize": [vp, P(i32), P(i32)],
    "MatGetOwnershipRange": [vp, P(i32), P(i32)], "MatGetVecs": [vp, P(vp), P(vp)],
    "MatDuplicate": [vp, i32, P(vp)], "MatSetOptionsPrefix": [vp, C.c_char_p], "MatDiagonalScale": [vp, vp, vp], "MatSetValuesBatch": [vp, i32, i32, vp, vp], "MatMult": [vp, vp, vp], "MatMultAdd": [vp, vp, vp, vp], "MatMultTranspose": [vp, vp, vp],
    "MatMultTransposeAdd": [vp, vp, vp, vp], "MatGetDiagonal": [vp, vp], "MatScale": [vp, dbl], "MatZeroEntries": [vp],
    "MatShift": [vp, dbl], "MatAXPY": [vp, dbl, vp, i32], "MatAYPX": [vp, dbl, vp, i32], "MatCopy": [vp, vp, i32],
    "MatZeroRows": [vp, i32, vp, dbl, vp, vp], "MatZeroRowsColumns": [vp, i32, vp, dbl, vp, vp], "MatSetOption": [vp, i32, i32],
    "MatHIPMI355XGetZeroRowsCounts": [vp, P(i32), P(i32)],
    "MatNorm": [vp, i32, P(dbl)], "MatGetRowMaxAbs": [vp, vp, vp], "MatGetRowMax": [vp, vp, vp], "MatGetRowMin": [vp, vp, vp],
    "MatGetRowSum": [vp, vp], "MatGetColumnNorms": [vp, i32, vp],
    "MatMatMult": [vp, vp, i32, dbl, P(vp)], "MatMatMultSymbolic": [vp, vp, dbl, P(vp)], "MatMatMultNumeric": [vp, vp, vp],
    "MatTranspose": [vp, i32, P(vp)], "MatPtAP": [vp, vp, i32, dbl, P(vp)], "MatHIPMI355XGetProductCounts": [vp, P(i32), P(i32), P(i32)],
    "MatSOR": [vp, vp, dbl, i32, dbl, i32, i32, vp], "MatHIPMI355XGetSORInfo": [vp, P(i32), P(i32), P(i32), P(i32), P(i32)],
    "MatSeqAIJGetArrays": [vp, P(i32), P(vp), P(vp), P(vp)], "MatMPIAIJGetSeqAIJ": [vp, P(vp), P(vp), P(vp)],
    "MatMPIAIJGetScatter": [vp, P(vp), P(vp), P(i32)],
    "MatHIPMI355XSetTiming": [vp, i32], "MatHIPMI355XGetTiming": [vp, P(i32), P(dbl)],
    "MatMPIAIJHIPMI355XSetHaloTiming": [vp, i32], "MatMPIAIJHIPMI355XGetHaloTiming": [vp, P(i32), P(dbl), P(dbl), P(dbl), P(dbl), P(i32)],
    "PetscCommDeviceAllreduceLatency": [vp, i32, P(dbl), P(dbl)],
    "MatHIPMI355XGetIndexCompression": [vp, P(i32)], "MatHIPMI355XGetRowPatterns": [vp, P(i32)], "MatHIPMI355XGetTiledInfo": [vp, P(i32), P(i32)], "MatHIPMI355XGetBlockedInfo": [vp, P(i32), P(i32)], "MatHIPMI355XGetValuePatterns": [vp, P(i32)], "MatHIPMI355XSetValuePatterns": [vp, i32], "VecHIPMI355XSetCGUpdateTiming": [i32], "VecHIPMI355XGetCGUpdateTiming": [P(i32), P(dbl)], "VecHIPMI355XGetDeferralCounts": [P(i32)], "MatHIPMI355XGetInodeInfo": [vp, P(i32), P(i32), P(i32)], "MatHIPMI355XGetUploadCount": [vp, P(i32)], "MatHIPMI355XGetTransposeCounts": [vp, P(i32), P(i32)],
    "PetscMiniGenPoisson7": [i32, i32, i32, C.c_long, C.c_long, vp, vp, vp, P(C.c_long)],
    "PetscViewerBinaryOpen": [vp, C.c_char_p, i32, P(vp)], "PetscViewerDestroy": [P(vp)],
    "MatLoad": [vp, vp], "MatView": [vp, vp], "VecLoad": [vp, vp], "VecView": [vp, vp],
    "PCCreate": [vp, P(vp)], "PCSetOperators": [vp, vp, vp, i32], "PCSetFromOptions": [vp], "PCApply": [vp, vp, vp], "PCDestroy": [P(vp)],
    "PCSetType": [vp, C.c_char_p], "PCILUGetLevels_HIPMI355X": [vp, P(i32), P(i32)], "PCILUGetShiftCount_HIPMI355X": [vp, P(i32)], "PCICCGetInfo_HIPMI355X": [vp, P(i32), P(i32), P(i32)], "PCILUGetSolver_HIPMI355X": [vp, P(i32), P(i32)], "PCFactorDebugSetAborted_HIPMI355X": [vp], "PCILUGetSweeps_HIPMI355X": [vp, P(i32)], "PCILUGetNumeric_HIPMI355X": [vp, P(i32), P(i32), P(i32)], "PCILUGetFill_HIPMI355X": [vp, P(i32), P(i32), P(i32)], "PCBILUGetInfo_HIPMI355X": [vp, P(i32), P(i32), P(i32), P(i32)], "PCBILUGetSolvePlan_HIPMI355X": [vp, P(i32), P(i32), P(i32)], "PCFactorSetLevels": [vp, i32], "PCILUApplyInPlace_HIPMI355X": [vp, vp], "PCILUGetNodeInfo_HIPMI355X": [vp, P(i32), P(i32), P(i32)], "PCFactorGetMatrix": [vp, P(vp)], "MatSolve": [vp, vp, vp], "MatSolveTranspose": [vp, vp, vp], "PCApplyTranspose": [vp, vp, vp], "PCApplyTransposeExists": [vp, P(i32)], "PCILUGetTransposeBuilds_HIPMI355X": [vp, P(i32), P(i32)], "PCBJacobiGetSubKSP": [vp, P(i32), P(i32), P(vp)],
    "PCKSPGetKSP": [vp, P(vp)], "PCKSPGetTotalIterations": [vp, P(i32)], "KSPFGMRESSetModifyPC": [vp, vp, vp, vp], "KSPGetTolerances": [vp, P(dbl), P(dbl), P(dbl), P(i32)], "KSPGetType": [vp, P(C.c_char_p)],
    "KSPCreate": [vp, P(vp)], "KSPSetType": [vp, C.c_char_p], "KSPSetOperators": [vp, vp, vp, i32], "KSPGetPC": [vp, P(vp)],
    "KSPSetTolerances": [vp, dbl, dbl, dbl, i32], "KSPSetNormType": [vp, i32], "KSPSetPCSide": [vp, i32], "KSPSetInitialGuessNonzero": [vp, i32], "KSPSetOptionsPrefix": [vp, C.c_char_p],
    "KSPSetFromOptions": [vp], "KSPGMRESSetRestart": [vp, i32], "KSPGMRESSetCGSRefinementType": [vp, i32],
    "KSPChebychevSetEigenvalues": [vp, dbl, dbl], "KSPRichardsonSetScale": [vp, dbl], "KSPMonitorSet": [vp, vp, vp, vp],
    "PCApplyRichardson": [vp, vp, vp, vp, dbl, dbl, dbl, i32, i32, P(i32), P(i32)], "PCApplyRichardsonExists": [vp, P(i32)],
    "KSPHIPMI355XGetFusedStepCounts": [vp, P(i32), P(i32)],
    "KSPSetConvergenceTest": [vp, vp, vp, vp], "KSPLSQRSetStandardErrorVec": [vp, vp], "KSPLSQRGetStandardErrorVec": [vp, P(vp)],
    "KSPLSQRGetArnorm": [vp, P(dbl), P(dbl), P(dbl)],
    "MatRestrict": [vp, vp, vp], "MatInterpolate": [vp, vp, vp], "MatInterpolateAdd": [vp, vp, vp, vp], "MatResidual": [vp, vp, vp, vp],
    "MatHIPMI355XGetResidualCounts": [vp, P(i32), P(i32)], "HIPMI355XGetLiveFactors": [P(i32), P(i32)],
    "PCMGSetLevels": [vp, i32, vp], "PCMGGetLevels": [vp, P(i32)], "PCMGSetType": [vp, i32], "PCMGSetCycleType": [vp, i32],
    "PCMGMultiplicativeSetCycles": [vp, i32], "PCMGSetNumberSmoothDown": [vp, i32], "PCMGSetNumberSmoothUp": [vp, i32],
    "PCMGSetGalerkin": [vp, i32], "PCMGSetInterpolation": [vp, i32, vp], "PCMGSetRestriction": [vp, i32, vp],
    "PCMGSetResidual": [vp, i32, vp, vp], "PCMGDefaultResidual": [vp, vp, vp, vp], "PCMGGetSmoother": [vp, i32, P(vp)],
    "PCMGGetSmootherDown": [vp, i32, P(vp)], "PCMGGetSmootherUp": [vp, i32, P(vp)], "PCMGGetCoarseSolve": [vp, P(vp)], "PCSetUp": [vp],
    "MatCoarsenAggregate": [vp, dbl, P(i32), vp], "MatHIPMI355XGetCoarsenCounts": [vp, P(i32), P(i32), P(i32)],
    "PCGAMGSetThreshold": [vp, dbl], "PCGAMGSetCoarseEqLimit": [vp, i32], "PCGAMGSetNlevels": [vp, i32], "PCGAMGSetNSmooths": [vp, i32],
    "PCGAMGSetReuseInterpolation": [vp, i32], "PCGAMGGetLevelSizes": [vp, i32, P(i32), vp],
    "PCGetOperators": [vp, P(vp), P(vp), P(i32)],
    "KSPSetUp": [vp], "KSPSolve": [vp, vp, vp], "KSPGetIterationNumber": [vp, P(i32)], "KSPGetResidualNorm": [vp, P(dbl)],
    "KSPGetConvergedReason": [vp, P(i32)], "KSPSetResidualHistory": [vp, vp, i32, i32],
    "KSPGetResidualHistory": [vp, P(vp), P(i32)], "KSPDestroy": [P(vp)],
}

# names exported by the plugin library; everything else in _SIG lives in the harness
_PLUGIN = {n for n in _SIG if "HIPMI355X" in n} | {
    "PetscCommSetDeviceComm", "PetscCommSetDeviceComms", "PetscCommGetDeviceTransport", "PetscCommDeviceAllreduceLatency", "VecScatterBegin", "VecScatterEnd",
    "VecScatterGetLists", "MatSeqAIJGetArrays", "MatMPIAIJGetSeqAIJ", "MatMPIAIJGetScatter"}

INSERT_VALUES, ADD_VALUES = 1, 2
SCATTER_FORWARD, SCATTER_REVERSE = 0, 1
NORM_1, NORM_2, NORM_FROBENIUS, NORM_INFINITY, NORM_1_AND_2 = 0, 1, 2, 3, 4
MAT_FINAL_ASSEMBLY, MAT_FLUSH_ASSEMBLY = 0, 1
PETSC_DECIDE, PETSC_DEFAULT = -1, -2
DIFFERENT_NONZERO_PATTERN, SUBSET_NONZERO_PATTERN, SAME_NONZERO_PATTERN = 0, 1, 2
MAT_INITIAL_MATRIX, MAT_REUSE_MATRIX = 0, 1          # MatReuse (petscmini.h)
KSP_NORM_NONE, KSP_NORM_PRECONDITIONED, KSP_NORM_UNPRECONDITIONED, KSP_NORM_NATURAL = 0, 1, 2, 3   # KSPNormType (petscmini.h)
MAT_KEEP_NONZERO_PATTERN = 9          # MatOption (petscmini.h)
# MatSORType (petscmini.h)
SOR_FORWARD_SWEEP, SOR_BACKWARD_SWEEP, SOR_SYMMETRIC_SWEEP = 1, 2, 3
SOR_LOCAL_FORWARD_SWEEP, SOR_LOCAL_BACKWARD_SWEEP, SOR_LOCAL_SYMMETRIC_SWEEP = 4, 8, 12
SOR_ZERO_INITIAL_GUESS, SOR_EISENSTAT, SOR_APPLY_UPPER, SOR_APPLY_LOWER = 16, 32, 64, 128
PC_MG_MULTIPLICATIVE, PC_MG_ADDITIVE, PC_MG_FULL, PC_MG_KASKADE = 0, 1, 2, 3   # PCMGType (petscmini.h)
PC_MG_CYCLE_V, PC_MG_CYCLE_W = 1, 2                                           # PCMGCycleType (petscmini.h)


class PetscError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("PetscErrorCode %d\n%s" % (code, text))
        self.code = code


class Lib:
    """Checked function access: lib.VecAXPY(y, a, x) raises PetscError on a non-zero return."""

    def __init__(self):
        load_kernels()
        self._h = load_harness()       # object model: VecCreate, MatMult, KSPSolve, ...
        self._p = load_host()          # plugin: type constructors, PetscHIPMI355X*, introspection
        self._h.PetscGetLastErrorMessage.restype = C.c_char_p
        self._p.PetscHIPMI355XVersion.restype = C.c_char_p
        for name, args in _SIG.items():
            fn = self._sym(name)
            fn.argtypes = args
            fn.restype = i32
        self.COMM_SELF = vp.in_dll(self._h, "PETSC_COMM_SELF")
        self.chk(self._p.PetscHIPMI355XInitialize(-1))

    def _sym(self, name):
        """a function of the plugin or of the harness (each name is exported by exactly one of them)"""
        try:
            return getattr(self._p, name) if name in _PLUGIN else getattr(self._h, name)
        except AttributeError:
            return getattr(self._h, name) if name in _PLUGIN else getattr(self._p, name)

    @property
    def COMM_WORLD(self):
        return vp.in_dll(self._h, "PETSC_COMM_WORLD")

    def chk(self, rc):
        if rc:
            raise PetscError(rc, self._h.PetscGetLastErrorMessage().decode(errors="replace"))

    def __getattr__(self, name):
        fn = self._sym(name)

        def call(*a):
            self.chk(fn(*a))
        return call

    def raw(self, name):
        return self._sym(name)


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = Lib()
    return _lib


def _ptr(a):
    return a.ctypes.data_as(vp) if a is not None else None


class Vec:
    def __init__(self, handle=None, own=True):
        self.h = handle if handle is not None else vp()
        self.own = own

    @classmethod
    def create(cls, n, N=None, comm=None, vtype=b"hipmi355x"):
        L = lib()
        v = cls()
        L.VecCreate(comm or L.COMM_WORLD, C.byref(v.h))
        L.VecSetSizes(v.h, n, PETSC_DECIDE if N is None else N)
        L.VecSetType(v.h, vtype)
        return v

    @classmethod
    def from_array(cls, a, comm=None, N=None, vtype=b"hipmi355x"):
        a = np.ascontiguousarray(a, dtype=np.float64)
        v = cls.create(a.size, N=N, comm=comm, vtype=vtype)
        v.set_array(a)
        return v

    def duplicate(self):
        w = Vec()
        lib().VecDuplicate(self.h, C.byref(w.h))
        return w

    @property
    def n(self):
        k = i32()
        lib().VecGetLocalSize(self.h, C.byref(k))
        return k.value

    def set_array(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = vp()
        lib().VecGetArray(self.h, C.byref(p))
        C.memmove(p, a.ctypes.data, a.nbytes)
        lib().VecRestoreArray(self.h, C.byref(p))

    def array(self):
        n = self.n
        p = vp()
        lib().VecGetArrayRead(self.h, C.byref(p))
        out = np.empty(n)
        if n:
            C.memmove(out.ctypes.data, p, out.nbytes)
        lib().VecRestoreArrayRead(self.h, C.byref(p))
        return out

    def norm(self, t=NORM_2):
        r = (dbl * 2)()
        lib().VecNorm(self.h, t, r)
        return (r[0], r[1]) if t == NORM_1_AND_2 else r[0]

    def dot(self, y):
        r = dbl()
        lib().VecDot(self.h, y.h, C.byref(r))
        return r.value

    def sum(self):
        r = dbl()
        lib().VecSum(self.h, C.byref(r))
        return r.value

    def shift(self, a):
        """every entry + a (VecShift)"""
        lib().VecShift(self.h, float(a))

    def max(self):
        """(location, value) of the maximum, the first one among equals (VecMax)"""
        p, r = i32(), dbl()
        lib().VecMax(self.h, C.byref(p), C.byref(r))
        return p.value, r.value

    def min(self):
        """(location, value) of the minimum, the first one among equals (VecMin)"""
        p, r = i32(), dbl()
        lib().VecMin(self.h, C.byref(p), C.byref(r))
        return p.value, r.value

    def destroy(self):
        if self.own and self.h:
            lib().VecDestroy(C.byref(self.h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def vec_table(vecs):
    return (vp * len(vecs))(*[v.h.value for v in vecs])


class Mat:
    def __init__(self, handle=None, own=True):
        self.h = handle if handle is not None else vp()
        self.own = own
        self._keep = None

    @classmethod
    def from_csr(cls, ai, aj, aa, ncols=None, comm=None):
        """sequential: MatCreateSeqAIJWithArrays"""
        L = lib()
        ai = np.ascontiguousarray(ai, dtype=np.int32); aj = np.ascontiguousarray(aj, dtype=np.int32)
        aa = np.ascontiguousarray(aa, dtype=np.float64)
        m = ai.size - 1
        A = cls()
        L.MatCreateSeqAIJWithArrays(comm or L.COMM_SELF, m, m if ncols is None else ncols, _ptr(ai), _ptr(aj), _ptr(aa), C.byref(A.h))
        return A

    @classmethod
    def from_csr_mpi(cls, ai, aj, aa, n_local_cols, M=PETSC_DECIDE, N=PETSC_DECIDE, comm=None):
        """this rank's rows with global column indices: MatCreateMPIAIJWithArrays"""
        L = lib()
        ai = np.ascontiguousarray(ai, dtype=np.int32); aj = np.ascontiguousarray(aj, dtype=np.int32)
        aa = np.ascontiguousarray(aa, dtype=np.float64)
        A = cls()
        L.MatCreateMPIAIJWithArrays(comm or L.COMM_WORLD, ai.size - 1, n_local_cols, M, N, _ptr(ai), _ptr(aj), _ptr(aa), C.byref(A.h))
        return A

    @classmethod
    def from_bsr(cls, bs, ai, aj, aa, nbcols=None, comm=None):
        L = lib()
        ai = np.ascontiguousarray(ai, dtype=np.int32); aj = np.ascontiguousarray(aj, dtype=np.int32)
        aa = np.ascontiguousarray(aa, dtype=np.float64)
        mbs = ai.size - 1
        nb = mbs if nbcols is None else nbcols
        A = cls()
        L.MatCreateSeqBAIJWithArrays(comm or L.COMM_SELF, bs, mbs * bs, nb * bs, _ptr(ai), _ptr(aj), _ptr(aa), C.byref(A.h))
        return A

    def get_vecs(self):
        r, l = Vec(), Vec()
        lib().MatGetVecs(self.h, C.byref(r.h), C.byref(l.h))
        return r, l

    def mult(self, x, y):
        lib().MatMult(self.h, x.h, y.h)

    def shift(self, alpha):
        """a(i,i) += alpha for every local row (MatShift)"""
        lib().MatShift(self.h, alpha)

    def axpy(self, alpha, X, structure=SAME_NONZERO_PATTERN):
        """self += alpha X (MatAXPY)"""
        lib().MatAXPY(self.h, alpha, X.h, structure)

    def copy(self, B, structure=SAME_NONZERO_PATTERN):
        """B <- self (MatCopy)"""
        lib().MatCopy(self.h, B.h, structure)

    @staticmethod
    def _rows(rows):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        return r, r.size, r.ctypes.data_as(vp)

    def zero_rows(self, rows, diag=0.0, x=None, b=None):
        """zero the listed rows, diag on their diagonal; b[r] = diag x[r] when x and b are given (MatZeroRows)"""
        r, n, p = self._rows(rows)
        lib().MatZeroRows(self.h, n, p, diag, x.h if x is not None else None, b.h if b is not None else None)

    def zero_rows_columns(self, rows, diag=0.0, x=None, b=None):
        """zero the listed rows and columns, diag on the diagonal, b corrected by the eliminated entries (MatZeroRowsColumns)"""
        r, n, p = self._rows(rows)
        lib().MatZeroRowsColumns(self.h, n, p, diag, x.h if x is not None else None, b.h if b is not None else None)

    def norm(self, kind=NORM_FROBENIUS):
        """NORM_1, NORM_FROBENIUS or NORM_INFINITY of the matrix (MatNorm)"""
        r = dbl()
        lib().MatNorm(self.h, kind, C.byref(r))
        return r.value

    def _row_extremum(self, name):
        _, v = self.get_vecs()
        idx = np.full(max(v.n, 1), -1, np.int32)
        getattr(lib(), name)(self.h, v.h, _ptr(idx))
        return v, idx[:v.n]

    def row_max_abs(self):
        """(Vec of max_j |a_ij|, ndarray of the columns they were found at) (MatGetRowMaxAbs)"""
        return self._row_extremum("MatGetRowMaxAbs")

    def row_max(self):
        """(Vec of the rows' largest entries, an implicit zero included, ndarray of their columns) (MatGetRowMax)"""
        return self._row_extremum("MatGetRowMax")

    def row_min(self):
        """(Vec of the rows' smallest entries, an implicit zero included, ndarray of their columns) (MatGetRowMin)"""
        return self._row_extremum("MatGetRowMin")

    def row_sum(self):
        """Vec of the row sums: the product with a vector of ones (MatGetRowSum)"""
        _, v = self.get_vecs()
        lib().MatGetRowSum(self.h, v.h)
        return v

    def column_norms(self, kind=NORM_2):
        """ndarray of the NORM_1, NORM_2 or NORM_INFINITY norms of all columns (MatGetColumnNorms)"""
        n = i32()
        lib().MatGetSize(self.h, None, C.byref(n))
        out = np.zeros(max(n.value, 1))
        lib().MatGetColumnNorms(self.h, kind, _ptr(out))
        return out[:n.value]

    def set_option(self, op, flag=True):
        lib().MatSetOption(self.h, op, 1 if flag else 0)

    def sor(self, b, x, omega=1.0, flag=SOR_LOCAL_SYMMETRIC_SWEEP, shift=0.0, its=1, lits=1):
        """its * lits (S)SOR sweeps on A x = b, x updated in place; flag: SOR_* bits, SOR_ZERO_INITIAL_GUESS to ignore x's content (MatSOR)"""
        lib().MatSOR(self.h, b.h, omega, flag, shift, its, lits, x.h)

    def sor_info(self):
        """levels, launches per sweep, inverted-diagonal builds, plan builds, device applications (MatHIPMI355XGetSORInfo)"""
        v = [i32() for _ in range(5)]
        lib().MatHIPMI355XGetSORInfo(self.h, *[C.byref(q) for q in v])
        return tuple(q.value for q in v)

    def matmult(self, B, reuse=None):
        """C = self B (MatMatMult); reuse: the Mat an earlier call with the same operands returned, filled again (MAT_REUSE_MATRIX)"""
        Cm = reuse if reuse is not None else Mat()
        lib().MatMatMult(self.h, B.h, MAT_INITIAL_MATRIX if reuse is None else MAT_REUSE_MATRIX, float(PETSC_DEFAULT), C.byref(Cm.h))
        return Cm

    def transpose(self, reuse=None):
        """B = self^T as a matrix of its own (MatTranspose); reuse as in matmult"""
        Bm = reuse if reuse is not None else Mat()
        lib().MatTranspose(self.h, MAT_INITIAL_MATRIX if reuse is None else MAT_REUSE_MATRIX, C.byref(Bm.h))
        return Bm

    def ptap(self, Pm, reuse=None):
        """C = Pm^T self Pm (MatPtAP); reuse as in matmult"""
        Cm = reuse if reuse is not None else Mat()
        lib().MatPtAP(self.h, Pm.h, MAT_INITIAL_MATRIX if reuse is None else MAT_REUSE_MATRIX, float(PETSC_DEFAULT), C.byref(Cm.h))
        return Cm

    def product_counts(self):
        """of the result of matmult / transpose / ptap: host symbolic passes, device numerics, host numerics (MatHIPMI355XGetProductCounts)"""
        v = [i32() for _ in range(3)]
        lib().MatHIPMI355XGetProductCounts(self.h, *[C.byref(q) for q in v])
        return tuple(q.value for q in v)

    def aggregate(self, theta=0.0):
        """MatCoarsenAggregate: (aggregate number of every row, number of aggregates) from the strength mask
        |a_ij| > theta sqrt(|a_ii| |a_jj|) and a distance-2 maximal independent set of its graph"""
        import numpy as np
        agg = np.zeros(max(self.local_size()[0], 1), dtype=np.int32)
        n = i32()
        lib().MatCoarsenAggregate(self.h, float(theta), C.byref(n), agg.ctypes.data_as(vp))
        return agg[:self.local_size()[0]], n.value

    def coarsen_counts(self):
        """coarsenings of this matrix on the device route, on the host route, device rounds of the last one (MatHIPMI355XGetCoarsenCounts)"""
        v = [i32() for _ in range(3)]
        lib().MatHIPMI355XGetCoarsenCounts(self.h, *[C.byref(q) for q in v])
        return tuple(q.value for q in v)

    @staticmethod
    def coarsen_counts_total():
        """the same over every matrix of the process (the level operators of a PCGAMG are the PC's own)"""
        v = [i32() for _ in range(3)]
        lib().MatHIPMI355XGetCoarsenCounts(None, *[C.byref(q) for q in v])
        return tuple(q.value for q in v)

    def residual(self, b, x, r):
        """r = b - self x: the type's own method, or MatMult and VecAYPX(r, -1, b) (MatResidual)"""
        lib().MatResidual(self.h, b.h, x.h, r.h)

    def restrict(self, x, y):
        """y = self x or self^T x, whichever fits the sizes (MatRestrict)"""
        lib().MatRestrict(self.h, x.h, y.h)

    def interpolate(self, x, y):
        """y = self x or self^T x, whichever fits the sizes (MatInterpolate)"""
        lib().MatInterpolate(self.h, x.h, y.h)

    def interpolate_add(self, x, y, w):
        """w = y + self x or y + self^T x, whichever fits the sizes; w may be y (MatInterpolateAdd)"""
        lib().MatInterpolateAdd(self.h, x.h, y.h, w.h)

    def residual_counts(self):
        """residuals of a sequential AIJ matrix that took the fused kernel / MatMult and VecAYPX, so far (MatHIPMI355XGetResidualCounts)"""
        f, c = i32(), i32()
        lib().MatHIPMI355XGetResidualCounts(self.h, C.byref(f), C.byref(c))
        return f.value, c.value

    def csr(self):
        """copies of a sequential matrix's host arrays: row pointer, columns, values (MatSeqAIJGetArrays)"""
        m, pi_, pj, pa = i32(), vp(), vp(), vp()
        lib().MatSeqAIJGetArrays(self.h, C.byref(m), C.byref(pi_), C.byref(pj), C.byref(pa))
        ai = np.ctypeslib.as_array(C.cast(pi_, P(i32)), (m.value + 1,)).copy()
        nz = int(ai[-1])
        aj = np.ctypeslib.as_array(C.cast(pj, P(i32)), (max(nz, 1),))[:nz].copy()
        aa = np.ctypeslib.as_array(C.cast(pa, P(dbl)), (max(nz, 1),))[:nz].copy()
        return ai, aj, aa

    def local_size(self):
        m, n = i32(), i32()
        lib().MatGetLocalSize(self.h, C.byref(m), C.byref(n))
        return m.value, n.value

    def destroy(self):
        if self.own and self.h:
            lib().MatDestroy(C.byref(self.h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class NullSpace:
    """MatNullSpace: the constant vector (constant=True) and / or orthonormal vectors; remove() projects it out of a vector"""

    def __init__(self, constant=True, vecs=(), comm=None):
        self.h = vp()
        self.vecs = list(vecs)
        lib().MatNullSpaceCreate(comm or lib().COMM_WORLD, 1 if constant else 0, len(self.vecs), vec_table(self.vecs) if self.vecs else None, C.byref(self.h))

    def set_device_constant(self):
        """project the constant out through the plug-in's callback (MatNullSpaceSetFunction with MatNullSpaceRemoveConstantHIPMI355X)"""
        fn = C.cast(lib().raw("MatNullSpaceRemoveConstantHIPMI355X"), vp)
        lib().MatNullSpaceSetFunction(self.h, fn, None)

    def remove(self, v, out=False):
        """in place, or (out=True) into the null space's own copy, which is returned (not owned by the caller)"""
        if not out:
            lib().MatNullSpaceRemove(self.h, v.h, None)
            return v
        w = Vec(own=False)
        lib().MatNullSpaceRemove(self.h, v.h, C.byref(w.h))
        return w

    def test(self, A):
        k = i32()
        lib().MatNullSpaceTest(self.h, A.h, C.byref(k))
        return bool(k.value)

    def destroy(self):
        if self.h:
            lib().MatNullSpaceDestroy(C.byref(self.h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PC:
    """a PC that belongs to a KSP (KSP.get_pc): not owned, never destroyed from here"""

    def __init__(self, handle):
        self.h = handle

    def set_type(self, t):
        lib().PCSetType(self.h, t.encode())

    def apply(self, x, y):
        lib().PCApply(self.h, x.h, y.h)

    def apply_transpose(self, x, y):
        """PCApplyTranspose: y = B^T x; PetscError(PETSC_ERR_SUP) for a type without a transposed application"""
        lib().PCApplyTranspose(self.h, x.h, y.h)

    def apply_transpose_exists(self):
        flg = i32()
        lib().PCApplyTransposeExists(self.h, C.byref(flg))
        return bool(flg.value)

    def ksp_get_ksp(self):
        """PCKSPGetKSP: the inner solver of a PC of type "ksp" (options prefix "<pc prefix>ksp_"), created now if need be; a borrowed
        KSP, never destroyed from here"""
        k = vp()
        lib().PCKSPGetKSP(self.h, C.byref(k))
        return KSP(handle=k)

    # ---- PCMG (type "mg"); the PC keeps a Python reference to the matrix in each slot it was handed one for; a new one replaces the old
    def _hold(self, slot, M):
        self.__dict__.setdefault("_mats", {})[slot] = M
        return M.h if M is not None else None

    def set_from_options(self):
        lib().PCSetFromOptions(self.h)

    def set_up(self):
        lib().PCSetUp(self.h)

    def mg_set_levels(self, n):
        lib().PCMGSetLevels(self.h, int(n), None)

    def mg_get_levels(self):
        n = i32()
        lib().PCMGGetLevels(self.h, C.byref(n))
        return n.value

    def mg_set_type(self, form):
        """PCMGSetType: "multiplicative", "additive", "full" ("kaskade": PETSC_ERR_SUP) or the PCMGType number"""
        names = {"multiplicative": PC_MG_MULTIPLICATIVE, "additive": PC_MG_ADDITIVE, "full": PC_MG_FULL, "kaskade": PC_MG_KASKADE}
        lib().PCMGSetType(self.h, names[form] if isinstance(form, str) else int(form))

    def mg_set_cycle_type(self, c):
        """PCMGSetCycleType: "v", "w" or the PCMGCycleType number"""
        names = {"v": PC_MG_CYCLE_V, "w": PC_MG_CYCLE_W}
        lib().PCMGSetCycleType(self.h, names[c] if isinstance(c, str) else int(c))

    def mg_set_cycles(self, n):
        """PCMGMultiplicativeSetCycles: cycles per application of the multiplicative form"""
        lib().PCMGMultiplicativeSetCycles(self.h, int(n))

    def mg_set_number_smooth(self, down=None, up=None):
        """PCMGSetNumberSmoothDown / PCMGSetNumberSmoothUp; unequal counts give every level a second smoother"""
        if down is not None:
            lib().PCMGSetNumberSmoothDown(self.h, int(down))
        if up is not None:
            lib().PCMGSetNumberSmoothUp(self.h, int(up))

    def mg_set_galerkin(self, flag=True):
        lib().PCMGSetGalerkin(self.h, 1 if flag else 0)

    def mg_set_interpolation(self, l, Pm):
        lib().PCMGSetInterpolation(self.h, int(l), self._hold(("interpolation", int(l)), Pm))

    def mg_set_restriction(self, l, Rm):
        lib().PCMGSetRestriction(self.h, int(l), self._hold(("restriction", int(l)), Rm))

    def mg_set_residual(self, l, A=None):
        """PCMGSetResidual with PCMGDefaultResidual (MatResidual) on A (None: the level's operator)"""
        lib().PCMGSetResidual(self.h, int(l), C.cast(lib().raw("PCMGDefaultResidual"), vp), self._hold(("residual", int(l)), A))

    def _mg_ksp(self, name, *a):
        k = vp()
        getattr(lib(), name)(self.h, *a, C.byref(k))
        return KSP(handle=k)

    def mg_get_smoother(self, l):
        """PCMGGetSmoother: level l's (down) solver, prefix "<pc prefix>mg_levels_<l>_" ("mg_coarse_" for level 0); a borrowed KSP"""
        return self._mg_ksp("PCMGGetSmoother", int(l))

    def mg_get_smoother_down(self, l):
        return self._mg_ksp("PCMGGetSmootherDown", int(l))

    def mg_get_smoother_up(self, l):
        """PCMGGetSmootherUp: level l's up smoother, made a solver of its own by this call; a borrowed KSP"""
        return self._mg_ksp("PCMGGetSmootherUp", int(l))

    def mg_get_coarse_solve(self):
        return self._mg_ksp("PCMGGetCoarseSolve")

    # ---- PCGAMG (type "gamg"): smoothed aggregation that fills a PCMG; the mg_* calls above work on it once it is set up
    def gamg_set_threshold(self, theta):
        lib().PCGAMGSetThreshold(self.h, float(theta))

    def gamg_set_coarse_eq_limit(self, n):
        lib().PCGAMGSetCoarseEqLimit(self.h, int(n))

    def gamg_set_nlevels(self, n):
        lib().PCGAMGSetNlevels(self.h, int(n))

    def gamg_set_nsmooths(self, n):
        lib().PCGAMGSetNSmooths(self.h, int(n))

    def gamg_set_reuse_interpolation(self, flag=True):
        lib().PCGAMGSetReuseInterpolation(self.h, 1 if flag else 0)

    def gamg_level_sizes(self):
        """PCGAMGGetLevelSizes: the rows of every level of the last set-up, the fine level first"""
        n = i32()
        sizes = (i32 * 1000)()
        lib().PCGAMGGetLevelSizes(self.h, 1000, C.byref(n), sizes)
        return [sizes[k] for k in range(n.value)]

    def ksp_total_iterations(self):
        """PCKSPGetTotalIterations: the inner iterations of all applications of a PC of type "ksp" so far"""
        n = i32()
        lib().PCKSPGetTotalIterations(self.h, C.byref(n))
        return n.value


MODIFY_PC_FN = C.CFUNCTYPE(i32, vp, i32, i32, dbl, vp)   # KSPFGMRESSetModifyPC's routine: (ksp, total_its, loc_its, res_norm, ctx)


class KSP:
    def __init__(self, comm=None, handle=None):
        """a new KSP on comm, or (handle given) a borrowed one that is never destroyed from here"""
        self._hist = None
        self._modify_pc = None
        self._pc = None
        self.own = handle is None
        if handle is not None:
            self.h = handle
            return
        self.h = vp()
        lib().KSPCreate(comm or lib().COMM_WORLD, C.byref(self.h))

    def set_null_space(self, nullsp):
        """KSPSetNullSpace; None takes it away"""
        lib().KSPSetNullSpace(self.h, nullsp.h if nullsp is not None else None)

    def set_operators(self, A, P_=None):
        lib().KSPSetOperators(self.h, A.h, (P_ or A).h, 0)

    def set_type(self, t):
        lib().KSPSetType(self.h, t.encode())

    def get_pc(self):
        """the KSP's PC: one wrapper per KSP, so that what the PC holds on to (the matrices of a PCMG) lives as long as the KSP's wrapper"""
        pc = vp()
        lib().KSPGetPC(self.h, C.byref(pc))
        if self._pc is None or self._pc.h.value != pc.value:
            self._pc = PC(pc)
        return self._pc

    def set_pc_type(self, t):
        pc = vp()
        lib().KSPGetPC(self.h, C.byref(pc))
        lib().PCSetType(pc, t.encode())

    def get_type(self):
        t = C.c_char_p()
        lib().KSPGetType(self.h, C.byref(t))
        return t.value.decode()

    def get_tolerances(self):
        """KSPGetTolerances: (rtol, abstol, dtol, max_it)"""
        r, a, d, m = dbl(), dbl(), dbl(), i32()
        lib().KSPGetTolerances(self.h, C.byref(r), C.byref(a), C.byref(d), C.byref(m))
        return r.value, a.value, d.value, m.value

    def fgmres_set_modify_pc(self, fn):
        """KSPFGMRESSetModifyPC: fn(total_its, loc_its, res_norm) runs before every preconditioner application of the fgmres types
        and may change the preconditioner; None restores KSPFGMRESModifyPCNoChange.  Ignored by any other type."""
        if fn is None:
            self._modify_pc = None
            lib().KSPFGMRESSetModifyPC(self.h, None, None, None)
            return

        def call(ksp, its, k, rn, ctx):
            fn(its, k, rn)
            return 0
        self._modify_pc = MODIFY_PC_FN(call)
        lib().KSPFGMRESSetModifyPC(self.h, C.cast(self._modify_pc, vp), None, None)

    def set_tolerances(self, rtol=PETSC_DEFAULT, abstol=PETSC_DEFAULT, dtol=PETSC_DEFAULT, max_it=PETSC_DEFAULT):
        lib().KSPSetTolerances(self.h, float(rtol), float(abstol), float(dtol), int(max_it))

    def set_from_options(self):
        lib().KSPSetFromOptions(self.h)

    def set_norm_type(self, norm):
        """KSPSetNormType: "none", "preconditioned", "unpreconditioned", "natural" or the KSPNormType number"""
        names = {"none": KSP_NORM_NONE, "preconditioned": KSP_NORM_PRECONDITIONED, "unpreconditioned": KSP_NORM_UNPRECONDITIONED, "natural": KSP_NORM_NATURAL}
        lib().KSPSetNormType(self.h, names[norm] if isinstance(norm, str) else int(norm))

    def set_initial_guess_nonzero(self, flag=True):
        lib().KSPSetInitialGuessNonzero(self.h, 1 if flag else 0)

    def set_chebychev_eigenvalues(self, emax, emin):
        """KSPChebychevSetEigenvalues: bounds of the preconditioned operator's spectrum (the chebychev types; ignored by any other)"""
        lib().KSPChebychevSetEigenvalues(self.h, float(emax), float(emin))

    def set_richardson_scale(self, scale):
        """KSPRichardsonSetScale: the damping factor (the richardson types; ignored by any other)"""
        lib().KSPRichardsonSetScale(self.h, float(scale))

    def set_convergence_test(self, name="KSPDefaultConverged"):
        """KSPSetConvergenceTest with one of the library's own tests, by name: KSPDefaultConverged, KSPSkipConverged, KSPLSQRDefaultConverged"""
        lib().KSPSetConvergenceTest(self.h, C.cast(lib().raw(name), vp), None, None)

    def lsqr_set_standard_error_vec(self, se):
        """KSPLSQRSetStandardErrorVec: the LSQR types keep the running sum of (w .* w) / rho^2 in se; the KSP takes over the reference"""
        lib().KSPLSQRSetStandardErrorVec(self.h, se.h)
        se.own = False

    def lsqr_get_standard_error_vec(self):
        """KSPLSQRGetStandardErrorVec: the vector (not owned by the caller), or None"""
        se = vp()
        lib().KSPLSQRGetStandardErrorVec(self.h, C.byref(se))
        return Vec(se, own=False) if se.value else None

    def lsqr_get_arnorm(self):
        """KSPLSQRGetArnorm: the estimates (||A^T r||, ||b||, ||A||_F) of the last solve of an LSQR type"""
        a, r, n = dbl(), dbl(), dbl()
        lib().KSPLSQRGetArnorm(self.h, C.byref(a), C.byref(r), C.byref(n))
        return a.value, r.value, n.value

    def fused_step_counts(self):
        """KSPHIPMI355XGetFusedStepCounts: (fused, opbyop) update steps of the pipelined CG types since the type was set; minreshipmi355x: (Lanczos sweeps run, 0); tfqmrhipmi355x / cgshipmi355x: (fused sweeps run, iterations with a step run op by op); lsqrhipmi355x: (bidiagonalisation sweeps run, update sweeps run); fgmreshipmi355x: (steps whose sweep wrote the next preconditioned direction, all other steps), over all solves since the type was set; (0, 0) for any other"""
        f = i32(); o = i32()
        lib().KSPHIPMI355XGetFusedStepCounts(self.h, C.byref(f), C.byref(o))
        return f.value, o.value

    def record_history(self, n=20000):
        self._hist = np.zeros(n)
        lib().KSPSetResidualHistory(self.h, _ptr(self._hist), n, 1)

    def solve(self, b, x):
        lib().KSPSolve(self.h, b.h, x.h)

    @property
    def its(self):
        k = i32()
        lib().KSPGetIterationNumber(self.h, C.byref(k))
        return k.value

    @property
    def reason(self):
        k = i32()
        lib().KSPGetConvergedReason(self.h, C.byref(k))
        return k.value

    @property
    def rnorm(self):
        r = dbl()
        lib().KSPGetResidualNorm(self.h, C.byref(r))
        return r.value

    def history(self):
        p = vp(); n = i32()
        lib().KSPGetResidualHistory(self.h, C.byref(p), C.byref(n))
        return self._hist[:n.value].copy()

    def destroy(self):
        if self.own and self.h:
            lib().KSPDestroy(C.byref(self.h))

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def gen_poisson7(nx, ny, nz, rstart=0, rend=None):
    """this rank's rows of P7(nx,ny,nz) as CSR with global columns (host arrays for MatCreate*WithArrays)"""
    L = lib()
    if rend is None:
        rend = nx * ny * nz
    nnz = C.c_long()
    L.PetscMiniGenPoisson7(nx, ny, nz, rstart, rend, None, None, None, C.byref(nnz))
    ai = np.zeros(rend - rstart + 1, dtype=np.int32)
    aj = np.zeros(nnz.value, dtype=np.int32)
    aa = np.zeros(nnz.value)
    L.PetscMiniGenPoisson7(nx, ny, nz, rstart, rend, _ptr(ai), _ptr(aj), _ptr(aa), C.byref(nnz))
    return ai, aj, aa
