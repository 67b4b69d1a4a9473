"""The life cycle of the plug-in's twelve KSP types without a GPU (petsc-dev_amd/host/kspfused.c): KSPSetType into each of them, out of
it into other plug-in types and back, and on to the harness's "cg".  What a type composes at create is there while the KSP has that
type and gone once it has another, so no method of a destroyed type stays callable: the step counts of a type that does not answer are
(0, 0) without an error, and KSPChebychevSetEigenvalues / KSPRichardsonSetScale / KSPLSQRGetArnorm on a KSP of another type do nothing."""
import ctypes as C

import pytest

COUNTS = "KSPHIPMI355XGetFusedStepCounts_C"
GMRES = ("KSPGMRESSetRestart_C", "KSPGMRESSetCGSRefinementType_C")
# what each type composes on its KSP; the types with COUNTS answer KSPHIPMI355XGetFusedStepCounts, the others do not
COMPOSED = {
    "cghipmi355x": (),
    "gmreshipmi355x": GMRES,
    "fgmreshipmi355x": GMRES + ("KSPFGMRESSetModifyPC_C", COUNTS),
    "bcgshipmi355x": (),
    "chebychevhipmi355x": ("KSPChebychevSetEigenvalues_C",),
    "richardsonhipmi355x": ("KSPRichardsonSetScale_C",),
    "pipecghipmi355x": (COUNTS,),
    "minreshipmi355x": (COUNTS,),
    "tfqmrhipmi355x": (COUNTS,),
    "cgshipmi355x": (COUNTS,),
    "bicghipmi355x": (COUNTS,),
    "lsqrhipmi355x": ("KSPLSQRSetStandardErrorVec_C", "KSPLSQRGetStandardErrorVec_C", "KSPLSQRGetArnorm_C", COUNTS, "KSPDefaultPCNone_C"),
}
ALL_NAMES = sorted({n for names in COMPOSED.values() for n in names})


def composed(L, ksp):
    """the names of ALL_NAMES that PetscObjectQueryFunction finds on the KSP"""
    query = L.raw("PetscObjectQueryFunction")
    query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
    query.restype = C.c_int
    found = set()
    for name in ALL_NAMES:
        f = C.c_void_p()
        assert query(ksp.h, name.encode(), C.byref(f)) == 0
        if f.value:
            found.add(name)
    return found


def live_factors(L):
    live, watched = C.c_int(), C.c_int()
    L.HIPMI355XGetLiveFactors(C.byref(live), C.byref(watched))
    return live.value, watched.value


def enter(L, ksp, name):
    ksp.set_type(name)
    assert ksp.get_type() == name
    assert composed(L, ksp) == set(COMPOSED[name]), name
    assert ksp.fused_step_counts() == (0, 0)


@pytest.mark.parametrize("name", sorted(COMPOSED))
def test_set_type_in_and_out_of_every_plugin_type(built, name):
    from petsc_dev_amd import petsc as P
    L = P.lib()
    before = live_factors(L)
    ksp = P.KSP(comm=L.COMM_SELF)
    enter(L, ksp, name)
    # one neighbour that answers KSPHIPMI355XGetFusedStepCounts and one that does not
    counting = next(t for t in ("tfqmrhipmi355x", "lsqrhipmi355x") if t != name)
    silent = next(t for t in ("chebychevhipmi355x", "gmreshipmi355x") if t != name)
    for other in (counting, silent):
        enter(L, ksp, other)
        enter(L, ksp, name)
    ksp.set_type("cg")
    assert ksp.get_type() == "cg"
    assert composed(L, ksp) == set()
    assert ksp.fused_step_counts() == (0, 0)
    # the setters and the getter of the types just left: no method by that name, so nothing happens.  A stale
    # KSPChebychevSetEigenvalues_C would refuse emax <= emin (PETSC_ERR_ARG_INCOMP)
    ksp.set_chebychev_eigenvalues(1.0, 2.0)
    ksp.set_richardson_scale(0.5)
    assert ksp.lsqr_get_arnorm() == (0.0, 0.0, 0.0)
    ksp.destroy()
    assert live_factors(L) == before


def test_the_table_above_covers_the_registered_types(built):
    """every type the plug-in's header names is in COMPOSED"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "petschipmi355x.h")).read()
    assert set(re.findall(r'#define\s+KSP\w+HIPMI355X\s+"(\w+)"', hdr)) == set(COMPOSED)
