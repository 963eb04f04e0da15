"""pve_mcc_amd/_capi.py states the C ABI once -- PROTOTYPES, the Structures, the constants and name tuples -- and this module
holds all of it to include/*.h: with the C++ compiler from the binding to the headers, by the headers' text from the headers to
the binding, and by symbol against the libraries (tests/binding_contract.py: the generator, the naming rules, what cannot be
checked).  A new entry point, struct or constant is a row, a Structure or a statement in _capi; nothing here names one."""
import ctypes as C
import os

import pytest

from pve_mcc_amd import _capi
from tests import binding_contract as BC


def test_binding_agrees_with_the_headers():
    """every Structure's layout, every prototype's arity and classes, every constant and tuple position: one compile"""
    b = BC.binding()
    assert BC.structures(b) and all(b.PROTOTYPES.values()) and BC.constants(b) and len(BC.tuple_positions(b)) == sum(
        len(getattr(b, t)) for t in BC.NAME_TUPLES.values())
    source = BC.checks(b)
    rc, said = BC.compile_checks(source)
    print("%d static_asserts" % source.count("static_assert("))
    assert rc == 0, said
    assert (len(b.ENV_OUT_NAMES), len(b.METRIC_NAMES), len(b.STAT_NAMES)) == (b.PVE_ENV_OUT_N, b.PVE_N_METRICS, b.PVE_STAT_N)


def test_headers_are_bound():
    """every prototype of a header is in that header's group of the table (and the reverse), every struct with a body has its
    Structure, every integer macro and enumerator its constant or tuple position.  No exceptions."""
    b = BC.binding()
    names = [n for group in b.PROTOTYPES.values() for n in group]
    assert len(names) == len(set(names)), "an entry point is in two groups"
    bound_structs = {BC.c_name(n) for n in BC.structures(b)}
    bound = set(BC.constants(b)) | set(BC.tuple_positions(b))
    for header, group in b.PROTOTYPES.items():
        h = BC.declared(header)
        assert h.prototypes == sorted(group), "%s and its group of _capi.PROTOTYPES: %s" % (header, set(h.prototypes) ^ set(group))
        for s in h.structs:
            assert s in bound_structs, "%s: struct %s has no Structure in _capi" % (header, s)
        for name in list(h.macros) + h.enumerators:
            assert name in bound, "%s: %s has neither a constant nor a name-tuple position in the package" % (header, name)
    assert sorted(os.listdir(BC.INCLUDE)) == sorted(b.PROTOTYPES), "a header without a group in _capi.PROTOTYPES"


def _libraries():
    import __graft_entry__
    from tests import rank_pairs_scenarios, test_capacity256
    from tests.hip_adapter import emulator_lib
    __graft_entry__.build()
    return {"product": _capi.load_library(), "emu": emulator_lib(), "emu_wide": test_capacity256.wide_lib(),
            "emu_diag": rank_pairs_scenarios.diag_emulator_lib()}


def test_libraries_export_the_table_at_the_headers_version():
    header_version = int(BC.declared("pve_env.h").macros["PVE_ABI_VERSION"], 0)
    for which, lib in _libraries().items():
        for group in _capi.PROTOTYPES.values():
            for name, (restype, argtypes) in group.items():
                assert hasattr(lib, name), "%s does not export %s" % (which, name)
                f = getattr(lib, name)
                assert f.restype is restype and list(f.argtypes) == argtypes, "%s: %s is not dressed by the table" % (which, name)
        assert lib.pve_abi_version() == _capi.ABI_VERSION == header_version, which


class _SwappedRollout(C.Structure):          # pve_rollout with n_pool and pool_tick0, two int32 side by side, swapped
    _fields_ = [f if f[0] not in ("n_pool", "pool_tick0") else ({"n_pool": "pool_tick0", "pool_tick0": "n_pool"}[f[0]], f[1])
                for f in _capi.PveRollout._fields_]


def _narrowed_step_wide():
    group = dict(_capi.PROTOTYPES["pve_env.h"])
    restype, argtypes = group["pve_learner_step_wide"]
    k = argtypes.index(C.c_int64)
    group["pve_learner_step_wide"] = (restype, argtypes[:k] + [C.c_int] + argtypes[k + 1:])
    return dict(_capi.PROTOTYPES, **{"pve_env.h": group}), "pve_learner_step_wide: argument %d" % k


@pytest.mark.parametrize("case", ["struct", "prototype", "constant"])
def test_the_compiler_names_a_doctored_binding(case):
    """the check is not vacuous: two equal-sized fields of PveRollout swapped, one c_int64 of a prototype narrowed to c_int, one
    constant off by one -- each fails the compile, and the compiler's message names the culprit"""
    if case == "struct":
        doctored, culprit = dict(PveRollout=_SwappedRollout), "PveRollout.pool_tick0: offset"       # (sizeof and every size hold)
    elif case == "prototype":
        table, culprit = _narrowed_step_wide()
        doctored = dict(PROTOTYPES=table)
    else:
        doctored, culprit = dict(NSTEP_RECORD=_capi.NSTEP_RECORD + 1), "NSTEP_RECORD = %d" % (_capi.NSTEP_RECORD + 1)
    rc, said = BC.compile_checks(BC.checks(BC.binding(**doctored)))
    failed = [line for line in said.splitlines() if "static assertion failed" in line]
    assert rc != 0 and failed and all(culprit in line or "PveRollout.n_pool: offset" in line for line in failed), said
    assert any(culprit in line for line in failed), said
