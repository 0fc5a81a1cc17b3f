"""The mask combiner's device form (sda_mask_combiner_begin_dev / update_dev / update_sealed_rows_dev / finish_dev) as far as
a box without a GPU can see it: the symbols, their arity in the header and in the ctypes table, the NULL checks, and the whole
begin / update / finish state machine on a None-scheme handle, which needs no device (none.rs:21-26)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sda_mask_combiner_begin_dev": 3, "sda_mask_combiner_update_dev": 6, "sda_mask_combiner_update_sealed_rows_dev": 13,
       "sda_mask_combiner_finish_dev": 4}


def _header_params(name):
    text = open(os.path.join(ROOT, "include", "sda_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;{}]*)\)\s*;", text)
    assert m, name + " is not declared in include/sda_hip.h"
    return [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]


def test_the_four_symbols_are_exported_by_both_libraries(built):
    from sda_amd import capi
    for path in (capi.RELEASE_LIB_PATH, capi.TEST_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = set(re.findall(r" T (sda_[a-z0-9_]+)", out))
        assert set(NEW) <= exported, (path, set(NEW) - exported)


def test_header_and_ctypes_table_agree_on_arity(built):
    from sda_amd import capi
    for name, arity in NEW.items():
        params = _header_params(name)
        assert len(params) == arity, (name, params)
        assert params[-1] == "void* stream", (name, params[-1])
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == arity and argtypes[-1] is C.c_void_p, name


def test_abi_version_is_still_6(built):
    from sda_amd import capi
    assert capi.load().sda_abi_version() == 6


def test_null_handles_are_refused(built):
    from sda_amd import capi
    lib = capi.load()
    key = bytes(32)
    calls = [lambda: lib.sda_mask_combiner_begin_dev(None, 5, None),
             lambda: lib.sda_mask_combiner_update_dev(None, None, 1, 0, 0, None),
             lambda: lib.sda_mask_combiner_update_sealed_rows_dev(None, None, None, key, key, None, 64, None, 1, 64, None, None, None),
             lambda: lib.sda_mask_combiner_finish_dev(None, None, 0, None)]
    for call in calls:
        assert call() == capi.ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.sda_last_error()


def test_none_scheme_runs_the_whole_state_machine_without_a_device(built):
    from sda_amd import capi
    lib = capi.load()
    h = C.c_void_p()
    scheme = capi.MaskingScheme(capi.MASKING_NONE, 0, 0, 0)
    assert lib.sda_mask_combiner_new(C.byref(scheme), C.byref(h)) == capi.OK
    key = bytes(32)
    try:
        assert lib.sda_mask_combiner_update_dev(h, None, 1, 0, 0, None) == capi.ERR_STATE
        assert lib.sda_mask_combiner_finish_dev(h, None, 0, None) == capi.ERR_STATE
        for _ in range(2):                                                    # a second begin / finish cycle works
            assert lib.sda_mask_combiner_begin_dev(h, 5, None) == capi.OK
            assert lib.sda_mask_combiner_update_dev(h, None, 3, 0, 0, None) == capi.OK
            assert lib.sda_mask_combiner_update_dev(h, None, 0, 7, 7, None) == capi.OK          # rows == 0 launches nothing
            assert lib.sda_mask_combiner_update_dev(h, None, 1, 1, 1, None) == capi.ERR_ASSERTION
            assert b"none.rs:23" in lib.sda_last_error()
            assert lib.sda_mask_combiner_update_sealed_rows_dev(h, None, None, key, key, None, 64, None, 1, 64, None, None,
                                                                None) == capi.ERR_UNSUPPORTED
            assert lib.sda_mask_combiner_finish_dev(h, None, 0, None) == capi.OK
            assert lib.sda_mask_combiner_finish_dev(h, None, 0, None) == capi.ERR_STATE          # finish ended the job
    finally:
        lib.sda_mask_combiner_free(h)


def test_python_mirror_has_the_device_methods(built):
    from sda_amd import crypto
    for name in ("begin_dev", "update_dev", "update_sealed_rows_dev", "finish_dev", "combine_sealed_job"):
        assert callable(getattr(crypto.MaskCombiner, name))
    comb = crypto.MaskCombiner(crypto.NoMask())
    with pytest.raises(crypto.SdaError) as e:
        comb.update_dev(0, 1, 0, 0)
    assert e.value.code == capi_code("ERR_STATE")
    comb.begin_dev(5)
    comb.update_dev(0, 2, 0, 0)
    with pytest.raises(AssertionError):
        comb.update_dev(0, 1, 1, 1)
    comb.finish_dev(0, 0)


def capi_code(name):
    from sda_amd import capi
    return getattr(capi, name)
