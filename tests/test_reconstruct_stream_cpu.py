"""The reconstructor's streaming device job (sda_secret_reconstructor_begin_dev / update_dev / update_sealed_rows_dev /
finish_dev) as far as a box without a GPU can see it: the symbols, their arity in the header and in the ctypes table, the NULL
checks; that every case of tests/reconstruct_stream_cases.py reconstructs, on the CPU, to the secrets it was shared from; and a
reach proof from a model of the kernel's lockstep - which cases leave the LDS window and take the global fallback."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reconstruct_stream_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sda_secret_reconstructor_begin_dev": 5, "sda_secret_reconstructor_update_dev": 6,
       "sda_secret_reconstructor_update_sealed_rows_dev": 14, "sda_secret_reconstructor_finish_dev": 4}


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
    calls = [lambda: lib.sda_secret_reconstructor_begin_dev(None, None, 4, 1, None),
             lambda: lib.sda_secret_reconstructor_update_dev(None, 0, None, 1, 1, None),
             lambda: lib.sda_secret_reconstructor_update_sealed_rows_dev(None, None, None, key, key, 0, None, 64, None, 1, 64, None, None,
                                                                         None),
             lambda: lib.sda_secret_reconstructor_finish_dev(None, None, 0, None)]
    for call in calls:
        assert call() == capi.ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.sda_last_error()


def test_python_mirror_has_the_device_methods(built):
    from sda_amd import crypto
    for name in ("begin_dev", "update_dev", "update_sealed_rows_dev", "finish_dev", "reconstruct_sealed_job"):
        assert callable(getattr(crypto.SecretReconstructor, name))


@pytest.mark.parametrize("name", [c.name for c in rc.CASES])
def test_every_case_reconstructs_on_the_cpu(built, name):
    """the C oracle on the rows of the case gives the secrets the case was shared from; crafted any-int64 rows are compared with
    Python integers mod q (reconstruct_python), which the oracle must equal on the rows' canonical residues"""
    from oracle import coracle
    case, b = rc.BY_NAME[name], rc.build(name)
    p, k, t, n, w2, w3 = rc.SCHEMES[case.scheme]
    assert b.rows.shape == (len(case.indices), b.batches + case.surplus)
    canon = (b.rows[:, :b.batches].astype(object) % p).astype(np.int64)
    if case.scheme == "additive":
        got = coracle.combine(p, canon)
    else:
        assert len(case.indices) >= t + k and len(set(case.indices)) == len(case.indices)
        got = coracle.packed_reconstruct(p, k, t, w2, w3, case.dim, list(case.indices), canon)
    assert np.array_equal(got, b.want)
    if case.values == "sums":
        assert np.array_equal(b.want, b.secrets_sum) and np.array_equal(rc.reconstruct_python(case, b.rows), b.want)
    else:
        assert (b.rows < 0).any() and (b.rows >= p).any()          # the canonicalising step has work to do


def _reach(name):
    from oracle import coracle
    b = rc.build(name)
    return rc.reach(rc.BY_NAME[name], [coracle.varint_encode(row) for row in b.rows])


def test_reach_the_drift_case_takes_the_global_fallback(built):
    """one-byte rows run ahead of ten-byte rows in the same workgroup: their products land beyond the 2048-column window"""
    r = _reach(rc.DRIFT)
    print(r)
    assert r["beyond"] > 0 and r["window"] > 0
    assert r["groups"] > 1                                          # the ten-byte rows hold the window back for several groups


def test_reach_every_other_case_stays_inside_the_window(built):
    """every case but the drift case and the wide k = 100 case"""
    for c in rc.CASES:
        if c.name not in (rc.DRIFT, rc.WIDE) and c.scheme != "additive":
            r = _reach(c.name)
            assert r["beyond"] == 0, (c.name, r)
            assert r["window"] == len(c.indices) * rc.batches(c) * rc.SCHEMES[c.scheme][1], (c.name, r)


def test_reach_the_wide_case_runs_the_large_k_instance_past_the_window(built):
    """k = 100: the window holds 20 batches, the case has 30, so the global fallback runs in the k > 16 instance too"""
    r = _reach(rc.WIDE)
    print(r)
    assert r["beyond"] >= 255 * 900 and r["window"] == 255 * 3000 - r["beyond"]


def test_reach_the_long_case_crosses_a_chunk_a_group_and_the_wrap(built):
    r = _reach(rc.LONG)
    print(r)
    assert r["chunks"] > 4 and r["groups"] > 1 and r["wrapped"] > 0 and r["beyond"] == 0


def test_reach_model_counts_terminators(built):
    """the model's column rule on a hand-made payload: values end where a byte has its top bit clear"""
    from oracle import coracle
    raw = coracle.varint_encode(np.array([0, -1, 64, 1 << 40, rc.I64_MIN], dtype=np.int64))
    assert list(rc.value_ends(raw)) == [1, 2, 4, 10, 20]
