"""The checked reveal (sda_secret_reconstructor_begin_checked_dev / finish_checked_dev / reconstruct_checked,
sda_reconstruct_report_words): what can be checked without a device - the symbols are exported by the release library and by its
twin with the test hooks, the header, the ctypes table and the mirrors declare them, the header states the contract, NULL handles
are refused before anything touches a device, and the addition left the ABI version alone."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN = "sda_secret_reconstructor_begin_checked_dev"
FINISH = "sda_secret_reconstructor_finish_checked_dev"
HOST = "sda_secret_reconstructor_reconstruct_checked"
WORDS = "sda_reconstruct_report_words"
PARAMS = {
    BEGIN: ["r", "indices", "n_rows", "row_len", "checks", "stream"],
    FINISH: ["r", "policy", "d_out", "out_cap", "d_report", "stream"],
    HOST: ["r", "indices", "rows", "row_lens", "n_rows", "checks", "policy", "out", "out_cap", "out_len", "report"],
}


def _header():
    return open(os.path.join(ROOT, "include", "sda_hip.h")).read()


def _declaration(name, ret="int"):
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sda_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_exported_by_both_libraries(built):
    import __graft_entry__ as g
    release, test = C.CDLL(g.LIB), C.CDLL(g.TEST_LIB)
    for name in (BEGIN, FINISH, HOST, WORDS):
        assert hasattr(release, name), f"{g.LIB} does not export {name}"
        assert hasattr(test, name), f"{g.TEST_LIB} does not export {name}"


def test_header_and_ctypes_table_declare_them(built):
    from sda_amd import capi
    for name, params in PARAMS.items():
        assert name in capi.SIGNATURES and name not in capi.HOOK_SIGNATURES
        ret, ctypes_params = capi.SIGNATURES[name]
        assert ret is C.c_int and len(ctypes_params) == len(params), name
        args = _declaration(name)
        assert [a.split()[-1] for a in args] == params, name
        assert args[0] == "sda_secret_reconstructor_t* r"
    assert _declaration(BEGIN)[4] == "unsigned checks" and _declaration(BEGIN)[1] == "const size_t* indices"
    assert _declaration(FINISH)[1] == "int policy" and _declaration(FINISH)[4] == "uint64_t* d_report"
    assert _declaration(HOST)[10] == "uint64_t* report" and _declaration(HOST)[2] == "const int64_t* const* rows"
    assert _declaration(WORDS, "size_t") == ["size_t n_rows"] and capi.SIGNATURES[WORDS] == (C.c_size_t, [C.c_size_t])
    text = _header()
    assert re.search(r"#define\s+SDA_RECONSTRUCT_MAX_CHECKS\s+16\b", text)
    assert re.search(r"#define\s+SDA_CHECK_REPORT\s+0\b", text) and re.search(r"#define\s+SDA_CHECK_CORRECT\s+1\b", text)
    assert (capi.CHECK_REPORT, capi.CHECK_CORRECT, capi.RECONSTRUCT_MAX_CHECKS) == (0, 1, 16)
    debug = open(os.path.join(ROOT, "include", "sda_hip_debug.h")).read()
    assert not any(re.search(r"\b" + n + r"\b", debug) for n in PARAMS)


def test_the_header_states_the_contract(built):
    text = _header()
    comment = text[:text.index("#define SDA_RECONSTRUCT_MAX_CHECKS")].rsplit("/*", 1)[1]
    for word in ("Reed-Solomon", "limits", "DETECTED", "never attributed", "MAY be attributed", "sodium.rs:78-80", "batched.rs:94",
                 "bit for bit", "SDA_ERR_STATE", "SDA_ERR_UNSUPPORTED", "SDA_ERR_INVALID_ARGUMENT", "SDA_ERR_NOT_ENOUGH_SHARES",
                 "SDA_ERR_ASSERTION", "n_rows == t + k", "blamed position", "POSITION", "*d_status", "NO SYNCHRONISATION",
                 "deterministic", "[4 + i]", "2^64 - 1", "checks == 1"):
        assert word in comment, word


def test_the_mirrors_name_them(built):
    from sda_amd import crypto
    R = crypto.SecretReconstructor
    assert list(inspect.signature(R.begin_checked_dev).parameters) == ["self", "indices", "n_rows", "row_len", "checks", "stream"]
    assert list(inspect.signature(R.finish_checked_dev).parameters) == ["self", "d_out", "out_cap", "d_report", "correct", "stream"]
    assert list(inspect.signature(R.reconstruct_checked).parameters) == ["self", "indexed_shares", "checks", "correct"]
    sig = inspect.signature(R.reconstruct_sealed_job_checked)
    assert list(sig.parameters) == ["self", "blob", "indices", "pk", "sk", "checks", "correct"]
    assert sig.parameters["checks"].default is None and sig.parameters["correct"].default is False
    sig = inspect.signature(crypto.reveal_sealed_checked)
    assert list(sig.parameters) == ["aggregation", "mask_job", "result_job", "indices", "recipient_pk", "recipient_sk", "checks", "correct"]
    assert sig.parameters["checks"].default is None and sig.parameters["correct"].default is False
    # the existing forms keep their parameter lists
    assert list(inspect.signature(crypto.reveal_sealed).parameters) == ["aggregation", "mask_job", "result_job", "indices", "recipient_pk",
                                                                        "recipient_sk"]
    assert list(inspect.signature(R.begin_dev).parameters) == ["self", "indices", "n_rows", "row_len", "stream"]
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    shim = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in (BEGIN, FINISH, HOST):
        assert name in hpp and name in shim, name
    assert WORDS in shim
    for method in ("begin_checked_dev", "finish_checked_dev", "reconstruct_checked"):
        assert re.search(r"\b" + method + r"\s*\(", hpp), method
    for doc, word in (("README.md", BEGIN), ("CHANGELOG.md", FINISH), ("DESIGN.md", "reveal_check_finish_kernel")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_reveal_check_tuple():
    from sda_amd import crypto
    c = crypto.RevealCheck.from_words([0, 0, 0, (1 << 64) - 1, 0, 0, 0])
    assert c.clean and c.first_bad is None and c.blame == (0, 0, 0) and c._fields == ("bad", "located", "corrected", "first_bad", "blame")
    c = crypto.RevealCheck.from_words([5, 4, 4, 17, 0, 4, 0, 0])
    assert not c.clean and (c.bad, c.located, c.corrected, c.first_bad, c.blame) == (5, 4, 4, 17, (0, 4, 0, 0))
    assert crypto.RevealCheck.from_words([1, 0, 0, -1 & 0xFFFFFFFFFFFFFFFF]).first_bad is None


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    idx = (C.c_size_t * 8)(*range(8))
    assert lib.sda_secret_reconstructor_begin_checked_dev(None, idx, 8, 1, 1, None) == bad
    assert b"NULL" in lib.sda_last_error()
    assert lib.sda_secret_reconstructor_finish_checked_dev(None, 0, None, 0, None, None) == bad
    assert b"NULL" in lib.sda_last_error()
    n = C.c_size_t(7)
    assert lib.sda_secret_reconstructor_reconstruct_checked(None, idx, None, None, 0, 1, 0, None, 0, C.byref(n), None) == bad
    assert b"NULL" in lib.sda_last_error()
    for rows in (0, 1, 8, 260, 65535):
        assert lib.sda_reconstruct_report_words(rows) == 4 + rows
    assert lib.sda_abi_version() == 6


def test_reveal_sealed_checked_refuses_on_the_host(built):
    """what reveal_sealed refuses on the host, and an additive scheme, before a handle that needs a device is made"""
    from sda_amd import capi, crypto
    import reconstruct_stream_cases as rc
    p, k, t, n, w2, w3 = rc.SCHEMES["k3_62"]
    key = bytes(range(32))
    sealed = bytes(crypto.JobContainer.build(capi.JOB_SEALED, [bytes(64)] * 8))
    varint = bytes(crypto.JobContainer.build(capi.JOB_VARINT, [bytes(8)] * 8))
    packed = crypto.Aggregation(6, p, crypto.Full(p), crypto.PackedShamir(k, n, t, p, w2, w3))
    additive = crypto.Aggregation(6, p, crypto.Full(p), crypto.Additive(8, p))

    def refused(code, *args):
        with pytest.raises(crypto.SdaError) as e:
            crypto.reveal_sealed_checked(*args)
        assert e.value.code == code, e.value
        return e.value.message
    bad = capi.ERR_INVALID_ARGUMENT
    assert "SEALED" in refused(bad, packed, sealed, varint, rc.ALL8, key, key)
    assert "32 bytes" in refused(bad, packed, sealed, sealed, rc.ALL8, key[:31], key)
    assert "indices" in refused(bad, packed, sealed, sealed, rc.SCATTERED, key, key)
    assert "indices" in refused(bad, packed, sealed, sealed, None, key, key)
    assert "mask job" in refused(bad, packed, None, sealed, rc.ALL8, key, key)
    assert "redundancy" in refused(capi.ERR_UNSUPPORTED, additive, sealed, sealed, None, key, key)
