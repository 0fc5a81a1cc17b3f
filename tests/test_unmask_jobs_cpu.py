"""sda_secret_unmasker_unmask_jobs_dev (receive.rs:148-156 from the two device jobs' sums in one call): what can be checked without
a device - the symbol is exported by the release library and by its twin with the test hooks, the header, the ctypes table and the
mirrors agree on it, NULL handles are refused before anything touches a device, reveal_sealed refuses what it can see on the host,
and the addition left the ABI version alone."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sda_secret_unmasker_unmask_jobs_dev"
PARAMS = ["u", "c", "r", "d_status_masks", "d_status_results", "d_out", "out_cap", "stream"]


def _declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/{header}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_is_exported_by_both_libraries(built):
    import __graft_entry__ as g
    release, test = C.CDLL(g.LIB), C.CDLL(g.TEST_LIB)
    assert hasattr(release, NAME), f"{g.LIB} does not export {NAME}"
    assert hasattr(test, NAME), f"{g.TEST_LIB} does not export {NAME}"


def test_header_and_ctypes_table_declare_it_with_eight_parameters(built):
    from sda_amd import capi
    assert NAME in capi.SIGNATURES and NAME not in capi.HOOK_SIGNATURES
    ret, params = capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(params) == len(PARAMS) == 8
    args = _declaration("sda_hip.h", NAME)
    assert [a.split()[-1] for a in args] == PARAMS
    assert args[0].startswith("sda_secret_unmasker_t*") and args[1].startswith("sda_mask_combiner_t*")
    assert args[2].startswith("sda_secret_reconstructor_t*")
    assert args[3] == "const uint32_t* d_status_masks" and args[4] == "const uint32_t* d_status_results"
    assert args[5] == "int64_t* d_out" and args[6] == "size_t out_cap" and args[7] == "void* stream"
    assert not re.search(r"\b" + NAME + r"\b", open(os.path.join(ROOT, "include", "sda_hip_debug.h")).read())


def test_the_header_states_the_contract(built):
    text = open(os.path.join(ROOT, "include", "sda_hip.h")).read()
    comment = text[:text.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("receive.rs:148-156", "bit for bit", "sodium.rs:78-80", "batched.rs:94", "full.rs:58", "chacha.rs:83", "chacha.rs:58",
                 "SDA_ERR_STATE", "SDA_ERR_ASSERTION", "SDA_ERR_UNSUPPORTED", "SDA_ERR_INVALID_ARGUMENT", "allocates", "NOTHING"):
        assert word in comment, word


def test_the_python_and_cpp_mirrors_name_it(built):
    from sda_amd import crypto
    sig = inspect.signature(crypto.SecretUnmasker.unmask_jobs_dev)
    assert list(sig.parameters) == ["self", "combiner", "reconstructor", "d_out", "out_cap", "d_status_masks", "d_status_results", "stream"]
    assert all(sig.parameters[p].default == 0 for p in ("d_status_masks", "d_status_results", "stream"))
    sig = inspect.signature(crypto.reveal_sealed)
    assert list(sig.parameters) == ["aggregation", "mask_job", "result_job", "indices", "recipient_pk", "recipient_sk"]
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    assert NAME in hpp and re.search(r"\bunmask_jobs\s*\(", hpp)
    shim = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert NAME in shim


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    call = getattr(lib, NAME)
    assert call(None, None, None, None, None, None, 0, None) == bad
    assert b"NULL" in lib.sda_last_error()
    # a None unmasker needs no device: the reconstructor is looked at next, then - for a kind with masks - the combiner
    none = capi.MaskingScheme(capi.MASKING_NONE, 0, 0, 0)
    u = C.c_void_p()
    assert lib.sda_secret_unmasker_new(C.byref(none), C.byref(u)) == capi.OK
    try:
        assert call(u, None, None, None, None, None, 0, None) == bad
        assert b"reconstructor is NULL" in lib.sda_last_error()
    finally:
        lib.sda_secret_unmasker_free(u)
    assert lib.sda_abi_version() == 6


def _aggregation(masking):
    from sda_amd import crypto
    import reconstruct_stream_cases as rc
    p, k, t, n, w2, w3 = rc.SCHEMES["k3_62"]
    return crypto.Aggregation(6, p, masking, crypto.PackedShamir(k, n, t, p, w2, w3))


def test_reveal_sealed_refuses_on_the_host(built):
    """a job that is not SEALED, keys that are not 32 bytes, an index count that is not the row count, a mask job with NoMask and
    none with a masking scheme: SDA_ERR_INVALID_ARGUMENT before a handle that needs a device is made (on a machine without one the
    handles would answer SDA_ERR_NO_DEVICE instead)"""
    from sda_amd import capi, crypto
    import reconstruct_stream_cases as rc
    key = bytes(range(32))
    sealed = bytes(crypto.JobContainer.build(capi.JOB_SEALED, [bytes(64)] * 4))
    varint = bytes(crypto.JobContainer.build(capi.JOB_VARINT, [bytes(8)] * 4))
    full, none = crypto.Full(rc.P62), crypto.NoMask()

    def refused(*args):
        with pytest.raises(crypto.SdaError) as e:
            crypto.reveal_sealed(*args)
        assert e.value.code == capi.ERR_INVALID_ARGUMENT, e.value
        return e.value.message
    assert "SEALED" in refused(_aggregation(full), sealed, varint, rc.SCATTERED, key, key)
    assert "SEALED" in refused(_aggregation(full), varint, sealed, rc.SCATTERED, key, key)
    assert "32 bytes" in refused(_aggregation(full), sealed, sealed, rc.SCATTERED, key[:31], key)
    assert "32 bytes" in refused(_aggregation(full), sealed, sealed, rc.SCATTERED, key, key + b"\0")
    assert "indices" in refused(_aggregation(full), sealed, sealed, rc.SCATTERED[:3], key, key)
    assert "indices" in refused(_aggregation(full), sealed, sealed, None, key, key)
    assert "indices" in refused(_aggregation(none), None, sealed, rc.ALL8, key, key)
    assert "mask job" in refused(_aggregation(full), None, sealed, rc.SCATTERED, key, key)
    assert "mask job" in refused(_aggregation(none), sealed, sealed, rc.SCATTERED, key, key)


def test_the_sealed_job_wrappers_keep_their_texts(built):
    """the feeding code of reconstruct_sealed_job / combine_sealed_job became shared helpers: a job of another kind is still refused
    in their own words"""
    from sda_amd import capi, crypto
    import reconstruct_stream_cases as rc
    varint = bytes(crypto.JobContainer.build(capi.JOB_VARINT, [bytes(8)] * 4))
    src = inspect.getsource(crypto)
    assert src.count("needs a job of sealed boxes (payload kind SEALED)") == 1      # the shared helper's
    with pytest.raises(crypto.SdaError) as e:
        crypto._parse_sealed_job("reconstruct_sealed_job", varint)
    assert e.value.message == "reconstruct_sealed_job needs a job of sealed boxes (payload kind SEALED)"
    with pytest.raises(crypto.SdaError) as e:
        crypto._parse_sealed_job("combine_sealed_job", varint)
    assert e.value.message == "combine_sealed_job needs a job of sealed boxes (payload kind SEALED)"
    for status, code, text in ((16, capi.ERR_SODIUM_DECRYPTION, "Sodium decryption failure"), (18, capi.ERR_SODIUM_DECRYPTION, "Sodium"),
                               (2, capi.ERR_WRONG_DIMENSION, "Wrong dimension"), (6, capi.ERR_WRONG_DIMENSION, "Wrong dimension"),
                               (4, capi.ERR_INVALID_ARGUMENT, "malformed varint stream (status 4)")):
        with pytest.raises(crypto.SdaError) as e:
            crypto._raise_sealed_status(status)
        assert e.value.code == code and text in e.value.message
    crypto._raise_sealed_status(0)
