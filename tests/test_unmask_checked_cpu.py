"""sda_secret_unmasker_unmask_checked_jobs_dev (the recipient's last step on a CHECKED reconstructor job, in one call): what can be
checked without a device - the symbol is exported by the release library and by its twin with the test hooks, the header declares
it and writes its refusal order out, the ctypes table and the Python and C++ mirrors agree on its parameters, NULL handles are
refused before anything touches a device, the ABI version stays 6, and the header still says that unmask_jobs_dev keeps refusing
checked jobs."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sda_secret_unmasker_unmask_checked_jobs_dev"
PARAMS = ["u", "c", "r", "end", "d_ok", "max_errors", "policy", "d_status_masks", "d_status_results", "results_pass_bits", "d_out", "out_cap",
          "d_report", "stream"]
MIRROR = ["combiner", "reconstructor", "end", "d_out", "out_cap", "d_report", "d_ok", "max_errors", "correct", "d_status_masks",
          "d_status_results", "results_pass_bits", "stream"]


def _header():
    return open(os.path.join(ROOT, "include", "sda_hip.h")).read()


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sda_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_is_exported_by_both_libraries(built):
    import __graft_entry__ as g
    release, test = C.CDLL(g.LIB), C.CDLL(g.TEST_LIB)
    assert hasattr(release, NAME), f"{g.LIB} does not export {NAME}"
    assert hasattr(test, NAME), f"{g.TEST_LIB} does not export {NAME}"


def test_header_and_ctypes_table_declare_it(built):
    from sda_amd import capi
    assert NAME in capi.SIGNATURES and NAME not in capi.HOOK_SIGNATURES
    ret, params = capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(params) == len(PARAMS) == 14
    args = _declaration(NAME)
    assert [a.split()[-1] for a in args] == PARAMS
    assert args[0].startswith("sda_secret_unmasker_t*") and args[1].startswith("sda_mask_combiner_t*")
    assert args[2].startswith("sda_secret_reconstructor_t*")
    assert args[3:7] == ["int end", "const uint32_t* d_ok", "unsigned max_errors", "int policy"]
    assert args[7:10] == ["const uint32_t* d_status_masks", "const uint32_t* d_status_results", "uint32_t results_pass_bits"]
    assert args[10:] == ["int64_t* d_out", "size_t out_cap", "uint64_t* d_report", "void* stream"]
    assert params[3] is C.c_int and params[5] is C.c_uint and params[6] is C.c_int and params[9] is C.c_uint32 and params[11] is C.c_size_t
    text = _header()
    for i, end in enumerate(("LOCATE", "DECODE", "ERASURES")):
        assert re.search(r"#define\s+SDA_CHECKED_END_" + end + r"\s+" + str(i) + r"\b", text)
    assert (capi.CHECKED_END_LOCATE, capi.CHECKED_END_DECODE, capi.CHECKED_END_ERASURES) == (0, 1, 2)
    assert not re.search(r"\b" + NAME + r"\b", open(os.path.join(ROOT, "include", "sda_hip_debug.h")).read())


def test_the_header_writes_the_refusal_order_out(built):
    text = _header()
    comment = text[:text.index("#define SDA_CHECKED_END_LOCATE")].rsplit("/*", 1)[1]           # the three #defines sit before the declaration
    assert "IN THIS ORDER" in comment
    order = ["1. those of unmask_jobs_dev", "2. an unknown `end`", "3. those of the named finish", "4. the mask job not begun",
             "5. SDA_VALUES_RUST_SIGNED", "6. Full / ChaCha with a mask job dimension other than L", "7. results_pass_bits"]
    at = [comment.find(step) for step in order]
    assert all(a >= 0 for a in at) and at == sorted(at), at
    steps = re.split(r"\n \*     \d\. ", comment)[1:]
    for step, code in zip(steps, ("SDA_ERR_STATE", "SDA_ERR_INVALID_ARGUMENT", "SDA_ERR_STATE", "SDA_ERR_STATE", "SDA_ERR_UNSUPPORTED",
                                  "SDA_ERR_ASSERTION", "SDA_ERR_INVALID_ARGUMENT")):
        assert code in step, (code, step)
    for word in ("bit for bit", "sodium.rs:78-80", "batched.rs:94", "full.rs:60-63", "chacha.rs:86-89", "WHETHER OR NOT THE GATE IS SHUT",
                 "results_pass_bits is 0, or 16", "no mask sum at or beyond L is read", "one kernel for LOCATE and DECODE, two for ERASURES",
                 "NO SYNCHRONISATION AND NO COPY TO THE HOST", "L == 0 is SDA_OK"):
        assert word in comment, word


def test_unmask_jobs_dev_still_refuses_checked_jobs(built):
    text = _header()
    assert "sda_secret_unmasker_unmask_jobs_dev keeps refusing checked jobs" in text
    assert "sda_secret_unmasker_unmask_jobs_dev on a checked job -> SDA_ERR_UNSUPPORTED" in text
    src = open(os.path.join(ROOT, "sda_amd", "csrc", "sda_capi.cpp")).read()
    assert "unmask_jobs_dev reads a plain job's sums: a checked job takes" in src


def test_the_python_and_cpp_mirrors_agree_on_the_parameters(built):
    from sda_amd import crypto
    sig = inspect.signature(crypto.SecretUnmasker.unmask_checked_jobs_dev)
    assert list(sig.parameters) == ["self"] + MIRROR
    defaults = {p: sig.parameters[p].default for p in MIRROR[6:]}
    assert defaults == {"d_ok": 0, "max_errors": 0, "correct": False, "d_status_masks": 0, "d_status_results": 0, "results_pass_bits": 0, "stream": 0}
    assert all(sig.parameters[p].default is inspect.Parameter.empty for p in MIRROR[:6])
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    m = re.search(r"void\s+unmask_checked_jobs_dev\s*\(([^)]*)\)", hpp)
    assert m and NAME in hpp
    cpp = [re.sub(r"\s*=.*", "", a).split()[-1].lstrip("*&") for a in m.group(1).split(",")]
    assert cpp == MIRROR
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the three reveals kept their signatures
    assert list(inspect.signature(crypto.reveal_sealed_checked).parameters)[-2:] == ["checks", "correct"]
    assert list(inspect.signature(crypto.reveal_sealed_decoded).parameters)[-3:] == ["checks", "max_errors", "correct"]
    assert list(inspect.signature(crypto.reveal_sealed_repaired).parameters)[-3:] == ["checks", "max_errors", "correct"]


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    call = getattr(lib, NAME)
    assert call(None, None, None, 0, None, 0, 0, None, None, 0, None, 0, None, None) == bad
    assert b"unmasker is NULL" in lib.sda_last_error()
    # a None unmasker needs no device: the reconstructor is looked at next, before `end` (7 is none) and the pass bits (5 is neither)
    none = capi.MaskingScheme(capi.MASKING_NONE, 0, 0, 0)
    u = C.c_void_p()
    assert lib.sda_secret_unmasker_new(C.byref(none), C.byref(u)) == capi.OK
    try:
        assert call(u, None, None, 7, None, 0, 0, None, None, 5, None, 0, None, None) == bad
        assert b"reconstructor is NULL" in lib.sda_last_error()
    finally:
        lib.sda_secret_unmasker_free(u)
    assert lib.sda_abi_version() == 6
