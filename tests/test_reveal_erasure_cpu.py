"""The erasure finish of the checked reveal (sda_secret_reconstructor_finish_erasures_dev / reconstruct_erasures): what can be
checked without a device - both libraries export the symbols, the header, the ctypes table and the mirrors declare them, the header
states the contract and keeps the reference's rule, what is refused before anything touches a device (a handle needs one, so that
is the NULL arguments: order, codes, texts), the ABI version is still 6 - and the lane decoder's erasure steps, host + device code
(sda_amd/csrc/reveal_decode.hpp), run on the CPU by tests/cpp/reveal_erasure_host.cpp, plain and under the sanitizers."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINISH = "sda_secret_reconstructor_finish_erasures_dev"
HOST = "sda_secret_reconstructor_reconstruct_erasures"
PARAMS = {
    FINISH: ["r", "d_ok", "max_errors", "policy", "d_out", "out_cap", "d_report", "stream"],
    HOST: ["r", "indices", "rows", "row_lens", "n_rows", "checks", "erased", "max_errors", "policy", "out", "out_cap", "out_len", "report"],
}


def _header():
    return open(os.path.join(ROOT, "include", "sda_hip.h")).read()


def _declaration(name):
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/sda_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbols_are_exported_by_both_libraries(built):
    import __graft_entry__ as g
    release, test = C.CDLL(g.LIB), C.CDLL(g.TEST_LIB)
    for name in (FINISH, HOST):
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
    assert _declaration(FINISH)[1:4] == ["const uint32_t* d_ok", "unsigned max_errors", "int policy"]
    assert _declaration(FINISH)[6] == "uint64_t* d_report"
    assert _declaration(HOST)[5:9] == ["unsigned checks", "const uint8_t* erased", "unsigned max_errors", "int policy"]
    debug = open(os.path.join(ROOT, "include", "sda_hip_debug.h")).read()
    assert not any(re.search(r"\b" + n + r"\b", debug) for n in (FINISH, HOST))


def test_the_header_states_the_contract(built):
    text = _header()
    comment = text[:text.index("int " + FINISH)].rsplit("/* The ERASURE finish", 1)[1]
    comment = " ".join(re.sub(r"\n \*", " ", comment).split())               # one line: the words, not where the lines break
    for word in ("MODIFIED SYNDROMES", "T_j = sum_m gamma_m S_{j+m}", "Gamma(z) = prod_{j in F} (z - x_j)", "WHATEVER THEY ADDED",
                 "CONSISTENT", "DECODED WITH nu POSITIONS", "NON-ERASED", "Vandermonde", "Y_i = Z_i / Gamma(x_i)", "checks == 1 is accepted",
                 "floor(checks / 2)", "SDA_ERR_STATE", "same order", "0 = erased", "NULL = none", "d_ok + first_pos", "never learns f",
                 "does not synchronise", "bit for bit", "n_rows - f - nu", "[6] = f", "[7] = 1 when f > checks", "an erased position stays 0",
                 "is not counted", "f = c detects nothing", "e' + 1 .. c - f - e'", "sodium.rs:78-80", "*d_status", "THE REFERENCE'S RULE STANDS",
                 "not a replacement", "sda_secret_unmasker_unmask_jobs_dev keeps refusing"):
        assert word in comment, word
    # the paragraphs of the sibling finishes still say what the reference does with a refused box
    assert text.count("sodium.rs:78-80") >= 3


def test_the_mirrors_name_them(built):
    from sda_amd import crypto
    R = crypto.SecretReconstructor
    assert list(inspect.signature(R.finish_erasures_dev).parameters) == ["self", "d_ok", "d_out", "out_cap", "d_report", "max_errors", "correct",
                                                                          "stream"]
    assert list(inspect.signature(R.reconstruct_erasures).parameters) == ["self", "indexed_shares", "erased", "checks", "max_errors", "correct"]
    sig = inspect.signature(crypto.reveal_sealed_repaired)
    assert list(sig.parameters) == ["aggregation", "mask_job", "result_job", "indices", "recipient_pk", "recipient_sk", "checks", "max_errors",
                                    "correct"]
    assert crypto.RevealRepair._fields == ("output", "decode", "status", "refused", "unrepaired")
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    shim = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in (FINISH, HOST):
        assert name in hpp and name in shim, name
    for method in ("finish_erasures_dev", "reconstruct_erasures"):
        assert re.search(r"\b" + method + r"\s*\(", hpp), method
    for doc, word in (("README.md", FINISH), ("CHANGELOG.md", FINISH), ("DESIGN.md", "reveal_erasure_finish_kernel"),
                      ("DESIGN.md", "reveal_erasure_setup_kernel")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_null_arguments_are_refused_in_order_and_the_abi_version_stays(built):
    """the refusals that need no device, with their codes and texts: the handle comes first in the device form, the handle and
    out_len first in the host form, then the rows"""
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    idx = (C.c_size_t * 8)(*range(8))
    flags = bytes(8)
    n = C.c_size_t(7)
    fin, host = getattr(lib, FINISH), getattr(lib, HOST)
    # every other argument bad as well: the NULL handle is what is named
    assert fin(None, None, 99, 7, None, 0, None, None) == bad
    assert lib.sda_last_error() == b"reconstructor is NULL"
    assert lib.sda_secret_reconstructor_finish_decoded_dev(None, 99, 7, None, 0, None, None) == bad
    assert lib.sda_last_error() == b"reconstructor is NULL", "the sibling's text"
    assert host(None, idx, None, None, 8, 99, flags, 99, 7, None, 0, C.byref(n), None) == bad
    assert lib.sda_last_error() == b"NULL argument" and n.value == 7
    assert host(None, idx, None, None, 8, 4, flags, 0, 0, None, 0, None, None) == bad
    assert lib.sda_last_error() == b"NULL argument"
    assert lib.sda_abi_version() == 6
    assert lib.sda_reconstruct_decode_report_words(26) == 42


def test_reveal_sealed_repaired_refuses_on_the_host(built):
    from sda_amd import capi, crypto
    import reconstruct_stream_cases as rc
    p, k, t, n, w2, w3 = rc.SCHEMES["k3_62"]
    key = bytes(range(32))
    sealed = bytes(crypto.JobContainer.build(capi.JOB_SEALED, [bytes(64)] * 8))
    varint = bytes(crypto.JobContainer.build(capi.JOB_VARINT, [bytes(8)] * 8))
    packed = crypto.Aggregation(6, p, crypto.Full(p), crypto.PackedShamir(k, n, t, p, w2, w3))
    additive = crypto.Aggregation(6, p, crypto.Full(p), crypto.Additive(8, p))
    for code, word, args in ((capi.ERR_INVALID_ARGUMENT, "SEALED", (packed, sealed, varint, rc.ALL8, key, key)),
                             (capi.ERR_INVALID_ARGUMENT, "indices", (packed, sealed, sealed, None, key, key)),
                             (capi.ERR_UNSUPPORTED, "redundancy", (additive, sealed, sealed, None, key, key))):
        with pytest.raises(crypto.SdaError) as e:
            crypto.reveal_sealed_repaired(*args)
        assert e.value.code == code and word in e.value.message, e.value
    # the default path is what it was: reveal_sealed_decoded has no new parameter
    assert "repair" not in " ".join(inspect.signature(crypto.reveal_sealed_decoded).parameters)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_the_erasure_steps_on_the_cpu(built, tmp_path, flags):
    """the functions the two kernels inline, compiled for the host as a stand-alone program: planted erased and faulty positions come
    back with their magnitudes for every f <= c and nu <= floor((c - f) / 2), the band above is refused, over four primes up to
    2^62 - 57 and committees of 8 .. 260 rows; once plain, once under UBSan + ASan as a plain executable"""
    exe = str(tmp_path / "reveal_erasure_host")
    subprocess.run(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "sda_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "reveal_erasure_host.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout, run.stderr[-2000:])
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.count("repaired as planted") == 9 and "FAILURES" not in run.stdout and "runtime error" not in run.stderr
    assert run.stdout.count("steered batches undecoded as constructed") == 9             # ... and the steered families on every shape
