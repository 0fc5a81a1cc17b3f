"""The decoding finish of the checked reveal (sda_secret_reconstructor_finish_decoded_dev / reconstruct_decoded,
sda_reconstruct_decode_report_words): what can be checked without a device - both libraries export the symbols, the header, the
ctypes table and the mirrors declare them, the header states the contract, NULL handles are refused before anything touches a
device, the ABI version is still 6, RevealDecode reads the report words - and the lane decoder itself, which is host + device code
(sda_amd/csrc/reveal_decode.hpp), run on the CPU by tests/cpp/reveal_decode_host.cpp on planted error patterns."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINISH = "sda_secret_reconstructor_finish_decoded_dev"
HOST = "sda_secret_reconstructor_reconstruct_decoded"
WORDS = "sda_reconstruct_decode_report_words"
PARAMS = {
    FINISH: ["r", "max_errors", "policy", "d_out", "out_cap", "d_report", "stream"],
    HOST: ["r", "indices", "rows", "row_lens", "n_rows", "checks", "max_errors", "policy", "out", "out_cap", "out_len", "report"],
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
    for name in (FINISH, HOST, WORDS):
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
    assert _declaration(FINISH)[1] == "unsigned max_errors" and _declaration(FINISH)[2] == "int policy"
    assert _declaration(FINISH)[5] == "uint64_t* d_report"
    assert _declaration(HOST)[5:8] == ["unsigned checks", "unsigned max_errors", "int policy"] and _declaration(HOST)[11] == "uint64_t* report"
    assert _declaration(WORDS, "size_t") == ["size_t n_rows"] and capi.SIGNATURES[WORDS] == (C.c_size_t, [C.c_size_t])
    debug = open(os.path.join(ROOT, "include", "sda_hip_debug.h")).read()
    assert not any(re.search(r"\b" + n + r"\b", debug) for n in (FINISH, HOST, WORDS))


def test_the_header_states_the_contract(built):
    text = _header()
    comment = text[:text.index("size_t " + WORDS)].rsplit("/*", 1)[1]
    for word in ("Reed-Solomon", "limits", "DECODED WITH nu POSITIONS", "unique", "Vandermonde", "Berlekamp-Massey", "max_errors == 0",
                 "floor(checks / 2)", "checks < 2", "SDA_ERR_STATE", "SDA_ERR_INVALID_ARGUMENT", "before any launch", "NO SYNCHRONISATION",
                 "bit for bit", "n_rows - nu", "16 + n_rows", "[4] the first UNDECODED", "2^64 - 1", "[8 + nu - 1]", "[16 + i]", "POSITION",
                 "once", "deterministic", "decoded and corrected exactly", "e + 1 .. checks - e", "always DETECTED", "never mis-corrected",
                 "MAY be decoded to wrong positions", "lower cap buys detection margin", "blamed position", "*d_status", "sodium.rs:78-80",
                 "batched.rs:94"):
        assert word in comment, word


def test_the_mirrors_name_them(built):
    from sda_amd import crypto
    R = crypto.SecretReconstructor
    assert list(inspect.signature(R.finish_decoded_dev).parameters) == ["self", "d_out", "out_cap", "d_report", "max_errors", "correct", "stream"]
    assert list(inspect.signature(R.reconstruct_decoded).parameters) == ["self", "indexed_shares", "checks", "max_errors", "correct"]
    sig = inspect.signature(R.reconstruct_sealed_job_decoded)
    assert list(sig.parameters) == ["self", "blob", "indices", "pk", "sk", "checks", "max_errors", "correct"]
    assert sig.parameters["checks"].default is None and sig.parameters["max_errors"].default == 0 and sig.parameters["correct"].default is False
    sig = inspect.signature(crypto.reveal_sealed_decoded)
    assert list(sig.parameters) == ["aggregation", "mask_job", "result_job", "indices", "recipient_pk", "recipient_sk", "checks", "max_errors",
                                    "correct"]
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    shim = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in (FINISH, HOST, WORDS):
        assert name in hpp and name in shim, name
    for method in ("finish_decoded_dev", "reconstruct_decoded"):
        assert re.search(r"\b" + method + r"\s*\(", hpp), method
    for doc, word in (("README.md", FINISH), ("CHANGELOG.md", FINISH), ("DESIGN.md", "reveal_decode_finish_kernel")):
        assert word in open(os.path.join(ROOT, doc)).read(), (doc, word)


def test_reveal_decode_tuple():
    from sda_amd import crypto
    none = (1 << 64) - 1
    d = crypto.RevealDecode.from_words([0, 0, 0, none, none, 0, 0, 0] + [0] * 8 + [0, 0, 0])
    assert d.clean and d.first_bad is None and d.first_undecoded is None and d.blame == (0, 0, 0) and d.by_count == (0,) * 8
    assert d._fields == ("bad", "decoded", "corrected", "first_bad", "first_undecoded", "most", "by_count", "blame")
    d = crypto.RevealDecode.from_words([7, 5, 5, 2, 9, 3, 0, 0, 1, 2, 2, 0, 0, 0, 0, 0, 5, 4, 0, 2])
    assert not d.clean and (d.bad, d.decoded, d.corrected, d.first_bad, d.first_undecoded, d.most) == (7, 5, 5, 2, 9, 3)
    assert d.by_count == (1, 2, 2, 0, 0, 0, 0, 0) and d.blame == (5, 4, 0, 2) and d.undecoded == 2
    assert sum((i + 1) * n for i, n in enumerate(d.by_count)) == sum(d.blame)
    assert crypto.RevealDecode.from_words([1, 0, 0, 0, -1 & none, 0, 0, 0] + [0] * 8).first_undecoded is None


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    idx = (C.c_size_t * 8)(*range(8))
    assert lib.sda_secret_reconstructor_finish_decoded_dev(None, 0, 0, None, 0, None, None) == bad
    assert b"NULL" in lib.sda_last_error()
    n = C.c_size_t(7)
    assert lib.sda_secret_reconstructor_reconstruct_decoded(None, idx, None, None, 0, 2, 0, 0, None, 0, C.byref(n), None) == bad
    assert b"NULL" in lib.sda_last_error()
    for rows in (0, 1, 8, 260, 65535):
        assert lib.sda_reconstruct_decode_report_words(rows) == 16 + rows
        assert lib.sda_reconstruct_report_words(rows) == 4 + rows
    assert lib.sda_abi_version() == 6


def test_reveal_sealed_decoded_refuses_on_the_host(built):
    from sda_amd import capi, crypto
    import pytest
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
            crypto.reveal_sealed_decoded(*args)
        assert e.value.code == code and word in e.value.message, e.value


def test_the_lane_decoder_on_the_cpu(built, tmp_path):
    """the functions the kernel inlines, compiled for the host: planted positions and magnitudes come back for every nu <= e, the
    band e + 1 .. c - e is refused, over four primes up to 2^62 - 57 and committees of 8 .. 260 rows"""
    exe = str(tmp_path / "reveal_decode_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "sda_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "reveal_decode_host.cpp"), "-o", exe], check=True, timeout=300)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-2000:]
    assert run.stdout.count("decoded as planted") == 10 and "FAILURES" not in run.stdout
    assert run.stdout.count("steered batches as constructed") == 10                       # ... and the steered families on every shape
