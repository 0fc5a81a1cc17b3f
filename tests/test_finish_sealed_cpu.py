"""sda_share_combiner_finish_sealed_rows_dev (clerk.rs:84-100 in one call: the clerk sums reduced, varint encoded and sealed to
the recipient, every row split over the chip, no plaintext result in device memory): what can be checked without a device - the
symbol is exported by the release library and by its twin with the test hooks, the header, the ctypes table and the mirrors agree
on its nine parameters, NULL handles are refused before anything touches a device, and the addition left the ABI version alone."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sda_share_combiner_finish_sealed_rows_dev"
PARAMS = ["c", "codec", "b", "pk[32]", "esk", "d_boxes", "slot_bytes", "d_row_bytes", "stream"]


def test_symbol_is_exported_by_both_libraries(built):
    import __graft_entry__ as g
    for path in (g.LIB, g.TEST_LIB):
        so = C.CDLL(path)
        assert hasattr(so, NAME), f"{path} does not export {NAME}"


def test_header_and_ctypes_table_declare_it_with_nine_parameters(built):
    from sda_amd import capi
    assert NAME in capi.SIGNATURES
    ret, params = capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(params) == len(PARAMS) == 9
    assert params[6] is C.c_size_t
    text = open(os.path.join(ROOT, "include", "sda_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", text)
    assert m, "not declared in include/sda_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1] for a in args] == PARAMS
    assert args[0].startswith("sda_share_combiner_t*") and args[1].startswith("sda_varint_codec_t*") and args[2].startswith("sda_sealedbox_t*")
    assert args[3] == "const uint8_t pk[32]" and args[4] == "const uint8_t* esk" and args[5] == "uint8_t* d_boxes"
    assert args[6] == "size_t slot_bytes" and args[7] == "uint64_t* d_row_bytes" and args[-1] == "void* stream"
    # the definition takes the same nine, in the same order
    src = open(os.path.join(ROOT, "sda_amd", "csrc", "sda_capi.cpp")).read()
    d = re.search(r'extern "C" int ' + NAME + r"\s*\(([^)]*)\)\s*\{", src)
    assert d and [" ".join(a.split()) for a in d.group(1).split(",")] == args


def test_the_python_and_cpp_mirrors_name_it(built):
    import inspect
    from sda_amd import crypto
    assert callable(crypto.ShareCombiner.finish_sealed_rows_dev) and callable(crypto.ShareCombiner.clerk_sealed_job)
    assert list(inspect.signature(crypto.ShareCombiner.clerk_sealed_job).parameters) == ["self", "blob", "pk", "sk", "recipient_pk", "dimension", "esk"]
    assert list(inspect.signature(crypto.ShareCombiner.finish_sealed_rows_dev).parameters)[:7] == \
        ["self", "codec", "box", "recipient_pk", "d_boxes", "slot_bytes", "d_row_bytes"]
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    call = re.search(NAME + r"\(([^;]*)\)\);", hpp)
    assert call and len(call.group(1).split(",")) == 9
    for doc in ("DESIGN.md", "README.md", "CHANGELOG.md", "include/sda_hip.h"):
        assert NAME in open(os.path.join(ROOT, doc)).read(), doc


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    key = bytes(32)
    assert getattr(lib, NAME)(None, None, None, key, key, None, 64, None, None) == bad
    assert b"NULL" in lib.sda_last_error()
    assert getattr(lib, NAME)(None, None, None, None, None, None, 0, None, None) == bad
    assert lib.sda_abi_version() == 6
