"""sda_share_generator_generate_sealed_rows_dev (participate.rs:75-101 in one call: share the secrets and seal every clerk's
vector, no share in device memory): what can be checked without a device - the symbol is exported by the release library and
by its twin with the test hooks, the header, the ctypes table and the library agree on it, NULL handles are refused before
anything touches a device, and the addition left the ABI version alone."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sda_share_generator_generate_sealed_rows_dev"
PARAMS = ["g", "codec", "b", "pks", "esk", "d_secrets", "participants", "len", "secrets_stride", "first_participant", "d_boxes",
          "slot_bytes", "d_row_bytes", "stream"]


def test_symbol_is_exported_by_both_libraries(built):
    import __graft_entry__ as g
    for path in (g.LIB, g.TEST_LIB):
        so = C.CDLL(path)
        assert hasattr(so, NAME), f"{path} does not export {NAME}"


def test_header_and_ctypes_table_declare_it_with_fourteen_parameters(built):
    from sda_amd import capi
    assert NAME in capi.SIGNATURES
    ret, params = capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(params) == len(PARAMS)
    assert params[9] is C.c_uint64                                  # first_participant is 64 bits wide on every platform
    text = open(os.path.join(ROOT, "include", "sda_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", text)
    assert m, "not declared in include/sda_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.split()[-1] for a in args] == PARAMS
    assert args[0].startswith("sda_share_generator_t*") and args[1].startswith("sda_varint_codec_t*") and args[2].startswith("sda_sealedbox_t*")
    assert args[9] == "uint64_t first_participant" and args[-1] == "void* stream"


def test_the_python_and_cpp_mirrors_name_it(built):
    from sda_amd import crypto
    assert callable(crypto.ShareGenerator.generate_sealed_rows_dev)
    assert NAME in open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    key = bytes(32)
    assert getattr(lib, NAME)(None, None, None, key, key, None, 1, 1, 1, 0, None, 64, None, None) == bad
    assert b"NULL" in lib.sda_last_error()
    assert getattr(lib, NAME)(None, None, None, None, None, None, 0, 0, 0, 0, None, 0, None, None) == bad
    assert lib.sda_abi_version() == 6
