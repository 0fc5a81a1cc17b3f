"""sda_secret_masker_mask_sealed_rows_dev (participate.rs:52-72 in one call: mask the secrets, seal the mask to the recipient, no
mask in device memory): what can be checked without a device - the symbol is exported by the release library and by its twin with
the test hooks, its seeded twin by the test library only, the header, the ctypes tables and the mirrors agree on it, NULL
handles are refused before anything touches a device, and the addition left the ABI version alone."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sda_secret_masker_mask_sealed_rows_dev"
HOOK = "sda_debug_secret_masker_mask_sealed_rows_seeded_dev"
PARAMS = ["m", "codec", "b", "pk", "esk", "d_secrets", "participants", "len", "secrets_stride", "first_participant", "d_masked",
          "masked_stride", "d_boxes", "slot_bytes", "d_row_bytes", "stream"]


def _declaration(header, name):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/{header}"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_symbol_is_exported_by_both_libraries_and_the_hook_by_the_test_library_only(built):
    import __graft_entry__ as g
    release, test = C.CDLL(g.LIB), C.CDLL(g.TEST_LIB)
    assert hasattr(release, NAME), f"{g.LIB} does not export {NAME}"
    assert hasattr(test, NAME), f"{g.TEST_LIB} does not export {NAME}"
    assert hasattr(test, HOOK), f"{g.TEST_LIB} does not export {HOOK}"
    assert not hasattr(release, HOOK), "the release library carries a test hook"


def test_header_and_ctypes_table_declare_it_with_sixteen_parameters(built):
    from sda_amd import capi
    assert NAME in capi.SIGNATURES and NAME not in capi.HOOK_SIGNATURES
    ret, params = capi.SIGNATURES[NAME]
    assert ret is C.c_int and len(params) == len(PARAMS)
    assert params[9] is C.c_uint64                                  # first_participant is 64 bits wide on every platform
    args = _declaration("sda_hip.h", NAME)
    assert [a.split()[-1].split("[")[0] for a in args] == PARAMS
    assert args[0].startswith("sda_secret_masker_t*") and args[1].startswith("sda_varint_codec_t*") and args[2].startswith("sda_sealedbox_t*")
    assert args[3] == "const uint8_t pk[32]" and args[9] == "uint64_t first_participant" and args[-1] == "void* stream"
    assert args[5].startswith("const int64_t*") and args[10] == "int64_t* d_masked"


def test_the_hook_is_the_same_call_with_seed_words(built):
    from sda_amd import capi
    assert HOOK in capi.HOOK_SIGNATURES and HOOK not in capi.SIGNATURES
    ret, params = capi.HOOK_SIGNATURES[HOOK]
    assert ret is C.c_int and len(params) == len(PARAMS) + 1
    args = _declaration("sda_hip_debug.h", HOOK)
    assert [a.split()[-1].split("[")[0] for a in args] == PARAMS[:1] + ["seed_words"] + PARAMS[1:]
    assert params[10] is C.c_uint64
    assert not re.search(r"\b" + HOOK + r"\b", open(os.path.join(ROOT, "include", "sda_hip.h")).read())


def test_the_python_and_cpp_mirrors_name_it(built):
    from sda_amd import crypto
    sig = inspect.signature(crypto.SecretMasker.mask_sealed_rows_dev)
    assert list(sig.parameters) == ["self", "codec", "box", "recipient_pk", "d_secrets", "participants", "length", "secrets_stride",
                                    "d_masked", "masked_stride", "d_boxes", "slot_bytes", "d_row_bytes", "first_participant", "esk", "stream"]
    assert sig.parameters["first_participant"].default == 0 and sig.parameters["esk"].default is None and sig.parameters["stream"].default == 0
    hpp = open(os.path.join(ROOT, "sda_amd", "host", "sda_crypto.hpp")).read()
    assert NAME in hpp and re.search(r"\bmask_sealed\s*\(", hpp)


def test_participate_sealed_exists(built):
    from sda_amd import crypto
    sig = inspect.signature(crypto.participate_sealed)
    assert list(sig.parameters) == ["aggregation", "secrets_2d", "recipient_pk", "clerk_pks", "first_participant", "mask_esk", "share_esk"]
    assert sig.parameters["first_participant"].default == 0
    assert sig.parameters["mask_esk"].default is None and sig.parameters["share_esk"].default is None


def test_null_handles_are_refused_and_the_abi_version_stays(built):
    from sda_amd import capi
    lib = capi.load()
    bad = capi.ERR_INVALID_ARGUMENT
    key = bytes(32)
    assert getattr(lib, NAME)(None, None, None, key, key, None, 1, 1, 1, 0, None, 1, None, 64, None, None) == bad
    assert b"NULL" in lib.sda_last_error()
    assert getattr(lib, NAME)(None, None, None, None, None, None, 0, 0, 0, 0, None, 0, None, 0, None, None) == bad
    assert lib.sda_abi_version() == 6
