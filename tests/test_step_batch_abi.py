"""ilm_engine_step_batch / ilm_debug_last_step_batch at the drop-in boundary, without a GPU: the header, the library and the ctypes
binding agree on the two symbols, and the arguments that can be refused before any device work are refused with the documented codes.
What the call computes is held in tests/test_step_batch_gpu.py.
"""
import ctypes as C
import os
import re

from illuminant_amd import abi, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "illuminant_hip.h")
SYMBOLS = ("ilm_engine_step_batch", "ilm_debug_last_step_batch")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_library_and_binding_agree_on_the_symbols():
    text = _header()
    handle = C.CDLL(native.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\bint32_t\s+%s\s*\(" % name, text), "%s is not declared in the header" % name
        assert hasattr(handle, name), "%s is not exported by the library" % name
        assert name in native.SYMBOLS, "%s is not bound by native.SYMBOLS" % name
    # the declared parameter lists are the ones the binding passes
    batch = re.search(r"ilm_engine_step_batch\s*\(([^)]*)\)", text).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in batch.split(",")] == ["IlmHandle", "const IlmHandle*", "const IlmStepDesc*", "int32_t"]
    assert len(native.SYMBOLS["ilm_engine_step_batch"][1]) == 4
    last = re.search(r"ilm_debug_last_step_batch\s*\(([^)]*)\)", text).group(1)
    assert [p.strip().rsplit(" ", 1)[0] for p in last.split(",")] == ["IlmHandle", "int32_t*", "int32_t*", "int32_t*"]
    assert len(native.SYMBOLS["ilm_debug_last_step_batch"][1]) == 4
    assert hasattr(native.Engine, "step_batch") and hasattr(native.Engine, "last_step_batch")


def test_the_batch_kernel_has_a_diagnostic_code_and_the_abi_version_moved():
    defines = dict(re.findall(r"#define (ILM_\w+)\s+(\d+)", open(HEADER).read()))
    assert int(defines["ILM_STEP_KERNEL_BATCH"]) == 5
    assert int(defines["ILM_ABI_VERSION"]) == abi.ABI_VERSION == native.lib().ilm_abi_version() == 11


def test_a_handle_that_is_no_engine_is_refused():
    lib = native.lib()
    handles = (abi.Handle * 1)(0)
    descs = (abi.StepDesc * 1)()
    assert lib.ilm_engine_step_batch(abi.Handle(0), C.cast(handles, C.c_void_p), C.cast(descs, C.c_void_p), 1) == abi.ERR_INVALID_HANDLE
    assert b"engine" in lib.ilm_last_error()
    assert lib.ilm_engine_step_batch(abi.Handle(0), None, None, 0) == abi.ERR_INVALID_HANDLE
    assert lib.ilm_engine_step_batch(abi.Handle(0x1234), C.cast(handles, C.c_void_p), C.cast(descs, C.c_void_p), 1) == abi.ERR_INVALID_HANDLE


def test_a_negative_count_and_missing_arrays_are_refused():
    """The argument checks come before the handle is looked up, so they hold whatever the handle is."""
    lib = native.lib()
    handles = (abi.Handle * 1)(0)
    descs = (abi.StepDesc * 1)()
    for engine in (abi.Handle(0), abi.Handle(0x1234)):
        assert lib.ilm_engine_step_batch(engine, C.cast(handles, C.c_void_p), C.cast(descs, C.c_void_p), -1) == abi.ERR_INVALID_ARGUMENT
        assert b"negative" in lib.ilm_last_error()
        assert lib.ilm_engine_step_batch(engine, None, C.cast(descs, C.c_void_p), 1) == abi.ERR_INVALID_ARGUMENT
        assert lib.ilm_engine_step_batch(engine, C.cast(handles, C.c_void_p), None, 1) == abi.ERR_INVALID_ARGUMENT
        assert lib.ilm_engine_step_batch(engine, None, None, 3) == abi.ERR_INVALID_ARGUMENT
        assert b"NULL" in lib.ilm_last_error()


def test_last_step_batch_of_no_engine_is_refused():
    lib = native.lib()
    a, b, c = C.c_int32(-7), C.c_int32(-7), C.c_int32(-7)
    assert lib.ilm_debug_last_step_batch(abi.Handle(0), C.byref(a), C.byref(b), C.byref(c)) == abi.ERR_INVALID_HANDLE
    assert (a.value, b.value, c.value) == (-7, -7, -7)
    assert lib.ilm_debug_last_step_batch(abi.Handle(0), None, None, None) == abi.ERR_INVALID_HANDLE
