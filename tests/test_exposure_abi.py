"""include/hrcore_exposure.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, both structs have the layout gcc gives them, no other header's version
moved, the library's defaults are the binding's, calls without a context fail loudly, and an Engine bound to a library without the
symbols (the CPU oracle) still constructs."""
import ctypes
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, exposure

HEADER = "hrcore_exposure.h"
NAMES = ["hr_exposure_api_version", "hr_exposure_default_params", "hr_exposure_meter", "hr_exposure_display", "hr_exposure_last", "hr_exposure_reset"]


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.EXPOSURE_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in abi_checks.HEADERS:
        assert not set(ffi.EXPOSURE_SYMBOLS) & set(abi_checks.symbols(header)), header
        assert "hrcore_exposure" not in abi_checks.header_text(header), header
    assert not set(ffi.EXPOSURE_SYMBOLS) & set(ffi.TREE_SYMBOLS)
    lib = core.load_library()
    for s in ffi.EXPOSURE_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_exposure_api_version.restype = ctypes.c_uint32
    assert lib.hr_exposure_api_version() == ffi.HR_EXPOSURE_API_VERSION == 1
    assert ffi.FEATURES["exposure"] == (ffi.EXPOSURE_SYMBOLS, ffi.HR_EXPOSURE_API_VERSION, "auto-exposure")
    abi_checks.check_no_version_moved()


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_EXPOSURE_API_VERSION (\d+)u", text)[0]) == ffi.HR_EXPOSURE_API_VERSION
    assert int(re.findall(r"#define HR_EXPOSURE_BINS (\d+)", text)[0]) == ffi.HR_EXPOSURE_BINS == 256
    for name in ("EMPTY", "CLAMPED_LOW", "CLAMPED_HIGH", "ADAPTED"):
        assert int(re.findall(rf"#define HR_EXPOSURE_{name} (\d+)u", text)[0]) == getattr(ffi, "HR_EXPOSURE_" + name), name


@pytest.mark.parametrize("struct, cname, size", [(ffi.ExposureParams, "hr_exposure_params", 64), (ffi.ExposureResult, "hr_exposure_result", 80)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_EXPOSURE_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_exposure_default_params.restype = None
    p = ffi.ExposureParams(*([7] * 6))
    p.window[:] = [1, 2, 3, 4]
    lib.hr_exposure_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(exposure.default_params())
    lib.hr_exposure_default_params(None)  # (ignored)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_exposure_meter, lib.hr_exposure_display, lib.hr_exposure_last, lib.hr_exposure_reset):
        fn.restype = ctypes.c_int
    r, d = ffi.ExposureResult(), ffi.display_params()
    buf = (ctypes.c_uint8 * 16)()
    assert lib.hr_exposure_meter(None, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_exposure_display(None, None, ctypes.byref(d), 0, None, buf, None) != ffi.HR_OK
    assert lib.hr_exposure_last(None, ctypes.byref(r), None) != ffi.HR_OK
    assert lib.hr_exposure_reset(None) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_exposure_calls_raise(oracle_lib):
    def calls(eng):
        eng.resize(4, 4)
        return (eng.exposure_meter, lambda: eng.exposure_display(16), eng.exposure_last, eng.exposure_reset)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no auto-exposure")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("exposure_meter", "exposure_display", "exposure_last", "exposure_reset"))
