"""CPU-side checks of the progressive-merge boundary (include/hrcore_reproject.h): the header, the Python binding and the library agree, the
symbols are disjoint from the six other headers', both structs have the layout gcc gives them, no other version moved (history's
included), hrcore_history.h declares what it declared, calls without a context fail loudly, and an Engine bound to the CPU oracle (which
has none of this) still constructs."""
import ctypes
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core

HEADER = "hrcore_reproject.h"


def test_header_and_python_binding_agree():
    abi_checks.check_binding_agrees_and_is_disjoint(HEADER)
    for name in ("hr_reproject_api_version", "hr_reproject_merge", "hr_reproject_examined_get", "hr_reproject_preview", "hr_reproject_preview_readback"):
        assert name in abi_checks.declared_functions(HEADER), name


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_REPROJECT_API_VERSION (\d+)u", text)[0]) == ffi.HR_REPROJECT_API_VERSION == 1
    assert '#include "hrcore_history.h"' in text


def test_the_history_header_declares_what_it_declared():
    assert abi_checks.declared_functions("hrcore_history.h") == sorted(
        ["hr_history_api_version", "hr_history_default_params", "hr_history_capture", "hr_history_merge", "hr_history_drop", "hr_history_info", "hr_history_readback"])
    assert sorted("hr_" + s for s in ffi.HISTORY_SYMBOLS) == abi_checks.declared_functions("hrcore_history.h")
    text = abi_checks.header_text("hrcore_history.h")
    assert int(re.findall(r"#define HR_HISTORY_API_VERSION (\d+)u", text)[0]) == ffi.HR_HISTORY_API_VERSION == 1


def test_the_other_headers_and_versions_did_not_move():
    for other in abi_checks.older_headers(HEADER):
        assert "hrcore_reproject" not in abi_checks.header_text(other), other
    abi_checks.check_no_version_moved()


def test_library_exports_every_symbol_and_the_version_matches():
    abi_checks.check_library_exports(HEADER)


@pytest.mark.parametrize("struct, cname", [(ffi.ReprojectResult, "hr_reproject_result"), (ffi.ReprojectPreviewResult, "hr_reproject_preview_result")])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_REPROJECT_API_VERSION")


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_reproject_merge, lib.hr_reproject_examined_get, lib.hr_reproject_preview, lib.hr_reproject_preview_readback):
        fn.restype = ctypes.c_int
    pp = ffi.PassParams()
    r, pr = ffi.ReprojectResult(), ffi.ReprojectPreviewResult()
    buf = (ctypes.c_uint8 * 16)()
    p = ctypes.POINTER(ctypes.c_float)()
    assert lib.hr_reproject_merge(None, ctypes.byref(pp), None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_reproject_examined_get(None, buf) != ffi.HR_OK
    assert lib.hr_reproject_preview(None, ctypes.byref(pp), None, buf, None, ctypes.byref(pr)) != ffi.HR_OK
    assert lib.hr_reproject_preview_readback(None, ctypes.byref(pp), None, ctypes.byref(p), None, None, ctypes.byref(pr)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_reproject_calls_raise(oracle_lib):
    pp = ffi.PassParams()

    def calls(eng):
        eng.resize(4, 4)
        return (lambda: eng.reproject_merge(pp), lambda: eng.reproject_preview(pp), lambda: eng.reproject_preview_to_device(16, pp), eng.reproject_examined)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "no progressive history merge")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("reproject_merge", "reproject_preview", "reproject_preview_to_device", "reproject_examined"))
