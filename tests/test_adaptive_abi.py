"""CPU-side checks of the adaptive-sampling boundary (include/hrcore_adaptive.h): the header, the Python binding and the library agree,
the symbols are disjoint from the four other headers', both structs have the layout gcc gives them, the other versions did not move,
calls without a context fail loudly, and an Engine bound to the CPU oracle (which has none of this) still constructs."""
import ctypes
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import adaptive, core

HEADER = "hrcore_adaptive.h"


def test_header_and_python_binding_agree():
    abi_checks.check_binding_agrees_and_is_disjoint(HEADER)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_ADAPTIVE_API_VERSION (\d+)u", text)[0]) == ffi.HR_ADAPTIVE_API_VERSION == 1
    for name in ("MIN_SAMPLES_LOWEST", "MIN_SAMPLES_HIGHEST", "MAX_RADIUS"):
        assert int(re.findall(rf"#define HR_ADAPTIVE_{name} (\d+)", text)[0]) == getattr(ffi, "HR_ADAPTIVE_" + name), name


def test_the_other_headers_and_versions_did_not_move():
    for other in abi_checks.older_headers(HEADER):
        assert "hrcore_adaptive" not in abi_checks.header_text(other), other
    abi_checks.check_no_version_moved()


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    abi_checks.check_library_exports(HEADER)
    lib = core.load_library()
    p = ffi.AdaptiveParams(-1.0, -1.0, -1, -1, (9, 9, 9, 9))
    lib.hr_adaptive_default_params.restype = None
    lib.hr_adaptive_default_params(ctypes.byref(p))
    d = adaptive.default_params()
    assert bytes(p) == bytes(d)
    assert (p.min_samples, p.radius, list(p.reserved)) == (16, 2, [0, 0, 0, 0])
    assert (p.threshold, p.floor) == (ctypes.c_float(0.02).value, ctypes.c_float(0.05).value)
    assert p.radius >= 1  # (the header's known limit: radius 0 switches pixels off for good)
    lib.hr_adaptive_default_params(None)  # (a null pointer is ignored)


@pytest.mark.parametrize("struct, cname", [(ffi.AdaptiveParams, "hr_adaptive_params"), (ffi.AdaptiveResult, "hr_adaptive_result")])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_ADAPTIVE_API_VERSION")


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_sample_mask_set, lib.hr_sample_mask_get, lib.hr_adaptive_update, lib.hr_adaptive_error_copy, lib.hr_adaptive_error_readback):
        fn.restype = ctypes.c_int
    buf = (ctypes.c_uint8 * 16)()
    inst = ctypes.c_int32()
    r = ffi.AdaptiveResult()
    assert lib.hr_sample_mask_set(None, buf) != ffi.HR_OK
    assert lib.hr_sample_mask_get(None, buf, ctypes.byref(inst)) != ffi.HR_OK
    assert lib.hr_adaptive_update(None, None, ctypes.c_int32(1), ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_adaptive_error_copy(None, ctypes.c_void_p(16), None) != ffi.HR_OK
    assert lib.hr_adaptive_error_readback(None, ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_adaptive_calls_raise(oracle_lib):
    import numpy as np

    def calls(eng):
        eng.resize(4, 4)
        return (lambda: eng.set_sample_mask(None), lambda: eng.set_sample_mask(np.ones((4, 4), np.uint8)), eng.sample_mask, eng.adaptive_update,
                eng.adaptive_error, lambda: eng.adaptive_error_to_device(16))
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "no adaptive sampling")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("set_sample_mask", "sample_mask", "adaptive_update", "adaptive_error", "adaptive_error_to_device"))
