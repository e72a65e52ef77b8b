"""CPU-side checks of the spatial variance estimate's boundary (include/hrcore_denoise_spatial.h): the header, the Python binding and the
library agree, the symbols are disjoint from the other headers', the structs have the layout gcc gives them, the older headers did not
move, calls without a context fail loudly, and an Engine bound to the CPU oracle (which has no denoiser) still constructs."""
import ctypes
import re

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise_spatial

HEADER = "hrcore_denoise_spatial.h"


def test_header_and_python_binding_agree():
    abi_checks.check_binding_agrees_and_is_disjoint(HEADER)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_DENOISE_SPATIAL_API_VERSION (\d+)u", text)[0]) == ffi.HR_DENOISE_SPATIAL_API_VERSION == 1
    for name in ("BELOW_LOWEST", "BELOW_HIGHEST", "MIN_TAPS_LOWEST", "MIN_TAPS_HIGHEST"):
        assert int(re.findall(rf"#define HR_DENOISE_SPATIAL_{name} (\d+)", text)[0]) == getattr(ffi, "HR_DENOISE_SPATIAL_" + name), name
    assert '#include "hrcore_denoise.h"' in text


def test_the_other_headers_and_versions_did_not_move():
    for other in abi_checks.older_headers(HEADER):
        if other != "hrcore_denoise.h":  # (the header this one builds on points to it)
            assert "denoise_spatial" not in abi_checks.header_text(other), other
    dn = abi_checks.header_text("hrcore_denoise.h")
    assert "#define HR_DENOISE_API_VERSION 1u" in dn and "uint32_t reserved[3]; /* 0 */" in dn
    abi_checks.check_no_version_moved()
    assert ctypes.sizeof(ffi.DenoiseParams) == 32


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    abi_checks.check_library_exports(HEADER)
    lib = core.load_library()
    p = ffi.DenoiseSpatialParams(-1, -1, (9, 9, 9, 9, 9, 9))
    lib.hr_denoise_spatial_default_params.restype = None
    lib.hr_denoise_spatial_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(denoise_spatial.default_params())
    assert (p.below, p.min_taps, list(p.reserved)) == (4, 6, [0] * 6)
    lib.hr_denoise_spatial_default_params(None)  # (a null pointer is ignored)


def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path):
    for cname, struct in (("hr_denoise_spatial_params", ffi.DenoiseSpatialParams), ("hr_denoise_spatial_result", ffi.DenoiseSpatialResult)):
        abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_DENOISE_SPATIAL_API_VERSION")
    assert (ctypes.sizeof(ffi.DenoiseSpatialParams), ctypes.sizeof(ffi.DenoiseSpatialResult)) == (32, 24)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    p = ctypes.POINTER(ctypes.c_float)()
    w, h, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32()
    r = ffi.DenoiseSpatialResult()
    for fn in (lib.hr_denoise_spatial, lib.hr_denoise_spatial_readback, lib.hr_denoise_spatial_display, lib.hr_denoise_spatial_variance):
        fn.restype = ctypes.c_int
    assert lib.hr_denoise_spatial(None, None, None, ctypes.c_void_p(16), None, ctypes.byref(n), ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_denoise_spatial_readback(None, None, None, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n), ctypes.byref(r)) != ffi.HR_OK
    dp = ffi.display_params()
    assert lib.hr_denoise_spatial_display(None, None, None, ctypes.byref(dp), ctypes.c_int32(0), ctypes.c_void_p(16), ctypes.byref(n)) != ffi.HR_OK
    out = (ctypes.c_float * 4)()
    assert lib.hr_denoise_spatial_variance(None, None, None, out, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_calls_raise(oracle_lib):
    def calls(eng):
        eng.width = eng.height = 2
        return (eng.denoise_spatial, lambda: eng.denoise_spatial(None, denoise_spatial.default_params()), lambda: eng.denoise_spatial_to_device(16),
                lambda: eng.denoise_spatial_display(16), eng.denoise_spatial_variance)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "no spatial variance estimate")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("denoise_spatial", "denoise_spatial_to_device", "denoise_spatial_display", "denoise_spatial_variance"))
