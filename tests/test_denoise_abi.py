"""CPU-side checks of the denoiser's boundary (include/hrcore_denoise.h): the header, the Python binding and the library agree, the
symbols are disjoint from the three other headers', the params struct has the layout gcc gives it, calls without a context fail
loudly, and an Engine bound to the CPU oracle (which has no denoiser) still constructs."""
import ctypes
import re

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise

HEADER = "hrcore_denoise.h"


def test_header_and_python_binding_agree():
    abi_checks.check_binding_agrees_and_is_disjoint(HEADER)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_DENOISE_API_VERSION (\d+)u", text)[0]) == ffi.HR_DENOISE_API_VERSION
    for name in ("MAX_ITERATIONS", "MAX_NORMAL_POWER", "KERNEL_AUTO", "KERNEL_PLAIN", "KERNEL_TILED"):
        assert int(re.findall(rf"#define HR_DENOISE_{name} (\d+)", text)[0]) == getattr(ffi, "HR_DENOISE_" + name), name


def test_the_other_headers_and_versions_did_not_move():
    for other in abi_checks.older_headers(HEADER):
        assert "hrcore_denoise" not in abi_checks.header_text(other), other
    abi_checks.check_no_version_moved()


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    abi_checks.check_library_exports(HEADER)
    lib = core.load_library()
    p = ffi.DenoiseParams(-1, -1, -1.0, -1.0, -1, (9, 9, 9))
    lib.hr_denoise_default_params.restype = None
    lib.hr_denoise_default_params(ctypes.byref(p))
    d = denoise.default_params()
    assert bytes(p) == bytes(d)
    assert (p.iterations, p.normal_power, p.sigma_l, p.sigma_z, p.kernel, list(p.reserved)) == (5, 7, 4.0, 4.0, 0, [0, 0, 0])
    lib.hr_denoise_default_params(None)  # (a null pointer is ignored)


def test_header_compiles_as_c_and_the_struct_has_gccs_layout(tmp_path):
    abi_checks.check_struct_layout(tmp_path, HEADER, ffi.DenoiseParams, "hr_denoise_params", "HR_DENOISE_API_VERSION + HR_DENOISE_KERNEL_AUTO")


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    p = ctypes.POINTER(ctypes.c_float)()
    w, h, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32()
    for fn in (lib.hr_denoise, lib.hr_denoise_readback, lib.hr_denoise_display):
        fn.restype = ctypes.c_int
    assert lib.hr_denoise(None, None, ctypes.c_void_p(16), None, ctypes.byref(n)) != ffi.HR_OK
    assert lib.hr_denoise_readback(None, None, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)) != ffi.HR_OK
    dp = ffi.display_params()
    assert lib.hr_denoise_display(None, None, ctypes.byref(dp), ctypes.c_int32(0), ctypes.c_void_p(16), ctypes.byref(n)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_denoise_calls_raise(oracle_lib):
    abi_checks.check_oracle_engine_lacks(oracle_lib, lambda eng: (eng.denoise, lambda: eng.denoise(denoise.default_params()), lambda: eng.denoise_to_device(16),
                                                                  lambda: eng.denoise_display(16)), "no denoiser")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("denoise", "denoise_to_device", "denoise_display"))
