"""include/hrcore_despeckle.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, both structs have the layout gcc gives them, no other header's version
moved, the library's defaults are the binding's, calls without a context fail loudly, and an Engine bound to a library without the
symbols (the CPU oracle) still constructs."""
import ctypes
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, despeckle

HEADER = "hrcore_despeckle.h"
NAMES = ["hr_despeckle_api_version", "hr_despeckle_default_params", "hr_despeckle", "hr_despeckle_readback", "hr_despeckle_denoise",
         "hr_despeckle_denoise_readback"]
CALLS = ("despeckle", "despeckle_to_device", "despeckle_denoise", "despeckle_denoise_to_device")


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.DESPECKLE_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in abi_checks.HEADERS:
        assert not set(ffi.DESPECKLE_SYMBOLS) & set(abi_checks.symbols(header)), header
        assert "hrcore_despeckle" not in abi_checks.header_text(header), header
    others = set(ffi.TREE_SYMBOLS) | set(ffi.EXPOSURE_SYMBOLS) | set(ffi.METRIC_SYMBOLS)
    assert not set(ffi.DESPECKLE_SYMBOLS) & others
    for header in ("hrcore_exposure.h", "hrcore_tree.h", "hrcore_metric.h"):
        assert "hrcore_despeckle" not in abi_checks.header_text(header), header
    for feature, (symbols, _, _) in ffi.FEATURES.items():
        assert feature == "despeckle" or not set(ffi.DESPECKLE_SYMBOLS) & set(symbols), feature
    lib = core.load_library()
    for s in ffi.DESPECKLE_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_despeckle_api_version.restype = ctypes.c_uint32
    assert lib.hr_despeckle_api_version() == ffi.HR_DESPECKLE_API_VERSION == 1
    assert ffi.FEATURES["despeckle"] == (ffi.DESPECKLE_SYMBOLS, ffi.HR_DESPECKLE_API_VERSION, "firefly suppression")
    abi_checks.check_no_version_moved()
    for fn in (lib.hr_exposure_api_version, lib.hr_tree_api_version, lib.hr_metric_api_version):
        fn.restype = ctypes.c_uint32
    assert (lib.hr_exposure_api_version(), lib.hr_tree_api_version(), lib.hr_metric_api_version()) == (1, 2, 1)
    assert (ffi.HR_EXPOSURE_API_VERSION, ffi.HR_TREE_API_VERSION, ffi.HR_METRIC_API_VERSION) == (1, 2, 1)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_DESPECKLE_API_VERSION (\d+)u", text)[0]) == ffi.HR_DESPECKLE_API_VERSION
    assert int(re.findall(r"#define HR_DESPECKLE_RANK_HIGHEST (\d+)", text)[0]) == ffi.HR_DESPECKLE_RANK_HIGHEST == 4
    assert int(re.findall(r"#define HR_DESPECKLE_TAPS (\d+)", text)[0]) == ffi.HR_DESPECKLE_TAPS == 24 == (2 * despeckle.RADIUS + 1) ** 2 - 1


@pytest.mark.parametrize("struct, cname, size", [(ffi.DespeckleParams, "hr_despeckle_params", 32), (ffi.DespeckleResult, "hr_despeckle_result", 64)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_DESPECKLE_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_despeckle_default_params.restype = None
    p = ffi.DespeckleParams(9, 9, 9.0, 9.0, 9.0)
    p.reserved[:] = [5, 6, 7]
    lib.hr_despeckle_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(despeckle.default_params())
    assert (p.rank, p.min_taps, p.ratio, p.sigmas, p.floor, list(p.reserved)) == (2, 8, 2.0, 3.0, 0.0, [0, 0, 0])
    lib.hr_despeckle_default_params(None)  # (ignored)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_despeckle, lib.hr_despeckle_readback, lib.hr_despeckle_denoise, lib.hr_despeckle_denoise_readback):
        fn.restype = ctypes.c_int
    r = ffi.DespeckleResult()
    buf = (ctypes.c_uint8 * 16)()
    p = ctypes.POINTER(ctypes.c_float)()
    assert lib.hr_despeckle(None, None, None, None, buf, None, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_despeckle_readback(None, None, ctypes.byref(p), None, None, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_despeckle_denoise(None, None, None, 0, None, buf, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_despeckle_denoise_readback(None, None, None, 1, None, ctypes.byref(p), None, None, None, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_despeckle_calls_raise(oracle_lib):
    def calls(eng):
        eng.resize(4, 4)
        return (eng.despeckle, lambda: eng.despeckle_to_device(16), eng.despeckle_denoise, lambda: eng.despeckle_denoise_to_device(16))
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no firefly suppression")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(CALLS)
