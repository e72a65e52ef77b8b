"""include/hrcore_metric.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, both structs have the layout gcc gives them, no other header's version
moved, the library's defaults are the binding's, calls without a context fail loudly, and an Engine bound to a library without the
symbols (the CPU oracle) still constructs."""
import ctypes
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, metric

HEADER = "hrcore_metric.h"
NAMES = ["hr_metric_api_version", "hr_metric_default_params", "hr_metric_compare", "hr_metric_estimate", "hr_metric_last"]


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.METRIC_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in abi_checks.HEADERS:
        assert not set(ffi.METRIC_SYMBOLS) & set(abi_checks.symbols(header)), header
        assert "hrcore_metric" not in abi_checks.header_text(header), header
    assert not set(ffi.METRIC_SYMBOLS) & (set(ffi.TREE_SYMBOLS) | set(ffi.EXPOSURE_SYMBOLS))
    assert "hrcore_metric" not in abi_checks.header_text("hrcore_exposure.h") and "hrcore_metric" not in abi_checks.header_text("hrcore_tree.h")
    lib = core.load_library()
    for s in ffi.METRIC_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_metric_api_version.restype = ctypes.c_uint32
    assert lib.hr_metric_api_version() == ffi.HR_METRIC_API_VERSION == 1
    assert ffi.FEATURES["metric"] == (ffi.METRIC_SYMBOLS, ffi.HR_METRIC_API_VERSION, "convergence metric")
    abi_checks.check_no_version_moved()
    lib.hr_exposure_api_version.restype = lib.hr_tree_api_version.restype = ctypes.c_uint32
    assert (lib.hr_exposure_api_version(), lib.hr_tree_api_version()) == (ffi.HR_EXPOSURE_API_VERSION, ffi.HR_TREE_API_VERSION) == (1, 2)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_METRIC_API_VERSION (\d+)u", text)[0]) == ffi.HR_METRIC_API_VERSION
    assert int(re.findall(r"#define HR_METRIC_BINS (\d+)", text)[0]) == ffi.HR_METRIC_BINS == 256
    for name in ("COMPARE", "ESTIMATE", "EMPTY", "ZERO_DENOMINATOR"):
        assert int(re.findall(rf"#define HR_METRIC_{name} (\d+)u", text)[0]) == getattr(ffi, "HR_METRIC_" + name), name


@pytest.mark.parametrize("struct, cname, size", [(ffi.MetricParams, "hr_metric_params", 32), (ffi.MetricResult, "hr_metric_result", 96)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_METRIC_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_metric_default_params.restype = None
    p = ffi.MetricParams()
    p.window[:] = [1, 2, 3, 4]
    p.reserved[:] = [5, 6, 7, 8]
    lib.hr_metric_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(metric.default_params()) == bytes(32)
    lib.hr_metric_default_params(None)  # (ignored)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_metric_compare, lib.hr_metric_estimate, lib.hr_metric_last):
        fn.restype = ctypes.c_int
    r = ffi.MetricResult()
    buf = (ctypes.c_uint8 * 16)()
    assert lib.hr_metric_compare(None, None, None, buf, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_metric_estimate(None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_metric_last(None, ctypes.byref(r), None, None) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_metric_calls_raise(oracle_lib):
    def calls(eng):
        eng.resize(4, 4)
        return (lambda: eng.metric_compare(16), eng.metric_estimate, eng.metric_last)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no convergence metric")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(("metric_compare", "metric_estimate", "metric_last"))
