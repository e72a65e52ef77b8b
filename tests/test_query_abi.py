"""include/hrcore_query.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, the three structs have the layout gcc gives them, no other header's
version moved, the constants are the header's, calls without a context fail loudly, an Engine bound to a library without the symbols (the
CPU oracle) still constructs, and the group engine inherits the calls."""
import ctypes
import re

import numpy as np
import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core

HEADER = "hrcore_query.h"
NAMES = ["hr_query_api_version", "hr_query_trace", "hr_query_trace_host", "hr_query_pixels", "hr_query_last"]
CALLS = ("query", "query_to_device", "query_pixels", "query_last")
NEWER = ("hrcore_exposure.h", "hrcore_tree.h", "hrcore_metric.h", "hrcore_despeckle.h", "hrcore_mesh.h", "hrcore_deform.h")


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.QUERY_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in tuple(abi_checks.HEADERS) + NEWER:
        assert not set("hr_" + s for s in ffi.QUERY_SYMBOLS) & set(abi_checks.declared_functions(header)), header
        assert "hrcore_query" not in abi_checks.header_text(header), header
    for feature, (symbols, _, _) in ffi.FEATURES.items():
        assert feature == "query" or not set(ffi.QUERY_SYMBOLS) & set(symbols), feature
    assert not set(ffi.QUERY_SYMBOLS) & set(ffi.ABI_SYMBOLS) and not set(ffi.QUERY_SYMBOLS) & set(ffi.GROUP_SYMBOLS)
    lib = core.load_library()
    for s in ffi.QUERY_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_query_api_version.restype = ctypes.c_uint32
    assert lib.hr_query_api_version() == ffi.HR_QUERY_API_VERSION == 1
    assert ffi.FEATURES["query"] == (ffi.QUERY_SYMBOLS, ffi.HR_QUERY_API_VERSION, "ray queries")
    abi_checks.check_no_version_moved()
    for fn in (lib.hr_exposure_api_version, lib.hr_tree_api_version, lib.hr_metric_api_version, lib.hr_despeckle_api_version, lib.hr_mesh_api_version,
               lib.hr_deform_api_version):
        fn.restype = ctypes.c_uint32
        assert fn() == (2 if fn is lib.hr_tree_api_version else 1)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_QUERY_API_VERSION (\d+)u", text)[0]) == ffi.HR_QUERY_API_VERSION
    names = ("HR_QUERY_ANY_HIT", "HR_QUERY_SF_FRONT", "HR_QUERY_SF_HAS_UV", "HR_QUERY_SF_NON_OCCLUDER")
    for name in names:
        assert int(re.findall(rf"#define {name} (\d+)u", text)[0]) == getattr(ffi, name), name
    assert tuple(getattr(ffi, n) for n in names) == (1, 1, 2, 4)
    assert int(re.findall(r"#define HR_QUERY_INVALID_RAY \((-\d+)\)", text)[0]) == ffi.HR_QUERY_INVALID_RAY == -2
    assert '#include "hrcore.h"' in text
    # the numpy record is the ctypes struct, field for field
    assert ffi.SURFACE_DTYPE.itemsize == ctypes.sizeof(ffi.QuerySurface) == 64
    for name, _ in ffi.QuerySurface._fields_:
        assert ffi.SURFACE_DTYPE.fields[name][1] == getattr(ffi.QuerySurface, name).offset, name


@pytest.mark.parametrize("struct, cname, size", [(ffi.QueryDesc, "hr_query_desc", 88), (ffi.QuerySurface, "hr_query_surface", 64),
                                                 (ffi.QueryResult, "hr_query_result", 64)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_QUERY_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for name in NAMES[1:]:
        getattr(lib, name).restype = ctypes.c_int
    d, r, cam = ffi.QueryDesc(), ffi.QueryResult(), ffi.PassParams()
    xy = (ctypes.c_float * 2)()
    hit = ffi.Hit()
    assert lib.hr_query_trace(None, ctypes.byref(d), None) != ffi.HR_OK
    assert lib.hr_query_trace_host(None, ctypes.byref(d)) != ffi.HR_OK
    assert lib.hr_query_pixels(None, ctypes.byref(cam), 1, xy, ctypes.byref(hit), None, None) != ffi.HR_OK
    assert lib.hr_query_last(None, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_query_calls_raise(oracle_lib):
    o = np.zeros((2, 3), np.float32)
    d = np.ones((2, 3), np.float32)

    def calls(eng):
        return (lambda: eng.query(o, d), lambda: eng.query(o, d, surface=True), lambda: eng.query_to_device(2, 256, 512, hits_ptr=1024),
                lambda: eng.query_pixels(ffi.PassParams(), [[0.5, 0.5]]), eng.query_last)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no ray queries")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(CALLS)
