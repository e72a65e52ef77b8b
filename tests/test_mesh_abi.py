"""include/hrcore_mesh.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, both structs have the layout gcc gives them, no other header's version
moved, the library's defaults are the binding's, calls without a context fail loudly, and an Engine bound to a library without the
symbols (the CPU oracle) still constructs."""
import ctypes
import re

import numpy as np
import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, meshprep

HEADER = "hrcore_mesh.h"
NAMES = ["hr_mesh_api_version", "hr_mesh_default_params", "hr_mesh_prepare", "hr_mesh_last"]
CALLS = ("prepare_mesh", "add_mesh_prepared", "mesh_last")


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.MESH_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in abi_checks.HEADERS:
        assert not set(ffi.MESH_SYMBOLS) & set(abi_checks.symbols(header)), header
        assert "hrcore_mesh" not in abi_checks.header_text(header), header
    for header in ("hrcore_exposure.h", "hrcore_tree.h", "hrcore_metric.h", "hrcore_despeckle.h"):
        assert "hrcore_mesh" not in abi_checks.header_text(header), header
    for feature, (symbols, _, _) in ffi.FEATURES.items():
        assert feature == "mesh" or not set(ffi.MESH_SYMBOLS) & set(symbols), feature
    lib = core.load_library()
    for s in ffi.MESH_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_mesh_api_version.restype = ctypes.c_uint32
    assert lib.hr_mesh_api_version() == ffi.HR_MESH_API_VERSION == 1
    assert ffi.FEATURES["mesh"] == (ffi.MESH_SYMBOLS, ffi.HR_MESH_API_VERSION, "mesh preparation")
    abi_checks.check_no_version_moved()
    for fn in (lib.hr_exposure_api_version, lib.hr_tree_api_version, lib.hr_metric_api_version, lib.hr_despeckle_api_version):
        fn.restype = ctypes.c_uint32
    assert (lib.hr_exposure_api_version(), lib.hr_tree_api_version(), lib.hr_metric_api_version(), lib.hr_despeckle_api_version()) == (1, 2, 1, 1)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_MESH_API_VERSION (\d+)u", text)[0]) == ffi.HR_MESH_API_VERSION
    for name in ("HR_MESH_WEIGHT_ANGLE", "HR_MESH_WEIGHT_AREA", "HR_MESH_WEIGHT_UNIFORM", "HR_MESH_WANT_NORMALS", "HR_MESH_WANT_TANGENTS"):
        assert int(re.findall(rf"#define {name} (\d+)", text)[0]) == getattr(ffi, name), name
    assert (ffi.HR_MESH_WEIGHT_ANGLE, ffi.HR_MESH_WEIGHT_AREA, ffi.HR_MESH_WEIGHT_UNIFORM, ffi.HR_MESH_WANT_NORMALS, ffi.HR_MESH_WANT_TANGENTS) == (0, 1, 2, 1, 2)
    assert '#include "hrcore.h"' in text


@pytest.mark.parametrize("struct, cname, size", [(ffi.MeshParams, "hr_mesh_params", 32), (ffi.MeshResult, "hr_mesh_result", 64)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_MESH_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_mesh_default_params.restype = None
    p = ffi.MeshParams(9, 9, 9)
    p.reserved[:] = [5, 6, 7, 8, 9]
    lib.hr_mesh_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(meshprep.default_params())
    assert (p.weight, p.weld, p.want, list(p.reserved)) == (ffi.HR_MESH_WEIGHT_ANGLE, 1, ffi.HR_MESH_WANT_NORMALS, [0] * 5)
    lib.hr_mesh_default_params(None)  # (ignored)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_mesh_prepare, lib.hr_mesh_last):
        fn.restype = ctypes.c_int
    r = ffi.MeshResult()
    d = ffi.MeshDesc()
    out = (ctypes.c_float * 3)()
    assert lib.hr_mesh_prepare(None, ctypes.byref(d), None, out, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_mesh_last(None, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_mesh_calls_raise(oracle_lib):
    pos, idx = np.eye(3, dtype=np.float32), np.arange(3, dtype=np.uint32)

    def calls(eng):
        return (lambda: eng.prepare_mesh(pos, idx), lambda: eng.add_mesh_prepared(pos, idx), eng.mesh_last)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no mesh preparation")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(CALLS)
