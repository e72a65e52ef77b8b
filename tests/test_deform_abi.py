"""include/hrcore_deform.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, the three structs have the layout gcc gives them, no other header's
version moved, the library's defaults are the binding's, calls without a context fail loudly, an Engine bound to a library without the
symbols (the CPU oracle) still constructs, and the group engine inherits the calls."""
import ctypes
import re

import numpy as np
import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, deform

HEADER = "hrcore_deform.h"
NAMES = ["hr_deform_api_version", "hr_deform_default_params", "hr_geom_update", "hr_geom_get_attribute", "hr_deform_bind", "hr_deform_pose",
         "hr_deform_unbind", "hr_deform_last"]
CALLS = ("update_mesh", "mesh_attribute", "deform_bind", "deform_pose", "deform_unbind", "deform_last")


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.DEFORM_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in abi_checks.HEADERS:
        assert not set(ffi.DEFORM_SYMBOLS) & set(abi_checks.symbols(header)), header
        assert "hrcore_deform" not in abi_checks.header_text(header), header
    for header in ("hrcore_exposure.h", "hrcore_tree.h", "hrcore_metric.h", "hrcore_despeckle.h", "hrcore_mesh.h"):
        assert "hrcore_deform" not in abi_checks.header_text(header), header
    for feature, (symbols, _, _) in ffi.FEATURES.items():
        assert feature == "deform" or not set(ffi.DEFORM_SYMBOLS) & set(symbols), feature
    lib = core.load_library()
    for s in ffi.DEFORM_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_deform_api_version.restype = ctypes.c_uint32
    assert lib.hr_deform_api_version() == ffi.HR_DEFORM_API_VERSION == 1
    assert ffi.FEATURES["deform"] == (ffi.DEFORM_SYMBOLS, ffi.HR_DEFORM_API_VERSION, "deformable meshes")
    abi_checks.check_no_version_moved()
    for fn in (lib.hr_exposure_api_version, lib.hr_tree_api_version, lib.hr_metric_api_version, lib.hr_despeckle_api_version, lib.hr_mesh_api_version):
        fn.restype = ctypes.c_uint32
        assert fn() == (2 if fn is lib.hr_tree_api_version else 1)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_DEFORM_API_VERSION (\d+)u", text)[0]) == ffi.HR_DEFORM_API_VERSION
    names = ("HR_GEOM_POSITIONS", "HR_GEOM_NORMALS", "HR_GEOM_UVS", "HR_GEOM_TANGENTS", "HR_GEOM_BITANGENTS", "HR_GEOM_COLORS", "HR_DEFORM_NORMALS",
             "HR_DEFORM_TANGENTS", "HR_DEFORM_MAX_MORPH", "HR_DEFORM_MAX_JOINTS")
    for name in names:
        assert int(re.findall(rf"#define {name} (\d+)", text)[0]) == getattr(ffi, name), name
    assert tuple(getattr(ffi, n) for n in names) == (0, 1, 2, 3, 4, 5, 1, 2, 8, 1024)
    assert (ffi.HR_DEFORM_NORMALS, ffi.HR_DEFORM_TANGENTS) == (ffi.HR_MESH_WANT_NORMALS, ffi.HR_MESH_WANT_TANGENTS)  # regenerate is handed on as `want`
    assert '#include "hrcore_mesh.h"' in text


@pytest.mark.parametrize("struct, cname, size", [(ffi.DeformParams, "hr_deform_params", 32), (ffi.DeformRig, "hr_deform_rig", 64),
                                                 (ffi.DeformResult, "hr_deform_result", 104)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_DEFORM_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_deform_default_params.restype = None
    p = ffi.DeformParams(9, 9, 9)
    p.reserved[:] = [5, 6, 7, 8, 9]
    lib.hr_deform_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(deform.default_params())
    assert (p.regenerate, p.weight, p.weld, list(p.reserved)) == (0, ffi.HR_MESH_WEIGHT_ANGLE, 1, [0] * 5)
    lib.hr_deform_default_params(None)  # (ignored)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for name in NAMES[2:]:
        getattr(lib, name).restype = ctypes.c_int
    r, d, rig = ffi.DeformResult(), ffi.MeshDesc(), ffi.DeformRig()
    out = (ctypes.c_float * 3)()
    assert lib.hr_geom_update(None, 0, ctypes.byref(d), None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_geom_get_attribute(None, 0, 0, out) != ffi.HR_OK
    assert lib.hr_deform_bind(None, 0, ctypes.byref(rig)) != ffi.HR_OK
    assert lib.hr_deform_pose(None, 0, None, None, None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_deform_unbind(None, 0) != ffi.HR_OK
    assert lib.hr_deform_last(None, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_deform_calls_raise(oracle_lib):
    pos = np.eye(3, dtype=np.float32)

    def calls(eng):
        return (lambda: eng.update_mesh(0, pos), lambda: eng.mesh_attribute(0, ffi.HR_GEOM_POSITIONS, n_vertices=3),
                lambda: eng.mesh_attribute(0, ffi.HR_GEOM_POSITIONS), lambda: eng.deform_bind(0, morph_positions=pos[None]),
                lambda: eng.deform_pose(0, morph_weights=[1.0]), lambda: eng.deform_unbind(0), eng.deform_last)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no deformable meshes")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(CALLS)
