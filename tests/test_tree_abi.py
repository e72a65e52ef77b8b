"""include/hrcore_tree.h without a GPU: the binding's symbol list is the header's declarations, the library exports them with the
binding's version, hr_tree_info has the layout gcc gives it, and hrcore.h's own version and hr_scene_info did not move for it."""
import ctypes
import re

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.TREE_SYMBOLS) == abi_checks.declared_functions("hrcore_tree.h")
    for header in abi_checks.HEADERS:
        assert not set(ffi.TREE_SYMBOLS) & set(abi_checks.symbols(header)), header
    lib = core.load_library()
    for s in ffi.TREE_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_tree_api_version.restype = ctypes.c_uint32
    assert lib.hr_tree_api_version() == ffi.HR_TREE_API_VERSION == 2
    assert ffi.FEATURES["tree"][:2] == (ffi.TREE_SYMBOLS, ffi.HR_TREE_API_VERSION)
    abi_checks.check_no_version_moved()


def test_tree_info_layout(tmp_path):
    abi_checks.check_struct_layout(tmp_path, "hrcore_tree.h", ffi.TreeInfo, "hr_tree_info", "HR_TREE_API_VERSION", version=2)
    assert ctypes.sizeof(ffi.TreeInfo) == 32


def test_tree_layout_layout_and_array_names(tmp_path):
    abi_checks.check_struct_layout(tmp_path, "hrcore_tree.h", ffi.TreeLayout, "hr_tree_layout", "HR_TREE_API_VERSION", version=2)
    assert ctypes.sizeof(ffi.TreeLayout) == 416 and ffi.TreeLayout.bytes.offset == 368
    text = abi_checks.header_text("hrcore_tree.h")
    names = ("NODE4", "NODE32", "LEAF_KEYS", "TRIS", "NODE_BOX", "SLOT_OF_PRIM", "ARRAYS")
    for value, name in enumerate(names):
        assert re.search(rf"#define HR_TREE_{name} {value}\b", text) and getattr(ffi, "HR_TREE_" + name) == value, name
