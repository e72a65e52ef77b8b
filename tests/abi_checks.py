"""What the test_*_abi.py files of the post-process features ask of every header under include/: one table of the headers, their
version functions and their symbol lists, and the checks that are the same for each of them.  A feature's file keeps its own names,
constants, calls and refusal text."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

# header: (version function, ffi constant, its value, ffi symbol list), oldest first: a header may name the ones above it, never one below
HEADERS = {
    "hrcore.h": ("hr_abi_version", "HR_ABI_VERSION", 6, "ABI_SYMBOLS"),
    "hrcore_group.h": ("hr_group_api_version", "HR_GROUP_API_VERSION", 1, "GROUP_SYMBOLS"),
    "hrcore_aov.h": ("hr_aov_api_version", "HR_AOV_API_VERSION", 1, "AOV_SYMBOLS"),
    "hrcore_denoise.h": ("hr_denoise_api_version", "HR_DENOISE_API_VERSION", 1, "DENOISE_SYMBOLS"),
    "hrcore_adaptive.h": ("hr_adaptive_api_version", "HR_ADAPTIVE_API_VERSION", 1, "ADAPTIVE_SYMBOLS"),
    "hrcore_history.h": ("hr_history_api_version", "HR_HISTORY_API_VERSION", 1, "HISTORY_SYMBOLS"),
    "hrcore_reproject.h": ("hr_reproject_api_version", "HR_REPROJECT_API_VERSION", 1, "REPROJECT_SYMBOLS"),
    "hrcore_denoise_spatial.h": ("hr_denoise_spatial_api_version", "HR_DENOISE_SPATIAL_API_VERSION", 1, "DENOISE_SPATIAL_SYMBOLS"),
}


def header_text(header):
    return open(os.path.join(INCLUDE, header)).read()


def declared_functions(header):
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", header_text(header), re.M)))


def symbols(header):
    return getattr(ffi, HEADERS[header][3])


def older_headers(header):
    names = list(HEADERS)
    return names[:names.index(header)]


def check_binding_agrees_and_is_disjoint(header):
    """the ffi list is the header's declarations, and shares no name with any other header's"""
    assert sorted("hr_" + s for s in symbols(header)) == declared_functions(header)
    for other in HEADERS:
        if other != header:
            assert not set(symbols(header)) & set(symbols(other)), other


def check_no_version_moved():
    """every header's version, in the binding and in the library, is what the table says"""
    lib = core.load_library()
    for header, (fn, const, want, _) in HEADERS.items():
        assert getattr(ffi, const) == want, const
        f = getattr(lib, fn)
        f.restype = ctypes.c_uint32
        assert f() == want, fn


def check_library_exports(header):
    """the library exports every function the header declares, and its version is the binding's"""
    lib = core.load_library()
    for name in declared_functions(header):
        assert hasattr(lib, name), name
    fn, const, want, _ = HEADERS[header]
    f = getattr(lib, fn)
    f.restype = ctypes.c_uint32
    assert f() == getattr(ffi, const) == want


def check_struct_layout(tmp_path, header, struct, cname, version_macro, version=1):
    """the header compiles as C with `version_macro` at `version`, and gcc gives `cname` the size and the field offsets of the ctypes `struct`,
    which names it as its C type"""
    assert struct._cname_ == cname
    fields = [n for n, _ in struct._fields_]
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void) {{\n'
                   f'  printf("%zu", sizeof({cname}));\n'
                   + "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + f"  return (int)({version_macro}) - {int(version)};\n}}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(v) for v in out.stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def check_oracle_engine_lacks(oracle_lib, calls_of, match):
    """an Engine bound to the CPU oracle, which has none of the feature's symbols, constructs; each of calls_of(engine) raises `match`"""
    eng = ffi.Engine(oracle_lib, "ora_")
    for call in calls_of(eng):
        with pytest.raises(ffi.EngineError, match=match):
            call()
    eng.close()


def check_group_engine_inherits(names):
    for name in names:
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
