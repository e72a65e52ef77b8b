"""CPU-side checks of the progressive-merge boundary (include/hrcore_reproject.h): the header, the Python binding and the library agree, the
symbols are disjoint from the six other headers', both structs have the layout gcc gives them, no other version moved (history's
included), hrcore_history.h declares what it declared, calls without a context fail loudly, and an Engine bound to the CPU oracle (which
has none of this) still constructs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hrcore_reproject.h")


def declared_functions(header=HEADER):
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", open(header).read(), re.M)))


def test_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.REPROJECT_SYMBOLS) == declared_functions()
    for other in (ffi.ABI_SYMBOLS, ffi.GROUP_SYMBOLS, ffi.AOV_SYMBOLS, ffi.DENOISE_SYMBOLS, ffi.ADAPTIVE_SYMBOLS, ffi.HISTORY_SYMBOLS):
        assert not set(ffi.REPROJECT_SYMBOLS) & set(other)
    for name in ("hr_reproject_api_version", "hr_reproject_merge", "hr_reproject_examined_get", "hr_reproject_preview", "hr_reproject_preview_readback"):
        assert name in declared_functions(), name


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.findall(r"#define HR_REPROJECT_API_VERSION (\d+)u", text)[0]) == ffi.HR_REPROJECT_API_VERSION == 1
    assert '#include "hrcore_history.h"' in text


def test_the_history_header_declares_what_it_declared():
    assert declared_functions(os.path.join(ROOT, "include", "hrcore_history.h")) == sorted(
        ["hr_history_api_version", "hr_history_default_params", "hr_history_capture", "hr_history_merge", "hr_history_drop", "hr_history_info", "hr_history_readback"])
    assert sorted("hr_" + s for s in ffi.HISTORY_SYMBOLS) == declared_functions(os.path.join(ROOT, "include", "hrcore_history.h"))
    text = open(os.path.join(ROOT, "include", "hrcore_history.h")).read()
    assert int(re.findall(r"#define HR_HISTORY_API_VERSION (\d+)u", text)[0]) == ffi.HR_HISTORY_API_VERSION == 1


def test_the_other_headers_and_versions_did_not_move():
    for other in ("hrcore.h", "hrcore_aov.h", "hrcore_group.h", "hrcore_denoise.h", "hrcore_adaptive.h", "hrcore_history.h"):
        assert "hrcore_reproject" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert (ffi.HR_ABI_VERSION, ffi.HR_AOV_API_VERSION, ffi.HR_GROUP_API_VERSION, ffi.HR_DENOISE_API_VERSION, ffi.HR_ADAPTIVE_API_VERSION, ffi.HR_HISTORY_API_VERSION) == (6, 1, 1, 1, 1, 1)
    lib = core.load_library()
    for fn, want in (("hr_abi_version", 6), ("hr_aov_api_version", 1), ("hr_group_api_version", 1), ("hr_denoise_api_version", 1), ("hr_adaptive_api_version", 1),
                     ("hr_history_api_version", 1)):
        f = getattr(lib, fn)
        f.restype = ctypes.c_uint32
        assert f() == want, fn


def test_library_exports_every_symbol_and_the_version_matches():
    lib = core.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), name
    lib.hr_reproject_api_version.restype = ctypes.c_uint32
    assert lib.hr_reproject_api_version() == ffi.HR_REPROJECT_API_VERSION == 1


@pytest.mark.parametrize("struct, cname", [(ffi.ReprojectResult, "hr_reproject_result"), (ffi.ReprojectPreviewResult, "hr_reproject_preview_result")])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname):
    fields = [n for n, _ in struct._fields_]
    src = tmp_path / "rp.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrcore_reproject.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n'
                   + "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + "  return (int)HR_REPROJECT_API_VERSION - 1;\n}\n")
    exe = tmp_path / "rp"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(v) for v in out.stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_reproject_merge, lib.hr_reproject_examined_get, lib.hr_reproject_preview, lib.hr_reproject_preview_readback):
        fn.restype = ctypes.c_int
    pp = ffi.PassParams()
    r, pr = ffi.ReprojectResult(), ffi.ReprojectPreviewResult()
    buf = (ctypes.c_uint8 * 16)()
    p = ctypes.POINTER(ctypes.c_float)()
    assert lib.hr_reproject_merge(None, ctypes.byref(pp), None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_reproject_examined_get(None, buf) != ffi.HR_OK
    assert lib.hr_reproject_preview(None, ctypes.byref(pp), None, buf, None, ctypes.byref(pr)) != ffi.HR_OK
    assert lib.hr_reproject_preview_readback(None, ctypes.byref(pp), None, ctypes.byref(p), None, None, ctypes.byref(pr)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_reproject_calls_raise(oracle_lib):
    eng = ffi.Engine(oracle_lib, "ora_")
    eng.resize(4, 4)
    pp = ffi.PassParams()
    for call in (lambda: eng.reproject_merge(pp), lambda: eng.reproject_preview(pp), lambda: eng.reproject_preview_to_device(16, pp), eng.reproject_examined):
        with pytest.raises(ffi.EngineError, match="no progressive history merge"):
            call()
    eng.close()


def test_group_engine_inherits_the_calls():
    for name in ("reproject_merge", "reproject_preview", "reproject_preview_to_device", "reproject_examined"):
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
