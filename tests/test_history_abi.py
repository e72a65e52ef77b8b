"""CPU-side checks of the history-reprojection boundary (include/hrcore_history.h): the header, the Python binding and the library agree,
the symbols are disjoint from the five other headers', both structs have the layout gcc gives them, the other versions did not move,
calls without a context fail loudly, and an Engine bound to the CPU oracle (which has none of this) still constructs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core, history

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hrcore_history.h")


def declared_functions():
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", open(HEADER).read(), re.M)))


def test_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.HISTORY_SYMBOLS) == declared_functions()
    for other in (ffi.ABI_SYMBOLS, ffi.GROUP_SYMBOLS, ffi.AOV_SYMBOLS, ffi.DENOISE_SYMBOLS, ffi.ADAPTIVE_SYMBOLS):
        assert not set(ffi.HISTORY_SYMBOLS) & set(other)
    for name in ("hr_history_capture", "hr_history_merge", "hr_history_drop", "hr_history_info", "hr_history_default_params", "hr_history_api_version"):
        assert name in declared_functions(), name


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.findall(r"#define HR_HISTORY_API_VERSION (\d+)u", text)[0]) == ffi.HR_HISTORY_API_VERSION == 1
    for name in ("MAX_HISTORY_LOWEST", "MAX_HISTORY_HIGHEST"):
        assert int(re.findall(rf"#define HR_HISTORY_{name} (\d+)", text)[0]) == getattr(ffi, "HR_HISTORY_" + name), name
    assert '#include "hrcore_aov.h"' in text


def test_the_other_headers_and_versions_did_not_move():
    for other in ("hrcore.h", "hrcore_aov.h", "hrcore_group.h", "hrcore_denoise.h", "hrcore_adaptive.h"):
        assert "hrcore_history" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert (ffi.HR_ABI_VERSION, ffi.HR_AOV_API_VERSION, ffi.HR_GROUP_API_VERSION, ffi.HR_DENOISE_API_VERSION, ffi.HR_ADAPTIVE_API_VERSION) == (6, 1, 1, 1, 1)
    lib = core.load_library()
    for fn, want in (("hr_abi_version", 6), ("hr_aov_api_version", 1), ("hr_group_api_version", 1), ("hr_denoise_api_version", 1), ("hr_adaptive_api_version", 1)):
        f = getattr(lib, fn)
        f.restype = ctypes.c_uint32
        assert f() == want, fn


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    lib = core.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), name
    lib.hr_history_api_version.restype = ctypes.c_uint32
    assert lib.hr_history_api_version() == ffi.HR_HISTORY_API_VERSION == 1
    p = ffi.HistoryParams(-1, -1.0, -1.0, -1.0, (9, 9, 9, 9))
    lib.hr_history_default_params.restype = None
    lib.hr_history_default_params(ctypes.byref(p))
    d = history.default_params()
    assert bytes(p) == bytes(d)
    assert (p.max_history, list(p.reserved)) == (32, [0, 0, 0, 0])
    assert (p.normal_cos, p.plane_tol, p.min_weight) == (ctypes.c_float(0.9).value, ctypes.c_float(0.02).value, ctypes.c_float(0.25).value)
    lib.hr_history_default_params(None)  # (a null pointer is ignored)


@pytest.mark.parametrize("struct, cname", [(ffi.HistoryParams, "hr_history_params"), (ffi.HistoryResult, "hr_history_result")])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname):
    fields = [n for n, _ in struct._fields_]
    src = tmp_path / "hs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrcore_history.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n'
                   + "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + "  return (int)HR_HISTORY_API_VERSION - 1;\n}\n")
    exe = tmp_path / "hs"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(v) for v in out.stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_history_capture, lib.hr_history_merge, lib.hr_history_drop, lib.hr_history_info, lib.hr_history_readback):
        fn.restype = ctypes.c_int
    pp = ffi.PassParams()
    r = ffi.HistoryResult()
    have, n = ctypes.c_int32(), ctypes.c_uint32()
    buf = (ctypes.c_float * 48)()
    assert lib.hr_history_capture(None, ctypes.byref(pp)) != ffi.HR_OK
    assert lib.hr_history_merge(None, ctypes.byref(pp), None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_history_drop(None) != ffi.HR_OK
    assert lib.hr_history_info(None, ctypes.byref(have), ctypes.byref(n)) != ffi.HR_OK
    assert lib.hr_history_readback(None, buf) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_history_calls_raise(oracle_lib):
    eng = ffi.Engine(oracle_lib, "ora_")
    eng.resize(4, 4)
    pp = ffi.PassParams()
    for call in (lambda: eng.history_capture(pp), lambda: eng.history_merge(pp), eng.history_drop, eng.history_info, eng.history):
        with pytest.raises(ffi.EngineError, match="no history reprojection"):
            call()
    eng.close()


def test_group_engine_inherits_the_calls():
    for name in ("history_capture", "history_merge", "history_drop", "history_info", "history"):
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
