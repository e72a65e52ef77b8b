"""CPU-side checks of the spatial variance estimate's boundary (include/hrcore_denoise_spatial.h): the header, the Python binding and the
library agree, the symbols are disjoint from the other headers', the structs have the layout gcc gives them, the older headers did not
move, calls without a context fail loudly, and an Engine bound to the CPU oracle (which has no denoiser) still constructs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise_spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hrcore_denoise_spatial.h")


def declared_functions():
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", open(HEADER).read(), re.M)))


def test_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.DENOISE_SPATIAL_SYMBOLS) == declared_functions()
    for other in (ffi.ABI_SYMBOLS, ffi.GROUP_SYMBOLS, ffi.AOV_SYMBOLS, ffi.DENOISE_SYMBOLS, ffi.ADAPTIVE_SYMBOLS, ffi.HISTORY_SYMBOLS, ffi.REPROJECT_SYMBOLS):
        assert not set(ffi.DENOISE_SPATIAL_SYMBOLS) & set(other)


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.findall(r"#define HR_DENOISE_SPATIAL_API_VERSION (\d+)u", text)[0]) == ffi.HR_DENOISE_SPATIAL_API_VERSION == 1
    for name in ("BELOW_LOWEST", "BELOW_HIGHEST", "MIN_TAPS_LOWEST", "MIN_TAPS_HIGHEST"):
        assert int(re.findall(rf"#define HR_DENOISE_SPATIAL_{name} (\d+)", text)[0]) == getattr(ffi, "HR_DENOISE_SPATIAL_" + name), name
    assert '#include "hrcore_denoise.h"' in text


def test_the_other_headers_and_versions_did_not_move():
    for other in ("hrcore.h", "hrcore_aov.h", "hrcore_adaptive.h", "hrcore_history.h", "hrcore_reproject.h", "hrcore_group.h"):
        assert "denoise_spatial" not in open(os.path.join(ROOT, "include", other)).read(), other
    dn = open(os.path.join(ROOT, "include", "hrcore_denoise.h")).read()
    assert "#define HR_DENOISE_API_VERSION 1u" in dn and "uint32_t reserved[3]; /* 0 */" in dn
    assert (ffi.HR_ABI_VERSION, ffi.HR_AOV_API_VERSION, ffi.HR_GROUP_API_VERSION, ffi.HR_DENOISE_API_VERSION) == (6, 1, 1, 1)
    assert ctypes.sizeof(ffi.DenoiseParams) == 32


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    lib = core.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), name
    lib.hr_denoise_spatial_api_version.restype = ctypes.c_uint32
    assert lib.hr_denoise_spatial_api_version() == ffi.HR_DENOISE_SPATIAL_API_VERSION
    p = ffi.DenoiseSpatialParams(-1, -1, (9, 9, 9, 9, 9, 9))
    lib.hr_denoise_spatial_default_params.restype = None
    lib.hr_denoise_spatial_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(denoise_spatial.default_params())
    assert (p.below, p.min_taps, list(p.reserved)) == (4, 6, [0] * 6)
    lib.hr_denoise_spatial_default_params(None)  # (a null pointer is ignored)


def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path):
    src = tmp_path / "ds.c"
    lines = []
    for struct, cls in (("hr_denoise_spatial_params", ffi.DenoiseSpatialParams), ("hr_denoise_spatial_result", ffi.DenoiseSpatialResult)):
        lines.append(f'  printf(" %zu", sizeof({struct}));\n')
        lines += [f'  printf(" %zu", offsetof({struct}, {f}));\n' for f, _ in cls._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrcore_denoise_spatial.h"\nint main(void) {\n' + "".join(lines)
                   + "  return (int)HR_DENOISE_SPATIAL_API_VERSION - 1;\n}\n")
    exe = tmp_path / "ds"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    want = []
    for cls in (ffi.DenoiseSpatialParams, ffi.DenoiseSpatialResult):
        want += [ctypes.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert [int(v) for v in out.stdout.split()] == want
    assert (ctypes.sizeof(ffi.DenoiseSpatialParams), ctypes.sizeof(ffi.DenoiseSpatialResult)) == (32, 24)


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    p = ctypes.POINTER(ctypes.c_float)()
    w, h, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32()
    r = ffi.DenoiseSpatialResult()
    for fn in (lib.hr_denoise_spatial, lib.hr_denoise_spatial_readback, lib.hr_denoise_spatial_display, lib.hr_denoise_spatial_variance):
        fn.restype = ctypes.c_int
    assert lib.hr_denoise_spatial(None, None, None, ctypes.c_void_p(16), None, ctypes.byref(n), ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_denoise_spatial_readback(None, None, None, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n), ctypes.byref(r)) != ffi.HR_OK
    dp = ffi.display_params()
    assert lib.hr_denoise_spatial_display(None, None, None, ctypes.byref(dp), ctypes.c_int32(0), ctypes.c_void_p(16), ctypes.byref(n)) != ffi.HR_OK
    out = (ctypes.c_float * 4)()
    assert lib.hr_denoise_spatial_variance(None, None, None, out, ctypes.byref(r)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_calls_raise(oracle_lib):
    eng = ffi.Engine(oracle_lib, "ora_")
    eng.width = eng.height = 2
    for call in (eng.denoise_spatial, lambda: eng.denoise_spatial(None, denoise_spatial.default_params()), lambda: eng.denoise_spatial_to_device(16),
                 lambda: eng.denoise_spatial_display(16), eng.denoise_spatial_variance):
        with pytest.raises(ffi.EngineError, match="no spatial variance estimate"):
            call()
    eng.close()


def test_group_engine_inherits_the_calls():
    for name in ("denoise_spatial", "denoise_spatial_to_device", "denoise_spatial_display", "denoise_spatial_variance"):
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
