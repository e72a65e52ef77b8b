"""CPU-side checks of the denoiser's boundary (include/hrcore_denoise.h): the header, the Python binding and the library agree, the
symbols are disjoint from the three other headers', the params struct has the layout gcc gives it, calls without a context fail
loudly, and an Engine bound to the CPU oracle (which has no denoiser) still constructs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hrcore_denoise.h")


def declared_functions():
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", open(HEADER).read(), re.M)))


def test_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.DENOISE_SYMBOLS) == declared_functions()
    for other in (ffi.ABI_SYMBOLS, ffi.GROUP_SYMBOLS, ffi.AOV_SYMBOLS):
        assert not set(ffi.DENOISE_SYMBOLS) & set(other)


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.findall(r"#define HR_DENOISE_API_VERSION (\d+)u", text)[0]) == ffi.HR_DENOISE_API_VERSION
    for name in ("MAX_ITERATIONS", "MAX_NORMAL_POWER", "KERNEL_AUTO", "KERNEL_PLAIN", "KERNEL_TILED"):
        assert int(re.findall(rf"#define HR_DENOISE_{name} (\d+)", text)[0]) == getattr(ffi, "HR_DENOISE_" + name), name


def test_the_other_headers_and_versions_did_not_move():
    assert "hrcore_denoise" not in open(os.path.join(ROOT, "include", "hrcore.h")).read()
    assert "hrcore_denoise" not in open(os.path.join(ROOT, "include", "hrcore_aov.h")).read()
    assert (ffi.HR_ABI_VERSION, ffi.HR_AOV_API_VERSION, ffi.HR_GROUP_API_VERSION) == (6, 1, 1)


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    lib = core.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), name
    lib.hr_denoise_api_version.restype = ctypes.c_uint32
    assert lib.hr_denoise_api_version() == ffi.HR_DENOISE_API_VERSION
    p = ffi.DenoiseParams(-1, -1, -1.0, -1.0, -1, (9, 9, 9))
    lib.hr_denoise_default_params.restype = None
    lib.hr_denoise_default_params(ctypes.byref(p))
    d = denoise.default_params()
    assert bytes(p) == bytes(d)
    assert (p.iterations, p.normal_power, p.sigma_l, p.sigma_z, p.kernel, list(p.reserved)) == (5, 7, 4.0, 4.0, 0, [0, 0, 0])
    lib.hr_denoise_default_params(None)  # (a null pointer is ignored)


def test_header_compiles_as_c_and_the_struct_has_gccs_layout(tmp_path):
    fields = [n for n, _ in ffi.DenoiseParams._fields_]
    src = tmp_path / "dn.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrcore_denoise.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(hr_denoise_params));\n'
                   + "".join(f'  printf(" %zu", offsetof(hr_denoise_params, {f}));\n' for f in fields)
                   + "  return (int)HR_DENOISE_API_VERSION - 1 + HR_DENOISE_KERNEL_AUTO;\n}\n")
    exe = tmp_path / "dn"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(v) for v in out.stdout.split()]
    assert got == [ctypes.sizeof(ffi.DenoiseParams)] + [getattr(ffi.DenoiseParams, f).offset for f in fields]


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    p = ctypes.POINTER(ctypes.c_float)()
    w, h, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32()
    for fn in (lib.hr_denoise, lib.hr_denoise_readback, lib.hr_denoise_display):
        fn.restype = ctypes.c_int
    assert lib.hr_denoise(None, None, ctypes.c_void_p(16), None, ctypes.byref(n)) != ffi.HR_OK
    assert lib.hr_denoise_readback(None, None, ctypes.byref(p), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)) != ffi.HR_OK
    dp = ffi.display_params()
    assert lib.hr_denoise_display(None, None, ctypes.byref(dp), ctypes.c_int32(0), ctypes.c_void_p(16), ctypes.byref(n)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_denoise_calls_raise(oracle_lib):
    eng = ffi.Engine(oracle_lib, "ora_")
    for call in (eng.denoise, lambda: eng.denoise(denoise.default_params()), lambda: eng.denoise_to_device(16), lambda: eng.denoise_display(16)):
        with pytest.raises(ffi.EngineError, match="no denoiser"):
            call()
    eng.close()


def test_group_engine_inherits_the_calls():
    for name in ("denoise", "denoise_to_device", "denoise_display"):
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
