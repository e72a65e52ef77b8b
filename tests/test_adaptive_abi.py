"""CPU-side checks of the adaptive-sampling boundary (include/hrcore_adaptive.h): the header, the Python binding and the library agree,
the symbols are disjoint from the four other headers', both structs have the layout gcc gives them, the other versions did not move,
calls without a context fail loudly, and an Engine bound to the CPU oracle (which has none of this) still constructs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import adaptive, core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hrcore_adaptive.h")


def declared_functions():
    return sorted(set(re.findall(r"^(?:int|void|uint32_t)\s+(hr_[a-z0-9_]+)\s*\(", open(HEADER).read(), re.M)))


def test_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.ADAPTIVE_SYMBOLS) == declared_functions()
    for other in (ffi.ABI_SYMBOLS, ffi.GROUP_SYMBOLS, ffi.AOV_SYMBOLS, ffi.DENOISE_SYMBOLS):
        assert not set(ffi.ADAPTIVE_SYMBOLS) & set(other)


def test_constants_match_the_header():
    text = open(HEADER).read()
    assert int(re.findall(r"#define HR_ADAPTIVE_API_VERSION (\d+)u", text)[0]) == ffi.HR_ADAPTIVE_API_VERSION == 1
    for name in ("MIN_SAMPLES_LOWEST", "MIN_SAMPLES_HIGHEST", "MAX_RADIUS"):
        assert int(re.findall(rf"#define HR_ADAPTIVE_{name} (\d+)", text)[0]) == getattr(ffi, "HR_ADAPTIVE_" + name), name


def test_the_other_headers_and_versions_did_not_move():
    for other in ("hrcore.h", "hrcore_aov.h", "hrcore_group.h", "hrcore_denoise.h"):
        assert "hrcore_adaptive" not in open(os.path.join(ROOT, "include", other)).read(), other
    assert (ffi.HR_ABI_VERSION, ffi.HR_AOV_API_VERSION, ffi.HR_GROUP_API_VERSION, ffi.HR_DENOISE_API_VERSION) == (6, 1, 1, 1)
    lib = core.load_library()
    for fn, want in (("hr_abi_version", 6), ("hr_aov_api_version", 1), ("hr_group_api_version", 1), ("hr_denoise_api_version", 1)):
        f = getattr(lib, fn)
        f.restype = ctypes.c_uint32
        assert f() == want, fn


def test_library_exports_every_symbol_and_the_version_and_defaults_match():
    lib = core.load_library()
    for name in declared_functions():
        assert hasattr(lib, name), name
    lib.hr_adaptive_api_version.restype = ctypes.c_uint32
    assert lib.hr_adaptive_api_version() == ffi.HR_ADAPTIVE_API_VERSION == 1
    p = ffi.AdaptiveParams(-1.0, -1.0, -1, -1, (9, 9, 9, 9))
    lib.hr_adaptive_default_params.restype = None
    lib.hr_adaptive_default_params(ctypes.byref(p))
    d = adaptive.default_params()
    assert bytes(p) == bytes(d)
    assert (p.min_samples, p.radius, list(p.reserved)) == (16, 2, [0, 0, 0, 0])
    assert (p.threshold, p.floor) == (ctypes.c_float(0.02).value, ctypes.c_float(0.05).value)
    assert p.radius >= 1  # (the header's known limit: radius 0 switches pixels off for good)
    lib.hr_adaptive_default_params(None)  # (a null pointer is ignored)


@pytest.mark.parametrize("struct, cname", [(ffi.AdaptiveParams, "hr_adaptive_params"), (ffi.AdaptiveResult, "hr_adaptive_result")])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname):
    fields = [n for n, _ in struct._fields_]
    src = tmp_path / "ad.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hrcore_adaptive.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n'
                   + "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields)
                   + "  return (int)HR_ADAPTIVE_API_VERSION - 1;\n}\n")
    exe = tmp_path / "ad"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0
    got = [int(v) for v in out.stdout.split()]
    assert got == [ctypes.sizeof(struct)] + [getattr(struct, f).offset for f in fields]


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for fn in (lib.hr_sample_mask_set, lib.hr_sample_mask_get, lib.hr_adaptive_update, lib.hr_adaptive_error_copy, lib.hr_adaptive_error_readback):
        fn.restype = ctypes.c_int
    buf = (ctypes.c_uint8 * 16)()
    inst = ctypes.c_int32()
    r = ffi.AdaptiveResult()
    assert lib.hr_sample_mask_set(None, buf) != ffi.HR_OK
    assert lib.hr_sample_mask_get(None, buf, ctypes.byref(inst)) != ffi.HR_OK
    assert lib.hr_adaptive_update(None, None, ctypes.c_int32(1), ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_adaptive_error_copy(None, ctypes.c_void_p(16), None) != ffi.HR_OK
    assert lib.hr_adaptive_error_readback(None, ctypes.cast(buf, ctypes.POINTER(ctypes.c_float))) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_adaptive_calls_raise(oracle_lib):
    eng = ffi.Engine(oracle_lib, "ora_")
    eng.resize(4, 4)
    import numpy as np
    for call in (lambda: eng.set_sample_mask(None), lambda: eng.set_sample_mask(np.ones((4, 4), np.uint8)), eng.sample_mask, eng.adaptive_update,
                 eng.adaptive_error, lambda: eng.adaptive_error_to_device(16)):
        with pytest.raises(ffi.EngineError, match="no adaptive sampling"):
            call()
    eng.close()


def test_group_engine_inherits_the_calls():
    for name in ("set_sample_mask", "sample_mask", "adaptive_update", "adaptive_error", "adaptive_error_to_device"):
        assert getattr(ffi.GroupEngine, name) is getattr(ffi.Engine, name)
