"""CPU-side checks of the AOV boundary (include/hrcore_aov.h): the header, the Python binding and the library agree, the symbols are
disjoint from hrcore.h's and hrcore_group.h's, calls without a context fail loudly, the oracle-style Engine without the symbols still
constructs, and the helper that turns the sums into means never divides by zero."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import aov, core

HEADER = "hrcore_aov.h"


def test_aov_header_and_python_binding_agree():
    abi_checks.check_binding_agrees_and_is_disjoint(HEADER)


def test_aov_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_AOV_API_VERSION (\d+)u", text)[0]) == ffi.HR_AOV_API_VERSION
    assert int(re.findall(r"#define HR_AOV_SURFACE (\d+)u", text)[0]) == ffi.HR_AOV_SURFACE
    assert int(re.findall(r"#define HR_AOV_MOMENTS (\d+)u", text)[0]) == ffi.HR_AOV_MOMENTS
    for i, name in enumerate(ffi.AOV_PLANE_NAMES):
        assert int(re.findall(rf"#define HR_AOV_PLANE_{name.upper()} (\d+)", text)[0]) == i
    assert (ffi.HR_AOV_PLANE_ALBEDO, ffi.HR_AOV_PLANE_NORMAL_DEPTH, ffi.HR_AOV_PLANE_MOMENTS) == (0, 1, 2)


def test_library_exports_every_aov_symbol_and_the_version_matches():
    abi_checks.check_library_exports(HEADER)


def test_header_compiles_as_c_and_adds_no_struct(tmp_path):
    # the header declares functions and constants only: nothing whose layout a ctypes mirror would have to follow
    assert not re.search(r"\bstruct\b|\btypedef\b", abi_checks.header_text(HEADER).split("#include \"hrcore.h\"", 1)[1])
    src = tmp_path / "aov.c"
    src.write_text('#include "hrcore_aov.h"\nint main(void) { return (int)HR_AOV_API_VERSION - 1 + HR_AOV_PLANE_ALBEDO; }\n')
    exe = tmp_path / "aov"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", abi_checks.INCLUDE, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_aov_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    lib.hr_aov_enable.restype = ctypes.c_int
    assert lib.hr_aov_enable(None, ctypes.c_uint32(ffi.HR_AOV_SURFACE)) != ffi.HR_OK
    p = ctypes.POINTER(ctypes.c_float)()
    w, h, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint64()
    lib.hr_aov_readback.restype = ctypes.c_int
    assert lib.hr_aov_readback(None, ctypes.c_int32(0), ctypes.byref(p), ctypes.byref(w), ctypes.byref(h), ctypes.byref(n)) != ffi.HR_OK
    lib.hr_aov_copy.restype = ctypes.c_int
    assert lib.hr_aov_copy(None, ctypes.c_int32(0), ctypes.c_void_p(16), None) != ffi.HR_OK
    m = ctypes.c_uint32()
    lib.hr_aov_mask.restype = ctypes.c_int
    assert lib.hr_aov_mask(None, ctypes.byref(m)) != ffi.HR_OK


def test_engine_without_aov_symbols_constructs_and_its_aov_calls_raise(oracle_lib):
    # the suite binds Engine to the CPU oracle, which has no AOVs: construction must not need them
    abi_checks.check_oracle_engine_lacks(oracle_lib, lambda eng: (lambda: eng.set_aovs(ffi.HR_AOV_SURFACE), eng.aovs, eng.aov_mask, lambda: eng.aov_plane(0),
                                                                  lambda: eng.aov_to_device(0, 16)), "no AOVs")


def test_resolve_turns_sums_into_means_without_dividing_by_zero():
    H, W = 2, 3
    alb = np.zeros((H, W, 4), np.float32)
    nd = np.zeros((H, W, 4), np.float32)
    mom = np.zeros((H, W, 4), np.float32)
    frame = np.zeros((H, W, 4), np.float32)
    # pixel (0, 0): four passes, three hit a surface; samples 1, 2, 3, 6 in every channel
    alb[0, 0] = (1.5, 0.3, 0.6, 3.0)
    nd[0, 0] = (0.0, 0.0, 3.0, 7.5)
    s = np.array([1.0, 2.0, 3.0, 6.0])
    mom[0, 0] = (*(3 * [float((s * s).sum())]), 4.0)
    frame[0, 0] = (*(3 * [float(s.sum())]), 4.0)
    # pixel (0, 1): one sample only; pixel (1, 2): nothing at all
    mom[0, 1] = (4.0, 4.0, 4.0, 1.0)
    frame[0, 1] = (2.0, 2.0, 2.0, 1.0)
    with np.errstate(all="raise"):
        r = aov.resolve({"albedo": alb, "normal_depth": nd, "moments": mom, "passes": 4}, frame)
    np.testing.assert_allclose(r["albedo"][0, 0], (0.5, 0.1, 0.2), rtol=1e-6)
    np.testing.assert_allclose(r["normal"][0, 0], (0.0, 0.0, 1.0))
    assert r["depth"][0, 0] == pytest.approx(2.5)
    assert r["hits"][0, 0] == 3.0 and r["coverage"][0, 0] == pytest.approx(0.75)
    np.testing.assert_allclose(r["variance"][0, 0], 3 * [np.var(s, ddof=1) / 4], rtol=1e-6)
    assert (r["variance"][0, 1] == 0).all() and (r["variance"][1, 2] == 0).all()
    for k in ("albedo", "normal", "depth", "coverage"):
        assert np.isfinite(r[k]).all() and (r[k][1, 2] == 0).all(), k
