"""CPU-side checks of the context-group boundary (include/hrcore_group.h): the library exports what the header declares, the
ctypes mirror has gcc's layout, create_group fails loudly without a device, the C++ layer's HEATRAY_DEVICES parser, and the
layer's group path under ThreadSanitizer / AddressSanitizer against the do-nothing stubs."""
import ctypes
import os
import re
import subprocess

import pytest

from heatray_amd import _ffi as ffi
from heatray_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "heatray_amd", "host")


def group_declared_functions():
    text = open(os.path.join(ROOT, "include", "hrcore_group.h")).read()
    return sorted(set(re.findall(r"\b(hr_[a-z0-9_]+)\s*\(", text)))


def test_group_header_and_python_binding_agree():
    assert sorted("hr_" + s for s in ffi.GROUP_SYMBOLS) == group_declared_functions()
    assert not set(ffi.GROUP_SYMBOLS) & set(ffi.ABI_SYMBOLS)


def test_library_exports_every_group_symbol():
    lib = core.load_library()
    for name in group_declared_functions():
        assert hasattr(lib, name), name
    lib.hr_group_api_version.restype = ctypes.c_uint32
    assert lib.hr_group_api_version() == ffi.HR_GROUP_API_VERSION


def test_group_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "hrcore_group.h")).read()
    assert int(re.findall(r"#define HR_GROUP_API_VERSION (\d+)u", text)[0]) == ffi.HR_GROUP_API_VERSION
    assert int(re.findall(r"#define HR_GROUP_MAX_MEMBERS (\d+)", text)[0]) == ffi.HR_GROUP_MAX_MEMBERS


def test_group_info_has_the_layout_gcc_gives_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hrcore_group.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(hr_group_info));']
    for fname, _ in ffi.GroupInfo._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(hr_group_info, {fname}));')
    lines += ["return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(ffi.GroupInfo) == 200
    for fname, _ in ffi.GroupInfo._fields_:
        assert int(got[fname]) == getattr(ffi.GroupInfo, fname).offset, fname


def test_no_device_means_create_group_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(ffi.EngineError):
        core.create_group()
    with pytest.raises(ffi.EngineError):
        core.create_group([0, 0])


@pytest.fixture(scope="module")
def device_list_exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("devlist") / "device_list_test"
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), "-I", HOST,
                    os.path.join(ROOT, "tests", "host", "device_list_test.cpp"), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


@pytest.mark.parametrize("text,want", [
    ("all", "ok all"), ("0", "ok 0"), ("0,1,2,3", "ok 0 1 2 3"), ("0,0", "ok 0 0"), ("0,0,0", "ok 0 0 0"), ("7,3,7", "ok 7 3 7"),
    (",".join(["0"] * 16), "ok " + " ".join(["0"] * 16)),
])
def test_heatray_devices_good_lists(device_list_exe, text, want):
    assert subprocess.run([device_list_exe, text], capture_output=True, text=True, check=True).stdout.strip() == want


@pytest.mark.parametrize("text", ["", "ALL", "al", "0,", ",0", "0,,1", "0 ,1", " 0", "-1", "+1", "0;1", "1.5", "x", "0,a",
                                  ",".join(["0"] * 17), "99999999999"])
def test_heatray_devices_bad_lists(device_list_exe, text):
    assert subprocess.run([device_list_exe, text], capture_output=True, text=True, check=True).stdout.startswith("error HEATRAY_DEVICES=")


@pytest.mark.parametrize("devices,members", [("0,0", "2 members on devices 0,0"), ("all", "1 members on devices 0")])
@pytest.mark.parametrize("san,env", [("tsan", {"TSAN_OPTIONS": "halt_on_error=1"}),
                                     ("asan", {"ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1"})])
def test_layer_group_path_under_sanitizers(san, env, devices, members):
    # PassGenerator's HEATRAY_DEVICES path (parse, hr_ctx_create_group, the member report, every later call on the group handle)
    # against the stubs (tests/host/hrcore_stub.cpp + tests/host/hrcore_group_stub.cpp, which sees one device)
    subprocess.check_call(["make", "-C", HOST, san], stdout=subprocess.DEVNULL)
    exe = os.path.join(ROOT, "tests", "host", f"host_threading_{san}")
    out = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, HEATRAY_DEVICES=devices, **env), timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    assert "threading checks: ok" in out.stdout
    assert f"PassGenerator: context group of {members}" in out.stdout
    assert "WARNING: ThreadSanitizer" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr
