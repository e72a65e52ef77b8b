"""include/hrcore_motion.h without a GPU: the binding's symbol list is the header's declarations and shares no name with any other
header's, the library exports them with the binding's version, the three structs have the layout gcc gives them, no other header's
version moved, the library's defaults are the binding's, every refusal the header names has its message in the entry points (the GPU
test provokes each of them), calls without a context fail loudly, an Engine bound to a library without the symbols (the CPU oracle)
still constructs, and the group engine inherits the calls."""
import ctypes
import os
import re

import pytest

import abi_checks
from heatray_amd import _ffi as ffi
from heatray_amd import core, motion

HEADER = "hrcore_motion.h"
NAMES = ["hr_motion_api_version", "hr_motion_default_params", "hr_motion_snapshot", "hr_motion_trace", "hr_motion_merge", "hr_motion_vectors",
         "hr_motion_vectors_readback", "hr_motion_readback", "hr_motion_snapshot_readback", "hr_motion_drop", "hr_motion_info"]
CALLS = ("motion_snapshot", "motion_trace", "motion_merge", "motion_planes", "motion_vectors", "motion_vectors_to_device", "motion_snapshot_triangles",
         "motion_drop", "motion_info")
OTHERS = ("hrcore_exposure.h", "hrcore_tree.h", "hrcore_metric.h", "hrcore_despeckle.h", "hrcore_mesh.h", "hrcore_deform.h", "hrcore_query.h")


def test_binding_header_and_library_agree():
    assert sorted("hr_" + s for s in ffi.MOTION_SYMBOLS) == abi_checks.declared_functions(HEADER) == sorted(NAMES)
    for header in tuple(abi_checks.HEADERS) + OTHERS:  # the calls are absent from every other header, and none of them includes this one
        assert not set("hr_" + s for s in ffi.MOTION_SYMBOLS) & set(abi_checks.declared_functions(header)), header
        assert '#include "hrcore_motion.h"' not in abi_checks.header_text(header), header
    for feature, (symbols, _, _) in ffi.FEATURES.items():
        assert feature == "motion" or not set(ffi.MOTION_SYMBOLS) & set(symbols), feature
    assert not set(ffi.MOTION_SYMBOLS) & set(ffi.ABI_SYMBOLS) and not set(ffi.MOTION_SYMBOLS) & set(ffi.GROUP_SYMBOLS)
    lib = core.load_library()
    for s in ffi.MOTION_SYMBOLS:
        assert hasattr(lib, "hr_" + s), s
    lib.hr_motion_api_version.restype = ctypes.c_uint32
    assert lib.hr_motion_api_version() == ffi.HR_MOTION_API_VERSION == 1
    assert ffi.FEATURES["motion"] == (ffi.MOTION_SYMBOLS, ffi.HR_MOTION_API_VERSION, "motion reprojection")


def test_no_other_version_moved():
    abi_checks.check_no_version_moved()
    lib = core.load_library()
    for fn in (lib.hr_exposure_api_version, lib.hr_tree_api_version, lib.hr_metric_api_version, lib.hr_despeckle_api_version, lib.hr_mesh_api_version,
               lib.hr_deform_api_version, lib.hr_query_api_version):
        fn.restype = ctypes.c_uint32
        assert fn() == (2 if fn is lib.hr_tree_api_version else 1)


def test_constants_match_the_header():
    text = abi_checks.header_text(HEADER)
    assert int(re.findall(r"#define HR_MOTION_API_VERSION (\d+)u", text)[0]) == ffi.HR_MOTION_API_VERSION
    assert '#include "hrcore_history.h"' in text


@pytest.mark.parametrize("struct, cname, size", [(ffi.MotionTraceResult, "hr_motion_trace_result", 32), (ffi.MotionResult, "hr_motion_result", 56),
                                                 (ffi.MotionInfo, "hr_motion_info_t", 24)])
def test_header_compiles_as_c_and_the_structs_have_gccs_layout(tmp_path, struct, cname, size):
    abi_checks.check_struct_layout(tmp_path, HEADER, struct, cname, "HR_MOTION_API_VERSION")
    assert ctypes.sizeof(struct) == size


def test_the_librarys_defaults_are_the_bindings():
    lib = core.load_library()
    lib.hr_motion_default_params.restype = None
    p = ffi.HistoryParams(-1, -1.0, -1.0, -1.0, (9, 9, 9, 9))
    lib.hr_motion_default_params(ctypes.byref(p))
    assert bytes(p) == bytes(motion.default_params())
    assert (p.max_history, list(p.reserved)) == (32, [0, 0, 0, 0])
    assert (p.normal_cos, p.plane_tol, p.min_weight) == (ctypes.c_float(0.8).value, ctypes.c_float(0.02).value, ctypes.c_float(0.25).value)
    lib.hr_motion_default_params(None)  # (a null pointer is ignored)


# what hr_last_error says for each refusal (tests/test_gpu_motion.py provokes every one of them on a device)
REFUSALS = {
    "a null camera": ": null camera",
    "a non-finite camera": ": the camera (view_matrix, fov_tan, aspect_ratio) is not finite",
    "no snapshot": ": no snapshot (hr_motion_snapshot; hr_motion_drop removes it)",
    "no captured history": "motion merge: no captured history (hr_history_capture; hr_frame_resize and hr_history_drop remove it)",
    "scene not committed": '"scene not committed"',
    "a second merge": "motion merge: a history has already been merged into this frame (one merge per hr_clear, of whatever kind: a second would count it twice)",
    "no trace": "no trace at this frame size (hr_motion_trace or hr_motion_merge; hr_frame_resize and hr_motion_drop remove it)",
    "no old camera": "motion vectors: no old camera and no captured history to take it from",
    "null output": ": null output",
    "alignment": "motion vectors: the output must be 16-byte aligned",
}
SHARED = {  # refusals the entry points take over from the history's and the post-process plumbing's checks
    "hr_postprocess.inl": ["a context group is not supported", "a tile-sharded context (world > 1)", '"no frame"', "the frame is empty (0 passes)",
                           " needs the AOV planes: hr_aov_enable(HR_AOV_SURFACE | HR_AOV_MOMENTS)"],
    "hr_history.inl": ["history: max_history = ", "history: normal_cos must lie in -1 .. 1", "history: plane_tol must be finite and greater than 0",
                       "history: min_weight must be greater than 0 and at most 1"],
}


def test_every_refusal_has_its_message():
    csrc = os.path.join(abi_checks.ROOT, "heatray_amd", "csrc")
    inl = open(os.path.join(csrc, "hr_motion.inl")).read()
    for what, text in REFUSALS.items():
        assert text in inl, what
    for name, texts in SHARED.items():
        src = open(os.path.join(csrc, name)).read()
        for text in texts:
            assert text in src, (name, text)
    for call in ("historyCheckParams", "historyCheckFrame", "frameKindReady"):  # ... and the entry points do go through those checks
        assert call + "(" in inl, call
    assert inl.count("FAIL(c, HR_ERR_INVALID") == inl.count("FAIL(")  # every refusal is HR_ERR_INVALID


def test_calls_without_a_context_fail_loudly():
    lib = core.load_library()
    for name in NAMES[2:]:
        getattr(lib, name).restype = ctypes.c_int
    pp, tr, r, info = ffi.PassParams(), ffi.MotionTraceResult(), ffi.MotionResult(), ffi.MotionInfo()
    buf = (ctypes.c_float * 32)()
    assert lib.hr_motion_snapshot(None) != ffi.HR_OK
    assert lib.hr_motion_trace(None, ctypes.byref(pp), ctypes.byref(tr)) != ffi.HR_OK
    assert lib.hr_motion_merge(None, ctypes.byref(pp), None, ctypes.byref(r)) != ffi.HR_OK
    assert lib.hr_motion_vectors(None, ctypes.byref(pp), buf, None) != ffi.HR_OK
    assert lib.hr_motion_vectors_readback(None, ctypes.byref(pp), buf) != ffi.HR_OK
    assert lib.hr_motion_readback(None, buf) != ffi.HR_OK
    assert lib.hr_motion_snapshot_readback(None, buf) != ffi.HR_OK
    assert lib.hr_motion_drop(None) != ffi.HR_OK
    assert lib.hr_motion_info(None, ctypes.byref(info)) != ffi.HR_OK


def test_engine_without_the_symbols_constructs_and_its_motion_calls_raise(oracle_lib):
    pp = ffi.PassParams()

    def calls(eng):
        eng.resize(4, 4)
        return (eng.motion_snapshot, lambda: eng.motion_trace(pp), lambda: eng.motion_merge(pp), eng.motion_planes, eng.motion_vectors,
                lambda: eng.motion_vectors_to_device(1024), eng.motion_snapshot_triangles, eng.motion_drop, eng.motion_info)
    abi_checks.check_oracle_engine_lacks(oracle_lib, calls, "this library has no motion reprojection")


def test_group_engine_inherits_the_calls():
    abi_checks.check_group_engine_inherits(CALLS)
