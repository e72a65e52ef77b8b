"""The HR_TUNE knobs without a GPU: heatray_amd/csrc/hr_tune.h (the defaults, the one table, the parser hr_ctx_create runs before its
first HIP call) compiled for the CPU under AddressSanitizer and UBSan and run as a program of its own (tests/host/tune_parse_cpu.cpp
holds the checks: defaults, round trips, first value wins, the malformed strings, every string the suite and the tools set); and what
hr_ctx_create does with a malformed string."""
import subprocess

import pytest

import cpu_header


def test_the_table_and_the_parser(tmp_path):
    exe = cpu_header.build("tune_parse", tmp_path, flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "tune parse cpu: ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_a_malformed_hr_tune_fails_context_creation_before_the_device(monkeypatch, capfd):
    # the check sits in front of hr_ctx_create's first HIP call: HR_ERR_INVALID (1) and a line that names the item, with or without a GPU
    # (without one a well-formed string gets as far as the device count and fails with HR_ERR_DEVICE instead)
    import ctypes

    from heatray_amd import _ffi as ffi
    from heatray_amd import core

    lib = core.load_library()
    lib.hr_ctx_create.restype = ctypes.c_int
    for tune, item in (("packets=1,leaf=4", "leaf=4"), ("groups=4,batch=16", "groups=4"), ("tblk=0", "tblk=0"), ("packets=1x", "packets=1x")):
        monkeypatch.setenv("HR_TUNE", tune)
        ctx = ctypes.c_void_p()
        assert lib.hr_ctx_create(None, ctypes.byref(ctx)) == 1 and not ctx.value, tune
        err = capfd.readouterr().err
        assert "hr_ctx_create: HR_TUNE:" in err and item in err, (tune, err)
        with pytest.raises(ffi.EngineError, match="HR_TUNE"):
            core.create_engine()
        capfd.readouterr()


@pytest.mark.gpu
def test_hr_tune_is_checked_when_an_engine_is_made(monkeypatch, capfd):
    import numpy as np

    from heatray_amd import core, scenes

    monkeypatch.setenv("HR_TUNE", "packets=1,leaf=4")
    with pytest.raises(core.EngineError):
        core.create_engine()
    assert "leaf=4" in capfd.readouterr().err
    sc = scenes.cornell_box(32, 32, bounces=3, passes=4)
    frames = []
    for tune in ("", "packets=1,"):  # (nothing to parse; an empty item after the last comma)
        monkeypatch.setenv("HR_TUNE", tune)
        eng = core.create_engine()
        sc.apply(eng)
        for s in range(2):
            eng.render_pass(sc.options.pass_params(s))
        frames.append(eng.readback())
        eng.close()
        assert frames[-1].shape == (32, 32, 4) and (frames[-1][..., 3] == 2.0).all() and np.isfinite(frames[-1]).all() and frames[-1][..., :3].max() > 0.0
    assert frames[0].tobytes() == frames[1].tobytes()  # (how the camera rays travel never changes the bits)
