"""The host side's owning handles without a GPU: heatray_amd/csrc/hr_owned.h (device buffer, pinned buffer, event, stream: what frees
everything a context holds) compiled against a counting fake of the HIP calls it makes (tests/host/fake_hip, first on the include path),
under AddressSanitizer and UBSan, and run as a program of its own.  tests/host/owned_cpu.cpp holds the checks: each handle's life cycle
and moves, reserve's grow-only rule, an aggregate shaped like hr_ctx::Group with every creation call failing in turn, and a struct of
handles assigned a default-constructed one."""
import os
import subprocess

import cpu_header


def test_handles_free_once_and_a_failed_creation_leaks_nothing(tmp_path):
    fake = os.path.join(cpu_header.ROOT, "tests", "host", "fake_hip")
    exe = cpu_header.build("owned", tmp_path, flags=("-I" + fake, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "owned cpu: ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
