"""The CPU builds of the kernels' per-pixel headers (tests/host/NAME_cpu.cpp over heatray_amd/csrc/hr_NAME.h): how the test_*_ref.py
files compile one and run it on the bytes of an input file."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(name, tmp_dir, flags=()):
    """tests/host/NAME_cpu.cpp compiled into tmp_dir (with further compiler flags, e.g. a sanitizer's); returns the program's path"""
    exe = tmp_dir / (name + "_cpu")
    # -ffp-contract=off like the library: the header's float lines must mean the same on both sides
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", *flags, "-I" + os.path.join(ROOT, "heatray_amd", "csrc"),
                           os.path.join(ROOT, "tests", "host", name + "_cpu.cpp"), "-o", str(exe)])
    return exe


def run(exe, in_bytes):
    """the bytes the program writes for this input; its exit status and stderr if it does not end with its "... cpu: ok" line"""
    d = exe.parent
    (d / "in.bin").write_bytes(in_bytes)
    out = subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and exe.name.replace("_", " ") + ": ok" in out.stdout, (out.returncode, out.stderr)
    return (d / "out.bin").read_bytes()
