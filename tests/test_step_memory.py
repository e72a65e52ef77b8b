"""The bytes of a macro step's ray memory without a GPU: heatray_amd/csrc/hr_step_memory.h (the one statement of what a pass's table entry
takes from scratch and from the step arena, which the step's need, the memory budget's record and the carve all use) compiled for the CPU
under AddressSanitizer and UBSan and run as a program of its own (tests/host/step_memory_cpu.cpp holds the checks: the segment bytes against
the pipeline's former expressions over a grid of bounds, the sum of a table against a walk of the two cursors, the budget's guarantee
against its former constants)."""
import subprocess

import cpu_header


def test_a_steps_bytes_are_what_the_pipeline_used_to_compute(tmp_path):
    exe = cpu_header.build("step_memory", tmp_path, flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "step memory cpu: ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
