"""Resource budgets of the progressive-merge and preview kernels (heatray_amd/csrc/hr_reproject.hip), checked at build time like
test_history_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled.  The register counts,
the waves per SIMD and the LDS are pinned at what the build gives (DESIGN.md has them): k_reproject_merge is k_history_merge with the
examined word in front — its own pixel and the twelve gathered float4 of the four taps held at once, the same occupancy —;
k_reproject_preview holds eight gathered float4 and stages the 36 x 12 guide records of its tile (a float4 and a class byte each) in LDS."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heatray_amd", "csrc")


def _resources(src):
    flags = subprocess.run(["make", "-s", "-C", CSRC, "print-flags"], capture_output=True, text=True, check=True).stdout.split()
    out = subprocess.run(["/opt/rocm/bin/hipcc", *flags, "-c", os.path.join(CSRC, src), "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, cwd=CSRC)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    return res


def test_reproject_kernels_use_no_scratch_and_keep_their_registers():
    res = _resources("hr_reproject.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_reproject_merge", "k_reproject_preview"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    assert kernels["k_reproject_merge"]["LDS Size"] == 5 * 4                        # the workgroup's five counters
    assert kernels["k_reproject_preview"]["LDS Size"] == 36 * 12 * (16 + 1) + 3 * 4  # the guide records, their classes, three counters
    assert (kernels["k_reproject_merge"]["VGPRs"], kernels["k_reproject_merge"]["Occupancy"]) == (85, 5), kernels["k_reproject_merge"]
    assert (kernels["k_reproject_preview"]["VGPRs"], kernels["k_reproject_preview"]["Occupancy"]) == (45, 8), kernels["k_reproject_preview"]
