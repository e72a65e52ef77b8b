"""Resource budgets of the denoiser's kernels (heatray_amd/csrc/hr_denoise.hip), checked at build time like test_kernel_resources.py
(no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch; the a-trous kernels keep a row of five taps' loads in flight and
still seven waves per SIMD (all 25 taps in flight cost 190 VGPRs and left two), and the tiled ones stay inside the LDS their tile and
halo need."""
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


def test_denoise_kernels_use_no_scratch_and_keep_their_occupancy():
    res = _resources("hr_denoise.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_denoise" in k}
    assert sorted(kernels) == ["k_denoise_atrous", "k_denoise_atrous_tiled<1>", "k_denoise_atrous_tiled<2>", "k_denoise_finish", "k_denoise_gradient",
                               "k_denoise_prepare"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    for name in ("k_denoise_prepare", "k_denoise_gradient", "k_denoise_finish"):
        assert kernels[name]["Occupancy"] >= 8 and kernels[name]["LDS Size"] == 0, (name, kernels[name])
    assert kernels["k_denoise_atrous"]["LDS Size"] == 0
    # tile + halo: (16 + 4 STEP)^2 entries of 16 + 16 + 4 bytes
    assert kernels["k_denoise_atrous_tiled<1>"]["LDS Size"] == 20 * 20 * 36
    assert kernels["k_denoise_atrous_tiled<2>"]["LDS Size"] == 24 * 24 * 36
    for name in ("k_denoise_atrous", "k_denoise_atrous_tiled<1>", "k_denoise_atrous_tiled<2>"):
        assert kernels[name]["VGPRs"] <= 72 and kernels[name]["Occupancy"] >= 7, (name, kernels[name])
