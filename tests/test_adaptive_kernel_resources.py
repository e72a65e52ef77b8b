"""Resource budgets of the adaptive-sampling kernels (heatray_amd/csrc/hr_adaptive.hip), checked at build time like
test_denoise_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled; the streaming
kernels run at full occupancy without LDS; k_adaptive_mask stays inside the LDS its tile and halo need.  That the sample mask's load in
cameraLane leaves the ray generators their occupancy is test_kernel_resources.py's business (unchanged: the packet kernel still runs
eight waves per SIMD)."""
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


def test_adaptive_kernels_use_no_scratch_and_only_the_lds_of_tile_and_halo():
    res = _resources("hr_adaptive.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_adaptive_error", "k_adaptive_mask", "k_mask_pack", "k_mask_unpack"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (name, r)
        assert r["Occupancy"] >= 8, (name, r)
    for name in ("k_adaptive_error", "k_mask_pack", "k_mask_unpack"):
        assert kernels[name]["LDS Size"] == 0, (name, kernels[name])
    # a tile of 64 x 16 pixels and a halo of HR_ADAPTIVE_MAX_RADIUS = 4, one byte per entry: the unconverged flags of tile + halo
    # ((16 + 8) x (64 + 8)), their maximum along the rows ((16 + 8) x 64), and four words for the workgroup's counts and maximum
    tw, th, r = 64, 16, 4
    assert kernels["k_adaptive_mask"]["LDS Size"] == (th + 2 * r) * (tw + 2 * r) + (th + 2 * r) * tw + 4 * 4

