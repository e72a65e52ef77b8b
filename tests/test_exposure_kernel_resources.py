"""Resource budgets of the auto-exposure kernels (heatray_amd/csrc/hr_exposure.hip), checked at build time like
test_reproject_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled, no AGPRs.  The LDS
is what the design says: k_exposure_hist holds the workgroup's 256 bins (1 KB) and its four class counters, k_exposure_reduce the 256
64-bit words of its scan, k_exposure_display nothing.  The register counts and the waves per SIMD are pinned at what the build
gives (DESIGN.md has them): all three are far below the 64 VGPRs at which occupancy begins to fall."""
from kernel_resources import resources


def test_exposure_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_exposure.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_exposure_display", "k_exposure_hist", "k_exposure_reduce"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    assert kernels["k_exposure_hist"]["LDS Size"] == 256 * 4 + 4 * 4  # the bins, the four class counters
    assert kernels["k_exposure_reduce"]["LDS Size"] == 256 * 8        # the scan's 64-bit words, one per bin
    assert kernels["k_exposure_display"]["LDS Size"] == 0
    assert (kernels["k_exposure_hist"]["VGPRs"], kernels["k_exposure_hist"]["Occupancy"]) == (33, 8), kernels["k_exposure_hist"]
    assert (kernels["k_exposure_reduce"]["VGPRs"], kernels["k_exposure_reduce"]["Occupancy"]) == (10, 8), kernels["k_exposure_reduce"]
    assert (kernels["k_exposure_display"]["VGPRs"], kernels["k_exposure_display"]["Occupancy"]) == (26, 8), kernels["k_exposure_display"]
