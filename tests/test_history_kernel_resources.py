"""Resource budgets of the history-reprojection kernels (heatray_amd/csrc/hr_history.hip), checked at build time like
test_adaptive_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled.  The register counts
and the waves per SIMD are pinned at what the build gives (DESIGN.md has them): k_history_capture is a streaming kernel at full
occupancy; k_history_merge holds its own pixel (four float4) and the twelve gathered float4 of its four taps at once — that is the point
of issuing every load before the first decision — and pays for it with occupancy."""
from kernel_resources import resources


def test_history_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_history.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_history_capture", "k_history_merge"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    assert kernels["k_history_capture"]["LDS Size"] == 0
    assert kernels["k_history_merge"]["LDS Size"] == 3 * 4  # the workgroup's three counters
    assert (kernels["k_history_capture"]["VGPRs"], kernels["k_history_capture"]["Occupancy"]) == (42, 8), kernels["k_history_capture"]
    assert (kernels["k_history_merge"]["VGPRs"], kernels["k_history_merge"]["Occupancy"]) == (82, 5), kernels["k_history_merge"]
    assert kernels["k_history_merge"]["VGPRs"] <= 96  # what five waves per SIMD hold: the budget behind the recorded count
