"""Resource budgets of the progressive-merge and preview kernels (heatray_amd/csrc/hr_reproject.hip), checked at build time like
test_history_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled.  The register counts,
the waves per SIMD and the LDS are pinned at what the build gives (DESIGN.md has them): k_reproject_merge is k_history_merge with the
examined word in front — its own pixel and the twelve gathered float4 of the four taps held at once, the same occupancy —;
k_reproject_preview holds eight gathered float4 and stages the 36 x 12 guide records of its tile (a float4 and a class byte each) in LDS."""
from kernel_resources import resources


def test_reproject_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_reproject.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_reproject_merge", "k_reproject_preview"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    assert kernels["k_reproject_merge"]["LDS Size"] == 5 * 4                        # the workgroup's five counters
    assert kernels["k_reproject_preview"]["LDS Size"] == 36 * 12 * (16 + 1) + 3 * 4  # the guide records, their classes, three counters
    assert (kernels["k_reproject_merge"]["VGPRs"], kernels["k_reproject_merge"]["Occupancy"]) == (86, 5), kernels["k_reproject_merge"]
    assert (kernels["k_reproject_preview"]["VGPRs"], kernels["k_reproject_preview"]["Occupancy"]) == (48, 8), kernels["k_reproject_preview"]
    # what five and eight waves per SIMD hold: the budgets behind the recorded counts
    assert kernels["k_reproject_merge"]["VGPRs"] <= 96 and kernels["k_reproject_preview"]["VGPRs"] <= 64
