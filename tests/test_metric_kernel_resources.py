"""Resource budgets of the convergence-metric kernel (heatray_amd/csrc/hr_metric.hip), checked at build time like
test_exposure_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled, no AGPRs.  The LDS
is what the design says: both instances of k_metric_accumulate hold the workgroup's two sets of 256 64-bit bins in four lane-striped
copies (16 KB), four class counters and the word of the maximum.  The register counts and the waves per SIMD are pinned at what the build
gives (DESIGN.md has them): both stay within the 64 VGPRs up to which a SIMD holds 8 waves."""
from kernel_resources import resources


def test_metric_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_metric.hip")
    kernels = {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_metric_accumulate<0>", "k_metric_accumulate<1>"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        bins, counters = 4 * 2 * 256 * 8, 5 * 4  # four copies of NUM and DEN; counted, differing, nonfinite, skipped, the bits of max_abs
        assert r["LDS Size"] == (bins + counters + 7) // 8 * 8 == 16408, (name, r)  # (the block's size is a multiple of the bins' alignment)
    assert (kernels["k_metric_accumulate<0>"]["VGPRs"], kernels["k_metric_accumulate<0>"]["Occupancy"]) == (64, 8), kernels["k_metric_accumulate<0>"]
    assert (kernels["k_metric_accumulate<1>"]["VGPRs"], kernels["k_metric_accumulate<1>"]["Occupancy"]) == (56, 8), kernels["k_metric_accumulate<1>"]
