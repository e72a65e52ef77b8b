"""Resource budgets of the firefly-suppression kernel (heatray_amd/csrc/hr_despeckle.hip), checked at build time like
test_metric_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled, no AGPRs.  The LDS is
what the design says: the luminances of the workgroup's 16 x 16 tile with its two-pixel halo, and the five counters.  The register count
and the waves per SIMD are pinned at what the build gives (DESIGN.md has them), within the 64 VGPRs up to which a SIMD holds 8 waves."""
from kernel_resources import resources


def test_despeckle_kernel_uses_no_scratch_and_keeps_its_registers():
    res = resources("hr_despeckle.hip")
    kernels = {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == ["k_despeckle"], sorted(kernels)
    r = kernels["k_despeckle"]
    assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, r
    tile, halo, counters = 16, 2, 5
    assert r["LDS Size"] == (tile + 2 * halo) ** 2 * 4 + counters * 4 == 1620, r
    assert (r["VGPRs"], r["Occupancy"]) == (34, 8) and r["VGPRs"] <= 64, r
