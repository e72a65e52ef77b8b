"""Resource budgets of the adaptive-sampling kernels (heatray_amd/csrc/hr_adaptive.hip), checked at build time like
test_denoise_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled; the streaming
kernels run at full occupancy without LDS; k_adaptive_mask stays inside the LDS its tile and halo need.  That the sample mask's load in
cameraLane leaves the ray generators their occupancy is test_kernel_resources.py's business (unchanged: the packet kernel still runs
eight waves per SIMD)."""
from kernel_resources import resources


def test_adaptive_kernels_use_no_scratch_and_only_the_lds_of_tile_and_halo():
    res = resources("hr_adaptive.hip")
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

