"""Resource budgets of the spatial variance estimate's kernel (heatray_amd/csrc/hr_denoise_spatial.hip), checked at build time like
test_denoise_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, no spill, no AGPRs; the LDS is the
staged tile and the counters and nothing else (a struct copied through a private array once showed up as 3072 more bytes of it)."""
from kernel_resources import resources


def test_spatial_kernel_uses_no_scratch_and_only_its_tile_of_lds():
    res = resources("hr_denoise_spatial.hip")
    kernels = {k.split("(")[0].replace("void ", "").replace("hr::", ""): v for k, v in res.items()}
    assert sorted(kernels) == ["k_spatial_variance"], sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    r = kernels["k_spatial_variance"]
    # tile + halo of 3: 22 x 22 entries of 16 (normal, depth) + 4 (lum of the colour) + 4 (lum of the albedo) + 4 (n) + 4 (cov) bytes,
    # and four words of counters
    assert r["LDS Size"] == 22 * 22 * 32 + 16 and r["LDS Size"] <= 16 * 1024, r
    # A record of what the build shows, not a target: 84 VGPRs (a row of seven taps in flight, every weight computed again in the second
    # pass) are five waves per SIMD (512 / 5 = 102, in granules of 8: up to 96 registers keep the fifth wave); the LDS allows ten
    # workgroups per CU.  Keeping the 49 weights between the passes needs both loops unrolled (registers have no dynamic index):
    # that build showed 256 VGPRs and one wave per SIMD.
    assert r["VGPRs"] <= 96 and r["Occupancy"] >= 5, r
