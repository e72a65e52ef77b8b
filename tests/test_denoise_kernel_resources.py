"""Resource budgets of the denoiser's kernels (heatray_amd/csrc/hr_denoise.hip), checked at build time like test_kernel_resources.py
(no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch; the a-trous kernels keep a row of five taps' loads in flight and
still seven waves per SIMD (all 25 taps in flight cost 190 VGPRs and left two), and the tiled ones stay inside the LDS their tile and
halo need."""
from kernel_resources import resources


def test_denoise_kernels_use_no_scratch_and_keep_their_occupancy():
    res = resources("hr_denoise.hip")
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
