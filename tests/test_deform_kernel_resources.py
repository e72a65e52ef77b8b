"""Resource budgets of the deformable-mesh kernels (heatray_amd/csrc/hr_deform.hip), checked at build time like
test_mesh_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled, no AGPRs, at most the 64
VGPRs up to which a SIMD holds 8 waves.  The only LDS is the pose kernel's two counters.  The register counts are pinned at what the build
gives: k_deform_pose poses, finishes and stores one output before it begins the next (hr_deform.h), which is what keeps it at 42; posed
joint by joint with all four outputs in flight it took 76."""
from kernel_resources import resources

WORD = 4

# kernel: (VGPRs, Occupancy, LDS Size)
PINNED = {
    "k_deform_gather": (8, 8, 0),
    "k_deform_scatter": (8, 8, 0),
    "k_deform_pose": (42, 8, 2 * WORD),  # rejected, kept
}


def test_deform_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_deform.hip")
    kernels = {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == sorted(PINNED), sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        assert (r["VGPRs"], r["Occupancy"], r["LDS Size"]) == PINNED[name] and r["VGPRs"] <= 64, (name, r)
