"""Resource budgets of the mesh-preparation kernels (heatray_amd/csrc/hr_mesh.hip), checked at build time like
test_despeckle_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  Nothing in scratch, nothing spilled, no AGPRs.  The LDS
is what the design says: a 256-bin digit histogram or offset table in the sort's two kernels, the scan's sixteen wave sums and its
carry, and the few counters of the kernels that count.  The register counts and the waves per SIMD are pinned at what the build gives,
all within the 64 VGPRs up to which a SIMD holds 8 waves."""
from kernel_resources import resources

BINS = 256          # hr_mesh.hip: 8-bit digits
SCAN_WAVES = 1024 // 64  # kMsScanBlock / 64
WORD = 4

# kernel: (VGPRs, Occupancy, LDS Size)
PINNED = {
    "k_mesh_face": (48, 8, 2 * WORD),                    # degenerate, degenerate-uv
    "k_mesh_sort_hist": (10, 8, BINS * WORD),
    "k_mesh_scan": (30, 8, SCAN_WAVES * WORD + WORD),    # the wave sums and the carry
    "k_mesh_sort_scatter": (19, 8, BINS * WORD),
    "k_mesh_ranges": (8, 8, 0),
    "k_mesh_iota": (6, 8, 0),
    "k_mesh_weld_keys": (4, 8, 0),
    "k_mesh_heads": (14, 8, 0),
    "k_mesh_groups": (16, 8, 0),
    "k_mesh_vertex": (27, 8, WORD),                      # the workgroup's longest list
    "k_mesh_group": (22, 8, 0),
    "k_mesh_finish": (20, 8, 3 * WORD),                  # unreferenced, cancelled, fallback
}


def test_mesh_kernels_use_no_scratch_and_keep_their_registers():
    res = resources("hr_mesh.hip")
    kernels = {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in res.items() if "k_" in k}
    assert sorted(kernels) == sorted(PINNED), sorted(kernels)
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        assert (r["VGPRs"], r["Occupancy"], r["LDS Size"]) == PINNED[name] and r["VGPRs"] <= 64, (name, r)
