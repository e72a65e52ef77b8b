"""Resource bounds of the motion-reprojection kernels (heatray_amd/csrc/hr_motion.hip), checked at build time like
test_query_kernel_resources.py (no GPU needed: hipcc cross-compiles gfx950).  k_motion_trace runs the render's traverse, so it may need
no more VGPRs, LDS or scratch than k_debug_trace (hr_trace.hip) does on the same commit: the LDS is traverse's stack (the workgroup's
three counters reuse its first words behind a barrier), the scratch traverse's private overflow stack, no vector register is spilled;
that is why the resolve is fused behind the walk instead of being a second kernel.  k_motion_merge has k_history_merge's shape: its own
pixel and the twelve gathered float4 at once, nothing in scratch, no LDS beyond the three counters.  The two streaming kernels use
neither LDS nor scratch and run at full occupancy."""
from kernel_resources import resources


def kernels(src):
    return {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in resources(src).items() if "k_" in k}


def test_motion_kernels_keep_their_resources():
    ref = kernels("hr_trace.hip")["k_debug_trace"]
    got = kernels("hr_motion.hip")
    assert sorted(got) == ["k_motion_merge", "k_motion_snapshot", "k_motion_trace", "k_motion_vectors"], sorted(got)
    for name, r in got.items():
        assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
    t = got["k_motion_trace"]
    assert t["VGPRs"] <= ref["VGPRs"] and t["LDS Size"] <= ref["LDS Size"] and t["ScratchSize"] <= ref["ScratchSize"], (t, ref)
    assert t["Occupancy"] >= ref["Occupancy"], (t, ref)
    assert t["LDS Size"] == 16 * 64 * 4 * 4  # [4 waves][kStackLDS = 16][64 lanes] ints: traverse's stack and nothing else
    m = got["k_motion_merge"]
    assert m["ScratchSize"] == 0 and m["SGPRs Spill"] == 0 and m["LDS Size"] == 3 * 4, m  # the workgroup's three counters
    hist = kernels("hr_history.hip")["k_history_merge"]
    assert m["Occupancy"] >= hist["Occupancy"], (m, hist)  # (two more float4 of its own pixel: no wave per SIMD lost to them)
    for name in ("k_motion_snapshot", "k_motion_vectors"):
        r = got[name]
        assert r["ScratchSize"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0 and r["Occupancy"] == 8, (name, r)
