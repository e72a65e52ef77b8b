"""Resource bounds of the ray-query kernels (heatray_amd/csrc/hr_query.hip), checked at build time like test_deform_kernel_resources.py (no
GPU needed: hipcc cross-compiles gfx950).  Every k_query_trace variant runs the render's traverse, so it may need no more VGPRs, LDS or
scratch than k_debug_trace (hr_trace.hip) does on the same commit: the LDS is traverse's stack, the scratch traverse's private overflow
stack, no vector register is spilled.  That holds for the variant that writes surface records too, which is why the surface step is fused behind
traverse instead of being a second kernel.  k_query_camera uses neither LDS nor scratch."""
from kernel_resources import resources


def kernels(src):
    return {k.replace("void ", "").replace("hr::", "").split("(")[0]: v for k, v in resources(src).items() if "k_" in k}


def test_query_kernels_need_no_more_than_the_debug_trace():
    ref = kernels("hr_trace.hip")["k_debug_trace"]
    got = kernels("hr_query.hip")
    assert sorted(got) == ["k_query_camera", "k_query_trace<false, false>", "k_query_trace<false, true>", "k_query_trace<true, false>"], sorted(got)
    for name, r in got.items():
        # (no vector register goes to scratch.  The occlusion variant, like k_debug_trace, keeps some scalar registers in lanes of a VGPR
        # — alphaPasses' texture fetch is inlined in both — and the VGPR counts compared below include those.)
        assert r["VGPRs Spill"] == 0 and r["AGPRs"] == 0, (name, r)
        if name == "k_query_camera":
            assert r["ScratchSize"] == 0 and r["LDS Size"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8, (name, r)
            continue
        assert r["VGPRs"] <= ref["VGPRs"] and r["LDS Size"] <= ref["LDS Size"] and r["ScratchSize"] <= ref["ScratchSize"], (name, r, ref)
        assert r["Occupancy"] >= ref["Occupancy"], (name, r, ref)
        assert r["LDS Size"] == 16 * 64 * 4 * 4  # [4 waves][kStackLDS = 16][64 lanes] ints: traverse's stack and nothing else
