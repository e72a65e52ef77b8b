"""Register budgets of the hot kernels, checked at build time (no GPU needed: hipcc cross-compiles gfx950).

k_trace sits EXACTLY at the VGPR count that lets five waves share a SIMD (96); one more register group and the kernel runs four
waves per SIMD, 4.5 % slower (measured in round 4, when an inlined prologue did just that: profiles/r4n_trace_occupancy.txt).
The compiler's remarks are the cheapest guard."""
from kernel_resources import resources


def test_trace_and_shade_kernels_keep_their_occupancy():
    res = resources("hr_trace.hip")
    trace = [v for k, v in res.items() if "k_trace<false>" in k]
    assert len(trace) == 1, list(res)
    assert trace[0]["Occupancy"] >= 5 and trace[0]["VGPRs"] <= 96 and trace[0]["VGPRs Spill"] == 0, trace[0]
    res = resources("hr_shade.hip")
    hits = [v for k, v in res.items() if "k_shade_hit<0, 0>" in k]
    assert len(hits) == 1 and hits[0]["Occupancy"] >= 4 and hits[0]["VGPRs"] <= 128, hits
    sort = [v for k, v in res.items() if "k_shade_sort" in k]
    assert len(sort) == 1 and sort[0]["Occupancy"] >= 8, sort
    res = resources("hr_raygen.hip")
    # the packet kernel hides the latency of its scalar node fetches behind other waves: eight per SIMD, nothing in scratch
    pkt = [v for k, v in res.items() if "k_raygen_packets<false, true>" in k]   # (pass parameters through the scalar cache: the usual batch)
    assert len(pkt) == 1 and pkt[0]["Occupancy"] >= 8 and pkt[0]["ScratchSize"] == 0, pkt
    pkt = [v for k, v in res.items() if "k_raygen_packets<false, false>" in k]  # (every lane its own pass's parameters)
    assert len(pkt) == 1 and pkt[0]["Occupancy"] >= 6 and pkt[0]["ScratchSize"] == 0, pkt
