"""The interval box test of the camera-ray packets without a GPU: heatray_amd/csrc/hr_packet_interval.h compiled for the CPU
(tests/host/packet_interval_cpu.cpp) and fuzzed against the per-ray test it replaces in the packet kernel.

The contract is exact: a child that ANY ray's own test enters is entered by the interval test (zero violations), for random 64-byte
nodes (scale exponents at both ends of the range, flat and inverted child boxes), packets of 1..64 rays with shared and differing
origins, footprints of 1e-5 .. 0.3 rad, origins up to 10^4 node sizes away, scenes moved 10^3 .. 10^4 sizes from the world's origin,
direction components down to and below safeInv's clamp, and tlim from hits at mixed distances.  A packet whose rays disagree in the
sign of a direction component — or hold a clamped one — must be flagged for the per-ray step.

Half of the pairs are adversarial: every ray is aimed at a point whose coordinates lie exactly on one child's lower or upper planes (its
faces, edges and corners; a flat box seen edge-on), the origin sometimes exactly in such a plane, tlim a ray's own plane distance a few
ulps either way, packets of one or two rays (tight bounds: the error term alone separates the two tests), near the world's origin and
10^3 .. 10^4 node sizes from it.  These are the cases where rounding decides tn <= tf, and the fuzz does see the error term: built with
the term at 1 u instead of 8 u (HR_PKI_ERR_ULPS) the same four seeds give 2 violations, at 0.5 u the first seed alone over 400; at 2 u and above none.  (The
derived 7 u is a worst case over six roundings; what the fuzz reaches is a little over 1 u.)  test_the_fuzz_sees_a_term_too_small holds
that, so that a later edit that weakens the term does not pass unseen.

The caps on over-inclusion keep the bound from degenerating towards "always enter": over narrow, well-conditioned packets (footprint
<= 1e-3 rad, one origin, at most 100 node sizes away, no direction component below 0.05, not adversarial) the arithmetic enters 1.011
children per child some ray enters near the world's origin and 1.073 where the scene lies 10^3 .. 10^4 of the node's size away from it
(there the error term 8 u (|a| + |o|) |1/d| is a percent or two of a child box; with the term at 0 the figure is 1.005, so the term is
what the far case costs, and the rays' own rounding is of the same order).  The caps are those figures with the sampling noise of ~5000
entered children (1.5 %) and a margin: 1.05 and 1.15.  Always-enter would give 11."""
import os
import subprocess
import struct

import pytest

import cpu_header

NAMES = ("pairs stepPairs fallback violations mixedMissed anyEntered ivEntered narrowAny narrowIv narrowPairs farAny farIv farPairs "
         "openPlanes diffOrigins culledByTlim advPairs advGrazes").split()
PAIRS = 300_000


def _total(exe, seeds):
    total = dict.fromkeys(NAMES, 0)
    for seed in seeds:
        raw = cpu_header.run(exe, struct.pack("<II", seed, PAIRS))
        for k, v in zip(NAMES, struct.unpack(f"<{len(NAMES)}Q", raw)):
            total[k] += v
    return total


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    exe = cpu_header.build("packet_interval", tmp_path_factory.mktemp("packet_interval_cpu"))
    total = _total(exe, (1, 2, 3, 4))  # (four runs: 1.2 M pairs, 3.6 M child tests of the packets that take the step)
    print(total)
    return total


def test_the_fuzz_covers_what_it_claims(fuzz):
    assert fuzz["pairs"] == 4 * PAIRS >= 10 ** 6
    assert fuzz["stepPairs"] >= 10 ** 6 * 0.8 and fuzz["fallback"] > 10 ** 4
    assert fuzz["advPairs"] > 3 * 10 ** 5 and fuzz["advGrazes"] > 10 ** 5  # (child tests where a ray's tn and tf are within 4 ulps)
    assert fuzz["diffOrigins"] > 10 ** 5          # packets whose rays do not share an origin take the step too
    assert fuzz["openPlanes"] > 100                # the overflow guard was reached (exponents at the top, directions near the clamp)
    assert fuzz["culledByTlim"] > 1000             # the packet's tlim pruned children
    assert fuzz["narrowPairs"] > 10 ** 4 and fuzz["farPairs"] > 10 ** 4
    assert fuzz["anyEntered"] > 10 ** 5


def test_superset_exactly(fuzz):
    assert fuzz["violations"] == 0, fuzz


def test_mixed_signs_and_clamped_components_are_flagged(fuzz):
    assert fuzz["mixedMissed"] == 0, fuzz


def test_over_inclusion_stays_small_on_narrow_packets(fuzz):
    near = fuzz["narrowIv"] / fuzz["narrowAny"]
    far = fuzz["farIv"] / fuzz["farAny"]
    print("children entered, interval / any ray: near the origin", near, "far from it", far)
    assert fuzz["narrowIv"] >= fuzz["narrowAny"] and fuzz["farIv"] >= fuzz["farAny"]
    assert near <= 1.05, near
    assert far <= 1.15, far


def test_the_fuzz_sees_a_term_too_small(tmp_path_factory):
    # the same program over a header whose error term is 1 u (0.5 u) instead of 8 u: the superset property must be seen to break
    d = tmp_path_factory.mktemp("packet_interval_weak")
    for ulps, seeds, at_least in (("1.0f", (1, 2, 3, 4), 1), ("0.5f", (1,), 50)):
        exe = d / "packet_interval_cpu"
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-DHR_PKI_ERR_ULPS=" + ulps, "-I" + os.path.join(cpu_header.ROOT, "heatray_amd", "csrc"),
                               os.path.join(cpu_header.ROOT, "tests", "host", "packet_interval_cpu.cpp"), "-o", str(exe)])
        got = _total(exe, seeds)
        print("error term", ulps, "u:", got["violations"], "violations")
        assert got["violations"] >= at_least, (ulps, got)
