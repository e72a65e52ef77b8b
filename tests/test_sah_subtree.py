"""The full-sweep SAH rebuild of the radix tree's bottom subtrees without a GPU: heatray_amd/csrc/hr_sah_subtree.h (the phases of
k_sah_subtrees in hr_build.hip) compiled for the CPU under AddressSanitizer and UBSan and run lane by lane as a program of its own
(tests/host/sah_subtree_cpu.cpp holds the checks: about 10^4 bottom subtrees of radix trees built as k_karras builds them, and the
hostile ones), and its splits against a numpy port of tools/tree_proto.py's sah_sweep."""
import struct
import subprocess

import numpy as np
import pytest

import cpu_header

FLAGS = ("-g", "-O2", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cpu_header.build("sah_subtree", tmp_path_factory.mktemp("sah_subtree"), flags=FLAGS)


def test_the_phases_build_valid_subtrees_that_are_never_dearer_or_deeper(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "sah subtree cpu: ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def area(lo, hi):
    d = hi - lo
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def sweep_costs(ids, lo, hi):
    """sah_sweep's candidates of one range (tools/tree_proto.py), in float32 like the header: per axis the ids in centroid order (equal
    centroids by index, a stable sort) and cost[k - 1] = A_L k + A_R (n - k) for k = 1 .. n - 1"""
    c = (lo[ids] + hi[ids]) * np.float32(0.5)
    n = len(ids)
    per_axis = []
    for ax in range(3):
        s = ids[np.argsort(c[:, ax], kind="stable")]
        l0, l1 = np.minimum.accumulate(lo[s], 0), np.maximum.accumulate(hi[s], 0)
        r0, r1 = np.minimum.accumulate(lo[s][::-1], 0)[::-1], np.maximum.accumulate(hi[s][::-1], 0)[::-1]
        k = np.arange(1, n)
        cost = area(l0[k - 1], l1[k - 1]) * k.astype(np.float32) + area(r0[k], r1[k]) * (n - k).astype(np.float32)
        assert cost.dtype == np.float32
        per_axis.append((s, cost))
    return per_axis


def test_the_header_picks_sah_sweeps_split_wherever_the_best_cost_is_unique(exe):
    rng = np.random.default_rng(7)
    subtrees = []
    for m in [3, 4, 5, 8, 17, 33, 63, 64] + list(rng.integers(3, 65, 56)):
        kind = len(subtrees) % 4
        c = rng.random((m, 3), dtype=np.float32)
        if kind == 1:  # flat in one axis
            c[:, 2] = np.float32(0.5)
        if kind == 2:  # clustered: many near-equal centroids
            c = np.round(c * 4) / np.float32(4)
        e = (0.01 + 0.1 * rng.random((m, 3), dtype=np.float32) ** 2).astype(np.float32)
        if kind == 3:
            e[:] = 0
        subtrees.append(((c - e).astype(np.float32), (c + e).astype(np.float32)))
    blob = struct.pack("<i", len(subtrees)) + b"".join(
        struct.pack("<i", len(lo)) + np.concatenate([lo, hi], 1).astype("<f4").tobytes() for lo, hi in subtrees)
    got = np.frombuffer(cpu_header.run(exe, blob), dtype="<i4").reshape(-1, 2)
    assert len(got) == sum(len(lo) - 1 for lo, _ in subtrees)
    at = unique = nodes = 0
    for lo, hi in subtrees:
        m = len(lo)
        splits = got[at:at + m - 1]
        at += m - 1
        todo = [(0, np.arange(m))]  # (node slot, its leaves): hr_sah_subtree.h's slot rule
        while todo:
            slot, ids = todo.pop()
            n = len(ids)
            axis, k = (int(v) for v in splits[slot])
            assert 0 <= axis < 3 and 1 <= k < n
            per_axis = sweep_costs(ids, lo, hi)
            allc = np.concatenate([c for _, c in per_axis])
            best = allc.min()
            nodes += 1
            # the header's choice is a least-cost candidate ...
            assert per_axis[axis][1][k - 1] == best, (m, slot, axis, k)
            # ... and THE candidate sah_sweep takes (argmin: the first k of the first axis) — that is the tie rule; where the least
            # cost is unique nothing else could be right
            first_axis = min(a for a in range(3) if per_axis[a][1].min() == best)
            assert (axis, k) == (first_axis, int(np.argmin(per_axis[first_axis][1])) + 1), (m, slot)
            unique += int((allc == best).sum() == 1)
            s = per_axis[axis][0]
            if k > 1:
                todo.append((slot + 1, np.sort(s[:k])))
            if n - k > 1:
                todo.append((slot + k, np.sort(s[k:])))
    # (a node of two leaves never has a unique best: its one split is a candidate of all three axes; the others usually have)
    assert nodes == len(got) and unique > 0


def test_the_sahsub_knob_parses_like_the_knobs_of_the_first_table(tmp_path):
    knobs = cpu_header.build("tune_build_knobs", tmp_path, flags=FLAGS)
    out = subprocess.run([str(knobs)], capture_output=True, text=True)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "tune build knobs cpu: ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
