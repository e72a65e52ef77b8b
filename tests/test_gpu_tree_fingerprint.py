"""The tree builder's fingerprint (hr_build.hip: buildLBVH) against a recording of an earlier library: for every scene of
test_gpu_sah_subtrees.SCENES — the smallest shapes that reach each branch of the build: the root is a leaf (1), no PLOC below 4 triangles, no
SAH rebuild at 64 or fewer, a PLOC tree too deep for the traversal stack (deep) — under each builder setting, the counts and costs the build
reports equal tests/golden/tree_fingerprints.json, floats by their bits.  The order of the nodes within a level is not deterministic
(k_collapse4 appends with atomics), which is why the fingerprint is counts and costs and not node bytes.  The fixture is made by
tests/golden/record_tree_fingerprints.py from the library of the commit it names, never from the library under test."""
import json
import os
import struct

import pytest

from heatray_amd import core
from test_gpu_sah_subtrees import SCENES

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_fingerprints.json")
TUNES = ("", "sahsub=0", "ploc=0", "ploc=2")
SCENE_FIELDS = ("n_triangles", "n_nodes", "bvh_levels", "builder", "cost_radix", "cost_ploc")
# the fields a recording may not leave out as unstable
REQUIRED = ("n_nodes", "bvh_levels", "builder", "subtrees_found", "subtrees_replaced")


def _plain(v):
    """a ctypes field as JSON: integers as they are, a float as the hex of its float32 bits, an array as a list"""
    if isinstance(v, float):
        return "f32:" + struct.pack("<f", v).hex()
    if isinstance(v, int):
        return v
    return [_plain(x) for x in v]


def fingerprint(scene, tune):
    """what a fresh engine reports after building `scene` under HR_TUNE=`tune` (the caller restores the environment)"""
    os.environ["HR_TUNE"] = tune
    g = core.create_engine()
    try:
        scene.apply(g)
        info, tree = g.scene_info(), g.tree_info()
        fp = {k: _plain(getattr(info, k)) for k in SCENE_FIELDS}
        fp.update({k: _plain(getattr(tree, k)) for k, _ in tree._fields_})
        return fp
    finally:
        g.close()


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_recording_covers_every_case_and_every_required_field(recorded):
    assert set(recorded["cases"]) == {f"{name}|{tune}" for name in SCENES for tune in TUNES}
    assert set(REQUIRED) <= set(recorded["fields"])


@pytest.mark.parametrize("name", list(SCENES))
def test_the_build_reports_what_the_recorded_library_reported(monkeypatch, recorded, name):
    monkeypatch.setenv("HR_TUNE", "")  # (restored after the test; fingerprint() sets it per build)
    scene = SCENES[name]()
    for tune in TUNES:
        got = fingerprint(scene, tune)
        want = recorded["cases"][f"{name}|{tune}"]
        print(f"{name} HR_TUNE={tune!r}: {got}")
        assert {k: got[k] for k in recorded["fields"]} == want, (name, tune)
