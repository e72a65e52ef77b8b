"""The lifetimes of the post-process features' state on the GPU: a context that has lived (every feature called, the frame resized and
cleared, the AOV planes narrowed and widened again) gives, byte for byte and counter for counter, what a fresh context gives for its
last step alone.

The frame is 40 x 24 with 32-pixel tiles, a partial tile on each axis, and 24 x 40 in between.  One plain context and one group of two
members on device 0 take the same walk; the group is compared with the plain context in the features that serve a group."""
import pytest

from device_support import BOTH, render_passes, same
from heatray_amd import _ffi as ffi
from heatray_amd import core, scenes

pytestmark = pytest.mark.gpu
MOMENTS = ffi.HR_AOV_MOMENTS
WIDE = lambda: scenes.cornell_box(width=40, height=24, bounces=2)
TALL = lambda: scenes.cornell_box(width=24, height=40, bounces=2)


def features(eng, sc, group):
    """every feature that serves this kind of context, called once: ({name: image}, {name: result counters})"""
    images, counters = {"frame": eng.readback()}, {}
    images["denoise"] = eng.denoise()
    images["denoise_spatial"], counters["denoise_spatial"] = eng.denoise_spatial(with_result=True)
    images["despeckle_denoise"], counters["despeckle"] = eng.despeckle_denoise(with_result=True)
    counters["adaptive"] = eng.adaptive_update(install=True).as_dict()
    images["adaptive error"] = eng.adaptive_error()
    mask, installed = eng.sample_mask()
    assert installed
    images["sample mask"] = mask
    if not group:
        eng.history_capture(sc.options.pass_params(0))
        for k, plane in enumerate(eng.history()):
            images[f"history H{k}"] = plane
        counters["history"] = eng.history_info()
    counters["metric"] = eng.metric_estimate()
    counters["exposure"] = eng.exposure_meter()
    images["frame after"] = eng.readback()
    return images, counters


def last_step(eng, group):
    """the walk's last step, and all a fresh context is given: 40 x 24, two passes with both AOV masks, every feature"""
    sc = WIDE()
    eng.resize(sc.width, sc.height)
    render_passes(eng, sc, range(2))
    return features(eng, sc, group)


def walk(eng, group):
    wide, tall = WIDE(), TALL()
    wide.apply(eng)
    eng.set_aovs(BOTH)
    render_passes(eng, wide, range(2))
    features(eng, wide, group)                                  # 1. every feature once
    eng.resize(tall.width, tall.height)                         # 2.
    assert eng.history_info() == (False, 0)                     # (the history went with the frame's size)
    assert not eng.sample_mask()[1]
    eng.clear()                                                 # 3.
    eng.set_aovs(BOTH)
    render_passes(eng, tall, range(2))
    features(eng, tall, group)
    if not group:
        pp = tall.options.pass_params(0)
        assert eng.history_merge(pp)["reused_pixels"] > 0
        with pytest.raises(ffi.EngineError, match="already been merged"):
            eng.history_merge(pp)
        eng.clear()
        eng.render_pass(pp)
        assert eng.history_merge(pp)["reused_pixels"] > 0       # (after hr_clear a second merge is allowed again)
    eng.set_aovs(MOMENTS)                                       # 4.
    with pytest.raises(ffi.EngineError, match="denoise needs the AOV planes: hr_aov_enable.*enabled mask: 2"):
        eng.denoise()
    eng.set_aovs(BOTH)                                          # 5.
    eng.clear()
    return last_step(eng, group)                                # 6.


def compare(got, want, what):
    for name, image in got[0].items():
        same(image, want[0][name], f"{what}: {name}")
    for name, result in got[1].items():
        assert repr(result) == repr(want[1][name]), (what, name, result, want[1][name])


@pytest.fixture(scope="module")
def fresh():
    eng = core.create_engine()
    WIDE().apply(eng)
    eng.set_aovs(BOTH)
    out = last_step(eng, False)
    eng.close()
    assert (out[0]["frame"][..., 3] == 2).all() and out[1]["history"] == (True, 2)
    return out


def test_a_context_that_has_lived_equals_a_fresh_one(fresh):
    eng = core.create_engine()
    got = walk(eng, False)
    eng.close()
    assert sorted(got[0]) == sorted(fresh[0]) and sorted(got[1]) == sorted(fresh[1])
    compare(got, fresh, "plain context")


def test_a_group_that_has_lived_equals_the_fresh_plain_context(fresh):
    grp = core.create_group([0, 0])
    got = walk(grp, True)
    grp.close()
    assert "denoise_spatial" in got[0] and "exposure" in got[1] and "history" not in got[1]
    compare(got, fresh, "group of 2")
