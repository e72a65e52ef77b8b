"""The convergence metric (include/hrcore_metric.h) on the GPU.  Every comparison with the reference is exact: the result's doubles to
the bit, the counts and all 2 x 256 bins equal.

 1. synthetic pairs as device images where the kernel can go wrong: tiny and odd sizes, windows, every class, only the last pixel
    differing, every term in one bin, all 255 bins in every workgroup
 2. one 1920 x 1080 pair: the grid-stride loop under the capped grid
 3. a rendered cornell box: 8 passes against a kept copy of its 64-pass frame, within 1e-6 of convergence.rel_l2, without a flush, a pure
    post-process, repeatable
 4. metric_estimate against its reference; its refusals
 5. context groups of 2 and 3 members give the plain context's result and bins for both kinds; a tile shard is refused
 6. the other refusals, metric_last
 7. convergence.run_on_device gives run_with_readback's pass count."""
import ctypes as C

import numpy as np
import pytest

from device_support import engine_with_passes, render_passes, same
from heatray_amd import _ffi as ffi
from heatray_amd import convergence, core, metric, scenes
from metric_frames import (CLASS_PIXELS, F, SIZES, all_bins_pair, class_rows, constant_difference, last_pixel_differs, params, same_bins,
                           same_result, seeded_pair, windows)

pytestmark = pytest.mark.gpu


def device(image):
    import torch
    return torch.from_numpy(np.ascontiguousarray(image, F)).to("cuda:0")


def blank_engine(W, H):
    eng = core.create_engine()
    eng.resize(W, H)
    return eng


def compare_and_check(eng, img, ref, p, what, t_img=None, t_ref=None):
    """metric_compare of two device images against the reference function; metric_last then returns the same result and the bins"""
    t_img = t_img if t_img is not None else device(img)
    t_ref = t_ref if t_ref is not None else device(ref)
    got = eng.metric_compare(t_ref.data_ptr(), image=t_img.data_ptr(), params=p)
    want, want_num, want_den = metric.reference_compare(img, ref, p)
    same_result(got, want, what)
    last, num, den = eng.metric_last(with_bins=True)
    same_result(last, want, what + ": metric_last")
    same_bins(num, want_num, what + ": num bins")
    same_bins(den, want_den, what + ": den bins")
    return got


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_shapes_whole_and_windowed(size):
    W, H = size
    img, ref = seeded_pair(W, H, seed=W * 1000 + H)
    t_img, t_ref = device(img), device(ref)
    eng = blank_engine(W, H)
    for name, win in windows(W, H).items():
        compare_and_check(eng, img, ref, params(win), f"{W}x{H} {name}", t_img, t_ref)
    eng.close()


def test_windows_of_one_pixel_one_row_and_one_off_the_tile():
    W, H = 100, 70
    img, ref = seeded_pair(W, H, seed=12)
    t_img, t_ref = device(img), device(ref)
    eng = blank_engine(W, H)
    for name, win in {"one pixel": (99, 69, 100, 70), "one row": (0, 33, 100, 34), "off the tile": (17, 5, 49, 37), "a strip": (31, 0, 33, 70)}.items():
        r = compare_and_check(eng, img, ref, params(win), name, t_img, t_ref)
        assert r["counted"] + r["nonfinite"] == (win[2] - win[0]) * (win[3] - win[1])
    eng.close()


def test_every_class_is_counted_where_the_contract_says():
    img, ref = class_rows()
    t_img, t_ref = device(img), device(ref)
    eng = blank_engine(img.shape[1], 1)
    for i, (name, (_, _, cls, differing)) in enumerate(CLASS_PIXELS.items()):
        r = compare_and_check(eng, img, ref, params((i, 0, i + 1, 1)), name, t_img, t_ref)
        assert r[cls] == 1 and r["differing"] == int(differing), (name, r)
    r = compare_and_check(eng, img, ref, None, "the whole row", t_img, t_ref)
    counted = sum(1 for p in CLASS_PIXELS.values() if p[2] == "counted")
    assert (r["counted"], r["nonfinite"], r["skipped"]) == (counted, len(CLASS_PIXELS) - counted, 0), r
    eng.close()


def test_identical_images_and_an_image_whose_only_differing_pixel_is_the_last():
    W, H = 131, 77
    img, ref = last_pixel_differs(W, H)
    eng = blank_engine(W, H)
    t_ref = device(ref)
    r = compare_and_check(eng, ref, ref, None, "identical", t_ref, t_ref)
    assert r["num"] == 0.0 and r["differing"] == 0 and r["value"] == 0.0 and r["max_abs"] == 0.0 and r["counted"] == W * H
    r = compare_and_check(eng, img, ref, None, "the last pixel differs", None, t_ref)
    assert r["differing"] == 1 and r["max_abs"] == 0.5 and r["num"] == 0.25
    eng.close()


def test_a_flat_pair_puts_every_term_into_one_bin():
    img, ref = constant_difference(300, 300)  # every lane of every wave adds to one LDS word per sum, every workgroup to one global word
    eng = blank_engine(300, 300)
    r = compare_and_check(eng, img, ref, None, "flat")
    _, num, den = eng.metric_last(with_bins=True)
    assert num[121] == 3 * 90000 * 2 ** 23 == num.sum() and den[125] == 3 * 90000 * 2 ** 23 == den.sum()
    assert r["num"] == 3 * 90000 / 64 and r["value"] == 0.25 and r["mse"] == 1 / 64
    eng.close()


def test_a_pair_with_all_255_bins_in_every_workgroup():
    img, ref = all_bins_pair(256, 20)  # any 85 consecutive pixels hold every bin: each of the five workgroups adds to all of them
    eng = blank_engine(256, 20)
    compare_and_check(eng, img, ref, None, "all bins")
    _, num, den = eng.metric_last(with_bins=True)
    assert (num[:255] > 0).all() and (den[:255] > 0).all() and num[255] == den[255] == 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 2
def test_full_size_pair_through_the_grid_stride_loop():
    W, H = 1920, 1080
    img, ref = seeded_pair(W, H, seed=2025)
    eng = blank_engine(W, H)
    r = compare_and_check(eng, img, ref, None, "1080p")
    assert r["counted"] + r["nonfinite"] == W * H and r["nonfinite"] > 0
    eng.close()


# ------------------------------------------------------------------------------------------------ 3
@pytest.fixture(scope="module")
def cornell():
    """the scene, its 64-pass frame (host copy and a kept device copy) and its 8-pass frame"""
    sc = scenes.cornell_box(64, 64, passes=64)
    eng = engine_with_passes(sc, range(64), mask=0)
    ref = eng.readback()
    eng.close()
    eng = engine_with_passes(sc, range(8), mask=0)
    frame8 = eng.readback()
    eng.close()
    return sc, ref, device(ref), frame8


def test_a_rendered_frame_against_a_kept_copy_of_its_64_pass_frame(cornell):
    sc, ref, t_ref, frame8 = cornell
    eng = engine_with_passes(sc, range(8), mask=0)
    got = eng.metric_compare(t_ref.data_ptr())  # right after render_pass, without a flush: it completes the passes
    want, want_num, want_den = metric.reference_compare(frame8, ref, passes=8)
    same_result(got, want, "8 passes against 64")
    _, num, den = eng.metric_last(with_bins=True)
    same_bins(num, want_num, "num bins")
    same_bins(den, want_den, "den bins")
    theirs = convergence.rel_l2(convergence.normalised(frame8), convergence.normalised(ref))
    print(f"value {got['value']!r}, convergence.rel_l2 {theirs!r}, relative difference {abs(got['value'] / theirs - 1):.3e}")
    assert abs(got["value"] / theirs - 1) <= 1e-6 and 0.0 < got["value"] < 1.0
    # flushed and synchronised first: the same
    eng.flush()
    eng.synchronize()
    same(eng.readback(), frame8, "the frame")
    stats = bytes(eng.stats())
    again = eng.metric_compare(t_ref.data_ptr())
    same_result(again, want, "after a flush")
    same_result(again, got, "two calls")
    # a pure post-process
    same(eng.readback(), frame8, "the frame after measuring")
    assert bytes(eng.stats()) == stats
    render_passes(eng, sc, range(8, 12))
    never = engine_with_passes(sc, range(12), mask=0)
    same(eng.readback(), never.readback(), "4 more passes after a measurement")
    never.close()
    # the frame against itself through its device pointer
    r = eng.metric_compare(eng.frame_device_ptr())
    assert r["num"] == 0.0 and r["value"] == 0.0 and r["differing"] == 0 and r["passes"] == 12
    eng.close()


# ------------------------------------------------------------------------------------------------ 4
def test_estimate_equals_its_reference_and_raises_the_documented_messages(cornell):
    sc = cornell[0]
    eng = engine_with_passes(sc, range(4), mask=ffi.HR_AOV_MOMENTS)
    got = eng.metric_estimate()
    frame, moments = eng.readback(), eng.aov_plane(ffi.HR_AOV_PLANE_MOMENTS)[0]
    want, want_num, want_den = metric.reference_estimate(frame, moments, passes=4)
    same_result(got, want, "estimate at 4 passes")
    last, num, den = eng.metric_last(with_bins=True)
    same_result(last, want, "metric_last")
    same_bins(num, want_num, "num bins")
    same_bins(den, want_den, "den bins")
    assert got["counted"] > 0 and got["kind"] == metric.ESTIMATE and 0.0 < got["value"] < 1.0, got
    win = params((5, 7, 50, 40))
    same_result(eng.metric_estimate(win), metric.reference_estimate(frame, moments, win, passes=4)[0], "a window")
    eng.clear()
    with pytest.raises(ffi.EngineError, match="metric: the frame is empty"):
        eng.metric_estimate()
    eng.close()
    # the plane off, and enabled late
    eng = engine_with_passes(sc, range(2), mask=0)
    with pytest.raises(ffi.EngineError, match="metric: the estimate needs the sample moments: hr_aov_enable\\(HR_AOV_MOMENTS\\) before the frame's first pass"):
        eng.metric_estimate()
    eng.set_aovs(ffi.HR_AOV_MOMENTS)
    render_passes(eng, sc, range(2, 3))
    with pytest.raises(ffi.EngineError, match="metric: the MOMENTS plane was enabled after the frame's first pass and does not hold"):
        eng.metric_estimate()
    eng.close()


# ------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("members", [2, 3])
def test_a_group_gives_the_plain_contexts_result_and_bins(members, cornell):
    sc, ref, t_ref, _ = cornell
    eng = engine_with_passes(sc, range(3), mask=ffi.HR_AOV_MOMENTS)
    want_c = eng.metric_compare(t_ref.data_ptr())
    _, want_cn, want_cd = eng.metric_last(with_bins=True)
    want_e = eng.metric_estimate()
    _, want_en, want_ed = eng.metric_last(with_bins=True)
    frame = eng.readback()
    eng.close()
    same_result(want_c, metric.reference_compare(frame, ref, passes=3)[0], "the plain context")
    grp = core.create_group([0] * members, tile_size=16)
    sc.apply(grp)
    grp.set_aovs(ffi.HR_AOV_MOMENTS)
    render_passes(grp, sc, range(3))
    same_result(grp.metric_compare(t_ref.data_ptr()), want_c, f"group of {members}: compare")
    last, num, den = grp.metric_last(with_bins=True)
    same_result(last, want_c, f"group of {members}: metric_last")
    same_bins(num, want_cn, "num bins")
    same_bins(den, want_cd, "den bins")
    same_result(grp.metric_estimate(), want_e, f"group of {members}: estimate")
    _, num, den = grp.metric_last(with_bins=True)
    same_bins(num, want_en, "estimate: num bins")
    same_bins(den, want_ed, "estimate: den bins")
    t = device(frame)  # a device image on the group's first device
    same_result(grp.metric_compare(t_ref.data_ptr(), image=t.data_ptr()), want_c, f"group of {members}: device image", skip=("passes",))
    grp.close()


# ------------------------------------------------------------------------------------------------ 5 (the shard) and 6
def test_refusals_leave_the_context_usable_and_metric_last_returns_the_last_result(cornell):
    sc, ref, t_ref, frame8 = cornell
    W, H = sc.width, sc.height
    eng = core.create_engine()
    with pytest.raises(ffi.EngineError, match="no frame"):
        eng.metric_compare(t_ref.data_ptr())
    sc.apply(eng)
    render_passes(eng, sc, range(8))
    with pytest.raises(ffi.EngineError, match="metric: nothing has been measured yet"):
        eng.metric_last()
    with pytest.raises(ffi.EngineError, match="metric: null reference"):
        eng.metric_compare(0)
    with pytest.raises(ffi.EngineError, match="metric: nothing has been measured yet"):
        eng.metric_last()
    good = eng.metric_compare(t_ref.data_ptr())
    same_result(good, metric.reference_compare(frame8, ref, passes=8)[0], "8 passes")
    p = params()
    p.reserved[2] = 1
    with pytest.raises(ffi.EngineError, match="metric: the reserved words"):
        eng.metric_compare(t_ref.data_ptr(), params=p)
    for win in ((0, 0, W + 1, H), (0, 0, W, H + 1), (-1, 0, W, H), (5, 5, 5, 9), (5, 9, 8, 9), (9, 5, 8, 9), (0, 0, 0, 1)):
        with pytest.raises(ffi.EngineError, match="metric: the window"):
            eng.metric_compare(t_ref.data_ptr(), params=params(win))
    with pytest.raises(ffi.EngineError, match="null output"):
        eng._feature_call("metric", "metric_compare", None, None, C.c_void_p(t_ref.data_ptr()), None)
    with pytest.raises(ffi.EngineError, match="null output"):
        eng._feature_call("metric", "metric_estimate", None, None)
    with pytest.raises(ffi.EngineError, match="null output"):
        eng._feature_call("metric", "metric_last", None, None, None)
    with pytest.raises(ffi.EngineError, match="metric: the estimate needs the sample moments"):
        eng.metric_estimate()
    last, num, den = eng.metric_last(with_bins=True)
    same_result(last, good, "the refusals left the last measurement alone")
    same_bins(num, metric.reference_compare(frame8, ref)[1], "its bins")
    # the state survives clear and resize
    eng.clear()
    same_result(eng.metric_last(), good, "after clear")
    eng.resize(20, 15)
    same_result(eng.metric_last(), good, "after resize")
    eng.close()
    # a tile shard outside a group
    eng = core.create_engine(rank=1, world=2, tile_size=16)
    with pytest.raises(ffi.EngineError, match="metric: a tile-sharded context"):
        eng.metric_compare(t_ref.data_ptr())
    sc.apply(eng)
    eng.set_aovs(ffi.HR_AOV_MOMENTS)
    render_passes(eng, sc, range(1))
    for call in (lambda: eng.metric_compare(t_ref.data_ptr()), lambda: eng.metric_compare(t_ref.data_ptr(), image=t_ref.data_ptr()), eng.metric_estimate):
        with pytest.raises(ffi.EngineError, match="metric: a tile-sharded context \\(world > 1\\).*the sum reads across them: use a context group"):
            call()
    with pytest.raises(ffi.EngineError, match="nothing has been measured"):
        eng.metric_last()
    assert eng.readback().any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 7
def test_run_on_device_gives_run_with_readbacks_pass_count():
    sc = scenes.cornell_box(32, 32, bounces=3, passes=96)
    eng = core.create_engine()
    sc.apply(eng)
    eng.set_seq_offsets(convergence.offsets_table(eng, 0, sc.width, sc.height))
    eng.clear()
    render_passes(eng, sc, range(96))
    ref_frame = eng.readback()
    t_ref = device(ref_frame)  # the kept copy of the reference run's frame
    ref_img = convergence.normalised(ref_frame)
    for run in range(2):
        n_host, e_host = convergence.run_with_readback(eng, sc.options, run, 96, ref_img, sc.width, sc.height, threshold=0.15)
        n_dev, e_dev = convergence.run_on_device(eng, sc.options, run, 96, t_ref.data_ptr(), sc.width, sc.height, threshold=0.15)
        assert n_dev == n_host and n_host is not None and n_host > 1 and len(e_dev) == len(e_host), (run, n_dev, n_host)
        worst = max(abs(d / h - 1) for d, h in zip(e_dev, e_host))
        print(f"run {run}: {n_dev} passes, errors within {worst:.3e} relative")
        assert worst <= 1e-6
    eng.close()
