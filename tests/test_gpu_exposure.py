"""Auto-exposure (include/hrcore_exposure.h) on the GPU.  Every comparison with the reference is exact: the result's floats to the bit,
the counts and all 256 bins equal, the displayed images byte for byte.

 1. rendered frames (three scenes, 1 and 4 passes, interactive mode's one-ninth frame) against exposure.reference(eng.readback())
 2. synthetic shapes where a kernel can go wrong: tiny and odd sizes, windows, every class, a flat image, all bins in every workgroup
 3. one 1920 x 1080 image: the grid-stride loop under the capped grid
 4. the metered display = hr_display of the pre-multiplied image, three formats, two settings; the denoiser's output as the image
 5. scaling the frame by a power of two shows the same bytes
 6. the adaptation state: it follows the reference, survives clear and resize, exposure_reset drops it; exposure_last
 7. a pure post-process: frame, planes and later passes untouched
 8. HR_DISPLAY_PROGRESSIVE after flush + synchronize is the complete display
 9. every refusal, the context usable after each; no AOVs and late AOVs are no obstacle
10. context groups of 2 and 3 members give the plain context's result, bins and image."""
import ctypes as C

import numpy as np
import pytest

from device_support import BOTH, engine_with_passes, render_passes, same
from exposure_frames import CLASS_PIXELS, F, all_bins, class_row, flat, params, same_result, seeded, windows
from heatray_amd import _ffi as ffi
from heatray_amd import core, exposure, scenes

pytestmark = pytest.mark.gpu

FORMATS = ((ffi.HR_DISPLAY_RGBA8, np.uint8), (ffi.HR_DISPLAY_RGBA32F, np.float32), (ffi.HR_DISPLAY_HDR_RGBA32F, np.float32))
DISPLAYS = {"defaults": lambda: ffi.display_params(), "aces_vignette": lambda: ffi.display_params(tonemapping_enabled=True, exposure=1.0, vignette_intensity=0.5, vignette_falloff=0.6)}
WIDE = dict(min_scale=2.0 ** -40, max_scale=2.0 ** 40)


def device(image):
    import torch
    return torch.from_numpy(np.ascontiguousarray(image, F)).to("cuda:0")


def blank_engine(W, H):
    eng = core.create_engine()
    eng.resize(W, H)
    return eng


def meter_and_check(eng, image, p, what, state=None, tensor=None):
    """exposure_meter of `image` (passed as a device image; None: the engine's frame, compared with its read-back) against the reference;
    exposure_last then returns the same result and the reference's bins.  state: the adaptation state the engine is in (None: it is
    reset first).  Returns (the result, the reference's state after)."""
    if state is None:
        eng.exposure_reset()
    t = tensor if tensor is not None else (device(image) if image is not None else None)
    got = eng.exposure_meter(p, image=t.data_ptr() if t is not None else None)
    want, want_bins, new_state = exposure.reference(image if image is not None else eng.readback(), p, state)
    same_result(got, want, what)
    last, bins = eng.exposure_last(with_bins=True)
    same_result(last, want, what + ": exposure_last")
    assert bins.dtype == np.uint64 and bins.tobytes() == want_bins.tobytes(), (what, np.nonzero(bins != want_bins)[0][:8], bins.sum(), want_bins.sum())
    return got, new_state


def shown(eng, fmt, dtype, display, p=None, image=None, progressive=False):
    """exposure_display into a torch tensor -> (numpy image, passes shown)"""
    import torch
    out = torch.zeros((eng.height, eng.width, 4), dtype=torch.uint8 if dtype is np.uint8 else torch.float32, device="cuda:0")
    n = eng.exposure_display(out.data_ptr(), display, fmt | (ffi.HR_DISPLAY_PROGRESSIVE if progressive else 0), p, image=image)
    eng.synchronize()
    torch.cuda.synchronize()
    return out.cpu().numpy(), n


def display_of(image, fmt, display):
    """hr_display of an engine whose bound frame is `image`"""
    H, W = image.shape[:2]
    t = device(image)
    eng = blank_engine(W, H)
    eng.bind_external_frame(t.data_ptr())
    out = eng.display(display, fmt)
    eng.close()
    return out


# ------------------------------------------------------------------------------------------------ 1
RENDERED = {
    "cornell": lambda: scenes.cornell_box(128, 128),
    "multi_material": lambda: scenes.multi_material(160, 90, textured=True),
    "soup_env": lambda: scenes.triangle_soup(3000, 96, 64, env=True),
}


@pytest.mark.parametrize("name", sorted(RENDERED))
def test_rendered_frames_equal_the_reference(name):
    sc = RENDERED[name]()
    eng = engine_with_passes(sc, range(1), mask=0)
    r1, _ = meter_and_check(eng, None, None, f"{name}: 1 pass")
    assert r1["counted"] > 0 and r1["invalid"] == 0, r1
    render_passes(eng, sc, range(1, 4))
    meter_and_check(eng, None, None, f"{name}: 4 passes")
    meter_and_check(eng, None, params((3, 5, sc.width - 7, sc.height - 2), low_permille=0, high_permille=500), f"{name}: a window")
    # interactive mode's first sub-pass: one pixel of every 3 x 3 block has a sample, the others are holes
    eng.clear()
    sc.options.enable_interactive_mode = True
    eng.render_pass(sc.options.pass_params(0, current_block_pixel=(0, 0)))
    r, _ = meter_and_check(eng, None, None, f"{name}: one ninth")
    holes = int((~(eng.readback()[..., 3] > 0)).sum())
    assert r["invalid"] == holes and 0.85 * sc.width * sc.height < holes < sc.width * sc.height, (r, holes)
    eng.close()


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("size", [(1, 1), (67, 35), (257, 3), (3, 257), (256, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_and_odd_shapes_whole_and_windowed(size):
    W, H = size
    image = seeded(W, H, seed=W * 1000 + H)
    t = device(image)
    eng = blank_engine(W, H)
    for name, win in windows(W, H).items():
        meter_and_check(eng, image, params(win), f"{W}x{H} {name}", tensor=t)
    eng.close()


def test_every_class_is_counted_where_the_contract_says():
    row = class_row()
    eng = blank_engine(row.shape[1], 1)
    t = device(row)
    for i, (name, (_, cls)) in enumerate(CLASS_PIXELS.items()):
        r, _ = meter_and_check(eng, row, params((i, 0, i + 1, 1)), name, tensor=t)
        assert (r["counted"] == 1) if isinstance(cls, int) else (r[cls] == 1 and r["flags"] == exposure.EMPTY), (name, r)
    r, _ = meter_and_check(eng, row, None, "the whole row", tensor=t)
    assert (r["counted"], r["below"], r["above"], r["nonfinite"], r["invalid"]) == (3, 5, 2, 3, 3), r
    eng.close()


def test_a_flat_image_puts_every_pixel_into_one_bin():
    image = flat(300, 300)  # every lane of every wave adds to one LDS word, every workgroup to one global word
    eng = blank_engine(300, 300)
    r, _ = meter_and_check(eng, image, None, "flat")
    _, bins = eng.exposure_last(with_bins=True)
    assert bins.max() == 90000 == bins.sum() == r["counted"] and r["used"] == 85500 - 9000, (bins.max(), r)
    eng.close()


def test_an_image_with_all_256_bins_in_every_workgroup():
    image = all_bins(512, 300)  # any 256 consecutive pixels hold the 256 bins once: every workgroup adds to every bin
    eng = blank_engine(512, 300)
    meter_and_check(eng, image, params(low_permille=0, high_permille=1000), "all bins")
    _, bins = eng.exposure_last(with_bins=True)
    assert (bins == 600).all()
    eng.close()


# ------------------------------------------------------------------------------------------------ 3
def test_full_size_image_through_the_grid_stride_loop():
    W, H = 1920, 1080
    image = seeded(W, H, seed=2025)
    eng = blank_engine(W, H)
    r, _ = meter_and_check(eng, image, None, "1080p")
    assert r["counted"] + r["below"] + r["above"] + r["nonfinite"] + r["invalid"] == W * H
    meter_and_check(eng, image, params((1, 1, W - 1, H - 1)), "1080p without its border")
    eng.close()


# ------------------------------------------------------------------------------------------------ 4 and 5
@pytest.fixture(scope="module")
def display_case():
    """a seeded frame with holes, its metering and the pre-multiplied image hr_display is given"""
    image = seeded(131, 77, seed=4, classes=False)
    image[np.random.default_rng(9).random((77, 131)) < 0.1] = 0  # holes: black, alpha as hr_display writes it
    p = params(**WIDE)
    res, _, _ = exposure.reference(image, p)
    assert res["flags"] == 0 and res["scale"] != 1.0
    return image, p, res, exposure.apply(image, res["scale"])


@pytest.mark.parametrize("setting", sorted(DISPLAYS))
@pytest.mark.parametrize("fmt, dtype", FORMATS, ids=["rgba8", "rgba32f", "hdr"])
def test_metered_display_is_display_of_the_premultiplied_image(display_case, fmt, dtype, setting):
    image, p, res, pre = display_case
    display = DISPLAYS[setting]()
    want = display_of(pre, fmt, display)
    H, W = image.shape[:2]
    t = device(image)
    eng = blank_engine(W, H)
    eng.bind_external_frame(t.data_ptr())
    got, _ = shown(eng, fmt, dtype, display, p)  # the frame
    same(got, want, f"frame, format {fmt}, {setting}")
    same_result(eng.exposure_last(), res, "the display's metering")
    eng.close()
    eng = blank_engine(W, H)
    got, n = shown(eng, fmt, dtype, display, p, image=t.data_ptr())  # a device image
    same(got, want, f"device image, format {fmt}, {setting}")
    assert n == 0
    if fmt == ffi.HR_DISPLAY_RGBA8:
        assert 0.05 < (got[..., :3] > 0).mean() and (got[..., :3] < 255).mean() > 0.05  # (an image, not a constant)
        for k in (-4, 3):  # 5: the frame times 2^k shows the same bytes
            scaled = image.copy()
            scaled[..., :3] *= F(2.0 ** k)
            ts = device(scaled)  # (held until the display has run: a freed tensor's memory is the next allocation's)
            got_k, _ = shown(eng, fmt, dtype, display, p, image=ts.data_ptr())
            same(got_k, want, f"frame x 2^{k}, {setting}")
            rk = eng.exposure_last()
            assert rk["position"] == res["position"] + 4096 * k and rk["flags"] == 0
    eng.close()


def test_metered_display_of_the_denoisers_output():
    import torch
    sc = scenes.multi_material(96, 64, bounces=3, textured=True)
    eng = engine_with_passes(sc, range(2))
    dn = torch.zeros((64, 96, 4), dtype=torch.float32, device="cuda:0")
    eng.denoise_to_device(dn.data_ptr())
    display = DISPLAYS["aces_vignette"]()
    got, _ = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, display, image=dn.data_ptr())  # (no synchronisation between the filter and the meter)
    image = dn.cpu().numpy()
    same(image, eng.denoise(), "denoise_to_device")
    res, bins, _ = exposure.reference(image)
    last, got_bins = eng.exposure_last(with_bins=True)
    same_result(last, res, "metering the denoised image")
    assert got_bins.tobytes() == bins.tobytes()
    same(got, display_of(exposure.apply(image, res["scale"]), ffi.HR_DISPLAY_RGBA8, display), "display of the denoised image")
    eng.close()


# ------------------------------------------------------------------------------------------------ 6
def test_the_adaptation_state_follows_the_reference_and_survives_clear_and_resize():
    bright, dark = flat(40, 30, (4.0, 4.0, 4.0)), flat(40, 30, (0.01, 0.01, 0.01))
    tb, td = device(bright), device(dark)
    eng = blank_engine(40, 30)
    with pytest.raises(ffi.EngineError, match="nothing has been metered"):
        eng.exposure_last()
    p = params(adapt=0.25)
    state, scales = None, []
    for i in range(5):
        image, t = (bright, tb) if i % 2 == 0 else (dark, td)
        r, state = meter_and_check(eng, image, p, f"metering {i}", state=state, tensor=t)
        assert r["flags"] == (exposure.ADAPTED if i else 0)
        scales.append(r["scale"])
    assert len(set(scales)) == 5
    eng.clear()
    _, state = meter_and_check(eng, bright, p, "after clear", state=state, tensor=tb)
    eng.resize(20, 15)
    small = flat(20, 15, (0.01, 0.01, 0.01))
    r, state = meter_and_check(eng, small, p, "after resize", state=state)
    assert r["flags"] == exposure.ADAPTED
    # an empty metering shows the state's scale and leaves it
    r, state = meter_and_check(eng, np.zeros((15, 20, 4), F), p, "holes only", state=state)
    assert r["flags"] == exposure.EMPTY and r["scale"] == float(state)
    # exposure_last after an asynchronous display: that display's metering
    ts = device(small)
    got, _ = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, ffi.display_params(), p, image=ts.data_ptr())
    want, want_bins, state = exposure.reference(small, p, state)
    last, bins = eng.exposure_last(with_bins=True)
    same_result(last, want, "exposure_last after exposure_display")
    assert bins.tobytes() == want_bins.tobytes() and want["flags"] == exposure.ADAPTED
    same(got, display_of(exposure.apply(small, want["scale"]), ffi.HR_DISPLAY_RGBA8, ffi.display_params()), "the display used the adapted scale")
    eng.exposure_reset()
    r, _ = meter_and_check(eng, small, p, "after exposure_reset", state=None)
    assert r["flags"] == 0 and r["scale"] == r["target"]
    same_result(eng.exposure_last(), r, "exposure_reset keeps the last metering")
    eng.close()


# ------------------------------------------------------------------------------------------------ 7 and 8
def test_it_changes_neither_the_frame_nor_the_planes_nor_later_passes_and_progressive_is_complete_after_a_flush():
    mk = lambda: scenes.multi_material(96, 64, bounces=3, textured=True)
    sc = mk()
    eng = engine_with_passes(sc, range(2))
    frame, planes = eng.readback(), eng.aovs()
    eng.exposure_meter()
    eng.exposure_meter(params(adapt=0.5))
    display = ffi.display_params()
    full, n_full = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, display)
    same(eng.readback(), frame, "frame after metering")
    after = eng.aovs()
    for name in ("albedo", "normal_depth", "moments"):
        same(after[name], planes[name], f"{name} after metering")
    render_passes(eng, sc, range(2, 10))
    never = engine_with_passes(mk(), range(10))
    same(eng.readback(), never.readback(), "8 more passes after a metering")
    never.close()
    # progressive: nothing pending after flush + synchronize, so it is the complete display
    eng.exposure_reset()
    eng.flush()
    eng.synchronize()
    prog, n_prog = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, display, progressive=True)
    eng.exposure_reset()
    full, n_full = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, display)
    same(prog, full, "progressive against complete")
    assert n_prog == n_full == 10
    res, _, _ = exposure.reference(eng.readback())
    same(full, display_of(exposure.apply(eng.readback(), res["scale"]), ffi.HR_DISPLAY_RGBA8, display), "the rendered frame, metered and shown")
    eng.close()


# ------------------------------------------------------------------------------------------------ 9
def test_every_refusal_leaves_the_context_usable():
    import torch
    sc = scenes.multi_material(70, 45, bounces=3, textured=True)
    W, H = sc.width, sc.height
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    eng = core.create_engine()
    with pytest.raises(ffi.EngineError, match="no frame"):
        eng.exposure_meter()
    with pytest.raises(ffi.EngineError, match="no frame"):
        eng.exposure_display(out.data_ptr())
    sc.apply(eng)
    render_passes(eng, sc, range(1))
    good = eng.exposure_meter()  # (no AOV enabled: the aov == 0 path of frameReady)
    bad_params = [("key", 0.0), ("key", -1.0), ("key", float("nan")), ("key", float("inf")), ("low_permille", -1), ("high_permille", 1001), ("low_permille", 950),
                  ("min_scale", 0.0), ("min_scale", float("nan")), ("max_scale", float("inf")), ("max_scale", 1.0 / 512.0), ("adapt", -0.1), ("adapt", 1.5),
                  ("adapt", float("nan"))]
    for field, value in bad_params:
        with pytest.raises(ffi.EngineError, match="exposure: .*" + field.split("_")[-1]):
            eng.exposure_meter(params(**{field: value}))
    p = params()
    p.reserved[3] = 1
    with pytest.raises(ffi.EngineError, match="reserved"):
        eng.exposure_meter(p)
    for win in ((0, 0, W + 1, H), (0, 0, W, H + 1), (-1, 0, W, H), (5, 5, 5, 9), (5, 9, 8, 9), (9, 5, 8, 9), (0, 0, 0, 1)):
        with pytest.raises(ffi.EngineError, match="exposure: the window"):
            eng.exposure_meter(params(win))
    with pytest.raises(ffi.EngineError, match="unknown display format"):
        eng.exposure_display(out.data_ptr(), fmt=3)
    with pytest.raises(ffi.EngineError, match="unknown display format"):
        eng.exposure_display(out.data_ptr(), fmt=7 | ffi.HR_DISPLAY_PROGRESSIVE)
    with pytest.raises(ffi.EngineError, match="null argument"):
        eng.exposure_display(0)
    with pytest.raises(ffi.EngineError, match="null argument"):
        eng._feature_call("exposure", "exposure_display", None, None, C.c_int32(0), None, C.c_void_p(out.data_ptr()), None)
    with pytest.raises(ffi.EngineError, match="null output"):
        eng._feature_call("exposure", "exposure_meter", None, None, None)
    with pytest.raises(ffi.EngineError, match="null output"):
        eng._feature_call("exposure", "exposure_last", None, None)
    same_result(eng.exposure_last(), good, "the refusals left the last metering alone")
    same_result(eng.exposure_meter(), good, "... and the context usable")
    # AOVs enabled after the frame's first pass: the planes do not hold the frame's passes, the meter reads none of them
    eng.set_aovs(BOTH)
    render_passes(eng, sc, range(1, 2))
    with pytest.raises(ffi.EngineError, match="hr_clear.*hr_aov_enable|hr_aov_enable.*hr_clear"):
        eng.denoise()
    meter_and_check(eng, None, None, "AOVs enabled late")
    eng.close()
    # a tile shard outside a group
    eng = core.create_engine(rank=1, world=2, tile_size=16)
    with pytest.raises(ffi.EngineError, match="exposure: a tile-sharded context"):
        eng.exposure_meter()
    sc.apply(eng)
    render_passes(eng, sc, range(1))
    for call in (eng.exposure_meter, lambda: eng.exposure_display(out.data_ptr()), lambda: eng.exposure_meter(image=out.data_ptr()),
                 lambda: eng.exposure_display(out.data_ptr(), fmt=ffi.HR_DISPLAY_PROGRESSIVE)):
        with pytest.raises(ffi.EngineError, match="exposure: a tile-sharded context \\(world > 1\\).*the meter reads across them: use a context group"):
            call()
    with pytest.raises(ffi.EngineError, match="nothing has been metered"):
        eng.exposure_last()
    assert eng.readback().any()
    eng.close()


# ------------------------------------------------------------------------------------------------ 10
@pytest.mark.parametrize("members", [2, 3])
def test_a_group_gives_the_plain_contexts_result_bins_and_image(members):
    mk = lambda: scenes.multi_material(100, 70, bounces=3, textured=True)
    display = DISPLAYS["aces_vignette"]()
    eng = engine_with_passes(mk(), range(2), mask=0)
    want = eng.exposure_meter()
    _, want_bins = eng.exposure_last(with_bins=True)
    want_img, want_n = shown(eng, ffi.HR_DISPLAY_RGBA8, np.uint8, display)
    frame = eng.readback()
    eng.close()
    same_result(want, exposure.reference(frame)[0], "the plain context")
    grp = core.create_group([0] * members, tile_size=16)
    sc = mk()
    sc.apply(grp)
    render_passes(grp, sc, range(2))
    same_result(grp.exposure_meter(), want, f"group of {members}")
    last, bins = grp.exposure_last(with_bins=True)
    same_result(last, want, f"group of {members}: exposure_last")
    assert bins.tobytes() == want_bins.tobytes()
    got, n = shown(grp, ffi.HR_DISPLAY_RGBA8, np.uint8, display)
    same(got, want_img, f"group of {members}: displayed image")
    assert n == want_n == 2
    prog, n = shown(grp, ffi.HR_DISPLAY_RGBA8, np.uint8, display, progressive=True)
    same(prog, want_img, f"group of {members}: progressive with nothing pending")
    assert n == 2
    # a device image on the group's first device
    t = device(frame)
    same_result(grp.exposure_meter(image=t.data_ptr()), want, f"group of {members}: device image")
    grp.close()
