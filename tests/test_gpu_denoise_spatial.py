"""The denoiser with the spatial variance estimate (include/hrcore_denoise_spatial.h) on the GPU: image, variance plane and counters are
heatray_amd.denoise_spatial's of the read-back frame and planes, bit for bit (tests/test_denoise_spatial_ref.py ties that reference to
the per-pixel header the kernel compiles); the early-out path; mixed sample counts; interactive mode; the entry points' ordering, life
cycle and errors; a context group gives the plain context's image; and what the estimate buys against the renderer itself.

Which case reaches which path of k_spatial_variance: after one pass every workgroup stages its tile (67 x 41: partial tiles on two
edges; 48 x 32: exact tiles); after `below` passes every workgroup takes the early out; the mixed-count frame has both kinds and
workgroups with spatial and plain pixels side by side."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
from device_support import BOTH, denoise_params, engine_with_passes, orbit, render_passes, same, truth
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise, denoise_spatial, history, scenes

pytestmark = pytest.mark.gpu
AUTO, PLAIN, TILED = ffi.HR_DENOISE_KERNEL_AUTO, ffi.HR_DENOISE_KERNEL_PLAIN, ffi.HR_DENOISE_KERNEL_TILED
NONE = {"spatial_pixels": 0, "estimated_pixels": 0, "starved_pixels": 0}


def _spatial(below=4, min_taps=6):
    s = denoise_spatial.default_params()
    s.below, s.min_taps = below, min_taps
    return s


def _check(eng, what, iterations=(0, 5), spatial=None):
    """device == reference for the frame the engine holds: variance plane, counters, and the image with both a-trous kernels"""
    frame, planes = eng.readback(), eng.aovs()
    want_v, want_r = denoise_spatial.variance(frame, planes, None, spatial, with_result=True)
    got_v, got_r = eng.denoise_spatial_variance(None, spatial, with_result=True)
    assert got_r == want_r, (what, got_r, want_r)
    same(got_v[..., None], want_v[..., None], f"{what}: variance plane")
    for it in iterations:
        want = denoise_spatial.reference(frame, planes, denoise_params(it), spatial)
        assert np.isfinite(want).all()
        for kernel in (PLAIN, TILED):
            got, r = eng.denoise_spatial(denoise_params(it, kernel), spatial, with_result=True)
            assert r == want_r, (what, it, kernel, r, want_r)
            same(got, want, f"{what}: {it} iterations, kernel {kernel}")
    return frame, planes, want_r


SCENES = {
    "odd_size_1": (lambda: scenes.multi_material(67, 41, bounces=3, textured=True), 1),
    "odd_size_2": (lambda: scenes.multi_material(67, 41, bounces=3, textured=True), 2),
    "exact_tiles": (lambda: scenes.multi_material(48, 32, bounces=3, textured=True), 1),
    "cornell": (lambda: scenes.cornell_box(128, 128, bounces=4), 1),
    "glass_passthrough_soup": (lambda: scenes.triangle_soup(3000, width=96, height=64, bounces=4, env=True, glass_fraction=0.25, passthrough_fraction=0.25), 1),
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_reference(name):
    mk, n = SCENES[name]
    eng = engine_with_passes(mk(), range(n))
    frame, _, res = _check(eng, name)
    assert res["spatial_pixels"] == frame.shape[0] * frame.shape[1] and res["estimated_pixels"] > 0
    same(eng.denoise_spatial(), denoise_spatial.reference(frame, eng.aovs()), f"{name}, NULL params")
    eng.close()


def test_no_spatial_pixel_is_the_plain_denoiser():
    eng = engine_with_passes(SCENES["odd_size_1"][0](), range(4))
    want = eng.denoise()
    got, res = eng.denoise_spatial(with_result=True)
    assert res == NONE
    same(got, want, "4 passes, defaults: the early-out path")
    for it in (0, 1, 2):
        same(eng.denoise_spatial(denoise_params(it)), eng.denoise(denoise_params(it)), f"early out, {it} iterations")
    frame, planes = eng.readback(), eng.aovs()
    same(eng.denoise_spatial_variance()[..., None], denoise.prepare(frame, planes["albedo"], planes["normal_depth"], planes["moments"])[0][..., 3:4], "prepared variance")
    eng.close()


def test_mixed_sample_counts():
    sc = scenes.multi_material(96, 64, bounces=3, textured=True)
    eng = engine_with_passes(sc, range(1))
    mask = np.ones((64, 96), np.uint8)
    mask[13:43, 21:61] = 0  # (30 x 40: no multiple of the tile, no tile boundary on its edges)
    eng.set_sample_mask(mask)
    render_passes(eng, sc, range(1, 16))
    frame, _, res = _check(eng, "mixed counts", iterations=(5,))
    n = frame[..., 3]
    assert (n[mask == 0] == 1).all() and (n[mask == 1] == 16).all()
    assert res["spatial_pixels"] == 30 * 40
    eng.close()


def test_interactive_mode():
    sc = scenes.multi_material(66, 39, bounces=3)
    sc.options.enable_interactive_mode = True
    eng = core.create_engine()
    sc.apply(eng)
    eng.set_aovs(BOTH)
    blocks = [(bx, by) for by in range(3) for bx in range(3)]
    for k, (bx, by) in enumerate(blocks[:4]):  # 4 of 9 blocks: the other pixels have no sample
        eng.render_pass(sc.options.pass_params(k, current_block_pixel=(bx, by)))
    frame, _, res = _check(eng, "interactive", iterations=(5,))
    holes = frame[..., 3] == 0
    assert 0.3 < holes.mean() < 0.8
    assert res["spatial_pixels"] == int((~holes).sum())
    got = eng.denoise_spatial()
    assert (got[holes] == 0).all() and (got[~holes][:, 3] == 1).all()
    eng.close()


def test_non_default_parameters():
    eng = engine_with_passes(SCENES["cornell"][0](), range(2))
    frame, planes = eng.readback(), eng.aovs()
    outs = []
    for p, s in ((denoise_params(sigma_z=0.0, normal_power=0), _spatial(2, 2)), (denoise_params(3, sigma_l=1.5, sigma_z=0.5, normal_power=16), _spatial(64, 49)),
                 (denoise_params(), _spatial(3, 20))):
        want, wr = denoise_spatial.reference(frame, planes, p, s, with_result=True)
        got, r = eng.denoise_spatial(p, s, with_result=True)
        assert r == wr
        same(got, want, f"below {s.below}, min_taps {s.min_taps}")
        outs.append((want, wr))
    assert outs[0][1] == NONE  # (two passes, below = 2)
    assert outs[1][1]["spatial_pixels"] == 128 * 128
    eng.close()


def test_device_output_on_a_foreign_stream_and_display():
    import torch
    eng = engine_with_passes(SCENES["odd_size_1"][0](), range(1))
    want = eng.denoise_spatial()
    H, W = want.shape[:2]
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    eng.denoise_spatial_to_device(t.data_ptr())  # the ctx stream
    eng.synchronize()
    torch.cuda.synchronize()
    same(t.cpu().numpy(), want, "hr_denoise_spatial on the ctx stream")
    s = torch.cuda.Stream()
    t2 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    eng.denoise_spatial_to_device(t2.data_ptr(), denoise_params(kernel=PLAIN), stream=s.cuda_stream)
    s.synchronize()
    same(t2.cpu().numpy(), want, "hr_denoise_spatial on a foreign stream")
    # the display resolve of the image = the oracle's display resolve of the read-back image
    ora = oracle_lib.engine()
    ora.resize(W, H)
    p = ffi.f32p()
    ww, hh = C.c_int32(), C.c_int32()
    ora._call("readback", C.byref(p), C.byref(ww), C.byref(hh))  # the oracle hands out its own buffer: write into it
    np.ctypeslib.as_array(p, shape=(H, W, 4))[...] = want
    dp = ffi.display_params(tonemapping_enabled=True, exposure=0.7, brightness=0.1, contrast=1.2, hue=0.9, saturation=1.3, vibrance=0.2,
                            red=1.1, green=0.9, blue=1.05, vignette_intensity=0.5, vignette_falloff=0.6)
    for fmt, dt in ((ffi.HR_DISPLAY_RGBA8, torch.uint8), (ffi.HR_DISPLAY_RGBA32F, torch.float32), (ffi.HR_DISPLAY_HDR_RGBA32F, torch.float32)):
        out = torch.zeros((H, W, 4), dtype=dt, device="cuda:0")
        eng.denoise_spatial_display(out.data_ptr(), dp, fmt)
        eng.synchronize()
        torch.cuda.synchronize()
        ref = ora.display(dp, fmt)
        got = out.cpu().numpy()
        assert got.dtype == ref.dtype
        same(got.view(np.uint8).reshape(H, W, -1), ref.view(np.uint8).reshape(H, W, -1), f"display format {fmt}")
    with pytest.raises(ffi.EngineError, match="display format"):
        eng.denoise_spatial_display(t.data_ptr(), dp, ffi.HR_DISPLAY_RGBA8 | ffi.HR_DISPLAY_PROGRESSIVE)
    ora.close()
    eng.close()


def test_it_changes_neither_the_frame_nor_the_planes_nor_later_passes():
    mk = SCENES["odd_size_1"][0]
    sc = mk()
    eng = engine_with_passes(sc, range(1))
    frame, planes = eng.readback(), eng.aovs()
    eng.denoise_spatial()
    eng.denoise_spatial_variance()
    eng.denoise_spatial(denoise_params(kernel=PLAIN))
    same(eng.readback(), frame, "frame after denoise_spatial")
    after = eng.aovs()
    for name in ("albedo", "normal_depth", "moments"):
        same(after[name], planes[name], f"{name} after denoise_spatial")
    same(eng.denoise(), denoise.reference(frame, planes), "hr_denoise after hr_denoise_spatial")
    render_passes(eng, sc, range(1, 5))
    plain = engine_with_passes(mk(), range(5), mask=0)
    same(eng.readback(), plain.readback(), "4 more passes after a denoise_spatial")
    plain.close()
    eng.close()


def test_group_of_three_gives_the_plain_contexts_image():
    mk = lambda: scenes.multi_material(100, 70, bounces=3, textured=True)
    eng = engine_with_passes(mk(), range(1))
    want, wr = eng.denoise_spatial(with_result=True)
    wv = eng.denoise_spatial_variance()
    eng.close()
    grp = core.create_group([0, 0, 0], tile_size=16)
    sc = mk()
    sc.apply(grp)
    grp.set_aovs(BOTH)
    render_passes(grp, sc, range(1))
    got, r = grp.denoise_spatial(with_result=True)
    assert r == wr and r["spatial_pixels"] == 100 * 70
    same(got, want, "group of three")
    same(grp.denoise_spatial_variance()[..., None], wv[..., None], "group of three: variance plane")
    import torch
    t = torch.zeros((70, 100, 4), dtype=torch.float32, device="cuda:0")
    grp.denoise_spatial_to_device(t.data_ptr())
    grp.synchronize()
    torch.cuda.synchronize()
    same(t.cpu().numpy(), want, "group: device output")
    grp.close()


def test_errors_and_life_cycle():
    mk = SCENES["odd_size_1"][0]
    sc = mk()
    eng = core.create_engine(rank=1, world=3, tile_size=16)
    sc.apply(eng)
    eng.set_aovs(BOTH)
    render_passes(eng, sc, range(1))
    for call in (eng.denoise_spatial, eng.denoise_spatial_variance):
        with pytest.raises(ffi.EngineError, match="tile-sharded.*world > 1"):
            call()
    eng.close()
    eng = core.create_engine()
    sc.apply(eng)
    render_passes(eng, sc, range(1))
    with pytest.raises(ffi.EngineError, match="hr_aov_enable"):      # AOVs off
        eng.denoise_spatial()
    for mask in (ffi.HR_AOV_SURFACE, ffi.HR_AOV_MOMENTS):            # only one mask on
        eng.clear()
        eng.set_aovs(mask)
        render_passes(eng, sc, range(1))
        with pytest.raises(ffi.EngineError, match="hr_aov_enable"):
            eng.denoise_spatial()
    eng.set_aovs(0)
    eng.clear()
    render_passes(eng, sc, range(1))
    eng.set_aovs(BOTH)                                               # enabled after the first pass
    render_passes(eng, sc, range(1, 2))
    with pytest.raises(ffi.EngineError, match="hr_clear.*hr_aov_enable|hr_aov_enable.*hr_clear"):
        eng.denoise_spatial()
    eng.clear()                                                      # ... and after hr_clear it works
    render_passes(eng, sc, range(1))
    same(eng.denoise_spatial(), denoise_spatial.reference(eng.readback(), eng.aovs()), "after clear")
    for kw, text in ((dict(below=1), "below"), (dict(below=65), "below"), (dict(min_taps=1), "min_taps"), (dict(min_taps=50), "min_taps")):
        for call in (eng.denoise_spatial, eng.denoise_spatial_variance):
            with pytest.raises(ffi.EngineError, match=text):
                call(None, _spatial(**kw))
    s = _spatial()
    s.reserved[5] = 1
    with pytest.raises(ffi.EngineError, match="reserved"):
        eng.denoise_spatial(None, s)
    for kw, text in ((dict(iterations=9), "iterations"), (dict(sigma_l=float("nan")), "sigma_l"), (dict(sigma_z=-0.5), "sigma_z"), (dict(normal_power=17), "normal_power"),
                     (dict(kernel=3), "kernel")):                    # what hr_denoise refuses
        with pytest.raises(ffi.EngineError, match=text):
            eng.denoise_spatial(denoise_params(**kw))
    eng.resize(50, 30)                                               # a resize frees the working planes and the counters: the next call has its own
    render_passes(eng, sc, range(1))
    got, r = eng.denoise_spatial(with_result=True)
    assert got.shape == (30, 50, 4) and r["spatial_pixels"] == 50 * 30
    same(got, denoise_spatial.reference(eng.readback(), eng.aovs()), "after resize")
    eng.close()


BUYS = {
    # name: (scene, is N = 1 asserted)
    # (passes=2048: the scene's sample tables must be as long as the passes rendered, or the ground truth repeats the passes under test)
    "cornell": (lambda: scenes.cornell_box(128, 128, bounces=4, passes=2048), True),
    "multi_material": (lambda: scenes.multi_material(160, 90, bounces=4, passes=2048, textured=True), True),
    "soup_env_glass": (lambda: scenes.triangle_soup(2000, width=128, height=96, bounces=4, passes=2048, env=True, glass_fraction=0.25), False),
}


@pytest.mark.parametrize("name", sorted(BUYS))
def test_what_it_buys(name):
    """err = denoise.relative_mse against passes 64 .. 1087 of the same scene.  Asserted for cornell and multi_material: denoise_spatial at
    N = 1 beats the plain frame at 2 passes (the bar the plain denoiser is held to from N = 4 on).  N = 2, N = 3, the factors and the soup
    are printed (lines starting SPATIAL_BUYS; DESIGN.md records them)."""
    mk, asserted = BUYS[name]
    ref = truth(mk)
    for N in (1, 2, 3):
        eng = engine_with_passes(mk(), range(N))
        frame = eng.readback()
        den, sp = eng.denoise(), eng.denoise_spatial()
        render_passes(eng, mk(), range(N, 2 * N))
        f2 = eng.readback()
        eng.close()
        e1, e2 = (denoise.relative_mse(f[..., :3] / f[..., 3:4], ref) for f in (frame, f2))
        ed, es = denoise.relative_mse(den, ref), denoise.relative_mse(sp, ref)
        print(f"SPATIAL_BUYS {name} N={N}: frame at N {e1:.5f}  at 2N {e2:.5f}  denoise at N {ed:.5f}  denoise_spatial at N {es:.5f}"
              f"  (frame at 2N / denoise_spatial: {e2 / es:.2f})")
        if asserted and N == 1:
            assert es < e2, (name, es, e2)


def test_what_it_buys_in_a_disocclusion():
    """cornell: 256 passes, capture, an orbit by 0.3, one pass of the new view, merge.  Over the pixels the merge rejected (F.a == 1: raw
    one-sample noise beside a history-rich surround) denoise_spatial's error is below denoise's; truth: passes 64 .. 1087 at the new
    camera."""
    mk = BUYS["cornell"][0]
    sc = mk()
    eng = engine_with_passes(sc, range(256))
    new_view = orbit(sc.options, 0.3)
    res = history.move_camera(eng, sc.options, new_view, 1)
    frame = eng.readback()
    rejected = frame[..., 3] == 1
    assert res["rejected_pixels"] > 0 and 0 < rejected.sum() < rejected.size
    den = eng.denoise()
    sp, r = eng.denoise_spatial(with_result=True)
    same(sp, denoise_spatial.reference(frame, eng.aovs()), "after a history merge")
    assert r["spatial_pixels"] >= int(rejected.sum())
    eng.close()

    def mk_new():
        s = mk()
        s.options.view_matrix = new_view
        return s
    ref = truth(mk_new)
    sub = lambda img: denoise.relative_mse(img[rejected][None, :, :3], ref[rejected][None])
    inside = [sub(frame[..., :3] / frame[..., 3:4]), sub(den), sub(sp)]
    keep = ~rejected
    outside = [denoise.relative_mse(img[keep][None, :, :3], ref[keep][None]) for img in (den, sp)]
    print(f"SPATIAL_BUYS cornell disocclusion (orbit 0.3, {int(rejected.sum())} rejected pixels of {rejected.size}): inside: frame {inside[0]:.5f}  denoise {inside[1]:.5f}"
          f"  denoise_spatial {inside[2]:.5f} | outside: denoise {outside[0]:.5f}  denoise_spatial {outside[1]:.5f}")
    assert inside[2] < inside[1], inside
