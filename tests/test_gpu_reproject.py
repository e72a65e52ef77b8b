"""The progressive history merge and the preview (include/hrcore_reproject.h) on the GPU.  Every comparison with the reference is exact: no
tolerance, no pixel left out.

1. non-interactive: hr_reproject_merge leaves what hr_history_merge leaves, and what heatray_amd.reproject.reference_merge_progressive
   gives (tests/test_reproject_ref.py ties that to the per-pixel header the kernels compile); a second call changes nothing
2. interactive mode: nine sub-passes, a merge after each, everything against the numpy chain fed the engine's own read-backs
3. the preview after sub-passes 1, 4 and 9 against reference_preview; it changes nothing; a foreign stream
4. a sample mask that switches a region off
5. the life cycle and every refusal
6. scheduling: HR_TUNE packets=0, packets=1 and batch=1 give the same bytes
7. what it buys: the error against 2048 passes at the new camera."""
import numpy as np
import pytest

from device_support import BOTH, F, device_engine, orbit, render, same
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise, history, reproject, scenes

pytestmark = pytest.mark.gpu
def state(eng):
    """everything a call may change: the frame, the three planes, the examined bits"""
    return eng.readback(), eng.aovs(), eng.reproject_examined()


def same_state(a, b, what):
    same(a[0], b[0], what + ": frame")
    for k in history.PLANES:
        same(a[1][k], b[1][k], f"{what}: {k}")
    same(a[2], b[2], what + ": examined")


SMALL = {
    "multi_material": lambda: scenes.multi_material(70, 45, bounces=4, textured=True),
    "cornell": lambda: scenes.cornell_box(70, 45, bounces=4),
}
OLD_PASSES = 24


def old_view(eng, sc, n=OLD_PASSES):
    """n passes of the view as it stands, captured: (the old camera, the history as the reference makes it)"""
    render(eng, [sc.options.pass_params(k) for k in range(n)])
    old_cam = sc.options.pass_params(0)
    want_hist = history.reference_capture(eng.readback(), eng.aovs())
    eng.history_capture(old_cam)
    same(eng.history(), want_hist, "history")
    return old_cam, want_hist


def sub_pass(options, k):
    return options.pass_params(0, current_block_pixel=reproject.sub_pass_pixel(k))


def merge_and_check(eng, hist, old_cam, cam, what, params=None, passes=None):
    """reproject_merge against the numpy reference fed the engine's own read-backs; returns (the result, the state after)"""
    frame, planes, E = state(eng)
    res = eng.reproject_merge(cam, params)
    after = state(eng)
    want_frame, want_planes, want_E, want = reproject.reference_merge_progressive(hist, old_cam, frame, planes, cam, E, params)
    same_state(after, (want_frame, want_planes, want_E), what)
    for k in ("reused_pixels", "rejected_pixels", "history_samples", "pending_pixels", "examined_pixels"):
        assert res[k] == want[k], (what, k, res, {k: v for k, v in want.items() if k != "nh"})
    assert res["history_passes"] == OLD_PASSES and (passes is None or res["passes"] == passes), (what, res)
    same(after[0][..., 3], after[1]["moments"][..., 3], f"{what}: F.a against M.a")
    assert (after[0][..., 3] == np.floor(after[0][..., 3])).all(), what
    return res, after


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("name", sorted(SMALL))
def test_one_call_on_a_full_frame_is_history_merge(golden, name):
    sc = SMALL[name]()
    new_view = orbit(sc.options, 0.05)
    a, b = device_engine(sc, golden), device_engine(sc, golden)
    old_cam, hist = old_view(a, sc)
    old_view(b, sc)
    sc.options.view_matrix = new_view
    cam = sc.options.pass_params(0)
    for eng in (a, b):
        eng.clear()
        assert not eng.reproject_examined().any()
        render(eng, [sc.options.pass_params(k) for k in range(2)])
    same_state(state(a), state(b), "two engines driven alike")
    plain = a.history_merge(cam)
    res, after = merge_and_check(b, hist, old_cam, cam, f"{name}: reproject_merge", passes=2)
    same(after[0], a.readback(), "frame against history_merge's")
    planes = a.aovs()
    for k in history.PLANES:
        same(after[1][k], planes[k], f"{k} against history_merge's")
    assert {k: res[k] for k in plain} == plain, (res, plain)
    unsampled = int((~(after[0][..., 3] > 0)).sum())
    assert res["pending_pixels"] == unsampled == 0 and res["examined_pixels"] == sc.width * sc.height and after[2].all()
    assert res["reused_pixels"] > 0.3 * sc.width * sc.height
    res2, after2 = merge_and_check(b, hist, old_cam, cam, f"{name}: a second call", passes=2)
    same_state(after2, after, "a second call changes nothing")
    assert (res2["reused_pixels"], res2["rejected_pixels"], res2["history_samples"]) == (0, 0, 0)
    assert (res2["pending_pixels"], res2["examined_pixels"]) == (0, sc.width * sc.height)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ 2 and 3
@pytest.mark.parametrize("dphi", [0.05, 0.3])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_interactive_mode_nine_sub_passes_with_a_merge_and_a_preview(golden, name, dphi):
    import torch
    sc = SMALL[name]()
    W, H = sc.width, sc.height
    new_view = orbit(sc.options, dphi)
    eng, never = device_engine(sc, golden), device_engine(sc, golden)  # `never` makes the same calls without a preview
    old_cam, hist = old_view(eng, sc)
    old_view(never, sc)
    sc.options.view_matrix = new_view
    sc.options.enable_interactive_mode = True
    cam = sc.options.pass_params(0)
    eng.clear(), never.clear()
    total = {"reused_pixels": 0, "rejected_pixels": 0}
    for k in range(9):
        eng.render_pass(sub_pass(sc.options, k)), never.render_pass(sub_pass(sc.options, k))
        res, after = merge_and_check(eng, hist, old_cam, cam, f"{name} {dphi}: sub-pass {k}", passes=k + 1)
        never.reproject_merge(cam)
        sampled = after[0][..., 3] > 0
        same(after[2], sampled, f"sub-pass {k}: examined = sampled")
        assert res["examined_pixels"] == int(sampled.sum()) and res["pending_pixels"] == W * H - int(sampled.sum())
        assert res["reused_pixels"] + res["rejected_pixels"] == int(sampled.sum()) - sum(total.values())  # the pixels this sub-pass sampled
        for key in total:
            total[key] += res[key]
        if k in (0, 3, 8):  # 3. the preview after sub-passes 1, 4 and 9
            image, counts = eng.reproject_preview(cam)
            want, want_counts = reproject.reference_preview(hist, old_cam, after[0], after[1], cam)
            same(image, want, f"{name} {dphi}: preview after sub-pass {k}")
            assert counts == want_counts and counts["own_pixels"] == int(sampled.sum()), (counts, want_counts)
            assert counts["own_pixels"] + counts["previewed_pixels"] + counts["empty_pixels"] == W * H
            if k == 8:
                assert counts["previewed_pixels"] == counts["empty_pixels"] == 0
            elif dphi == 0.05:
                assert counts["previewed_pixels"] > 0.5 * (W * H - counts["own_pixels"]), counts
            same_state(state(eng), after, f"{name} {dphi}: the preview after sub-pass {k} changed nothing")
            s = torch.cuda.Stream()
            t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            eng.reproject_preview_to_device(t.data_ptr(), cam, stream=s.cuda_stream)
            s.synchronize()
            same(t.cpu().numpy(), image, "the preview on a foreign stream")
            t2 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            eng.reproject_preview_to_device(t2.data_ptr(), cam)  # the ctx stream
            eng.synchronize()
            same(t2.cpu().numpy(), image, "the preview on the context's stream")
        same_state(state(eng), state(never), f"{name} {dphi}: sub-pass {k} against an engine that never previewed")
    assert res["pending_pixels"] == 0 and res["examined_pixels"] == W * H
    assert total["reused_pixels"] > 0.3 * W * H, total  # (sanity, not tuning: the bound tests/test_gpu_history.py asks of these scenes and moves)
    # a following render is what it is without the previews
    sc.options.enable_interactive_mode = False
    for e in (eng, never):
        render(e, [sc.options.pass_params(k) for k in range(1, 3)])
    same_state(state(eng), state(never), "the passes after")
    eng.close(), never.close()


# ------------------------------------------------------------------------------------------------ 4
def test_a_sample_mask_that_switches_a_region_off(golden):
    sc = SMALL["multi_material"]()
    W, H = sc.width, sc.height
    new_view = orbit(sc.options, 0.05)
    eng = device_engine(sc, golden)
    old_cam, hist = old_view(eng, sc)
    sc.options.view_matrix = new_view
    cam = sc.options.pass_params(0)
    eng.clear()
    mask = np.ones((H, W), np.uint8)
    mask[10:30, 20:50] = 0
    eng.set_sample_mask(mask)
    render(eng, [sc.options.pass_params(k) for k in range(2)])
    res, after = merge_and_check(eng, hist, old_cam, cam, "masked", passes=2)
    off = mask == 0
    assert res["pending_pixels"] == int(off.sum()) and not after[2][off].any() and after[2][~off].all()
    image, counts = eng.reproject_preview(cam)
    want, want_counts = reproject.reference_preview(hist, old_cam, after[0], after[1], cam)
    same(image, want, "masked: preview")
    assert counts == want_counts
    y, x = np.mgrid[0:H, 0:W]
    deep = (y >= 12) & (y < 28) & (x >= 22) & (x < 48)  # farther than two pixels from every sample
    assert not image[deep].any() and counts["empty_pixels"] >= int(deep.sum())
    rim = off & ~deep
    assert (image[rim][:, 3] == 1).mean() > 0.5 and counts["previewed_pixels"] == int((image[off][:, 3] == 1).sum())
    eng.close()


# ------------------------------------------------------------------------------------------------ 5
def test_the_life_cycle_and_every_refusal(golden):
    sc = SMALL["multi_material"]()
    W, H = sc.width, sc.height
    pp = sc.options.pass_params
    calls = lambda e: (lambda: e.reproject_merge(pp(0)), lambda: e.reproject_preview(pp(0)))
    # tile shards and a context group
    eng = core.create_engine(rank=1, world=2, tile_size=16)
    sc.apply(eng)
    eng.set_aovs(BOTH)
    eng.render_pass(pp(0))
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="tile-sharded.*world > 1"):
            call()
    eng.close()
    grp = core.create_group([0, 0], tile_size=16)
    sc.apply(grp)
    grp.set_aovs(BOTH)
    grp.render_pass(pp(0))
    for call in calls(grp):
        with pytest.raises(ffi.EngineError, match="context group"):
            call()
    with pytest.raises(ffi.EngineError, match="context group"):
        grp.reproject_examined()
    grp.close()

    eng = core.create_engine()
    sc.apply(eng)
    eng.render_pass(pp(0))
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="hr_aov_enable.*HR_AOV_SURFACE . HR_AOV_MOMENTS"):   # no planes
            call()
    eng.set_aovs(BOTH)                                                               # enabled after the frame's first pass
    eng.render_pass(pp(1))
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="hr_clear.*hr_aov_enable|hr_aov_enable.*hr_clear"):
            call()
    eng.clear()
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="empty"):                          # 0 passes
            call()
    render(eng, [pp(k) for k in range(4)])
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="no captured history"):
            call()
    assert not eng.reproject_examined().any()
    eng.history_capture(pp(0))
    for field, value in (("fov_tan", float("inf")), ("aspect_ratio", float("nan"))):
        bad = pp(0)
        setattr(bad, field, value)
        for call in (lambda: eng.reproject_merge(bad), lambda: eng.reproject_preview(bad)):
            with pytest.raises(ffi.EngineError, match="camera.*not finite"):
                call()
    bad = pp(0)
    bad.view_matrix[13] = float("nan")
    with pytest.raises(ffi.EngineError, match="camera.*not finite"):
        eng.reproject_merge(bad)

    def P(**kw):
        p = history.default_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    before = state(eng)
    nan, inf = float("nan"), float("inf")
    for kw, text in ((dict(max_history=0), "max_history"), (dict(max_history=65537), "max_history"), (dict(normal_cos=1.5), "normal_cos"), (dict(normal_cos=nan), "normal_cos"),
                     (dict(plane_tol=0.0), "plane_tol"), (dict(plane_tol=inf), "plane_tol"), (dict(min_weight=0.0), "min_weight"), (dict(min_weight=nan), "min_weight")):
        for call in (lambda: eng.reproject_merge(pp(0), P(**kw)), lambda: eng.reproject_preview(pp(0), P(**kw))):
            with pytest.raises(ffi.EngineError, match=text):
                call()
    same_state(state(eng), before, "after the refused calls")
    # after hr_history_merge the progressive call is refused (the preview is not) ...
    eng.history_merge(pp(0))
    with pytest.raises(ffi.EngineError, match="hr_history_merge has already merged"):
        eng.reproject_merge(pp(0))
    eng.reproject_preview(pp(0))
    # ... and after reproject_merge the plain merge is; the progressive one goes on
    eng.clear()
    assert not eng.reproject_examined().any()
    render(eng, [pp(k) for k in range(2)])
    r = eng.reproject_merge(pp(0))
    assert r["reused_pixels"] + r["rejected_pixels"] == W * H == r["examined_pixels"] and (r["history_passes"], r["passes"]) == (4, 2)
    with pytest.raises(ffi.EngineError, match="already been merged"):
        eng.history_merge(pp(0))
    r = eng.reproject_merge(pp(0))
    assert (r["reused_pixels"], r["rejected_pixels"], r["examined_pixels"]) == (0, 0, W * H)
    assert eng.reproject_examined().all()
    # a new capture and hr_history_drop leave E alone; without a history the merge is refused
    eng.history_capture(pp(0))
    assert eng.reproject_examined().all()
    eng.history_drop()
    assert eng.reproject_examined().all()
    for call in calls(eng):
        with pytest.raises(ffi.EngineError, match="no captured history"):
            call()
    # hr_clear resets E: the counters start from the full frame again
    eng.history_capture(pp(0))
    eng.clear()
    assert not eng.reproject_examined().any()
    eng.render_pass(pp(0))
    r = eng.reproject_merge(pp(0))
    assert r["reused_pixels"] + r["rejected_pixels"] == W * H == r["examined_pixels"] and r["pending_pixels"] == 0 and r["reused_pixels"] > 0
    # hr_frame_resize frees E and the history; a later call works
    eng.resize(W - 3, H - 2)
    assert eng.reproject_examined().shape == (H - 2, W - 3) and not eng.reproject_examined().any()
    sc2 = scenes.multi_material(W - 3, H - 2, bounces=4, textured=True)
    eng.render_pass(sc2.options.pass_params(0))
    with pytest.raises(ffi.EngineError, match="no captured history"):
        eng.reproject_merge(sc2.options.pass_params(0))
    eng.history_capture(sc2.options.pass_params(0))
    r = eng.reproject_merge(sc2.options.pass_params(0))
    assert r["examined_pixels"] == (W - 3) * (H - 2) and r["reused_pixels"] > 0
    image, counts = eng.reproject_preview(sc2.options.pass_params(0))
    assert image.shape == (H - 2, W - 3, 4) and counts["own_pixels"] == (W - 3) * (H - 2)
    eng.close()


# ------------------------------------------------------------------------------------------------ 6
def _interactive_run(golden, sub_passes=4):
    sc = SMALL["multi_material"]()
    new_view = orbit(sc.options, 0.05)
    eng = device_engine(sc, golden)
    render(eng, [sc.options.pass_params(k) for k in range(OLD_PASSES)])
    out = []
    results = reproject.move_camera_interactive(eng, sc.options, new_view, sub_passes, on_sub_pass=lambda k, r: out.append(eng.reproject_preview(sc.options.pass_params(0))))
    final = state(eng)
    eng.close()
    return results, out, final


def test_the_results_do_not_depend_on_the_scheduling(golden, monkeypatch):
    monkeypatch.delenv("HR_TUNE", raising=False)
    base = _interactive_run(golden)
    assert len(base[0]) == 4 and base[0][-1]["passes"] == 4 and base[0][0]["reused_pixels"] > 0
    for mode in ("packets=0", "packets=1", "batch=1"):
        monkeypatch.setenv("HR_TUNE", mode)
        got = _interactive_run(golden)
        assert got[0] == base[0], mode
        for (img, counts), (bimg, bcounts) in zip(got[1], base[1]):
            same(img, bimg, mode + ": preview")
            assert counts == bcounts
        same_state(got[2], base[2], mode)


# ------------------------------------------------------------------------------------------------ 7
BUYS = {
    "cornell": (lambda: scenes.cornell_box(128, 128, bounces=4, passes=2048), True),
    "multi_material": (lambda: scenes.multi_material(160, 90, bounces=4, passes=2048, textured=True), True),
    "soup": (lambda: scenes.triangle_soup(3000, 96, 64, bounces=4, passes=2048, env=True, glass_fraction=0.25), False),
}
BUYS_CASES = [("cornell", 0.05), ("cornell", 0.3), ("multi_material", 0.05), ("multi_material", 0.3), ("soup", 0.05)]


@pytest.mark.parametrize("name, dphi", BUYS_CASES)
def test_what_it_buys(golden, name, dphi):
    """denoise.relative_mse against 2048 passes at the new camera, after an orbit by dphi about the focus point that follows 256 passes at
    the old camera, in interactive mode (one pixel of every 3 x 3 block per sub-pass); default parameters:
      (a) the plain frame's mean after the first sub-pass (8/9 of it holes)
      (b) the plain frame's mean after nine sub-passes, no history — from the renderer alone
      (c) the preview after the first sub-pass, behind the progressive merge
    Asserted at an orbit of 0.05 for cornell and multi_material: (c) < (b) — one ninth of a pass plus history beats one whole pass
    without it.  Everything else (orbit 0.3, the soup) is printed (lines starting REPROJECT_BUYS) and recorded in DESIGN.md, not
    asserted.

    Measured on an MI355X (a / b / c; sampled pixels reused, pixels without a sample previewed; DESIGN.md §2 has the table):
      cornell 0.05:         0.2991 / 1.833 / 0.01767   97 %, 94 %
      cornell 0.3:          0.2879 / 1.863 / 0.05635   86 %, 84 %
      multi_material 0.05:  0.9793 / 1.479 / 0.08224   94 %, 93 %
      multi_material 0.3:   0.9767 / 1.334 / 0.3123    71 %, 69 %
      soup 0.05:            0.7099 / 0.9809 / 0.2024   86 %, 86 %"""
    mk, asserted = BUYS[name]
    sc = mk()
    eng = device_engine(sc, golden)
    new_view = orbit(sc.options, dphi)
    render(eng, [sc.options.pass_params(k) for k in range(256)])
    eng.history_capture(sc.options.pass_params(0))
    sc.options.view_matrix = new_view
    eng.clear()
    render(eng, [sc.options.pass_params(k) for k in range(2048)])
    ref = eng.readback()
    refm = ref[..., :3] / ref[..., 3:]
    mean = lambda f: f[..., :3] / np.maximum(f[..., 3:], F(1e-30))
    sc.options.enable_interactive_mode = True
    cam = sc.options.pass_params(0)
    eng.clear()  # the renderer alone: (a) and (b)
    eng.render_pass(sub_pass(sc.options, 0))
    a = denoise.relative_mse(mean(eng.readback()), refm)
    render(eng, [sub_pass(sc.options, k) for k in range(1, 9)])
    b = denoise.relative_mse(mean(eng.readback()), refm)
    eng.clear()  # (c)
    eng.render_pass(sub_pass(sc.options, 0))
    r = eng.reproject_merge(cam)
    image, counts = eng.reproject_preview(cam)
    c = denoise.relative_mse(image, refm)
    eng.close()
    unsampled = counts["previewed_pixels"] + counts["empty_pixels"]
    print(f"REPROJECT_BUYS {name} dphi {dphi}: (a) first sub-pass, plain {a:.4g} | (b) nine sub-passes, plain {b:.4g} | (c) first sub-pass, merge + preview {c:.4g}"
          f" | reused {r['reused_pixels'] / max(1, r['examined_pixels']):.0%} of the sampled, previewed {counts['previewed_pixels'] / max(1, unsampled):.0%} of the others")
    if asserted and dphi == 0.05:
        assert c < b, (c, b)
