"""AOVs (include/hrcore_aov.h) on the GPU.  The frame never changes when they are on; ALBEDO and NORMAL_DEPTH are, bit for bit, what the
debug visualizers write (which are pinned to the oracle by test_gpu_parity.py::test_debug_visualizers); depth follows the camera
geometry; MOMENTS is the float32 sequential sum of the squared samples; the planes live and die with the frame; and a context group or a
tile-sharded context gives a plain context's planes."""
import ctypes as C

import numpy as np
import pytest

from device_support import F, render_passes, same
from heatray_amd import _ffi as ffi
from heatray_amd import aov, core, host, scenes

pytestmark = pytest.mark.gpu
SURF, MOM, BOTH = ffi.HR_AOV_SURFACE, ffi.HR_AOV_MOMENTS, ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS
ALB, ND, MOMP = ffi.HR_AOV_PLANE_ALBEDO, ffi.HR_AOV_PLANE_NORMAL_DEPTH, ffi.HR_AOV_PLANE_MOMENTS


def _run(sc, mask, passes, engine=None, **kw):
    """(frame, {plane name: sums, "passes": n}) of a render with the AOVs of `mask` enabled before the first pass."""
    eng = engine if engine is not None else core.create_engine()
    sc.apply(eng)
    if mask:
        eng.set_aovs(mask)
    render_passes(eng, sc, passes, **kw)
    frame = eng.readback()
    planes = eng.aovs() if mask else {}
    eng.close()
    return frame, planes


def _no_env(sc):
    sc.env_pixels = None
    sc.lights.env_enabled = False
    return sc


# ---------------------------------------------------------------------------------------------------------- 1. the frame is unchanged
FRAME_CASES = {
    **{f"multi_material_textured_est{e}_lod{l}": (lambda e=e, l=l: (scenes.multi_material(64, 36, bounces=4, textured=True), dict(estimator=e, texture_lod=l)))
       for e in (ffi.HR_ESTIMATOR_REFERENCE, ffi.HR_ESTIMATOR_ENV_MIS, ffi.HR_ESTIMATOR_ALL_LIGHTS) for l in (ffi.HR_TEXTURE_LOD_BASE, ffi.HR_TEXTURE_LOD_CONE)},
    "glass_soup": lambda: (scenes.triangle_soup(3000, width=96, height=64, bounces=6, env=True, glass_fraction=0.5), {}),
    "stacked_sheets": lambda: (scenes.stacked_sheets(40, width=48, height=32, bounces=3), {}),
    "visualizer_base_color": lambda: (scenes.multi_material(64, 36, bounces=2, textured=True), dict(enable_visualizer=1, visualizer_mode=ffi.HR_VIS_BASE_COLOR)),
}


@pytest.mark.parametrize("case", sorted(FRAME_CASES))
def test_frame_is_unchanged_with_aovs_on(case):
    sc, kw = FRAME_CASES[case]()
    off, _ = _run(sc, 0, range(6), **kw)
    for mask in (SURF, BOTH):
        sc, kw = FRAME_CASES[case]()
        on, planes = _run(sc, mask, range(6), **kw)
        same(on, off, f"{case}: frame with AOVs {mask}")
        assert planes["passes"] == 6
        if mask & MOM:
            same(planes["moments"][..., 3:], on[..., 3:], f"{case}: MOMENTS.a is the frame's alpha")


def test_frame_is_unchanged_in_interactive_mode():
    def run(mask):
        sc = scenes.multi_material(66, 39, bounces=3)
        sc.options.enable_interactive_mode = True
        eng = core.create_engine()
        sc.apply(eng)
        if mask:
            eng.set_aovs(mask)
        for by in range(3):
            for bx in range(3):
                eng.render_pass(sc.options.pass_params(by, current_block_pixel=(bx, by)))
        out = eng.readback(), (eng.aovs() if mask else None)
        eng.close()
        return out
    off, _ = run(0)
    on, planes = run(BOTH)
    same(on, off, "interactive")
    assert (planes["moments"][..., 3] == on[..., 3]).all() and (on[..., 3] == 1.0).all()
    assert (planes["albedo"][..., 3] <= 1.0).all() and planes["albedo"][..., 3].sum() > 0


def test_frame_is_unchanged_under_a_tight_memory_budget():
    sc = scenes.triangle_soup(20000, width=320, height=180, bounces=4, env=True)
    off, _ = _run(sc, 0, range(24))
    sc = scenes.triangle_soup(20000, width=320, height=180, bounces=4, env=True)
    tight = core.create_engine(memory_budget=256 << 20)
    on, planes = _run(sc, BOTH, range(24), engine=tight)
    same(on, off, "memory budget")
    assert planes["passes"] == 24
    same(planes["moments"][..., 3:], on[..., 3:], "memory budget: MOMENTS.a")


# ------------------------------------------------------------------------------------------------ 2. ALBEDO = HR_VIS_BASE_COLOR
ALBEDO_SCENES = {
    "multi_material_textured": lambda: _no_env(scenes.multi_material(64, 36, bounces=3, textured=True)),
    "stacked_sheets": lambda: _no_env(scenes.stacked_sheets(40, width=48, height=32, bounces=3)),
    "glass_soup": lambda: _no_env(scenes.triangle_soup(3000, width=96, height=64, bounces=4, glass_fraction=0.5)),
}


@pytest.mark.parametrize("name", sorted(ALBEDO_SCENES))
def test_albedo_is_the_base_color_visualizer(name):
    n = 5
    frame, planes = _run(ALBEDO_SCENES[name](), SURF, range(n))
    vis, _ = _run(ALBEDO_SCENES[name](), 0, range(n), enable_visualizer=1, visualizer_mode=ffi.HR_VIS_BASE_COLOR)
    alb = planes["albedo"]
    same(alb[..., :3].copy(), vis[..., :3].copy(), f"{name}: ALBEDO.rgb vs HR_VIS_BASE_COLOR")
    assert (alb[..., 3] == vis[..., 3] - frame[..., 3]).all(), name
    assert alb[..., 3].max() == n and alb[..., :3].max() > 0.0
    if name == "stacked_sheets":  # every camera ray passes the sheets: what one pass records is the surface behind them
        _, one = _run(ALBEDO_SCENES[name](), SURF, [2])
        a = one["albedo"]
        hit = a[..., 3] == 1
        assert hit.mean() > 0.5 and (a[~hit] == 0).all()
        wall = np.array(host.bake_pbr(base_color=(0.7, 0.7, 0.75), roughness=0.9).base_color[:], F)
        sheet = np.array([0.9, 0.8, 0.7], F)  # (an opaque texel of an alpha sheet is a surface too)
        is_wall = np.isclose(a[hit][:, :3], wall, atol=1e-6).all(axis=1)
        assert (is_wall | np.isclose(a[hit][:, :3], sheet, atol=1e-6).all(axis=1)).all() and is_wall.mean() > 0.5


# ------------------------------------------------------------------------------------------------------------- 3. normals
def _normal_mapped_scene():
    """test_gpu_parity.py::test_debug_visualizers' normal-mapped, tangent-space mesh (every texture slot filled)."""
    rng = np.random.default_rng(17)
    tex = lambda c: ((rng.uniform(0.2, 1.0, (16, 16, c)) * 255).astype(np.uint8), ffi.HR_WRAP_REPEAT, ffi.HR_FILTER_LINEAR)
    sc = _no_env(scenes.multi_material(64, 36, bounces=2))
    sc.textures = [tex(4), tex(3), tex(3), tex(3), tex(1), tex(1), tex(3)]
    sc.materials[3] = host.bake_pbr(base_color=(0.7, 0.6, 0.5), roughness=0.5, metallic=0.2, clear_coat=1.0, clear_coat_roughness=0.3,
                                    base_color_texture=0, metallic_roughness_texture=1, emissive_texture=2, normalmap=3,
                                    clear_coat_texture=4, clear_coat_roughness_texture=5, clear_coat_normalmap=6)
    for me in sc.meshes:
        k = me.positions.shape[0]
        me.tangents = np.tile(np.array([1, 0, 0], F), (k, 1))
        me.bitangents = np.tile(np.array([0, 0, 1], F), (k, 1))
        me.material_id = 3
    return sc


def test_normals_per_pass_are_the_final_normals_visualizer():
    for k in (0, 3, 11):
        frame, planes = _run(_normal_mapped_scene(), SURF, [k])
        vis, _ = _run(_normal_mapped_scene(), 0, [k], enable_visualizer=1, visualizer_mode=ffi.HR_VIS_FINAL_NORMALS)
        nd, hit = planes["normal_depth"], planes["albedo"][..., 3] > 0
        want = np.where(hit[..., None], (nd[..., :3] + F(1.0)) * F(0.5), F(0.0)).astype(F)
        same(want, vis[..., :3].copy(), f"sample {k}: (N + 1) * 0.5 vs HR_VIS_FINAL_NORMALS")
        assert hit.mean() > 0.5 and (nd[~hit] == 0).all()


def test_normals_over_many_passes():
    n = 12
    _, planes = _run(_normal_mapped_scene(), SURF, range(n))
    hits = planes["albedo"][..., 3]
    full = hits == n
    assert full.mean() > 0.3
    mean = planes["normal_depth"][full][:, :3].astype(np.float64) / n
    ref = np.zeros_like(mean)
    for k in range(n):  # the visualizer's normals of every pass, averaged on the host
        vis, _ = _run(_normal_mapped_scene(), 0, [k], enable_visualizer=1, visualizer_mode=ffi.HR_VIS_FINAL_NORMALS)
        ref += vis[full][:, :3].astype(np.float64) * 2.0 - 1.0
    ref /= n
    unit = lambda v: v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)
    np.testing.assert_allclose(unit(mean), unit(ref), atol=1e-5)


# --------------------------------------------------------------------------------------------------------------- 4. depth
def _plane_scene(d, tilt=0.0, w=48, h=32):
    """A large double-sided quad through (0, 0, -d) (camera at the origin looking down -z), rotated by `tilt` about the x axis."""
    sc = scenes.Scene("plane", width=w, height=h)
    c, s = np.cos(tilt), np.sin(tilt)
    L = 50.0 * d
    corners = [(-L, -L), (L, -L), (L, L), (-L, L)]
    pos = np.array([(x, y * c, -d - y * s) for x, y in corners], F)
    nrm = np.tile(np.array([0.0, s, c], F), (4, 1))
    sc.materials[0] = host.bake_pbr(base_color=(0.5, 0.5, 0.5), roughness=1.0, double_sided=True)
    sc.meshes.append(scenes.MeshData(pos, nrm, np.array([0, 1, 2, 0, 2, 3], np.uint32), material_id=0))
    sc.lights.add_directional(illuminance=683.0, phi=0.3, theta=0.5)
    o = sc.options
    o.max_ray_depth, o.max_render_passes = 2, 8
    o.aspect_ratio = w / h
    o.view_matrix = np.eye(4, dtype=F)
    o.focus_distance = d
    o.fstop = host.FSTOP_DISABLED
    return sc


def test_depth_of_a_fronto_parallel_plane():
    for d in (0.75, 3.0, 20.0):
        _, planes = _run(_plane_scene(d), SURF, range(4))
        hits = planes["albedo"][..., 3]
        assert (hits == 4).all()
        np.testing.assert_allclose(planes["normal_depth"][..., 3] / hits, d, rtol=1e-5)


def test_depth_of_a_tilted_plane_follows_the_camera_geometry():
    d, tilt = 4.0, 0.5
    sc = _plane_scene(d, tilt)
    _, planes = _run(sc, SURF, [0])
    hit = planes["albedo"][..., 3] == 1
    assert hit.all()
    # the camera ray through the pixel's sample point hits the plane n.(p - (0, 0, -d)) = 0 at depth z = d / (cos + sin y_c / -z_c ...):
    # along the ray o + t dir (o = 0: no aperture), depth = -t dir.z with t = -d cos / (n . dir)
    ys = np.arange(sc.height, dtype=np.float64)
    p = sc.options.pass_params(0)
    n = np.array([0.0, np.sin(tilt), np.cos(tilt)])
    depth = planes["normal_depth"][..., 3]
    # the ray's direction depends on the pixel's jitter; depth = d cos / (cos - sin * cy), cy = direction.y / -direction.z in [row +- 1 px]
    for y in (2, sc.height // 2, sc.height - 3):
        lo = (1.0 - 2.0 * (y + 1.0) / sc.height) * p.fov_tan * -1.0
        hi = (1.0 - 2.0 * (y - 0.0) / sc.height) * p.fov_tan * -1.0
        want = [d * n[2] / (n[2] - n[1] * cy) for cy in (lo, hi)]
        assert (depth[y] >= min(want) * (1 - 1e-5)).all() and (depth[y] <= max(want) * (1 + 1e-5)).all(), (y, depth[y].min(), depth[y].max(), want)
    assert np.all(np.diff(depth.mean(axis=1)) != 0)


# ------------------------------------------------------------------------------------------------------------- 5. MOMENTS
@pytest.mark.parametrize("estimator", [ffi.HR_ESTIMATOR_REFERENCE, ffi.HR_ESTIMATOR_ALL_LIGHTS])
def test_moments_are_the_sequential_sum_of_squared_samples(estimator):
    K = 6
    mk = lambda: scenes.multi_material(48, 32, bounces=4, textured=True)
    want = None
    for k in range(K):  # each in a fresh context: the frame is exactly the sample s_k
        s, _ = _run(mk(), 0, [k], estimator=estimator)
        sq = (s * s).astype(F)
        if want is None:
            want = np.zeros_like(s)
        want[..., :3] = want[..., :3] + sq[..., :3]
        want[..., 3] = want[..., 3] + s[..., 3]
    frame, planes = _run(mk(), MOM, range(K), estimator=estimator)
    assert set(planes) == {"moments", "passes"} and planes["passes"] == K
    same(planes["moments"], want, "MOMENTS vs numpy")
    same(planes["moments"][..., 3:], frame[..., 3:], "MOMENTS.a vs the frame's alpha")
    r = aov.resolve(planes, frame)
    assert np.isfinite(r["variance"]).all() and r["variance"].max() > 0


# ----------------------------------------------------------------------------------------------------------- 6. life cycle
def test_life_cycle():
    sc = scenes.multi_material(64, 36, bounces=3)
    eng = core.create_engine()
    sc.apply(eng)
    with pytest.raises(ffi.EngineError, match="not enabled"):
        eng.aov_plane(ALB)
    assert eng.aov_mask() == 0 and eng.aovs() == {}
    render_passes(eng, sc, range(3))
    eng.set_aovs(BOTH)                                    # enabled after 3 passes: the planes start at zero
    assert eng.aov_mask() == BOTH
    alb, n = eng.aov_plane(ALB)
    assert n == 0 and not alb.any()
    render_passes(eng, sc, range(3, 7))
    frame = eng.readback()
    planes = eng.aovs()
    assert planes["passes"] == 4 and (planes["moments"][..., 3] == 4).all() and (frame[..., 3] == 7).all()
    # the same four passes in a context that had AOVs from the start of a cleared frame
    ref = core.create_engine()
    sc.apply(ref)
    ref.set_aovs(BOTH)
    render_passes(ref, sc, range(3, 7))
    for name in ("albedo", "normal_depth", "moments"):
        same(planes[name], ref.aovs()[name], f"enabled late: {name}")
    ref.close()
    for bad in (-1, 3, 99):
        with pytest.raises(ffi.EngineError, match="bad AOV plane"):
            eng.aov_plane(bad)
    with pytest.raises(ffi.EngineError, match="unknown AOV mask"):
        eng.set_aovs(4)
    eng.clear()                                           # hr_clear zeroes them
    for p in (ALB, ND, MOMP):
        a, n = eng.aov_plane(p)
        assert n == 0 and not a.any()
    render_passes(eng, sc, range(2))
    eng.resize(40, 30)                                    # so does a resize, at the new size
    for p in (ALB, ND, MOMP):
        a, n = eng.aov_plane(p)
        assert a.shape == (30, 40, 4) and n == 0 and not a.any()
    render_passes(eng, sc, range(2))
    assert eng.aovs()["passes"] == 2
    eng.set_aovs(MOM)                                     # a smaller mask frees what it no longer names
    with pytest.raises(ffi.EngineError, match="not enabled"):
        eng.aov_plane(ALB)
    eng.set_aovs(0)
    for p in (ALB, ND, MOMP):
        with pytest.raises(ffi.EngineError, match="not enabled"):
            eng.aov_plane(p)
    render_passes(eng, sc, range(2))                             # and the plain path renders on
    assert (eng.readback()[..., 3] == 4).all()
    eng.close()


def test_aov_to_device_is_the_readback():
    import torch
    sc = scenes.multi_material(64, 36, bounces=3)
    eng = core.create_engine()
    sc.apply(eng)
    eng.set_aovs(BOTH)
    render_passes(eng, sc, range(4))
    for p in (ALB, ND, MOMP):
        t = torch.empty((36, 64, 4), dtype=torch.float32, device="cuda:0")
        eng.aov_to_device(p, t.data_ptr())
        eng.synchronize()
        torch.cuda.synchronize()
        same(t.cpu().numpy(), eng.aov_plane(p)[0], f"plane {p}: device copy")
    s = torch.cuda.Stream()
    t = torch.empty((36, 64, 4), dtype=torch.float32, device="cuda:0")
    eng.aov_to_device(ALB, t.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    same(t.cpu().numpy(), eng.aov_plane(ALB)[0], "copy on a foreign stream")
    eng.close()


@pytest.mark.parametrize("tune", ["packets=0", "packets=1", "batch=1", "batch=5,groups=2"])
def test_planes_do_not_depend_on_scheduling(tune, monkeypatch):
    mk = lambda: scenes.triangle_soup(3000, width=96, height=64, bounces=4, env=True, glass_fraction=0.25, passthrough_fraction=0.25)
    ref_frame, ref = _run(mk(), BOTH, range(10))
    monkeypatch.setenv("HR_TUNE", tune)
    frame, planes = _run(mk(), BOTH, range(10))
    same(frame, ref_frame, f"{tune}: frame")
    for name in ("albedo", "normal_depth", "moments"):
        same(planes[name], ref[name], f"{tune}: {name}")


# ------------------------------------------------------------------------------------------------------------- 7. sharding
def _owned(h, w, tile, rank, world):
    ty, tx = np.meshgrid(np.arange(h) // tile, np.arange(w) // tile, indexing="ij")
    return ((ty * ((w + tile - 1) // tile) + tx) % world) == rank


def test_group_of_three_on_one_device_gives_a_plain_contexts_planes():
    mk = lambda: scenes.multi_material(100, 70, bounces=3, textured=True)
    ref_frame, ref = _run(mk(), BOTH, range(5))
    grp = core.create_group([0, 0, 0], tile_size=16)
    sc = mk()
    sc.apply(grp)
    grp.set_aovs(BOTH)
    assert grp.aov_mask() == BOTH
    render_passes(grp, sc, range(5))
    same(grp.readback(), ref_frame, "group frame")
    planes = grp.aovs()
    assert planes["passes"] == 5
    for name in ("albedo", "normal_depth", "moments"):
        same(planes[name], ref[name], f"group: {name}")
    import torch
    t = torch.empty((70, 100, 4), dtype=torch.float32, device="cuda:0")
    grp.aov_to_device(ND, t.data_ptr())
    grp.synchronize()
    torch.cuda.synchronize()
    same(t.cpu().numpy(), ref["normal_depth"], "group: device copy")
    grp.clear()
    a, n = grp.aov_plane(MOMP)
    assert n == 0 and not a.any()
    grp.close()


def test_tile_sharded_contexts_own_their_pixels_and_zero_the_rest():
    mk = lambda: scenes.multi_material(100, 70, bounces=3, textured=True)
    _, ref = _run(mk(), BOTH, range(4))
    for rank in range(3):
        eng = core.create_engine(rank=rank, world=3, tile_size=16)
        _, planes = _run(mk(), BOTH, range(4), engine=eng)
        own = _owned(70, 100, 16, rank, 3)
        for name in ("albedo", "normal_depth", "moments"):
            same(planes[name][own], ref[name][own], f"rank {rank}: {name} on owned pixels")
            assert (planes[name][~own].view(np.uint32) == 0).all(), (rank, name)
