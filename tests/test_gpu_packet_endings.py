"""How the camera-ray packets end (heatray_amd/csrc/hr_raygen.hip: raygenPackets): a ray that hits nothing runs its miss shader in the
packet kernel and leaves nothing behind, a ray that hits stores its ray and its hit record after the traversal and is put on its pass's
hit list by the packet kernel itself (PBR from the front, glass from the back, an invalid material not at all); k_shade_sort leaves
these passes' camera rays out.  Nothing of that
may show: every frame here is the CPU oracle's bit for bit, and frame and counters are those of the same engine with one ray per lane
(HR_TUNE packets=0: k_raygen, k_trace and the miss shader of k_shade_sort).  A launch with a lens runs the packet kernel without the in-place
endings (k_raygen_packets_rays<.., false>: every ray stored, misses shaded and hits listed by k_shade_sort); its case holds it to the same frames and counters.

Frames of 70 x 50 pixels (lanes beyond the frame, partial tiles), 19 passes (a full batch of 16, then 2 + 1), packets forced on
(packets=1: no probe can switch them off), in front of k_trace (corun=0) and beside it on the second stream (corun=2)."""

import numpy as np
import pytest

import oracle_lib
from device_support import F, host_tables, same
from heatray_amd import _ffi as ffi
from heatray_amd import core, host, scenes

pytestmark = pytest.mark.gpu

W, H, PASSES = 70, 50, 19
CORUN = (0, 2)
COUNTERS = ("paths", "rays_closest", "rays_any", "accumulates", "shaded_hits")


def _grid(x0, x1, y0, y1, z, n=4):
    """the rectangle [x0, x1] x [y0, y1] in the plane of this z, facing +z, as n x n quads"""
    xs, ys = np.linspace(x0, x1, n + 1), np.linspace(y0, y1, n + 1)
    return [scenes._quad((xs[i], ys[j], z), (xs[i + 1], ys[j], z), (xs[i + 1], ys[j + 1], z), (xs[i], ys[j + 1], z)) for j in range(n) for i in range(n)]


def _mesh(parts, material_id):
    p, n, i = scenes._merge(parts)
    return scenes.MeshData(p, n, i, material_id=material_id)


def _tiny_far_triangle():
    """widens the root's box far beyond the frame: the rays beside the quad pass the root cull, walk the tree and hit nothing"""
    p = np.array([(30.0, 20.0, -40.0), (30.01, 20.0, -40.0), (30.0, 20.01, -40.0)], dtype=F)
    return p, np.tile(np.array([0.0, 0.0, 1.0], dtype=F), (3, 1)), np.arange(3, dtype=np.uint32)


def _scene(name):
    """The camera stands at (0, 0, 3) and looks along -z: the frame is [-1.008, 1.008] x [-0.72, 0.72] in the plane z = 0.  A quad
    fills its left part up to x = 0.2 and y = 0.5: packets whose every ray hits, packets whose every ray misses, mixed ones between."""
    sc = scenes.Scene("endings_" + name, width=W, height=H)
    sc.materials = {0: host.bake_pbr(base_color=(0.8, 0.6, 0.3), roughness=0.6, metallic=0.0)}
    if name == "materials":  # PBR | glass | a triangle strip of a material nobody set: front of the hit list, its back, not listed
        sc.materials[1] = host.bake_glass(base_color=(0.7, 0.9, 0.8), roughness=0.05, ior=1.5, density=0.5)
        sc.meshes.append(_mesh(_grid(-3.0, -0.4, -3.0, 0.5, 0.0), 0))
        sc.meshes.append(_mesh(_grid(-0.4, 0.2, -3.0, 0.5, 0.0), 1))
        sc.meshes.append(_mesh(_grid(0.3, 0.6, -0.5, 0.3, 0.0, n=2), 7))
    else:
        sc.meshes.append(_mesh(_grid(-3.0, 0.2, -3.0, 0.5, 0.0), 0))
    sc.meshes.append(_mesh([_tiny_far_triangle()], 0))
    sc.lights.add_directional(color=(1, 1, 1), illuminance=3.0, phi=0.4, theta=1.0)
    if name != "no_environment":
        sc.env_pixels = scenes.synthetic_hdri(64, 32)  # (small and far from constant: a wrong direction or weight shows)
    o = sc.options
    o.max_ray_depth, o.max_render_passes = 3, 32
    o.fstop = 1.4 if name == "lens" else host.FSTOP_DISABLED  # (a lens: k_raygen_packets_rays<.., false>)
    o.focal_length, o.focus_distance, o.aspect_ratio = 50.0, 3.0, W / H
    m = np.eye(4, dtype=F)
    m[:3, 3] = (0.0, 0.0, 3.0)
    o.view_matrix = m
    if name == "all_lights":
        o.estimator = ffi.HR_ESTIMATOR_ALL_LIGHTS
    return sc


def _mask():
    """pixels switched off: every third column, one 8 x 8 block on the quad's edge and one beside the quad"""
    y, x = np.mgrid[0:H, 0:W]
    m = (x % 3 != 1).astype(np.uint8)
    m[16:24, 32:40] = 0
    m[32:40, 56:64] = 0
    return m


def _device(sc, golden, name, tune, monkeypatch, **kw):
    """frame, counters and (for "aov") the surface planes of PASSES passes under this HR_TUNE"""
    monkeypatch.setenv("HR_TUNE", tune)
    eng = core.create_engine(**kw)
    sc.apply(eng, lut=golden["multiscatter_lut"], tables=host_tables(sc))
    if name == "aov":
        eng.set_aovs(ffi.HR_AOV_SURFACE)
    if name == "mask":
        eng.set_sample_mask(_mask())
    for s in range(PASSES):
        eng.render_pass(sc.options.pass_params(s))
    frame = eng.readback().copy()
    planes = eng.aovs() if name == "aov" else None
    st = eng.stats().as_dict()
    eng.close()
    return frame, {k: st[k] for k in COUNTERS}, planes


_ORACLE = {}


def _oracle(sc, golden, name):
    """the oracle's frame, computed once per scene (the oracle knows no mask: the masked frame is put together from its passes)"""
    if name not in _ORACLE:
        o = oracle_lib.engine()
        sc.apply(o, lut=golden["multiscatter_lut"], tables=host_tables(sc))
        if name == "mask":
            acc = np.zeros((H, W, 4), dtype=F)
            for s in range(PASSES):
                o.clear()
                o.render_pass(sc.options.pass_params(s))
                acc = (acc + np.where((_mask() != 0)[..., None], o.readback(), F(0.0)).astype(F)).astype(F)
            _ORACLE[name] = acc
        else:
            for s in range(PASSES):
                o.render_pass(sc.options.pass_params(s))
            _ORACLE[name] = o.readback().copy()
        o.close()
    return _ORACLE[name]


_PER_LANE = {}


def _per_lane(sc, golden, name, monkeypatch):
    if name not in _PER_LANE:
        _PER_LANE[name] = _device(sc, golden, name, "packets=0", monkeypatch)
    return _PER_LANE[name]


def _check(monkeypatch, golden, name, corun, more="", **kw):
    sc = _scene(name)
    want = _oracle(sc, golden, name)
    ref_frame, ref_counters, ref_planes = _per_lane(sc, golden, name, monkeypatch)
    same(ref_frame, want, f"{name}: packets=0 against the oracle")
    frame, counters, planes = _device(sc, golden, name, f"packets=1,corun={corun}{more}", monkeypatch, **kw)
    print(name, "corun", corun, more, counters)
    same(frame, want, f"{name}, corun={corun}: against the oracle")
    same(frame, ref_frame, f"{name}, corun={corun}: against packets=0")
    assert counters == ref_counters, (name, corun, counters, ref_counters)
    if planes is not None:
        for k in ("albedo", "normal_depth"):
            same(planes[k], ref_planes[k], f"{name}, corun={corun}: plane {k} against packets=0")
    return frame, counters


@pytest.mark.parametrize("corun", CORUN)
def test_quad_and_tiny_triangle_with_an_environment(monkeypatch, golden, corun):
    frame, counters = _check(monkeypatch, golden, "environment", corun)
    assert (frame[..., 3] == PASSES).all()
    # the scene is what the case needs: camera rays that hit (shaded) and camera rays that end on the environment
    assert 0 < counters["shaded_hits"] and counters["paths"] == W * H * PASSES
    lit = frame[..., :3].sum(axis=-1)
    assert (lit[:, W - 8:] > 0).all(), "the pixels right of the quad see the environment"


@pytest.mark.parametrize("corun", CORUN)
def test_without_an_environment_a_miss_accumulates_nothing(monkeypatch, golden, corun):
    frame, _ = _check(monkeypatch, golden, "no_environment", corun)
    assert (frame[..., 3] == PASSES).all()
    assert (frame[:, W - 8:, :3] == 0).all() and not np.signbit(frame[:, W - 8:, :3]).any()


@pytest.mark.parametrize("corun", CORUN)
def test_pbr_glass_and_an_invalid_material(monkeypatch, golden, corun):
    _check(monkeypatch, golden, "materials", corun)


@pytest.mark.parametrize("corun", CORUN)
@pytest.mark.parametrize("mode", ["all_lights", "aov", "mask"])
def test_modes(monkeypatch, golden, mode, corun):
    frame, _ = _check(monkeypatch, golden, mode, corun)
    if mode == "mask":
        assert (frame[..., 3] == np.where(_mask() != 0, F(PASSES), F(0.0))).all()


@pytest.mark.parametrize("corun", CORUN)
def test_two_shards_on_one_device(monkeypatch, golden, corun):
    name = "environment"
    sc = _scene(name)
    tune = f"packets=1,corun={corun}"
    one, one_counters, _ = _device(sc, golden, name, tune, monkeypatch, tile_size=16)
    parts = [_device(sc, golden, name, tune, monkeypatch, rank=r, world=2, tile_size=16) for r in range(2)]
    assert (sum((p[0][..., 3] > 0).astype(int) for p in parts) == 1).all()
    same(parts[0][0] + parts[1][0], one, f"corun={corun}: two shards against one context")
    same(one, _oracle(sc, golden, name), f"corun={corun}: one context, 16 x 16 tiles, against the oracle")
    assert {k: parts[0][1][k] + parts[1][1][k] for k in COUNTERS} == one_counters


@pytest.mark.parametrize("corun", CORUN)
def test_lens(monkeypatch, golden, corun):
    _check(monkeypatch, golden, "lens", corun)


@pytest.mark.parametrize("corun", CORUN)
def test_per_ray_step_kernel_without_a_lens(monkeypatch, golden, corun):
    # pstep=0: k_raygen_packets_rays<.., true>, the per-ray body WITH the in-place endings (a lens runs <.., false>: misses end in k_shade_sort)
    _check(monkeypatch, golden, "environment", corun, more=",pstep=0")


@pytest.mark.parametrize("corun", CORUN)
@pytest.mark.parametrize("name", ["materials", "lens"])
def test_with_the_traversal_counters_collected(monkeypatch, golden, name, corun):
    # collect_stats: k_raygen_packets<true, ..>, the per-ray body that ends and lists its rays itself — with a lens too (the one launch
    # with a lens that does): k_shade_sort must leave exactly those passes out
    _check(monkeypatch, golden, name, corun, collect_stats=True)
