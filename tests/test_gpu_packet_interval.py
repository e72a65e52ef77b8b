"""The interval step of the camera-ray packets (heatray_amd/csrc/hr_packet_interval.h; HR_TUNE pstep=1, the default, uses it where the
selector's probe finds it tight enough — always when packets are forced with packets=1, where nothing probes) on the device: the
packet enters a superset of the children its rays' own box tests enter, and every lane tests every triangle the packet reaches, so
the frame is the same bits as with the per-ray step (pstep=0), with one ray per lane (packets=0) and as the CPU oracle's — at the
smallest shapes where the step can go wrong.  tests/test_packet_interval_ref.py holds the arithmetic itself on the CPU."""
import copy

import numpy as np
import pytest

import oracle_lib
from device_support import host_tables
from heatray_amd import core, host, scenes

pytestmark = pytest.mark.gpu

TUNES = ("packets=1,pstep=1", "packets=1,pstep=0", "packets=0")


def _render(eng, sc, params, lut):
    sc.apply(eng, lut=lut, tables=host_tables(sc))
    for pp in params:
        eng.render_pass(pp)
    frame = eng.readback().copy()
    eng.close()
    return frame


def _same_frame_four_ways(monkeypatch, golden, sc, params, what):
    lut = golden["multiscatter_lut"]
    want = _render(oracle_lib.engine(), sc, params, lut)
    assert (want[..., 3] == len(params)).all(), what
    for tune in TUNES:
        monkeypatch.setenv("HR_TUNE", tune)
        got = _render(core.create_engine(), sc, params, lut)
        nbad = int((got != want).any(axis=-1).sum())
        assert got.tobytes() == want.tobytes(), f"{what} with HR_TUNE={tune}: {nbad} pixels differ from the oracle's"


def _passes(sc, n):
    return [sc.options.pass_params(s) for s in range(n)]


def _soup(n_tris=4096, width=96, height=72, **kw):
    return scenes.triangle_soup(n_tris, width=width, height=height, bounces=2, passes=32, env=True, **kw)


def _look(sc, eye, right, up, back):
    m = np.eye(4, dtype=np.float32)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, back, eye
    sc.options.view_matrix = m
    sc.options.aspect_ratio = sc.width / sc.height


def test_soup_with_partial_tiles(monkeypatch, golden):
    # 96 x 72 is no multiple of the 32 x 32 tile: waves at the frame's edge have lanes without a ray, which must stay out of the bounds
    sc = _soup()
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "soup 4096, 96x72")


def test_camera_inside_looking_along_an_axis(monkeypatch, golden):
    # from the soup's centre along +z: the packets around the frame's centre hold rays of both signs in x and in y (the per-ray step,
    # reached by a wave-uniform branch), their neighbours take the interval step
    sc = _soup(width=32, height=32)
    _look(sc, (0.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -1.0))
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "camera at the centre along +z")


def test_depth_of_field_gives_the_rays_different_origins(monkeypatch, golden):
    # (packets whose rays do not share one origin take the per-ray step: this is that branch and its boundary)
    sc = _soup()
    sc.options.fstop = 1.4
    sc.options.focus_distance = 3.0
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "soup with depth of field")


def test_closed_room_every_ray_hits_so_the_packets_tlim_prunes(monkeypatch, golden):
    sc = _soup(n_tris=2048, room=True)
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "room around 2048 triangles")


def test_scene_far_from_the_worlds_origin(monkeypatch, golden):
    # the soup and its camera moved by (1000, -2000, 500): the error term of the bound grows with |a| + |o|, the bound itself does not
    sc = _soup()
    shift = np.array([1000.0, -2000.0, 500.0])
    for me in sc.meshes:
        me.world = scenes._translate(*shift)
    vm = np.array(sc.options.view_matrix, dtype=np.float64)
    vm[:3, 3] += shift
    sc.options.view_matrix = vm.astype(np.float32)
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "soup moved by (1000, -2000, 500)")


def test_passes_of_a_batch_with_different_cameras(monkeypatch, golden):
    # every lane reads its own pass's parameters (the kernel's other instantiation); origins differ inside a packet (the per-ray step)
    # in the frame's middle passes only where the cameras stand apart
    sc = _soup()
    base = np.array(sc.options.view_matrix, dtype=np.float64)
    params = []
    for s in range(32):
        o = copy.copy(sc.options)
        vm = base.copy()
        vm[:3, 3] += 0.02 * np.array([s % 3 - 1, (s // 3) % 3 - 1, s % 2])
        o.view_matrix = vm.astype(np.float32)
        o.focal_length = 35.0 + 3.0 * (s % 5)
        o.fstop = host.FSTOP_DISABLED if s % 4 else 2.0
        params.append(o.pass_params(s))
    _same_frame_four_ways(monkeypatch, golden, sc, params, "a batch of 32 cameras")


@pytest.mark.parametrize("n_tris", [0, 1, 4])
def test_root_leaf_and_empty_scenes(monkeypatch, golden, n_tris):
    sc = _soup(n_tris=max(n_tris, 1), width=40, height=24)
    if n_tris == 0:
        sc.meshes = []
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 16), f"{n_tris} triangles")


def test_camera_in_the_plane_of_a_large_quad(monkeypatch, golden):
    # a quad in y = 0 seen from inside that plane along -z: the middle of the frame has |d.y| down to 0 (safeInv's clamp: those packets
    # take the per-ray step), the node boxes are flat in y
    sc = _soup(n_tris=64, width=32, height=32)
    p, n, i = scenes._merge([scenes._quad((-40.0, 0.0, 4.0), (40.0, 0.0, 4.0), (40.0, 0.0, -80.0), (-40.0, 0.0, -80.0))])
    sc.meshes.append(scenes.MeshData(p, n, i, material_id=0))
    _look(sc, (0.0, 0.0, 3.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    _same_frame_four_ways(monkeypatch, golden, sc, _passes(sc, 32), "camera in the plane of a quad")


def test_pprobe_makes_the_probe_walk_with_the_interval_step(monkeypatch, golden):
    # measurement only: packet_union under pprobe=1 is what the interval step enters per child a ray's own test enters; it can only be
    # more than the per-ray walk's (a superset at every node), and on a fog of small triangles it is strictly more
    sc = _soup()
    union = {}
    for pprobe in (0, 1):
        monkeypatch.setenv("HR_TUNE", f"pprobe={pprobe}")  # (packets=2, the default: the selector probes)
        g = core.create_engine()
        sc.apply(g, lut=golden["multiscatter_lut"], tables=host_tables(sc))
        for s in range(3 * g.pass_batch(sc.options.max_ray_depth) + 1):  # (the probe of the first batch has reported by the third)
            g.render_pass(sc.options.pass_params(s))
        union[pprobe] = g.kernel_times()["camera_packets"][1]
        g.close()
    print("packet_union: pprobe=0", union[0], "pprobe=1", union[1])
    assert union[0] > 1.0 and union[1] > union[0], union


def test_the_selector_chooses_the_step_by_the_probes_looseness(monkeypatch, golden, capfd):
    # the probe walks both ways and reports F = children the interval step enters / children the per-ray step enters; the interval step
    # is used while F < pstepf / 100.  With a threshold nothing can meet the per-ray step is chosen; the frame is the oracle's either way
    sc = _soup()
    lut = golden["multiscatter_lut"]
    monkeypatch.setenv("HR_DEBUG_PIPE", "1")
    o = oracle_lib.engine()
    sc.apply(o, lut=lut, tables=host_tables(sc))
    for tune, want in (("packets=2,punion=1000,pstepf=150", "on"), ("packets=2,punion=1000,pstepf=100", "off")):
        monkeypatch.setenv("HR_TUNE", tune)
        g = core.create_engine()
        sc.apply(g, lut=lut, tables=host_tables(sc))
        n = 3 * g.pass_batch(sc.options.max_ray_depth) + 1  # (the probe of the first batch has reported by the third)
        for s in range(n):
            g.render_pass(sc.options.pass_params(s))
        frame = g.readback().copy()
        g.close()
        lines = [l for l in capfd.readouterr().err.splitlines() if "interval step F" in l]
        assert lines, tune
        f = float(lines[0].split("interval step F")[1].split()[0])
        assert 1.0 < f < 1.5 and lines[0].rstrip().endswith("-> " + want), (tune, lines[0])
        o.clear()
        for s in range(n):
            o.render_pass(sc.options.pass_params(s))
        assert frame.tobytes() == o.readback().tobytes(), tune
    o.close()
