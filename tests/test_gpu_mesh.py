"""Mesh preparation on the device (include/hrcore_mesh.h) against heatray_amd.meshprep.reference: all three arrays byte for byte and all
eight counters, on the smallest meshes, at every tile boundary of the implementation, on inputs as callers hold them, on degenerate
UVs; determinism across calls, contexts and context groups; a frame rendered from prepared meshes; the call as a pure side call; and
every refusal with its message."""
import ctypes as C

import numpy as np
import pytest

from device_support import same
from heatray_amd import _ffi as ffi
from heatray_amd import core, meshprep, scenes
from mesh_cases import BOTH, F, WEIGHTS, check, cube24, fan, fin, given_normals, grid

pytestmark = pytest.mark.gpu

U32 = np.uint32
# heatray_amd/csrc/hr_mesh.hip: lanes per workgroup of the per-triangle / per-vertex / per-group kernels (kMsBlock), keys per sort tile
# (kMsSortTile), values the scan takes per round (kMsScanBlock * kMsScanPer); a sort tile gives the scan 256 values
TILES = {"block": 256, "sort": 2048, "scan": 1024 * 4}


@pytest.fixture(scope="module")
def eng():
    e = core.create_engine()
    yield e
    e.close()


def run(e, pos, idx, uvs=None, normals=None, mode=ffi.HR_TRIANGLES, params=None, what=""):
    """prepare_mesh on the device, held to the reference; returns the device's tuple"""
    got = e.prepare_mesh(pos, idx, uvs=uvs, normals=normals, mode=mode, params=params, with_result=True)
    check(got, pos, idx, uvs=uvs, normals=normals, mode=mode, params=params, what=what)
    return got


def every_setting(e, pos, uv, idx, mode=ffi.HR_TRIANGLES, what=""):
    """all three weights, weld on and off, want = 1, 2 (against given normals) and 3; returns the results by (weight, weld, want)"""
    given = given_normals(pos)
    out = {}
    for weight in WEIGHTS:
        for weld in (1, 0):
            for want in (1, 2, 3):
                p = meshprep.params(weight, weld, want)
                out[weight, weld, want] = run(e, pos, idx, uvs=uv if want & 2 else None, normals=given if want == 2 else None, mode=mode, params=p,
                                              what=f"{what} weight={weight} weld={weld} want={want}")
    return out


# ---- 1. the smallest meshes
def test_one_triangle_and_two_sharing_an_edge(eng):
    pos = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.25], [1, 1, -0.5]], F)
    uv = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], F)
    r = every_setting(eng, pos[:3], uv[:3], np.array([0, 1, 2], U32), what="one triangle")
    assert r[0, 1, 3][3] == dict(triangles=1, degenerate_triangles=0, degenerate_uv_triangles=0, weld_groups=3, unreferenced_vertices=0, cancelled_vertices=0,
                                 fallback_tangents=0, max_valence=1)
    r = every_setting(eng, pos, uv, np.array([0, 1, 2, 2, 1, 3], U32), what="two triangles")
    assert r[0, 1, 3][3]["max_valence"] == 2 and r[0, 0, 1][3]["weld_groups"] == 4


def test_degenerate_triangles_alone(eng):
    pos = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5]], F)
    uv = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], F)
    r = every_setting(eng, pos[:3], uv[:3], np.array([0, 1, 2], U32), what="one degenerate triangle")
    assert r[0, 1, 3][3]["degenerate_triangles"] == 1 and r[0, 1, 3][3]["unreferenced_vertices"] == 3 and not r[0, 1, 3][0].any()
    r = every_setting(eng, pos, uv, np.array([0, 1, 2, 0, 0, 3, 1, 3, 3, 2, 1, 0], U32), what="all degenerate")
    assert r[0, 1, 3][3]["degenerate_triangles"] == 4 == r[0, 1, 3][3]["triangles"] and r[0, 1, 3][3]["unreferenced_vertices"] == 4


def test_a_vertex_nobody_names_and_a_fan_longer_than_a_wave(eng):
    pos, uv, idx = fan(70)
    pos, uv = np.concatenate([pos, [[9, 9, 9]]]).astype(F), np.concatenate([uv, [[0, 0]]]).astype(F)
    r = every_setting(eng, pos, uv, idx, what="fan of 70")
    res = r[0, 1, 3][3]
    assert res["max_valence"] == 70 and res["unreferenced_vertices"] == 1 and res["weld_groups"] == 72 and not r[0, 1, 3][0][71].any()
    assert r[0, 1, 3][0][0, 1] > 0.9  # the cone's tip points up


def test_no_triangles_at_all(eng):
    pos = np.array([[0, 0, 0], [1, 0, 0]], F)
    for idx in (np.zeros(0, U32), np.array([0, 1], U32)):
        got = run(eng, pos, idx, uvs=pos[:, :2], params=meshprep.params(want=BOTH), what="no triangles")
        assert got[3]["triangles"] == 0 and got[3]["unreferenced_vertices"] == 2 and got[3]["max_valence"] == 0


# ---- 2. the boundaries of the implementation
def random_mesh(V, T, seed):
    """V vertices and T triangles with random indices: exact counts, coincident positions to weld, and coordinates from a small set (both
    zeros among them) so that every one of the weld's three sorts has ties to keep in order"""
    rng = np.random.default_rng(seed)
    base = rng.choice(np.array([-1.0, -0.5, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5], F), size=(V, 3)) + (rng.integers(0, 3, (V, 1)) == 0) * rng.normal(size=(V, 3)).astype(F)
    pos = base[rng.integers(0, max(1, (3 * V) // 4), V)].astype(F)
    uv = rng.uniform(0, 1, (V, 2)).astype(F)
    return pos, uv, rng.integers(0, V, 3 * T).astype(U32)


B, S, SC = TILES["block"], TILES["sort"], TILES["scan"]
BOUNDARY = [
    # (vertices, triangles): vertex counts one below, at and one above each tile; triangle counts likewise for the 256-lane kernels, and
    # corner counts 3 T as near below and above 2048 and 4096 as a multiple of three gets, and either side of the 16 sort tiles whose
    # 16 * 256 histogram values are exactly one round of the scan
    (B - 1, B // 3), (B, B - 1), (B + 1, B), (S - 1, B + 1), (S, S // 3), (S + 1, S // 3 + 1), (SC - 1, SC // 3), (SC, SC // 3 + 1),
    (SC + 1, (16 * S) // 3), (300, (16 * S) // 3 + 1), (16 * S - 1, 5), (16 * S, 6), (16 * S + 1, 7),
]


@pytest.mark.parametrize("V, T", BOUNDARY, ids=lambda v: str(v))
def test_tile_boundaries(eng, V, T):
    pos, uv, idx = random_mesh(V, T, seed=V * 7 + T)
    got = run(eng, pos, idx, uvs=uv, params=meshprep.params(want=BOTH), what=f"V={V} T={T}")
    assert got[3]["weld_groups"] < V and got[3]["triangles"] == T
    run(eng, pos, idx, params=meshprep.params(weld=0, weight=ffi.HR_MESH_WEIGHT_AREA), what=f"V={V} T={T} unwelded")


@pytest.fixture(scope="module")
def terrain256():
    m = scenes.terrain(256, 256, width=64, height=36).meshes[0]
    p = meshprep.params(want=BOTH)
    return m, p, meshprep.reference(m.positions, m.indices, uvs=m.uvs, params=p)


def test_terrain_with_a_live_third_key_byte(eng, terrain256):
    m, p, want = terrain256
    assert len(m.positions) == 66049 and m.indices.size == 3 * 131072
    got = eng.prepare_mesh(m.positions, m.indices, uvs=m.uvs, params=p, with_result=True)
    for name, g, w in zip(("normals", "tangents", "bitangents"), got[:3], want[:3]):
        same(g.reshape(-1, 1, 3), w.reshape(-1, 1, 3), "terrain(256, 256): " + name)
    assert got[3] == want[3] and got[3]["max_valence"] == 6 and got[3]["weld_groups"] == 66049 and got[3]["degenerate_triangles"] == 0
    assert eng.mesh_last() == got[3]


def test_twenty_vertices_skip_three_digit_passes(eng):
    pos, uv, idx, _ = grid(4, 3)
    assert len(pos) == 20
    every_setting(eng, pos, uv, idx, what="20 vertices")


# ---- 3. inputs as callers hold them
def test_interleaved_and_oddly_strided_buffers(eng):
    pos, uv, idx, _ = grid(13, 7)
    V = len(pos)
    p = meshprep.params(want=BOTH)
    want = meshprep.reference(pos, idx, uvs=uv, params=p)
    buf = np.zeros((V, 5), F)  # one interleaved buffer: a stride of 20 bytes for both attributes
    buf[:, :3], buf[:, 3:] = pos, uv
    got = eng.prepare_mesh(buf[:, :3], idx, uvs=buf[:, 3:], params=p, with_result=True)
    assert buf[:, :3].strides == (20, 4)
    for g, w in zip(got[:3], want[:3]):
        same(g.reshape(-1, 1, 3), w.reshape(-1, 1, 3), "interleaved")
    assert got[3] == want[3]
    # strides that are no multiple of four: 13 bytes between positions, 11 between uvs, 17 between given normals
    def odd(a, stride):
        raw = np.zeros(len(a) * stride + 16, np.uint8)
        view = np.ndarray(a.shape, F, buffer=raw.data, strides=(stride, 4))
        view[...] = a
        return view
    given = given_normals(pos)
    p2 = meshprep.params(want=2)
    got = eng.prepare_mesh(odd(pos, 13), idx, uvs=odd(uv, 11), normals=odd(given, 17), params=p2, with_result=True)
    check(got, pos, idx, uvs=uv, normals=given, params=p2, what="odd strides")
    got = eng.prepare_mesh(odd(pos, 13), idx, uvs=odd(uv, 11), params=p, with_result=True)
    check(got, pos, idx, uvs=uv, params=p, what="odd strides, both")


def test_strips_and_trailing_indices(eng):
    p, _, uv, idx = scenes.plane_strip(15, 15)
    r = every_setting(eng, p, uv, idx, mode=ffi.HR_TRIANGLE_STRIP, what="plane_strip")
    assert (r[0, 1, 1][0] == np.array([0, 1, 0], F)).all()
    pos, uv, sidx, mode = grid(40, 3, strip=True)
    got = run(eng, pos, sidx, uvs=uv, mode=mode, params=meshprep.params(want=BOTH), what="40 x 3 strip")
    assert got[3]["degenerate_triangles"] == 2 * 4 and got[3]["triangles"] == sidx.size - 2
    # 7 indices as a list: two triangles, the trailing index ignored
    pos, uv, idx, _ = grid(2, 1)
    a = run(eng, pos, np.array([0, 3, 4, 0, 4, 1, 5], U32), what="7 indices")
    b = run(eng, pos, np.array([0, 3, 4, 0, 4, 1], U32), what="6 indices")
    assert a[3]["triangles"] == 2 and a[0].tobytes() == b[0].tobytes() and not a[0][5].any()


def test_signed_zeros_weld_and_a_last_bit_seam_does_not(eng):
    pos, uv, idx = cube24()
    pos = (pos * F(0.5) + F(0.5)).astype(F)  # corners at 0 and 1
    pos[::2][pos[::2] == 0] = -0.0              # every other vertex spells its zeros -0
    assert np.signbit(pos).any()
    got = run(eng, pos, idx, uvs=uv, params=meshprep.params(want=BOTH), what="cube with -0")
    assert got[3]["weld_groups"] == 8
    sp, _, suv, si = scenes.uv_sphere(50, 50, 1)
    got = run(eng, sp, si, uvs=suv, params=meshprep.params(want=BOTH), what="uv_sphere")
    vs = 52
    assert (got[0][1:vs - 1].view(U32) != got[0][50 * vs + 1:51 * vs - 1].view(U32)).any()  # the u = 0 / u = 1 seam is not welded
    assert got[3]["weld_groups"] == len(sp) - 50 and got[3]["unreferenced_vertices"] == 1  # (only the top pole's 51 copies coincide)


# ---- 4. degenerate uvs
def test_zero_mirrored_and_nan_uvs(eng):
    pos, uv, idx, _ = grid(12, 9)
    p = meshprep.params(want=BOTH)
    got = run(eng, pos, idx, uvs=np.zeros_like(uv), params=p, what="zero uvs")
    assert got[3]["degenerate_uv_triangles"] == got[3]["triangles"] and got[3]["fallback_tangents"] == len(pos)
    plain = run(eng, pos, idx, uvs=uv, params=p, what="plain uvs")
    mirrored = run(eng, pos, idx, uvs=uv * np.array([-1, 1], F), params=p, what="mirrored uvs")
    assert mirrored[3]["fallback_tangents"] == 0
    # the mirror turns the tangent round and with it cross(N, tangent); the bitangent stays on the side the v direction is on
    assert ((plain[1] * mirrored[1]).sum(axis=1) < -0.99).all() and ((plain[2] * mirrored[2]).sum(axis=1) > 0.99).all()
    bad = uv.copy()
    bad[::5, 0] = np.nan
    got = run(eng, pos, idx, uvs=bad, params=p, what="NaN uvs")
    assert 0 < got[3]["degenerate_uv_triangles"] < got[3]["triangles"]
    assert np.isfinite(got[1]).all() and np.isfinite(got[2]).all()


# ---- 5. determinism
def test_the_same_bytes_on_every_call_context_and_group(eng, terrain256):
    m, p, want = terrain256
    def prepared(e):
        return e.prepare_mesh(m.positions, m.indices, uvs=m.uvs, params=p, with_result=True)
    first = prepared(eng)
    engines = [eng, core.create_engine(), core.create_group(device_ids=[0, 0]), core.create_group(device_ids=[0, 0, 0])]
    for e in engines:
        got = prepared(e)
        for a, b, w in zip(got[:3], first[:3], want[:3]):
            assert a.tobytes() == b.tobytes() == w.tobytes()
        assert got[3] == first[3] == e.mesh_last()
    for e in engines[1:]:
        e.close()


# ---- 6. end to end
class _Preparing:
    """an engine whose add_mesh drops the normals, tangents and bitangents it is given and has the device make them"""

    def __init__(self, e):
        self._e = e

    def __getattr__(self, name):
        return getattr(self._e, name)

    def add_mesh(self, positions, normals, indices, uvs=None, tangents=None, bitangents=None, **kw):
        return self._e.add_mesh_prepared(positions, indices, uvs=uvs, **kw)


def _normal_mapped_scene():
    sc = scenes.multi_material(width=64, height=36, passes=2, textured=True)
    rng = np.random.default_rng(9)
    bumps = np.concatenate([rng.uniform(0.2, 0.8, (16, 16, 2)), np.ones((16, 16, 1))], axis=-1).astype(F)
    sc.textures.append((bumps, ffi.HR_WRAP_REPEAT, ffi.HR_FILTER_LINEAR))
    for mid in (0, 1, 3):  # the ground plane and the two opaque spheres read the normal map through their tangent frames
        sc.materials[mid].normalmap = len(sc.textures) - 1
        sc.materials[mid].flags |= ffi.HR_MF_HAS_NORMALMAP
    return sc


def _frame(sc, e):
    sc.apply(e)
    for s in range(2):
        e.render_pass(sc.options.pass_params(s))
    return e.readback()


def test_a_frame_from_prepared_meshes(golden):
    sc = _normal_mapped_scene()
    p = meshprep.params(want=BOTH)
    mapped = (0, 1, 3)  # the meshes of the three normal-mapped materials: the ground plane and the two opaque spheres
    scenes_ = [sc, _normal_mapped_scene()] + [_normal_mapped_scene() for _ in mapped]
    for k, m in enumerate(scenes_[1].meshes):
        m.normals, m.tangents, m.bitangents, _ = meshprep.reference(m.positions, m.indices, uvs=m.uvs, mode=m.mode, params=p)
        for z, which in zip(scenes_[2:], mapped):  # the same arrays, with zero tangents on one of the three
            zm = z.meshes[k]
            zm.normals = m.normals
            zm.tangents, zm.bitangents = (np.zeros_like(m.tangents), np.zeros_like(m.bitangents)) if k == which else (m.tangents, m.bitangents)
    frames = []
    for scene, wrap in zip(scenes_, [_Preparing] + [lambda e: e] * 4):
        e = core.create_engine()
        frames.append(_frame(scene, wrap(e)))
        e.close()
    same(frames[0], frames[1], "add_mesh_prepared against the reference's arrays through add_mesh")
    assert (frames[0][..., 3] == 2.0).all()
    for f, which in zip(frames[2:], mapped):  # the tangent frames are read: each mesh shades differently without them
        assert (frames[0][..., :3] != f[..., :3]).any(), which


# ---- 7. a pure side call
def test_prepare_between_passes_changes_nothing():
    sc = scenes.multi_material(width=64, height=36, passes=4, textured=True)
    pos, uv, idx, _ = grid(30, 20)
    frames = []
    for interrupt in (False, True):
        e = core.create_engine()
        sc.apply(e)
        info = bytes(e.scene_info())
        for s in range(4):
            if interrupt and s == 2:
                run(e, pos, idx, uvs=uv, params=meshprep.params(want=BOTH), what="between passes")
                assert bytes(e.scene_info()) == info
            e.render_pass(sc.options.pass_params(s))
        frames.append(e.readback())
        assert bytes(e.scene_info()) == info
        e.close()
    same(frames[0], frames[1], "four passes with a prepare_mesh in their middle")


# ---- 8. refusals
def _desc(pos, idx, uv=None, nrm=None, mode=ffi.HR_TRIANGLES):
    d = ffi.MeshDesc()
    d.positions, d.uvs, d.normals = ffi._ptr(pos), ffi._ptr(uv), ffi._ptr(nrm)
    d.n_vertices = len(pos)
    d.indices, d.n_indices, d.mode = ffi._ptr(idx, ffi.u32p), idx.size, mode
    return d


def test_every_refusal_names_its_cause_and_leaves_the_context_usable(eng):
    pos, uv, idx, _ = grid(3, 2)
    nrm = given_normals(pos)
    out = [np.empty((len(pos), 3), F) for _ in range(3)]
    last = run(eng, pos, idx, uvs=uv, params=meshprep.params(want=BOTH), what="before the refusals")[3]

    def refused(match, desc=None, params=None, outs=(0, 1, 2), **fields):
        d = desc if desc is not None else _desc(pos, idx, uv, nrm)
        for k, v in fields.items():
            setattr(d, k, v)
        ptrs = [ffi._ptr(out[i]) if i in outs else ffi.f32p() for i in range(3)]
        with pytest.raises(ffi.EngineError, match=match):
            eng._feature_call("mesh", "mesh_prepare", C.byref(d) if d != "null" else None, C.byref(params) if params is not None else None, *ptrs, None)
        # the context stays usable, and the last successful result stays the last
        good = run(eng, pos, idx, what="after a refusal")
        assert eng.mesh_last() == good[3]

    both = meshprep.params(want=BOTH)
    refused("null desc", desc="null")
    refused("null positions", positions=ffi.f32p())
    refused("null indices", indices=ffi.u32p())
    refused("normals_out is null", outs=(1, 2))
    refused("tangents_out is null", params=both, outs=(0, 2))
    refused("bitangents_out is null", params=both, outs=(0, 1))
    refused("n_vertices = 0 must be positive", n_vertices=0)
    refused("n_indices = -3 is negative", n_indices=-3)
    refused("unsupported draw mode", mode=2)
    refused("unknown weight 3", params=meshprep.params(weight=3))
    refused("unknown want 4", params=meshprep.params(want=4))
    refused("want = 0 asks for nothing", params=meshprep.params(want=0))
    refused("weld = 2 is neither 0 nor 1", params=meshprep.params(weld=2))
    r = meshprep.default_params()
    r.reserved[4] = 1
    refused(r"reserved\[4\] must be 0", params=r)
    refused("index out of range", desc=_desc(pos, np.array([0, 1, len(pos)], U32)))
    refused("attribute stride smaller than the attribute", position_stride=8)
    refused("attribute stride smaller than the attribute", params=both, uv_stride=4)
    refused("attribute stride smaller than the attribute", params=meshprep.params(want=2), normal_stride=-12)
    for bad in (np.nan, np.inf, 3.2e37):
        q = pos.copy()
        q[5, 1] = bad
        refused("vertex positions must be finite", desc=_desc(q, idx, uv, nrm))
    refused("tangents need uvs", desc=_desc(pos, idx, None, nrm), params=both)
    refused("tangents need normals", desc=_desc(pos, idx, uv, None), params=meshprep.params(want=2))
    assert last["triangles"] == 12
    # before a context's first success there is no last result
    e = core.create_engine()
    with pytest.raises(ffi.EngineError, match="no mesh has been prepared"):
        e.mesh_last()
    e.close()
