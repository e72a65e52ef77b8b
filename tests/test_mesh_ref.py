"""The arithmetic of mesh preparation without a GPU: heatray_amd/csrc/hr_mesh.h compiled for the CPU (tests/host/mesh_cpu.cpp, plain
and once more under AddressSanitizer + UBSan) against its numpy restatement in heatray_amd.meshprep, byte for byte, and properties of
the reference alone on meshes whose answers are known (include/hrcore_mesh.h is the contract).  tests/test_gpu_mesh.py holds the device
to the same reference."""
import numpy as np
import pytest

import cpu_header
from heatray_amd import _ffi as ffi
from heatray_amd import meshprep, scenes
from mesh_cases import BOTH, F, WEIGHTS, cube24, fin, grid

U32 = np.uint32


def _bits(a):
    return np.ascontiguousarray(a, F).view(U32)


def _same(got, want, what):
    """float32 arrays of one shape with the same bits"""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((_bits(got) != _bits(want)).reshape(len(got), -1).any(axis=1))[0]
    assert not len(bad), f"{what}: {len(bad)} records differ, first {bad[0]}: {got[bad[0]]} vs {want[bad[0]]}"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cpu(request, tmp_path_factory):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    exe = cpu_header.build("mesh", tmp_path_factory.mktemp("mesh_" + request.param), flags=flags)

    def run(op, records, out_words, weight=0):
        records = np.ascontiguousarray(records, F)
        raw = cpu_header.run(exe, np.array([op, weight, len(records), 0], np.int32).tobytes() + records.tobytes())
        return np.frombuffer(raw, F).reshape(len(records), out_words)
    return run


def _triangles(seed=5):
    """records of op 0: random triangles, slivers, zero-area ones, huge ones whose l2 overflows, tiny ones whose l2 underflows, with
    random, zero, mirrored and NaN uvs"""
    rng = np.random.default_rng(seed)
    n = 400
    p = rng.normal(size=(n, 3, 3)).astype(F)
    p[50:100, 2] = p[50:100, 0] + (p[50:100, 1] - p[50:100, 0]) * F(0.5) + rng.normal(size=(50, 3)).astype(F) * F(1e-6)  # slivers
    p[100:120, 2] = p[100:120, 1]            # two corners coincide
    p[120:140, 1] = p[120:140, 0] + F(1.0)   # collinear: p2 on the line too
    p[120:140, 2] = p[120:140, 0] + F(2.0)
    p[140:170] *= F(1e19)                    # l2 overflows
    p[170:200] *= F(1e-12)                   # l2 underflows
    p[200:230] *= F(3e5)
    uv = rng.uniform(-2, 2, size=(n, 3, 2)).astype(F)
    uv[::7] = 0                              # zero uvs
    uv[1::7, :, 0] *= F(-1.0)                # mirrored
    uv[2::7, 1] = np.nan                     # NaN
    uv[3::7, 2] = uv[3::7, 1]                # det = 0
    return np.concatenate([p.reshape(n, 9), uv.reshape(n, 6)], axis=1)


@pytest.mark.parametrize("weight", WEIGHTS)
def test_face_functions_equal_the_numpy_reference_byte_for_byte(cpu, weight):
    rec = _triangles()
    out = cpu(0, rec, 22, weight)
    p, uv = rec[:, :9].reshape(-1, 3, 3), rec[:, 9:].reshape(-1, 3, 2)
    face, e1, e2, u, w = meshprep.face_terms(p[:, 0], p[:, 1], p[:, 2], weight)
    ok, Tn, Bn = meshprep.face_tangents(e1, e2, uv[:, 0], uv[:, 1], uv[:, 2])
    ok = ok & face
    Tn, Bn = np.where(ok[:, None], Tn, F(0)), np.where(ok[:, None], Bn, F(0))
    flags = out[:, 0].view(U32)
    assert (flags == face * 1 + ok * 2).all()
    assert 20 <= (~face).sum() <= 150 and face.sum() > 200 and 50 < (face & ~ok).sum() < 300  # (every class is exercised)
    _same(out[:, 1:4], u, "u")
    _same(out[:, 4:7], w, "w")
    with np.errstate(all="ignore"):
        _same(out[:, 7:16], (u[:, None, :] * w[:, :, None]).reshape(-1, 9), "corner contributions")
    _same(out[:, 16:19], Tn, "unit T")
    _same(out[:, 19:22], Bn, "unit B")
    if weight == ffi.HR_MESH_WEIGHT_ANGLE:  # a triangle's three angles sum to pi
        s = w[face].astype(np.float64).sum(axis=1)
        assert np.abs(s[np.isfinite(s)] - np.pi).max() < 1e-5


def test_atan2_bit_for_bit(cpu):
    rng = np.random.default_rng(11)
    special = []
    for t in (F(0.41421357), F(2.4142137)):  # atan_'s range thresholds and their float neighbours
        special += [np.nextafter(t, F(0)), t, np.nextafter(t, F(10))]
    special += [F(0.0), F(-0.0), F(1.0), F(-1.0), F(1e-30), F(1e30), F(3.4e38), F(1e-45)]
    ys, xs = np.meshgrid(np.array(special + [-v for v in special], F), np.array([F(1.0), F(-1.0), F(0.0), F(-0.0), F(3.0), F(-0.25)], F))
    y = np.concatenate([ys.reshape(-1), rng.normal(size=4000).astype(F), np.array(special, F)])
    x = np.concatenate([xs.reshape(-1), rng.normal(size=4000).astype(F), np.ones(len(special), F)])
    for sy in (1, -1):       # all four quadrants, both zeros for each argument
        for sx in (1, -1):
            yy, xx = (y * F(sy)).astype(F), (x * F(sx)).astype(F)
            got = cpu(1, np.stack([yy, xx], axis=1), 1)[:, 0]
            want = meshprep.atan2_(yy, xx)
            _same(got[:, None], want[:, None], f"atan2_ {sy} {sx}")
            fin_ = np.isfinite(want) & ((yy != 0) | (xx != 0))
            # (a sanity check beside the bits: libm's angle, up to a turn — atan2_(-0, x < 0) is +pi where libm's is -pi, and
            # atan2_(+-0, +-0) is 0 whatever the signs)
            d = np.abs(want[fin_].astype(np.float64) - np.arctan2(yy[fin_].astype(np.float64), xx[fin_].astype(np.float64)))
            assert np.minimum(d, 2 * np.pi - d).max() < 1e-6


def test_finish_functions_equal_the_numpy_reference_byte_for_byte(cpu):
    rng = np.random.default_rng(13)
    n = 300
    G = rng.normal(size=(n, 3)).astype(F)
    G[:40] = 0
    G[40:60] *= F(1e25)   # dot overflows
    G[60:80] *= F(1e-30)  # ... underflows
    G[80:90, 0] = np.nan
    first = rng.integers(0, 1000, n).astype(U32)
    first[::3] = 0xFFFFFFFF
    uf = meshprep.normalize(rng.normal(size=(n, 3)).astype(F))
    out = cpu(2, np.concatenate([G, first.view(F)[:, None], uf], axis=1), 4)
    N, cls = meshprep.finish_normal(G, first, uf)
    _same(out[:, :3], N, "normal")
    assert (out[:, 3].view(U32) == cls).all() and set(cls) == {0, 1, 2}
    # given normals
    out = cpu(4, G, 4)
    have, Ng = meshprep.given_normal(G)
    assert (out[:, 0].view(U32) == have).all() and 0 < have.sum() < n
    _same(out[:, 1:], Ng, "given normal")
    # tangents: own ones, Ta parallel to N or zero (the fallback), every axis of the fallback with its ties, no N at all
    Nn = meshprep.normalize(rng.normal(size=(n, 3)).astype(F))
    Nn[:6] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [F(0.70710678), F(0.70710678), 0], [F(0.57735027)] * 3]
    Ta, Ba = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    Ta[:60] = 0
    Ta[60:90] = Nn[60:90] * F(2.0)
    Ta[90:100, 1] = np.nan
    Ba[::5] = 0
    have = np.ones(n, U32)
    have[100:120] = 0
    out = cpu(3, np.concatenate([have.view(F)[:, None], Nn, Ta, Ba], axis=1), 7)
    t, b, fb = meshprep.finish_tangent(have != 0, Nn, Ta, Ba)
    _same(out[:, :3], t, "tangent")
    _same(out[:, 3:6], b, "bitangent")
    assert (out[:, 6].view(U32) == fb).all() and 60 <= fb.sum() < 120
    assert not t[100:120].any() and not b[100:120].any()


# ---- properties of the reference alone
def test_cube_welded_and_not():
    pos, uv, idx = cube24()
    n, _, _, r = meshprep.reference(pos, idx)
    assert r["weld_groups"] == 8 and r["max_valence"] == 2 and r["degenerate_triangles"] == 0 and r["triangles"] == 12
    for corner in np.unique(pos, axis=0):
        copies = n[(pos == corner).all(axis=1)]
        assert len(copies) == 3 and (copies.view(U32) == copies[0].view(U32)).all()  # identical bits
        assert np.abs(copies[0] - corner / np.sqrt(3)).max() < 1e-6
    n0, _, _, r0 = meshprep.reference(pos, idx, params=meshprep.params(weld=0))
    assert r0["weld_groups"] == 24
    axes = np.sign(pos) * (np.arange(24)[:, None] // 8 == np.arange(3)[None, :])  # faces come axis by axis, 8 vertices each
    assert np.abs(n0 - axes).max() < 1e-6


@pytest.fixture(scope="module")
def sphere():
    p, _, uv, idx = scenes.uv_sphere(50, 50, 1)
    return p, uv, idx, meshprep.reference(p, idx, uvs=uv, params=meshprep.params(want=BOTH))


def test_sphere_normals_agree_with_every_incident_face(sphere):
    p, uv, idx, (n, t, b, r) = sphere
    tri = meshprep.triangles(idx)
    face, _, _, u, _ = meshprep.face_terms(p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]], 0)
    assert r["degenerate_triangles"] == 0 == (~face).sum()
    d = np.einsum("tkc,tc->tk", n[tri].astype(np.float64), u.astype(np.float64))
    print(f"uv_sphere(50, 50): min dot(normal, incident face u) = {d.min():.4f}")
    assert d.min() > 0
    # the vertices no index names: the last column's two poles.  The top pole's copies share one position (sin(0) = 0) and weld, so
    # the unnamed one takes its group's normal; the bottom pole's do not (sin(float(pi)) is not 0): that one is unreferenced.  Without
    # the weld the unreferenced vertices are exactly the unnamed ones
    named = np.zeros(len(p), bool)
    named[idx] = True
    assert list(np.nonzero(~named)[0]) == [50 * 52, 51 * 52 - 1]
    assert r["unreferenced_vertices"] == 1 and n[50 * 52].any() and not n[51 * 52 - 1].any()
    n0, _, _, r0 = meshprep.reference(p, idx, params=meshprep.params(weld=0))
    assert r0["unreferenced_vertices"] == int((~named).sum()) == 2
    assert not n0[~named].any() and n0[named].any(axis=1).all()
    # the u = 0 and u = 1 columns differ in the last bits: the seam is not welded (include/hrcore_mesh.h, LIMITS)
    vs = 52
    assert (p[:vs] != p[50 * vs:]).any() and np.abs(p[:vs] - p[50 * vs:]).max() < 1e-6
    assert (n[1:vs - 1].view(U32) != n[50 * vs + 1:51 * vs - 1].view(U32)).any()


def test_strip_and_list_of_the_same_triangles_give_identical_bytes():
    pos, uv, sidx, mode = grid(9, 5, strip=True)
    tri = meshprep.triangles(sidx, mode)
    keep = ~((tri[:, 0] == tri[:, 1]) | (tri[:, 1] == tri[:, 2]) | (tri[:, 0] == tri[:, 2]))  # the strip's joins are zero-area triangles
    p = meshprep.params(want=BOTH)
    a = meshprep.reference(pos, sidx, uvs=uv, mode=mode, params=p)
    b = meshprep.reference(pos, tri[keep].reshape(-1), uvs=uv, params=p)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3]["degenerate_triangles"] == int((~keep).sum()) == 4 * 4 and b[3]["degenerate_triangles"] == 0
    assert a[3]["triangles"] == len(tri) and b[3]["triangles"] == 2 * 9 * 5
    # and the list winds like scenes.terrain's: up
    assert (a[0][:, 1] > 0).all()


def test_a_fin_is_cancelled_with_the_documented_fallback():
    pos, uv, idx = fin()
    n, _, _, r = meshprep.reference(pos, idx, params=meshprep.params(weight=ffi.HR_MESH_WEIGHT_AREA))
    assert r["cancelled_vertices"] == 3 and r["unreferenced_vertices"] == 0
    assert (n == np.array([0, 0, 1], F)).all()  # the u of corner 0's triangle, the first one
    # a vertex pair: the fin's far vertices alone, when the shared edge also carries a third face
    pos2 = np.concatenate([pos, [[0, 0, 1]]]).astype(F)
    idx2 = np.concatenate([idx, [0, 1, 3]]).astype(U32)
    n2, _, _, r2 = meshprep.reference(pos2, idx2, params=meshprep.params(weight=ffi.HR_MESH_WEIGHT_AREA))
    assert r2["cancelled_vertices"] == 1 and (n2[2] == np.array([0, 0, 1], F)).all()


def _orthogonality(n, t, b):
    live = n.any(axis=1)
    n, t, b = (a[live].astype(np.float64) for a in (n, t, b))
    return max(np.abs((n * t).sum(axis=1)).max(), np.abs((t * b).sum(axis=1)).max())


def test_frames_are_orthogonal(sphere):
    sc = scenes.terrain(64, 32, width=64, height=36)
    m = sc.meshes[0]
    nt, tt, bt, _ = meshprep.reference(m.positions, m.indices, uvs=m.uvs, params=meshprep.params(want=BOTH))
    worst = max(_orthogonality(nt, tt, bt), _orthogonality(*sphere[3][:3]))
    print(f"orthogonality: max |dot(N, tangent)|, |dot(tangent, bitangent)| over terrain(64, 32) and uv_sphere(50, 50) = {worst:.3e}")
    # measured 8.945e-08 (a few float32 roundings of unit vectors); the cap is 4 x that, rounded up to a power of two: 2^-21
    assert worst < 2.0 ** -21


def _reference64(pos, idx):
    """the contract's normal formulas in float64 (libm's atan2), weld on, weight ANGLE"""
    pos = pos.astype(np.float64)
    tri = idx.reshape(-1, 3)
    p0, p1, p2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    fn = np.cross(p1 - p0, p2 - p0)
    ln = np.linalg.norm(fn, axis=1)
    u = fn / ln[:, None]
    w = np.stack([np.arctan2(ln, ((p1 - p0) * (p2 - p0)).sum(1)), np.arctan2(ln, ((p2 - p1) * (p0 - p1)).sum(1)),
                  np.arctan2(ln, ((p0 - p2) * (p1 - p2)).sum(1))], axis=1)
    S = np.zeros_like(pos)
    np.add.at(S, tri.reshape(-1), (u[:, None, :] * w[:, :, None]).reshape(-1, 3))
    return S / np.linalg.norm(S, axis=1, keepdims=True)


def test_normals_are_close_to_float64():
    m = scenes.terrain(64, 32, width=64, height=36).meshes[0]
    n, _, _, r = meshprep.reference(m.positions, m.indices)
    assert r["weld_groups"] == 65 * 33 and r["max_valence"] == 6
    n64 = _reference64(m.positions, m.indices)
    ang = np.arccos(np.clip((n.astype(np.float64) * n64).sum(axis=1), -1, 1))
    cr = np.linalg.norm(np.cross(n.astype(np.float64), n64), axis=1)  # (arccos is blind below 1e-8: the sine is not)
    print(f"terrain(64, 32): max angle between the float32 and float64 normals = {cr.max():.3e} rad (arccos: {ang.max():.3e})")
    # measured 1.465e-07 rad: sums of at most 6 terms and the polynomial atan_; the cap is 4 x that, rounded up to a power of two: 2^-20
    assert cr.max() < 2.0 ** -20


def test_default_params_and_the_parameter_check():
    p = meshprep.default_params()
    assert (p.weight, p.weld, p.want, list(p.reserved)) == (0, 1, 1, [0] * 5)
    pos, uv, idx = fin()
    bad = [meshprep.params(weight=3), meshprep.params(weld=2), meshprep.params(want=0), meshprep.params(want=4)]
    r = meshprep.default_params()
    r.reserved[2] = 1
    for q in bad + [r]:
        with pytest.raises(ValueError):
            meshprep.reference(pos, idx, params=q)
    with pytest.raises(ValueError):
        meshprep.reference(pos, idx, params=meshprep.params(want=BOTH))  # no uvs
    with pytest.raises(ValueError):
        meshprep.reference(pos, idx, uvs=uv, params=meshprep.params(want=2))  # no normals
    with pytest.raises(ValueError):
        meshprep.reference(pos, np.array([0, 1, 3], U32))
