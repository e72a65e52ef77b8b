"""Context groups (include/hrcore_group.h) on the GPU: one frame rendered by N member contexts behind one handle must be the frame a
plain context renders, bit for bit — read-back, display, the device frame and the summed counters — through every per-pass mode,
scene edits, progressive read-backs, the tree cache and the C++ layer.  N members on one device are the one-device emulation of an
N-way split; a group over distinct devices runs where a second one is visible."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from device_support import same
from heatray_amd import _ffi as ffi
from heatray_amd import core, host, scenes, tiles

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "host", "host_layer_test")


def _render(eng, sc, first, count, **kw):
    for s in range(first, first + count):
        p = sc.options.pass_params(s)
        for k, v in kw.items():
            setattr(p, k, v)
        eng.render_pass(p)


def _device_frame(eng):
    """The frame hr_frame_device_ptr hands out, copied to the host after the context's work has completed."""
    ptr = eng.frame_device_ptr()
    eng.synchronize()
    hip = C.CDLL("libamdhip64.so")
    out = np.empty((eng.height, eng.width, 4), np.float32)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return out


def _compare_all(grp, plain, what):
    same(grp.readback(), plain.readback(), what + ": readback")
    for fmt in (ffi.HR_DISPLAY_RGBA8, ffi.HR_DISPLAY_HDR_RGBA32F):
        (gi, gn), (pi, pn) = grp.display(fmt=fmt, with_passes=True), plain.display(fmt=fmt, with_passes=True)
        same(gi, pi, f"{what}: display format {fmt}")
        assert gn == pn, (what, gn, pn)
    same(_device_frame(grp), _device_frame(plain), what + ": frame_device_ptr")
    gs, ps = grp.stats(), plain.stats()
    assert (gs.paths, gs.rays_closest, gs.rays_any, gs.shaded_hits) == (ps.paths, ps.rays_closest, ps.rays_any, ps.shaded_hits), what
    assert grp.passes_resolved() == plain.passes_resolved(), what


SCENES = {"multi_material_200x120": lambda: scenes.multi_material(200, 120, bounces=4),
          "cornell_64x64": lambda: scenes.cornell_box(64, 64, bounces=4)}


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_group_on_one_device_matches_plain_context(n, scene):
    sc = SCENES[scene]()
    plain, grp = core.create_engine(), core.create_group([0] * n)
    info = grp.group_info()
    assert info["n_members"] == n and info["device_ids"] == [0] * n
    for e in (plain, grp):
        sc.apply(e)
        _render(e, sc, 0, 3)
    owned = grp.group_info()["owned_pixels"]
    owner = tiles.owner_map(sc.width, sc.height, n)
    assert owned == [int((owner == i).sum()) for i in range(n)] and sum(owned) == sc.width * sc.height
    if scene == "cornell_64x64" and n == 8:
        assert owned[4:] == [0, 0, 0, 0]  # four tiles: members 4..7 own none
    _compare_all(grp, plain, f"{scene}, {n} members")
    member = [grp.member_stats(i) for i in range(n)]
    assert [m.paths for m in member] == [o * 3 for o in owned]
    grp.close()


def test_group_through_every_per_pass_mode():
    sc = scenes.multi_material(200, 120, bounces=4, textured=True)
    plain, grp = core.create_engine(), core.create_group([0, 0, 0])
    perm = np.random.default_rng(3).permutation(9)
    coords = np.array([(i // 3, i % 3) for i in perm], dtype=np.int32).reshape(3, 3, 2)
    for e in (plain, grp):
        sc.apply(e)
        _render(e, sc, 0, 2, estimator=ffi.HR_ESTIMATOR_ALL_LIGHTS)
        _render(e, sc, 2, 2, texture_lod=ffi.HR_TEXTURE_LOD_CONE)
        _render(e, sc, 4, 2, max_ray_depth=2)                       # a depth change mid-render
        e.set_interactive_blocks(coords)
        for by in range(3):
            for bx in range(3):
                p = sc.options.pass_params(6, current_block_pixel=(bx, by))
                p.interactive_mode, p.block_size[0], p.block_size[1] = 1, 3, 3
                e.render_pass(p)
    _compare_all(grp, plain, "every per-pass mode")


def test_group_scene_edit_mid_render_and_clear():
    sc = scenes.multi_material(200, 120, bounces=4)
    plain, grp = core.create_engine(), core.create_group([0, 0])
    move = scenes._translate(0.05, 0.0, -0.02)
    for e in (plain, grp):
        sc.apply(e)
        _render(e, sc, 0, 2)
        e.set_transform(0, move)                                    # refit on every member
        e.commit()
        assert e.scene_info().refitted == 1
        _render(e, sc, 2, 2)
    _compare_all(grp, plain, "transform edit mid-render")
    for e in (plain, grp):
        e.clear()
        _render(e, sc, 0, 2)
    _compare_all(grp, plain, "after clear")


def test_group_progressive_readback():
    sc = scenes.multi_material(200, 120, bounces=4)
    n = 3
    grp = core.create_group([0] * n)
    sc.apply(grp)
    owner = tiles.owner_map(sc.width, sc.height, n)
    posted = 0
    for _ in range(4):
        _render(grp, sc, posted, 5)
        posted += 5
        img, shown = grp.readback_progressive()
        assert 0 <= shown <= posted
        for i in range(n):
            a = np.unique(img[..., 3][owner == i])
            assert a.size == 1, (i, a)                               # a member's tiles hold one pass count
            assert shown <= a[0] <= posted, (i, a[0], shown, posted)
    grp.flush()
    snap, shown = grp.readback_progressive()
    full = grp.readback()
    assert shown == posted and (full[..., 3] == posted).all()
    same(snap, full, "progressive snapshot after flush")
    img, shown = grp.display(fmt=ffi.HR_DISPLAY_RGBA8 | ffi.HR_DISPLAY_PROGRESSIVE, with_passes=True)
    assert shown == posted
    same(img, grp.display(fmt=ffi.HR_DISPLAY_RGBA8), "progressive display after flush")


def test_group_tree_cache(tmp_path):
    sc = scenes.multi_material(200, 120, bounces=4)
    path = str(tmp_path / "tree.bin")
    first = core.create_group([0, 0, 0])
    first.set_scene_cache(path)
    sc.apply(first)                                                 # member 0 builds and writes the file, the others read it
    assert os.path.exists(path)
    second = core.create_group([0, 0])
    second.set_scene_cache(path)
    sc.apply(second)
    assert second.scene_info().refitted == 2                        # member 0 of the second group read the tree from the file
    plain = core.create_engine()
    sc.apply(plain)
    for e in (first, second, plain):
        _render(e, sc, 0, 2)
    ref = plain.readback()
    same(first.readback(), ref, "first cached group")
    same(second.readback(), ref, "second cached group")


def test_group_unsupported_calls_and_bad_creation():
    sc = scenes.cornell_box(64, 64, bounces=2)
    grp = core.create_group([0, 0])
    sc.apply(grp)
    _render(grp, sc, 0, 1)
    calls = [lambda: grp.kernel_times(), lambda: grp.step_log(), lambda: grp.bind_external_frame(0), lambda: grp.packed_slots(0, 1),
             lambda: grp.pack_owned(1), lambda: grp.unpack(0, 1, 1, 1)]
    for call in calls:
        with pytest.raises(ffi.EngineError, match="status 3"):
            call()
    assert (grp.readback()[..., 3] == 1).all()                      # still usable afterwards
    for bad in ([0, 4096], [-1], [0] * 17):
        with pytest.raises(ffi.EngineError):
            core.create_group(bad)
    lib = core.load_library()
    plain = core.create_engine()
    info = ffi.GroupInfo()
    lib.hr_group_get_info.restype = C.c_int
    assert lib.hr_group_get_info(plain._ctx, C.byref(info)) == 1     # HR_ERR_INVALID on a plain context
    desc = ffi.CtxDesc(0, 1, 2, 32, None, 0, 0)                      # no group inside a tile shard
    out = C.c_void_p()
    lib.hr_ctx_create_group.restype = C.c_int
    assert lib.hr_ctx_create_group(C.byref(desc), None, C.c_int32(0), C.byref(out)) == 1 and not out.value


def test_group_over_distinct_devices():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip(f"one visible device ({torch.cuda.device_count()}): a group over distinct devices needs two or more")
    n = min(torch.cuda.device_count(), 4)
    for name in sorted(SCENES):
        sc = SCENES[name]()
        plain, grp = core.create_engine(), core.create_group(list(range(n)))
        for e in (plain, grp):
            sc.apply(e)
            _render(e, sc, 0, 3)
        _compare_all(grp, plain, f"{name} over devices 0..{n - 1}")


def _host_layer_scene(path):
    # the scene of tests/test_gpu_host_layer.py
    W, H, depth = 96, 54, 6
    sp, sn, suv, si = scenes.uv_sphere(16, 16, 1.0)
    pp, pn, puv, pi = scenes.plane_strip(15, 15)
    meshes = [(1, 0, scenes._translate(0, -1.5, 0), pp, pn, puv, pi),
              (0, 1, scenes._translate(-0.9, -0.5, -0.8), sp, sn, suv, si),
              (0, 2, scenes._translate(1.2, -0.5, 0.8), sp, sn, suv, si),
              (0, 3, scenes._translate(0.2, -1.0, 1.8), (sp * np.float32(0.5)).astype(np.float32), sn, suv, si)]
    view = host.orbit_view_matrix(8.0, 0.5, 0.35, target=(0, -0.5, 0))
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", W, H, depth, len(meshes)))
        f.write(np.asarray(view, np.float32).T.tobytes())
        for strip, mat, xf, p, n, uv, idx in meshes:
            f.write(struct.pack("<2i", strip, mat))
            f.write(np.asarray(xf, np.float32).T.tobytes())
            for arr, dt in ((p, np.float32), (n, np.float32), (uv, np.float32), (idx, np.int32)):
                a = np.ascontiguousarray(arr, dtype=dt).reshape(-1)
                f.write(struct.pack("<i", a.size))
                f.write(a.tobytes())
    return W, H


def test_cpp_layer_with_heatray_devices(tmp_path):
    assert os.path.exists(EXE), "tests/host/host_layer_test not built (python -c 'import __graft_entry__ as g; g.build()')"
    W, H = _host_layer_scene(tmp_path / "scene.bin")
    passes = 16
    outs = {}
    for name, extra in (("plain", {}), ("group", {"HEATRAY_DEVICES": "0,0,0"})):
        d = tmp_path / name
        d.mkdir()
        env = {k: v for k, v in os.environ.items() if k != "HEATRAY_DEVICES"}
        env.update(extra)
        out = subprocess.run([EXE, str(tmp_path / "scene.bin"), str(d), str(passes)], capture_output=True, text=True, env=env, timeout=240)
        assert out.returncode == 0, out.stdout + out.stderr
        outs[name] = (out.stdout, np.fromfile(d / "pixels.bin", dtype=np.float32).reshape(H, W, 4))
    assert "context group" not in outs["plain"][0]
    assert "PassGenerator: context group of 3 members on devices 0,0,0" in outs["group"][0]
    assert (outs["plain"][1][..., 3] == passes).all()
    same(outs["group"][1], outs["plain"][1], "C++ layer, HEATRAY_DEVICES=0,0,0")
