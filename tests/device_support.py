"""What the GPU tests of the post-process features share: the bit-exact comparison, the host-made sample tables, engines with a scene
applied and passes rendered, and the camera moves.  (`same` needs no GPU: tests/test_support.py pins it.)"""
import numpy as np

import oracle_lib
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise
from synthetic_frames import rot_y, translate

F = np.float32
BOTH = ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS

_TABLE_CACHE = {}


def host_tables(sc):
    """Sample tables generated ONCE on the host (by the oracle's generators, themselves pinned to the
    reference's Random.h) and uploaded to both engines, as PassGenerator does with its uniform blocks."""
    key = (sc.options.sample_mode, sc.options.bokeh_shape, sc.options.max_render_passes, sc.width, sc.height)
    if key not in _TABLE_CACHE:
        o = oracle_lib.engine()
        P = sc.options.max_render_passes
        seq = np.stack([o.qmc_generate(sc.options.sample_mode, s, P) for s in range(16)])
        ap = np.stack([o.qmc_generate(ffi.HR_SAMPLE_SOBOL, s, P, radial=True) for s in range(16)])
        off = o.qmc_generate(ffi.HR_SAMPLE_SOBOL, 0, sc.width * sc.height)
        o.close()
        _TABLE_CACHE[key] = (seq, ap, off)
    return _TABLE_CACHE[key]


def same(a, b, what):
    """a and b (H x W or H x W x C, any dtype) have one shape, one dtype and the same bytes: -0.0 is not +0.0, a NaN equals its own payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.tobytes() != b.tobytes():
        pixel_bytes = lambda v: v.reshape(v.shape[0], v.shape[1], -1).view(np.uint8)
        bad = (pixel_bytes(a) != pixel_bytes(b)).any(axis=-1)
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"{what}: {int(bad.sum())} pixels differ, first at (x={xs[0]}, y={ys[0]}): {a[ys[0], xs[0]]} vs {b[ys[0], xs[0]]}")


def device_engine(sc, golden, aovs=BOTH, **kw):
    """an engine with the scene, the golden LUT and the host's sample tables: what the CPU oracle can be given too"""
    eng = core.create_engine(**kw)
    sc.apply(eng, lut=golden["multiscatter_lut"], tables=host_tables(sc))
    if aovs:
        eng.set_aovs(aovs)
    return eng


def render(eng, pps):
    for pp in pps:
        eng.render_pass(pp)


def render_passes(eng, sc, passes, **kw):
    """the passes of these indices, each with the fields of `kw` set on its parameters"""
    for s in passes:
        p = sc.options.pass_params(s)
        for k, v in kw.items():
            setattr(p, k, v)
        eng.render_pass(p)


def engine_with_passes(sc, passes, mask=BOTH):
    eng = core.create_engine()
    sc.apply(eng)
    if mask:
        eng.set_aovs(mask)
    render_passes(eng, sc, passes)
    return eng


def truth(mk):
    """the mean of passes 64 .. 1087 of the scene mk() makes"""
    eng = engine_with_passes(mk(), range(64, 64 + 1024), mask=0)
    f = eng.readback()
    eng.close()
    return f[..., :3] / f[..., 3:4]


def denoise_params(iterations=5, kernel=ffi.HR_DENOISE_KERNEL_AUTO, normal_power=7, sigma_l=4.0, sigma_z=4.0):
    p = denoise.default_params()
    p.iterations, p.kernel, p.normal_power, p.sigma_l, p.sigma_z = iterations, kernel, normal_power, sigma_l, sigma_z
    return p


def orbit(options, dphi):
    """the view matrix after an orbit by dphi about the world's y axis through the focus point"""
    v = np.asarray(options.view_matrix, np.float64)
    target = v[:3, 3] - v[:3, 2] * options.focus_distance
    return (translate(*target) @ rot_y(dphi) @ translate(*-target) @ v).astype(F)


def dolly(options, share):
    v = np.asarray(options.view_matrix, np.float64)
    return (translate(*(-v[:3, 2] * options.focus_distance * share)) @ v).astype(F)
