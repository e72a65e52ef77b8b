"""The denoiser's arithmetic without a GPU: heatray_amd/csrc/hr_denoise.h compiled for the CPU (tests/host/denoise_cpu.cpp) against its
numpy restatement heatray_amd.denoise.reference, bit for bit; the numpy exp_ against the oracle's; and properties of the reference
whose answers are exact (include/hrcore_denoise.h is the contract).  tests/test_gpu_denoise.py holds the device to the same reference."""
import ctypes as C

import numpy as np
import pytest

import cpu_header
from device_support import same
from heatray_amd import _ffi as ffi
from heatray_amd import denoise
from synthetic_frames import F, filter_params as params, synthetic


@pytest.fixture(scope="module")
def cpu_filter(tmp_path_factory):
    exe = cpu_header.build("denoise", tmp_path_factory.mktemp("denoise_cpu"))

    def run(frame, planes, p):
        H, W = frame.shape[:2]
        data = [np.array([W, H, p.iterations, p.normal_power], np.int32), np.array([p.sigma_l, p.sigma_z], F)]
        data += [np.ascontiguousarray(a, F) for a in (frame, planes["albedo"], planes["normal_depth"], planes["moments"])]
        return np.frombuffer(cpu_header.run(exe, b"".join(a.tobytes() for a in data)), F).reshape(H, W, 4)
    return run


CASES = [
    # (W, H, passes, hits, holes, iterations, normal_power, sigma_l, sigma_z)
    (67, 41, 4, "partial", False, 5, 7, 4.0, 4.0),
    (67, 41, 4, "partial", True, 6, 7, 4.0, 4.0),
    (67, 41, 16, "partial", True, 3, 2, 1.5, 0.5),
    (1, 1, 4, "all", False, 5, 7, 4.0, 4.0),
    (5, 300, 3, "partial", True, 4, 7, 4.0, 4.0),
    (40, 33, 1, "partial", False, 5, 7, 4.0, 4.0),   # n == 1 everywhere: no variance estimate
    (40, 33, 4, "none", False, 5, 7, 4.0, 4.0),      # hits == 0 everywhere: no surface, no guides
    (40, 33, 4, "all", False, 2, 0, 0.0, 0.0),       # the degenerate parameters
] + [(31, 22, 5, "partial", True, it, 7, 4.0, 4.0) for it in range(0, 7)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_cpu_header_equals_numpy_reference_bit_for_bit(cpu_filter, case):
    W, H, n, hits, holes, it, power, sl, sz = case
    frame, planes = synthetic(W, H, n, seed=W * 1000 + H + it, hits=hits, holes=holes)
    p = params(it, power, sl, sz)
    want = denoise.reference(frame, planes, p)
    assert np.isfinite(want).all()
    same(cpu_filter(frame, planes, p), want, f"case {case}")


def test_numpy_exp_equals_the_oracles_bit_for_bit(oracle_lib):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-100, 100, 100000), [np.inf, -np.inf, np.nan, 87.0, -87.0, 88.0, 0.0, -0.0]]).astype(F)
    fn = oracle_lib.ora_exp
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    want = np.array([fn(float(v)) for v in x], F)
    got = denoise.exp_(x)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    bad = [i for i in bad if not (np.isnan(got[i]) and np.isnan(want[i]))]
    assert not bad, (len(bad), x[bad[:5]], got[bad[:5]], want[bad[:5]])


def _flat_planes(H, W, n, colour, normal=(0.0, 0.0, 1.0), depth=2.0, albedo=0.5):
    """n identical samples per pixel of `colour` on one surface: variance exactly 0"""
    colour = np.broadcast_to(np.asarray(colour, F), (H, W, 3))
    frame = np.concatenate([colour * F(n), np.full((H, W, 1), n, F)], -1).astype(F)
    mom = np.concatenate([colour * colour * F(n), np.full((H, W, 1), n, F)], -1).astype(F)
    alb = np.concatenate([np.full((H, W, 3), albedo * n, F), np.full((H, W, 1), n, F)], -1)
    nd = np.concatenate([np.broadcast_to(np.asarray(normal, F) * F(n), (H, W, 3)), np.full((H, W, 1), depth * n, F)], -1).astype(F)
    return frame, {"albedo": alb, "normal_depth": nd, "moments": mom}


def test_perpendicular_half_planes_never_exchange_colour():
    H, W = 24, 40
    frame, planes = synthetic(W, H, 4, seed=3, hits="all")
    left = np.zeros((H, W), bool)
    left[:, : W // 2] = True
    planes["normal_depth"][..., :3] = np.where(left[..., None], F([4, 0, 0]), F([0, 4, 0]))  # the unit normals' dot is exactly 0
    a = denoise.reference(frame, planes)
    frame2 = frame.copy()
    planes2 = {k: v.copy() for k, v in planes.items()}
    frame2[~left, :3] *= F(7.0)  # another right half: colours, moments, albedo, depth
    planes2["moments"][~left, :3] *= F(55.0)
    planes2["albedo"][~left, :3] *= F(0.5)
    planes2["normal_depth"][~left, 3] *= F(3.0)
    b = denoise.reference(frame2, planes2)
    assert a[left].tobytes() == b[left].tobytes()
    assert a[~left].tobytes() != b[~left].tobytes()


def test_invalid_pixels_stay_zero_and_influence_nobody():
    H, W = 30, 37
    frame, planes = synthetic(W, H, 4, seed=5)
    holes = np.random.default_rng(1).random((H, W)) < 0.25
    frame[holes] = 0  # n == 0 there; the planes still hold whatever they hold
    a = denoise.reference(frame, planes)
    assert (a[holes] == 0).all() and (a[~holes][:, 3] == 1).all()
    planes2 = {k: v.copy() for k, v in planes.items()}
    for v in planes2.values():
        v[holes] = F(123.0)
    b = denoise.reference(frame, planes2)
    assert a.tobytes() == b.tobytes()


def test_zero_variance_image_with_distinct_neighbours_comes_back_unharmed():
    # every tap differs from the centre by >= 0.01 in demodulated luminance and the variance is 0: every off-centre weight is
    # exp_(-(..) / 1e-6) = exactly 0, what remains is the rounding of (k d) / k and of c / a * a
    H, W = 33, 33
    y, x = np.mgrid[0:H, 0:W]
    l = (F(0.02) * (y * W + x + 5)).astype(F)  # a ramp: any two pixels differ by >= 0.02 in colour, >= 0.01 after / albedo 0.5 .. 1
    frame, planes = _flat_planes(H, W, 4, np.stack([l, l, l], -1))
    out = denoise.reference(frame, planes)
    c = frame[..., :3] / frame[..., 3:4]
    ulps = np.abs(out[..., :3].astype(np.float64) - c) / np.spacing(c)
    assert ulps.max() <= 4, ulps.max()
    assert (out[..., 3] == 1).all()


def test_constant_demodulated_image_with_arbitrary_guides_comes_back():
    H, W = 29, 43
    rng = np.random.default_rng(11)
    frame, planes = synthetic(W, H, 4, seed=9)  # arbitrary normals, depths, coverage
    n = frame[..., 3:4]
    hits = planes["albedo"][..., 3:4]
    a = ((planes["albedo"][..., :3] + (n - hits)) / n).astype(F)
    assert (a >= 0.01).all()
    frame[..., :3] = (F(0.75) * a) * n  # mean colour = 0.75 x albedo: the demodulated image is 0.75 up to rounding
    c = frame[..., :3] / n
    planes["moments"][..., :3] = (c * c * n * F(1.5)).astype(F)  # and a variance that lets the filter mix freely
    out = denoise.reference(frame, planes)
    ulps = np.abs(out[..., :3].astype(np.float64) - c) / np.spacing(c)
    assert ulps.max() <= 8, ulps.max()  # d = c / a (1/2 ulp), a weighted mean of values within 1 ulp of each other, d * a
    del rng


def test_output_is_finite_for_huge_samples_and_for_moments_below_the_square_of_the_mean():
    H, W = 20, 21
    frame, planes = synthetic(W, H, 4, seed=13)
    frame[3:9, 4:11, :3] = F(1e30)
    planes["moments"][3:9, 4:11, :3] = F(np.inf)                 # 1e60 does not fit
    planes["moments"][12:18, 2:19, :3] *= F(0.25)                 # MOMENTS < n c^2
    frame[0, 0, :3] = F(4e30)
    planes["moments"][0, 0, :3] = F(3e38)
    for it in (0, 1, 5):
        out = denoise.reference(frame, planes, params(it))
        assert np.isfinite(out).all(), it


def test_one_sample_pixels_pass_through_unfiltered():
    H, W = 16, 18
    frame, planes = synthetic(W, H, 1, seed=17, hits="all")
    out = denoise.reference(frame, planes)
    c = frame[..., :3]
    # v = 0 and distinct noisy neighbours: nothing but the pixel's own sample (taps of exactly equal luminance aside)
    assert np.abs(out[..., :3] - c).max() <= 1e-5 * np.abs(c).max()


def test_relative_mse_is_the_issues_measure():
    a = np.zeros((2, 2, 4), F)
    r = np.ones((2, 2, 4), F)
    assert denoise.relative_mse(a, r) == pytest.approx(3 / 3.01)


def test_default_params_are_the_documented_ones():
    p = denoise.default_params()
    assert (p.iterations, p.normal_power, p.sigma_l, p.sigma_z, p.kernel) == (5, 7, 4.0, 4.0, ffi.HR_DENOISE_KERNEL_AUTO)
