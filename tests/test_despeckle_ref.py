"""The arithmetic of firefly suppression without a GPU: heatray_amd/csrc/hr_despeckle.h compiled for the CPU
(tests/host/despeckle_cpu.cpp, plain and once more under AddressSanitizer + UBSan) against its numpy restatement
heatray_amd.despeckle.reference, byte for byte in both outputs and equal in all five counters, on seeded frames and on hand-made inputs
whose answers are known (include/hrcore_despeckle.h is the contract).  tests/test_gpu_despeckle.py holds the device to the same
reference."""
import numpy as np
import pytest

import cpu_header
from despeckle_frames import FLAT, F, fireflies_at, flat, params, plant_classes, same_counters, speckled, with_spot
from heatray_amd import denoise, despeckle
from synthetic_frames import same_bits, synthetic

SIZES = [(1, 1), (2, 2), (5, 300), (67, 41), (16, 16)]


def _runner(exe):
    def run(frame, mom, p):
        p = p if p is not None else despeckle.default_params()
        H, W = frame.shape[:2]
        head = np.array([W, H, p.rank, p.min_taps], np.int32).tobytes() + np.array([p.ratio, p.sigmas, p.floor, 0], F).tobytes()
        raw = cpu_header.run(exe, head + np.ascontiguousarray(frame, F).tobytes() + np.ascontiguousarray(mom, F).tobytes())
        n = W * H * 16
        assert len(raw) == 2 * n + 40
        words = np.frombuffer(raw[2 * n:], np.uint64)
        res = dict(zip(("valid_pixels", "clamped_pixels", "kept_pixels", "starved_pixels", "nonfinite_pixels"), (int(v) for v in words)))
        return np.frombuffer(raw[:n], F).reshape(H, W, 4), np.frombuffer(raw[n:2 * n], F).reshape(H, W, 4), res
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cpu(request, tmp_path_factory):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _runner(cpu_header.build("despeckle", tmp_path_factory.mktemp("despeckle_" + request.param), flags=flags))


def _check(cpu, frame, mom, p, what):
    """the header's host build against the reference; returns the reference's (out, moments_out, result, classes)"""
    want = despeckle.reference(frame, mom, p, with_classes=True)
    out, mout, res = cpu(frame, mom, p)
    same_bits(out, want[0], what + ": frame")
    same_bits(mout, want[1], what + ": moments")
    same_counters(res, want[2], what)
    r, cls = want[2], want[3]
    # every pixel is in one class; clamped, kept and starved pixels are valid ones and exclude each other
    assert r["clamped_pixels"] + r["kept_pixels"] + r["starved_pixels"] <= r["valid_pixels"] <= frame.shape[0] * frame.shape[1] - r["nonfinite_pixels"], (what, r)
    assert not (cls["clamped"] & cls["kept"]).any() and not (cls["starved"] & (cls["clamped"] | cls["kept"])).any()
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cpu_header_equals_numpy_reference_byte_for_byte(cpu, size):
    W, H = size
    seed = W * 1000 + H
    seen = {k: 0 for k in ("clamped_pixels", "kept_pixels", "starved_pixels", "nonfinite_pixels")}
    for n in (1, 4):
        for name, (frame, planes) in {"synthetic": synthetic(W, H, n, seed), "with holes": synthetic(W, H, n, seed + 1, holes=True)}.items():
            r = _check(cpu, frame, planes["moments"], None, f"{name} {W}x{H} n={n}")[2]
            for k in seen:
                seen[k] += r[k]
        frame, mom, _, _ = speckled(W, H, n, seed + 2, rate=0.02)
        kinds = plant_classes(frame, mom, seed + 3)
        if W * H > 1000:  # two bright pixels whose samples agree: with n >= 2 the guard keeps them
            for x, y in ((W // 2, H // 2), (W // 3, H // 3)):
                frame[y, x], mom[y, x] = (50 * n, 50 * n, 50 * n, n), (2500 * n, 2500 * n, 2500 * n, n)
                for k in kinds.values():
                    k[y, x] = False
        for rank in (1, 2, 3, 4):
            for min_taps in (rank, 24):
                want = _check(cpu, frame, mom, params(rank=rank, min_taps=min_taps), f"speckled with classes {W}x{H} n={n} rank={rank} min_taps={min_taps}")
                for k in seen:
                    seen[k] += want[2][k]
                bad = kinds["nan_f"] | kinds["inf_f"] | kinds["inf_n"]
                assert (want[3]["nonfinite"] == bad).all() and want[2]["nonfinite_pixels"] == int(bad.sum())
                assert not want[0][bad].any() and not want[1][bad].any()  # 0 0 0 0 in both outputs
                same_bits(want[0][kinds["hole"]], frame[kinds["hole"]], "an EMPTY pixel is copied")
                if n >= 2:  # (with one sample nobody is KEPT: the guard asks for two)
                    assert not (want[3]["kept"] & (kinds["nan_m"] | kinds["inf_m"])).any()  # non-finite moments never keep a pixel
                else:
                    assert want[2]["kept_pixels"] == 0
    if W * H > 1000:  # (the inputs exercise every class)
        assert all(v > 0 for v in seen.values()), seen


def test_other_ratios_sigmas_and_floors(cpu):
    frame, mom, _, _ = speckled(67, 41, 3, seed=7, rate=0.02)
    plant_classes(frame, mom, 8)
    for p in (params(ratio=1.0), params(ratio=1.5, sigmas=0.0), params(ratio=4.0, sigmas=10.0, floor=0.25), params(floor=100.0), params(ratio=1e30)):
        want = _check(cpu, frame, mom, p, f"ratio={p.ratio} sigmas={p.sigmas} floor={p.floor}")
        if p.floor == 100.0 or p.ratio == 1e30:  # nobody is above such a threshold
            assert want[2]["clamped_pixels"] == want[2]["kept_pixels"] == 0


def test_a_flat_frame_comes_back_byte_for_byte(cpu):
    for n in (1, 4):
        frame, mom = flat(67, 41, n)
        out, mout, r, _ = _check(cpu, frame, mom, None, f"flat n={n}")
        same_bits(out, frame, "flat: frame")
        same_bits(mout, mom, "flat: moments")
        assert r == {"valid_pixels": 67 * 41, "clamped_pixels": 0, "kept_pixels": 0, "starved_pixels": 0, "nonfinite_pixels": 0}


def test_a_bright_pixel_sure_of_itself_is_kept_and_one_sample_is_clamped(cpu):
    lum_flat = denoise.lum(*(F(v) for v in FLAT))
    # four samples that agree: zero variance, ex * ex > 0: KEPT, the frame comes back byte for byte
    frame, mom = with_spot(33, 18, 4, 20, 9)
    out, mout, r, cls = _check(cpu, frame, mom, None, "a certain spot")
    same_bits(out, frame, "certain spot: frame")
    same_bits(mout, mom, "certain spot: moments")
    assert r["kept_pixels"] == 1 and r["clamped_pixels"] == 0 and cls["kept"][9, 20]
    # the same pixel with one sample: CLAMPED to twice the field's luminance, exactly (every factor is a power of two away from exact)
    frame, mom = with_spot(33, 18, 1, 20, 9)
    out, mout, r, cls = _check(cpu, frame, mom, None, "a one-sample spot")
    assert r["clamped_pixels"] == 1 and r["kept_pixels"] == 0 and cls["clamped"][9, 20]
    assert denoise.lum(*out[9, 20, :3]) == F(2.0) * lum_flat and out[9, 20, 3] == 1
    assert denoise.lum(*mout[9, 20, :3]) == (F(2.0) * lum_flat) * (F(2.0) * lum_flat) and mout[9, 20, 3] == 1
    others = np.ones((18, 33), bool)
    others[9, 20] = False
    same_bits(out[others], frame[others], "everybody else is copied")
    # rank 1 looks at the maximum: the spot's neighbours see the spot and stay; the spot sees only the field
    _, _, r1, _ = _check(cpu, frame, mom, params(rank=1, min_taps=1), "rank 1")
    assert r1["clamped_pixels"] == 1


def test_tiny_images_are_all_starved(cpu):
    for W, H in ((1, 1), (2, 2)):
        frame, mom, _, _ = speckled(W, H, 1, seed=5, rate=0.5)
        out, mout, r, _ = _check(cpu, frame, mom, None, f"{W}x{H}")
        same_bits(out, frame, "starved: copied")
        same_bits(mout, mom, "starved: copied")
        assert r["starved_pixels"] == r["valid_pixels"] == W * H and r["clamped_pixels"] == 0
    # a corner has exactly the default's eight taps: not starved there, starved with nine
    frame, mom = flat(16, 16, 2)
    assert _check(cpu, frame, mom, None, "corner, 8")[2]["starved_pixels"] == 0
    assert _check(cpu, frame, mom, params(min_taps=9), "corner, 9")[2]["starved_pixels"] == 4


def test_a_nan_pixel_becomes_a_hole_and_is_nobodys_tap(cpu):
    frame, mom = flat(16, 16, 2)
    frame[8, 8, 0] = np.nan
    frame[3, 3] = mom[3, 3] = 0  # EMPTY
    frame[3, 3, 1] = -0.0        # ... whose bits come back
    out, mout, r, cls = _check(cpu, frame, mom, params(min_taps=24), "NaN and hole")
    assert not out[8, 8].any() and not mout[8, 8].any() and r["nonfinite_pixels"] == 1 and r["valid_pixels"] == 254
    same_bits(out[3, 3], frame[3, 3], "EMPTY: copied")
    # with min_taps 24 every pixel that has the NaN pixel or the hole inside its window is starved, and nobody else away from the border
    reach = np.zeros((16, 16), bool)
    reach[6:11, 6:11] = reach[1:6, 1:6] = True
    inner = np.zeros((16, 16), bool)
    inner[2:14, 2:14] = True
    assert (cls["starved"][inner] == (reach & cls["valid"])[inner]).all()


@pytest.mark.parametrize("n, seed", [(1, 101), (4, 104)])
def test_speckled_frame_every_firefly_is_clamped_and_the_error_falls(n, seed):
    """The issue's caps: every injected pixel clamped, at most 1 % of the others, and relative MSE against the analytic mean (injected
    energy included) falls."""
    W, H = 128, 96
    frame, mom, injected, truth = speckled(W, H, n, seed)
    out, _, r, cls = despeckle.reference(frame, mom, with_classes=True)
    assert injected.sum() > 0 and cls["clamped"][injected].all()
    others = cls["clamped"] & ~injected
    before = denoise.relative_mse(frame[..., :3] / frame[..., 3:4], truth)
    after = denoise.relative_mse(out[..., :3] / out[..., 3:4], truth)
    print(f"speckled {W}x{H} n={n} seed={seed}: injected {int(injected.sum())}, all clamped; others clamped {others.sum() / (~injected).sum():.4%}; "
          f"relative MSE {before:.3f} -> {after:.3f}")
    assert others.sum() <= 0.01 * (~injected).sum()
    assert after < before


def test_reference_denoise_is_the_denoiser_over_the_despeckled_pair():
    from heatray_amd import denoise_spatial
    frame, planes = synthetic(33, 18, 2, seed=3)
    fireflies_at(frame, planes["moments"], [(20, 9)])  # one more sample, 500 times the pixel's mean
    out, mout, r = despeckle.reference(frame, planes["moments"])
    assert r["clamped_pixels"] >= 1
    clean = dict(planes, moments=mout)
    same_bits(despeckle.reference_denoise(frame, planes), denoise.reference(out, clean), "plain")
    img, res = despeckle.reference_denoise(frame, planes, spatial=True, with_result=True)
    same_bits(img, denoise_spatial.reference(out, clean), "spatial")
    assert res == r
    # a threshold nobody reaches: the denoiser over the raw pair
    same_bits(despeckle.reference_denoise(frame, planes, params(ratio=1e30)), denoise.reference(frame, planes), "ratio 1e30")


def test_default_params_and_the_parameter_check():
    p = despeckle.default_params()
    assert (p.rank, p.min_taps, p.ratio, p.sigmas, p.floor, list(p.reserved)) == (2, 8, 2.0, 3.0, 0.0, [0, 0, 0])
    frame, mom = flat(4, 4, 1)
    for bad in (params(rank=0), params(rank=5), params(rank=3, min_taps=2), params(min_taps=25), params(ratio=0.5), params(ratio=float("nan")),
                params(sigmas=-1.0), params(floor=float("inf"))):
        with pytest.raises(ValueError):
            despeckle.reference(frame, mom, bad)
