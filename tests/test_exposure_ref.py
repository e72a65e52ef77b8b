"""The arithmetic of auto-exposure without a GPU: heatray_amd/csrc/hr_exposure.h compiled for the CPU (tests/host/exposure_cpu.cpp, plain
and once more under AddressSanitizer + UBSan) against its numpy restatement heatray_amd.exposure.reference, byte for byte, on seeded
images and on hand-made inputs whose answers are known (include/hrcore_exposure.h is the contract).  tests/test_gpu_exposure.py holds
the device to the same reference."""
import numpy as np
import pytest

import cpu_header
from exposure_frames import CLASS_PIXELS, F, all_bins, bits, class_row, flat, params, same_result, seeded, windows
from heatray_amd import exposure

WIDE = dict(min_scale=2.0 ** -40, max_scale=2.0 ** 40)  # clamps no image of these tests reaches


def _runner(exe):
    def run(p, image=None, bins=None, state=None):
        """exposure.reference's triple (image) or exposure.reduce's pair plus the bins (bins), from the header's host build"""
        H, W = image.shape[:2] if image is not None else (0, 0)
        head = np.array([0 if image is not None else 1, W, H, 0 if state is None else 1, *p.window, p.low_permille, p.high_permille], np.int32)
        fl = np.array([p.key, p.min_scale, p.max_scale, p.adapt, 0.0 if state is None else state], F)
        payload = np.ascontiguousarray(image, F) if image is not None else np.asarray(bins, np.uint64)
        raw = cpu_header.run(exe, head.tobytes() + fl.tobytes() + payload.tobytes())
        words = np.frombuffer(raw[:260 * 8], np.uint64)
        scale, target, lavg = (float(v) for v in np.frombuffer(raw[2080:2092], F))
        q = int(np.frombuffer(raw[2092:2096], np.uint32)[0])
        counted, used = (int(v) for v in np.frombuffer(raw[2096:2112], np.uint64))
        flags, has = (int(v) for v in np.frombuffer(raw[2112:2120], np.uint32))
        nxt = np.frombuffer(raw[2120:2124], F)[0]
        assert len(raw) == 2124
        res = {"scale": scale, "target": target, "key_luminance": lavg, "position": q, "counted": counted, "used": used, "flags": flags}
        if image is not None:
            res.update(below=int(words[256]), above=int(words[257]), nonfinite=int(words[258]), invalid=int(words[259]))
        return res, words[:256].copy(), (nxt if has else None)
    return run


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def cpu(request, tmp_path_factory):
    flags = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") if request.param == "sanitized" else ()
    return _runner(cpu_header.build("exposure", tmp_path_factory.mktemp("exposure_" + request.param), flags=flags))


def _check_image(cpu, image, p, what, state=None):
    want, want_bins, want_state = exposure.reference(image, p, state)
    got, got_bins, got_state = cpu(p, image=image, state=state)
    assert got_bins.tobytes() == want_bins.tobytes(), (what, np.nonzero(got_bins != want_bins))
    same_result(got, want, what)
    assert (got_state is None) == (want_state is None) and (got_state is None or F(got_state).tobytes() == F(want_state).tobytes()), (what, got_state, want_state)
    H, W = image.shape[:2]
    x0, y0, x1, y1 = p.window
    n = (x1 - x0) * (y1 - y0) if any(p.window) else W * H
    assert want["counted"] + want["below"] + want["above"] + want["nonfinite"] + want["invalid"] == n, (what, want)  # every pixel is in one class
    return want, want_bins, want_state


def _check_bins(cpu, bins, p, what, state=None):
    want, want_state = exposure.reduce(bins, p, state)
    got, got_bins, got_state = cpu(p, bins=bins, state=state)
    assert got_bins.tobytes() == np.asarray(bins, np.uint64).tobytes()
    same_result(got, want, what)
    assert (got_state is None) == (want_state is None) and (got_state is None or F(got_state).tobytes() == F(want_state).tobytes()), (what, got_state, want_state)
    return want, want_state


SIZES = [(1, 1), (67, 35), (257, 3), (3, 257), (256, 4)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cpu_header_equals_numpy_reference_byte_for_byte(cpu, size):
    W, H = size
    image = seeded(W, H, seed=W * 1000 + H)
    for name, win in windows(W, H).items():
        want, _, _ = _check_image(cpu, image, params(win), f"{W}x{H} {name}")
    if W * H > 100:  # (the whole image: the inputs exercise every class)
        whole, _, _ = exposure.reference(image)
        assert all(whole[k] > 0 for k in ("counted", "below", "above", "nonfinite", "invalid")), whole


def test_every_class_lands_where_the_contract_says(cpu):
    row = class_row()
    for i, (name, (px, cls)) in enumerate(CLASS_PIXELS.items()):
        want, bins, _ = _check_image(cpu, row, params((i, 0, i + 1, 1)), name)
        if isinstance(cls, int):
            assert bins[cls] == 1 and bins.sum() == 1 and want["counted"] == 1, (name, np.nonzero(bins))
        else:
            assert want[cls] == 1 and bins.sum() == 0 and want["flags"] == exposure.EMPTY, (name, want)
    want, bins, _ = _check_image(cpu, row, params(), "the whole row")
    assert (want["counted"], want["below"], want["above"], want["nonfinite"], want["invalid"]) == (3, 5, 2, 3, 3), want
    assert sorted(np.nonzero(bins)[0]) == [0, 128, 255] and bins[128] == 1


def _one_bin(k, n):
    b = np.zeros(256, np.uint64)
    b[k] = n
    return b


def test_reduce_on_hand_made_histograms(cpu):
    # N = 1: lo = 0, hi = 0 -> 1; the sample's bin centre comes back
    r, s = _check_bins(cpu, _one_bin(128, 1), params(), "N = 1")
    assert (r["used"], r["position"]) == (1, 257 * 256) and r["key_luminance"] == float(bits((127 << 23) | (256 << 11))) == 1.0625 and s == F(r["scale"])
    # hi <= lo forced
    r, _ = _check_bins(cpu, _one_bin(40, 1), params(low_permille=100, high_permille=900), "hi <= lo")
    assert (r["used"], r["position"]) == (1, 81 * 256)
    # the whole range
    full = np.arange(1, 257).astype(np.uint64)
    r, _ = _check_bins(cpu, full, params(low_permille=0, high_permille=1000), "0 .. 1000")
    assert r["used"] == r["counted"] == int(full.sum())
    assert r["position"] == (sum(int(h) * (2 * k + 1) for k, h in enumerate(full)) << 8) // int(full.sum())
    # all 256 bins occupied, the default percentiles: by hand with a sorted list
    r, _ = _check_bins(cpu, full, params(), "all bins")
    pos = np.repeat(2 * np.arange(256) + 1, full.astype(np.int64))
    N = len(pos)
    lo, hi = N * 100 // 1000, N * 950 // 1000
    assert r["used"] == hi - lo and r["position"] == (int(pos[lo:hi].sum()) << 8) // (hi - lo)
    # the ends of the map, and both clamps
    r, _ = _check_bins(cpu, _one_bin(0, 1000), params(), "all in bin 0")
    assert r["position"] == 256 and r["key_luminance"] == 2.0 ** -16 * 1.0625 and r["flags"] == exposure.CLAMPED_HIGH and r["target"] == r["scale"] == 256.0
    r, _ = _check_bins(cpu, _one_bin(255, 1000), params(), "all in bin 255")
    assert r["position"] == 511 * 256 and r["key_luminance"] == 2.0 ** 15 * 1.9375 and r["flags"] == exposure.CLAMPED_LOW and r["target"] == 1.0 / 256.0
    r, _ = _check_bins(cpu, _one_bin(255, 1000), params(**WIDE), "all in bin 255, wide clamps")
    assert r["flags"] == 0 and r["target"] == float(F(0.18) / F(2.0 ** 15 * 1.9375))
    # the integer widths: 2^27 samples in one bin (2^27 * 1000 and T << 8 pass 2^32)
    r, _ = _check_bins(cpu, _one_bin(255, 1 << 27), params(**WIDE), "N = 2^27")
    assert r["counted"] == 1 << 27 and r["used"] == (1 << 27) * 950 // 1000 - (1 << 27) * 100 // 1000 and r["position"] == 511 * 256
    r, _ = _check_bins(cpu, _one_bin(7, 1 << 27) + _one_bin(200, 1 << 27), params(**WIDE), "N = 2^28 in two bins")
    assert r["counted"] == 1 << 28


def test_an_empty_metering_keeps_the_state(cpu):
    zero = np.zeros(256, np.uint64)
    r, s = _check_bins(cpu, zero, params(), "EMPTY without a state")
    assert r["flags"] == exposure.EMPTY and r["scale"] == r["target"] == 1.0 and s is None and (r["counted"], r["used"], r["position"], r["key_luminance"]) == (0, 0, 0, 0.0)
    r, s = _check_bins(cpu, zero, params(adapt=0.25), "EMPTY with a state", state=F(3.5))
    assert r["flags"] == exposure.EMPTY and r["scale"] == r["target"] == 3.5 and s == F(3.5)
    holes = np.zeros((5, 7, 4), F)
    want, _, s = _check_image(cpu, holes, params(), "an image of holes", state=F(0.75))
    assert want["flags"] == exposure.EMPTY and want["invalid"] == 35 and want["scale"] == 0.75 and s == F(0.75)


def test_an_adaptation_sequence_of_five_meterings(cpu):
    p = params(adapt=0.25)
    state, scales = None, []
    for i in range(5):
        image = flat(9, 5, (4.0, 4.0, 4.0) if i % 2 == 0 else (0.01, 0.01, 0.01))
        want, _, state = _check_image(cpu, image, p, f"metering {i}", state=state)
        assert want["flags"] == (exposure.ADAPTED if i else 0), want
        scales.append(F(want["scale"]))
        assert state == scales[-1]
    assert scales[0] == F(exposure.reference(flat(9, 5, (4.0, 4.0, 4.0)))[0]["target"])  # the first has nothing to adapt from
    dark = F(exposure.reference(flat(9, 5, (0.01, 0.01, 0.01)))[0]["target"])
    assert scales[1].tobytes() == F(scales[0] + F(F(dark - scales[0]) * F(0.25))).tobytes()
    assert scales[0] < scales[2] < scales[4] and scales[1] < scales[3]  # both sub-sequences creep towards the other image's target
    # adapt = 1 has no memory, adapt = 0 never moves
    assert exposure.reference(flat(9, 5), params(adapt=1.0), state=F(7.0))[0]["flags"] == 0
    r, _, s = _check_image(cpu, flat(9, 5), params(adapt=0.0), "adapt = 0", state=F(7.0))
    assert r["scale"] == 7.0 and s == F(7.0) and r["flags"] == exposure.ADAPTED


def test_scaling_by_a_power_of_two_moves_the_position_and_nothing_else(cpu):
    image = seeded(67, 35, seed=5, classes=False)
    p = params(**WIDE)
    base, base_bins, _ = _check_image(cpu, image, p, "unscaled")
    assert base["flags"] == 0 and base["counted"] == 67 * 35
    shown = exposure.apply(image, base["scale"])
    for k in (-4, -1, 1, 3):
        scaled = image.copy()
        scaled[..., :3] *= F(2.0 ** k)
        r, b, _ = _check_image(cpu, scaled, p, f"k = {k}")
        assert r["flags"] == 0, (k, r)  # neither clamp engages, or the identity below would not hold
        assert r["position"] == base["position"] + 4096 * k and r["used"] == base["used"]
        assert F(F(r["scale"]) * F(2.0 ** k)).tobytes() == F(base["scale"]).tobytes(), (k, r, base)
        assert (np.roll(base_bins, 8 * k) == b).all()
        assert exposure.apply(scaled, r["scale"]).tobytes() == shown.tobytes(), k  # the pre-multiplied image is the same image


@pytest.mark.parametrize("median", [2.0 ** -6, 1.0, 2.0 ** 3])
def test_key_luminance_is_within_a_quarter_octave_of_the_trimmed_geometric_mean(median):
    """the bound is derived in include/hrcore_exposure.h: 0.0861 octave of the piecewise-linear log each way and 1/16 octave of bin width"""
    image = seeded(160, 90, seed=11, median=median, sigma=2.0, classes=False, max_n=1)
    r, _, _ = exposure.reference(image, params(**WIDE))
    assert r["counted"] == 160 * 90
    L = np.sort((image[..., :3] / image[..., 3:4]) @ np.array([0.2126, 0.7152, 0.0722]), axis=None)
    lo, hi = len(L) * 100 // 1000, len(L) * 950 // 1000
    geo = np.log2(L[lo:hi].astype(np.float64)).mean()
    err = np.log2(r["key_luminance"]) - geo
    print(f"median {median}: key_luminance {r['key_luminance']:.6g}, trimmed geometric mean {2 ** geo:.6g}, {err:+.4f} octave")
    assert abs(err) <= 0.25


def test_default_params_and_adapt_rate():
    p = exposure.default_params()
    assert (F(p.key), p.low_permille, p.high_permille, p.min_scale, p.max_scale, p.adapt, list(p.window), list(p.reserved)) == \
        (F(0.18), 100, 950, 1.0 / 256.0, 256.0, 1.0, [0] * 4, [0] * 6)
    assert exposure.adapt_rate(1.0, 0.0) == 1.0 and exposure.adapt_rate(0.0, 1.0) == 0.0 and abs(exposure.adapt_rate(0.5, 0.5) - (1 - np.exp(-1))) < 1e-15


def test_all_bins_image_occupies_every_bin():
    _, bins, _ = exposure.reference(all_bins(256, 4))
    assert (bins == 4).all()
