"""The arithmetic of the progressive history merge and the preview without a GPU: heatray_amd/csrc/hr_reproject.h compiled for the CPU
(tests/host/reproject_cpu.cpp) against its numpy restatement heatray_amd.reproject.reference_merge_progressive / reference_preview, bit
for bit, every pixel, on synthetic frames, planes and cameras; and properties of the reference itself on constructed inputs whose answers
are known (include/hrcore_reproject.h is the contract).  tests/test_gpu_reproject.py holds the device to the same reference."""
import numpy as np
import pytest

import cpu_header
from heatray_amd import history, reproject, scenes
from synthetic_frames import F, MOVES, camera, flat, merge_input, plane_view, rot_x, rot_y, same_bits, translate, uniform

U = 2.0 ** -24  # unit roundoff of binary32


def keep(view, mask):
    """the view with only the pixels of `mask` sampled: the others are 0 0 0 0 in the frame and in every plane"""
    frame, planes = view
    m = np.asarray(mask, bool)[..., None]
    return np.where(m, frame, F(0.0)).astype(F), {k: np.where(m, planes[k], F(0.0)).astype(F) for k in history.PLANES}


def sub_pass_mask(W, H, k):
    """the pixels sub-pass k of the 3 x 3 walk samples"""
    y, x = np.mgrid[0:H, 0:W]
    bx, by = reproject.sub_pass_pixel(k)
    return (x % 3 == bx) & (y % 3 == by)


@pytest.fixture(scope="module")
def cpu(tmp_path_factory):
    exe = cpu_header.build("reproject", tmp_path_factory.mktemp("reproject_cpu"))

    def run(old, old_cam, new, new_cam, examined, p):
        H, W = old[0].shape[:2]
        raw = np.frombuffer(cpu_header.run(exe, merge_input(old, old_cam, new, new_cam, p) + np.ascontiguousarray(examined, np.uint8).tobytes()), np.uint8)
        n = W * H * 16
        img = lambda k: raw[k * n:(k + 1) * n].view(F).reshape(H, W, 4)
        E = raw[8 * n:8 * n + W * H].reshape(H, W).astype(bool)
        res = np.frombuffer(raw[8 * n + W * H:8 * n + W * H + 64].tobytes(), np.uint64)
        return {"history": raw[:3 * n].view(F).reshape(3, H, W, 4), "preview": img(3), "frame": img(4), "planes": {k: img(5 + i) for i, k in enumerate(history.PLANES)},
                "examined": E,
                "merge": dict(zip(("reused_pixels", "rejected_pixels", "history_samples", "pending_pixels", "examined_pixels"), (int(v) for v in res[:5]))),
                "counts": dict(zip(("own_pixels", "previewed_pixels", "empty_pixels"), (int(v) for v in res[5:8])))}
    return run


def _check(cpu, old, old_cam, new, new_cam, examined, p, what):
    """the CPU build of the header against the numpy reference, bit for bit; returns (merged frame, planes, examined, result, preview image, counts)"""
    hist = history.reference_capture(*old)
    image, counts = reproject.reference_preview(hist, old_cam, new[0], new[1], new_cam, p)
    frame, planes, E, res = reproject.reference_merge_progressive(hist, old_cam, new[0], new[1], new_cam, examined, p)
    got = cpu(old, old_cam, new, new_cam, examined, p)
    same_bits(got["history"], hist, what + ": history")
    same_bits(got["preview"], image, what + ": preview")
    assert got["counts"] == counts, (what, got["counts"], counts)
    same_bits(got["frame"], frame, what + ": frame")
    for k in history.PLANES:
        same_bits(got["planes"][k], planes[k], f"{what}: {k}")
    same_bits(got["examined"], E, what + ": examined")
    assert got["merge"] == {k: res[k] for k in got["merge"]}, (what, got["merge"], res)
    H, W = image.shape[:2]
    assert counts["own_pixels"] + counts["previewed_pixels"] + counts["empty_pixels"] == W * H
    assert res["pending_pixels"] + res["examined_pixels"] == W * H
    assert set(np.unique(image[..., 3])) <= {0.0, 1.0} and not image[image[..., 3] == 0].any()
    return frame, planes, E, res, image, counts


CASES = [(67, 41, "none", 1, "third"), (67, 41, "yaw", 2, "ninth"), (67, 41, "orbit", 3, "random"), (131, 19, "pitch_shift", 4, "ninth"), (5, 300, "dolly", 5, "random"),
         (64, 16, "zoom", 6, "third"), (1, 1, "none", 7, "random"), (70, 45, "orbit", 9, "ninth")]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_cpu_header_equals_numpy_reference_bit_for_bit(cpu, case):
    W, H, move, seed, sampling = case
    base = translate(0.1, 0.2, 0.3) @ rot_y(0.2) @ rot_x(-0.1)  # (no identity matrices: every product of R and t rounds)
    m, fov_new = MOVES[move]()
    old_cam = camera(base, 0.24, W=W, H=H)
    new_cam = camera(base @ m, fov_new, W=W, H=H)
    old = plane_view(W, H, old_cam, seed)
    rng = scenes.SplitMix64(seed + 1000)
    u = uniform(rng, (2, H, W))
    sampled = {"ninth": sub_pass_mask(W, H, seed % 9), "third": sub_pass_mask(W, H, 0) | sub_pass_mask(W, H, 4) | sub_pass_mask(W, H, 8), "random": u[0] < 0.5}[sampling]
    new = keep(plane_view(W, H, new_cam, seed + 100), sampled)
    examined = u[1] < 0.3  # (some pixels have been examined by an earlier call, sampled or not)
    _, _, _, res, _, counts = _check(cpu, old, old_cam, new, new_cam, examined, history.default_params(), f"case {case}")
    todo = int(((new[0][..., 3] > 0) & ~examined).sum())
    assert res["reused_pixels"] + res["rejected_pixels"] == todo
    if W * H > 1000:  # the inputs exercise every answer
        assert res["reused_pixels"] > 0 and res["rejected_pixels"] > 0
        assert counts["own_pixels"] > 0 and counts["previewed_pixels"] > 0 and counts["empty_pixels"] > 0, counts


def _views(W, H, move, seed):
    base = translate(0.1, 0.2, 0.3) @ rot_y(0.2) @ rot_x(-0.1)
    m, fov_new = MOVES[move]()
    old_cam, new_cam = camera(base, 0.24, W=W, H=H), camera(base @ m, fov_new, W=W, H=H)
    return old_cam, new_cam, plane_view(W, H, old_cam, seed), plane_view(W, H, new_cam, seed + 100)


@pytest.mark.parametrize("split", ["one", "nine", "random"])
def test_any_partition_of_the_sampled_pixels_gives_one_merge(split):
    """MERGE reads the pixel's own four values and the immutable history: the frame filled in and merged subset by subset ends with the
    bits, and the summed counters, of one history.reference_merge over the whole frame."""
    W, H = 70, 45
    old_cam, new_cam, old, new = _views(W, H, "orbit", 11)
    hist = history.reference_capture(*old)
    want_frame, want_planes, want = history.reference_merge(hist, old_cam, new[0], new[1], new_cam)
    if split == "one":
        parts = [np.ones((H, W), bool)]
    elif split == "nine":
        parts = [sub_pass_mask(W, H, k) for k in range(9)]
    else:
        pick = (uniform(scenes.SplitMix64(5), (H, W)) * 4).astype(int)
        parts = [pick == k for k in range(4)]
    assert np.sum(parts, axis=0).min() == 1 == np.sum(parts, axis=0).max()
    frame, planes = keep(new, np.zeros((H, W), bool))
    E = np.zeros((H, W), bool)
    total = {"reused_pixels": 0, "rejected_pixels": 0, "history_samples": 0}
    for part in parts:  # the part's pixels get their samples, then the call
        frame = np.where(part[..., None], new[0], frame)
        planes = {k: np.where(part[..., None], new[1][k], planes[k]) for k in history.PLANES}
        frame, planes, E, res = reproject.reference_merge_progressive(hist, old_cam, frame, planes, new_cam, E)
        for k in total:
            total[k] += res[k]
        assert res["examined_pixels"] == int(E.sum()) and res["pending_pixels"] == W * H - int(E.sum())
    same_bits(frame, want_frame, "frame")
    for k in history.PLANES:
        same_bits(planes[k], want_planes[k], k)
    assert total == {k: want[k] for k in total}
    sampled = new[0][..., 3] > 0
    same_bits(E, sampled, "examined = sampled")
    # a further call changes nothing and counts nothing
    frame2, planes2, E2, res2 = reproject.reference_merge_progressive(hist, old_cam, frame, planes, new_cam, E)
    same_bits(frame2, frame, "second call: frame")
    for k in history.PLANES:
        same_bits(planes2[k], planes[k], "second call: " + k)
    same_bits(E2, E, "second call: examined")
    assert (res2["reused_pixels"], res2["rejected_pixels"], res2["history_samples"]) == (0, 0, 0)
    assert (res2["pending_pixels"], res2["examined_pixels"]) == (int((~sampled).sum()), int(sampled.sum()))


def test_a_second_call_changes_nothing_and_counts_nothing_on_the_cpu_build(cpu):
    W, H = 67, 41
    old_cam, new_cam, old, new = _views(W, H, "yaw", 21)
    new = keep(new, sub_pass_mask(W, H, 0) | sub_pass_mask(W, H, 5))
    p = history.default_params()
    frame, planes, E, res, _, _ = _check(cpu, old, old_cam, new, new_cam, np.zeros((H, W), bool), p, "first")
    assert res["reused_pixels"] > 0
    frame2, planes2, E2, res2, _, _ = _check(cpu, old, old_cam, (frame, planes), new_cam, E, p, "second")
    same_bits(frame2, frame, "frame")
    for k in history.PLANES:
        same_bits(planes2[k], planes[k], k)
    same_bits(E2, E, "examined")
    assert (res2["reused_pixels"], res2["rejected_pixels"], res2["history_samples"]) == (0, 0, 0)


def test_the_preview_of_a_fully_sampled_frame_is_every_pixels_own_mean(cpu):
    W, H = 67, 41
    old_cam, new_cam, old, _ = _views(W, H, "pitch_shift", 31)
    new = plane_view(W, H, new_cam, 32, holes=False)
    _, _, _, _, image, counts = _check(cpu, old, old_cam, new, new_cam, np.zeros((H, W), bool), history.default_params(), "full")
    assert counts == {"own_pixels": W * H, "previewed_pixels": 0, "empty_pixels": 0}
    same_bits(image[..., :3], new[0][..., :3] / new[0][..., 3:], "own mean")
    assert (image[..., 3] == 1).all()


def _one_hole(W, H, x, y, guides):
    """a new view (same camera as the old) in which only the pixels of `guides` {(x, y): "sky" | "surface"} have a sample"""
    surf, sky = flat(W, H, 1), flat(W, H, 1, cov=0.0)
    frame, planes = keep(surf, np.zeros((H, W), bool))
    for (gx, gy), kind in guides.items():
        src = surf if kind == "surface" else sky
        frame[gy, gx] = src[0][gy, gx]
        for k in history.PLANES:
            planes[k][gy, gx] = src[1][k][gy, gx]
    return frame, planes


@pytest.mark.parametrize("guides, previewed", [
    ({(5, 3): "sky", (4, 4): "surface"}, False),      # (0, -1) before (-1, 0): dy decides, the sky guide below wins, and a surface history passes no sky pixel
    ({(5, 3): "surface", (4, 4): "sky"}, True),
    ({(4, 4): "sky", (6, 4): "surface"}, False),      # (-1, 0) before (1, 0): the same dy, dx decides
    ({(4, 4): "surface", (6, 4): "sky"}, True),
    ({(5, 5): "sky", (6, 4): "surface"}, True),       # (1, 0) before (0, 1)
    ({(4, 3): "sky", (5, 2): "surface", (7, 4): "surface"}, False),  # distance 2 before distance 4
    ({(3, 4): "sky", (4, 2): "surface"}, False),      # distance 4 before distance 5
    ({(7, 6): "surface"}, True),                      # the last offset, (2, 2)
    ({(8, 4): "surface", (5, 7): "surface"}, False),  # three pixels away: no guide
])
def test_the_guide_is_the_first_in_the_contracts_order(cpu, guides, previewed):
    """The old view saw one surface everywhere, so a surface guide previews the hole at (5, 4) and a sky guide leaves it empty (a tap
    counts only when its class is the guide's): which of two candidates was taken shows in the answer."""
    W, H = 11, 9
    cam = camera(rot_y(0.03), 0.24, W=W, H=H)
    old = flat(W, H, 32)
    new = _one_hole(W, H, 5, 4, guides)
    _, _, _, _, image, counts = _check(cpu, old, cam, new, cam, np.zeros((H, W), bool), history.default_params(), str(guides))
    assert (image[4, 5, 3] == 1) == previewed, image[4, 5]
    assert counts["own_pixels"] == len(guides)


def test_a_candidate_outside_the_image_is_skipped(cpu):
    W, H = 11, 9
    cam = camera(rot_y(0.03), 0.24, W=W, H=H)
    old = flat(W, H, 32)
    # the corner (0, 0): (0, -1) and (-1, 0) lie outside; (1, 0) is the first inside.  A sky there wins over the surface at (0, 1) ...
    _, _, _, _, image, _ = _check(cpu, old, cam, _one_hole(W, H, 0, 0, {(1, 0): "sky", (0, 1): "surface"}), cam, np.zeros((H, W), bool), history.default_params(), "corner")
    assert image[0, 0, 3] == 0
    # ... and the other way round the surface does
    _, _, _, _, image, _ = _check(cpu, old, cam, _one_hole(W, H, 0, 0, {(1, 0): "surface", (0, 1): "sky"}), cam, np.zeros((H, W), bool), history.default_params(), "corner")
    assert image[0, 0, 3] == 1
    # the far corner: (W, H - 1) is no pixel although its index H * W - 1 + 1 would be one in a flat array
    _, _, _, _, image, _ = _check(cpu, old, cam, _one_hole(W, H, W - 1, H - 2, {(0, H - 1): "surface"}), cam, np.zeros((H, W), bool), history.default_params(), "wrap")
    assert image[H - 2, W - 1, 3] == 0


def test_a_guide_normal_perpendicular_to_the_pixels_ray_gives_an_empty_pixel(cpu):
    """The centre pixel of an odd-sized image under an identity camera: ray = (0, 0, -1) exactly, so a guide normal (1, 0, 0) has
    dot(Nq, rc) = 0 and s is a quotient by zero: not (s > 0 and s < +inf)."""
    W, H = 11, 9
    cam = camera(np.eye(4), 0.24, W=W, H=H)
    old = flat(W, H, 32)
    new = _one_hole(W, H, 5, 4, {(5, 3): "surface"})
    new[1]["normal_depth"][3, 5, :3] = (1.0, 0.0, 0.0)
    _, _, _, _, image, _ = _check(cpu, old, cam, new, cam, np.zeros((H, W), bool), history.default_params(), "perpendicular")
    assert not image[4, 5].any()
    new[1]["normal_depth"][3, 5, :3] = (0.0, 0.0, 1.0)  # the same guide facing the camera previews it
    _, _, _, _, image, _ = _check(cpu, old, cam, new, cam, np.zeros((H, W), bool), history.default_params(), "facing")
    assert image[4, 5, 3] == 1


def test_a_sky_guide_gives_the_skys_history(cpu):
    W, H = 40, 30
    C3 = np.array([0.7310586, 0.2689414, 1.6180340], F)
    old_cam = camera(rot_x(0.1), 0.24, W=W, H=H)
    new_cam = camera(rot_x(0.1) @ rot_y(0.02), 0.24, W=W, H=H)
    old = flat(W, H, 32, colour=C3, cov=0.0)
    new = keep(flat(W, H, 1, cov=0.0), sub_pass_mask(W, H, 4))
    _, _, _, _, image, counts = _check(cpu, old, old_cam, new, new_cam, np.zeros((H, W), bool), history.default_params(), "sky")
    pv = (image[..., 3] == 1) & ~(new[0][..., 3] > 0)
    assert counts["previewed_pixels"] == int(pv.sum()) > 0.8 * (W * H - counts["own_pixels"])
    assert (np.abs(image[pv][:, :3].astype(np.float64) - C3) <= 16 * U * C3).all()
    # ... and a surface history gives a sky guide nothing
    _, _, _, _, image, counts = _check(cpu, flat(W, H, 32, colour=C3), old_cam, new, new_cam, np.zeros((H, W), bool), history.default_params(), "sky against surface")
    assert counts["previewed_pixels"] == 0


@pytest.mark.parametrize("move", sorted(MOVES))
def test_a_constant_history_of_an_exact_plane_comes_back_as_that_constant(cpu, move):
    """P = (sum w_k C) / (sum w_k) over at most four taps, all weights positive.  Roundings: one per product w_k C (four), three for the
    sums of the products, three for the sum of the weights, one for the division, none cancelling because every term has one sign:
    within 16 u |C| with the input's own roundings and the second-order terms.  With the camera unmoved every pixel without a sample
    has a guide on the same plane and is previewed."""
    W, H = 48, 36
    C3 = np.array([0.7310586, 0.2689414, 1.6180340], F)
    base = translate(0.1, 0.2, 0.3) @ rot_y(0.2) @ rot_x(-0.1)
    m, fov_new = MOVES[move]()
    old_cam, new_cam = camera(base, 0.24, W=W, H=H), camera(base @ m, fov_new, W=W, H=H)
    old = flat(W, H, 64, colour=C3)
    old = (old[0], {**old[1], "normal_depth": plane_view(W, H, old_cam, 6, max_n=64, holes=False, sky=False, noise=False)[1]["normal_depth"]})
    new = keep(plane_view(W, H, new_cam, 5, holes=False, sky=False, noise=False), sub_pass_mask(W, H, 0))
    _, _, _, _, image, counts = _check(cpu, old, old_cam, new, new_cam, np.zeros((H, W), bool), history.default_params(), move)
    unsampled = ~(new[0][..., 3] > 0)
    pv = unsampled & (image[..., 3] == 1)
    assert counts["previewed_pixels"] == int(pv.sum()) > 0
    if move == "none":
        assert counts["empty_pixels"] == 0
    assert (np.abs(image[pv][:, :3].astype(np.float64) - C3) <= 16 * U * C3).all()


def test_the_references_leave_their_inputs_alone():
    W, H = 67, 41
    old_cam, new_cam, old, new = _views(W, H, "orbit", 41)
    new = keep(new, sub_pass_mask(W, H, 2))
    hist = history.reference_capture(*old)
    E = np.zeros((H, W), bool)
    arrays = [hist, new[0], E] + [new[1][k] for k in history.PLANES]
    before = [a.tobytes() for a in arrays]
    reproject.reference_preview(hist, old_cam, new[0], new[1], new_cam)
    reproject.reference_merge_progressive(hist, old_cam, new[0], new[1], new_cam, E)
    assert [a.tobytes() for a in arrays] == before


def test_the_offsets_are_the_contracts():
    offs = reproject.GUIDE_OFFSETS
    assert len(offs) == 24 == len(set(offs)) and (0, 0) not in offs and all(abs(dx) <= 2 and abs(dy) <= 2 for dx, dy in offs)
    assert offs[:4] == [(0, -1), (-1, 0), (1, 0), (0, 1)] and offs[-1] == (2, 2)
    keys = [(dx * dx + dy * dy, dy, dx) for dx, dy in offs]
    assert keys == sorted(keys)
