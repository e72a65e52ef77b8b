"""The progressive history merge and the preview of unsampled pixels (include/hrcore_reproject.h) restated in numpy float32, operation
for operation — `reference_merge_progressive` and `reference_preview` give the bits the device kernels (heatray_amd/csrc/hr_reproject.h)
give — and a small driver that makes the sequence a viewer makes when its camera moves in interactive mode.

    eng.set_aovs(HR_AOV_SURFACE | HR_AOV_MOMENTS); eng.clear()
    ... render with options.view_matrix = old ...
    def show(k, result):
        image, counts = eng.reproject_preview(options.pass_params(0))       # H x W x 4, alpha 1 where there is something to show
    reproject.move_camera_interactive(eng, options, new_view_matrix, sub_passes=9, on_sub_pass=show)

The limits (the header has them in full): everything history reprojection is limited by; a previewed pixel is biased history with no
sample of the new view in it; the guide is at most two pixels away, so a pixel farther than that from every sample stays empty.
"""
import numpy as np

from . import history
from .history import F, PLANES, _dot, _finite, _ray_x, _ray_y, cameras, default_params

GUIDE_NONE, GUIDE_SKY, GUIDE_SURFACE = 0, 1, 2

# the 24 offsets (dx, dy) with |dx| <= 2, |dy| <= 2 without (0, 0), in ascending order of (dx * dx + dy * dy, dy, dx)
GUIDE_OFFSETS = sorted(((dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if (dx, dy) != (0, 0)), key=lambda o: (o[0] * o[0] + o[1] * o[1], o[1], o[0]))


def reference_merge_progressive(history_planes, old_pass_params, frame, planes, new_pass_params, examined, params=None):
    """What hr_reproject_merge leaves: (frame, planes, examined, result).  `examined` is the H x W bool map of the bits before the call.
    MERGE (history.reference_merge) is committed where ~examined & (F.a > 0) and nowhere else; it reads nothing but the pixel's own
    four values and the immutable history, so committing a subset is exact.  result holds the call's own reused_pixels,
    rejected_pixels and history_samples, and pending_pixels / examined_pixels after it."""
    Fr = np.ascontiguousarray(frame, F)
    E = np.asarray(examined, bool)
    todo = ~E & (Fr[..., 3] > 0)
    masked = Fr.copy()
    masked[~todo] = F(0.0)  # (a pixel without a sample is neither changed nor counted by MERGE: that is how the others are left out)
    out_frame, out_planes, res = history.reference_merge(history_planes, old_pass_params, masked, planes, new_pass_params, params)
    out_frame[~todo] = Fr[~todo]
    now = E | todo
    result = {"reused_pixels": res["reused_pixels"], "rejected_pixels": res["rejected_pixels"], "history_samples": res["history_samples"],
              "pending_pixels": int((~now).sum()), "examined_pixels": int(now.sum()), "nh": res["nh"]}
    return out_frame, out_planes, now, result


def reference_guides(frame, planes):
    """hr_reproject.h's rpGuide per pixel: (class H x W: 0 unsampled, 1 sky, 2 surface; record H x W x 4: unit normal, mean depth)"""
    Fr = np.ascontiguousarray(frame, F)
    A, G = (np.ascontiguousarray(planes[k], F) for k in PLANES[:2])
    with np.errstate(all="ignore"):
        n = Fr[..., 3]
        have = n > 0
        surf = have & (A[..., 3] / n >= F(0.5))
        l2 = _dot(G[..., 0], G[..., 1], G[..., 2], G[..., 0], G[..., 1], G[..., 2])
        l = np.sqrt(l2)
        N = np.where((l2 > 0)[..., None], G[..., :3] / l[..., None], F(0.0))
        rec = np.concatenate([N, (G[..., 3] / A[..., 3])[..., None]], -1).astype(F)
        rec[~surf] = F(0.0)
    cls = np.where(surf, GUIDE_SURFACE, np.where(have, GUIDE_SKY, GUIDE_NONE)).astype(np.int32)
    return cls, rec


def reference_preview(history_planes, old_pass_params, frame, planes, new_pass_params, params=None):
    """What hr_reproject_preview writes: (image H x W x 4 float32, {"own_pixels", "previewed_pixels", "empty_pixels"}) — hr_reproject.h's
    rpOwn, rpFindGuide and rpPreviewFromGuide per pixel.  The inputs are not changed."""
    p = params if params is not None else default_params()
    cam = cameras(old_pass_params, new_pass_params)
    Hs = np.ascontiguousarray(history_planes, F)
    Fr = np.ascontiguousarray(frame, F)
    H, W = Fr.shape[:2]
    Wf, Hf = F(W), F(H)
    R, O, t = cam["R"], cam["O"], cam["t"]
    ncos, ptol, minw = F(p.normal_cos), F(p.plane_tol), F(p.min_weight)
    y, x = np.mgrid[0:H, 0:W]
    gcls, grec = reference_guides(Fr, planes)
    own = Fr[..., 3] > 0
    # the first guide in the contract's order
    cls = np.zeros((H, W), np.int32)
    gx, gy = x.copy(), y.copy()
    rec = np.zeros((H, W, 4), F)
    for dx, dy in GUIDE_OFFSETS:
        ax, ay = x + dx, y + dy
        inside = (ax >= 0) & (ax < W) & (ay >= 0) & (ay < H)
        cx_, cy_ = np.clip(ax, 0, W - 1), np.clip(ay, 0, H - 1)
        take = (cls == GUIDE_NONE) & inside & (gcls[cy_, cx_] != GUIDE_NONE)
        cls = np.where(take, gcls[cy_, cx_], cls)
        gx, gy = np.where(take, ax, gx), np.where(take, ay, gy)
        rec = np.where(take[..., None], grec[cy_, cx_], rec)
    with np.errstate(all="ignore"):
        ok = cls != GUIDE_NONE
        surf = cls == GUIDE_SURFACE
        cx, cy, cz = _ray_x(x, Wf, cam["aspect_new"], cam["fov_new"]), _ray_y(y, Hf, cam["fov_new"]), F(-1.0)
        rc = [((R[i, 0] * cx + R[i, 1] * cy) + R[i, 2] * cz).astype(F) for i in range(3)]
        N = [rec[..., k] for k in range(3)]
        gcx, gcy = _ray_x(gx, Wf, cam["aspect_new"], cam["fov_new"]), _ray_y(gy, Hf, cam["fov_new"])
        rcg = [((R[i, 0] * gcx + R[i, 1] * gcy) + R[i, 2] * cz).astype(F) for i in range(3)]
        Nq = [np.where(surf, _dot(O[i, 0], O[i, 1], O[i, 2], N[0], N[1], N[2]), F(0.0)).astype(F) for i in range(3)]
        sd = ((rec[..., 3] * _dot(Nq[0], Nq[1], Nq[2], rcg[0], rcg[1], rcg[2])) / _dot(Nq[0], Nq[1], Nq[2], rc[0], rc[1], rc[2])).astype(F)
        ok &= ~surf | ((sd > 0) & (sd < F(np.inf)))
        q = [np.where(surf, sd * rc[i] + t[i], rc[i]).astype(F) for i in range(3)]
        z = -q[2]
        ok &= z > 0
        sx = (((q[0] / z) / cam["ax_old"] + F(1.0)) * F(0.5)) * Wf
        sy = (((q[1] / z) / cam["fov_old"] + F(1.0)) * F(0.5)) * Hf
        ok &= (sx >= F(-1.0)) & (sx <= Wf + F(1.0)) & (sy >= F(-1.0)) & (sy <= Hf + F(1.0))
        fx = np.where(ok, sx - F(0.5), F(0.0)).astype(F)
        fy = np.where(ok, sy - F(0.5), F(0.0)).astype(F)
        x0f, y0f = np.floor(fx), np.floor(fy)
        wx, wy = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tol = ptol * z
        wsum = np.zeros((H, W), F)
        hs = np.zeros((H, W, 3), F)
        for k in range(4):
            tx, ty = x0 + (k & 1), y0 + (k >> 1)
            w = (wx if k & 1 else F(1.0) - wx) * (wy if k >> 1 else F(1.0) - wy)
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            ux, uy = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            h0, h2 = Hs[0, uy, ux], Hs[2, uy, ux]
            use = ok & inside & (h0[..., 3] > 0) & (_finite(h2[..., 3]) == surf)
            nd = _dot(N[0], N[1], N[2], h2[..., 0], h2[..., 1], h2[..., 2])
            px = h2[..., 3] * _ray_x(ux, Wf, cam["aspect_old"], cam["fov_old"])
            py = h2[..., 3] * _ray_y(uy, Hf, cam["fov_old"])
            pz = h2[..., 3] * F(-1.0)
            pd = np.abs(_dot(Nq[0], Nq[1], Nq[2], px - q[0], py - q[1], pz - q[2]))
            use &= ~surf | ((nd >= ncos) & (pd <= tol))
            wsum = np.where(use, wsum + w, wsum).astype(F)
            hs = np.where(use[..., None], hs + w[..., None] * h0[..., :3], hs).astype(F)
        ok &= ~(wsum < minw)
        previewed = ok & ~own
        image = np.zeros((H, W, 4), F)
        image[..., :3] = np.where(own[..., None], Fr[..., :3] / Fr[..., 3:], np.where(previewed[..., None], hs / wsum[..., None], F(0.0)))
        image[..., 3] = np.where(own | previewed, F(1.0), F(0.0))
    result = {"own_pixels": int(own.sum()), "previewed_pixels": int(previewed.sum()), "empty_pixels": int((~own & ~previewed).sum())}
    return image, result


def sub_pass_pixel(k):
    """the block pixel (x, y) of sub-pass k of the 3 x 3 walk"""
    return (k % 3, (k // 3) % 3)


def move_camera_interactive(eng, options, new_view_matrix, sub_passes=9, params=None, on_sub_pass=None, sample_index=0):
    """The sequence a viewer makes when its camera moves in interactive mode: capture the frame rendered so far with `options` (a
    scenes.RenderOptions) as it stands, clear, set options.view_matrix = new_view_matrix and options.enable_interactive_mode, then for
    each of `sub_passes` sub-passes of the 3 x 3 walk render it and call reproject_merge.  on_sub_pass(k, result) is called after each
    merge and may ask for a preview (eng.reproject_preview) or a display.  The engine needs HR_AOV_SURFACE | HR_AOV_MOMENTS enabled
    before the captured frame's first pass.  Returns the list of the merges' result dicts."""
    if sub_passes < 1:
        raise ValueError("move_camera_interactive: the new view needs at least one sub-pass before a merge (its planes are the guides)")
    eng.history_capture(options.pass_params(0))
    eng.clear()
    options.view_matrix = np.asarray(new_view_matrix, dtype=F)
    options.enable_interactive_mode = True
    results = []
    for k in range(sub_passes):
        eng.render_pass(options.pass_params(sample_index, current_block_pixel=sub_pass_pixel(k)))
        r = eng.reproject_merge(options.pass_params(sample_index), params)
        results.append(r)
        if on_sub_pass is not None:
            on_sub_pass(k, r)
    return results
