"""tools/adaptive_cost.py [workload=c3] [passes=128] [rounds=3] — GPU box: what the sample mask and hr_adaptive_update cost
(include/hrcore_adaptive.h).

For HR_TUNE packets=0 and the default (one context each, in this process), renders `passes` passes of the workload (1920 x 1080) under:
no mask; a mask of all ones; block-random masks (whole 8 x 8 blocks) with 50 %, 10 % and 1 % of the pixels set.  The legs alternate inside
each round after a warm-up of 32 passes; a leg is timed by the host clock from the first hr_render_pass to the end of hr_synchronize.
Printed: ms per pass of every round, the best, and the spread of the no-mask leg between rounds (what a difference has to beat).
Then, on a flushed and synchronised context: one hr_adaptive_update (host clock around the call, which ends in a synchronise: kernels +
the result's read-back), and what the drain an update implies costs: `passes` passes in one go against the same passes with a
flush + synchronise every 1, 2 and 4 batches."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import adaptive, core, scenes

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 128
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3

sc = bench.build_scene(wl, 0, 0, max(32, passes))
W, H = sc.width, sc.height


def block_mask(share, seed):
    nbx, nby = (W + 7) // 8, (H + 7) // 8
    u = scenes.SplitMix64(seed).uniform((nby, nbx))
    y, x = np.mgrid[0:H, 0:W]
    return (u < share)[y // 8, x // 8].astype(np.uint8)


LEGS = [("no mask", None), ("all ones", np.ones((H, W), np.uint8)), ("50 %", block_mask(0.5, 1)), ("10 %", block_mask(0.1, 2)), ("1 %", block_mask(0.01, 3))]


def timed(eng, n, sync_every=0):
    eng.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        eng.render_pass(sc.options.pass_params(i))
        if sync_every and (i + 1) % sync_every == 0:
            eng.flush()
            eng.synchronize()
    eng.flush()
    eng.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


print(f"{wl} {W}x{H}, {passes} passes per leg, {rounds} rounds, legs alternating; ms per pass")
for tune in ("packets=0", None):
    if tune:
        os.environ["HR_TUNE"] = tune
    else:
        os.environ.pop("HR_TUNE", None)
    eng = core.create_engine()
    sc.apply(eng)
    eng.set_aovs(ffi.HR_AOV_MOMENTS)
    for i in range(32):  # warm-up: fills the pipeline, allocates the pass slots
        eng.render_pass(sc.options.pass_params(i))
    eng.synchronize()
    res = {name: [] for name, _ in LEGS}
    for r in range(rounds):
        for name, mask in LEGS:
            eng.clear()
            eng.set_sample_mask(mask)
            set_px = W * H if mask is None else int(mask.sum())
            res[name].append(timed(eng, passes))
            assert eng.stats().paths == set_px * passes, (name, eng.stats().paths, set_px * passes)
    base = res["no mask"]
    print(f"HR_TUNE={tune or '(default)'}: camera rays as packets at the end: {eng.kernel_times()['camera_packets'][0]}")
    print(f"  spread of the no-mask leg between rounds: {min(base):.3f} .. {max(base):.3f} ms ({(max(base) / min(base) - 1) * 100:.2f} %)")
    for name, mask in LEGS:
        v = res[name]
        share = 1.0 if mask is None else mask.mean()
        print(f"  {name:9s} ({share * 100:5.1f} % of the pixels): " + "  ".join(f"{x:.3f}" for x in v) + f"   best {min(v):.3f} = {min(v) / min(base):.3f} x no mask")
    if tune is None:
        # one update on a flushed, synchronised context (the frame of the last leg is as good as any: the kernels' work does not depend on it)
        eng.clear()
        eng.set_sample_mask(None)
        pass_ms = timed(eng, passes)
        for _ in range(5):
            eng.adaptive_update(install=False)
        for install in (False, True):
            t = []
            for _ in range(50):
                eng.synchronize()
                t0 = time.perf_counter()
                eng.adaptive_update(install=install)
                t.append((time.perf_counter() - t0) * 1e3)
            t.sort()
            print(f"  hr_adaptive_update(install={int(install)}) on a drained context: median {t[len(t) // 2]:.3f} ms, best {t[0]:.3f} ms per call "
                  f"(kernels + result read-back + synchronise) = {t[len(t) // 2] / pass_ms:.3f} of one pass ({pass_ms:.3f} ms)")
        eng.set_sample_mask(None)
        B = eng.pass_batch(sc.options.max_ray_depth)
        for every in (B, 2 * B, 4 * B):
            a, b = [], []
            for r in range(rounds):
                eng.clear()
                a.append(timed(eng, passes))
                eng.clear()
                b.append(timed(eng, passes, sync_every=every))
            drains = passes // every
            print(f"  a drain every {every} passes (batch {B}): {min(b):.3f} against {min(a):.3f} ms per pass: {(min(b) - min(a)) * passes / max(drains, 1):.3f} ms per drain, "
                  f"{(min(b) / min(a) - 1) * 100:.1f} % of the render")
    eng.close()
