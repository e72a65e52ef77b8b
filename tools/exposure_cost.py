"""tools/exposure_cost.py [rounds=5] [reps=50] — GPU box: what auto-exposure costs (include/hrcore_exposure.h).
tools/exposure_cost.py trace | kernels DIR — the histogram kernel alone, from a kernel trace (below).

On a flushed and synchronised context with c3's frame (1920 x 1080, 8 passes), on a stream of its own, after a warm-up, legs alternating
inside each round; a leg is `reps` calls back to back between two device events, printed as ms per call:

  (a)  hr_display RGBA8                                             one read of the frame
  (b)  hr_exposure_display RGBA8 of the frame                       zeroing 2 KB, k_exposure_hist, k_exposure_reduce, k_exposure_display
  (bf) (bn) the same with a flat image and with white noise over all 256 bins as device_image (what contention in the bins costs end to end)

Printed: every round, the best, the spread of (a) between rounds (what a difference has to beat), (b) / (a) of the same run.

(c) The histogram kernel alone cannot be enqueued alone through the API, and a device event around a synchronous call times the host's
round trip, so its time comes from the kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/exposure_cost.py trace
    python tools/exposure_cost.py kernels DIR

`trace` meters the rendered frame, the flat image and the noise image 40 times each, in this order, after 5 warm-up meterings of each;
`kernels` reads the dispatches of k_exposure_hist in start order, drops the warm-up and prints mean, least and greatest per image, the
flat-to-noise ratio, and the same for k_exposure_reduce and k_exposure_display where the trace has them."""
import csv
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED = 5, 40
IMAGES = ("rendered c3 frame", "flat image", "white noise over all bins")


def kernels(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {directory}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for kernel in ("k_exposure_hist", "k_exposure_reduce", "k_exposure_display"):
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
        if kernel == "k_exposure_display":
            if us:
                print(f"{kernel}: {len(us)} dispatches, mean {sum(us) / len(us):.2f} us, least {min(us):.2f}, greatest {max(us):.2f}")
            continue
        per = WARM * len(IMAGES) + TIMED * len(IMAGES)
        assert len(us) == per, (kernel, len(us), per)
        us = us[WARM * len(IMAGES):]
        means = []
        for i, name in enumerate(IMAGES):
            v = us[i * TIMED:(i + 1) * TIMED]
            means.append(sum(v) / len(v))
            print(f"{kernel} on the {name}: {len(v)} dispatches, mean {means[-1]:.2f} us, least {min(v):.2f}, greatest {max(v):.2f}")
        if kernel == "k_exposure_hist":
            print(f"k_exposure_hist: flat / noise = {means[1] / means[2]:.3f} (expected: at most 2), rendered / noise = {means[0] / means[2]:.3f}; "
                  f"the frame is {1920 * 1080 * 16 / 1e6:.1f} MB: {1920 * 1080 * 16 / 1e3 / means[0]:.0f} GB/s on the rendered frame")


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    kernels(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 and not trace else 50

sc = bench.build_scene("c3", 0, 0, 32)
W, H = sc.width, sc.height
stream = torch.cuda.Stream()
eng = core.create_engine(stream=stream.cuda_stream)
sc.apply(eng)
for i in range(8):
    eng.render_pass(sc.options.pass_params(i))
eng.flush()
eng.synchronize()

rng = np.random.default_rng(1)
flat = np.zeros((H, W, 4), np.float32)
flat[...] = (2.0, 1.0, 0.5, 4.0)
noise = np.ones((H, W, 4), np.float32)
noise[..., :3] = np.exp2(rng.uniform(-16, 16, (H, W, 1))).astype(np.float32)  # every bin alike: a lane's neighbours are in other bins
with torch.cuda.stream(stream):
    t_flat, t_noise = torch.from_numpy(flat).to("cuda:0"), torch.from_numpy(noise).to("cuda:0")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
stream.synchronize()
display = ffi.display_params()

if trace:
    metered = []
    for n in (WARM, TIMED):
        for image in (None, t_flat.data_ptr(), t_noise.data_ptr()):
            for _ in range(n):
                r = eng.exposure_meter(image=image)
            metered.append(r)
    for name, r in zip(IMAGES, metered[3:]):
        print(f"{name}: counted {r['counted']}, below {r['below']}, above {r['above']}, position {r['position']}, scale {r['scale']:.6g}")
    eng.close()
    sys.exit(0)

LEGS = {
    "(a)  hr_display": lambda: eng.display_device(out.data_ptr(), display),
    "(b)  hr_exposure_display, the frame": lambda: eng.exposure_display(out.data_ptr(), display),
    "(bf) hr_exposure_display, flat image": lambda: eng.exposure_display(out.data_ptr(), display, image=t_flat.data_ptr()),
    "(bn) hr_exposure_display, noise image": lambda: eng.exposure_display(out.data_ptr(), display, image=t_noise.data_ptr()),
}


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    eng.synchronize()
    e0.record(stream)
    for _ in range(reps):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


for call in LEGS.values():  # warm-up: code objects, the meter's buffers
    for _ in range(10):
        call()
eng.synchronize()
res = {name: [] for name in LEGS}
for _ in range(rounds):
    for name, call in LEGS.items():
        res[name].append(timed(call))
a = res["(a)  hr_display"]
print(f"c3 {W}x{H}, RGBA8, {reps} calls per leg between two device events, {rounds} rounds, legs alternating; ms per call")
print(f"  spread of (a) between rounds: {min(a):.4f} .. {max(a):.4f} ms ({(max(a) / min(a) - 1) * 100:.2f} %)")
for name, v in res.items():
    print(f"  {name:40s} " + "  ".join(f"{x:.4f}" for x in v) + f"   best {min(v):.4f} = {min(v) / min(a):.3f} x (a)")
b = res["(b)  hr_exposure_display, the frame"]
print(f"  (b) / (a) round by round: " + "  ".join(f"{y / x:.3f}" for x, y in zip(a, b)) + "   (expected: at most 2.5)")
r = eng.exposure_last()
print(f"  the frame's metering: counted {r['counted']}, below {r['below']}, position {r['position']}, scale {r['scale']:.6g}")
eng.close()
