"""tools/metric_cost.py [rounds=5] [reps=200] — GPU box: what the convergence metric costs (include/hrcore_metric.h).
tools/metric_cost.py trace | kernels DIR — the kernels alone, from a kernel trace (below).

On a flushed and synchronised context with c3's frame (1920 x 1080, 12 passes) and a kept device copy of its 8-pass frame as the
reference, on a stream of its own, after a warm-up, legs alternating inside each round.  Both legs wait for their number, so a leg is
`reps` calls timed on the host's clock, printed as ms per call:

  (b)  Engine.metric_compare(reference)                       zeroing 4 KB, k_metric_accumulate<COMPARE>, the fetch of 4 KB, the fold
  (bf) (bn) the same with a flat pair (every term in one bin) and a noise pair (terms spread over the bins) as device images
  (c)  Engine.readback() + convergence.rel_l2 on the host     the path it replaces: 33 MB to the host, normalised and summed in binary64

Printed: every round, the best, the spread of (c) between rounds, (c) / (b) of the same round.  The acceptance condition is (b) < (c).

The kernels alone come from the kernel trace, as in tools/exposure_cost.py:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python tools/metric_cost.py trace
    python tools/metric_cost.py kernels DIR

`trace` runs, 40 times each after 5 warm-up calls of each, in this order: exposure_meter of the frame ((a): k_exposure_hist reads one
image), metric_compare of the frame, of the flat pair, of the noise pair ((b): k_metric_accumulate reads two images and does six 64-bit
LDS adds per pixel against one 32-bit add in (a)); `kernels` reads the dispatches in start order, drops the warm-up and prints mean, least
and greatest per case, (b) / (a), and flat / noise."""
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED = 5, 40
CASES = ("rendered c3 frame against its 8-pass frame", "flat pair, every term in one bin", "noise pair, terms over the bins")


def kernels(directory):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no *kernel_trace.csv under {directory}"
    rows = [r for f in files for r in csv.DictReader(open(f))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = lambda kernel: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if kernel in r["Kernel_Name"]]
    hist = us("k_exposure_hist")
    assert len(hist) == WARM + TIMED, len(hist)
    hist = hist[WARM:]
    a = sum(hist) / len(hist)
    print(f"(a) k_exposure_hist on the rendered c3 frame: {len(hist)} dispatches, mean {a:.2f} us, least {min(hist):.2f}, greatest {max(hist):.2f}")
    acc = us("k_metric_accumulate")
    assert len(acc) == (WARM + TIMED) * len(CASES), len(acc)
    means = []
    for i, name in enumerate(CASES):
        v = acc[i * (WARM + TIMED) + WARM:(i + 1) * (WARM + TIMED)]
        means.append(sum(v) / len(v))
        print(f"(b) k_metric_accumulate<COMPARE> on the {name}: {len(v)} dispatches, mean {means[-1]:.2f} us, least {min(v):.2f}, greatest {max(v):.2f}")
    mb = 2 * 1920 * 1080 * 16 / 1e6
    print(f"(b) / (a) on the rendered frame = {means[0] / a:.3f} (the traffic alone: 2); flat / noise = {means[1] / means[2]:.3f}; "
          f"the two images are {mb:.1f} MB: {mb * 1e3 / means[0]:.0f} GB/s on the rendered frame")


if len(sys.argv) > 2 and sys.argv[1] == "kernels":
    kernels(sys.argv[2])
    sys.exit(0)

import numpy as np
import torch

import bench
from heatray_amd import convergence, core

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 and not trace else 200

sc = bench.build_scene("c3", 0, 0, 32)
W, H = sc.width, sc.height
stream = torch.cuda.Stream()
eng = core.create_engine(stream=stream.cuda_stream)
sc.apply(eng)
for i in range(8):
    eng.render_pass(sc.options.pass_params(i))
ref_host = eng.readback()
ref_img = convergence.normalised(ref_host)
for i in range(8, 12):
    eng.render_pass(sc.options.pass_params(i))
eng.flush()
eng.synchronize()

rng = np.random.default_rng(1)
flat_i, flat_r = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
flat_i[...], flat_r[...] = (2.5, 2.5, 2.5, 4.0), (1.0, 1.0, 1.0, 2.0)  # d = 2^-3, cR = 2^-1 in every channel
noise_i, noise_r = np.ones((H, W, 4), np.float32), np.ones((H, W, 4), np.float32)
noise_i[..., :3] = np.exp2(rng.uniform(-16, 16, (H, W, 3))).astype(np.float32)  # a lane's neighbours are in other bins
noise_r[..., :3] = np.exp2(rng.uniform(-16, 16, (H, W, 3))).astype(np.float32)
with torch.cuda.stream(stream):
    t_ref = torch.from_numpy(ref_host).to("cuda:0")
    t_fi, t_fr, t_ni, t_nr = (torch.from_numpy(v).to("cuda:0") for v in (flat_i, flat_r, noise_i, noise_r))
stream.synchronize()

COMPARES = (lambda: eng.metric_compare(t_ref.data_ptr()), lambda: eng.metric_compare(t_fr.data_ptr(), image=t_fi.data_ptr()),
            lambda: eng.metric_compare(t_nr.data_ptr(), image=t_ni.data_ptr()))

if trace:
    for _ in range(WARM + TIMED):
        eng.exposure_meter()
    measured = []
    for call in COMPARES:
        for _ in range(WARM + TIMED):
            r = call()
        measured.append(r)
    for name, r in zip(CASES, measured):
        print(f"{name}: value {r['value']:.9g}, counted {r['counted']}, differing {r['differing']}, nonfinite {r['nonfinite']}")
    eng.close()
    sys.exit(0)

LEGS = {
    "(b)  metric_compare, the frame": COMPARES[0],
    "(bf) metric_compare, flat pair": COMPARES[1],
    "(bn) metric_compare, noise pair": COMPARES[2],
    "(c)  readback + rel_l2 on the host": lambda: convergence.rel_l2(convergence.normalised(eng.readback()), ref_img),
}


def timed(call, n):
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        call()
    return (time.perf_counter() - t0) * 1e3 / n


for call in LEGS.values():  # warm-up: code objects, the buffers
    for _ in range(3):
        call()
res = {name: [] for name in LEGS}
for _ in range(rounds):
    for name, call in LEGS.items():
        res[name].append(timed(call, reps if name.startswith("(b") else max(2, reps // 10)))
b, c = res["(b)  metric_compare, the frame"], res["(c)  readback + rel_l2 on the host"]
print(f"c3 {W}x{H}, calls that wait for their number, host clock, {rounds} rounds, legs alternating; ms per call")
print(f"  spread of (c) between rounds: {min(c):.3f} .. {max(c):.3f} ms ({(max(c) / min(c) - 1) * 100:.2f} %)")
for name, v in res.items():
    print(f"  {name:40s} " + "  ".join(f"{x:.4f}" for x in v) + f"   best {min(v):.4f}")
print("  (c) / (b) round by round: " + "  ".join(f"{y / x:.1f}" for x, y in zip(b, c)) + "   (acceptance: above 1)")
dev, host = COMPARES[0]()["value"], LEGS["(c)  readback + rel_l2 on the host"]()
print(f"  the frame's value: device {dev!r}, host {host!r}, relative difference {abs(dev / host - 1):.3e}")
eng.close()
