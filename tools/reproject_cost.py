"""tools/reproject_cost.py [workload=c3] [passes=16] [calls=50] [out=profiles/reproject_cost.txt] — GPU box: what the progressive history merge and the preview
(include/hrcore_reproject.h) cost.

Renders `passes` passes of the workload (1920 x 1080) with both AOV masks on and captures them, orbits the camera by 0.05 rad about the
focus point, then times with HIP events on the context's stream, 5 warm-up calls and `calls` timed calls each (the median is reported):
  hr_reproject_merge, 1/9 sampled   every call is: clear, the first sub-pass of interactive mode, flush + synchronise, then the events
                                    around the merge alone (the zeroing of the examined words and of five counters, the kernel, the
                                    read-back of 40 bytes)
  hr_reproject_merge, full frame    beside hr_history_merge in the same process, the two legs alternating call by call: clear, one pass,
                                    flush + synchronise, the events around the merge
  hr_reproject_preview, 1/9 sampled after the first sub-pass and its merge, back to back into device memory on the context's stream (it
                                    changes nothing, so no clear between the calls); events around all the calls
Each call of either entry point completes the enqueued passes first; here the context is drained before the events, so the times are the
kernels' and their copies' — what a caller pays on top is the pipeline's fill and drain (hr_adaptive_update).
The lines go to stdout and, appended, to `out`."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 16
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "reproject_cost.txt")
WARM = 5
lines = []
torch.cuda.init()
sc = bench.build_scene(wl, 0, 0, max(32, passes))
eng = core.create_engine(stream=torch.cuda.current_stream().cuda_stream)
sc.apply(eng)
eng.set_aovs(ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS)
for i in range(32):  # warm-up: fills the pipeline, allocates the pass slots
    eng.render_pass(sc.options.pass_params(i))
eng.clear()
eng.synchronize()
t0 = time.perf_counter()
for i in range(passes):
    eng.render_pass(sc.options.pass_params(i))
eng.flush()
eng.synchronize()
pass_ms = (time.perf_counter() - t0) * 1e3 / passes
eng.history_capture(sc.options.pass_params(0))

# an orbit by 0.05 rad about the focus point, as a viewer's drag makes it
v = np.asarray(sc.options.view_matrix, np.float64)
target = v[:3, 3] - v[:3, 2] * sc.options.focus_distance
c, s = math.cos(0.05), math.sin(0.05)
rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
to, back = np.eye(4), np.eye(4)
to[:3, 3], back[:3, 3] = -target, target
sc.options.view_matrix = (back @ rot @ to @ v).astype(np.float32)
new_cam = sc.options.pass_params(0)
px = sc.width * sc.height


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), r


def fresh(pp):
    eng.clear()
    eng.render_pass(pp)
    eng.flush()
    eng.synchronize()


def median(v):
    return sorted(v)[len(v) // 2]


# the full frame: the progressive merge beside hr_history_merge, alternating
full = {"reproject": [], "history": []}
res = {}
for k in range(WARM + calls):
    for leg, call in (("reproject", lambda: eng.reproject_merge(new_cam)), ("history", lambda: eng.history_merge(new_cam))):
        fresh(new_cam)
        ms, res[leg] = timed(call)
        if k >= WARM:
            full[leg].append(ms)
assert {k: res["reproject"][k] for k in res["history"]} == res["history"], res

# after the first sub-pass of interactive mode
sc.options.enable_interactive_mode = True
sub0 = sc.options.pass_params(0, current_block_pixel=(0, 0))
ninth = []
for k in range(WARM + calls):
    fresh(sub0)
    ms, res["ninth"] = timed(lambda: eng.reproject_merge(new_cam))
    if k >= WARM:
        ninth.append(ms)
out = torch.zeros((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
for _ in range(WARM):
    eng.reproject_preview_to_device(out.data_ptr(), new_cam)
eng.synchronize()
preview_ms = timed(lambda: [eng.reproject_preview_to_device(out.data_ptr(), new_cam) for _ in range(calls)])[0] / calls
_, counts = eng.reproject_preview(new_cam)

lines.append(f"{wl} {sc.width}x{sc.height}, history of {passes} passes, orbit 0.05; one rendered pass: {pass_ms:.3f} ms; {calls} calls after {WARM} warm-ups, medians (best)")
r = res["reproject"]
lines.append(f"full frame ({r['reused_pixels'] / px:.1%} of the pixels reused), legs alternating: hr_reproject_merge {median(full['reproject']):.4f} ({min(full['reproject']):.4f}) ms, "
      f"hr_history_merge {median(full['history']):.4f} ({min(full['history']):.4f}) ms per call: ratio {median(full['reproject']) / median(full['history']):.3f}; "
      f"{median(full['reproject']) / pass_ms:.4f} of one pass")
r = res["ninth"]
lines.append(f"after the first sub-pass ({r['examined_pixels'] / px:.1%} of the pixels sampled, {r['reused_pixels'] / max(1, r['examined_pixels']):.1%} of them reused): "
      f"hr_reproject_merge {median(ninth):.4f} ({min(ninth):.4f}) ms per call; {median(ninth) / pass_ms:.4f} of one pass")
lines.append(f"after the first sub-pass: hr_reproject_preview {preview_ms:.4f} ms per call (mean of back-to-back calls; own {counts['own_pixels'] / px:.1%}, "
      f"previewed {counts['previewed_pixels'] / px:.1%}, empty {counts['empty_pixels'] / px:.1%} of the pixels); {preview_ms / pass_ms:.4f} of one pass")
eng.close()
print("\n".join(lines))
with open(out_path, "a") as f:
    f.write("\n".join(lines) + "\n")
