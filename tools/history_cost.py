"""tools/history_cost.py [workload=c3] [passes=16] [calls=50] — GPU box: what history reprojection (include/hrcore_history.h) costs.

Renders `passes` passes of the workload (1920 x 1080) with both AOV masks on, then times with HIP events on the context's stream, 5
warm-up calls and `calls` timed calls each:
  hr_history_capture  back to back (it does not wait for the device): events around all the calls
  hr_history_merge    one per hr_clear, so every call is: clear, one pass of the orbited camera, flush + synchronise, then the events around
                      the merge alone (the zeroing of its three counters, the kernel, the read-back of 24 bytes)
Each beside its unique bytes over that time — capture: 64 B read + 48 B written per pixel; merge: 64 B read + 64 B written per reused pixel
of its own plus at most 48 B of history (every history value is tapped by about four pixels, from cache after the first) — and beside one
rendered pass of the same workload."""
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
old_cam = sc.options.pass_params(0)


def events():
    return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


for _ in range(5):
    eng.history_capture(old_cam)
e0, e1 = events()
e0.record()
for _ in range(calls):
    eng.history_capture(old_cam)
e1.record()
e1.synchronize()
capture_ms = e0.elapsed_time(e1) / calls

# an orbit by 0.05 rad about the focus point, as a viewer's drag makes it
v = np.asarray(sc.options.view_matrix, np.float64)
target = v[:3, 3] - v[:3, 2] * sc.options.focus_distance
c, s = math.cos(0.05), math.sin(0.05)
rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
to, back = np.eye(4), np.eye(4)
to[:3, 3], back[:3, 3] = -target, target
sc.options.view_matrix = (back @ rot @ to @ v).astype(np.float32)
new_cam = sc.options.pass_params(0)
merge_ms, res = [], None
for k in range(5 + calls):
    eng.clear()
    eng.render_pass(new_cam)
    eng.flush()
    eng.synchronize()
    e0, e1 = events()
    e0.record()
    res = eng.history_merge(new_cam)
    e1.record()
    e1.synchronize()
    if k >= 5:
        merge_ms.append(e0.elapsed_time(e1))
merge_ms.sort()
px = sc.width * sc.height
merge = merge_ms[len(merge_ms) // 2]
own = 64 * px + 64 * res["reused_pixels"]
print(f"{wl} {sc.width}x{sc.height}, history of {passes} passes; one rendered pass: {pass_ms:.3f} ms; {calls} calls after 5 warm-ups")
print(f"hr_history_capture: {capture_ms:.4f} ms per call (mean of back-to-back calls); 112 B per pixel unique = {112 * px / (capture_ms * 1e-3) / 1e12:.2f} TB/s; "
      f"{capture_ms / pass_ms:.4f} of one pass")
print(f"hr_history_merge (orbit 0.05, {res['reused_pixels'] / px:.1%} of the pixels reused): median {merge:.4f} ms, best {merge_ms[0]:.4f} ms per call "
      f"(counters zeroed + kernel + 24-byte read-back); own pixels {own / px:.0f} B per pixel + 48 B of history unique = "
      f"{(own + 48 * px) / (merge * 1e-3) / 1e12:.2f} TB/s at the median; {merge / pass_ms:.4f} of one pass")
eng.close()
