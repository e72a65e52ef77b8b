"""tools/denoise_spatial_time.py [workload=c3] [calls=50] — GPU box: what the spatial variance estimate (include/hrcore_denoise_spatial.h)
costs beside hr_denoise on the same frame in the same process.

Renders the workload (1920 x 1080) with both AOV masks on and times hr_denoise and hr_denoise_spatial into a device tensor with HIP
events on the context's stream, default parameters: 5 warm-up calls, then `calls` timed calls one by one (an event pair around each),
the two entry points alternating call by call; medians.  Two frames: after 1 pass (every pixel is a spatial pixel: every workgroup
stages its tile and runs both tap passes) and after 16 passes (none is: every workgroup takes the early out, a streaming copy of cv)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
torch.cuda.init()
sc = bench.build_scene(wl, 0, 0, 32)
eng = core.create_engine(stream=torch.cuda.current_stream().cuda_stream)
sc.apply(eng)
eng.set_aovs(ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS)
out = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
print(f"{wl} {sc.width}x{sc.height}, default parameters; {calls} calls each after 5 warm-ups, alternating, medians (ms)")
done = 0
for passes in (1, 16):
    for i in range(done, passes):
        eng.render_pass(sc.options.pass_params(i))
    done = passes
    eng.flush()
    eng.synchronize()
    _, res = eng.denoise_spatial(with_result=True)
    fns = {"hr_denoise": lambda: eng.denoise_to_device(out.data_ptr()), "hr_denoise_spatial": lambda: eng.denoise_spatial_to_device(out.data_ptr())}
    ms = {k: [] for k in fns}
    for _ in range(5):
        for fn in fns.values():
            fn()
    for _ in range(calls):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    a, b = statistics.median(ms["hr_denoise"]), statistics.median(ms["hr_denoise_spatial"])
    print(f"after {passes:2d} passes ({res['spatial_pixels']} spatial pixels, {res['estimated_pixels']} estimated): hr_denoise {a:.4f}  hr_denoise_spatial {b:.4f}"
          f"  difference {b - a:+.4f} ({(b - a) / a:+.1%})   [min {min(ms['hr_denoise']):.4f} / {min(ms['hr_denoise_spatial']):.4f}]")
eng.close()
