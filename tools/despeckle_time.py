"""tools/despeckle_time.py [workload=c3] [passes=16] [calls=50] [rounds=3] — GPU box: what firefly suppression (include/hrcore_despeckle.h) costs.

Renders `passes` passes of the workload (1920 x 1080) with both AOV masks on, then times, with HIP events on the context's stream (5 warm-up
calls, `calls` timed calls, the variants alternating inside each round, the best round kept):
  hr_despeckle of the context's own frame into device tensors, with and without the moments output (k_despeckle and the zeroing of its counters);
  hr_denoise_spatial and hr_despeckle_denoise(spatial) of the same frame, for scale.
Prints each time against the kernel's traffic model (32 B read + 32 B written per pixel, 16 B fewer without the moments output) and the
bandwidth it implies."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 16
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
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
out = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
mom = torch.empty((sc.height, sc.width, 4), dtype=torch.float32, device="cuda:0")
VARIANTS = {
    "despeckle, both outputs": lambda: eng.despeckle_to_device(out.data_ptr(), mom.data_ptr()),
    "despeckle, no moments output": lambda: eng.despeckle_to_device(out.data_ptr()),
    "denoise_spatial": lambda: eng.denoise_spatial_to_device(out.data_ptr()),
    "despeckle_denoise (spatial)": lambda: eng.despeckle_denoise_to_device(out.data_ptr(), spatial=True),
}
best = {}
for r in range(rounds):
    for name, call in VARIANTS.items():
        for _ in range(5):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            call()
        e1.record()
        e1.synchronize()
        best[name] = min(best.get(name, 1e9), e0.elapsed_time(e1) / calls)
result = eng.despeckle_to_device(out.data_ptr(), mom.data_ptr(), with_result=True)
px = sc.width * sc.height
print(f"{wl} {sc.width}x{sc.height} after {passes} passes; one rendered pass: {pass_ms:.3f} ms; {calls} calls after 5 warm-ups, best of {rounds} rounds")
print(f"the frame: {result}")
for name, model in (("despeckle, both outputs", 64), ("despeckle, no moments output", 48)):
    ms = best[name]
    print(f"  {name:30s} {ms:.4f} ms per call; model {model} B per pixel = {px * model / 1e6:.1f} MB: {px * model / (ms * 1e-3) / 1e12:.2f} TB/s")
for name in ("denoise_spatial", "despeckle_denoise (spatial)"):
    print(f"  {name:30s} {best[name]:.4f} ms per call")
print(f"  despeckle_denoise - denoise_spatial = {best['despeckle_denoise (spatial)'] - best['denoise_spatial']:.4f} ms; "
      f"despeckle / denoise_spatial = {best['despeckle, both outputs'] / best['denoise_spatial']:.3f}; despeckle = {best['despeckle, both outputs'] / pass_ms:.4f} rendered passes")
eng.close()
