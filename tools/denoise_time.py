"""tools/denoise_time.py [workload=c3] [passes=16] [calls=50] [rounds=3] — GPU box: what the denoiser (include/hrcore_denoise.h) costs.

Renders `passes` passes of the workload (1920 x 1080) with both AOV masks on, then times hr_denoise into a device tensor with HIP events
on the context's stream: 5 warm-up calls, `calls` timed calls, for every kernel choice (PLAIN / TILED / AUTO) and every iteration count
0 .. 5, the choices alternating inside each round, the best round kept.  The difference between k and k - 1 iterations is what the
iteration at step 2^(k-1) costs (the last iteration of a call also writes the remodulated image instead of the working plane);
0 iterations = prepare + gradient + remodulate.  Also prints the unique bytes an iteration touches over its time and one rendered
pass of the same workload for scale."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core, denoise

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 16
calls = int(sys.argv[3]) if len(sys.argv) > 3 else 50
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
KERNELS = (("plain", ffi.HR_DENOISE_KERNEL_PLAIN), ("tiled", ffi.HR_DENOISE_KERNEL_TILED), ("auto", ffi.HR_DENOISE_KERNEL_AUTO))
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
best = {}
for r in range(rounds):
    for it in range(0, 6):
        for name, kernel in KERNELS:
            p = denoise.default_params()
            p.iterations, p.kernel = it, kernel
            for _ in range(5):
                eng.denoise_to_device(out.data_ptr(), p)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                eng.denoise_to_device(out.data_ptr(), p)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / calls
            best[(name, it)] = min(best.get((name, it), 1e9), ms)
px = sc.width * sc.height
print(f"{wl} {sc.width}x{sc.height} after {passes} passes; one rendered pass: {pass_ms:.3f} ms; {calls} calls after 5 warm-ups, best of {rounds} rounds")
print("total ms per call by iterations:")
for name, _ in KERNELS:
    print(f"  {name:6s} " + "  ".join(f"{it}: {best[(name, it)]:.4f}" for it in range(6)))
print("ms per iteration (difference of consecutive totals), unique bytes per iteration (36 B read + 16 B written per pixel + 4 B gradient) over that time:")
uniq = px * (36 + 16 + 4)
for name, _ in KERNELS:
    d = [best[(name, it)] - best[(name, it - 1)] for it in range(1, 6)]
    print(f"  {name:6s} " + "  ".join(f"step {1 << k}: {v:.4f} ms ({uniq / (v * 1e-3) / 1e12:.2f} TB/s)" for k, v in enumerate(d)))
print(f"prepare + gradient + remodulate (0 iterations): {best[('auto', 0)]:.4f} ms; default call (auto, 5 iterations): {best[('auto', 5)]:.4f} ms = "
      f"{best[('auto', 5)] / pass_ms:.2f} rendered passes")
eng.close()
