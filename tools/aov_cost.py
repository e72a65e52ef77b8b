"""tools/aov_cost.py [workload=c3] [passes=128] [rounds=2] — GPU box: what AOVs (include/hrcore_aov.h) cost.  For AOVs off, HR_AOV_SURFACE and
HR_AOV_SURFACE | HR_AOV_MOMENTS, in alternation: ms per pass over `passes` passes (after a warm-up of 32 that fills the pipeline and allocates
the pass slots, then hr_clear) and the device memory the context holds after the run beyond the scene (hipMemGetInfo through torch, as
tools/mem_probe.py measures it)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from heatray_amd import _ffi as ffi
from heatray_amd import core

wl = sys.argv[1] if len(sys.argv) > 1 else "c3"
passes = int(sys.argv[2]) if len(sys.argv) > 2 else 128
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 2
MODES = (("off", 0), ("SURFACE", ffi.HR_AOV_SURFACE), ("SURFACE|MOMENTS", ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS))
torch.cuda.init()
sc = bench.build_scene(wl, 0, 0, max(32, passes))
res = {name: [] for name, _ in MODES}
mem = {}
for r in range(rounds):
    for name, mask in MODES:
        torch.cuda.synchronize()
        free0, _ = torch.cuda.mem_get_info()
        e = core.create_engine(stream=torch.cuda.current_stream().cuda_stream)
        sc.apply(e)
        if mask:
            e.set_aovs(mask)
        free1, _ = torch.cuda.mem_get_info()
        for i in range(32):
            e.render_pass(sc.options.pass_params(i))
        e.clear()
        e.synchronize()
        t0 = time.perf_counter()
        for i in range(passes):
            e.render_pass(sc.options.pass_params(i))
        e.flush()
        e.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / passes
        free2, _ = torch.cuda.mem_get_info()
        res[name].append(ms)
        mem[name] = ((free0 - free1) / 2**20, (free1 - free2) / 2**20)
        e.close()
        print(f"round {r} {name:16s}: {ms:.4f} ms/pass", flush=True)
base = min(res["off"])
for name, _ in MODES:
    best = min(res[name])
    print(f"{wl} {sc.width}x{sc.height}, {passes} passes, AOVs {name:16s}: best {best:.4f} ms/pass ({100.0 * (best / base - 1.0):+.2f} % vs off), "
          f"runs {[round(v, 4) for v in res[name]]}; device memory: scene + frame + planes {mem[name][0]:.0f} MiB, pass pipeline {mem[name][1]:.0f} MiB")
