"""Context groups (include/hrcore_group.h) against a plain context on workload c3 (scenes.triangle_soup(1_000_000, env=True): 1080p,
8 bounces): ms per pass and Mrays/s at 20 and 128 passes, for a plain context and for groups of k = 1 ... n members — over the
visible devices (member i on device i), or with --same-device K, K members on device 0 (the one-device emulation of a K-way split:
the members share one GPU, so this is the cost of the split, not a scaling).  Also the assembly time: device events on the assembly
stream around hr_frame_device_ptr once every pass has completed (members' packs, their peer copies, k_gather_members).

    python tools/group_scaling.py                     # groups over 1 ... every visible device
    python tools/group_scaling.py --same-device 4     # groups of 1 ... 4 members on device 0
    python tools/group_scaling.py --copy-reference    # also 20 device-to-device copies of one frame (33 MB), for a kernel trace

An experiment tool: bench.py measures the project's benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from heatray_amd import core, scenes  # noqa: E402


def run(make, sc, passes, reps, stream):
    eng = make()
    sc.apply(eng)
    for s in range(4):  # warm-up: slot allocation, ray memory, the packet selector's first probe
        eng.render_pass(sc.options.pass_params(s))
    eng.readback()
    times, rays = [], 0
    for _ in range(reps):
        eng.clear()
        eng.synchronize()
        t0 = time.perf_counter()
        for s in range(passes):
            eng.render_pass(sc.options.pass_params(s))
        eng.readback()  # completes every pass (and assembles a group's frame)
        times.append(time.perf_counter() - t0)
        st = eng.stats()
        rays = st.rays_closest + st.rays_any
    out = {"ms_per_pass": 1e3 * statistics.median(times) / passes, "mrays_s": rays / statistics.median(times) / 1e6}
    if hasattr(eng, "group_info") and stream is not None:
        eng.synchronize()
        asm = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.frame_device_ptr()
            e1.record(stream)
            e1.synchronize()
            asm.append(e0.elapsed_time(e1))
        out["assembly_ms"] = statistics.median(asm)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--same-device", type=int, default=0, metavar="K", help="groups of 1..K members, all on device 0")
    ap.add_argument("--passes", default="20,128")
    ap.add_argument("--reps", type=int, default=3, help="timed renders per configuration (median)")
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--copy-reference", action="store_true", help="20 device-to-device copies of one 1080p RGBA32F frame first")
    a = ap.parse_args()
    n_dev = torch.cuda.device_count()
    if n_dev < 1:
        sys.exit("no visible device")
    torch.cuda.init()
    if a.copy_reference:
        src = torch.empty(1080 * 1920 * 4, dtype=torch.float32, device="cuda:0")
        dst = torch.empty_like(src)
        for _ in range(20):
            dst.copy_(src)
        torch.cuda.synchronize()
    sc = scenes.triangle_soup(a.tris, env=True)
    stream = torch.cuda.Stream(device=0)
    if a.same_device:
        groups = [[0] * k for k in range(1, a.same_device + 1)]
    else:
        groups = [list(range(k)) for k in range(1, n_dev + 1)]
    for passes in (int(p) for p in a.passes.split(",")):
        base = run(lambda: core.create_engine(device_id=0), sc, passes, a.reps, None)
        print(json.dumps({"config": "plain", "devices": [0], "passes": passes, **{k: round(v, 4) for k, v in base.items()}}), flush=True)
        for ids in groups:
            r = run(lambda: core.create_group(ids, stream=stream.cuda_stream), sc, passes, a.reps, stream)
            r["vs_plain"] = base["ms_per_pass"] / r["ms_per_pass"]
            print(json.dumps({"config": f"group of {len(ids)}", "devices": ids, "passes": passes, **{k: round(v, 4) for k, v in r.items()}}), flush=True)
    if not a.same_device and n_dev == 1:
        print("(one visible device: scaling over several GPUs is not measured here; --same-device K emulates a K-way split on it)")


if __name__ == "__main__":
    main()
