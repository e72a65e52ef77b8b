"""tools/motion_rate.py [--passes N] [--calls N] [--out FILE] — what motion reprojection (include/hrcore_motion.h) costs on the bench's c3
scene at 1920 x 1080, for a GPU machine.

Renders N passes with both AOV masks on, captures them, takes the snapshot, shifts mesh 0 by a hundredth of the scene's size
(hr_geom_set_transform), commits (a refit) and orbits the camera by 0.05 rad.  Then, with device events on the context's stream, WARM
warm-up calls and `calls` timed calls each, median (min .. max):
  hr_motion_snapshot                  the gather kernel alone (asynchronous: events around `calls` back-to-back calls, per call)
  hr_motion_trace                     beside its yardstick, hr_query_trace of the same 2,073,600 raster-order rays with surface records
                                      (k_query_trace<false, true>: the same walk, the same coherence), the two alternating call by call.
                                      A trace call holds the upload of the mesh table, the zeroing and the read-back of its counters; a
                                      query call the zeroing and the copy of its counters.
  hr_motion_merge                     beside its yardstick, hr_history_merge, alternating: clear, one pass, flush + synchronise, then
                                      the events around the merge.  hr_motion_merge holds a trace; the line gives the call and the call
                                      less the trace's median.
  hr_motion_vectors                   into device memory, `calls` back-to-back calls, per call
Before the parent touches the GPU, a child process under `rocprofv3 --kernel-trace` makes the same calls a few times: the profiler's
kernel durations of k_motion_trace against k_query_trace<false, true> and of k_motion_merge against k_history_merge are the comparison
of the kernels themselves, free of the calls' copies."""
import argparse
import csv
import glob
import math
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

WARM = 3


def setup(passes, stream=None):
    """the engine with a captured history and a snapshot of the old pose, the new pose committed; (eng, sc, new camera, rays)"""
    import bench
    from heatray_amd import _ffi as ffi
    from heatray_amd import core, motion
    sc = bench.build_scene("c3", 0, 0, max(32, passes))
    eng = core.create_engine(stream=stream)
    sc.apply(eng)
    eng.set_aovs(ffi.HR_AOV_SURFACE | ffi.HR_AOV_MOMENTS)
    eng.clear()
    for i in range(passes):
        eng.render_pass(sc.options.pass_params(i))
    eng.history_capture(sc.options.pass_params(0))
    eng.motion_snapshot()
    info = eng.scene_info()
    size = float(np.linalg.norm(np.array(list(info.aabb_max), np.float64) - np.array(list(info.aabb_min), np.float64)))
    world = np.eye(4, dtype=np.float32) if sc.meshes[0].world is None else np.asarray(sc.meshes[0].world, np.float32).reshape(4, 4).copy()
    world[0, 3] += 0.01 * size
    eng.set_transform(0, world)
    eng.commit()
    # an orbit by 0.05 rad about the focus point, as a viewer's drag makes it
    v = np.asarray(sc.options.view_matrix, np.float64)
    target = v[:3, 3] - v[:3, 2] * sc.options.focus_distance
    c, s = math.cos(0.05), math.sin(0.05)
    rot = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1.0]])
    to, back = np.eye(4), np.eye(4)
    to[:3, 3], back[:3, 3] = -target, target
    sc.options.view_matrix = (back @ rot @ to @ v).astype(np.float32)
    new_cam = sc.options.pass_params(0)
    rays = motion.camera_rays(new_cam, sc.width, sc.height)
    return eng, sc, new_cam, rays


def fresh(eng, pp):
    eng.clear()
    eng.render_pass(pp)
    eng.flush()
    eng.synchronize()


def child(passes):
    import torch
    eng, sc, cam, rays = setup(passes)
    dev = torch.device("cuda:0")
    t_o, t_d = torch.from_numpy(np.ascontiguousarray(rays[:, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(rays[:, 3:])).to(dev)
    n = rays.shape[0]
    hits, surf = torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.zeros((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for _ in range(8):
        eng.motion_trace(cam)
        eng.query_to_device(n, t_o.data_ptr(), t_d.data_ptr(), hits_ptr=hits.data_ptr(), surfaces_ptr=surf.data_ptr(), tmin=0.0)
        eng.query_last()
        fresh(eng, cam)
        eng.motion_merge(cam)
        fresh(eng, cam)
        eng.history_merge(cam)
    print("child: done")


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def kernel_times(lines, passes):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        lines.append("kernel times: rocprofv3 not found: not measured")
        return
    d = tempfile.mkdtemp(prefix="hr_mr_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "-d", d, "-o", "mr", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child", "--passes", str(passes)]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=500)
    if r.returncode != 0:
        lines.append(f"kernel times: the profiled child failed (rc {r.returncode}): not measured: " + r.stderr.decode(errors="replace")[-300:])
        return
    dur = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                for key in ("k_motion_snapshot", "k_motion_trace", "k_query_trace", "k_motion_merge", "k_history_merge"):
                    if key in row["Kernel_Name"]:
                        dur.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    shutil.rmtree(d, ignore_errors=True)
    lines.append("kernel durations by rocprofv3 --kernel-trace, one process alternating the calls, the first (warm-up) launch of each dropped:")
    med = {}
    for key, v in sorted(dur.items()):
        v = v[1:] if len(v) > 1 else v
        med[key] = spread(v)
        lines.append(f"  {key:20s} {len(v):3d} launches  median {med[key][0]:8.4f} ms  min {med[key][1]:8.4f}  max {med[key][2]:8.4f}")
    for a, b in (("k_motion_trace", "k_query_trace"), ("k_motion_merge", "k_history_merge")):
        if a in med and b in med:
            lines.append(f"  {a} / {b} (medians): {med[a][0] / med[b][0]:.4f};  spread (max / min) of {a}: {med[a][2] / med[a][1]:.4f}, of {b}: {med[b][2] / med[b][1]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_rate.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.passes)
    lines = []
    kernel_times(lines, args.passes)  # (first: the parent has not initialised the GPU yet)
    import torch
    torch.cuda.init()
    eng, sc, cam, rays = setup(args.passes, stream=torch.cuda.current_stream().cuda_stream)
    W, H, n, calls = sc.width, sc.height, rays.shape[0], args.calls
    dev = torch.device("cuda:0")
    t_o, t_d = torch.from_numpy(np.ascontiguousarray(rays[:, :3])).to(dev), torch.from_numpy(np.ascontiguousarray(rays[:, 3:])).to(dev)
    hits, surf = torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.zeros((n, 16), dtype=torch.int32, device=dev)
    out = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), r

    def fmt(v):
        m, lo, hi = spread(v)
        return f"median {m:8.4f} ms  ({lo:.4f} .. {hi:.4f})"

    info = eng.motion_info()
    lines.append(f"c3 {W}x{H}, {info['triangles']} triangles in {info['meshes']} mesh(es), history of {args.passes} passes; mesh 0 shifted, camera orbit 0.05; "
                 f"{calls} timed calls after {WARM} warm-ups, device events on the context's stream")
    # ---- the trace beside the query with surface records, alternating
    legs = {"trace": [], "query": []}
    tr = None
    for k in range(WARM + calls):
        ms, tr = timed(lambda: eng.motion_trace(cam))
        ms_q, _ = timed(lambda: eng.query_to_device(n, t_o.data_ptr(), t_d.data_ptr(), hits_ptr=hits.data_ptr(), surfaces_ptr=surf.data_ptr(), tmin=0.0))
        if k >= WARM:
            legs["trace"].append(ms), legs["query"].append(ms_q)
    q = eng.query_last()
    assert q["hits"] == tr["surface_pixels"] + tr["unmatched_pixels"], (q, tr)
    lines.append(f"  hr_motion_trace ({tr['surface_pixels'] / n:.1%} surface, {tr['sky_pixels'] / n:.1%} sky, {tr['unmatched_pixels']} unmatched)  {fmt(legs['trace'])}  {n / np.median(legs['trace']) * 1e-3:8.1f} Mrays/s")
    lines.append(f"  hr_query_trace, the same rays, surface records                 {fmt(legs['query'])}  {n / np.median(legs['query']) * 1e-3:8.1f} Mrays/s")
    lines.append(f"  hr_motion_trace / hr_query_trace (medians): {np.median(legs['trace']) / np.median(legs['query']):.4f}")
    # ---- the merge beside hr_history_merge, alternating
    trace_ms = float(np.median(legs["trace"]))
    legs = {"motion": [], "history": []}
    res = {}
    for k in range(WARM + calls):
        for leg, call in (("motion", lambda: eng.motion_merge(cam)), ("history", lambda: eng.history_merge(cam))):
            fresh(eng, cam)
            ms, res[leg] = timed(call)
            if k >= WARM:
                legs[leg].append(ms)
    lines.append(f"  hr_motion_merge ({res['motion']['reused_pixels'] / n:.1%} of the pixels reused)   {fmt(legs['motion'])}")
    lines.append(f"  hr_history_merge ({res['history']['reused_pixels'] / n:.1%} of the pixels reused)  {fmt(legs['history'])}")
    merge_only = float(np.median(legs["motion"])) - trace_ms
    lines.append(f"  hr_motion_merge less the trace's median: {merge_only:.4f} ms; over hr_history_merge (medians): {merge_only / np.median(legs['history']):.4f}")
    # ---- the snapshot and the vectors: asynchronous calls, back to back
    for _ in range(WARM):
        eng.motion_snapshot()
        eng.motion_vectors_to_device(out.data_ptr())
    eng.synchronize()
    snap_ms = timed(lambda: [eng.motion_snapshot() for _ in range(calls)])[0] / calls
    vec_ms = timed(lambda: [eng.motion_vectors_to_device(out.data_ptr()) for _ in range(calls)])[0] / calls
    lines.append(f"  hr_motion_snapshot   {snap_ms:8.4f} ms per call (mean of {calls} back-to-back calls; {info['triangles'] * 48 / 1e6:.1f} MB written)")
    lines.append(f"  hr_motion_vectors    {vec_ms:8.4f} ms per call (mean of {calls} back-to-back calls)")
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
