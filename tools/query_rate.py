"""tools/query_rate.py [--out FILE] — the rate of ray queries (include/hrcore_query.h) on the bench's c3 scene, for a GPU machine.

2,073,600 rays (the pixel centres of the 1080p camera) through hr_query_trace with device buffers, device-event times around the call on a
stream of its own (so a figure holds the counters' memset and copy and the two event waits of a foreign stream beside the kernel), after
a warm-up call, CALLS timed calls each, median and spread of
  (a) the camera rays in raster order              (b) the same rays in a seeded random permutation
  (c) (b) as occlusion queries, tmax = the closest hit's t       (d) (a), closest hit with surface records
then the wall time of one hr_query_trace_host call and of hr_debug_trace on the same rays (host arrays in, host arrays out).

Before the parent touches the GPU, a child process under `rocprofv3 --kernel-trace` alternates hr_debug_trace and hr_query_trace_host on
the rays of (a): the profiler's kernel durations of k_debug_trace and k_query_trace<false, false> are the comparison DESIGN.md asks for
(the same traversal on the same rays: equal within the run-to-run spread)."""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CALLS = 20


def scene_and_rays():
    import bench
    from heatray_amd import core, query
    sc = bench.build_scene("c3", 0, 0, 32)
    eng = core.create_engine()
    sc.apply(eng)
    W, H = sc.width, sc.height
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.reshape(-1) + 0.5, ys.reshape(-1) + 0.5], axis=-1).astype(np.float32)
    rays = query.camera_rays(sc.options.pass_params(0), W, H, xy)
    return eng, np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])


def child():
    eng, o, d = scene_and_rays()
    eng.debug_trace(o, d), eng.query(o, d)  # warm-up
    for _ in range(12):
        a = eng.debug_trace(o, d)
        b = eng.query(o, d)
    assert a.tobytes() == b.tobytes()
    print("child: hits equal, hit rate %.4f" % float((a["prim"] >= 0).mean()))


def spread(v):
    v = np.sort(np.asarray(v, np.float64))
    return float(np.median(v)), float(v[0]), float(v[-1])


def kernel_times(lines):
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        lines.append("kernel times: rocprofv3 not found: not measured")
        return
    d = tempfile.mkdtemp(prefix="hr_qr_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "-d", d, "-o", "qr", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child"]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=400)
    if r.returncode != 0:
        lines.append(f"kernel times: the profiled child failed (rc {r.returncode}): not measured: " + r.stderr.decode(errors="replace")[-300:])
        return
    dur = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                for key in ("k_debug_trace", "k_query_trace"):  # (the child launches no other variant than <false, false>)
                    if key in name:
                        dur.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6)
    shutil.rmtree(d, ignore_errors=True)
    lines.append("kernel durations by rocprofv3 --kernel-trace, one process alternating the two on the rays of (a), the first (warm-up) launch of each dropped:")
    for key, v in sorted(dur.items()):
        v = v[1:]
        m, lo, hi = spread(v)
        lines.append(f"  {key:32s} {len(v):3d} launches  median {m:8.3f} ms  min {lo:8.3f}  max {hi:8.3f}  ({2.0736 / m * 1e3:7.1f} Mrays/s)")
    if len(dur) == 2:
        a, b = spread(dur["k_debug_trace"][1:]), spread(dur["k_query_trace"][1:])
        lines.append(f"  k_query_trace / k_debug_trace (medians): {b[0] / a[0]:.4f};  spread of k_debug_trace (max / min): {a[2] / a[1]:.4f}, of k_query_trace: {b[2] / b[1]:.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_rate.txt"))
    args = ap.parse_args()
    if args.child:
        return child()
    lines = []
    kernel_times(lines)  # (first: the parent has not initialised the GPU yet)
    import torch
    from heatray_amd import _ffi as ffi
    eng, o, d = scene_and_rays()
    n = o.shape[0]
    dev = torch.device("cuda:0")
    perm = np.random.default_rng(0).permutation(n)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    p_o, p_d = torch.from_numpy(o[perm]).to(dev), torch.from_numpy(d[perm]).to(dev)
    hits = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    surf = torch.zeros((n, 16), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    raw = stream.cuda_stream

    def timed(name, **kw):
        ms = []
        for k in range(CALLS + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            eng.query_to_device(n, stream=raw, **kw)
            e1.record(stream)
            e1.synchronize()
            if k:
                ms.append(e0.elapsed_time(e1))
        m, lo, hi = spread(ms)
        last = eng.query_last()
        lines.append(f"  {name:58s} median {m:8.3f} ms  min {lo:8.3f}  max {hi:8.3f}  {n / m * 1e-3:8.1f} Mrays/s   hits {last['hits']}")
        return m

    lines.append(f"hr_query_trace, {n} rays on c3, device events around the call, {CALLS} timed calls after a warm-up call:")
    a = timed("(a) camera rays, raster order, closest hit", origins_ptr=t_o.data_ptr(), dirs_ptr=t_d.data_ptr(), hits_ptr=hits.data_ptr())
    b = timed("(b) the same rays, random permutation, closest hit", origins_ptr=p_o.data_ptr(), dirs_ptr=p_d.data_ptr(), hits_ptr=hits.data_ptr())
    stream.synchronize()
    h = hits.cpu().numpy().view(ffi.HIT_DTYPE).reshape(-1)
    tmax = torch.from_numpy(np.where(h["prim"] >= 0, h["t"], np.float32(np.inf)).astype(np.float32)).to(dev)
    torch.cuda.synchronize()
    timed("(c) (b) as occlusion queries, tmax = the closest hit's t", origins_ptr=p_o.data_ptr(), dirs_ptr=p_d.data_ptr(), hits_ptr=hits.data_ptr(), tmax_ptr=tmax.data_ptr(), any_hit=True)
    timed("(d) (a), closest hit with surface records", origins_ptr=t_o.data_ptr(), dirs_ptr=t_d.data_ptr(), hits_ptr=hits.data_ptr(), surfaces_ptr=surf.data_ptr())
    lines.append(f"  (b) over (a): {b / a:.3f}")
    eng.query(o, d), eng.debug_trace(o, d)  # warm-up at full size: the staging scratch has its size
    t0 = time.perf_counter()
    hq = eng.query(o, d)
    t1 = time.perf_counter()
    hd = eng.debug_trace(o, d)
    t2 = time.perf_counter()
    assert hq.tobytes() == hd.tobytes()
    lines.append(f"wall time, host arrays in and out, {n} rays: hr_query_trace_host {(t1 - t0) * 1e3:.1f} ms, hr_debug_trace {(t2 - t1) * 1e3:.1f} ms (the same bytes)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
