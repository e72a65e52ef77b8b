"""tools/hit_truth_table.py [--rays N] [--lib liboracle.so] — how many ROBUST TRUE HITS the hit rule loses on thin triangles,
by aspect, distance and plane: float64 truth (tests/thin_cases.py) against the numpy float32 restatement of the rule with conditions 1-3
only ("before": the rule without the plane retry), with the retry ("after"), and against the oracle's answer (tree; --lib: another build
of the oracle, e.g. an older one).  No GPU.  D = 20 and 70 diagonals lie outside the domain the suite asserts; they are printed for
the record (the far-coordinate limit: h does not grow with the coordinates).  Output -> profiles/hit_truth_table.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib  # noqa: E402
import thin_cases as tc  # noqa: E402

DISTANCES = (0.2, 1.5, 5.0, 20.0, 70.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=14000)
    ap.add_argument("--lib", default=None, help="an oracle build to ask instead of the tree's")
    a = ap.parse_args()
    if a.lib:
        oracle_lib._LIB = ctypes.CDLL(os.path.abspath(a.lib))
    print(f"# robust true hits LOST of those counted (float64 truth: u, v > 0.1, u + v < 0.9, t > 10 eps, |d.n| > 0.3); {a.rays} rays per cell,")
    print("# 64 triangles per plane, scene [-1, 1]^3.  before = conditions 1-3 only (numpy float32), after = with the plane retry (numpy float32),")
    print(f"# oracle = {'the tree of ' + a.lib if a.lib else 'the oracle (tree)'}; max |t - t64| of the oracle's hits on the aimed-at triangle, in units of D |diagonal|")
    print(f"{'aspect':>8} {'plane':>9} " + " ".join(f"{'D = ' + str(D):>34}" for D in DISTANCES))
    print(f"{'':>8} {'':>9} " + " ".join(f"{'counted before after oracle  t err':>34}" for _ in DISTANCES))
    for aspect in tc.ASPECTS:
        for plane in tc.PLANES:
            tris = tc.make_cell(aspect, plane)
            eng = oracle_lib.engine()
            tc.scene(tris).apply(eng)
            eps, h, diag = tc.scene_constants(eng.scene_info())
            cols = []
            for D in DISTANCES:
                o, d, k = tc.make_rays(aspect, plane, D, n=a.rays)
                robust, alone, t64 = tc.truth(tris, o, d, k, float(eps), D)
                before = tc.hit_rule(tris[k, 0], tris[k, 1], tris[k, 2], o, d, eps, np.inf, h, retry=False)[0]
                after = tc.hit_rule(tris[k, 0], tris[k, 1], tris[k, 2], o, d, eps, np.inf, h, retry=True)[0]
                hit = eng.debug_trace(o, d)
                on = alone & (hit["prim"] == k)
                err = (np.abs(hit["t"][on].astype(np.float64) - t64[on]).max() / (D * float(diag))) if on.any() else float("nan")
                cols.append(f"{robust.sum():7d} {(robust & ~before).sum():6d} {(robust & ~after).sum():5d} {(robust & (hit['prim'] < 0)).sum():6d} {err:6.0e}")
            eng.close()
            print(f"{'1:' + str(aspect):>8} {plane:>9} " + " ".join(f"{c:>34}" for c in cols), flush=True)


if __name__ == "__main__":
    main()
