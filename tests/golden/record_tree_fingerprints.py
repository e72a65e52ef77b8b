"""HRCORE_LIB=<an earlier commit's libhrcore.so> python tests/golden/record_tree_fingerprints.py COMMIT [OUT]  — records
tests/golden/tree_fingerprints.json, the expected values of tests/test_gpu_tree_fingerprint.py (needs the GPU).

The library is the one HRCORE_LIB names (tools/build_variant.sh in a checkout of COMMIT makes one); without HRCORE_LIB nothing is recorded,
so that the library under test is never the source of the expected values.  Every case is built twice.  A field whose two values differ
in some case is left out of the fixture (and printed); if it is one of the required fields, or a recorded field still differs, nothing is
written."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    if not os.environ.get("HRCORE_LIB") or len(sys.argv) < 2:
        sys.exit(__doc__)
    from test_gpu_tree_fingerprint import FIXTURE, REQUIRED, SCENES, TUNES, fingerprint

    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    runs = ({}, {})
    for name, make in SCENES.items():
        scene = make()
        for tune in TUNES:
            for run in runs:
                run[f"{name}|{tune}"] = fingerprint(scene, tune)
    fields = list(next(iter(runs[0].values())))
    unstable = sorted({k for case in runs[0] for k in fields if runs[0][case][k] != runs[1][case][k]})
    for k in unstable:
        print(f"unstable, left out: {k}: " + ", ".join(f"{c}: {runs[0][c][k]} / {runs[1][c][k]}" for c in runs[0] if runs[0][c][k] != runs[1][c][k]))
    if set(unstable) & set(REQUIRED):
        sys.exit(f"a required field is unstable: {sorted(set(unstable) & set(REQUIRED))}: nothing written")
    fields = [k for k in fields if k not in unstable]
    cases = [{c: {k: fp[k] for k in fields} for c, fp in run.items()} for run in runs]
    if cases[0] != cases[1]:
        sys.exit("the two recordings differ: nothing written")
    with open(out, "w") as f:
        json.dump({"recorded_from_commit": sys.argv[1], "fields": fields, "unstable_fields": unstable, "cases": cases[0]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{out}: {len(cases[0])} cases, fields {fields}")


if __name__ == "__main__":
    main()
