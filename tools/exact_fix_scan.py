"""Which verdicts of the EXACT fix-up logic does a run reach?  For each candidate case of tests/exact_cases.py (or the
cases named on the command line as start:kind:seed:iters:batch:a:b) run the engine in EXACT rounds, compare it with the
oracle's sequential run (tree, rows, counters, per-iteration records) and print the case's clrrt_exact_fix_hist and
clrrt_exact_stats as one JSON line.  The cases of tests/test_exact_rounds.py and the histograms recorded beside them
were picked from this output; run it again on an MI355X after a change to the fix-up logic.

    python tools/exact_fix_scan.py [--options k=v,k=v] [case ...]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cl-rrt_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
import exact_cases as X  # noqa: E402

CANDIDATES = (
    [("fresh", kind, seed, iters, batch, 0, 0)
     for kind, iters in (("obb200", 400), ("moving", 300), ("empty", 300)) for seed in (2, 3, 4, 5)
     for batch in (256, 32)] +
    [("fresh", kind, seed, 300, 256, lim, 0)  # a narrow sortLimit window: the result pushed out of it
     for kind, seed in (("obb200", 3), ("obb200", 5), ("moving", 5), ("empty", 3)) for lim in (3, 5)] +
    [("copies", kind, seed, 300, 256, a, b)
     for kind in ("obb200", "empty") for seed in (3, 5) for a, b in ((150, 60), (300, 300), (40, 200))] +
    [("replan", kind, seed, 300, 256, 300, 0) for kind in ("obb200", "empty") for seed in (3, 5, 11)]
)


def parse(arg):
    f = arg.split(":")
    return (f[0], f[1]) + tuple(int(v) for v in f[2:7])


def main(argv):
    options = {}
    if argv and argv[0] == "--options":
        options = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in argv[1].split(",")}
        argv = argv[2:]
    cases = [parse(a) for a in argv] or CANDIDATES
    union = {}
    for case in cases:
        try:
            ref = X.reference(case)
        except AssertionError as e:  # (a replanning start whose first query found no path)
            print(json.dumps({"case": case, "skipped": str(e)}), flush=True)
            continue
        pl, st, rec = X.run_engine(case, options)
        try:
            try:
                X.assert_parity(ref, pl, rec, str(case))
                parity = "ok"
            except AssertionError as e:
                parity = str(e)[:300]
            hist = {k: v for k, v in pl.exact_fix_hist().items() if v}
            for k, v in hist.items():
                union[k] = union.get(k, 0) + v
            print(json.dumps({"case": case, "options": options, "parity": parity, "rounds": st["rounds"],
                              "nodes": len(ref["nodes"]["parent"]), "elapsed_ms": round(st["elapsed_ms"], 1),
                              "hist": hist, "stats": {k: v for k, v in pl.exact_stats().items() if v}}), flush=True)
        finally:
            pl.close()
    import clrrt
    print(json.dumps({"union": union,
                      "unreached": [k for k in clrrt.Planner.EXACT_FIX_BUCKETS if not union.get(k)]}), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
