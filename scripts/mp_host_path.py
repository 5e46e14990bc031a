"""The MP-layer host path before and after a change to it: the cases of tests/launch_trace.py, their launch traces and their bits.

  python scripts/mp_host_path.py record  --outputs DIR [--golden tests/golden/launch_traces.json --commit SHA]
      runs every case under LaunchTrace, saves its outputs (torch.save, one file per case) into DIR — a scratch directory, not
      committed — and, with --golden, writes the traces there.  Run it on the commit the change starts from.
  python scripts/mp_host_path.py compare --outputs DIR
      runs every case again and reports torch.equal of every output (for the grad case every parameter gradient) against DIR; the
      kernels are deterministic, so anything but `equal` is a changed launch.  Exit status 1 on any difference.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import launch_trace as LT          # noqa: E402


def write_golden(path, commit, traces):
    with open(path, "w") as f:
        f.write('{"recorded_from": %s,\n "cases": {\n' % json.dumps(commit))
        for ci, (case, threads) in enumerate(traces.items()):
            f.write('  %s: {\n' % json.dumps(case))
            for ti, (who, rows) in enumerate(sorted(threads.items())):
                f.write('   %s: [\n' % json.dumps(who))
                f.write(",\n".join("    " + json.dumps(r, separators=(",", ":")) for r in rows))
                f.write("\n   ]%s\n" % ("," if ti + 1 < len(threads) else ""))
            f.write("  }%s\n" % ("," if ci + 1 < len(traces) else ""))
        f.write(" }\n}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("record", "compare"))
    ap.add_argument("--outputs", required=True)
    ap.add_argument("--golden")
    ap.add_argument("--commit", default="")
    a = ap.parse_args()
    os.makedirs(a.outputs, exist_ok=True)
    traces, bad = {}, 0
    for case in LT.case_ids():
        with LT.LaunchTrace() as rows:
            out = {k: v.detach().cpu() for k, v in LT.run(case).items()}
        traces[case] = {who: list(r) for who, r in rows.items()}
        path = os.path.join(a.outputs, case + ".pt")
        n_rows = sum(len(r) for r in rows.values())
        if a.mode == "record":
            torch.save(out, path)
            print(f"{case}: {n_rows} launches, {len(out)} outputs saved", flush=True)
            continue
        ref = torch.load(path)
        diff = [k for k in ref if k not in out or not torch.equal(ref[k], out[k])] + [k for k in out if k not in ref]
        bad += len(diff)
        print(f"{case}: {n_rows} launches, {len(ref)} outputs: " + ("torch.equal for all" if not diff else f"DIFFERENT: {diff}"), flush=True)
    if a.mode == "record" and a.golden:
        write_golden(a.golden, a.commit, traces)
        print(f"traces of {len(traces)} cases -> {a.golden}")
    if a.mode == "compare":
        print("ALL EQUAL" if not bad else f"{bad} outputs differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
