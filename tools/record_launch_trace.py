#!/usr/bin/env python3
"""No GPU needed: the launch trace of every fast-engine case of tests/launch_trace.py (entry points, canonical arguments, streams,
events and marks of one step, recorded with `call` replaced) and the hashes of the index maps _build_packs produces.

    python tools/record_launch_trace.py --write            tests/golden/launch_traces.json (run ONCE, at the commit a host refactor starts from;
                                                           tests/test_launch_trace.py compares every later tree with it)
    python tools/record_launch_trace.py --dump DIR         one <case>.json per case with one trace item per line, of THIS checkout: diff two
                                                           checkouts' dumps to see which launch moved

The file names the commit it was recorded at."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_traces.json")


def lines(trace):
    return "[\n" + ",\n".join(json.dumps(item) for item in trace) + "\n]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--dump")
    ap.add_argument("--cases", default="")
    a = ap.parse_args()
    import pytest
    from tests import launch_trace as lt
    names = [n for n in lt.TRACE_CASES if not a.cases or n in a.cases.split(",")]
    out = {}
    for name in names:
        with pytest.MonkeyPatch.context() as mp:
            trace, packs, forms = lt.record(name, mp)
        out[name] = (trace, packs, forms)
        print("%-30s %4d items, %3d launches, %s" % (name, len(trace), sum(i[0] == "call" for i in trace), lt.digest(trace)[:16]), file=sys.stderr)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for name, (trace, _, _) in out.items():
            with open(os.path.join(a.dump, name + ".json"), "w") as f:
                f.write(lines(trace) + "\n")
    if a.write:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "music_amd"], text=True).strip()
        assert not dirty, "music_amd/ differs from the commit the file would name:\n" + dirty
        parts = ['"%s": {"forms": %s, "packs": %s, "trace": %s}' % (name, json.dumps(forms, sort_keys=True), json.dumps(packs, sort_keys=True),
                                                                  lines(trace)) for name, (trace, packs, forms) in out.items()]
        with open(GOLDEN, "w") as f:
            f.write('{"recorded_at": "%s",\n"cases": {\n%s\n}}\n' % (commit, ",\n".join(parts)))
        print("%s: %d bytes" % (GOLDEN, os.path.getsize(GOLDEN)), file=sys.stderr)


if __name__ == "__main__":
    main()
