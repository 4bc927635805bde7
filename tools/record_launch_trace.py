#!/usr/bin/env python3
"""No GPU needed: the launch trace of every fast-engine case of tests/launch_trace.py (entry points, canonical arguments, streams,
events and marks of one step, recorded with `call` replaced) and the hashes of the index maps _build_packs produces.

    python tools/record_launch_trace.py --write            tests/golden/launch_traces.json (run ONCE, at the commit a host refactor starts from;
                                                           tests/test_launch_trace.py compares every later tree with it)
    python tools/record_launch_trace.py --write --set epilogue     the cases of another set (SETS below: `epilogue`, `optimizers`, the
                                                           optimizer steps, or `decode`, the generators) into that set's file, or into --out FILE;
                                                           --cases a,b narrows either set
    python tools/record_launch_trace.py --dump DIR         one <case>.json per case with one trace item per line, of THIS checkout: diff two
                                                           checkouts' dumps to see which launch moved (--set all: every set)

The file names the commit it was recorded at."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# set -> (its file under tests/golden, the name of its traced cases in tests/launch_trace.py, ... of its pack-map-only cases)
SETS = {"steps": ("launch_traces.json", "TRACE_CASES", None),
        "epilogue": ("launch_traces_epilogue.json", "EPILOGUE_CASES", "PACK_CASES"),
        "optimizers": ("launch_traces_optimizers.json", "OPTIMIZER_CASES", None),      # recorded by lt.record_optimizer
        "decode": ("launch_traces_decode.json", "DECODE_CASES", None)}                 # the generators, by lt.record_decode


def lines(trace):
    return "[\n" + ",\n".join(json.dumps(item) for item in trace) + "\n]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--dump")
    ap.add_argument("--cases", default="")
    ap.add_argument("--set", default="steps", choices=list(SETS) + ["all"])
    ap.add_argument("--out", help="the file --write writes (default: the set's file under tests/golden)")
    a = ap.parse_args()
    import pytest
    from tests import launch_trace as lt
    assert not (a.write and a.set == "all"), "--write takes one set"
    sets = list(SETS) if a.set == "all" else [a.set]
    want = lambda n: not a.cases or n in a.cases.split(",")
    names = [n for s in sets for n in getattr(lt, SETS[s][1]) if want(n)]
    record = lambda name, mp: (lt.record_optimizer if name in lt.OPTIMIZER_CASES else lt.record_decode if name in lt.DECODE_CASES
                               else lt.record)(name, mp)
    pack_names = [n for s in sets if SETS[s][2] for n in getattr(lt, SETS[s][2]) if want(n)]
    out, pack_only = {}, {}
    for name in names:
        with pytest.MonkeyPatch.context() as mp:
            trace, packs, forms = record(name, mp)
        out[name] = (trace, packs, forms)
        print("%-30s %4d items, %3d launches, %s" % (name, len(trace), sum(i[0] == "call" for i in trace), lt.digest(trace)[:16]), file=sys.stderr)
    for name in pack_names:
        with pytest.MonkeyPatch.context() as mp:
            pack_only[name] = lt.record_packs(name, mp)
        print("%-30s %d pack maps" % (name, len(pack_only[name])), file=sys.stderr)
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for name, (trace, _, _) in out.items():
            with open(os.path.join(a.dump, name + ".json"), "w") as f:
                f.write(lines(trace) + "\n")
        with open(os.path.join(a.dump, "packs.json"), "w") as f:
            json.dump(dict({n: p for n, (_, p, _) in out.items()}, **pack_only), f, indent=0, sort_keys=True)
    if a.write:
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
        dirty = subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain", "--", "music_amd"], text=True).strip()
        assert not dirty, "music_amd/ differs from the commit the file would name:\n" + dirty
        parts = ['"%s": {"forms": %s, "packs": %s, "trace": %s}' % (name, json.dumps(forms, sort_keys=True), json.dumps(packs, sort_keys=True),
                                                                  lines(trace)) for name, (trace, packs, forms) in out.items()]
        path = a.out or os.path.join(GOLDEN, SETS[a.set][0])
        tail = ',\n"packs_only": %s' % json.dumps(pack_only, sort_keys=True) if SETS[a.set][2] else ""
        with open(path, "w") as f:
            f.write('{"recorded_at": "%s",\n"cases": {\n%s\n}%s}\n' % (commit, ",\n".join(parts), tail))
        print("%s: %d bytes" % (path, os.path.getsize(path)), file=sys.stderr)


if __name__ == "__main__":
    main()
