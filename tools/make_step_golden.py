#!/usr/bin/env python3
"""Launch record of the whole training step: tests/golden/step/ (tests/step_trace.py says what a trace is and how it is
recorded on a machine without a GPU or the library).

    index.json             per configuration: sha256 of the canonical JSON of its trace, launch count, count per entry
    <config>.trace.json    the whole trace, one launch per line, for the configurations in step_trace.FULL

Like tools/make_dispatch_golden.py this hooks module globals only, so the same file records any revision of engine.py and
ops.py: the committed files were written at the revision before the engine's unused path selectors were removed and its block
backward restructured, and tests/test_step_trace_cpu.py / tests/test_step_trace_gpu.py hold every later revision to them.

    python tools/make_step_golden.py                       # rewrite tests/golden/step/
    python tools/make_step_golden.py --dump CONFIG > f     # the whole trace of any configuration, to diff between revisions
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLD = os.path.join(ROOT, "tests", "golden", "step")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=GOLD)
    ap.add_argument("--dump", metavar="CONFIG", default=None, help="print the whole trace of one configuration, one launch per line")
    a = ap.parse_args()
    import pytorch_kaldi_resnet_amd  # noqa: F401
    import step_trace as S
    if a.dump:
        S.dump_trace(S.record(a.dump), "/dev/stdout")
        return
    os.makedirs(a.out_dir, exist_ok=True)
    lines = []
    for name in S.CONFIGS:
        trace = S.record(name)
        if name in S.FULL:
            S.dump_trace(trace, os.path.join(a.out_dir, name + ".trace.json"))
        lines.append("%s: %s" % (json.dumps(name), json.dumps(S.summary(trace), separators=(",", ":"))))
        print(name, lines[-1][len(name) + 4:100], flush=True)
    with open(os.path.join(a.out_dir, "index.json"), "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join(lines))


if __name__ == "__main__":
    main()
