"""The convolution dispatch on the card against the launch record (tests/golden/dispatch/*.json, tools/make_dispatch_golden.py):
every config of the record except the batch-256 one runs again under the same recorder, and the set of unique records -
planner-level inputs, entry, label, every C ABI scalar, the tap tables, the NULL / aliasing pattern of the pointers - must
equal the committed file exactly.  The files were written at the revision before ops._plan_conv / ops._plan_wgrad existed."""
import json
import os
import sys

import pytest

from conftest import GOLD, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_dispatch_golden as G  # noqa: E402

CONFIGS = [n for n, c in G.CONFIGS.items() if "B" not in c]


def _keys(content):
    return {json.dumps(r, sort_keys=True) for r in content["records"]}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CONFIGS)
def test_launches_equal_the_record(name, tmp_path):
    """each config in a child process of its own under a time limit: the operand mode and the library (chosen at import) stay
    out of this process"""
    gold = G.load(os.path.join(GOLD, "dispatch", name + ".json"))
    if G.CONFIGS[name].get("lib") == "exp" and not os.path.exists(G.EXP_LIB):
        pytest.skip("variants/libspkhip_exp.so is not built")
    got = G.run_child(name, str(tmp_path / "got.json"), timeout=120)
    assert got["config"] == gold["config"] and got["experimental"] == gold["experimental"]
    want, have = _keys(gold), _keys(got)
    assert have == want, "%d records not in the golden file, %d golden records not launched; first of each:\n%s\n%s" % (
        len(have - want), len(want - have), next(iter(sorted(have - want)), None), next(iter(sorted(want - have)), None))
