"""The variable-length sweep of tests/test_varlen_parity_gpu.py covers the chunk lengths scripts/train_resnet.py --var-chunk draws
at its defaults.  Read with ast (the script is not executed): when the training range or quantum changes, the committed parity
lengths must be chosen again."""
import ast
import os

from helpers import ROOT, VARLEN_LENGTHS, VARLEN_MAX, VARLEN_MIN, VARLEN_QUANTUM


def _argparse_defaults(path):
    out = {}
    for node in ast.walk(ast.parse(open(path).read(), filename=path)):
        if (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument"
                and node.args and isinstance(node.args[0], ast.Constant)):
            for kw in node.keywords:
                if kw.arg == "default":
                    out[node.args[0].value] = ast.literal_eval(kw.value)
    return out


def test_varlen_sweep_matches_the_training_defaults():
    d = _argparse_defaults(os.path.join(ROOT, "scripts", "train_resnet.py"))
    got = (d["--min-chunk-size"], d["--max-chunk-size"], d["--chunk-quantum"])
    assert got == (VARLEN_MIN, VARLEN_MAX, VARLEN_QUANTUM), (
        "scripts/train_resnet.py --var-chunk now draws from %s (min, max, quantum): revisit the production set in tests/helpers.py "
        "and the parity lengths of tests/test_varlen_parity_gpu.py" % (got,))
    assert VARLEN_LENGTHS == tuple(range(got[0], got[1] + 1, got[2])) and len(VARLEN_LENGTHS) == 26
