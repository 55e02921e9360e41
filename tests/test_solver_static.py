"""CPU: static properties of the package's GPU orchestration (solver.py, step_graphs.py, optim.py
and every other module), checked on its source.

Every HIP-graph capture must use the thread-local capture mode: with an RCCL process group
alive its watchdog thread queries events, and under the default global mode such a query
invalidates an ongoing capture (found by the round-3 RCCL test).  The package
has one capture site, step_graphs._capturing, so a capture added anywhere else is caught too.
"""
import ast
import pathlib

import deeppde_actorcritic_amd
from deeppde_actorcritic_amd import solver as psol

PKG = pathlib.Path(deeppde_actorcritic_amd.__file__).parent


def _calls(attr):
    """(module file name, ast.Call) of every `<something>.<attr>(...)` call in the package."""
    files = sorted(PKG.glob("*.py"))
    assert {"solver.py", "step_graphs.py", "optim.py", "ops.py"} <= {f.name for f in files}
    for f in files:
        for node in ast.walk(ast.parse(f.read_text())):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == attr:
                yield f.name, node


def test_every_graph_capture_is_thread_local():
    assert psol._CAPTURE_MODE == "thread_local"
    calls = list(_calls("graph"))
    assert [name for name, _ in calls] == ["step_graphs.py"]  # one capture site in the package
    for _, c in calls:
        kw = {k.arg: k.value for k in c.keywords}
        assert "capture_error_mode" in kw, ast.dump(c)
        v = kw["capture_error_mode"]
        assert isinstance(v, ast.Name) and v.id == "_CAPTURE_MODE", ast.dump(v)
    assert [name for name, _ in _calls("CUDAGraph")] == ["step_graphs.py"]  # and one graph constructor


def test_gback_default_and_choices():
    assert psol.GBACK in ("early", "late")
    assert psol.SAMPLE_STREAM in ("gside", "own")
