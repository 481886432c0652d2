"""What the Python binding hands to the C-ABI (oracle/gen_binding_contract.py, tests/golden/binding_contract.json): for
every public function and Prepared* class, in both memory spaces, the descriptor, the scalars, which array every pointer
argument points at and the shapes and dtypes of what comes back -- replayed through a recording stand-in for the
binding's `_lib` and compared row for row, so that the binding's marshalling does not move by accident."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _replay(csp, monkeypatch, space):
    from oracle import gen_binding_contract as gen
    with open(os.path.join(ROOT, "tests", "golden", "binding_contract.json")) as f:
        rows = json.load(f)[space]
    cases = gen.cases(space)
    assert [r["case"] for r in rows] == [name for name, _, _ in cases] and len(rows) >= 100
    rec = gen.Recorder(csp.raw_lib(), space)
    monkeypatch.setattr(csp, "_lib", rec)
    for row, (name, fn, kw) in zip(rows, cases):
        got = gen.run_case(csp, rec, space, fn, kw)
        if got is not None:   # None: a case with torch tensors in host memory, on a machine without torch
            assert json.loads(json.dumps(dict(case=name, **got))) == row, name


def test_recorded_host_table(csp, monkeypatch):
    """numpy inputs; the compute entries are recorded and not run, so this replays without a device."""
    _replay(csp, monkeypatch, "host")


@pytest.mark.gpu
def test_recorded_device_table(csp, monkeypatch):
    """torch CUDA tensors; every call runs on the device."""
    _replay(csp, monkeypatch, "device")
