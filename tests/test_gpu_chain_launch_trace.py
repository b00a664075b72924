"""The runtime's synchronisation as behaviour: the calls a pass makes on chains, streams and events (tools/chain_launch_trace.py), call for call
what was recorded before ProcessingChain's runtime was reshaped (tests/golden/chain_launch_trace.json).  Results alone do not show a missing
``wait_event``; this does."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("chain_launch_trace", os.path.join(ROOT, "tools", "chain_launch_trace.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


with open(os.path.join(ROOT, "tests", "golden", "chain_launch_trace.json")) as _f:
    RECORDED = json.load(_f)


@pytest.mark.parametrize("config", sorted(RECORDED))
def test_a_pass_makes_the_recorded_calls_in_the_recorded_order(config):
    got = json.loads(json.dumps(_tool().trace(config)))  # (through JSON, as the record went)
    want = RECORDED[config]
    assert sorted(RECORDED) == ["a", "b", "c", "d", "e", "f"] and len(want) > 10
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"configuration {config}, call {k}: {g} where {w} was recorded"
    assert len(got) == len(want)
