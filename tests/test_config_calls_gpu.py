"""Every configuration call of the engine (flowgnn_set_num_tasks .. flowgnn_jk_residual: width, numeric mode, pooling, eps, the two
virtual nodes, the two readouts, JK / residual) against the record of what it answered before those calls moved into
engine_config.hip: status, flowgnn_last_error's text and the getters' state after every call of every script of tests/config_calls.py,
entry for entry, against tests/golden/config_calls.json.  Marked gpu because flowgnn_create needs the device; no script sets weights
or a batch or runs, so no model kernel is launched.  The fixture is never recorded again: a mismatch is a fault of the code."""
import pytest

from tests import config_calls as cc

pytestmark = pytest.mark.gpu
SCRIPTS = cc.scripts()


@pytest.fixture(scope="module")
def recorded():
    return cc.load_fixture()


def test_the_fixture_holds_exactly_the_scripts(recorded):
    assert sorted(recorded) == sorted(s["name"] for s in SCRIPTS)  # none left uncompared, none without a record
    for s in SCRIPTS:
        assert len(recorded[s["name"]]) == 1 + len(s["calls"]), s["name"]  # (the runner's opening call, then the script's)
    assert 24 <= len(SCRIPTS) <= 80 and sum(len(s["calls"]) for s in SCRIPTS) >= 2000


@pytest.mark.parametrize("script", SCRIPTS, ids=[s["name"] for s in SCRIPTS])
def test_every_call_answers_as_recorded(script, recorded):
    want = recorded[script["name"]]
    got = cc.run(script)
    assert len(got) == len(want)
    calls = [cc.PRIME] + script["calls"]
    for i, (g, w) in enumerate(zip(got, want)):
        call = calls[i][0] + str(tuple(a if a is None or isinstance(a, int) else "<%s>" % (a[1:],) for a in calls[i][1:]))
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], "call %d, %s:\n got  %r\n want %r" % (i, call, g, w)
