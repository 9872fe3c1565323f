"""The weight-gradient partition the library holds is keyed without the row width, so a 176-bin (spec='CQT') and a 229-bin
(spec='Mel') model share its entries: every launch must still run the plan decided for ITS OWN shape (CPU: a recording stand-in
for the library; the shipped plan table decides the plans)."""
import pytest

from reconvat_amd import ops, plans, tuning


class Lib:
    def __init__(self):
        self.pinned, self.calls = {}, []

    def rv_conv_wgrad_set_plan(self, taps, bb, hv, ca, cb, nw, wgs):
        self.pinned[(taps, bb, hv, ca, cb)] = (nw, wgs)
        self.calls.append((taps, bb, hv, ca, cb, nw, wgs))
        return 0


@pytest.fixture
def fresh(monkeypatch):
    monkeypatch.setattr(ops, 'AUTOTUNE', 'table')
    for name in ('_wgrad_tuned', '_wgrad_plans', '_wgrad_owner'):
        fresh_state = type(getattr(tuning, name))()       # the state lives in tuning; ops re-exports the same objects
        monkeypatch.setattr(tuning, name, fresh_state)
        monkeypatch.setattr(ops, name, fresh_state)
    return Lib()


def launch(lib, taps, bb, hv, wv, ca, cb):
    ops._tune_wgrad(lib, ops.WgradProblem(0, taps, None, 0, hv, wv, ca, None, 0, hv, wv, cb, bb, 0, 0, 0), None)


def _mel_key_with_plan():
    for key, plan in sorted(plans.wgrad_entries().items()):
        taps, bb, hv, wv, ca, cb = key
        if wv == 229 and ca * cb * taps > 144 and ca > 1 and plans.lookup_wgrad((taps, bb, hv, 176, ca, cb)) is None:
            return key, tuple(plan)
    pytest.fail('the shipped table has no 229-wide weight-gradient entry without a 176-wide sibling')


def test_mel_shape_gets_its_table_plan_after_a_cqt_shape_of_the_same_library_key(fresh):
    (taps, bb, hv, wv, ca, cb), plan = _mel_key_with_plan()
    lib = fresh
    launch(lib, taps, bb, hv, 176, ca, cb)            # the CQT layer first: not in the table, library default
    assert lib.pinned.get((taps, bb, hv, ca, cb), (0, 0)) == (0, 0)
    launch(lib, taps, bb, hv, 229, ca, cb)            # the Mel layer of the same library key: its own table plan
    assert lib.pinned[(taps, bb, hv, ca, cb)] == plan
    launch(lib, taps, bb, hv, 176, ca, cb)            # back to the CQT model: the default again, not the Mel plan
    assert lib.pinned[(taps, bb, hv, ca, cb)] == (0, 0)
    n = len(lib.calls)
    launch(lib, taps, bb, hv, 176, ca, cb)            # same width again: nothing to re-pin
    assert len(lib.calls) == n
    launch(lib, taps, bb, hv, 229, ca, cb)
    assert lib.pinned[(taps, bb, hv, ca, cb)] == plan
    assert ops._wgrad_plans == {(taps, bb, hv, 229, ca, cb): plan}
