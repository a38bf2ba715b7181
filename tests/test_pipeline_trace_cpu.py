"""The call trace of kangaroo_amd/pipeline.py: which operators, collectives and handle methods every pipeline class issues, in
which order, on which buffers and with which arguments, for a fixed list of configurations (tests/pipeline_trace.py), compared with
the recorded traces under tests/golden/pipeline_trace/.  Bit-for-bit image tests do not see an extra summary rebuild or a merge
issued per level instead of once; this does.  No GPU, no libkfx, no oracle: the operator set and `dist` are recorders."""
import pytest

import pipeline_trace as pt

_GOLDEN = {}


def _golden(group):
    if group not in _GOLDEN:
        _GOLDEN[group] = pt.load(group)
    return _GOLDEN[group]


def test_fixtures_hold_exactly_the_cases():
    for group, cases in pt.CASES.items():
        assert sorted(_golden(group)) == sorted(cases)


@pytest.mark.parametrize("group,name", [(g, n) for g, cases in pt.CASES.items() for n in cases])
def test_call_trace(group, name, monkeypatch):
    got, want = pt.record(group, name, monkeypatch), _golden(group)[name]
    for k, (a, b) in enumerate(zip(got, want)):
        assert a == b, "%s: call %d differs\n  recorded: %s\n  now:      %s\n  after:    %s" % (name, k, b, a, got[max(0, k - 3):k])
    assert len(got) == len(want), "%s: %d calls, recorded %d; the first one beyond: %s" % (name, len(got), len(want), (got + want)[min(len(got), len(want))])
