"""The planner's output pinned: every (model, load flags, knob set) of tests/golden/plan_snapshot.json is loaded again and its
plan steps — label, own / issued / direct-form FLOPs and bytes per frame — and cost() totals must equal the recorded ones exactly
(host arithmetic on shapes: no tolerance).  Regenerate with tests/golden/make_plan_snapshot.py only when a plan is meant to change."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_plan_snapshot as snap  # noqa: E402


def test_plans_match_snapshot(gpu):
    with open(snap.PATH) as f:
        want = json.load(f)
    table = want["steps"]
    assert [(r["model"], r["flags"], r["knobs"]) for r in want["records"]] == snap.corpus()     # the whole corpus, nothing dropped
    bad = []
    for r in want["records"]:
        cost, steps = snap.plan_of(r["model"], r["flags"], r["knobs"], device=gpu)
        expect = [table[k] for k in r["steps"]]
        if cost != r["cost"] or steps != expect:
            diff = next(((i, a, b) for i, (a, b) in enumerate(zip(steps, expect)) if a != b), (None, len(steps), len(expect)))
            bad.append(f"{r['model']} flags {r['flags']} knobs {r['knobs']}: cost {cost} vs {r['cost']}; first difference {diff}")
    assert not bad, "\n".join(bad)
