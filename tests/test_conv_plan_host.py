"""The host-side plans of the three convolution families answer as recorded (no GPU: the size and applicability queries of
include/sscg.h make no HIP call).  tests/golden/g10_conv_plans.json holds what the library answered before the families' launch setup
moved into csrc/conv_plan.h - workspace bytes, record bytes of the fused statistics and backward sums, which fusions apply - for every
bench shape and a few edge shapes, under every dtype combination, forced tile class and forced split (tests/golden/gen_conv_plans.py).
Every answer must be equal."""
import json
import os
import sys

import pytest

from conftest import ROOT, load_sub

GOLDEN = os.path.join(ROOT, "tests", "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)

import gen_conv_plans as gen  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "g10_conv_plans.json")))


def test_the_fixture_covers_the_cases_of_its_generator(golden):
    """the shape lists, dtype combinations, tunings and queries the generator enumerates today are the recorded ones, and no query's
    recorded answers are all alike within a family that serves it"""
    assert [tuple(s) for s in golden["shapes"]] == gen.shapes()
    assert set(gen.EDGE_SHAPES) <= set(tuple(s) for s in golden["shapes"])
    assert golden["families"] == [[f, list(dt), gen.tunings(n)] for f, dt, n in gen.FAMILIES]
    assert golden["queries"] == list(gen.QUERIES)
    assert gen.vacuous(golden["answers"]) == []
    for fa in golden["answers"]:
        for cols in fa:
            assert len(cols) == len(gen.QUERIES) and all(len(c) == len(golden["shapes"]) for c in cols)


def test_every_plan_answers_as_recorded(golden):
    if [k for k in os.environ if k.startswith("SSCG_KS_")]:
        pytest.skip("the SSCG_KS_* variables move the split family's tile-class thresholds")
    L = load_sub("_lib")
    shapes = [tuple(s) for s in golden["shapes"]]
    wrong, n_refused = [], 0
    for (family, dtypes, tunings), fa, fr in zip(golden["families"], golden["answers"], golden["refusals"]):
        for tuning, cols, ref in zip(tunings, fa, fr):
            want_rc = {e: dict(map(tuple, pairs)) for e, pairs in ref.items()}
            for i, shape in enumerate(shapes):
                # (gen.ask calls a compute entry only where the workspace query it has just made is positive)
                got, rc = gen.ask(L, gen.desc(L, shape, dtypes, tuning))
                want = [col[i] for col in cols]
                if [int(v) for v in got] != want:
                    wrong.append((family, dtypes, hex(tuning), shape, dict((q, (w, int(g))) for q, w, g in zip(gen.QUERIES, want, got) if w != g)))
                for e in gen.REFUSALS:
                    if (e in rc) != (i in want_rc[e]) or (e in rc and rc[e] != want_rc[e][i]):
                        wrong.append((family, dtypes, hex(tuning), shape, e, want_rc[e].get(i), rc.get(e)))
                    n_refused += rc.get(e) == gen.ERR_WORKSPACE
    assert not wrong, "%d descriptors answer differently, the first: %s" % (len(wrong), wrong[:5])
    assert n_refused > 0
