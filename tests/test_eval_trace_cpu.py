"""The launch sequences of the whole-set evaluators are the recorded ones, call for call (``tests/eval_trace.py``): every
launcher call and every torch op that writes tensor data, from the evaluator's constructor to the end of ``run()``, with the
storage, offset, shape, strides and dtype of every operand -- for one replay, both row shards of two ranks and the
row-chunked evaluation of every recorded model variant.  A moved launch, an extra copy, a changed stride or a buffer that
stopped being shared fails here, with the first call that differs."""
import json

import pytest

from tests import eval_trace as T

with open(T.GOLDEN) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_file_holds_every_case():
    assert sorted(GOLDEN) == sorted('%s/%s' % (v, r) for v in T.VARIANTS for r in T.ROUTES)


@pytest.mark.parametrize('route', T.ROUTES)
@pytest.mark.parametrize('variant', sorted(T.VARIANTS))
def test_trace_is_the_recorded_one(variant, route):
    want = T.unpack(GOLDEN['%s/%s' % (variant, route)])
    got = T.trace(variant, route)
    for i, (a, b) in enumerate(zip(got['names'], want['names'])):
        assert a == b, 'call %d is %s, recorded: %s (after %s)' % (i, a, b, got['names'][max(0, i - 3):i])
    n_got, n_want = len(got['names']), len(want['names'])
    assert n_got == n_want, '%d calls, recorded: %d; the first one past the shorter list: %s' % (
        n_got, n_want, max(got['names'], want['names'], key=len)[min(n_got, n_want)])
    for i, (a, b) in enumerate(zip(got['digests'], want['digests'])):
        assert a == b, 'the arguments of call %d (%s) differ from the recorded ones: %s' % (
            i, got['names'][i], json.dumps(got['calls'][i][1]))
