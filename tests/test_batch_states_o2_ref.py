"""Why order-2 segment states need a speculation of their own, on the CPU model of tests/states_o2_ref.py: with
the order-0/1 rule most text streams are left to the one-lane walk after the 8 repair passes; with the recovery rule nearly
none is.  The inputs are those of the GPU convergence condition (tests/test_gpu_batch_states_o2.py), so this also pins that
the condition is a fair one.  The model alone gives 0 of 30 text streams and 1 of the 1 581 wiki lines."""
import pytest

import states_o2_ref as ref


@pytest.fixture(scope="module")
def text_runs():
    msgs = ref.text_batch()
    return ref.run(msgs, "today"), ref.run(msgs, "recover")


def test_the_order_1_rule_leaves_most_text_streams_to_the_walk(text_runs):
    today, _ = text_runs
    print("text, today's rule: wrong entries %s, %d of %d streams walked, %d null warm-ups" % (
        today["wrong"], today["walked"], today["streams"], today["null_warmups"]))
    assert today["streams"] == 30
    assert today["walked"] * 2 > today["streams"]
    assert today["null_warmups"] * 2 > today["segments"] - today["streams"]     # the warm-up dies in a context without codes


def test_the_recovery_rule_settles_text(text_runs):
    _, rec = text_runs
    print("text, recovery rule: wrong entries %s, %d of %d streams walked" % (rec["wrong"], rec["walked"], rec["streams"]))
    assert rec["walked"] * 20 <= rec["streams"]
    assert rec["wrong"][0] * 4 < rec["segments"]                               # most guesses are right before any repair


def test_the_recovery_rule_settles_the_wiki_lines():
    lines = ref.wiki_lines()
    assert len(lines) == 1581
    rec = ref.run(lines, "recover")
    print("wiki lines, recovery rule: %d segments, wrong entries %s, %d of %d streams walked" % (
        rec["segments"], rec["wrong"], rec["walked"], rec["streams"]))
    assert rec["walked"] * 100 <= rec["streams"]


def test_segment_1_is_exact_and_short_streams_need_no_repair():
    """W = S: segment 1 warms up from the stream's true start state."""
    msgs = [ref.text(k, 40 + k) for k in (1, 200, 400, 500, 600, 650)]
    rec = ref.run(msgs, "recover", train_extra=ref.text_batch())
    assert max(int(b) for b in rec["nbits"]) <= 2 * ref.SEG_BITS and rec["segments"] >= 9
    assert rec["wrong"][0] == 0 and rec["walked"] == 0
