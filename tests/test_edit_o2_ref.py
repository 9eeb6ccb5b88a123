"""tests/edit_o2_ref.py against plain string slicing, on the boundary cases the GPU tests of "ORDER 2 IN EDITING AND SPLICING"
lean on it for.  No GPU."""
import numpy as np

import edit_o2_ref
import splice_table_ref

P0 = 0x20


def live_of(training, order, prev0=P0):
    """live[(context << 8) | symbol] of the pairs that occur in `training`, by slicing."""
    live = np.zeros(256 << (8 * order), dtype=np.uint8)
    padded = bytes([prev0, prev0]) + training
    for p in range(len(training)):
        ctx = int.from_bytes(padded[p + 2 - order:p + 2], "big") if order else 0
        live[(ctx << 8) | padded[p + 2]] = 1
    return live


def dropped_by_slicing(message, live, order, prev0):
    padded = bytes([prev0, prev0]) + message
    return sum(1 for p in range(len(message))
               if not live[((int.from_bytes(padded[p + 2 - order:p + 2], "big") if order else 0) << 8) | padded[p + 2]])


def test_dropped_counts_the_pairs_without_a_code_in_every_order():
    training = b"abcabcaab" + bytes([P0]) + b"ab"
    cases = [b"", b"a", b"b", b"ab", b"ba", b"abc", b"abx", b"xab", b"abcabcx", b"ccc", bytes([P0, P0, 0x61]), b"aab" * 9 + b"zab"]
    seen = set()
    for order in (0, 1, 2):
        live = live_of(training, order)
        for m in cases:
            want = dropped_by_slicing(m, live, order, P0)
            assert edit_o2_ref.dropped(m, live, P0) == want, (order, m)
            seen.add((order, want > 0))
    assert seen == {(o, f) for o in (0, 1, 2) for f in (False, True)}
    # the first two symbols lie under (prev0, prev0) and (prev0, y0): "ab" has codes there only when prev0 makes it so
    live2 = live_of(b"ab", 2)
    assert edit_o2_ref.dropped(b"ab", live2, P0) == 0 and edit_o2_ref.dropped(b"ab", live2, 0x61) == 2
    # a dropped symbol still advances the context: behind the unknown x, "b" lies under (a, x) and "c" under (x, b)
    assert edit_o2_ref.dropped(b"abcaxbca", live_of(b"abcabca", 2), P0) == 3


def test_contexts_in_front_of_position_zero_are_prev0():
    assert edit_o2_ref.contexts(b"xyz", 7, 2).tolist() == [0x0707, 0x0778, 0x7879]
    assert edit_o2_ref.contexts(b"xyz", 7, 1).tolist() == [7, 0x78, 0x79]
    assert edit_o2_ref.contexts(b"xyz", 7, 0).tolist() == [0, 0, 0]
    assert edit_o2_ref.contexts(b"", 7, 2).tolist() == []


def start_by_slicing(msg, lst, reps, F, prev0):
    """The splice of msg[:F] by the spans that begin in front of F, prev0 twice in front: its last two bytes."""
    if F >= len(msg):
        return None
    front = [(b, e, t) for b, e, t in lst if b < F]
    off, sp, tg = splice_table_ref.tagged_lists([front])
    y = bytes([prev0, prev0]) + splice_table_ref.apply([msg[:F]], off, sp, tg, reps)[0]
    return (y[-2] << 8) | y[-1]


def test_start_context_at_every_alignment_around_a_boundary():
    F = 256
    msg = bytes((7 * p + 3) % 251 for p in range(600))
    reps = [b"", b"R", b"ST", b"UVWXY"]
    lists = [[]]
    for b in range(F - 3, F + 4):
        for e in range(b, F + 4):
            for t in range(4):
                lists.append([(b, e, t)])
                for front in ([(b - 4, b, 0)], [(b - 4, b, 1)], [(b - 9, b - 6, 0), (b - 6, b - 2, 1), (b - 2, b, 0)], [(b, b, 1)],
                              [(b - 5, b - 1, 0)]):                     # touching in front, a chain of three, an insertion, one byte apart
                    lists.append(front + [(b, e, t)])
    lists += [[(0, F, 0)], [(0, 600, 0)], [(0, 0, 1), (0, F + 1, 0)], [(0, F - 1, 0)], [(1, F, 0)], [(F, F, 2), (F, F, 1)],
              [(F - 1, F - 1, 2), (F - 1, F - 1, 1)], [(F - 1, F - 1, 1), (F - 1, F, 0)], [(0, 1, 0), (1, F, 1)]]
    msgs = [msg] * len(lists)
    off, sp, tg = splice_table_ref.tagged_lists(lists)
    got = edit_o2_ref.start_context(msgs, off, sp, tg, reps, F, P0)
    want = [start_by_slicing(msg, lst, reps, F, P0) for lst in lists]
    assert got == want
    assert got[0] == (msg[F - 2] << 8) | msg[F - 1]
    k = lists.index([(0, F, 0)])
    assert got[k] == (P0 << 8) | P0 and got[k + 1] == (P0 << 8) | P0          # everything in front deleted: prev0 twice
    assert got[lists.index([(0, 0, 1), (0, F + 1, 0)])] == (P0 << 8) | ord("R")
    assert got[lists.index([(F, F, 2), (F, F, 1)])] == got[0]                 # insertions at F belong to what follows
    assert got[lists.index([(F - 1, F, 1)])] == (msg[F - 2] << 8) | ord("R")      # the last byte replaced by one
    assert got[lists.index([(F - 2, F - 1, 0)])] == (msg[F - 3] << 8) | msg[F - 1]  # x[F - 2] deleted: the `end + 1` case
    assert got[lists.index([(F - 3, F - 1, 2)])] == (ord("T") << 8) | msg[F - 1]    # two bytes in, x[F - 1] behind them
    assert got[lists.index([(F - 6, F - 2, 0), (F - 1, F, 0)])] == (msg[F - 7] << 8) | msg[F - 2]   # one byte apart: not touching
    # a message without position F
    assert edit_o2_ref.start_context([msg[:F], msg[:F + 1]], [0, 0, 0], [], [], reps, F, P0) == [None, got[0]]
