"""include/cwq.h's capture contract on the CPU: the calls that
tests/test_graph_replay_gpu.py leaves out are exactly those the header documents
as synchronising or as not capturable."""
import graph_replay as G


def test_the_header_names_the_calls_outside_the_contract():
    assert G.header_not_capturable(G.header_text()) == G.NOT_CAPTURABLE


def test_the_parser_reads_a_comment_and_the_declarations_under_it():
    text = """/* Enqueues.  Capturable. */
int cwq_a(void* stream);
/* Sorts, then SYNCHRONISES the
 * stream once. */
size_t cwq_b_workspace_size(int64_t n);
int cwq_b(void* stream);
/* cwq_b mentioned in passing. */
int cwq_c(void* stream);
/* This one cannot be
 * captured into a graph. */
int cwq_d(void* stream);"""
    assert G.header_not_capturable(text) == {"cwq_b", "cwq_d"}


def test_classify_names_each_kind_of_wrong_word():
    import numpy as np
    n_steps, nb = 3, 4
    want = np.arange(100, 100 + nb * n_steps, dtype=np.int32)
    filled = np.full(want.size, -1, np.int32)
    prev = want.copy()
    prev[7] = 555                       # the replay before left a wrong word here
    got = want.copy()
    got[2] = -1                         # block 0, step 2: never stored
    got[4] = 0                          # block 1, step 1: index 0
    got[5] = want[4]                    # block 1, step 2: the step before's index
    got[7] = 555                        # block 2, step 1: kept from the replay before
    got[11] = 77                        # block 3, step 2: something else
    lay = G.Steps("idx", n_steps, np.arange(nb + 1) * 8)
    msg = G.classify(got, want, filled, prev, lay)
    assert "5 of 12 words differ" in msg
    assert "step 2 even blocks: 1 hold the fill pattern" in msg
    assert "step 1 odd blocks: 1 hold index 0" in msg
    assert "step 2 odd blocks: 1 hold the previous step's index, 1 hold something else" in msg
    assert "step 1 even blocks: 1 hold the previous replay's value" in msg
    assert G.classify(want, want, filled, prev, lay) == ""
    s = G.Steps("sample", n_steps, np.array([0, 3, 3, 12]))
    assert "all steps even blocks: 1 hold something else" in \
        G.classify(got[:12] * 0 + np.where(np.arange(12) == 5, 9, want), want, filled, prev, s)
