"""CPU: the deferral regions of the uniform encoder's workspace
(csrc/cwq_workspace.h defer_ws; DESIGN.md 4 "Deferral").

tests/native/defer_plan.cpp runs the header on the host.  Checked here: where
the four regions lie (behind the encoder's layout, which stays what it was,
256-aligned, apart, inside the total), that the total is what
cwq_greedy_encode_uniform_defer_bytes answers and never below
cwq_greedy_encode_uniform_workspace_size, that both are monotone in the block
count, the slot index and the count word, and tests/defer_layout.py, with
which tests/test_prune_defer_gpu.py reads the regions back.  The same program
built with -fsanitize=address,undefined writes and reads every region of a
heap buffer of exactly the total.
"""
import os
import subprocess

import pytest

import defer_layout as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "defer_plan.cpp")
SHAPES = [(nb, d) for nb in (1, 3, 7, 70, 1000, 16384, 1000000) for d in (8, 16, 24, 32, 64)]
OTHER = [(0, 32), (5, 0), (5, 4), (5, 9), (37, 72), (3, 2000)]  # no deferral: no region


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("defer_plan") / "defer_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, SRC])

    def run(*args):
        out = subprocess.check_output([exe] + [str(a) for a in args], text=True)
        return [ln.split() for ln in out.splitlines()]
    return run


def _layout(prog, nb, d):
    rows = prog("layout", nb, d)
    enc = int(rows[0][1])
    assert rows[0][0] == "enc" and rows[-1][0] == "total"
    return enc, {r[0]: (int(r[1]), int(r[2])) for r in rows[1:-1]}, int(rows[-1][1])


def test_constants(prog):
    got = dict((k, int(v)) for k, v in prog("consts"))
    assert got == {"slots": L.SLOTS, "q": L.Q}
    assert 0 <= L.Q <= L.SLOTS


@pytest.mark.parametrize("nb,d", SHAPES + OTHER)
def test_regions(prog, nb, d):
    enc, reg, total = _layout(prog, nb, d)
    assert list(reg) == ["surv", "count", "dlist", "dcount"]
    want, want_total = L.regions(enc, nb, d)
    assert reg == want and total == want_total
    n = nb if L.applies(nb, d) else 0
    assert [reg[k][1] for k in reg] == [16 * n, 4 * n, 4 * n, 4 if n else 0]
    end = enc
    for name, (off, nbytes) in reg.items():
        assert off % 256 == 0 and off >= end, (name, off, end)  # apart, aligned, in order
        end = off + nbytes
    assert end <= total and total % 256 == 0
    assert (total == enc) == (n == 0)


@pytest.mark.parametrize("nb,d", SHAPES + OTHER)
def test_library_sizes(prog, cwqlib, nb, d):
    enc, _, total = _layout(prog, nb, d)
    assert int(cwqlib.cwq_greedy_encode_uniform_workspace_size(nb, d)) == enc
    assert int(cwqlib.cwq_greedy_encode_uniform_defer_bytes(nb, d)) == total


def test_invalid_sizes(cwqlib):
    for bad in ((-1, 32), (4, -1), (1 << 62, 32)):
        assert int(cwqlib.cwq_greedy_encode_uniform_defer_bytes(*bad)) == 0


@pytest.mark.parametrize("d", [8, 32, 64, 9])
def test_sizes_are_monotone(prog, d):
    last = (0, 0)
    for nb in (0, 1, 2, 3, 63, 64, 65, 1000, 16383, 16384, 100000):
        enc, _, total = _layout(prog, nb, d)
        assert total >= enc and enc >= last[0] and total >= last[1], (nb, d)
        last = (enc, total)


def test_slots_and_count_words(prog):
    for nb in (1, 7, 1000000):
        got = [(int(g), int(q), int(i)) for g, q, i in prog("slots", nb)]
        assert got and all(i == L.slot(g, q) for g, q, i in got)
        assert max(i for _, _, i in got) == nb * L.SLOTS - 1  # the last slot of the region
        assert len({i for _, _, i in got}) == len({(g, q) for g, q, _ in got})
    for q in range(L.SLOTS + 1):
        got = [(int(c), int(w)) for c, w in prog("words", q)]
        assert [c for c, _ in got] == list(range(L.SLOTS + 3))
        for c, w in got:
            # at most Q rows are listed as they are; more defer the block (word 0)
            assert w == L.count_word(c, q) == (c if c <= q else 0) and w <= L.SLOTS


def test_sanitized_walk(tmp_path):
    exe = str(tmp_path / "defer_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SRC])
    out = subprocess.run([exe, "walk"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr[-2000:]
