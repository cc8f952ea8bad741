"""CPU: the workspace layouts (csrc/cwq_workspace.h).

* Sizes did not move: every *_workspace_size function answers what
  tests/golden/workspace_sizes.json recorded (gen_workspace_sizes.py) before
  the layouts moved to that header.
* Layouts are sound: over the same table, every region of every layout starts
  where it says it may, lies inside the total and apart from every other
  region (named aliases aside), and the total is the library's.
* The nesting the code relies on: an encode that runs inside a region sized
  for a larger shape, a plan that is placed by the groups a call came out with.

The layouts are compiled for the host from the header itself
(tests/native/ws_layout.cpp), as the dispatch rules are.
"""
import ctypes
import functools
import itertools
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
c_i64 = ctypes.c_int64


@functools.lru_cache(maxsize=None)
def _rows():
    with open(os.path.join(GOLDEN, "workspace_sizes.json")) as f:
        return [(r["function"], tuple(r["arguments"]), r["bytes"]) for r in json.load(f)["rows"]]


def test_golden_table_covers_every_size_function():
    from compression_without_quantization_amd import _lib
    names = {n for n in list(_lib.SIGNATURES) + list(_lib.TOOL_SIGNATURES)
             if n.endswith("_workspace_size")}
    assert len(names) == 18 and {r[0] for r in _rows()} == names
    assert ("cwq_greedy_encode_workspace_size", (18, 8711, 4095), 602880) in _rows()
    assert any(b == 0 for _, _, b in _rows()) and any(a and a[0] == 1 for _, a, _ in _rows())


def test_sizes_did_not_move(cwqlib):
    bad = [(fn, args, int(getattr(cwqlib, fn)(*args)), want) for fn, args, want in _rows()
           if int(getattr(cwqlib, fn)(*args)) != want]
    assert not bad, f"{len(bad)} of {len(_rows())} sizes moved (function, arguments, got, " \
                    f"golden): {bad[:10]}"


# ---------------------------------------------------------------------------
# the layouts, from the header
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("ws_layout") / "libws_layout.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared",
                           "-o", so, os.path.join(REPO, "tests", "native", "ws_layout.cpp")])
    lib = ctypes.CDLL(so)
    lib.wsl_dump.restype = ctypes.c_int
    lib.wsl_dump.argtypes = [ctypes.c_char_p, ctypes.POINTER(c_i64), ctypes.c_char_p, ctypes.c_int]
    lib.wsl_imp_plan.restype = None
    lib.wsl_imp_plan.argtypes = [c_i64, c_i64, c_i64, ctypes.c_int, ctypes.POINTER(c_i64)]
    buf = ctypes.create_string_buffer(1 << 14)

    def layout(what, *args):
        """(regions: [(name, off, bytes)], total)"""
        v = (c_i64 * max(len(args), 1))(*[int(a) for a in args])
        n = lib.wsl_dump(what.encode(), v, buf, len(buf))
        assert n > 0, f"wsl_dump({what}, {args}) = {n}"
        lines = [ln.split() for ln in buf.raw[:n].decode().splitlines()]
        assert lines[-1][0] == "total"
        return [(a, int(b), int(c)) for a, b, c in lines[:-1]], int(lines[-1][1])

    layout.imp_plan = lambda off, nbytes, G, seeds: _imp_plan(lib, off, nbytes, G, seeds)
    return layout


def _imp_plan(lib, off, nbytes, G, seeds):
    out = (c_i64 * 5)()
    lib.wsl_imp_plan(off, nbytes, G, int(seeds), out)
    return list(out)


# size function -> (layout, golden arguments -> the layout's arguments)
LAYOUT_OF = {
    "cwq_greedy_encode_workspace_size": ("enc_csr", lambda a: a),
    "cwq_greedy_encode_uniform_workspace_size": ("enc_uniform", lambda a: a),
    "cwq_greedy_encode_uniform_var_workspace_size": ("var", lambda a: a + (1,)),
    "cwq_greedy_encode_var_workspace_size": ("var_csr", lambda a: a),
    "cwq_pack_indices_var_workspace_size": ("pack", lambda a: a),
    "cwq_code_grouped_greedy_workspace_size": ("grouped", lambda a: a + (a[0] + 1,)),
    "cwq_code_grouped_greedy_batch_workspace_size": ("batch", lambda a: a),
    "cwq_code_grouped_greedy_batch_host_workspace_size": ("batch_host", lambda a: a),
    "cwq_importance_workspace_size": ("imp", lambda a: a),
    "cwq_code_grouped_importance_workspace_size": ("grouped_imp", lambda a: a + (1,)),
    "cwq_code_grouped_importance_batch_workspace_size": ("grouped_imp", lambda a: a),
    "cwq_decode_grouped_greedy_batch_workspace_size":
        ("dec", lambda a: (a[0], a[1], 1, 4 * a[2])),
    "cwq_decode_grouped_greedy_batch_host_workspace_size":
        ("dec_plan", lambda a: (a[1], 1, 4 * a[2])),
    "cwq_decode_grouped_importance_batch_workspace_size": ("dec", lambda a: (a[0], a[1], 0, 8)),
    "cwq_decode_grouped_importance_batch_host_workspace_size":
        ("dec_plan", lambda a: (a[1], 0, 8)),
    "cwq_beam_encode_workspace_size": ("beam", lambda a: (a[0], a[1], a[3], a[4])),
    "cwq_greedy_backfit_workspace_size": ("backfit", lambda a: (1,) + a),
    "cwq_debug_partition_workspace_size": ("part_debug", lambda a: a),
}


def _cases():
    """Every golden row with valid arguments (the size functions answer 0 for
    the others before any layout is computed), and the layouts no size
    function names: the uniform variable-budget call at other step counts, the
    uniform backfit, the partition alone, the grouped importance host staging."""
    out = []
    for fn, args, want in _rows():
        if want == 0 and (fn, args) != ("cwq_beam_encode_workspace_size", (0, 0, 0, 1, 1)):
            continue  # (an empty beam call is the one valid shape that needs no byte)
        what, conv = LAYOUT_OF[fn]
        out.append((what, tuple(conv(args)), want))
    for fn, args, want in _rows():
        if want == 0:
            continue
        if fn == "cwq_greedy_encode_uniform_var_workspace_size":
            out += [("var", args + (s,), None) for s in (3, 4 * args[1], 4 * args[1] + 1, 30)]
        if fn == "cwq_greedy_backfit_workspace_size" and args[0] and args[1] == args[0] * args[2]:
            out.append(("backfit", (0,) + args, None))
        if fn == "cwq_debug_partition_workspace_size":
            out.append(("part", args, None))
        if fn == "cwq_code_grouped_importance_batch_workspace_size" and args[0] > 0:
            out.append(("grouped_imp_host", args, None))
    return out


def test_every_size_function_has_its_layout():
    assert set(LAYOUT_OF) == {r[0] for r in _rows()}
    seen = {c[0] for c in _cases()}
    assert seen == {v[0] for v in LAYOUT_OF.values()} | {"part", "grouped_imp_host"}
    assert len(_cases()) > 300


def _check_layout(what, args, regions, total):
    tag = f"{what}{args}"
    by_name = {}
    for name, off, nbytes in regions:
        base = name.rstrip("!").split("@")[0].split("~")[0]
        assert base not in by_name, f"{tag}: two regions called {base}"
        by_name[base] = (off, nbytes)
    kin = {}  # name -> the regions it may lie on
    prev_end = 0
    for name, off, nbytes in regions:
        base = name.rstrip("!").split("@")[0].split("~")[0]
        assert off + nbytes <= total, f"{tag}: {base} ends at {off + nbytes} past total {total}"
        if "@" in name or "~" in name:
            other = name.split("@")[-1].split("~")[-1]
            po, pb = by_name[other]
            if nbytes:
                assert po <= off and off + nbytes <= po + pb, \
                    f"{tag}: {base} [{off}, +{nbytes}) outside {other} [{po}, +{pb})"
            kin[base] = {other} | ({n.split("@")[0] for n, _, _ in regions
                                   if n.endswith("@" + other)} if "~" in name else set())
        elif name.endswith("!"):
            assert off == prev_end, f"{tag}: packed {base} at {off}, the one before ends {prev_end}"
        else:
            assert off % 256 == 0, f"{tag}: {base} starts at {off}"
        if "~" not in name:
            prev_end = off + nbytes
    assert total % 256 == 0 or what == "part_debug", f"{tag}: total {total}"
    live = [(n, o, b) for n, (o, b) in by_name.items() if b > 0]
    for (n1, o1, b1), (n2, o2, b2) in itertools.combinations(live, 2):
        if n2 in kin.get(n1, ()) or n1 in kin.get(n2, ()):
            continue
        assert o1 + b1 <= o2 or o2 + b2 <= o1, \
            f"{tag}: {n1} [{o1}, +{b1}) overlaps {n2} [{o2}, +{b2})"


def test_layouts_are_sound(shim):
    """Regions start at multiples of 256 (or packed where declared), are
    pairwise disjoint except for named aliases, end inside the total; the
    total is libcwq.so's (the golden table, which test_sizes_did_not_move
    holds the library to)."""
    aliased = 0
    for what, args, want in _cases():
        regions, total = shim(what, *args)
        if want is not None:
            assert total == want, f"{what}{args}: total {total}, the library says {want}"
        _check_layout(what, args, regions, total)
        aliased += any("~" in n for n, _, _ in regions)
    assert aliased > 10  # the staged indices on the dead sorted inputs


def test_the_checks_can_fail():
    ok = [("a", 0, 100), ("b", 256, 10), ("c!", 266, 6), ("k@p", 512, 8), ("p", 512, 300),
          ("s~p", 512, 300)]
    _check_layout("ok", (), ok, 1024)
    for bad in ([("a", 0, 300), ("b", 256, 10)],                  # overlap
                [("a", 0, 100), ("b", 128, 10)],                  # not aligned
                [("a", 0, 100), ("c!", 104, 6)],                  # not packed
                [("k@p", 500, 20), ("p", 512, 300)],              # outside its parent
                [("a", 0, 100), ("s~a", 0, 100), ("b", 0, 10)],   # an overlap no alias names
                [("a", 0, 2000)]):                                # past the total
        with pytest.raises(AssertionError):
            _check_layout("bad", (), bad, 1024)


# ---------------------------------------------------------------------------
# the nesting conditions the entry points rely on
# ---------------------------------------------------------------------------
NB = [0, 1, 2, 7, 37, 300, 5000]
DIMS = [0, 1, 9, 64, 1024, 1025, 3000, 25000]
MAXD = [0, 1, 9, 64, 65, 1024, 1025, 4095]


def _total(shim, what, *args):
    return shim(what, *args)[1]


def test_encoder_layout_is_monotone(shim):
    t = functools.lru_cache(maxsize=None)(lambda nb, D, m: _total(shim, "enc_csr", nb, D, m))
    for (i, nb), (j, D), (k, m) in itertools.product(enumerate(NB), enumerate(DIMS),
                                                     enumerate(MAXD)):
        here = t(nb, D, m)
        if i:
            assert t(NB[i - 1], D, m) <= here
        if j:
            assert t(nb, DIMS[j - 1], m) <= here
        if k:
            assert t(nb, D, MAXD[k - 1]) <= here


def test_grouped_encode_fits_its_region(shim):
    """grouped_ws sizes `enc` for (D + 1, D, D) (the batch: D + 2 n + 1 groups)
    and runs the encoder at (G, D, longest group)."""
    for D in [0, 1, 3, 37, 1024, 1025, 2049, 5000]:
        cap = _total(shim, "enc_csr", D + 1, D, D)
        regions, _ = shim("grouped", D, 2, D + 1)
        assert dict((n, b) for n, _, b in regions)["enc"] == cap
        for G in sorted({0, 1, 2, D // 2, D, D + 1}):
            for m in sorted({0, 1, min(D, 64), min(D, 1024), min(D, 1025), D}):
                assert _total(shim, "enc_csr", G, D, m) <= cap, (D, G, m)


def test_uniform_never_exceeds_ragged(shim):
    """cwq_greedy_backfit sizes for ragged blocks and runs uniform ones too."""
    for nb, d in itertools.product([1, 2, 37, 300, 5000], [1, 4, 8, 9, 32, 64, 65, 72, 1024, 1025,
                                                           2000]):
        assert _total(shim, "enc_uniform", nb, d) <= _total(shim, "enc_csr", nb, nb * d, d)
        for steps in (1, 3, 30):
            assert _total(shim, "backfit", 0, nb, nb * d, d, steps) <= \
                _total(shim, "backfit", 1, nb, nb * d, d, steps)


def test_a_bucket_fits_its_call(shim):
    """The variable-budget calls run every bucket in the call's `enc` region:
    a bucket has no more blocks or dims and no longer a block than the call."""
    for nb, d in itertools.product([1, 37, 5000], [4, 9, 64, 72, 2000]):
        cap = _total(shim, "enc_uniform", nb, d)
        assert dict((n, b) for n, _, b in shim("var", nb, d, 2)[0])["enc"] == cap
        for c in sorted({1, nb // 2 or 1, nb}):
            assert _total(shim, "enc_uniform", c, d) <= cap
    for nb, D, m in [(18, 8711, 4095), (7, 3000, 1025), (7, 3000, 1024), (300, 9600, 32)]:
        cap = _total(shim, "enc_csr", nb, D, m)
        assert dict((n, b) for n, _, b in shim("var_csr", nb, D, m, 2)[0])["enc"] == cap
        for c, dims, longest in itertools.product(sorted({1, nb // 2, nb}), sorted({0, D // 3, D}),
                                                  sorted({0, 1, m // 2, m})):
            assert _total(shim, "enc_csr", c, dims, longest) <= cap


def test_importance_plan_stays_inside_its_region(shim):
    for what, D, I in [("grouped_imp", 0, 1), ("grouped_imp", 1, 1), ("grouped_imp", 37, 1),
                       ("grouped_imp", 863, 4), ("grouped_imp", 65536, 48),
                       ("grouped_imp_host", 863, 4), ("grouped_imp_host", 37, 1)]:
        regions = {n.split("@")[0]: (o, b) for n, o, b in shim(what, D, I)[0]}
        off, nbytes = regions["plan"]
        for G in sorted({0, 1, 2, 31, 32, 33, (D + I) // 2, D + I - 1, D + I}):
            if not 0 <= G <= D + I:
                continue
            for seeds in (False, True):
                counts, offs, sd, end, copy = shim.imp_plan(off, nbytes, G, seeds)
                assert counts == off and counts + 8 * G <= offs and offs + 8 * (G + 1) <= sd
                assert offs % 256 == 0 and sd % 256 == 0
                assert end == sd + 4 * G and end <= off + nbytes, (what, D, I, G)
                assert copy == (end - off if seeds else offs + 8 * (G + 1) - off)


def test_decoder_plan_fits_device_and_host_regions(shim):
    """The decoders plan the G groups they decode into workspaces sized for
    G_total >= G, on both sides with one layout; the device sample follows the
    G_total plan."""
    for slots, idx_b in [(1, 4), (1, 12), (1, 120), (0, 8)]:
        for cap in [0, 1, 9, 48, 300]:
            host = _total(shim, "dec_plan", cap, slots, idx_b)
            dev_regions, dev = shim("dec", 4137, cap, slots, idx_b)
            out = dict((n, (o, b)) for n, o, b in dev_regions)["out"]
            assert out == (host, 4 * 4137) and dev >= host + 4 * 4137
            for G in sorted({0, min(1, cap), cap // 2, cap}):
                assert _total(shim, "dec_plan", G, slots, idx_b) <= host
