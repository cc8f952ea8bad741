"""GPU: the PLN codec with a bit budget per level-1 group
(code_image_greedy / decode_image_greedy with first_level_group_bits=True)
against the oracle's composition, the plain codec and the prune_mode=0 coder,
bit for bit."""
import math

import numpy as np
import pytest
import torch

from compression_without_quantization_amd.binary_io import read_bin_code, to_bit_string

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def P(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    torch.backends.cudnn.benchmark = False
    torch.backends.cudnn.deterministic = True
    from compression_without_quantization_amd import pln
    return pln


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _eq(got, want, what):
    g, w = _bits(got).reshape(-1), _bits(want).reshape(-1)
    bad = np.nonzero(g != w)[0]
    assert g.size == w.size and bad.size == 0, f"{what}: {bad.size} of {w.size} differ"


def _wrap32(x):
    return int(np.int32(np.uint32(int(x) & 0xFFFFFFFF)))


def _image(h, w, seed=0):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w] / max(h, w)
    base = np.stack([np.sin(6 * xx + c) * np.cos(4 * yy - c) for c in range(3)], -1)
    img = 0.5 + 0.35 * base + 0.05 * rng.standard_normal((h, w, 3))
    return np.clip(img, 0, 1).astype(np.float32)[None]


def _model(P, seed=0, **kw):
    args = dict(first_level_filters=32, second_level_filters=16, first_level_latent_channels=32,
                second_level_latent_channels=8, init_seed=seed)
    args.update(kw)
    return P.ProbabilisticLadderNetwork(**args).cuda().eval()


def _imp_decoder_view(oracle, ind, st, oi, oq, pl, ps, seed):
    """What decode_grouped_importance_sample reconstructs (:337-361): coded
    rows destandardised, dequantised outliers where non-zero."""
    n = pl.size
    z, o = np.zeros(n, np.float32), np.ones(n, np.float32)
    coded = np.zeros(n, np.float32)
    for g, (a, b) in enumerate(zip(st[:-1], st[1:])):
        coded[a:b] = oracle.importance_decode_block(ind[g] - 1, z[a:b], o[a:b], seed + g)
    coded = oracle.destandardise(coded, pl, ps)
    upd = np.zeros(n, np.float32)
    upd[np.asarray(oi, np.int64)] = oracle.dequantize_quint16(oq)
    return np.where(upd == 0, coded, upd).astype(np.float32)


def _oracle_levels_var(oracle, model, img, seed, kw, min_bits=0):
    """The budget codec restated on the oracle: latents from the model; level 2
    by the oracle's grouped importance coder; level 1 by the oracle's partition,
    NumPy-float64 budgets from the float32 per-dim KLs, and the oracle's greedy
    coder per group at its budget."""
    from compression_without_quantization_amd import group_size_threshold
    lat = model.latent_distributions(img, seed)
    q1, q2 = lat["q1"], lat["q2"]
    s1, s2 = tuple(q1.loc.shape), tuple(q2.loc.shape)
    perm1, perm2 = oracle.pln_permutations(seed, int(np.prod(s1)), int(np.prod(s2)))
    f = lambda t, p: oracle.nhwc_permute_flatten(t.cpu().numpy(), p)
    q2l, q2s = f(q2.loc, perm2), f(q2.scale, perm2)
    n2 = q2l.size
    z, o = np.zeros(n2, np.float32), np.ones(n2, np.float32)
    samp2, ind2, st2, (oi2, oq2) = oracle.code_grouped_importance_sample(
        q2l, q2s, z, o, seed, kw["second_level_n_bits_per_group"],
        kw["second_level_max_group_size_bits"], kw["second_level_dim_kl_bit_limit"])
    dec2 = _imp_decoder_view(oracle, ind2, st2, oi2, oq2, z, o, seed)
    z2 = torch.from_numpy(oracle.unpermute_to_nchw(dec2, perm2, s2)).cuda()
    with torch.no_grad():
        pl1, ps1 = model.synthesis_transform_2(z2)
    p1l, p1s = f(pl1, perm1), f(ps1, perm1)
    q1l, q1s = f(q1.loc, perm1), f(q1.scale, perm1)
    n_steps, cap = kw["n_steps"], kw["n_bits_per_step"]
    tl, ts = oracle.standardise(q1l, q1s, p1l, p1s)
    kl = oracle.kl_normal_normal(q1l, q1s, p1l, p1s)
    starts = oracle.group_starts(kl, cap * n_steps,
                                 group_size_threshold(kw["greedy_max_group_size_bits"]))
    G = len(starts) - 1
    S = np.array([np.cumsum(kl[starts[g]:starts[g + 1]].astype(np.float64))[-1]
                  for g in range(G)])
    x = (S / np.log(2.0) + 1.0 / math.log(2.0)) / float(n_steps)
    assert np.abs(x - np.round(x)).min() > 1e-6  # no group on an integer boundary
    bits = np.clip(np.ceil(x), min_bits, cap).astype(np.int32)
    n1 = q1l.size
    samp = np.zeros(n1, np.float32)
    idx = np.zeros((G, n_steps), np.int32)
    zeros, ones = np.zeros(n1, np.float32), np.ones(n1, np.float32)
    for g in range(G):
        sl = slice(starts[g], starts[g + 1])
        idx[g], samp[sl] = oracle.code_greedy_sample(tl[sl], ts[sl], zeros[sl], ones[sl],
                                                     int(bits[g]), n_steps, _wrap32(seed + g), 1.0)
    samp1 = oracle.destandardise(samp, p1l, p1s)
    return samp2, st2, samp1, list(starts), bits, idx, perm1, s1


KW = dict(n_steps=2, n_bits_per_step=8, greedy_max_group_size_bits=12,
          second_level_n_bits_per_group=12, second_level_max_group_size_bits=2,
          second_level_dim_kl_bit_limit=10)
DEC = dict(use_importance_sampling=False, greedy_max_group_size_bits=12,
           second_level_max_group_size_bits=2)


def _reconstruction(P, model, sample1, perm1, s1):
    z1 = P.unpermute_unflatten(torch.from_numpy(np.asarray(sample1, np.float32)).cuda(),
                               torch.from_numpy(perm1).cuda(), s1)
    with torch.no_grad():
        return model.synthesis_transform_1(z1)[0].permute(1, 2, 0).cpu().numpy()


# ---------------------------------------------------------------------------
# (a) against the oracle's composition, and the round trip
# ---------------------------------------------------------------------------
def test_codec_var_vs_oracle_and_roundtrip(P, oracle, tmp_path):
    # model seed 1, image seed 1, greedy_max_group_size_bits=12: the 14 level-1
    # groups (3,072 dims, closed by KL at 139 .. 254 dims) get the budgets
    # histogram [0, 1, 0, 0, 0, 0, 1, 0, 12] (bits 0 .. 8) on an MI355X
    model = _model(P, seed=1)
    img = _image(128, 192, seed=1)
    seed = 42
    path = str(tmp_path / "img.miracle")
    cap = {}
    (sample2, sample1), summ = model.code_image_greedy(
        None, img, seed, comp_file_path=path, first_level_group_bits=True, capture=cap, **KW)
    w2, wst2, w1, wst1, wbits, widx, perm1, s1 = _oracle_levels_var(oracle, model, img, seed, KW)
    # the inputs show what the plain codec cannot: budgets differ, some below the cap
    assert len(set(wbits.tolist())) >= 2 and (wbits < KW["n_bits_per_step"]).any()
    _eq(sample2, w2, "level-2 sample")
    _eq(sample1, w1, "level-1 sample")
    assert cap["level1"]["kind"] == "greedy_var"
    _, code1, starts1, bits1 = cap["level1"]["result"]
    assert list(starts1) == wst1 and np.array_equal(bits1, wbits)
    want_code = ''.join(to_bit_string(int(widx[g, k]), int(wbits[g]))
                        for g in range(len(wbits)) for k in range(KW["n_steps"]))
    assert code1 == want_code
    total = KW["n_steps"] * int(wbits.sum())
    assert summ["first_level_code_bits"] == total == len(code1)
    assert summ["first_level_bits_histogram"] == \
        np.bincount(wbits, minlength=KW["n_bits_per_step"] + 1).tolist()
    assert summ["first_level_groups"] == len(wst1) and summ["second_level_groups"] == len(wst2)
    # the container: 11 extras, three variable bit strings, the budgets in the third
    code, extras, evb, _ = read_bin_code(path, num_extras=P.NUM_EXTRAS, num_extra_var_bits=3,
                                         num_var_length_extras=2)
    assert extras[5] == total and code[:total] == want_code
    sym = P._budget_coder("", KW["n_bits_per_step"]).decode_fast(evb[2])
    assert sym[-1] == 0
    assert np.array_equal(P._budgets_from_symbols(sym[:-1], KW["n_bits_per_step"]), wbits)
    assert summ["extra_byte_size"] == len(evb[0]) + len(evb[1]) + len(evb[2]) + 9 * 2 // 8
    rec = model.decode_image_greedy(None, path, first_level_group_bits=True, **DEC)
    assert rec.shape == (128, 192, 3)
    _eq(rec, _reconstruction(P, model, w1, perm1, s1), "reconstruction")


# ---------------------------------------------------------------------------
# (b) every budget forced to the cap: the plain codec's sample and image
# ---------------------------------------------------------------------------
def test_min_bits_at_the_cap_is_the_plain_codec(P, tmp_path):
    model = _model(P, seed=1)
    img = _image(128, 192, seed=1)
    a, b = str(tmp_path / "plain.miracle"), str(tmp_path / "var.miracle")
    (p2, p1), psumm = model.code_image_greedy(None, img, 42, comp_file_path=a, **KW)
    (v2, v1), vsumm = model.code_image_greedy(None, img, 42, comp_file_path=b,
                                              first_level_group_bits=True,
                                              first_level_min_bits=KW["n_bits_per_step"], **KW)
    _eq(v2, p2, "level-2 sample")
    _eq(v1, p1, "level-1 sample")
    G = psumm["first_level_groups"] - 1
    assert vsumm["first_level_bits_histogram"] == [0] * KW["n_bits_per_step"] + [G]
    assert vsumm["first_level_code_bits"] == G * KW["n_steps"] * KW["n_bits_per_step"]
    assert "first_level_code_bits" not in psumm and "first_level_bits_histogram" not in psumm
    assert set(psumm) <= set(vsumm)
    _eq(model.decode_image_greedy(None, b, first_level_group_bits=True, **DEC),
        model.decode_image_greedy(None, a, **DEC), "reconstruction")


# ---------------------------------------------------------------------------
# (c) determinism and refusals
# ---------------------------------------------------------------------------
def test_deterministic_file_and_refusals(P, tmp_path):
    model = _model(P, seed=1)
    img = _image(128, 192, seed=1)
    a, b, c = (str(tmp_path / n) for n in ("a.miracle", "b.miracle", "plain.miracle"))
    kw = dict(KW, first_level_group_bits=True)
    _, summ = model.code_image_greedy(None, img, 42, comp_file_path=a, **kw)
    model.code_image_greedy(None, img, 42, comp_file_path=b, **kw)
    assert open(a, "rb").read() == open(b, "rb").read()
    with pytest.raises(ValueError, match="use_importance_sampling"):
        model.code_image_greedy(None, img, 42, use_importance_sampling=True, **kw)
    with pytest.raises(ValueError, match="use_importance_sampling"):
        model.decode_image_greedy(None, a, use_importance_sampling=True,
                                  first_level_group_bits=True)
    gi1 = model.code_image_greedy(None, img, 42, return_first_level_group_sizes=True, **kw)
    assert gi1[0] == 0 and gi1[-1] == 32 * 8 * 12 and \
        len(gi1) == summ["first_level_groups"]
    # A plain file read as a budget file.  The container does not say which mode
    # wrote it, so the third "bit string" is the first outlier list's header; the
    # decoder refuses what follows: the parser fails on the shifted sections
    # (observed: "integer list of bit width 0", the empty level-2 outlier lists),
    # or else the budgets decoded from those bytes do not match the number of
    # groups or the level-1 code length.  Every one of these is a ValueError.
    model.code_image_greedy(None, img, 42, comp_file_path=c, **KW)
    with pytest.raises(ValueError):
        model.decode_image_greedy(None, c, first_level_group_bits=True, **DEC)
    # A budget file read as a plain file.  The plain decoder has no check of its
    # own, so the test accepts either outcome and shows the second is detectable:
    # the third string's 16-bit length and first byte are taken for an integer
    # list's count and width, which runs past the end of this file (observed:
    # ValueError "truncated .miracle file"); were it to parse, the level-1 code
    # length in the header disagrees with groups x n_steps x n_bits_per_step,
    # because a group below the cap makes the budget code shorter.
    try:
        rec = model.decode_image_greedy(None, a, **DEC)
    except ValueError:
        rec = None
    _, extras, evb, _ = read_bin_code(a, num_extras=P.NUM_EXTRAS, num_extra_var_bits=2)
    groups = summ["first_level_groups"] - 1
    assert extras[5] == summ["first_level_code_bits"]
    assert rec is None or extras[5] != groups * KW["n_steps"] * KW["n_bits_per_step"]
    assert extras[5] < groups * KW["n_steps"] * KW["n_bits_per_step"]


# ---------------------------------------------------------------------------
# (d) groups of 4,095 dims inside the codec: the shape the wave-per-row kernel
# is for
# ---------------------------------------------------------------------------
def test_full_size_groups_in_the_codec(P, cwqlib, tmp_path):
    """With seeded random weights the level-1 groups close by KL after a few
    hundred dims whatever the image size, so the model is quietened first: loc
    heads x 0.01, scale heads' kernels x 0.25 and the level-1 prior's scale
    bias at -1.1 bring a 256x256 image's 8,192 level-1 dims under 20 bits per
    4,095 (observed: groups [4095, 4095, 1, 1] at budgets [6, 6, 1, 1])."""
    import compression_without_quantization_amd as C
    model = _model(P, seed=1)
    with torch.no_grad():
        model.analysis_transform_1.loc_head.kernel.mul_(0.01)
        model.synthesis_transform_2.loc_head.kernel.mul_(0.01)
        model.analysis_transform_1.scale_head.kernel.mul_(0.25)
        model.synthesis_transform_2.scale_head.kernel.mul_(0.25)
        model.synthesis_transform_2.scale_head.bias.fill_(-1.1)
    img = _image(256, 256, seed=3)
    kw = dict(KW, n_steps=2, n_bits_per_step=10, greedy_max_group_size_bits=12)
    path = str(tmp_path / "big.miracle")
    cap = {}
    (_, sample1), summ = model.code_image_greedy(None, img, 42, comp_file_path=path,
                                                 first_level_group_bits=True, capture=cap, **kw)
    l1 = cap["level1"]
    _, code1, starts1, bits1 = l1["result"]
    lens = np.diff(np.asarray(starts1))
    full = lens == 4095
    assert full.sum() >= 2
    # the full-size groups' bucket meets the dispatch rule: below 4,096
    # candidates (and at more than one), mean length >= 256
    for b in set(bits1[full].tolist()):
        assert 1 <= b < 12 and lens[bits1 == b].sum() >= 256 * (bits1 == b).sum()
    # the same coder with every candidate scored by k_encode_eval
    t, p = C.Normal(l1["q_loc"], l1["q_scale"]), C.Normal(l1["p_loc"], l1["p_scale"])
    s0, code0, total0, starts0, bits0 = C.code_grouped_greedy_sample_var(
        t, p, kw["n_steps"], kw["n_bits_per_step"], 42, max_group_size_bits=12, prune_mode=0)
    assert starts0 == list(starts1) and np.array_equal(bits0, bits1)
    assert total0 == len(code1) == summ["first_level_code_bits"]
    assert P._chars_of(code0, total0) == code1
    _eq(sample1, s0, "level-1 sample (default mode vs prune_mode=0)")
    rec = model.decode_image_greedy(None, path, first_level_group_bits=True, **DEC)
    lat = model.latent_distributions(img, 42)
    s1 = tuple(lat["q1"].loc.shape)
    perm1, _ = P.permutations(42, int(np.prod(s1)), int(np.prod(lat["q2"].loc.shape)))
    _eq(rec, _reconstruction(P, model, sample1, perm1, s1), "reconstruction")
