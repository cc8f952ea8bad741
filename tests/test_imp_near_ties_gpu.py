"""Every scoring path of the importance coder on rounding-sized gaps
(tests/importance_shapes.py NEAR_TIE_CASES; tests/test_importance_plan.py
checks on the CPU that each case takes the path it names), held to the CPU
oracle bit for bit in prune_mode 0 (every row exact) and 2 (screened).

tests/test_imp_near_ties.py certifies on the CPU, by the oracle alone, that on
these inputs every required neighbouring arithmetic (x as one fma, log p
without the round trip through x, the TFP >= 0.8 form, the term as a float
quadratic, either normaliser one ulp off) emits other indices than the
declared one, that exact ties are won by indices other than 0 and that the
winners are spread out.  Here each of those variants' index tables is also
compared with what the GPU returned and must differ: swapping the reference
for a variant would fail."""
import numpy as np
import pytest
import torch

import imp_near_ties as NT
import importance_shapes as S

pytestmark = pytest.mark.gpu
MODES = [0, 2]


@pytest.fixture(scope="module")
def cwq(cwqlib):
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    import compression_without_quantization_amd as C
    import compression_without_quantization_amd.coded_importance_sampler as I
    I.VERBOSE = False
    return C


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def _assert_bits_equal(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.size == w.size, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {w.size} differ, first at {bad[:8]}"


_REF = {}


def _reference(oracle, name):
    """(case, inputs, oracle indices, oracle samples, certificate, required
    variants) of a case, computed once per module and left unchanged."""
    if name not in _REF:
        case = S.near_tie_case(name)
        values = case.inputs()
        wi, ws = oracle.importance_encode(*values, case.off, case.oracle_counts, case.seed,
                                          case.base)
        cert = NT.certificate(case)
        for a in (wi, ws, cert["declared"], cert["gap"]) + tuple(cert["tables"].values()):
            a.setflags(write=False)
        assert np.array_equal(wi[cert["groups"]], cert["declared"])
        _REF[name] = (case, values, wi, ws, cert, NT.required(case, cert))
    return _REF[name]


def _encode(cwq, case, values, mode):
    gi, gs = cwq.importance_encode_blocks(*values, case.off, case.counts, case.seed,
                                          block_id_base=case.base, prune_mode=mode)
    return gi.cpu().numpy(), gs.cpu().numpy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", S.NEAR_TIE_CASES)
def test_near_tie_case(cwq, oracle, name, mode):
    case, values, wi, ws, cert, required = _reference(oracle, name)
    what = f"{name}, prune_mode {mode}"
    runs = [_encode(cwq, case, values, mode) for _ in range(3)]
    gi, gs = runs[0]
    bad = np.nonzero(gi != wi)[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {wi.size} indices differ, first groups "
                           f"{bad[:8]} (counts {case.counts[bad[:8]]}, dims {case.sizes[bad[:8]]}, "
                           f"got {gi[bad[:8]]}, want {wi[bad[:8]]})")
    _assert_bits_equal(gs, ws, f"{what}: samples")
    # which tile of a group publishes its threshold first must never show
    for k, (ri, rs) in enumerate(runs[1:]):
        assert np.array_equal(ri, gi), f"{what}: run {k + 2} differs"
        _assert_bits_equal(rs, gs, f"{what}: run {k + 2} samples")
    # the comparison has teeth: no required variant's table is what the GPU returned
    assert len(required) >= 8
    for v in required:
        diff = int((cert["tables"][v] != gi[cert["groups"]]).sum())
        assert diff >= NT.MIN_FLIPS, f"{what}: variant {v} differs on {diff} groups only"
    # ties won by an index other than 0 were among what was compared
    assert int(((cert["gap"] == 0) & (gi[cert["groups"]] > 0)).sum()) >= NT.MIN_TIES


@pytest.mark.parametrize("name", S.NEAR_TIE_CASES)
def test_near_tie_decode(cwq, oracle, name):
    case, values, wi, ws, _, _ = _reference(oracle, name)
    _, _, pl, ps = values
    dec = cwq.importance_decode_blocks(wi.copy(), pl, ps, case.off, case.seed,
                                       block_id_base=case.base)
    _assert_bits_equal(dec.cpu().numpy(), ws, f"{name}: decode of the oracle's indices")
