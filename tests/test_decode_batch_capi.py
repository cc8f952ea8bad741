"""CPU: host-side validation of the batched grouped decoders
(cwq_decode_grouped_greedy_batch, cwq_decode_grouped_importance_batch): bad
arguments are refused before any launch, with cwq_last_error() set, and the
workspace size functions are monotone.  Device pointers are never
dereferenced on these paths, so placeholders stand in for them."""
import numpy as np

from compression_without_quantization_amd import _lib  # noqa: F401

DEV = 4096  # a placeholder device pointer (never dereferenced before validation ends)


class _Batch:
    """Two items of 6 and 4 dims; item 0 in groups [0,2) [2,6), item 1 in [0,4)."""

    def __init__(self, n_steps=1, bits=8):
        self.n_steps, self.bits = n_steps, bits
        self.item_off = np.array([0, 6, 10], np.int64)
        self.starts = np.array([0, 2, 0], np.int64)
        self.starts_off = np.array([0, 2, 3], np.int64)
        self.code = np.frombuffer(b"0" * (3 * n_steps * bits), np.uint8).copy()
        self.bits_off = np.array([0, 2 * n_steps * bits, 3 * n_steps * bits], np.int64)
        self.index = np.zeros(3, np.int64)
        self.seeds = np.array([1, 2], np.int32)
        self.sample = np.zeros(10, np.float32)

    def greedy(self, lib, **kw):
        a = dict(n_items=2, item_off=self.item_off.ctypes.data, n_steps=self.n_steps,
                 bits=self.bits, sample_host=self.sample.ctypes.data, sample_dev=None,
                 ws=DEV, ws_bytes=lib.cwq_decode_grouped_greedy_batch_workspace_size(
                     10, 3, max(self.n_steps, 1)),
                 hws_bytes=lib.cwq_decode_grouped_greedy_batch_host_workspace_size(
                     10, 3, max(self.n_steps, 1)))
        a.update(kw)
        hws = np.zeros(max(int(a["hws_bytes"]), 1), np.uint8)
        return lib.cwq_decode_grouped_greedy_batch(
            a["n_items"], a["item_off"], DEV, DEV, self.code.ctypes.data,
            self.bits_off.ctypes.data, self.starts.ctypes.data, self.starts_off.ctypes.data,
            a["n_steps"], a["bits"], self.seeds.ctypes.data, 1.0, a["sample_host"],
            a["sample_dev"], a["ws"], a["ws_bytes"], hws.ctypes.data, a["hws_bytes"], None, None)

    def importance(self, lib, **kw):
        a = dict(n_items=2, item_off=self.item_off.ctypes.data,
                 sample_host=self.sample.ctypes.data, sample_dev=None, ws=DEV,
                 ws_bytes=lib.cwq_decode_grouped_importance_batch_workspace_size(10, 3),
                 hws_bytes=lib.cwq_decode_grouped_importance_batch_host_workspace_size(10, 3))
        a.update(kw)
        hws = np.zeros(max(int(a["hws_bytes"]), 1), np.uint8)
        return lib.cwq_decode_grouped_importance_batch(
            a["n_items"], a["item_off"], DEV, DEV, self.index.ctypes.data,
            self.starts_off.ctypes.data, self.starts.ctypes.data, self.starts_off.ctypes.data,
            self.seeds.ctypes.data, a["sample_host"], a["sample_dev"], a["ws"], a["ws_bytes"],
            hws.ctypes.data, a["hws_bytes"], None, None)


def _refused(lib, rc, code, word):
    err = lib.cwq_last_error()
    assert rc == code, (rc, err)
    assert word in err, err


def test_greedy_batch_decode_rejects_bad_arguments(cwqlib):
    b = _Batch()
    _refused(cwqlib, b.greedy(cwqlib, item_off=None), -1, b"null pointer")
    _refused(cwqlib, b.greedy(cwqlib, n_items=-1), -1, b"n_items")
    _refused(cwqlib, b.greedy(cwqlib, n_steps=0), -1, b"n_steps")
    _refused(cwqlib, b.greedy(cwqlib, bits=-1), -1, b"n_bits_per_step")
    _refused(cwqlib, b.greedy(cwqlib, bits=31), -1, b"n_bits_per_step")
    _refused(cwqlib, b.greedy(cwqlib, sample_host=None, sample_dev=None), -1, b"sample_host")
    need = cwqlib.cwq_decode_grouped_greedy_batch_workspace_size(10, 3, 1)
    _refused(cwqlib, b.greedy(cwqlib, ws_bytes=need - 1), -3, b"workspace")
    hneed = cwqlib.cwq_decode_grouped_greedy_batch_host_workspace_size(10, 3, 1)
    _refused(cwqlib, b.greedy(cwqlib, hws_bytes=hneed - 1), -3, b"host workspace")


def test_greedy_batch_decode_rejects_uncovered_items(cwqlib):
    # item 1's code is one group short: nothing of it is decoded
    b = _Batch()
    b.bits_off[2] = b.bits_off[1]
    _refused(cwqlib, b.greedy(cwqlib), -1, b"item 1: decoded groups cover 0 of 4 dims")
    # item 0's code holds one group of two: [0, 2) of 6 dims
    b = _Batch()
    b.bits_off[1] = 8
    _refused(cwqlib, b.greedy(cwqlib), -1, b"item 0: decoded groups cover 2 of 6 dims")
    # starts that fall, and starts that do not begin at 0
    b = _Batch()
    b.starts[:2] = [0, 7]
    _refused(cwqlib, b.greedy(cwqlib), -1, b"item 0: group starts")
    b = _Batch()
    b.starts[2] = 1
    _refused(cwqlib, b.greedy(cwqlib), -1, b"item 1: group starts")
    # a multi-step code: the same rule per group of n_steps * bits chars
    b = _Batch(n_steps=3, bits=5)
    b.bits_off[2] = b.bits_off[1]
    _refused(cwqlib, b.greedy(cwqlib), -1, b"item 1: decoded groups cover 0 of 4 dims")


def test_importance_batch_decode_rejects_bad_arguments(cwqlib):
    b = _Batch()
    _refused(cwqlib, b.importance(cwqlib, item_off=None), -1, b"null pointer")
    _refused(cwqlib, b.importance(cwqlib, n_items=-1), -1, b"n_items")
    _refused(cwqlib, b.importance(cwqlib, sample_host=None, sample_dev=None), -1, b"sample_host")
    need = cwqlib.cwq_decode_grouped_importance_batch_workspace_size(10, 3)
    _refused(cwqlib, b.importance(cwqlib, ws_bytes=need - 1), -3, b"workspace")
    hneed = cwqlib.cwq_decode_grouped_importance_batch_host_workspace_size(10, 3)
    _refused(cwqlib, b.importance(cwqlib, hws_bytes=hneed - 1), -3, b"host workspace")
    b.starts[2] = 1   # item 1 does not start at 0
    _refused(cwqlib, b.importance(cwqlib), -1, b"item 1: group starts")
    b = _Batch()
    b.starts[:2] = [1, 2]   # item 0 starts at 1
    _refused(cwqlib, b.importance(cwqlib), -1, b"item 0: group starts")
    b = _Batch()
    b.starts_off[:] = [0, 3, 3]  # item 1 lists no group at all
    b.starts[:] = [0, 2, 4]
    _refused(cwqlib, b.importance(cwqlib), -1, b"item 1: decoded groups cover 0 of 4 dims")


def test_empty_batches_succeed_without_a_device(cwqlib):
    b = _Batch()
    assert b.greedy(cwqlib, n_items=0) == 0 and cwqlib.cwq_last_error() == b""
    assert b.importance(cwqlib, n_items=0) == 0 and cwqlib.cwq_last_error() == b""


def test_batch_decode_workspace_sizes_monotone(cwqlib):
    g = cwqlib.cwq_decode_grouped_greedy_batch_workspace_size
    gh = cwqlib.cwq_decode_grouped_greedy_batch_host_workspace_size
    i = cwqlib.cwq_decode_grouped_importance_batch_workspace_size
    ih = cwqlib.cwq_decode_grouped_importance_batch_host_workspace_size
    Ds, Gs, Ss = [0, 1, 63, 64, 1000, 10 ** 6], [0, 1, 64, 65, 5000, 10 ** 5], [1, 2, 30]
    for f in (g, gh):
        for D in Ds:
            for G in Gs:
                for S in Ss:
                    v = f(D, G, S)
                    assert v <= f(D + 1, G, S) and v <= f(D, G + 1, S) and v <= f(D, G, S + 1)
    for f in (i, ih):
        for D in Ds:
            for G in Gs:
                v = f(D, G)
                assert v <= f(D + 1, G) and v <= f(D, G + 1)
    # the plan (offsets, quad prefix, seeds, n_steps indices per group) and the samples fit
    assert gh(1000, 5000, 30) >= 5001 * 16 + 5000 * 4 + 5000 * 30 * 4
    assert g(1000, 5000, 30) >= gh(1000, 5000, 30) + 1000 * 4
    assert ih(1000, 5000) >= 5001 * 8 + 5000 * 4 + 5000 * 8
    assert i(1000, 5000) >= ih(1000, 5000) + 1000 * 4
