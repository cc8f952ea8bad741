"""Rate tables for the single-step greedy coder, and bit budgets chosen from them.

The candidate rows of a block come from one stream whatever the budget, so a
b-bit code's ``2**b`` rows are the first ``2**b`` rows of a B-bit code.  One
call (cwq_rate_table, include/cwq.h) therefore answers, for every block and
every budget ``b = 0 .. B``, which index ``encode_blocks`` would choose at b bits
and the log-density it wins; from that table a budget per block is chosen on the
device by a Lagrangian rule (cwq_choose_bits) or under a total.

  rate_table          (idx, value), both [nb, B + 1]
  choose_bits         the lowest b maximising value[g, b] - lam * b, per block
  choose_bits_total   the same at the smallest lam whose total fits a target
  choose_bits_total_device   choose_bits_total solved on the device: no host wait
  encode_blocks_rate  table, budgets and the code, the triple of encode_blocks_var
  encode_blocks_rate_total   the same under a total in one capturable call
  code_grouped_greedy_sample_rate   the single-step grouped coder on top of it

All arithmetic runs in libcwq.so; nothing here computes samples on the CPU.
"""
import math

import numpy as np
import torch

from . import _lib
from .coded_greedy_sampler import _device_of, _f32, _ptr
from .varbits import (MAX_BITS, _code_grouped_var_with, _nb_of, _offsets, _one_of, _seed32,
                      decode_blocks_var)


def rate_table_workspace_bytes(nb, total_dims, max_block_dim, max_bits):
    """Workspace bytes of rate_table (cwq_rate_table_workspace_bytes)."""
    return int(_lib.load().cwq_rate_table_workspace_bytes(
        int(nb), int(total_dims), int(max_block_dim), int(max_bits)))


def rate_table(t_loc, t_scale, p_loc, p_scale, max_bits, seed, rho=1., block_dim=None,
               block_off=None, block_id_base=0, workspace=None, prune_mode=None):
    """For every block g and budget ``b = 0 .. max_bits``: ``idx[g, b]``, the
    index ``encode_blocks(..., b, 1, seed, ...)`` returns for the block, and
    ``value[g, b]``, the float32 log-density of that row as the coder's argmax
    key holds it (NaN and anything <= -FLT_MAX as -FLT_MAX).

    Blocks are uniform (``block_dim``) or ragged (``block_off``, nb + 1
    offsets).  Returns (idx int32 [nb, B + 1], value f32 [nb, B + 1]) as cuda
    tensors.  The call only enqueues launches on the current stream; with
    ``workspace`` (a uint8 cuda tensor of rate_table_workspace_bytes) it
    allocates nothing but its outputs.  ``prune_mode`` selects the scoring
    kernels of the budgets from 12 bits on; results never depend on it."""
    lib = _lib.load()
    _one_of(block_dim, block_off)
    dev = _device_of(t_loc, t_scale, p_loc, p_scale)
    tl = _f32(t_loc, dev, "t_loc")
    ts = _f32(t_scale, dev, "t_scale")
    pl = _f32(p_loc, dev, "p_loc")
    ps = _f32(p_scale, dev, "p_scale")
    D = tl.numel()
    if not (ts.numel() == pl.numel() == ps.numel() == D):
        raise ValueError("t_loc, t_scale, p_loc, p_scale must have the same size")
    if block_off is not None:
        offs, nb, longest = _offsets(block_off, D, dev)
    else:
        longest, nb = _nb_of(D, block_dim)
        offs = None
    B = int(max_bits)
    cols = B + 1 if 0 <= B <= MAX_BITS else 0  # the library refuses such a B
    idx = torch.empty((nb, cols), dtype=torch.int32, device=dev)
    value = torch.empty((nb, cols), dtype=torch.float32, device=dev)
    if workspace is None:
        need = rate_table_workspace_bytes(nb, D, longest, B)
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(prune_mode)
    with torch.cuda.device(dev):
        rc = lib.cwq_rate_table(
            _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, B, _seed32(seed), float(rho), int(block_id_base), _ptr(idx),
            _ptr(value), workspace.data_ptr(), workspace.numel(), opts,
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_rate_table")
    return idx, value


def _table(value):
    if not isinstance(value, torch.Tensor):
        value = torch.from_numpy(np.array(value, dtype=np.float32, order="C"))
    if value.dim() != 2 or value.shape[1] < 1:
        raise ValueError("value must be a table [nb, B + 1]")
    if not value.is_cuda:
        value = value.cuda()
    return value.to(torch.float32).contiguous()


def _choose(lib, value, lam, lo, hi, bits, total):
    dev = value.device
    with torch.cuda.device(dev):
        rc = lib.cwq_choose_bits(_ptr(value), value.shape[0], value.shape[1] - 1, float(lam),
                                 int(lo), int(hi), _ptr(bits), _ptr(total),
                                 torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_choose_bits")


def choose_bits(value, lam, min_bits=0, max_bits=None):
    """Per block the lowest ``b`` in ``[min_bits, min(max_bits, B)]`` that
    maximises ``float64(value[g, b]) - lam * b`` (``lam`` >= 0: nats per bit).
    Returns an int32 cuda tensor [nb]."""
    value = _table(value)
    hi = value.shape[1] - 1 if max_bits is None else int(max_bits)
    bits = torch.empty(value.shape[0], dtype=torch.int32, device=value.device)
    _choose(_lib.load(), value, lam, min_bits, hi, bits, None)
    return bits


def choose_bits_total(value, total_bits, min_bits=0, max_bits=None):
    """Budgets whose sum is at most ``total_bits``: choose_bits at the smallest
    ``lam`` that 60 halvings of ``[0, lam_hi]`` find with a total within the
    target.  At ``lam_hi``, the largest ``value[g, b] - value[g, min_bits]`` of
    the table, every block sits at ``min_bits``.  Each halving is one
    cwq_choose_bits call and one read of its total.  Returns (bits int32 cuda
    tensor [nb], lam).  Raises ValueError when ``min_bits`` everywhere exceeds
    the target."""
    lib = _lib.load()
    value = _table(value)
    nb, B = value.shape[0], value.shape[1] - 1
    lo_b = int(min_bits)
    hi_b = B if max_bits is None else min(int(max_bits), B)
    if not 0 <= lo_b <= hi_b:
        raise ValueError(f"min_bits={min_bits} outside [0, min(max_bits, {B})]")
    if nb * lo_b > int(total_bits):
        raise ValueError(f"{nb} blocks at min_bits={lo_b} exceed total_bits={total_bits}")
    dev = value.device
    bits = torch.empty(nb, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)

    def total_at(lam):
        _choose(lib, value, lam, lo_b, hi_b, bits, total)
        return int(total.item())

    if total_at(0.0) <= int(total_bits):
        return bits, 0.0
    span = value[:, lo_b:hi_b + 1].double() - value[:, lo_b:lo_b + 1].double()
    lam_lo, lam_hi = 0.0, float(span.max().item())  # total(lam_lo) > target >= total(lam_hi)
    for _ in range(60):
        mid = 0.5 * (lam_lo + lam_hi)
        if total_at(mid) <= int(total_bits):
            lam_hi = mid
        else:
            lam_lo = mid
    if total_at(lam_hi) > int(total_bits):  # cannot happen for a finite table
        raise ValueError(f"no lam in [0, {lam_hi}] brings the total within {total_bits} bits")
    return bits, lam_hi


def encode_blocks_rate(t_loc, t_scale, p_loc, p_scale, seed, max_bits, lam=None, total_bits=None,
                       min_bits=0, rho=1., block_dim=None, block_off=None, block_id_base=0,
                       prune_mode=None):
    """A single-step code with budgets chosen from the blocks' rate table: by
    ``lam`` (choose_bits) or under ``total_bits`` (choose_bits_total), exactly
    one of the two.  Returns (idx int32 [nb, 1], sample f32 [D], n_bits int32
    [nb]), the triple of ``encode_blocks_var(..., n_bits, 1, seed, ...)``, which
    goes to pack_indices, decode_blocks_var and backfit_blocks_var as that one
    does.  The indices are read off the table and the sample comes from the
    decoder: there is no second encode."""
    if (lam is None) == (total_bits is None):
        raise ValueError("give exactly one of lam / total_bits")
    tidx, tval = rate_table(t_loc, t_scale, p_loc, p_scale, max_bits, seed, rho=rho,
                            block_dim=block_dim, block_off=block_off,
                            block_id_base=block_id_base, prune_mode=prune_mode)
    if lam is not None:
        n_bits = choose_bits(tval, lam, min_bits=min_bits)
    else:
        n_bits, _ = choose_bits_total(tval, total_bits, min_bits=min_bits)
    idx = tidx.gather(1, n_bits.long().unsqueeze(1)).contiguous()
    sample = decode_blocks_var(idx, n_bits, p_loc, p_scale, 1, seed, rho=rho, block_dim=block_dim,
                               block_id_base=block_id_base, block_off=block_off)
    return idx, sample, n_bits


# ---------------------------------------------------------------------------
# budgets under a total, solved on the device
# ---------------------------------------------------------------------------
def choose_bits_total_workspace_bytes(max_bits_table):
    """Workspace bytes of choose_bits_total_device (cwq_choose_bits_total_workspace_bytes)."""
    return int(_lib.load().cwq_choose_bits_total_workspace_bytes(int(max_bits_table)))


def choose_bits_total_device(value, total_bits, min_bits=0, max_bits=None, workspace=None):
    """choose_bits_total without a host wait (cwq_choose_bits_total): the same
    60 halvings, taken several at a time from one pass over the table each, so
    the budgets and ``lam`` equal choose_bits_total's bit for bit.  Returns (bits
    int32 [nb], lam float64 [1], total int64 [1]) as cuda tensors; the call only
    enqueues launches on the current stream and, given ``workspace`` (a uint8
    cuda tensor of choose_bits_total_workspace_bytes), allocates nothing but its
    outputs.  Raises choose_bits_total's ValueError when ``min_bits`` everywhere
    exceeds the target."""
    lib = _lib.load()
    value = _table(value)
    nb, B = value.shape[0], value.shape[1] - 1
    lo_b = int(min_bits)
    hi_b = B if max_bits is None else min(int(max_bits), B)
    if not 0 <= lo_b <= hi_b:
        raise ValueError(f"min_bits={min_bits} outside [0, min(max_bits, {B})]")
    if nb * lo_b > int(total_bits):
        raise ValueError(f"{nb} blocks at min_bits={lo_b} exceed total_bits={total_bits}")
    dev = value.device
    bits = torch.empty(nb, dtype=torch.int32, device=dev)
    if nb == 0:  # the library launches nothing
        return (bits, torch.zeros(1, dtype=torch.float64, device=dev),
                torch.zeros(1, dtype=torch.int64, device=dev))
    lam = torch.empty(1, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    if workspace is None:
        workspace = torch.empty(choose_bits_total_workspace_bytes(B), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.cwq_choose_bits_total(_ptr(value), nb, B, int(total_bits), lo_b, hi_b, _ptr(bits),
                                       _ptr(lam), _ptr(total), workspace.data_ptr(),
                                       workspace.numel(), torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_choose_bits_total")
    return bits, lam, total


def encode_rate_total_workspace_bytes(nb, total_dims, max_block_dim, max_bits):
    """Workspace bytes of encode_blocks_rate_total (cwq_greedy_encode_rate_workspace_bytes)."""
    return int(_lib.load().cwq_greedy_encode_rate_workspace_bytes(
        int(nb), int(total_dims), int(max_block_dim), int(max_bits)))


def encode_blocks_rate_total(t_loc, t_scale, p_loc, p_scale, seed, max_bits, total_bits, min_bits=0,
                             rho=1., block_dim=None, block_off=None, block_id_base=0,
                             workspace=None, prune_mode=None):
    """encode_blocks_rate(total_bits=...) in one library call that only enqueues
    launches (cwq_greedy_encode_rate: the table, the budgets under the total, the
    indices read off the table, the decoder's sample), so it can be captured
    into a graph.  Returns (idx int32 [nb, 1], sample f32 [D], n_bits int32
    [nb], lam float64 [1], total int64 [1]) as cuda tensors; the first three are
    encode_blocks_rate's triple, bit for bit.  ``workspace``: a uint8 cuda tensor
    of encode_rate_total_workspace_bytes."""
    lib = _lib.load()
    _one_of(block_dim, block_off)
    dev = _device_of(t_loc, t_scale, p_loc, p_scale)
    tl = _f32(t_loc, dev, "t_loc")
    ts = _f32(t_scale, dev, "t_scale")
    pl = _f32(p_loc, dev, "p_loc")
    ps = _f32(p_scale, dev, "p_scale")
    D = tl.numel()
    if not (ts.numel() == pl.numel() == ps.numel() == D):
        raise ValueError("t_loc, t_scale, p_loc, p_scale must have the same size")
    if block_off is not None:
        offs, nb, longest = _offsets(block_off, D, dev)
    else:
        longest, nb = _nb_of(D, block_dim)
        offs = None
    B, lo_b = int(max_bits), int(min_bits)
    if 0 <= B <= MAX_BITS:  # (the library refuses any other B)
        if not 0 <= lo_b <= B:
            raise ValueError(f"min_bits={min_bits} outside [0, {B}]")
        if nb * lo_b > int(total_bits):
            raise ValueError(f"{nb} blocks at min_bits={lo_b} exceed total_bits={total_bits}")
    idx = torch.empty((nb, 1), dtype=torch.int32, device=dev)
    sample = torch.empty(D, dtype=torch.float32, device=dev)
    bits = torch.empty(nb, dtype=torch.int32, device=dev)
    lam = torch.zeros(1, dtype=torch.float64, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if workspace is None:
        need = encode_rate_total_workspace_bytes(nb, D, longest, B)
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(prune_mode)
    with torch.cuda.device(dev):
        rc = lib.cwq_greedy_encode_rate(
            _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, B, int(total_bits), lo_b, _seed32(seed), float(rho),
            int(block_id_base), _ptr(idx), _ptr(sample), _ptr(bits), _ptr(lam), _ptr(total), None,
            workspace.data_ptr(), workspace.numel(), opts,
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_greedy_encode_rate")
    return idx, sample, bits, lam, total


def code_grouped_greedy_sample_rate(target, proposal, n_bits_per_step, seed, total_bits=None,
                                    max_group_size_bits=12, rho=1.,
                                    extra_bits=1.0 / math.log(2.0), min_bits=0, prune_mode=None):
    """The single-step grouped coder with budgets from the groups' rate table.

    Standardisation, per-dim KL and partition are code_grouped_greedy_sample_var's
    at ``n_steps = 1``; the groups' budgets then come from encode_blocks_rate_total
    on the standardised groups with ``max_bits = n_bits_per_step``, under
    ``total_bits`` (None: what that call would spend, the sum of its block_bits
    budgets).  Returns code_grouped_greedy_sample_var's 5-tuple (sample, code
    bytes, total_bits, group_start_indices, group_bits), which
    ``decode_grouped_greedy_sample_var(code, starts, group_bits, proposal, 1,
    seed)`` decodes."""
    def encode(t_loc, t_scale, zeros, ones, kl_bits, starts):
        target_bits = int(kl_bits.sum(dtype=torch.int64).item()) if total_bits is None \
            else int(total_bits)
        idx, sample, bits, _, _ = encode_blocks_rate_total(
            t_loc, t_scale, zeros, ones, seed, n_bits_per_step, target_bits, min_bits=min_bits,
            rho=rho, block_off=starts, prune_mode=prune_mode)
        return idx, sample, bits

    return _code_grouped_var_with(encode, target, proposal, 1, n_bits_per_step, seed,
                                  max_group_size_bits, extra_bits, min_bits,
                                  encoder_chooses_bits=True)
