"""The greedy coder with a beam over its steps.

``encode_blocks`` keeps the single best partial sum after every step.  With
more than one step that is a poor search: the best row of step 1 need not lie
on the best two-step path.  The calls here keep the ``beam`` best partial sums
instead (cwq_beam_encode, include/cwq.h states the definition).  Every beam of
a step is scored against the same candidate rows, so the result is still one
row index per step: the indices, the bit string and the ``.miracle`` file are
those of the greedy coder, and every existing decoder reads them.  A beam
sample has a higher target log-density than the greedy one on average, not
block by block; ``beam=1`` is the greedy coder bit for bit.

  encode_blocks_beam               encode_blocks with a beam
  code_grouped_greedy_sample_beam  code_grouped_greedy_sample with a beam

and with a bit budget per block (cwq_beam_encode_var: block g is coded as
encode_blocks_beam codes it at ``n_bits[g]``, all blocks in one launch
sequence, no sort and no wait):

  encode_blocks_var_beam               encode_blocks_var with a beam
  code_grouped_greedy_sample_var_beam  code_grouped_greedy_sample_var with a beam

All arithmetic runs in libcwq.so; nothing here computes samples on the CPU.
"""
import math

import numpy as np
import torch

from . import _lib
from .binary_io import indices_to_bitcode
from .coded_greedy_sampler import _device_of, _dist_parts, _f32, _group_starts_array, _ptr
from .varbits import (MAX_BITS, _bits_tensor, _code_grouped_var_with, _nb_of, _offsets, _one_of,
                      _seed32)

MAX_BEAM = 16  # CWQ_MAX_BEAM


def beam_workspace_bytes(nb, total_dims, max_block_dim, n_steps, beam):
    """Workspace bytes of encode_blocks_beam (cwq_beam_encode_workspace_size):
    about ``(3 + 2 beam) * 4`` bytes per dim plus the key lists."""
    return int(_lib.load().cwq_beam_encode_workspace_size(
        int(nb), int(total_dims), int(max_block_dim), int(n_steps), int(beam)))


def encode_blocks_beam(t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps, seed, beam,
                       rho=1., block_dim=None, block_off=None, block_id_base=0,
                       return_value=False, workspace=None, eval_events=None, _path=None):
    """encode_blocks with the ``beam`` best partial sums kept after each step
    (1 <= beam <= 16, any value; ``beam * 2**n_bits_per_step <= 2**31``).

    Blocks are uniform (``block_dim``) or ragged (``block_off``, nb + 1
    offsets); block g is coded with seed ``seed + block_id_base + g``.  Returns
    (idx int32 [nb, n_steps], sample f32 [D]) as cuda tensors, and with
    ``return_value`` also the log-density the last step's selection saw for the
    returned sample (f32 [nb]).  The outputs feed ``decode_blocks`` and
    ``indices_to_bitcode`` unchanged.  The call is asynchronous on the current
    stream and can be captured into a graph (pass ``workspace`` then);
    ``eval_events``: (start, stop) hipEvent_t handles around the scoring launches.
    """
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
    n_steps, beam = int(n_steps), int(beam)
    out_idx = torch.empty((nb, max(n_steps, 0)), dtype=torch.int32, device=dev)
    out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    out_value = torch.empty(nb, dtype=torch.float32, device=dev) if return_value else None
    need = beam_workspace_bytes(nb, D, longest, n_steps, beam)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(None, eval_events)
    args = (_ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, int(n_bits_per_step), n_steps, beam, _seed32(seed), float(rho),
            int(block_id_base), _ptr(out_idx), _ptr(out_sample), _ptr(out_value),
            workspace.data_ptr(), workspace.numel(), opts)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if _path is None:
            rc = lib.cwq_beam_encode(*args, stream)
        else:  # the tests' kernel and tiling choice
            rc = lib.cwq_selftest_beam_encode(*args, stream, int(_path))
    _lib.check(rc, "cwq_beam_encode")
    return (out_idx, out_sample, out_value) if return_value else (out_idx, out_sample)


def _code_grouped_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                       max_group_size_bits):
    """code_grouped_greedy_sample's pipeline around a block encoder: standardise,
    per-dim KL, partition, ``encode(t_loc, t_scale, zeros, ones, starts)`` ->
    (idx, sample) on the standard proposal, destandardise, bit string."""
    lib = _lib.load()
    dev = _device_of(target.loc, target.scale, proposal.loc, proposal.scale)
    q_loc, q_scale = _dist_parts(target, dev, "Target")
    p_loc, p_scale = _dist_parts(proposal, dev, "Proposal")
    D = p_loc.numel()
    n_steps, n_bits_per_step = int(n_steps), int(n_bits_per_step)
    t_loc = torch.empty(D, dtype=torch.float32, device=dev)
    t_scale = torch.empty(D, dtype=torch.float32, device=dev)
    kl = torch.empty(D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.cwq_standardise(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc), _ptr(p_scale), D,
                                       _ptr(t_loc), _ptr(t_scale), stream), "cwq_standardise")
        _lib.check(lib.cwq_kl_normal_normal(_ptr(q_loc), _ptr(q_scale), _ptr(p_loc),
                                            _ptr(p_scale), D, _ptr(kl), stream),
                   "cwq_kl_normal_normal")
    starts = _group_starts_array(kl.cpu().numpy(), n_bits_per_step * n_steps,
                                 max_group_size_bits)
    zeros = torch.zeros(D, dtype=torch.float32, device=dev)
    ones = torch.ones(D, dtype=torch.float32, device=dev)
    idx, sample = encode(t_loc, t_scale, zeros, ones, starts)
    out = torch.empty(D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cwq_destandardise(_ptr(sample), _ptr(p_loc), _ptr(p_scale), D, _ptr(out),
                                         torch.cuda.current_stream(dev).cuda_stream),
                   "cwq_destandardise")
    bitcode = indices_to_bitcode(idx.cpu().numpy(), n_bits_per_step)
    return out.cpu().numpy(), bitcode, starts.tolist()


def code_grouped_greedy_sample_beam(target, proposal, n_steps, n_bits_per_step, seed, beam,
                                    max_group_size_bits=12, rho=1.):
    """code_grouped_greedy_sample with a beam of ``beam`` partial sums per group.

    The standardisation, the per-dim KL and the partition are those of
    code_grouped_greedy_sample; group g is coded with seed ``seed + g`` on the
    standard proposal by encode_blocks_beam.  Returns (sample np.float32 [D],
    bitcode str, group_start_indices list with D appended), the triple of
    code_grouped_greedy_sample, which ``beam=1`` reproduces;
    decode_grouped_greedy_sample decodes it.
    """
    def encode(t_loc, t_scale, zeros, ones, starts):
        return encode_blocks_beam(t_loc, t_scale, zeros, ones, n_bits_per_step, n_steps, seed,
                                  beam, rho=rho, block_off=starts)
    return _code_grouped_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                              max_group_size_bits)


# ---------------------------------------------------------------------------
# a bit budget per block
# ---------------------------------------------------------------------------
def encode_blocks_var_beam(t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, beam, rho=1.,
                           block_dim=None, block_off=None, block_id_base=0, return_value=False,
                           workspace=None, eval_events=None, max_bits=None, check=True,
                           _path=None):
    """encode_blocks_beam with a bit count per block: block g is coded exactly
    as ``encode_blocks_beam(..., n_bits[g], ...)`` codes it in a call of its own
    (seed ``seed + block_id_base + g``), all blocks in one launch sequence.
    ``n_bits``: int tensor, array or list of nb counts in [0, 30];
    ``beam * 2**max(n_bits) <= 2**31``.  Returns what encode_blocks_beam
    returns; row g of the indices lies in ``[0, 2**n_bits[g])``, the table
    decode_blocks_var, pack_indices and backfit_blocks_var read.  ``beam=1`` is
    encode_blocks_var bit for bit.

    ``check=True`` reads the counts' smallest and largest (one wait for the
    device) and raises ValueError for a count outside [0, 30] or above a given
    ``max_bits``; without ``max_bits`` the largest count is taken.  With
    ``check=False`` ``max_bits`` is required, nothing waits, and a count outside
    ``[0, max_bits]`` is read as clamped to it (cwq_beam_encode_var): pass a
    ``workspace`` (beam_workspace_bytes) as well and the call can be captured
    into a graph.
    """
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
    bits = _bits_tensor(n_bits, nb, dev)
    if max_bits is not None:
        max_bits = int(max_bits)
        if not 0 <= max_bits <= MAX_BITS:
            raise ValueError(f"max_bits={max_bits} outside [0, {MAX_BITS}]")
    if check:
        lo, hi = (int(v) for v in torch.aminmax(bits)) if nb else (0, 0)
        top = MAX_BITS if max_bits is None else max_bits
        if lo < 0 or hi > top:
            raise ValueError(f"n_bits holds a count outside [0, {top}]")
        if max_bits is None:
            max_bits = hi
    elif max_bits is None:
        raise ValueError("check=False needs max_bits, the bound the counts are read under")
    n_steps, beam = int(n_steps), int(beam)
    out_idx = torch.empty((nb, max(n_steps, 0)), dtype=torch.int32, device=dev)
    out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    out_value = torch.empty(nb, dtype=torch.float32, device=dev) if return_value else None
    if workspace is None:
        need = beam_workspace_bytes(nb, D, longest, n_steps, beam)
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(None, eval_events)
    args = (_ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, _ptr(bits), max_bits, n_steps, beam, _seed32(seed), float(rho),
            int(block_id_base), _ptr(out_idx), _ptr(out_sample), _ptr(out_value),
            workspace.data_ptr(), workspace.numel(), opts)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if _path is None:
            rc = lib.cwq_beam_encode_var(*args, stream)
        else:  # the tests' kernel and tiling choice
            rc = lib.cwq_selftest_beam_encode_var(*args, stream, int(_path))
    _lib.check(rc, "cwq_beam_encode_var")
    return (out_idx, out_sample, out_value) if return_value else (out_idx, out_sample)


def code_grouped_greedy_sample_var_beam(target, proposal, n_steps, n_bits_per_step, seed, beam,
                                        max_group_size_bits=12, rho=1.,
                                        extra_bits=1.0 / math.log(2.0), min_bits=0):
    """code_grouped_greedy_sample_var with a beam of ``beam`` partial sums per
    group, each group at its own budget.

    The standardisation, the per-dim KL, the partition and the budgets are
    those of code_grouped_greedy_sample_var; group g is coded with seed ``seed
    + g`` on the standard proposal by encode_blocks_var_beam with ``max_bits =
    n_bits_per_step`` (the budgets' own upper clamp).  Returns the 5-tuple of
    code_grouped_greedy_sample_var (sample, code bytes, total_bits, group
    starts, group_bits), which ``beam=1`` reproduces byte for byte; the budgets,
    hence total_bits, do not depend on ``beam``, and
    decode_grouped_greedy_sample_var decodes the result.
    """
    def encode(t_loc, t_scale, zeros, ones, bits, starts):
        return encode_blocks_var_beam(t_loc, t_scale, zeros, ones, bits, n_steps, seed, beam,
                                      rho=rho, block_off=starts, max_bits=n_bits_per_step)
    return _code_grouped_var_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                                  max_group_size_bits, extra_bits, min_bits)
