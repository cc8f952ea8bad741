"""Backfitting for the greedy coder: re-choose steps, same decoders.

A multi-step greedy code picks each step's row given the steps before it and
never looks back.  Backfitting is coordinate ascent over the steps of a
finished code (cwq_greedy_backfit, include/cwq.h states the definition): for
step s every other step's row is held, all ``2**n_bits_per_step`` rows of step
s's stream are scored against their sum, and the best row replaces the step's
if the decoded sample's log-density gets larger.  The result is still one row
index per step: the indices, the bit string and the ``.miracle`` file are those
of the greedy coder, and every existing decoder reads them.  No block ever
ends below the code it started from, and a sweep costs about one
``encode_blocks`` call.

  backfit_blocks                      refine an index table
  encode_blocks_backfit               encode_blocks (or a beam), then refine
  code_grouped_greedy_sample_backfit  code_grouped_greedy_sample, refined

and with a bit budget per block (cwq_greedy_backfit_var: block g is refined as
backfit_blocks refines it at ``n_bits[g]``, all blocks in one call):

  backfit_blocks_var                      refine encode_blocks_var's table
  encode_blocks_var_backfit               encode_blocks_var (or a beam), then refine
  code_grouped_greedy_sample_var_backfit  code_grouped_greedy_sample_var, refined

All arithmetic runs in libcwq.so; nothing here computes samples on the CPU.
"""
import math

import numpy as np
import torch

from . import _lib
from .beam import _code_grouped_with, encode_blocks_beam, encode_blocks_var_beam
from .coded_greedy_sampler import _device_of, _f32, _ptr, encode_blocks
from .varbits import (_bits_tensor, _code_grouped_var_with, _nb_of, _offsets, _one_of, _seed32,
                      encode_blocks_var)

MAX_SWEEPS = 16  # CWQ_MAX_BACKFIT_SWEEPS


def backfit_workspace_bytes(nb, total_dims, max_block_dim, n_steps):
    """Workspace bytes of backfit_blocks (cwq_greedy_backfit_workspace_size):
    encode_blocks' for ragged blocks plus ``4 * n_steps`` bytes per dim."""
    return int(_lib.load().cwq_greedy_backfit_workspace_size(
        int(nb), int(total_dims), int(max_block_dim), int(n_steps)))


def backfit_blocks(idx, t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps, seed, sweeps,
                   rho=1., block_dim=None, block_off=None, block_id_base=0, return_value=False,
                   return_accepted=False, prune_mode=None, workspace=None, eval_events=None):
    """``sweeps`` backfitting sweeps (0 .. 16) over the index table ``idx``
    ([nb, n_steps], from encode_blocks, encode_blocks_beam or anywhere else;
    it is not modified).

    Blocks are uniform (``block_dim``) or ragged (``block_off``, nb + 1
    offsets); block g's streams are those of seed ``seed + block_id_base + g``.
    Returns (idx int32 [nb, n_steps], sample f32 [D]) as cuda tensors, then with
    ``return_value`` the sample's log-density as the coder's keys hold it (f32
    [nb]) and with ``return_accepted`` the replacements accepted per block
    (int32 [nb]).  ``sweeps=0`` returns the table with its decoded sample and
    value; a code of one step is returned as given.  ``prune_mode`` selects the
    scoring kernels as in encode_blocks; results never depend on it.

    The table's entries must lie in ``[0, 2**n_bits_per_step)``: they are
    checked here, which waits for the device, except while the current stream
    is being captured into a graph (the call itself is asynchronous and
    capturable; pass ``workspace`` then).
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
    n_steps, sweeps, n_bits = int(n_steps), int(sweeps), int(n_bits_per_step)
    table = torch.as_tensor(idx if isinstance(idx, torch.Tensor) else np.asarray(idx))
    if table.numel() != nb * max(n_steps, 0):
        raise ValueError(f"idx holds {table.numel()} entries, not nb * n_steps = {nb * n_steps}")
    out_idx = table.to(device=dev, dtype=torch.int32, copy=True).reshape(nb, max(n_steps, 0))
    out_idx = out_idx.contiguous()
    if 0 <= n_bits <= 30 and out_idx.numel() and not torch.cuda.is_current_stream_capturing():
        if bool(((out_idx < 0) | (out_idx >= (1 << n_bits))).any()):
            raise ValueError(f"idx holds an index outside [0, {1 << n_bits})")
    out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    out_value = torch.empty(nb, dtype=torch.float32, device=dev) if return_value else None
    out_acc = torch.empty(nb, dtype=torch.int32, device=dev) if return_accepted else None
    need = backfit_workspace_bytes(nb, D, longest, n_steps)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(prune_mode, eval_events)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.cwq_greedy_backfit(
            _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, n_bits, n_steps, sweeps, _seed32(seed), float(rho),
            int(block_id_base), _ptr(out_idx), _ptr(out_sample), _ptr(out_value), _ptr(out_acc),
            workspace.data_ptr(), workspace.numel(), opts, stream)
    _lib.check(rc, "cwq_greedy_backfit")
    out = (out_idx, out_sample)
    if return_value:
        out += (out_value,)
    if return_accepted:
        out += (out_acc,)
    return out


def encode_blocks_backfit(t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps, seed, sweeps,
                          beam=1, rho=1., block_dim=None, block_off=None, block_id_base=0,
                          return_value=False, return_accepted=False, prune_mode=None):
    """encode_blocks (``beam=1``) or encode_blocks_beam (``beam > 1``), then
    ``sweeps`` backfitting sweeps over its table.  Returns what backfit_blocks
    returns; with ``sweeps=0`` that is the encoder's own result."""
    _one_of(block_dim, block_off)
    kw = dict(rho=rho, block_dim=block_dim, block_off=block_off, block_id_base=block_id_base)
    if int(beam) > 1:
        idx, _ = encode_blocks_beam(t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps,
                                    seed, beam, **kw)
    else:
        idx, _ = encode_blocks(t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps, seed,
                               prune_mode=prune_mode, **kw)
    return backfit_blocks(idx, t_loc, t_scale, p_loc, p_scale, n_bits_per_step, n_steps, seed,
                          sweeps, return_value=return_value, return_accepted=return_accepted,
                          prune_mode=prune_mode, **kw)


def code_grouped_greedy_sample_backfit(target, proposal, n_steps, n_bits_per_step, seed, sweeps,
                                       beam=1, max_group_size_bits=12, rho=1.):
    """code_grouped_greedy_sample with ``sweeps`` backfitting sweeps per group
    (after a beam of ``beam`` partial sums when ``beam > 1``).

    The standardisation, the per-dim KL and the partition are those of
    code_grouped_greedy_sample; group g is coded with seed ``seed + g`` on the
    standard proposal by encode_blocks_backfit.  Returns (sample np.float32
    [D], bitcode str, group_start_indices list with D appended), the triple of
    code_grouped_greedy_sample, which ``sweeps=0, beam=1`` reproduces;
    decode_grouped_greedy_sample decodes it.
    """
    def encode(t_loc, t_scale, zeros, ones, starts):
        return encode_blocks_backfit(t_loc, t_scale, zeros, ones, n_bits_per_step, n_steps, seed,
                                     sweeps, beam=beam, rho=rho, block_off=starts)
    return _code_grouped_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                              max_group_size_bits)


# ---------------------------------------------------------------------------
# a bit budget per block
# ---------------------------------------------------------------------------
def backfit_var_workspace_bytes(nb, total_dims, max_block_dim, n_steps, uniform=False):
    """Workspace bytes of backfit_blocks_var, as include/cwq.h states them: the
    budget call's layout plus what backfitting adds to the encoder's (the
    selected rows, values and counts); uniform blocks (``max_block_dim`` dims
    each) also hold the sorted table, ``4 * nb * n_steps`` bytes rounded up to
    256."""
    lib = _lib.load()
    nb, D, d, n_steps = int(nb), int(total_dims), int(max_block_dim), int(n_steps)
    extra = int(lib.cwq_greedy_backfit_workspace_size(nb, D, d, n_steps)) - \
        int(lib.cwq_greedy_encode_workspace_size(nb, D, d))
    if uniform:
        return int(lib.cwq_greedy_encode_uniform_var_workspace_size(nb, d)) + \
            (4 * nb * n_steps + 255) // 256 * 256 + extra
    return int(lib.cwq_greedy_encode_var_workspace_size(nb, D, d, n_steps)) + extra


def backfit_blocks_var(idx, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, sweeps,
                       rho=1., block_dim=None, block_off=None, block_id_base=0,
                       return_value=False, return_accepted=False, prune_mode=None,
                       workspace=None, eval_events=None):
    """backfit_blocks with a bit count per block: block g is refined exactly as
    ``backfit_blocks(..., n_bits[g], ...)`` refines it (seed ``seed +
    block_id_base + g``).  ``idx``: the table [nb, n_steps] of encode_blocks_var
    (or any other whose row g lies in ``[0, 2**n_bits[g])``); it is not
    modified.  ``n_bits``: int tensor, array or list of nb counts in [0, 30].
    Returns what backfit_blocks returns.

    The call waits for the device once (the bucket sizes decide its launches),
    so it cannot be captured into a graph; the table's range and the counts
    are checked on the device in that wait, and a refusal raises CwqError.
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
    n_steps, sweeps = int(n_steps), int(sweeps)
    table = torch.as_tensor(idx if isinstance(idx, torch.Tensor) else np.asarray(idx))
    if table.numel() != nb * max(n_steps, 0):
        raise ValueError(f"idx holds {table.numel()} entries, not nb * n_steps = {nb * n_steps}")
    out_idx = table.to(device=dev, dtype=torch.int32, copy=True).reshape(nb, max(n_steps, 0))
    out_idx = out_idx.contiguous()
    out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    out_value = torch.empty(nb, dtype=torch.float32, device=dev) if return_value else None
    out_acc = torch.empty(nb, dtype=torch.int32, device=dev) if return_accepted else None
    if workspace is None:
        need = backfit_var_workspace_bytes(nb, D, longest, max(n_steps, 1), uniform=offs is None)
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(prune_mode, eval_events)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.cwq_greedy_backfit_var(
            _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr() if offs is not None else None,
            nb, D, longest, _ptr(bits), n_steps, sweeps, _seed32(seed), float(rho),
            int(block_id_base), _ptr(out_idx), _ptr(out_sample), _ptr(out_value), _ptr(out_acc),
            workspace.data_ptr(), workspace.numel(), opts, stream)
    _lib.check(rc, "cwq_greedy_backfit_var")
    out = (out_idx, out_sample)
    if return_value:
        out += (out_value,)
    if return_accepted:
        out += (out_acc,)
    return out


def encode_blocks_var_backfit(t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, sweeps,
                              rho=1., block_dim=None, block_off=None, block_id_base=0,
                              return_value=False, return_accepted=False, prune_mode=None, beam=1):
    """encode_blocks_var (``beam=1``) or encode_blocks_var_beam (``beam > 1``),
    then ``sweeps`` backfitting sweeps over its table.  Returns what
    backfit_blocks_var returns; with ``sweeps=0`` that is the encoder's own
    result."""
    _one_of(block_dim, block_off)
    kw = dict(rho=rho, block_dim=block_dim, block_off=block_off, block_id_base=block_id_base,
              prune_mode=prune_mode)
    if int(beam) > 1:
        idx, _ = encode_blocks_var_beam(t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed,
                                        beam, rho=rho, block_dim=block_dim, block_off=block_off,
                                        block_id_base=block_id_base)
    else:
        idx, _ = encode_blocks_var(t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, **kw)
    return backfit_blocks_var(idx, t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, sweeps,
                              return_value=return_value, return_accepted=return_accepted, **kw)


def code_grouped_greedy_sample_var_backfit(target, proposal, n_steps, n_bits_per_step, seed,
                                           sweeps, max_group_size_bits=12, rho=1.,
                                           extra_bits=1.0 / math.log(2.0), min_bits=0,
                                           prune_mode=None, beam=1):
    """code_grouped_greedy_sample_var with ``sweeps`` backfitting sweeps per
    group (after a beam of ``beam`` partial sums when ``beam > 1``), each group
    at its own budget.

    The standardisation, the per-dim KL, the partition and the budgets are
    those of code_grouped_greedy_sample_var; group g is coded with seed ``seed
    + g`` on the standard proposal by encode_blocks_var_backfit.  Returns the
    5-tuple of code_grouped_greedy_sample_var (sample, code bytes, total_bits,
    group starts, group_bits), which ``sweeps=0, beam=1`` reproduces byte for
    byte; the budgets, hence total_bits, depend on neither, and
    decode_grouped_greedy_sample_var decodes the result.
    """
    def encode(t_loc, t_scale, zeros, ones, bits, starts):
        return encode_blocks_var_backfit(t_loc, t_scale, zeros, ones, bits, n_steps, seed, sweeps,
                                         rho=rho, block_off=starts, prune_mode=prune_mode,
                                         beam=beam)
    return _code_grouped_var_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                                  max_group_size_bits, extra_bits, min_bits)
