"""Blocks (uniform or CSR) with a bit budget of their own, and their packed bitstream.

``encode_blocks`` spends one ``n_bits_per_step`` on every block of a call.
Rows of real latents differ in KL, and a greedy coder needs about KL_g bits
for row g, so here every block carries its own count:

  block_bits          the budget of each block from its KL (cwq_block_bits)
  encode_blocks_var   encode_blocks with ``n_bits`` per block
                      (cwq_greedy_encode_uniform_var: the blocks are sorted by
                      budget and each budget runs the tuned uniform encoder)
  pack_indices        the indices as the bytes binary_io writes for their
  unpack_indices      joined to_bit_string fields, made and read on the device
  decode_blocks_var   the inverse of encode_blocks_var, from indices or bytes
  code_grouped_greedy_sample_var / decode_grouped_greedy_sample_var
                      the grouped coder with a budget per group

Every entry takes uniform blocks (``block_dim``) or ragged ones (``block_off``,
nb + 1 offsets: cwq_block_bits_csr, cwq_greedy_encode_var), exactly one of the
two.  The bit counts are side information the caller ships (5 bits per block raw).
All arithmetic runs in libcwq.so; nothing here computes samples on the CPU.
"""
import math

import numpy as np
import torch

from . import _lib
from .coded_greedy_sampler import _device_of, _dist_parts, _f32, _group_starts_array, _ptr

MAX_BITS = 30  # CWQ_MAX_BITS_PER_STEP


def _seed32(seed):
    return int(np.int32(np.uint32(int(seed) & 0xFFFFFFFF)))


def _bits_tensor(n_bits, nb, dev):
    """``n_bits`` (tensor, array or list) as a contiguous int32 cuda tensor [nb]."""
    if isinstance(n_bits, torch.Tensor):
        t = n_bits
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f"n_bits must hold integers, got {t.dtype}")
    else:
        a = np.asarray(n_bits)
        if a.size == 0:
            a = a.astype(np.int32)
        if a.dtype.kind not in "iu":
            raise TypeError(f"n_bits must hold integers, got {a.dtype}")
        # out-of-range values must reach the library as such: clip to int32 first
        t = torch.from_numpy(np.ascontiguousarray(np.clip(a, -1, MAX_BITS + 1).astype(np.int32)))
    t = t.reshape(-1)
    if t.numel() != nb:
        raise ValueError(f"n_bits holds {t.numel()} counts for {nb} blocks")
    if t.dtype != torch.int32:
        t = t.clamp(-1, MAX_BITS + 1).to(torch.int32)
    return t.to(device=dev).contiguous()


def _nb_of(D, block_dim):
    block_dim = int(block_dim)
    if block_dim < 0 or (block_dim == 0 and D != 0) or (block_dim and D % block_dim):
        raise ValueError(f"D={D} is not a multiple of block_dim={block_dim}")
    return block_dim, (D // block_dim if block_dim else 0)


def _offsets(block_off, D, dev):
    """``block_off`` checked as encode_blocks checks it: (device int64 tensor,
    nb, longest block)."""
    offs_h = np.asarray(block_off.cpu() if isinstance(block_off, torch.Tensor)
                        else block_off, dtype=np.int64).reshape(-1)
    nb = offs_h.size - 1
    if nb < 0 or offs_h[0] != 0 or offs_h[-1] != D or (np.diff(offs_h) < 0).any():
        raise ValueError("block_off must be non-decreasing from 0 to D")
    longest = int(np.diff(offs_h).max()) if nb > 0 else 0
    return torch.from_numpy(offs_h).to(dev), nb, longest


def _one_of(block_dim, block_off):
    if (block_dim is None) == (block_off is None):
        raise ValueError("give exactly one of block_dim / block_off")


def block_bits(post_loc, post_scale, prior_loc, prior_scale, block_dim=None,
               extra_bits=1.0 / math.log(2.0), min_bits=0, max_bits=MAX_BITS,
               return_kl_bits=False, block_off=None, n_steps=1):
    """The bit budget of each uniform block of ``block_dim`` dims:
    ``clamp(ceil(KL_g / ln 2 + extra_bits), min_bits, max_bits)`` with KL_g the
    float64 sum of the block's float32 per-dim KL(post || prior); a non-finite
    KL_g gives ``max_bits``.  The default margin is the reference's: it closes
    a group at ``n_bits ln 2 - 1`` nats (coded_greedy_sampler.py:226).
    With ``block_off`` (nb + 1 offsets) the blocks are ragged and the budget is
    per step of a code of ``n_steps`` steps:
    ``clamp(ceil((KL_g / ln 2 + extra_bits) / n_steps), min_bits, max_bits)``.
    Returns an int32 cuda tensor [nb] (with ``return_kl_bits`` also KL_g / ln 2
    as float32 [nb], for logging)."""
    lib = _lib.load()
    dev = _device_of(post_loc, post_scale, prior_loc, prior_scale)
    ql = _f32(post_loc, dev, "post_loc")
    qs = _f32(post_scale, dev, "post_scale")
    pl = _f32(prior_loc, dev, "prior_loc")
    ps = _f32(prior_scale, dev, "prior_scale")
    D = ql.numel()
    if not (qs.numel() == pl.numel() == ps.numel() == D):
        raise ValueError("post_loc, post_scale, prior_loc, prior_scale must have the same size")
    _one_of(block_dim, block_off)
    if block_off is not None:
        offs, nb, _ = _offsets(block_off, D, dev)
    else:
        if int(n_steps) != 1:
            raise ValueError("n_steps applies to block_off (ragged blocks) only")
        block_dim, nb = _nb_of(D, block_dim)
    bits = torch.empty(nb, dtype=torch.int32, device=dev)
    klb = torch.empty(nb, dtype=torch.float32, device=dev) if return_kl_bits else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if block_off is not None:
            rc = lib.cwq_block_bits_csr(_ptr(ql), _ptr(qs), _ptr(pl), _ptr(ps), offs.data_ptr(),
                                        nb, D, float(extra_bits), int(n_steps), int(min_bits),
                                        int(max_bits), _ptr(bits), _ptr(klb), stream)
        else:
            rc = lib.cwq_block_bits(_ptr(ql), _ptr(qs), _ptr(pl), _ptr(ps), nb, block_dim,
                                    float(extra_bits), int(min_bits), int(max_bits), _ptr(bits),
                                    _ptr(klb), stream)
    _lib.check(rc, "cwq_block_bits")
    return (bits, klb) if return_kl_bits else bits


def encode_var_workspace_bytes(nb, block_dim, n_steps=1):
    """Workspace bytes of encode_blocks_var (include/cwq.h: the size function
    covers n_steps <= 4 d, more steps stage their indices in a tail)."""
    need = int(_lib.load().cwq_greedy_encode_uniform_var_workspace_size(int(nb), int(block_dim)))
    if int(n_steps) > 4 * int(block_dim):
        need += (4 * int(nb) * int(n_steps) + 255) // 256 * 256
    return need


def encode_blocks_var(t_loc, t_scale, p_loc, p_scale, n_bits, n_steps, seed, rho=1.,
                      block_dim=None, block_id_base=0, out_idx=None, out_sample=None,
                      workspace=None, prune_mode=None, eval_events=None, block_off=None,
                      max_block_dim=None):
    """encode_blocks over uniform blocks of ``block_dim``, or ragged blocks
    ``block_off`` (nb + 1 offsets), with a bit count per
    block: block g is coded exactly as ``encode_blocks(..., n_bits[g], ...)``
    codes it (seed ``seed + block_id_base + g``).  ``n_bits``: int tensor,
    array or list of nb counts in [0, 30].  Returns (idx int32 [nb, n_steps],
    sample f32 [D]) as cuda tensors.  The call waits for the device once (the
    bucket sizes decide its launches), so it cannot be captured into a graph.
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
        if max_block_dim is None:
            max_block_dim = longest
    else:
        block_dim, nb = _nb_of(D, block_dim)
    bits = _bits_tensor(n_bits, nb, dev)
    n_steps = int(n_steps)
    if out_idx is None:
        out_idx = torch.empty((nb, n_steps), dtype=torch.int32, device=dev)
    if out_sample is None:
        out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    if block_off is not None:
        need = int(lib.cwq_greedy_encode_var_workspace_size(nb, D, int(max_block_dim), n_steps))
    else:
        need = encode_var_workspace_bytes(nb, block_dim, n_steps)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    opts = _lib.options(prune_mode, eval_events)
    if block_off is not None:
        with torch.cuda.device(dev):
            rc = lib.cwq_greedy_encode_var(
                _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), offs.data_ptr(), nb, D,
                int(max_block_dim), _ptr(bits), n_steps, _seed32(seed), float(rho),
                int(block_id_base), _ptr(out_idx), _ptr(out_sample), workspace.data_ptr(),
                workspace.numel(), opts, torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "cwq_greedy_encode_var")
        return out_idx, out_sample
    with torch.cuda.device(dev):
        rc = lib.cwq_greedy_encode_uniform_var(
            _ptr(tl), _ptr(ts), _ptr(pl), _ptr(ps), nb, block_dim, _ptr(bits), n_steps,
            _seed32(seed), float(rho), int(block_id_base), _ptr(out_idx), _ptr(out_sample),
            workspace.data_ptr(), workspace.numel(), opts,
            torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_greedy_encode_uniform_var")
    return out_idx, out_sample


def _pack_ws(lib, nb, dev):
    return torch.empty(max(int(lib.cwq_pack_indices_var_workspace_size(nb)), 1),
                       dtype=torch.uint8, device=dev)


def pack_indices(idx, n_bits):
    """The indices [nb, n_steps] as a packed stream: field (g, s) is
    ``to_bit_string(idx[g, s], n_bits[g])``, fields in block then step order,
    the bit string packed MSB-first into bytes with a zero-padded last byte
    (``binary_io._pack_bits``).  Returns (uint8 cuda tensor, total_bits)."""
    lib = _lib.load()
    dev = _device_of(idx, n_bits)
    it = idx if isinstance(idx, torch.Tensor) else torch.from_numpy(np.asarray(idx))
    if it.dim() != 2:
        raise ValueError("idx must be [nb, n_steps]")
    nb, n_steps = int(it.shape[0]), int(it.shape[1])
    it = it.to(device=dev, dtype=torch.int32).contiguous()
    bits = _bits_tensor(n_bits, nb, dev)
    if nb == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), 0
    if n_steps < 1:
        raise ValueError("idx must hold at least one step per block")
    # the buffer's size from the counts; the device's own total must agree
    expect = int(bits.clamp(0, MAX_BITS).sum(dtype=torch.int64).item()) * n_steps
    n_bytes = (expect + 7) // 8
    out = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = _pack_ws(lib, nb, dev)
    with torch.cuda.device(dev):
        rc = lib.cwq_pack_indices_var(_ptr(it), _ptr(bits), nb, n_steps, _ptr(out), n_bytes,
                                      total.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_pack_indices_var")
    got = int(total.item())
    if got < 0:
        raise _lib.CwqError(f"cwq_pack_indices_var failed: n_bits values outside [0, {MAX_BITS}]")
    if got != expect:
        raise _lib.CwqError(f"cwq_pack_indices_var wrote {got} bits, the counts give {expect}")
    return out, got


def unpack_indices(code, n_bits, n_steps):
    """Inverse of pack_indices: ``code`` (uint8 tensor, bytes or ndarray) back
    to int32 indices [nb, n_steps] (cuda).  Bits past the end of ``code`` read
    as 0, the project's rule for short codes."""
    lib = _lib.load()
    dev = _device_of(code, n_bits)
    if isinstance(code, (bytes, bytearray, memoryview)):
        code = np.frombuffer(bytes(code), dtype=np.uint8)
    ct = code if isinstance(code, torch.Tensor) else torch.from_numpy(np.array(code, copy=True))
    if ct.dtype != torch.uint8:
        raise TypeError(f"code must be uint8, got {ct.dtype}")
    ct = ct.to(device=dev).contiguous().reshape(-1)
    nb = int(n_bits.numel() if isinstance(n_bits, torch.Tensor) else np.asarray(n_bits).size)
    bits = _bits_tensor(n_bits, nb, dev)
    n_steps = int(n_steps)
    if n_steps < 1:
        raise ValueError(f"n_steps={n_steps} must be >= 1")
    if nb and (int(bits.min().item()) < 0 or int(bits.max().item()) > MAX_BITS):
        raise _lib.CwqError(f"cwq_unpack_indices_var failed: n_bits values outside "
                            f"[0, {MAX_BITS}]")
    out = torch.empty((nb, n_steps), dtype=torch.int32, device=dev)
    ws = _pack_ws(lib, nb, dev)
    with torch.cuda.device(dev):
        rc = lib.cwq_unpack_indices_var(_ptr(ct), ct.numel(), _ptr(bits), nb, n_steps, _ptr(out),
                                        ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "cwq_unpack_indices_var")
    return out


def decode_blocks_var(code_or_idx, n_bits, p_loc, p_scale, n_steps, seed, rho=1.,
                      block_dim=None, block_id_base=0, out_sample=None, block_off=None):
    """Inverse of encode_blocks_var.  ``code_or_idx``: the packed stream (uint8
    tensor / ndarray, bytes) or the indices themselves (any other integer
    array, nb * n_steps of them).  The decoders use the bit count only as the
    indices' range, so the unpacked indices go to the plain uniform (or, with
    ``block_off``, CSR) decoder at the largest count."""
    lib = _lib.load()
    _one_of(block_dim, block_off)
    dev = _device_of(code_or_idx, p_loc, p_scale)
    pl = _f32(p_loc, dev, "p_loc")
    ps = _f32(p_scale, dev, "p_scale")
    D = pl.numel()
    if ps.numel() != D:
        raise ValueError("p_loc and p_scale must have the same size")
    if block_off is not None:
        offs, nb, longest = _offsets(block_off, D, dev)
    else:
        block_dim, nb = _nb_of(D, block_dim)
    n_steps = int(n_steps)
    bits = _bits_tensor(n_bits, nb, dev)
    is_code = isinstance(code_or_idx, (bytes, bytearray, memoryview)) or \
        (isinstance(code_or_idx, torch.Tensor) and code_or_idx.dtype == torch.uint8) or \
        (isinstance(code_or_idx, np.ndarray) and code_or_idx.dtype == np.uint8)
    if is_code:
        it = unpack_indices(code_or_idx, bits, n_steps).reshape(-1)
    else:
        it = code_or_idx if isinstance(code_or_idx, torch.Tensor) \
            else torch.from_numpy(np.asarray(code_or_idx))
        it = it.to(device=dev, dtype=torch.int32).contiguous().reshape(-1)
        if it.numel() != nb * n_steps:
            raise ValueError("idx must hold nb * n_steps entries")
        # indices that came from elsewhere: each must fit its block's count
        lim = (torch.ones_like(bits) << bits.clamp(0, MAX_BITS)).repeat_interleave(n_steps)
        if nb and bool(((it < 0) | (it >= lim)).any().item()):
            raise ValueError("an index does not fit its block's bit count")
    if out_sample is None:
        out_sample = torch.empty(D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if block_off is not None:
            rc = lib.cwq_greedy_decode(
                _ptr(it), _ptr(pl), _ptr(ps), offs.data_ptr(), nb, D, longest, MAX_BITS, n_steps,
                _seed32(seed), float(rho), int(block_id_base), _ptr(out_sample), stream)
        else:
            rc = lib.cwq_greedy_decode_uniform(
                _ptr(it), _ptr(pl), _ptr(ps), nb, block_dim, MAX_BITS, n_steps, _seed32(seed),
                float(rho), int(block_id_base), _ptr(out_sample), stream)
    _lib.check(rc, "cwq_greedy_decode_uniform" if block_off is None else "cwq_greedy_decode")
    return out_sample


# ---------------------------------------------------------------------------
# the grouped coder with a budget per group (composed from the calls above)
# ---------------------------------------------------------------------------
def _code_grouped_var_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                           max_group_size_bits, extra_bits, min_bits, encoder_chooses_bits=False):
    """code_grouped_greedy_sample_var's pipeline around a block encoder:
    standardise, per-dim KL, partition, budgets, ``encode(t_loc, t_scale, zeros,
    ones, bits, starts)`` -> (idx, sample) on the standard proposal,
    destandardise, pack_indices.  With ``encoder_chooses_bits`` the encoder
    returns (idx, sample, the budgets it coded at) and those are packed and
    returned in place of block_bits' budgets."""
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
    # the budgets sum the float32 per-dim KLs the partition saw (same arithmetic)
    bits = block_bits(q_loc, q_scale, p_loc, p_scale, block_off=starts, extra_bits=extra_bits,
                      n_steps=n_steps, min_bits=min_bits, max_bits=n_bits_per_step)
    zeros = torch.zeros(D, dtype=torch.float32, device=dev)
    ones = torch.ones(D, dtype=torch.float32, device=dev)
    if encoder_chooses_bits:
        idx, sample, bits = encode(t_loc, t_scale, zeros, ones, bits, starts)
    else:
        idx, sample = encode(t_loc, t_scale, zeros, ones, bits, starts)
    out = torch.empty(D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cwq_destandardise(_ptr(sample), _ptr(p_loc), _ptr(p_scale), D, _ptr(out),
                                         torch.cuda.current_stream(dev).cuda_stream),
                   "cwq_destandardise")
    code, total_bits = pack_indices(idx, bits)
    return (out.cpu().numpy(), code.cpu().numpy().tobytes(), total_bits, starts.tolist(),
            bits.cpu().numpy())


def code_grouped_greedy_sample_var(target, proposal, n_steps, n_bits_per_step, seed,
                                   max_group_size_bits=12, rho=1.,
                                   extra_bits=1.0 / math.log(2.0), min_bits=0, prune_mode=None):
    """code_grouped_greedy_sample with a bit count per group.

    The standardisation, the per-dim KL and the partition are those of
    code_grouped_greedy_sample (``n_bits_per_step * n_steps`` decides where a
    group closes); group g is then coded with seed ``seed + g`` at
    ``block_bits(block_off=starts, n_steps=n_steps, min_bits=min_bits,
    max_bits=n_bits_per_step)[g]`` bits per step instead of ``n_bits_per_step``,
    so no group spends more than the reference call, and
    ``min_bits = n_bits_per_step`` gives its sample and indices exactly.
    Returns (sample np.float32 [D], code bytes (pack_indices), total_bits,
    group_start_indices list with D appended, group_bits np.int32 [G]); the
    decoder needs the last two next to the code.  ``prune_mode``: the encoder's
    cwq_options.prune_mode; results never depend on it.  Leave it at the
    default: buckets of long groups at fewer than 12 bits are then scored with a
    wave per candidate row (c2low: 18.7 ms against 82-88 ms with
    ``prune_mode=0``).
    """
    def encode(t_loc, t_scale, zeros, ones, bits, starts):
        return encode_blocks_var(t_loc, t_scale, zeros, ones, bits, n_steps, seed, rho=rho,
                                 block_off=starts, prune_mode=prune_mode)
    return _code_grouped_var_with(encode, target, proposal, n_steps, n_bits_per_step, seed,
                                  max_group_size_bits, extra_bits, min_bits)


def decode_grouped_greedy_sample_var(code, group_start_indices, group_bits, proposal, n_steps,
                                     seed, rho=1.):
    """Inverse of code_grouped_greedy_sample_var.  Returns np.float32 [D]."""
    lib = _lib.load()
    dev = _device_of(proposal.loc, proposal.scale)
    p_loc, p_scale = _dist_parts(proposal, dev, "Proposal")
    D = p_loc.numel()
    G = int(np.asarray(group_bits.cpu() if isinstance(group_bits, torch.Tensor)
                       else group_bits).size)
    offs = np.asarray(group_start_indices, dtype=np.int64).reshape(-1)
    if offs.size == G:  # a list without its end
        offs = np.append(offs, D)
    if offs.size != G + 1:
        raise ValueError(f"{offs.size} group starts for {G} group budgets")
    zeros = torch.zeros(D, dtype=torch.float32, device=dev)
    ones = torch.ones(D, dtype=torch.float32, device=dev)
    sample = decode_blocks_var(code, group_bits, zeros, ones, n_steps, seed, rho=rho,
                               block_off=offs)
    out = torch.empty(D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.cwq_destandardise(_ptr(sample), _ptr(p_loc), _ptr(p_scale), D, _ptr(out),
                                         torch.cuda.current_stream(dev).cuda_stream),
                   "cwq_destandardise")
    return out.cpu().numpy()
