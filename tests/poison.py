"""Known contents for every buffer the Python wrappers hand to libcwq.so.

The wrappers allocate their workspaces, outputs and host staging with
``torch.empty``, ``torch.empty_like`` and ``np.empty`` (the only uninitialised
allocations in compression_without_quantization_amd/*.py).  ``poisoned(pattern)``
replaces those three for its duration: each wrapper calls the original and
fills the new buffer's bytes through a uint8 view, whatever its dtype and
wherever it lives (device, page-locked host, host).  A result that depends on
what a workspace or an output buffer held on entry then differs between
patterns (tests/test_workspace_state_gpu.py).

Patterns: 0x00 (the clean run), 0xFF (every float a NaN, every signed int -1,
every counter at its maximum), "random" (seeded bytes).

Guard bands (``poisoned(pattern, guard=True)``): the wrappers allocate exactly
the bytes a *_workspace_size function names, so a store past the end of a
workspace lands in whatever the allocator placed next and no result shows it.
In guard mode every device or page-locked uint8 buffer handed out is the
middle of a larger allocation, with GUARD_BYTES of GUARD_BYTE before and
after it (the data pointer stays 256-aligned, the guard after it starts at the
buffer's last byte + 1); ``Filled.assert_guards_intact()`` reads them back.

A plain module, not a conftest: nothing changes unless a test enters the
context manager.
"""
import contextlib
import threading

import numpy as np
import torch

GUARD_BYTES = 4096  # on either side of a guarded buffer
GUARD_BYTE = 0xA5   # no pattern's byte, no plausible counter, offset or float
_RANDOM_BLOCK = 1 << 20  # seeded bytes are drawn once per context and tiled over larger buffers


def _dtype_name(dtype):
    """'torch.uint8' for torch dtypes, numpy's own name ('float32') otherwise."""
    return str(dtype) if isinstance(dtype, torch.dtype) else np.dtype(dtype).name


class Filled:
    """What one ``poisoned`` context filled: (where, dtype, nbytes) per buffer,
    where in {"device", "pinned", "host"}."""

    def __init__(self, pattern):
        self.pattern = pattern
        self.buffers = []
        self.guards = []  # guard mode: (whole allocation, first byte handed out, bytes handed out)
        self._lock = threading.Lock()

    def _add(self, where, dtype, nbytes):
        with self._lock:
            self.buffers.append((where, _dtype_name(dtype), int(nbytes)))

    def count(self, where=None, dtype=None, min_bytes=0):
        return sum(1 for w, d, n in list(self.buffers)
                   if (where is None or w == where)
                   and (dtype is None or d == _dtype_name(dtype))
                   and n >= min_bytes)

    def assert_guards_intact(self, what=""):
        """Every byte before and after every guarded buffer still holds
        GUARD_BYTE (call after the device is idle).  Returns how many buffers
        were guarded, which the caller holds against what it expects."""
        for whole, start, n in self.guards:
            for side, band in (("before", whole[:start]), ("after", whole[start + n:])):
                bad = torch.nonzero(band != GUARD_BYTE).reshape(-1)
                at = int(bad[0]) + (-start if side == "before" else n) if bad.numel() else 0
                assert bad.numel() == 0, \
                    f"{what}: {bad.numel()} guard bytes {side} a {n}-byte " \
                    f"{'device' if whole.is_cuda else 'pinned'} buffer were overwritten, the " \
                    f"first at byte {at} of the buffer"
        return len(self.guards)

    def assert_workspace(self, need, what=""):
        """A condition of the test, not a measurement: a device uint8 buffer of
        at least ``need`` bytes (the entry point's *_workspace_size) was
        allocated through the patched functions, so the call under test did run
        on poisoned memory."""
        assert need > 0, f"{what}: workspace size {need}"
        assert self.count("device", torch.uint8, need) >= 1, \
            f"{what}: no device uint8 buffer of >= {need} bytes was filled with " \
            f"{self.pattern!r}: {self.buffers[-8:]}"


@contextlib.contextmanager
def poisoned(pattern, seed=0, guard=False):
    """Replace torch.empty, torch.empty_like and np.empty by versions that fill
    what they allocate with ``pattern`` (0x00, 0xFF or any byte, or "random");
    the originals come back on exit, also on error.  Yields a ``Filled``.
    guard: device and page-locked uint8 buffers get guard bands (above)."""
    if pattern != "random" and not (isinstance(pattern, int) and 0 <= pattern <= 255):
        raise ValueError(f"pattern {pattern!r}: a byte or 'random'")
    orig_empty, orig_empty_like, orig_np_empty = torch.empty, torch.empty_like, np.empty
    filled = Filled(pattern)
    busy = threading.local()  # re-entrancy: allocations made while filling pass through
    block = {}                # "random": the seeded block, drawn on first use
    state = {"at": 0}

    def host_block():
        # numpy's Generator.integers itself calls np.empty through the module
        # attribute: drawn under the busy flag, with the patched functions a
        # pass-through, or the fill would recurse without end
        if "host" not in block:
            rng = np.random.Generator(np.random.PCG64(seed))
            block["host"] = rng.integers(0, 256, _RANDOM_BLOCK, dtype=np.uint8)
        return block["host"]

    def random_bytes(n):
        b = host_block()
        at = state["at"] % _RANDOM_BLOCK
        state["at"] += 4099  # buffers of one size do not all start alike
        reps = (at + n + _RANDOM_BLOCK - 1) // _RANDOM_BLOCK
        return (b if reps == 1 else np.tile(b, reps))[at:at + n]

    def with_guards(t):
        """t (1-d uint8, device or page-locked) as the middle of a larger
        allocation of its kind between two guard bands."""
        n = t.numel()
        whole = orig_empty(n + 2 * GUARD_BYTES + 256, dtype=torch.uint8, device=t.device,
                           pin_memory=not t.is_cuda)
        start = GUARD_BYTES + (-(whole.data_ptr() + GUARD_BYTES)) % 256
        whole[:start] = GUARD_BYTE
        whole[start + n:] = GUARD_BYTE
        filled.guards.append((whole, start, n))
        return whole[start:start + n]

    def fill_tensor(t, whole_storage=True):
        """Fills t's whole storage, or (a guarded uint8 buffer) t alone; returns t."""
        if not isinstance(t, torch.Tensor) or t.is_meta or t.layout != torch.strided:
            return t
        st = t.untyped_storage()
        n = st.nbytes() if whole_storage else t.numel()
        where = "device" if t.is_cuda else ("pinned" if t.is_pinned() else "host")
        filled._add(where, t.dtype, n)
        if n == 0:
            return t
        with torch.no_grad():
            u8 = orig_empty(0, dtype=torch.uint8, device=t.device).set_(st) if whole_storage else t
            if pattern == "random":
                src = torch.from_numpy(np.ascontiguousarray(random_bytes(n)))
                u8.copy_(src)  # a synchronous upload: src may go once this returns
            else:
                u8.fill_(pattern)
        return t

    def fill_array(a):
        if not isinstance(a, np.ndarray) or a.dtype.hasobject:
            return a  # object arrays hold pointers: not bytes to overwrite
        filled._add("host", a.dtype, a.nbytes)
        if a.nbytes == 0:
            return a
        u8 = a.reshape(-1, order="A").view(np.uint8)  # a view: a fresh array is contiguous
        u8[...] = random_bytes(u8.size) if pattern == "random" else pattern
        return a

    def guarded(orig, fill):
        def wrapper(*args, **kwargs):
            out = orig(*args, **kwargs)
            if getattr(busy, "on", False):
                return out
            busy.on = True
            try:
                out = fill(out)
            finally:
                busy.on = False
            return out
        wrapper.__name__ = getattr(orig, "__name__", "empty")
        wrapper.__doc__ = getattr(orig, "__doc__", None)
        return wrapper

    def fill_or_guard(t):
        if not (guard and isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 1
                and t.numel() > 0 and (t.is_cuda or t.is_pinned())):
            return fill_tensor(t)
        return fill_tensor(with_guards(t), whole_storage=False)

    torch.empty = guarded(orig_empty, fill_or_guard)
    torch.empty_like = guarded(orig_empty_like, fill_tensor)
    np.empty = guarded(orig_np_empty, fill_array)
    try:
        yield filled
    finally:
        torch.empty, torch.empty_like, np.empty = orig_empty, orig_empty_like, orig_np_empty
