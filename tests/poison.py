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

A plain module, not a conftest: nothing changes unless a test enters the
context manager.
"""
import contextlib
import threading

import numpy as np
import torch

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
        self._lock = threading.Lock()

    def _add(self, where, dtype, nbytes):
        with self._lock:
            self.buffers.append((where, _dtype_name(dtype), int(nbytes)))

    def count(self, where=None, dtype=None, min_bytes=0):
        return sum(1 for w, d, n in list(self.buffers)
                   if (where is None or w == where)
                   and (dtype is None or d == _dtype_name(dtype))
                   and n >= min_bytes)

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
def poisoned(pattern, seed=0):
    """Replace torch.empty, torch.empty_like and np.empty by versions that fill
    what they allocate with ``pattern`` (0x00, 0xFF or any byte, or "random");
    the originals come back on exit, also on error.  Yields a ``Filled``."""
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

    def fill_tensor(t):
        if not isinstance(t, torch.Tensor) or t.is_meta or t.layout != torch.strided:
            return
        st = t.untyped_storage()
        n = st.nbytes()
        where = "device" if t.is_cuda else ("pinned" if t.is_pinned() else "host")
        filled._add(where, t.dtype, n)
        if n == 0:
            return
        with torch.no_grad():
            u8 = orig_empty(0, dtype=torch.uint8, device=t.device).set_(st)
            if pattern == "random":
                src = torch.from_numpy(np.ascontiguousarray(random_bytes(n)))
                u8.copy_(src)  # a synchronous upload: src may go once this returns
            else:
                u8.fill_(pattern)

    def fill_array(a):
        if not isinstance(a, np.ndarray) or a.dtype.hasobject:
            return  # object arrays hold pointers: not bytes to overwrite
        filled._add("host", a.dtype, a.nbytes)
        if a.nbytes == 0:
            return
        u8 = a.reshape(-1, order="A").view(np.uint8)  # a view: a fresh array is contiguous
        u8[...] = random_bytes(u8.size) if pattern == "random" else pattern

    def guarded(orig, fill):
        def wrapper(*args, **kwargs):
            out = orig(*args, **kwargs)
            if getattr(busy, "on", False):
                return out
            busy.on = True
            try:
                fill(out)
            finally:
                busy.on = False
            return out
        wrapper.__name__ = getattr(orig, "__name__", "empty")
        wrapper.__doc__ = getattr(orig, "__doc__", None)
        return wrapper

    torch.empty = guarded(orig_empty, fill_tensor)
    torch.empty_like = guarded(orig_empty_like, fill_tensor)
    np.empty = guarded(orig_np_empty, fill_array)
    try:
        yield filled
    finally:
        torch.empty, torch.empty_like, np.empty = orig_empty, orig_empty_like, orig_np_empty
