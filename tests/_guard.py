"""Guard bands and misaligned operands for the launches of bayesian_torch_amd.functional.  A plain module (no fixtures, no pytest
hooks), importable the way _grad_cases.py is; everything here runs on CPU tensors as well as on GPU tensors.

Every operand or result a test hands to a kernel can be made an interior view of ONE larger 1-d buffer:

- ``place(t, off)``: a contiguous copy of ``t`` that starts ``off`` fp32 elements past a 16-byte boundary (off 2: 8-byte aligned, the
  float2 / uint2 case), with ``band`` NaN elements on each side -- a read outside the tensor that is USED poisons the result;
- ``place_result(shape, off)``: the same for a buffer a kernel writes, body and bands filled with the quiet-NaN pattern ``PATTERN``;
  ``check`` then holds, after the launch and a synchronise, that both bands still hold the pattern bit for bit (nothing was written
  outside) and that no body element does (every element was written);
- ``guarded_allocations(off)``: replaces the name ``torch`` inside bayesian_torch_amd.functional by a proxy whose ``empty`` /
  ``empty_like`` return such result buffers and record them: out, kl, dx, dmu, drho, the backward workspace, the packs, the packed
  draws, the rng_fill_* / mc_epilogue / max-pool outputs -- with no product change;
- ``seated_workspace(owner, device, scratch)``: puts a guarded buffer where ``_lib.workspace`` keeps the zero-initialised one: its
  64 KiB head must read all zero after every launch, the scratch behind it holds the pattern BEFORE the launch ("contents never
  matter"), and its bands are checked like any result's.
"""
import contextlib

import torch

PATTERN = 0x7FE5A5A5          # a quiet NaN no kernel computes: compared as int32
BAND = 4096                   # elements on each side: >= the widest row any read-out stores in one pass (512 pixels), and >= 4096


def _i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


class Guarded:
    """A result buffer inside its bands.  ``view``: what the kernel gets.  ``words``: the whole allocation as int32."""

    def __init__(self, words, start, nbytes, view, tag=""):
        self.words, self.start, self.nbytes, self.view, self.tag = words, start, nbytes, view, tag

    @property
    def n_words(self):
        return (self.nbytes + 3) // 4


def _carve(nbytes, off, band, device):
    """-> (int32 words of one allocation, index of the first body word): the body starts 4 * off bytes past a 16-byte boundary, has
    at least ``band`` words before it and behind it."""
    if off not in (0, 1, 2, 3):
        raise ValueError("off must be 0, 1, 2 or 3")
    nw = (nbytes + 3) // 4
    words = torch.empty(nw + 2 * band + 8, dtype=torch.int32, device=device)
    if words.data_ptr() % 4:
        raise RuntimeError("allocation is not 4-byte aligned")
    first = (words.data_ptr() // 4 + band)                      # word address of the earliest possible start
    start = band + (off - first) % 4
    assert (words.data_ptr() + 4 * start) % 16 == 4 * off and start >= band and start + nw + band <= words.numel()
    return words, start


def place(t, off, band=BAND):
    """A contiguous copy of the fp32 tensor ``t`` as an interior view: data_ptr() % 16 == 4 * off, ``band`` NaNs before and behind."""
    if t.dtype != torch.float32:
        raise TypeError("place: fp32 tensors")
    words, start = _carve(4 * t.numel(), off, band, t.device)
    buf = words.view(torch.float32)
    buf.fill_(float("nan"))
    view = buf[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def place_result(shape, off, band=BAND, device="cpu", dtype=torch.float32, tag=""):
    """A result buffer of ``shape`` / ``dtype`` at element offset ``off`` (in fp32 words), body and bands filled with PATTERN."""
    shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (int(shape),)
    n = 1
    for d in shape:
        n *= int(d)
    es = torch.empty((), dtype=dtype).element_size()
    words, start = _carve(n * es, off, band, device)
    words.fill_(_i32(PATTERN))
    nw = (n * es + 3) // 4
    view = words[start:start + nw].view(dtype)[:n].view(shape)
    assert view.is_contiguous() and view.data_ptr() == words.data_ptr() + 4 * start
    return Guarded(words, start, n * es, view, tag)


def _first_bad(mask):
    idx = mask.nonzero()
    return None if idx.numel() == 0 else int(idx[0])


def check(buf, body=True):
    """After the launch and a synchronise: both bands still hold PATTERN, and (``body``) no whole body word does.  Raises
    AssertionError naming the first offending word offset relative to the body's first element (negative: the band before it)."""
    w, s, nw = buf.words, buf.start, buf.n_words
    pat = _i32(PATTERN)
    bad = _first_bad(w[:s] != pat)
    if bad is None:
        hi = _first_bad(w[s + nw:] != pat)
        bad = None if hi is None else s + nw + hi
    assert bad is None, f"{buf.tag or 'buffer'}: write outside the result at word offset {bad - s} (body holds {nw} words)"
    if body:
        whole = buf.nbytes // 4          # (a last partial word of a byte buffer keeps pattern bytes)
        hole = _first_bad(w[s:s + whole] == pat)
        assert hole is None, f"{buf.tag or 'buffer'}: element at word offset {hole} was never written (body holds {nw} words)"


class _TorchProxy:
    """``torch`` as bayesian_torch_amd.functional sees it under guarded_allocations: empty / empty_like hand out guarded buffers."""

    def __init__(self, real, off, band, log):
        self._real, self._off, self._band, self._log = real, off, band, log

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _make(self, shape, dtype, device):
        off = self._off(shape, dtype) if callable(self._off) else self._off
        g = place_result(shape, off, self._band, device, dtype, tag=f"empty{tuple(shape)} {dtype}")
        self._log.append(g)
        return g.view

    def empty(self, *size, dtype=None, device=None, **kw):
        if kw:
            raise TypeError(f"guarded empty: unexpected {sorted(kw)}")
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        return self._make(tuple(int(d) for d in size), dtype or torch.float32, "cpu" if device is None else device)

    def empty_like(self, t, **kw):
        if kw:
            raise TypeError(f"guarded empty_like: unexpected {sorted(kw)}")
        return self._make(tuple(t.shape), t.dtype, t.device)


@contextlib.contextmanager
def guarded_allocations(off, band=BAND):
    """Inside: every torch.empty / empty_like of bayesian_torch_amd.functional is a guarded result buffer at offset ``off`` (an int,
    or ``off(shape, dtype) -> int``).  Yields the list they are recorded in, in allocation order.  Restores the module on exit."""
    from bayesian_torch_amd import functional as F
    real, log = F.torch, []
    F.torch = _TorchProxy(real, off, band, log)
    try:
        yield log
    finally:
        F.torch = real


def check_all(log, body=lambda g: g.view.dtype == torch.float32):
    """check() over a recorded list; the body test for the buffers ``body(g)`` selects (default: the fp32 ones -- a byte workspace
    or a packed sign image promises no written-everywhere)."""
    for g in log:
        check(g, body=bool(body(g)))


@contextlib.contextmanager
def seated_workspace(owner, device, scratch=0, band=BAND):
    """Seat a guarded buffer as _lib.workspace(owner, device): 64 KiB of zeros, then ``scratch`` bytes (rounded as _lib.workspace
    rounds them) of PATTERN.  Yields the Guarded buffer; ``check_workspace`` holds it after a launch.  Restores the entry on exit."""
    from bayesian_torch_amd import _lib
    need = _lib.WORKSPACE_BYTES + ((int(scratch) + 255) // 256) * 256
    g = place_result((need,), 0, band, device, torch.uint8, tag=f"workspace {owner}")
    g.view[:_lib.WORKSPACE_BYTES].zero_()
    dev = torch.device(device)
    key = (owner, dev.index if dev.index is not None else torch.cuda.current_device())
    had, old = key in _lib._ws, _lib._ws.get(key)
    _lib._ws[key] = g.view
    try:
        yield g
    finally:
        if had:
            _lib._ws[key] = old
        else:
            _lib._ws.pop(key, None)


def check_workspace(g):
    """Bands intact, and the zero-initialised head reads all zero again."""
    from bayesian_torch_amd import _lib
    check(g, body=False)
    nz = _first_bad(g.view[:_lib.WORKSPACE_BYTES] != 0)
    assert nz is None, f"{g.tag}: byte {nz} of the zero-initialised head is not zero after the launch"
