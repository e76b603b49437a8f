"""Guarded buffers: what a test hands to the C ABI (through ctypes, the only way to hand over exact sizes) so that WHERE a kernel
writes, and what it reads beyond its operands, is judged - not only the values.  Pure torch / numpy; works on CPU tensors
(tests/test_guarded_cpu.py shows every kind of violation being caught there, which is how a GPU test built on it is known to be
able to fail).

A guarded array is a contiguous view in the middle of a flat backing buffer, with a MOAT on each side:

    [ moat | offset_elems more moat words | the view | moat ]

  outputs and workspaces   the moat holds SENTINEL (a fixed, finite bit pattern, compared as integers); the interior is pre-filled
                           with quiet NaNs (0xff bytes for an integer or byte array), so an element the call did not write shows as
                           NaN instead of the stale - often correct - value a recycled allocation holds;
  inputs                   the moat holds quiet NaNs: a kernel that reads past an operand and multiplies what it read by a zero mask
                           turns its output non-finite (the only read check there is without a sanitizer).

The moat.  MOAT_FLOOR_BYTES = 64 KiB is the least a moat may be: 16 padded rows of the widest padded row the tests use are
16 x 256 floats = 16 KiB, so a kernel that stores a whole padded window past the end of Y - rows N .. ceil16(N) - 1, or the columns
D .. round_up(D, 16) - 1 of every row - lands inside it four times over.  The default, MOAT_BYTES = 320 KiB, also holds the scores
of a whole 16-row window of the densest row catalogued (65 536 edges per window: 256 KiB of ef) with 64 KiB of margin, so a kernel
that writes one window too many of an edge array is caught as well.  A write further away than that is not what these tests look for.

The view's address is `align`-aligned and NOT 2 x align-aligned, plus offset_elems elements: code that silently relies on more
alignment than the contract states meets an address that has exactly the stated one."""
import numpy as np
import torch

MOAT_FLOOR_BYTES = 64 * 1024
MOAT_BYTES = 320 * 1024
SENTINEL = 0x5A5A5A5A            # 1.54e16 as fp32, 0x5a as a byte: finite, and no value a kernel computes from the test data
QNAN = 0x7FC00000                # quiet NaN, fp32
_UNWRITTEN_BYTE = 0xFF           # interior of outputs: 0xffffffff is a NaN as fp32, 0xffff as fp16, -1 as int32


def _fill_words(t, word):
    """every 32-bit word of the flat tensor t (whole words long) set to the pattern"""
    t.view(torch.uint8).view(torch.int32).fill_(word if word < 2 ** 31 else word - 2 ** 32)


def guarded(dev, shape, dtype, fill, offset_elems=0, align=512, moat_bytes=MOAT_BYTES):
    """-> (buf, view).  buf: the flat backing buffer (dtype); view: a contiguous view of `shape` that starts
    moat + offset_elems elements into buf, at an address that is align-aligned (and not 2 align-aligned) + offset_elems elements.
    fill = "output": SENTINEL moats, interior unwritten (NaN).  fill = an array of `shape`: an input - its values inside NaN moats."""
    item = torch.empty(0, dtype=dtype).element_size()
    if moat_bytes < MOAT_FLOOR_BYTES:
        raise ValueError("a moat of %d bytes is below the %d-byte floor (16 padded rows of 256 floats, four times over)" % (moat_bytes, MOAT_FLOOR_BYTES))
    if moat_bytes % 4 or moat_bytes % item or align % 4 or align % item or offset_elems < 0:
        raise ValueError("moat and alignment must be whole elements and whole 32-bit words, the offset non-negative")
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    numel = int(np.prod(shape)) if shape else 1
    moat = moat_bytes // item
    tail_pad = (-(offset_elems + numel) * item) % 4          # (so that the buffer is whole 32-bit words)
    total = 2 * moat + offset_elems + numel + tail_pad // item
    raw = torch.empty(total * item + 2 * align, dtype=torch.uint8, device=dev)
    skip = (align - (raw.data_ptr() + moat_bytes)) % (2 * align)
    buf = raw[skip: skip + total * item].view(dtype)
    start = moat + offset_elems
    view = buf[start: start + numel].view(shape)
    is_output = isinstance(fill, str)
    if is_output:
        if fill != "output":
            raise ValueError("fill is 'output' or the input's values")
        pattern = SENTINEL
        _fill_words(buf, pattern)
        view.view(-1).view(torch.uint8).fill_(_UNWRITTEN_BYTE)
    else:
        pattern = QNAN
        _fill_words(buf, pattern)
        src = torch.as_tensor(np.ascontiguousarray(fill) if isinstance(fill, np.ndarray) else fill)
        if tuple(src.shape) != shape or src.dtype != dtype:
            raise ValueError("the input's values must have shape %s and dtype %s, got %s %s" % (shape, dtype, tuple(src.shape), src.dtype))
        view.copy_(src.to(dev))
    buf._guard = (pattern, start, numel, is_output)
    at = address(buf)
    assert view.is_contiguous() and (numel == 0 or view.data_ptr() == at), "guarded: the view is not where it was asked to be"
    assert (at - offset_elems * item) % align == 0 and (at - offset_elems * item) % (2 * align) == align, "guarded: the view has not exactly the alignment asked for"
    return buf, view


def address(buf):
    """the address of the guarded view's first element (what to hand to the C ABI: an EMPTY view has no data pointer of its own)"""
    return buf.data_ptr() + buf._guard[1] * buf.element_size()


def exact_workspace(dev, nbytes, moat_bytes=MOAT_BYTES):
    """-> (buf, view): a uint8 view of exactly nbytes at a 256-byte aligned (not 512) address inside SENTINEL moats, interior 0xff"""
    return guarded(dev, (int(nbytes),), torch.uint8, "output", align=256, moat_bytes=moat_bytes)


def moat_intact(buf, view):
    """-> the offsets (in elements, relative to the view's first element: negative in front, >= view.numel() behind) of the moat
    elements that no longer hold the pattern; an empty list when both moats are intact."""
    pattern, start, numel, _ = buf._guard
    assert view.numel() == numel and (numel == 0 or view.data_ptr() == address(buf)), "not this buffer's view"
    item = buf.element_size()
    words = buf.view(torch.uint8).view(torch.int32)          # (the buffer is whole words and starts on a word of the pattern)
    want = pattern if pattern < 2 ** 31 else pattern - 2 ** 32
    lo, hi = start * item, (start + numel) * item            # the view's bytes
    raw = buf.view(torch.uint8)
    pat = [(pattern >> (8 * k)) & 0xFF for k in range(4)]    # (little endian)
    suspects = list(range(lo // 4 * 4, lo)) + list(range(hi, (hi + 3) // 4 * 4))   # moat bytes of the (at most two) words shared with the view
    for w0, w1 in ((0, lo // 4), ((hi + 3) // 4, words.numel())):
        bad = torch.nonzero(words[w0:w1] != want).view(-1)
        suspects += [(int(w) + w0) * 4 + k for w in bad.cpu() for k in range(4)]   # only the changed words are looked at byte by byte
    changed = {b // item - start for b in suspects if int(raw[b]) != pat[b % 4]}
    return sorted(changed)


def unwritten(view):
    """number of elements of an output's interior that still hold the pre-fill (NaN for floats, 0xff bytes otherwise)"""
    if view.dtype.is_floating_point:
        return int(torch.isnan(view).sum())
    raw = view.contiguous().view(-1).view(torch.uint8).view(-1, view.element_size())
    return int((raw == _UNWRITTEN_BYTE).all(dim=1).sum())


def pristine(buf, view):
    """True when a refused call left an OUTPUT buffer as it was handed over, bit for bit: both moats intact, every interior byte 0xff"""
    assert buf._guard[3], "pristine() is for outputs"
    return not moat_intact(buf, view) and bool((view.contiguous().view(-1).view(torch.uint8) == _UNWRITTEN_BYTE).all())


def snapshot(t):
    return t.detach().clone()


def unchanged(t, snap):
    """bitwise equality (NaNs and signed zeros included) of a tensor with its snapshot"""
    if t.shape != snap.shape or t.dtype != snap.dtype:
        return False
    return bool(torch.equal(t.contiguous().view(-1).view(torch.uint8), snap.contiguous().view(-1).view(torch.uint8)))
