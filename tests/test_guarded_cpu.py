"""tests/guarded.py on CPU tensors: every kind of violation of the C ABI's memory contract (include/tcgnn.h "Alignment", "Workspace
size", "fully overwritten") is caught by the helper - which is how a GPU test built on it is known to be able to fail, without ever
making a kernel misbehave.  No GPU needed."""
import numpy as np
import pytest
import torch

import guarded as G

CPU = torch.device("cpu")
N, D = 17, 41                      # a ragged last window (N % 16 = 1), a row that is no multiple of 4 or 16


def _output(offset=0, align=512):
    buf, view = G.guarded(CPU, (N, D), torch.float32, "output", offset_elems=offset, align=align)
    return buf, view


def _written(view):
    view.copy_(torch.arange(view.numel(), dtype=torch.float32).view(view.shape))


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("align", [16, 256, 512])
def test_the_view_sits_where_it_was_asked_to(offset, align):
    buf, view = _output(offset, align)
    assert view.shape == (N, D) and view.is_contiguous() and view.dtype == torch.float32
    assert (view.data_ptr() - 4 * offset) % align == 0 and (view.data_ptr() - 4 * offset) % (2 * align) == align   # exactly the stated alignment
    moat = G.MOAT_BYTES // 4
    assert (view.data_ptr() - buf.data_ptr()) // 4 == moat + offset and buf.numel() >= 2 * moat + offset + N * D
    assert G.unwritten(view) == N * D and G.pristine(buf, view) and G.moat_intact(buf, view) == []
    words = buf.view(torch.int32)
    assert int(words[0]) == G.SENTINEL and int(words[moat + offset - 1]) == G.SENTINEL and int(words[moat + offset + N * D]) == G.SENTINEL
    _written(view)
    assert G.unwritten(view) == 0 and not G.pristine(buf, view) and G.moat_intact(buf, view) == []


def test_one_word_just_before_the_view_is_caught():
    buf, view = _output(1)
    _written(view)
    start = (view.data_ptr() - buf.data_ptr()) // 4
    buf[start - 1] = 0.0
    assert G.moat_intact(buf, view) == [-1]


def test_one_word_just_after_the_view_is_caught():
    buf, view = _output()
    _written(view)
    start = (view.data_ptr() - buf.data_ptr()) // 4
    buf[start + N * D] = 1.0
    assert G.moat_intact(buf, view) == [N * D]


def test_a_write_sixteen_rows_past_the_end_is_caught():
    """a kernel that stores the padded window - rows N .. - or a whole window too many, 256 padded floats per row"""
    buf, view = _output()
    _written(view)
    start = (view.data_ptr() - buf.data_ptr()) // 4
    for pitch in (D, 48, 256):
        far = N * D + 16 * pitch - 1                     # the last element of the sixteenth row past the end
        assert far * 4 < N * D * 4 + G.MOAT_FLOOR_BYTES   # inside even the smallest moat allowed
        buf[start + far] = 2.0
        assert far in G.moat_intact(buf, view)
    assert len(G.moat_intact(buf, view)) == 3


def test_a_sentinel_valued_write_is_the_one_thing_not_seen_and_a_changed_bit_is():
    buf, view = _output()
    start = (view.data_ptr() - buf.data_ptr()) // 4
    words = buf.view(torch.int32)
    words[start - 5] = G.SENTINEL                        # (writing the pattern itself changes nothing: no kernel computes 1.54e16 from the test data)
    assert G.moat_intact(buf, view) == []
    words[start - 5] = G.SENTINEL ^ 1                    # one bit
    assert G.moat_intact(buf, view) == [-5]


def test_an_interior_element_left_unwritten_is_caught():
    buf, view = _output()
    _written(view)
    assert G.unwritten(view) == 0
    view[N - 1, D - 1] = float("nan")                    # what the pre-fill leaves where nothing was stored
    assert G.unwritten(view) == 1
    ints_buf, ints = G.guarded(CPU, (5,), torch.int32, "output")
    assert G.unwritten(ints) == 5
    ints[:4] = torch.arange(4, dtype=torch.int32)
    assert G.unwritten(ints) == 1 and G.moat_intact(ints_buf, ints) == []


def test_a_refused_call_must_leave_the_output_pristine():
    buf, view = _output()
    assert G.pristine(buf, view)
    view[3, 3] = 0.0                                     # a memset that ran before the refusal
    assert not G.pristine(buf, view)


def test_one_bit_of_a_snapshot_changed_is_caught():
    x = np.random.default_rng(0).standard_normal((N, D)).astype(np.float32)
    x[2, 2] = np.nan; x[3, 3] = -0.0
    buf, view = G.guarded(CPU, (N, D), torch.float32, x)
    snap = G.snapshot(view)
    assert G.unchanged(view, snap) and G.moat_intact(buf, view) == []           # (a NaN equals itself bit for bit)
    view.view(torch.int32)[7, 7] ^= 1
    assert not G.unchanged(view, snap)
    view.view(torch.int32)[7, 7] ^= 1
    view[3, 3] = 0.0                                                            # -0.0 -> +0.0: equal as floats, not as bits
    assert not G.unchanged(view, snap)
    assert not G.unchanged(view[:5], snap)


def test_inputs_sit_in_quiet_nans():
    x = np.ones((N, D), np.float32)
    buf, view = G.guarded(CPU, (N, D), torch.float32, x, offset_elems=1)
    start = (view.data_ptr() - buf.data_ptr()) // 4
    assert bool(torch.isnan(buf[:start]).all()) and bool(torch.isnan(buf[start + N * D:]).all()) and bool((view == 1).all())
    assert int(buf.view(torch.int32)[start - 1]) == G.QNAN
    buf[start + N * D + 2] = 0.0
    assert G.moat_intact(buf, view) == [N * D + 2]
    with pytest.raises(ValueError, match="shape"):
        G.guarded(CPU, (N, D + 1), torch.float32, x)


def test_a_moat_below_the_floor_is_refused():
    assert G.MOAT_FLOOR_BYTES == 64 * 1024 and G.MOAT_BYTES >= G.MOAT_FLOOR_BYTES + 65536 * 4   # a 65 536-edge window of ef, with margin
    assert G.MOAT_FLOOR_BYTES >= 4 * 16 * 256 * 4                                               # 16 padded rows of 256 floats, four times over
    with pytest.raises(ValueError, match="floor"):
        G.guarded(CPU, (N, D), torch.float32, "output", moat_bytes=G.MOAT_FLOOR_BYTES - 4)
    with pytest.raises(ValueError, match="floor"):
        G.exact_workspace(CPU, 1000, moat_bytes=4096)
    G.guarded(CPU, (N, D), torch.float32, "output", moat_bytes=G.MOAT_FLOOR_BYTES)


@pytest.mark.parametrize("nbytes", [0, 1, 255, 256, 4099])
def test_exact_workspace(nbytes):
    buf, ws = G.exact_workspace(CPU, nbytes)
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and G.address(buf) % 512 == 256 and (nbytes == 0 or ws.data_ptr() == G.address(buf))
    assert G.pristine(buf, ws) and bool((ws == 0xFF).all())
    start = G.address(buf) - buf.data_ptr()
    assert start == G.MOAT_BYTES and buf.numel() - start - nbytes >= G.MOAT_BYTES
    ws.zero_()
    assert G.moat_intact(buf, ws) == []
    buf[start + nbytes] = 0                              # the byte a size that is one slot short would write
    buf[start - 1] = 7
    assert G.moat_intact(buf, ws) == [-1, nbytes]


def test_an_empty_array_is_guarded_too():
    buf, view = G.guarded(CPU, (0,), torch.float32, "output")
    assert view.numel() == 0 and G.pristine(buf, view) and G.unwritten(view) == 0
    buf[G.MOAT_BYTES // 4] = 0.0                         # where element 0 would be
    assert G.moat_intact(buf, view) == [0]
