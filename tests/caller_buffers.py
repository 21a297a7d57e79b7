"""Caller-owned tensors carved out of larger allocations: views that are only element-aligned, between guard words.

The C ABI (include/helmnet_hip.h, "alignment and overlap") promises that a tensor argument needs no more than the alignment of its element type
unless an entry point says otherwise.  ``offset_view`` builds such an argument: a contiguous view that starts ``k`` elements past a 16-byte boundary
inside a larger buffer whose margins hold the guard word of tests/test_config_matrix.py (``PAYLOAD``, the idea of its ``_guarded``), and
``margins_intact`` says afterwards whether every margin word still holds it: an out-of-bounds write overwrites the payload, an out-of-bounds read
brings it into the result (a quiet NaN for fp32; as a double, 0x7FC0BEEF7FC0BEEF is 1.6e307, which no result survives either).

Used by tests/test_caller_buffers_host.py (the helper itself, on the CPU) and tests/test_caller_buffers_gpu.py.
"""
import torch

from test_config_matrix import PAYLOAD

MARGIN = 4096          # guard elements on either side (at least; up to 3 more in front, see offset_view)


def offset_view(t, k, margin=MARGIN, device=None):
    """(buffer, view): ``view`` has the shape, dtype and values of ``t``, is contiguous, and starts ``k`` elements past a 16-byte boundary of
    ``buffer`` (``view.data_ptr() % 16 == k * itemsize``: k in 0..3 for fp32, 0..1 for float64), wherever the allocator put the buffer.  Everything
    outside the view holds PAYLOAD in every 32-bit word; there are at least ``margin`` guard elements on either side."""
    item = t.element_size()
    per16 = 16 // item
    assert item in (4, 8) and 0 <= k < per16, (item, k)
    device = t.device if device is None else device
    buf = torch.empty(2 * margin + per16 + t.numel(), dtype=t.dtype, device=device)
    buf.view(torch.int32).fill_(PAYLOAD)
    assert buf.data_ptr() % item == 0
    start = margin + (k - (buf.data_ptr() // item + margin)) % per16
    view = buf[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def margin_words(buf, view):
    """The two guard regions of ``buf`` around ``view`` as int32 words (front, back)."""
    item = view.element_size()
    start = (view.data_ptr() - buf.data_ptr()) // item
    assert 0 <= start and start + view.numel() <= buf.numel()
    return buf[:start].view(torch.int32), buf[start + view.numel():].view(torch.int32)


def margins_intact(buf, view):
    front, back = margin_words(buf, view)
    return bool((front == PAYLOAD).all()) and bool((back == PAYLOAD).all())


class Carved:
    """A set of named tensors, each either plain (its own allocation) or an offset view between guard words.

    ``Carved(tensors, device, offsets={name: k})``: names missing from ``offsets`` (or with k None) stay plain copies.  ``c[name]`` is what to hand
    to the library; ``c.check()`` asserts every guard word of every carved tensor."""

    def __init__(self, tensors, device, offsets=None, margin=MARGIN):
        offsets = offsets or {}
        self.t, self.bufs = {}, {}
        for name, v in tensors.items():
            k = offsets.get(name)
            if v is None:
                self.t[name] = None
            elif k is None:
                self.t[name] = v.to(device).clone().contiguous()
            else:
                self.bufs[name], self.t[name] = offset_view(v.to(device), k, margin)
                assert self.t[name].data_ptr() % 16 == k * v.element_size() and self.t[name].is_contiguous()

    def __getitem__(self, name):
        return self.t[name]

    def check(self):
        bad = [name for name, buf in self.bufs.items() if not margins_intact(buf, self.t[name])]
        assert not bad, f"guard words overwritten around {bad}"
