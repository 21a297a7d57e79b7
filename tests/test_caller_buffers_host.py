"""The helpers of tests/caller_buffers.py on the CPU: the offset view really is only element-aligned, contiguous, holds the tensor's values, and the
guard check sees a single overwritten word on either side and nothing else.  (The GPU tests that use them: tests/test_caller_buffers_gpu.py.)"""
import pytest
import torch

import test_config_matrix as TCM
from caller_buffers import MARGIN, PAYLOAD, Carved, margin_words, margins_intact, offset_view


def test_payload_is_the_guard_word_of_the_config_matrix():
    assert PAYLOAD == TCM.PAYLOAD == 0x7FC0BEEF
    assert torch.isnan(torch.tensor([PAYLOAD], dtype=torch.int32).view(torch.float32)).all()


@pytest.mark.parametrize("dtype,ks", [(torch.float32, (0, 1, 2, 3)), (torch.float64, (0, 1))])
@pytest.mark.parametrize("shape", [(1,), (2, 2, 7, 5), (3, 1001)])
def test_offset_view_alignment_values_and_margins(dtype, ks, shape):
    g = torch.Generator().manual_seed(5)
    t = torch.randn(shape, generator=g, dtype=dtype)
    for k in ks:
        buf, view = offset_view(t, k)
        assert view.data_ptr() % 16 == k * t.element_size()          # 4 * k for fp32, 8 for the one float64 offset
        assert view.is_contiguous() and view.shape == t.shape and view.dtype == dtype and torch.equal(view, t)
        assert view.data_ptr() >= buf.data_ptr() and view.data_ptr() + view.numel() * view.element_size() <= buf.data_ptr() + buf.numel() * buf.element_size()
        front, back = margin_words(buf, view)
        words = t.element_size() // 4
        assert front.numel() >= MARGIN * words and back.numel() >= MARGIN * words
        assert front.numel() + back.numel() + view.numel() * words == buf.numel() * words
        assert margins_intact(buf, view)
        view.mul_(2.0)                                               # writing the view leaves the margins alone ...
        assert margins_intact(buf, view) and torch.equal(view, 2.0 * t)
        for word in (front[-1:], back[:1], front[:1], back[-1:]):    # ... and one overwritten word next to it, or at either end, is seen
            keep = word.clone()
            word.fill_(0)
            assert not margins_intact(buf, view)
            word.copy_(keep)
            assert margins_intact(buf, view)


def test_offset_view_does_not_depend_on_where_the_allocator_put_the_buffer():
    """A base that is itself off a 16-byte boundary (a view handed in as the tensor's device memory would be) still gives the asked-for remainder."""
    t = torch.arange(10, dtype=torch.float32)
    seen = set()
    for _ in range(8):
        for k in range(4):
            buf, view = offset_view(t, k, margin=5)
            seen.add(buf.data_ptr() % 16)
            assert view.data_ptr() % 16 == 4 * k
    assert seen          # (whatever the allocator's alignment is, the view's remainder is the one asked for)


def test_carved_set_keeps_plain_tensors_plain_and_checks_every_guard():
    ts = {"a": torch.ones(2, 3), "b": torch.zeros(4, dtype=torch.float64), "c": None, "d": torch.full((5,), 2.0)}
    c = Carved(ts, "cpu", {"a": 3, "b": 1})
    assert c["c"] is None and set(c.bufs) == {"a", "b"}
    assert c["a"].data_ptr() % 16 == 12 and c["b"].data_ptr() % 16 == 8
    assert torch.equal(c["d"], ts["d"]) and c["d"].data_ptr() != ts["d"].data_ptr()
    c.check()
    front, _ = margin_words(c.bufs["b"], c["b"])
    front[-1] = 0
    with pytest.raises(AssertionError, match="b"):
        c.check()
