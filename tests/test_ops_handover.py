"""The hand-over record one conv block's backward keeps for its neighbours (_ops._Handover), on plain CPU tensors: they
have data_ptr() and _version, which is all the record looks at."""
import pytest
import torch

from pix2pixhdaudiosr_amd import _lib, _ops


def test_take_sums_only_for_the_tensor_the_consumer_wrote():
    sums, gx = torch.ones(2, 8, 2), torch.zeros(2, 4, 4, 8)
    ho = _ops._Handover()
    ho.leave_sums(sums, gx)
    assert ho.sums_left()
    assert ho.take_sums(gx, gx.shape) is sums
    assert not ho.sums_left() and ho.take_sums(gx, gx.shape) is None          # consumed once

    ho.leave_sums(sums, gx)
    gx.add_(1.0)                                                               # in-place edit: version bump
    assert ho.take_sums(gx, gx.shape) is None
    ho.leave_sums(sums, gx)
    assert ho.take_sums(gx.clone(), gx.shape) is None                          # another tensor
    assert ho.take_sums(gx, gx.shape) is None                                  # ... and the miss consumed the marker
    ho.leave_sums(sums, gx)
    assert ho.take_sums(gx, (1, 4, 4, 8)) is None                              # another shape
    assert ho.take_sums(gx, gx.shape) is None


def test_parked_gradients_add_up_and_are_taken_once():
    ho = _ops._Handover()
    assert ho.take_parked() is None
    a, b = torch.full((3,), 1.5), torch.full((3,), 2.0)
    ho.park(a)
    ho.park(b)
    assert torch.equal(ho.take_parked(), a + b)
    assert ho.take_parked() is None
    assert torch.equal(a, torch.full((3,), 1.5))                               # the first gradient itself is not written


def test_take_act_done():
    ho = _ops._Handover()
    gx = torch.zeros(2, 4, 4, 8)
    assert ho.take_act_done(gx, gx.shape, True) is False                      # no marker
    ho.leave_act_done(gx)
    assert ho.take_act_done(gx, gx.shape, True) is True
    assert ho.take_act_done(gx, gx.shape, True) is False                      # consumed once
    for arrived, shape, plain_act in ((gx.clone(), gx.shape, True), (gx, (1, 4, 4, 8), True), (gx, gx.shape, False)):
        ho.leave_act_done(gx)
        with pytest.raises(_lib.P2PHDError, match="already applied this block's activation derivative, but the gradient that "
                                                  "arrived is not the tensor it wrote"):
            ho.take_act_done(arrived, shape, plain_act)
        assert ho.take_act_done(gx, gx.shape, True) is False                  # ... and the raise consumed the marker
    ho.leave_act_done(gx)
    gx.mul_(2.0)
    with pytest.raises(_lib.P2PHDError, match="rerun with P2PHD_BSUM=0"):
        ho.take_act_done(gx, gx.shape, True)


def test_consumers_are_counted_on_the_producer():
    class Producer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            ctx.ho = _ops._Handover()
            return x * 2

        @staticmethod
        def backward(ctx, g):
            return g * 2

    out = Producer.apply(torch.ones(4, requires_grad=True))
    assert _ops._note_consumer(out) is out.grad_fn and _ops._note_consumer(out) is out.grad_fn
    assert out.grad_fn.ho.consumers == 2
    plain = torch.ones(4, requires_grad=True) * 2                              # not a conv block: nothing to count
    assert _ops._note_consumer(plain) is plain.grad_fn and _ops._note_consumer(torch.ones(4)) is None
