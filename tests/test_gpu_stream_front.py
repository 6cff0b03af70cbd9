"""The front of a streamed window on the GPU (generate/stream.py: _stream_front): on float noise, the low-rate round trip run on the
plan's windows with their halo (plans.stream_plan) and cut as the plan says is bit for bit the whole-file lr_round_trip on the range
the window's segments are gathered from -- for the three rate chains, windows of one segment and of several."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.mark.parametrize("W", [1e-6, 0.1])
@pytest.mark.parametrize("in_rate,is_lr,frames", [(48000, False, 20011), (44100, False, 18011), (8000, True, 3001)])
def test_windows_are_the_whole_round_trip(in_rate, is_lr, frames, W):
    from pix2pixhdaudiosr_amd.data.audio_dataset import lr_round_trip
    from pix2pixhdaudiosr_amd.generate import SuperResolver, stream_plan
    T, overlap, C = 992, 0.25, 2
    x = torch.randn((C, frames), generator=torch.Generator().manual_seed(frames)).to(DEV)
    whole = lr_round_trip(x, in_rate, 8000, 48000, is_lr)
    if not is_lr and in_rate == 48000:
        whole = whole[..., :frames]
    plan = stream_plan(frames, in_rate, 8000, 48000, is_lr, T, overlap, C, 1, W)
    assert plan['L'] == whole.shape[-1] and len(plan['windows']) == -(-plan['S'] // plan['K'])
    assert plan['K'] == (1 if W == 1e-6 else 6) and len(plan['windows']) > 2
    sr = SuperResolver.__new__(SuperResolver)
    for w in plan['windows']:
        f0, f1 = w['read']
        sr._decode = lambda host, meta, slot: x[:, f0:f1]
        got = sr._stream_front(None, None, None, C, plan, w)
        a, b = w['need']
        assert tuple(got.shape) == (C, b - a)
        assert torch.equal(got.contiguous().view(torch.int32), whole[:, a:b].contiguous().view(torch.int32)), (in_rate, W, w)
    torch.cuda.synchronize()
