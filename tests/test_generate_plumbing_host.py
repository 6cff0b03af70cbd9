"""The plumbing of whole-file generation without a GPU, on a stub in the style of the other host tests: the two entry points take
the same options with the same defaults in the same order, and with everything on that a stub can carry the result's keys, a folder
record's keys and the keywords the output stage receives are exactly these, in this order -- for an enhanced file and for one that
does not parse."""
import inspect
from types import SimpleNamespace

import pytest
import torch

SUMS = [4.0, 4.0, 3.28, 0.1, 1.0, 1.0, 0.80, 0.0]                  # one clip's eight stereo sums
OUTPUT = {'peak': [1.7, 1.7], 'peak_dbfs': [4.6, 4.6], 'clipped': [3, 3], 'nonfinite': [0, 0], 'gain': 0.5}


def test_the_two_entry_points_take_the_same_options():
    from pix2pixhdaudiosr_amd.generate import SuperResolver
    one = list(inspect.signature(SuperResolver.enhance_file).parameters.values())
    many = list(inspect.signature(SuperResolver.enhance_folder).parameters.values())
    assert [p.name for p in one[:3]] == ['self', 'path_in', 'path_out'] and [p.name for p in many[:3]] == ['self', 'dir_in', 'dir_out']
    assert one[2].default is None and many[2].default is inspect.Parameter.empty
    shared = one[3:]
    names = [p.name for p in shared]
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in one + many)
    in_folder = [p for p in many[3:] if p.name in names]
    assert [p.name for p in in_folder] == names                   # every one of them, in the same relative order
    assert [p.default for p in in_folder] == [p.default for p in shared]
    assert [p.name for p in many[3:] if p.name not in names] == ['seed', 'report', 'album_cache_bytes', 'input_formats']


def _stub_resolver():
    """SuperResolver with every device step replaced; the measurements 'return' fixed figures and the output stage records what
    it is given."""
    from pix2pixhdaudiosr_amd.generate import SuperResolver

    class Stub(SuperResolver):
        def __init__(self):
            self.opt = SimpleNamespace(lr_sampling_rate=8000, hr_sampling_rate=48000)
            self.device = torch.device("cpu")
            self.calls = []

        def _read(self, path, slot='in0'):
            from pix2pixhdaudiosr_amd.data import wavio
            self.calls.append(('read', path))
            return torch.zeros(0, dtype=torch.uint8), wavio.info(path), slot

        def _decode(self, host, meta, slot):
            return torch.linspace(-1, 1, meta.num_frames)[None].repeat(meta.num_channels, 1)

        def enhance_lr(self, lr_audio, noise=None):
            return 1.7 * lr_audio

        def _measure_bandwidth(self, bw, lr, sr, hr):
            n = 2 if hr is None else 3
            res = torch.tensor([[k, k // bw['band_bins'], 1.0, 1e-6] for k in (146, 989, 170)[:n]], dtype=torch.float64)
            return {'packed': res.reshape(-1).view(torch.uint8), 'clips': n, 'frames': 5}

        def _measure_stereo(self, st, lr, sr, hr):
            n = 2 if hr is None else 3
            return {'packed': torch.tensor([SUMS] * n, dtype=torch.float64).reshape(-1).view(torch.uint8), 'clips': n, 'frames': 5}

        def _write(self, path_out, sr, encoding, stage=None, **extra):
            self.calls.append(('write', path_out, encoding, stage, extra))
            return None if stage is None else dict(OUTPUT)
    return Stub()


@pytest.fixture
def stub(tmp_path, monkeypatch):
    from pix2pixhdaudiosr_amd.data import audio_dataset, wavio
    monkeypatch.setattr(audio_dataset, "lr_round_trip", lambda raw, *a, **k: raw)
    src = tmp_path / "in"
    src.mkdir()
    wavio.save(str(src / "a.wav"), torch.zeros(2, 64), 16000)
    (src / "b.wav").write_bytes(b"RIFF not a wav file at all")
    return _stub_resolver(), src


EVERYTHING = dict(is_lr_input=True, channels='all', clip='guard', ceiling_dbfs=-1.0, true_peak=True, limiter=True, bandwidth=True, stereo_report=True)
RESULT_KEYS = ['sr', 'lr', 'hr', 'metrics', 'info', 'bandwidth', 'stereo', 'output']
RECORD_KEYS = ['path', 'rate', 'channels', 'frames', 'written_channels', 'out_frames', 'metrics', 'error', 'output', 'bandwidth', 'stereo']
WRITE_KEYS = ['bandwidth', 'limiter', 'stereo', 'true_peak']


def _check_write(call, path_out):
    from pix2pixhdaudiosr_amd.generate import encoding_limit
    what, path, encoding, stage, extra = call
    ceiling = 10.0 ** (-1.0 / 20.0)
    assert (what, path, encoding) == ('write', path_out, 'pcm16')
    assert stage['clip'] == 'guard' and stage['ceiling'] == ceiling
    assert sorted(extra) == WRITE_KEYS
    assert extra['true_peak'] == {'rate': 48000, 'ceiling': ceiling, 'limit': encoding_limit('pcm16')}
    assert sorted(extra['limiter']) == ['ceiling', 'hold', 'lookahead', 'rate'] and extra['limiter']['ceiling'] == ceiling
    assert extra['bandwidth']['clips'] == 2 and extra['stereo']['clips'] == 2
    return extra


def test_everything_on_in_one_file(stub, tmp_path):
    sr, src = stub
    out = str(tmp_path / "o.wav")
    res = sr.enhance_file(str(src / "a.wav"), out, **EVERYTHING)
    assert list(res) == RESULT_KEYS
    assert [c[0] for c in sr.calls] == ['read', 'write']
    first = _check_write(sr.calls[-1], out)
    assert res['output'] == OUTPUT and res['hr'] is None and res['metrics'] is None and torch.equal(res['sr'], 1.7 * res['lr'])
    assert res['bandwidth']['input'] == 146 * 48000.0 / 2048 and res['bandwidth']['output'] == 989 * 48000.0 / 2048
    assert res['stereo']['mode'] == 'lr' and res['stereo']['original'] is None and res['stereo']['frames'] == 5
    # the true-peak and the limiter option are one file's: the next file gets dicts of its own
    sr.enhance_file(str(src / "a.wav"), out, **EVERYTHING)
    second = _check_write(sr.calls[-1], out)
    assert second['true_peak'] is not first['true_peak'] and second['limiter'] is not first['limiter']


def test_everything_on_in_a_folder_with_a_file_that_does_not_parse(stub, tmp_path):
    sr, src = stub
    seen = []
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), report=seen.append, **EVERYTHING)
    assert seen == recs and [r['path'] for r in recs] == ['a.wav', 'b.wav']
    assert [list(r) for r in recs] == [RECORD_KEYS] * 2
    good, bad = recs
    assert [c[0] for c in sr.calls] == ['read', 'write', 'read']    # the second file is opened and nothing else
    _check_write(sr.calls[1], str(tmp_path / "out" / "a.wav"))
    assert good['error'] is None and (good['rate'], good['channels'], good['frames'], good['written_channels'], good['out_frames']) == (16000, 2, 64, 2, 64)
    assert good['output'] == OUTPUT and good['metrics'] is None and good['bandwidth']['frames'] == 5 and good['stereo']['frames'] == 5
    assert bad['error'] is not None and bad['error'].startswith(('ValueError: ', 'EOFError: ', 'error: '))
    assert {k: v for k, v in bad.items() if k not in ('path', 'error')} == \
        {'rate': None, 'channels': None, 'frames': None, 'written_channels': 0, 'out_frames': 0, 'metrics': None, 'output': None,
         'bandwidth': None, 'stereo': None}
