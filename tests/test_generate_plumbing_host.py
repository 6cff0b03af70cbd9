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


# ------------------------------------------------------------------------------------------
# the remaining options: key orders, the channel-count refusals, the printed lines.  Every expected list, text and line below is a
# literal taken from a run on the commit before resolver.py was split into rows.py, fileio.py and resolver.py.
# ------------------------------------------------------------------------------------------
LOUDNESS = {'input': -30.0, 'measured': -20.0, 'gain_db': -3.0, 'output': -23.0, 'momentary_max': -18.5, 'target': -23.0}
RANGE = {'input': 4.0, 'output': 5.5, 'low': -30.25, 'high': -24.75, 'threshold': -43.0, 'blocks': 17, 'short_term_max': -21.5}
SPEECH = {'input': -31.0, 'measured': -27.5, 'gain_db': -3.5, 'output': -31.0, 'target': -31.0, 'long_term': -33.0, 'activity': 0.625,
          'activity_input': 0.5, 'channels': [{'active': -31.0, 'long_term': -33.0, 'activity': 0.625}] * 2}
FLAC = {'block': 4096, 'frames': 1, 'bytes': 120, 'pcm_bytes': 256, 'md5': '00ff', 'lpc': 8}
LIMITER = {'lookahead': 240, 'hold': 960, 'max_reduction_db': -1.25, 'limited_samples': 16, 'input_true_peak_dbtp': 4.75}
CROSSOVER = {'hz': 3230.0, 'taps': 255, 'edge_hz': 3400.0}


def _report_stub(**attrs):
    """The stub above with the loudness, the speech-level and the picture stage replaced as well; `attrs`: what the constructor's
    options would have left on the object."""
    class Reports(type(_stub_resolver())):
        def _measure_loudness(self, loud, lr, sr):
            return {'packed': torch.zeros(8, dtype=torch.uint8), 'gain': torch.tensor(0.5)}

        @staticmethod
        def _loudness_result(loud, measure):
            return dict(LOUDNESS, **({'range': dict(RANGE)} if loud.get('range') else {}))

        def _measure_speech_level(self, sl, lr, sr):
            return {'packed': torch.zeros(8, dtype=torch.uint8), 'gain': torch.tensor(0.5), 'channels': (lr.shape[0], sr.shape[0])}

        @staticmethod
        def _speech_level_result(sl, measure):
            return dict(SPEECH)

        @staticmethod
        def _render_picture(spec, lr, sr, hr):
            return {'image': torch.zeros((4, 4, 3), dtype=torch.uint8), 'top': torch.zeros(1), 'panels': 2, 'frames': 5, 'bins': 513}

        @staticmethod
        def _save_picture(spec, picture):
            return {'path': spec['path'], 'panels': picture['panels'], 'frames': picture['frames'], 'bins': picture['bins'], 'top_db': -3.0,
                    'range_db': spec['plan']['range_db']}

        def _write(self, path_out, sr, encoding, stage=None, **extra):
            output = super()._write(path_out, sr, encoding, stage, **extra)
            if 'flac' in extra:
                extra['flac']['result'] = dict(FLAC)
            if 'true_peak' in extra:
                output['true_peak_dbtp'] = [5.0, 5.0]
            if 'limiter' in extra:
                output['limiter'] = dict(LIMITER)
            return output
    sr = Reports()
    for name, value in attrs.items():
        setattr(sr, name, value)
    return sr


@pytest.fixture
def no_converter(monkeypatch):
    from pix2pixhdaudiosr_amd.generate import resolver
    monkeypatch.setattr(resolver, "rate_convert", lambda clip, rate_in, rate_out, plan: clip[..., ::2])


COMBINATIONS = {
    'loudness': (dict(norm_scope='clip', last_norm=torch.zeros(2, 2), crossover_auto=True, last_crossover=CROSSOVER),
                 dict(is_lr_input=True, channels='all', loudness=-23.0, loudness_range=True, spectrogram='pictures', extended_metrics=True,
                      container='flac', flac_md5=True, flac_lpc=8, bandwidth=True, stereo_report=True, report_peaks=True)),
    'speech': (dict(segment_norm=True, last_norm=torch.zeros(2, 1, 2)),
               dict(is_lr_input=True, channels='all', speech_level='input', output_rate=44100, container='flac', clip='guard', true_peak=True,
                    limiter=True)),
    'plain': (dict(), dict(is_lr_input=True)),
}
BASE_RESULT = ['sr', 'lr', 'hr', 'metrics', 'info']
BASE_RECORD = ['path', 'rate', 'channels', 'frames', 'written_channels', 'out_frames', 'metrics', 'error']
EXPECTED = {
    'loudness': (BASE_RESULT + ['norm', 'spectrogram', 'loudness', 'bandwidth', 'crossover', 'stereo', 'metrics_ext', 'output', 'flac'],
                 BASE_RECORD + ['written', 'metrics_ext', 'output', 'spectrogram', 'loudness', 'bandwidth', 'crossover', 'stereo', 'norm', 'flac'],
                 ['bandwidth', 'flac', 'loudness', 'picture', 'stereo']),
    'speech': (BASE_RESULT + ['norm', 'speech_level', 'output_rate', 'output', 'flac'],
               BASE_RECORD + ['written', 'output', 'speech_level', 'output_rate', 'norm', 'flac'],
               ['flac', 'limiter', 'rate', 'speech_level', 'true_peak']),
    'plain': (BASE_RESULT, BASE_RECORD, []),
}


@pytest.mark.parametrize("name", sorted(COMBINATIONS))
def test_key_orders_with_the_remaining_options(name, stub, no_converter, tmp_path):
    _, src = stub
    attrs, kw = COMBINATIONS[name]
    result_keys, record_keys, write_keys = EXPECTED[name]
    sr = _report_stub(**attrs)
    one = dict(kw, **({'spectrogram': str(tmp_path / "p.png")} if 'spectrogram' in kw else {}))
    res = sr.enhance_file(str(src / "a.wav"), str(tmp_path / "o.wav"), **one)
    assert list(res) == result_keys
    assert sorted(sr.calls[-1][4]) == write_keys
    many = dict(kw, **({'spectrogram': str(tmp_path / "pictures")} if 'spectrogram' in kw else {}))
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), **many)
    assert [list(r) for r in recs] == [record_keys] * 2
    assert [c[0] for c in sr.calls] == ['read', 'write', 'read', 'write', 'read']
    assert sorted(sr.calls[3][4]) == write_keys
    good, bad = recs
    assert good['error'] is None and bad['error'] is not None
    assert all(bad[k] is None for k in record_keys[8:] if k != 'written')
    for key in record_keys[8:]:
        if key != 'written':
            assert (good[key] is None) == (res[key] is None), key
    if name == 'loudness':
        assert res['loudness'] == dict(LOUDNESS, range=RANGE) and res['crossover'] == CROSSOVER and res['flac'] == FLAC
        assert res['metrics_ext'] is None and good['metrics_ext'] is None          # (no original: the key is there, its value None)
        assert res['spectrogram']['path'] == str(tmp_path / "p.png") and good['spectrogram']['path'] == str(tmp_path / "pictures" / "a.wav.png")
        assert res['norm'] is sr.last_norm and torch.equal(res['sr'], 0.5 * 1.7 * res['lr'])
    if name == 'speech':
        assert res['speech_level'] == SPEECH and res['output_rate']['rate'] == 44100 and res['output_rate']['model_rate'] == 48000
        assert sr.calls[-2][4]['rate'] == 44100 and good['out_frames'] == 32 and good['written'] == 'a.flac'
        assert torch.equal(res['sr'], 0.5 * 1.7 * res['lr'][..., ::2])


def _wav(folder, name, channels):
    from pix2pixhdaudiosr_amd.data import wavio
    path = folder / name
    wavio.save(str(path), torch.zeros(channels, 16), 16000)
    return str(path)


# (the object's attributes, the options, the channels of the file) -> the refusal; where two apply, the one that comes first
REFUSALS = [
    (dict(), dict(spectrogram='p', spectrogram_channel=1), 2, "spectrogram_channel 1: the file has 2 channels and channels='first' writes 1"),
    (dict(stereo='ms'), dict(channels='all'), 3, "stereo='ms' takes one or two channels, 3 would be written"),
    (dict(), dict(channels='all', container='flac'), 9, "a FLAC stream holds at most 8 channels, 9 would be written"),
    (dict(), dict(channels='all', speech_level='report'), 9, "the active speech level is measured over at most 8 channels, 9 would be written"),
    (dict(stereo='ms'), dict(channels='all', spectrogram='p', spectrogram_channel=9, container='flac', speech_level='report'), 9,
     "spectrogram_channel 9: the file has 9 channels and channels='all' writes 9"),
    (dict(stereo='ms'), dict(channels='all', container='flac', speech_level='report'), 9, "stereo='ms' takes one or two channels, 9 would be written"),
    (dict(), dict(channels='all', container='flac', speech_level='report'), 9, "a FLAC stream holds at most 8 channels, 9 would be written"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_channel_count_refusals(case, stub, tmp_path):
    attrs, kw, channels, text = REFUSALS[case]
    src = tmp_path / "wide"
    src.mkdir()
    path = _wav(src, "w.wav", channels)
    sr = _report_stub(**attrs)
    one = dict(kw, **({'spectrogram': str(tmp_path / "p.png")} if 'spectrogram' in kw else {}))
    with pytest.raises(ValueError) as e:
        sr.enhance_file(path, str(tmp_path / "o.wav"), is_lr_input=True, **one)
    assert str(e.value) == text
    many = dict(kw, **({'spectrogram': str(tmp_path / "pictures")} if 'spectrogram' in kw else {}))
    recs = sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, **many)
    assert [r['error'] for r in recs] == ['ValueError: ' + text]
    assert not any(c[0] == 'write' for c in sr.calls) and recs[0]['written_channels'] == 0


def test_the_loudness_channel_limit_ends_a_folder(stub, tmp_path):
    src = tmp_path / "wide"
    src.mkdir()
    path = _wav(src, "w.wav", 65)
    sr = _report_stub()
    text = "loudness is measured over at most 64 channels, 65 would be written"
    with pytest.raises(ValueError) as e:
        sr.enhance_file(path, str(tmp_path / "o.wav"), is_lr_input=True, channels='all', loudness='report')
    assert str(e.value) == text
    with pytest.raises(ValueError) as e:                           # not a skipped file: the run ends
        sr.enhance_folder(str(src), str(tmp_path / "out"), is_lr_input=True, channels='all', loudness='report')
    assert str(e.value) == text
    # it stands behind the FLAC limit and in front of nothing a folder skips a file for
    with pytest.raises(ValueError) as e:
        sr.enhance_file(path, str(tmp_path / "o.flac"), is_lr_input=True, channels='all', loudness='report', container='flac')
    assert str(e.value) == "a FLAC stream holds at most 8 channels, 65 would be written"


CLI = {
    'loudness': ["--channels", "all", "--loudness", "-23", "--loudness_range", "--metrics_ext", "--container", "flac", "--flac_md5", "--flac_lpc", "8",
                 "--bandwidth", "--stereo_report", "--report_peaks"],
    'speech': ["--channels", "all", "--speech_level", "input", "--output_rate", "44100", "--container", "flac", "--clip", "guard", "--true_peak",
               "--limiter"],
}


NOTE = "note: the input's band ends at 3.42 kHz, under the low rate's Nyquist frequency 4.00 kHz: the generator was trained on inputs that reach it"
LINES = {                                                          # (a single file, a folder); TMP: the test's folder
    'loudness': (['wrote TMP/o.flac (64 samples at 48000 Hz, 2 channels)',
                  'TMP/o.flac: FLAC 16 bit, 1 frames of 4096, 120 bytes (46.9 % of the PCM), MD5 00ff, LPC up to order 8',
                  'TMP/o.flac: peak +4.60 +4.60 dBFS, 6 clipped, 0 non-finite, gain 0.500000',
                  'spectrogram: TMP/p.png (2 panels, 5 frames x 513 bins, 90.0 dB down from -3.0 dB)',
                  'TMP/o.flac: loudness input -30.00 LUFS, output -23.00 LUFS, gain -3.00 dB',
                  'TMP/o.flac: loudness range input 4.00 LU, output 5.50 LU (-30.25 .. -24.75 LUFS), short-term max -21.50 LUFS',
                  'crossover: 3.23 kHz, 255 taps (input band ends at 3.40 kHz)',
                  "TMP/o.flac: bandwidth input 3.42 kHz, output 23.18 kHz (-60 dB, low rate's Nyquist 4.00 kHz)",
                  'TMP/o.flac: ' + NOTE,
                  'TMP/o.flac: stereo correlation below / above 4.01 kHz: input +0.82 / +0.80, output +0.82 / +0.80',
                  'metrics: TMP/m.csv'],
                 ['wrote TMP/outdir/a.flac (64 samples at 48000 Hz, 2 channels)',
                  'TMP/outdir/a.flac: FLAC 16 bit, 1 frames of 4096, 120 bytes (46.9 % of the PCM), MD5 00ff, LPC up to order 8',
                  'a.wav: peak +4.60 +4.60 dBFS, 6 clipped, 0 non-finite, gain 0.500000',
                  'spectrogram: TMP/pictures/a.wav.png (2 panels, 5 frames x 513 bins, 90.0 dB down from -3.0 dB)',
                  'a.wav: loudness input -30.00 LUFS, output -23.00 LUFS, gain -3.00 dB',
                  'a.wav: loudness range input 4.00 LU, output 5.50 LU (-30.25 .. -24.75 LUFS), short-term max -21.50 LUFS',
                  'crossover: 3.23 kHz, 255 taps (input band ends at 3.40 kHz)',
                  "a.wav: bandwidth input 3.42 kHz, output 23.18 kHz (-60 dB, low rate's Nyquist 4.00 kHz)",
                  'a.wav: ' + NOTE,
                  'a.wav: stereo correlation below / above 4.01 kHz: input +0.82 / +0.80, output +0.82 / +0.80',
                  'skipped b.wav: ValueError: TMP/in/b.wav: not a RIFF/WAVE file',
                  '1 of 2 files enhanced, 1 skipped',
                  'metrics: TMP/m.csv']),
    'speech': (['wrote TMP/o.flac (32 samples at 44100 Hz, 2 channels)',
                'TMP/o.flac: FLAC 16 bit, 1 frames of 4096, 120 bytes (46.9 % of the PCM), MD5 00ff, LPC up to order 8',
                'TMP/o.flac: peak +4.60 +4.60 dBFS, true peak +5.00 +5.00 dBTP, 6 clipped, 0 non-finite, gain 0.500000',
                'limiter: -1.25 dB at most, 50.0 % of the samples, true peak in +4.75 dBTP',
                'TMP/o.flac: speech level input -31.00 dBov (activity 50.0 %), measured -27.50 dBov (activity 62.5 %), gain -3.50 dB -> -31.00 dBov',
                'metrics: TMP/m.csv'],
               ['wrote TMP/outdir/a.flac (32 samples at 44100 Hz, 2 channels)',
                'TMP/outdir/a.flac: FLAC 16 bit, 1 frames of 4096, 120 bytes (46.9 % of the PCM), MD5 00ff, LPC up to order 8',
                'a.wav: peak +4.60 +4.60 dBFS, true peak +5.00 +5.00 dBTP, 6 clipped, 0 non-finite, gain 0.500000',
                'limiter: -1.25 dB at most, 50.0 % of the samples, true peak in +4.75 dBTP',
                'a.wav: speech level input -31.00 dBov (activity 50.0 %), measured -27.50 dBov (activity 62.5 %), gain -3.50 dB -> -31.00 dBov',
                'skipped b.wav: ValueError: TMP/in/b.wav: not a RIFF/WAVE file',
                '1 of 2 files enhanced, 1 skipped',
                'metrics: TMP/m.csv']),
}
COLUMNS = {
    'loudness': ['file', 'channel', 'frames', 'mse', 'snr_sr', 'snr_lr', 'lsd', 'lsd_lf', 'lsd_hf', 'ssnr_sr', 'ssnr_lr', 'peak_dbfs', 'clipped', 'gain',
                 'lufs_in', 'lufs_out', 'loudness_gain_db', 'lra_in', 'lra_out', 'short_term_max', 'bw_in', 'bw_out', 'bw_orig', 'corr_lf_out',
                 'corr_hf_out', 'corr_hf_orig', 'side_hf_out_db'],
    'speech': ['file', 'channel', 'frames', 'mse', 'snr_sr', 'snr_lr', 'lsd', 'true_peak_dbtp', 'limiter_reduction_db', 'limited_samples', 'asl_in',
               'asl_out', 'activity_out'],
}


@pytest.mark.parametrize("name", sorted(CLI))
def test_cli_prints_the_report_lines_of_the_remaining_options(name, stub, no_converter, tmp_path, capsys):
    import csv
    from pix2pixhdaudiosr_amd.generate import _parser, _run
    _, src = stub
    attrs, kw = COMBINATIONS[name]
    stage = {k: v for k, v in kw.items() if k not in ('is_lr_input', 'channels', 'extended_metrics')}
    rate = 44100 if name == 'speech' else 48000
    got = {}
    for folder_mode, inp, out in ((False, src / "a.wav", tmp_path / "o.flac"), (True, src, tmp_path / "outdir")):
        sr = _report_stub(**attrs)
        csv_path = tmp_path / "m.csv"
        picture = ["--spectrogram", str(tmp_path / ("pictures" if folder_mode else "p.png"))] if 'spectrogram' in kw else []
        a = _parser().parse_args(["--input", str(inp), "--output", str(out), "--load_pretrain", "ck", "--is_lr_input", "--metrics_csv", str(csv_path)]
                                 + CLI[name] + picture)
        mine = dict(stage, **({'spectrogram': picture[1]} if picture else {}))
        assert _run(a, sr, mine, None, rate, folder_mode) == 0
        got[folder_mode] = [l.replace(str(tmp_path), "TMP") for l in capsys.readouterr().out.splitlines()]
        with open(csv_path, newline="") as f:
            got[folder_mode, 'csv'] = next(csv.reader(f))
    assert got[False] == LINES[name][0]
    assert got[True] == LINES[name][1]
    assert got[False, 'csv'] == got[True, 'csv'] == COLUMNS[name]
