"""enhance_file(loudness_range=True) / enhance_folder / --loudness_range on the GPU: the three kernels in a row on a Tech 3342
sequence of sines; the result's 'range' against the restatement of tests/_loudness_range_ref.py on the returned clip; without the
option every key, line, column and launch is the parent's; folders, two runs, the command line.  The tiny model, the resolver
(crossover='input') and the short files are those of tests/test_gpu_generate_loudness.py; a clip of 3.6 s with a level step joins
them, since the short ones have no 3 s block."""
import csv
import math
import os
import re

import numpy as np
import pytest
import torch

import _loudness_range_ref as RR
import _loudness_ref as R
from test_gpu_generate_loudness import KEYS, RATE, _bytes, _clip, _count, _excerpt, _opt, files, resolver  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

RANGE_KEYS = ['blocks', 'high', 'input', 'low', 'output', 'short_term_max', 'threshold']
TOL = 1e-6                                                         # LU: the hop kernel's own 1e-8 bound on energies, with room


def _same(got, want, tol=TOL):
    if math.isinf(want) or math.isinf(got):
        return got == want
    return abs(got - want) <= tol


def _ref_range(rows, gain=None):
    from pix2pixhdaudiosr_amd.generate import loudness_channel_weights
    rows = rows.cpu().numpy()
    return RR.measure(R.hop_energies(rows, RATE), RATE, loudness_channel_weights(rows.shape[0]), gain)


@pytest.fixture(scope="module")
def long_file(tmp_path_factory):
    """3.6 s, 36 hops, 7 short-term blocks: the stored excerpt eight times over, its first 3 s 20 dB down -- block b holds b loud
    hops, so the blocks lie some 12 dB apart."""
    from pix2pixhdaudiosr_amd.data import wavio
    x = _excerpt()
    x = torch.cat([x, 0.7 * x.flip(0)] * 4)[:36 * (RATE // 10) + 321]
    x[:30 * (RATE // 10)] *= 0.1
    path = str(tmp_path_factory.mktemp("loudness_range_in") / "long.wav")
    wavio.save(path, 0.5 * x, RATE)
    return path


def test_three_kernels_on_a_tech_3342_sequence():
    """A 1 kHz sine at 8 kHz, mono, 20 s at -20 dBFS and 20 s at -30 dBFS: 10 LU within the standard's 1 LU, and the restatement's
    figure on the same hop energies."""
    from pix2pixhdaudiosr_amd.generate import loudness_hops, loudness_range, loudness_short_term
    rate = 8000
    t = np.arange(40 * rate) / rate
    x = np.sin(2.0 * np.pi * 1000.0 * t) * np.where(t < 20.0, 10.0 ** (-20.0 / 20.0), 10.0 ** (-30.0 / 20.0))
    xt = torch.from_numpy(x.astype(np.float32)[None]).to("cuda:0")
    _count(reset=True)
    z = loudness_hops(xt, rate)
    res8 = loudness_range(loudness_short_term(z, rate)).cpu().numpy()
    assert _count() == 3
    want = RR.measure(z.cpu().numpy(), rate)
    print("LRA %.9f LU (restatement %.9f), %.4f .. %.4f LUFS, n %d, short-term max %.4f" % (res8[0], want['lra'], res8[1], res8[2], res8[4], res8[5]))
    assert abs(res8[0] - 10.0) <= 1.0
    assert abs(res8[0] - want['lra']) <= TOL and res8[4] == want['n'] == 371 and _same(res8[5], want['short_term_max'])


def test_report_with_the_range(resolver, files, long_file, tmp_path):
    resolver.enhance_file(str(files / "mono.wav"), None)          # capture, tables, packed weights
    torch.manual_seed(5)
    plain = resolver.enhance_file(long_file, str(tmp_path / "plain.wav"), encoding='float32', loudness='report')
    assert sorted(plain['loudness']) == KEYS
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(long_file, str(tmp_path / "on.wav"), encoding='float32', loudness='report', loudness_range=True)
    assert _count() == 8                                           # two hop, two gate, two short-term and two range launches
    info = res['loudness']
    assert sorted(info) == sorted(KEYS + ['range']) and sorted(info['range']) == RANGE_KEYS
    assert {k: v for k, v in info.items() if k != 'range'} == plain['loudness']                   # the other figures: as without it
    assert _bytes(str(tmp_path / "on.wav")) == _bytes(str(tmp_path / "plain.wav")) and torch.equal(res['sr'], plain['sr'])
    rng = info['range']
    want_out, want_in = _ref_range(res['sr']), _ref_range(res['lr'])
    print("result %r\nrestatement out %r\nrestatement in %r" % (rng, want_out, want_in))
    assert want_out['n'] == 7 and want_out['lra'] > 3.0            # (the test would show nothing on a clip without dynamics)
    assert _same(rng['output'], want_out['lra']) and _same(rng['input'], want_in['lra'])
    assert _same(rng['low'], want_out['low']) and _same(rng['high'], want_out['high']) and _same(rng['threshold'], want_out['threshold'])
    assert rng['blocks'] == want_out['n'] and isinstance(rng['blocks'], int) and _same(rng['short_term_max'], want_out['short_term_max'])
    assert rng['low'] <= rng['high'] <= rng['short_term_max']
    # twice: the same figures
    torch.manual_seed(5)
    again = resolver.enhance_file(long_file, None, loudness='report', loudness_range=True)
    assert again['loudness'] == info


def test_the_figures_are_those_of_the_clip_behind_the_gain(resolver, long_file):
    """With a target the powers take the gate's gain from device memory: the levels move with the clip, the range stays."""
    torch.manual_seed(5)
    rep = resolver.enhance_file(long_file, None, loudness='report', loudness_range=True)
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(long_file, None, loudness=-23.0, loudness_range=True)
    assert _count() == 8
    info, rng = res['loudness'], res['loudness']['range']
    assert abs(info['gain_db']) > 0.5
    want = _ref_range(rep['sr'], np.float32(10.0 ** (info['gain_db'] / 20.0)))
    print("gain %+.4f dB: %r; restatement %r" % (info['gain_db'], rng, want))
    for key, name in (('output', 'lra'), ('low', 'low'), ('high', 'high'), ('threshold', 'threshold'), ('short_term_max', 'short_term_max')):
        assert _same(rng[key], want[name]), key
    assert rng['blocks'] == want['n'] and rng['input'] == rep['loudness']['range']['input']
    assert _same(rng['output'], rep['loudness']['range']['output']) and _same(rng['high'], rep['loudness']['range']['high'] + info['gain_db'])


def test_a_clip_under_three_seconds(resolver, files):
    ninf = float('-inf')
    _count(reset=True)
    res = resolver.enhance_file(str(files / "mono.wav"), None, loudness='report', loudness_range=True)
    assert _count() == 6                                           # no block: the short-term kernel is not launched
    assert res['loudness']['range'] == {'input': 0.0, 'output': 0.0, 'low': ninf, 'high': ninf, 'threshold': ninf, 'blocks': 0,
                                        'short_term_max': ninf}


def test_option_off_is_the_parent(resolver, files, long_file, tmp_path):
    torch.manual_seed(5)
    _count(reset=True)
    res = resolver.enhance_file(long_file, str(tmp_path / "off.wav"), encoding='float32', loudness='report', loudness_range=False)
    assert _count() == 4 and sorted(res['loudness']) == KEYS and sorted(res) == ['hr', 'info', 'loudness', 'lr', 'metrics', 'sr']
    with pytest.raises(ValueError, match="loudness_range is an option of loudness"):
        resolver.enhance_file(long_file, str(tmp_path / "never.wav"), loudness_range=True)
    with pytest.raises(ValueError, match="loudness_range is an option of loudness"):
        resolver.enhance_folder(str(files), str(tmp_path / "never"), loudness_range=True)
    assert not os.path.exists(str(tmp_path / "never.wav")) and not os.path.exists(str(tmp_path / "never"))


def test_folder_and_file_agree(resolver, files, long_file, tmp_path):
    from pix2pixhdaudiosr_amd.generate import (METRICS_COLUMNS, METRICS_COLUMNS_LOUDNESS, METRICS_COLUMNS_LOUDNESS_RANGE, write_metrics_csv)
    src = tmp_path / "in"
    src.mkdir()
    (src / "long.wav").write_bytes(_bytes(long_file))
    (src / "stereo.wav").write_bytes(_bytes(str(files / "stereo.wav")))
    _count(reset=True)
    recs = resolver.enhance_folder(str(src), str(tmp_path / "on"), channels='all', seed=11, encoding='float32', loudness='input', loudness_range=True)
    assert _count() == 8 + 6                                       # the stereo file is under 3 s
    by = {r['path']: r for r in recs}
    for name in ("long.wav", "stereo.wav"):
        torch.manual_seed(11)
        one = resolver.enhance_file(str(src / name), str(tmp_path / ("one_" + name)), channels='all', encoding='float32', loudness='input',
                                    loudness_range=True)
        assert by[name]['loudness'] == one['loudness'] and sorted(one['loudness']['range']) == RANGE_KEYS
        assert _bytes(str(tmp_path / "on" / name)) == _bytes(str(tmp_path / ("one_" + name)))
    assert by["long.wav"]['loudness']['range']['blocks'] == 7 and by["stereo.wav"]['loudness']['range']['blocks'] == 0
    write_metrics_csv(str(tmp_path / "on.csv"), recs, False, False, True, loudness_range=True)
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == METRICS_COLUMNS + METRICS_COLUMNS_LOUDNESS + METRICS_COLUMNS_LOUDNESS_RANGE and len(rows) == 1 + 3 + 1
    for row in rows[1:-1]:
        r = by[row[0]]['loudness']['range']
        assert [float(v) for v in row[-3:]] == [r['input'], r['output'], r['short_term_max']]


def test_cli_lines_and_csv_columns(files, long_file, tmp_path, capsys):
    """Without --loudness_range main() prints the lines and writes the columns of the parent; with it one `loudness range` line
    more per file, behind the loudness line, and three columns more, holding what enhance_file returns."""
    from pix2pixhdaudiosr_amd import generate as G
    from pix2pixhdaudiosr_amd.models.models import create_model
    common = dict(mdct_type="mdct4", checkpoints_dir=str(tmp_path), name="run", seed=1234)
    torch.manual_seed(1234)
    create_model(_opt(**common)).save('latest')
    folder = tmp_path / "run"
    with open(folder / "opt.txt", "w") as f:                       # the dump of options/base_options.py:102-107
        f.write('------------ Options -------------\n')
        for k, v in sorted(vars(_opt(**common)).items()):
            f.write('%s: %s\n' % (str(k), str(v)))
        f.write('-------------- End ----------------\n')
    base = ["--input", long_file, "--load_pretrain", str(folder), "--encoding", "float32", "--crossover", "input", "--loudness", "report"]
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "off.wav"), "--metrics_csv", str(tmp_path / "off.csv")]) == 0
    assert _count() == 4
    off = capsys.readouterr().out.splitlines()
    assert sum(": loudness " in l for l in off) == 1 and not any("loudness range" in l for l in off)
    assert open(str(tmp_path / "off.csv")).readline().strip() == ",".join(G.METRICS_COLUMNS + G.METRICS_COLUMNS_LOUDNESS)
    _count(reset=True)
    assert G.main(base + ["--output", str(tmp_path / "on.wav"), "--metrics_csv", str(tmp_path / "on.csv"), "--loudness_range"]) == 0
    assert _count() == 8
    on = capsys.readouterr().out.splitlines()
    extra = [l for l in on if ": loudness range " in l]
    assert len(extra) == 1 and [l.replace("on.wav", "off.wav").replace("on.csv", "off.csv") for l in on if l not in extra] == off
    level = r"([-+]\d+\.\d\d|-inf)"
    m = re.fullmatch(re.escape(str(tmp_path / "on.wav")) + r": loudness range input (\d+\.\d\d) LU, output (\d+\.\d\d) LU \(%s \.\. %s LUFS\), "
                     r"short-term max %s LUFS" % (level, level, level), extra[0])
    assert m, extra[0]
    assert ": loudness input " in on[on.index(extra[0]) - 1]      # behind its file's loudness line
    rows = list(csv.reader(open(str(tmp_path / "on.csv"))))
    assert tuple(rows[0]) == G.METRICS_COLUMNS + G.METRICS_COLUMNS_LOUDNESS + G.METRICS_COLUMNS_LOUDNESS_RANGE and len(rows) == 3
    assert ["%.2f" % float(rows[1][-3]), "%.2f" % float(rows[1][-2]), "%+.2f" % float(rows[1][-1])] == [m.group(1), m.group(2), m.group(5)]
    assert float(m.group(2)) > 3.0 and rows[1][:10] == list(csv.reader(open(str(tmp_path / "off.csv"))))[1][:10] and rows[2][-3:] == rows[1][-3:]
    assert _bytes(str(tmp_path / "on.wav")) == _bytes(str(tmp_path / "off.wav"))
    # folder mode: one line per file; a file under 3 s prints 0.00 LU and -inf
    assert G.main(["--input", str(files), "--output", str(tmp_path / "dir"), "--load_pretrain", str(folder), "--channels", "all",
                   "--crossover", "input", "--loudness", "report", "--loudness_range"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if ": loudness range " in l]
    assert len(lines) == 2 and all(l.endswith("loudness range input 0.00 LU, output 0.00 LU (-inf .. -inf LUFS), short-term max -inf LUFS")
                                   for l in lines)
    # an option of --loudness: the parser's error, before anything is loaded
    with pytest.raises(SystemExit):
        G.main(["--input", long_file, "--output", str(tmp_path / "no.wav"), "--load_pretrain", str(folder), "--loudness_range"])
    assert "--loudness_range is an option of --loudness" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "no.wav"))
