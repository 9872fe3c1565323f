"""Score-to-recording alignment on the host (reconvat_amd/align.py): the yardstick `dtw_host` against a plain double
loop, the band construction, the refusals, the end-to-end case, and align_scores.py / train_on=Scores:<folder> on device='cpu'."""
import os
import re

import numpy as np
import pytest
import torch

import align_cases as ac
from reconvat_amd import _lib, align, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = [(1, 1), (1, 7), (9, 1), (13, 11)]


@pytest.mark.parametrize('N,M', TINY)
@pytest.mark.parametrize('values', [(0, 1, 2), (4095,)])
def test_dtw_host_equals_the_double_loop(N, M, values):
    """Costs from {0, 1, 2}: ties everywhere, the tie rule decides every direction; all 4095: the largest sums."""
    rng = np.random.RandomState(N * 100 + M)
    for _ in range(4):
        cost = rng.choice(values, size=(N, M)).astype(np.uint16)
        lo = np.zeros(N, dtype=np.int32)
        res = align.dtw_host(cost, lo, M)
        ac.check_result(res, cost, lo, M, M)
        assert res['N'] == N and res['M'] == M
        if values == (4095,):                                 # every path weighs N + M: the diagonal comes first on the way back
            assert res['total'] == 4095 * (N + M) and res['length'] == max(N, M)


def test_dtw_host_banded_against_the_double_loop():
    rng = np.random.RandomState(5)
    lo, W, M = ac.jumpy_lo(), 33, 200
    cost = rng.choice([0, 1, 2], size=(len(lo), W)).astype(np.uint16)
    cost[lo[:, None] + np.arange(W)[None, :] >= M] = align.DEAD
    res = align.dtw_host(cost, lo, W)                        # M inferred from the dead cells of the last row
    assert res['M'] == M
    ac.check_result(res, cost, lo, W, M)
    assert res['total'] != align.SENTINEL


def test_banded_equals_full_when_the_band_covers_the_path():
    rng = np.random.RandomState(6)
    N, M = 40, 37
    full = rng.randint(0, 4096, size=(N, M)).astype(np.uint16)
    full[np.abs(np.arange(N)[:, None] - np.arange(M)[None, :]) > 3] = 4095      # the cheap cells hug the diagonal
    full[np.abs(np.arange(N)[:, None] - np.arange(M)[None, :]) <= 3] //= 64
    a = align.dtw_host(full, np.zeros(N, dtype=np.int32), M)
    W = 15
    lo = np.clip(np.arange(N) - 7, 0, M - W).astype(np.int32)
    assert (a['row_lo'] >= lo).all() and (a['row_hi'] < lo + W).all()            # the band holds the full matrix's path
    cols = lo[:, None] + np.arange(W)[None, :]
    band = np.where(cols < M, full[np.arange(N)[:, None], np.minimum(cols, M - 1)], align.DEAD).astype(np.uint16)
    b = align.dtw_host(band, lo, W, M)
    ac.same_result(a, b)


def test_disconnected_band_gives_the_sentinel_and_the_python_layer_raises():
    N, M, W = 6, 12, 3
    lo = np.array([0, 0, 0, 8, 8, 9], dtype=np.int32)         # row 2 ends at column 2, row 3 starts at column 8
    cost = np.ones((N, W), dtype=np.uint16)
    res = align.dtw_host(cost, lo, W, M)
    ac.check_result(res, cost, lo, W, M)
    assert res['total'] == align.SENTINEL and res['length'] == 0 and (res['col_lo'] == -1).all()
    # a last row that does not reach the last column is no path either
    res = align.dtw_host(np.ones((3, 2), dtype=np.uint16), np.zeros(3, dtype=np.int32), 2, 5)
    assert res['total'] == align.SENTINEL
    rng = np.random.RandomState(0)
    X, Y = ac.unit_rows(rng, N, 8), ac.unit_rows(rng, M, 8)
    with pytest.raises(ValueError, match=r'piece7.*wider radius'):
        align.dtw_pairs([(X, Y)], [lo], [W], 'cpu', ['piece7'])


def test_cost_host_quantises_and_marks_dead_cells():
    rng = np.random.RandomState(1)
    X, Y = ac.unit_rows(rng, 5, 7), ac.unit_rows(rng, 6, 7)
    lo = np.array([0, 0, 1, 3, 3], dtype=np.int32)
    c = align.cost_host(X, Y, lo, 4)
    for i in range(5):
        for k in range(4):
            j = lo[i] + k
            want = align.DEAD if j >= 6 else int(np.rint(min(max(1.0 - float(X[i] @ Y[j]), 0.0), 1.0) * 4095))
            assert c[i, k] == want
    assert c.dtype == np.uint16 and (c[3:, 3] == align.DEAD).all()
    assert (align.cost_host(X, X, np.zeros(5, dtype=np.int32), 5).diagonal() == 0).all()


def test_band_construction():
    """The band reaches R + S columns past S row_lo_c, so it holds the fine cells of every coarse path cell of a row as long as
    S (row_hi_c - row_lo_c) <= R + 1 -- at the defaults (R = 125, S = 8) a horizontal run of 15 coarse cells, 3.8 s of score against
    a quarter second of recording.  Here the longest run is 2 cells and R = 16; `align_logmels` reports a longer run as
    coarse_inside = False."""
    N, M, S, R = 83, 97, 8, 16
    row_lo_c = np.array([0, 0, 1, 2, 2, 3, 5, 6, 8, 10])    # N // S = 10 coarse rows, M // S = 12 coarse columns
    row_hi_c = np.array([0, 1, 2, 2, 3, 5, 6, 8, 10, 11])
    lo, W = align.band_from_coarse(row_lo_c, N, M, S, R)
    assert W == 2 * R + S + 1 and lo.dtype == np.int32 and len(lo) == N
    assert lo[0] == 0 and (np.diff(lo) >= 0).all() and lo.max() <= M - W
    assert lo[-1] + W >= M                                     # the last row reaches column M - 1
    # every fine cell under a coarse path cell lies inside the band (rows past the last whole coarse row belong to it; so do the
    # columns past the last whole coarse column)
    for ic in range(len(row_lo_c)):
        rows = range(ic * S, N if ic == len(row_lo_c) - 1 else (ic + 1) * S)
        for jc in range(row_lo_c[ic], row_hi_c[ic] + 1):
            cols = range(jc * S, M if jc == M // S - 1 else (jc + 1) * S)
            for i in rows:
                assert lo[i] <= cols[0] and cols[-1] < lo[i] + W, (ic, jc, i)
    # a band as wide as the matrix
    lo, W = align.band_from_coarse(row_lo_c, N, 20, S, R)
    assert W == 20 and (lo == 0).all()
    # S doubles while the coarse matrix would pass 8192 columns
    assert align.coarse_factor(8192 * 8, 8) == 8 and align.coarse_factor(8192 * 8 + 8, 8) == 16
    assert align.coarse_factor(100, 8) == 8 and align.coarse_factor(200000, 8) == 32 and 200000 // 32 <= align.MAX_W


def test_refusals_come_before_any_work():
    big = np.broadcast_to(np.zeros((1, 229)), (200000, 229))               # no memory behind it: nothing may touch it
    small = np.broadcast_to(np.zeros((1, 229)), (70000, 229))
    with pytest.raises(ValueError, match=r'2\^18'):
        align.align_logmels([(big, small)], names=['symphony'])
    with pytest.raises(ValueError, match=r'2\^18'):
        align.dtw_host(np.broadcast_to(np.zeros((1, 1), dtype=np.uint16), (1 << 18, 1)), np.zeros(1 << 18, dtype=np.int32), 1, 5)
    with pytest.raises(ValueError, match='band of 9000'):
        align.dtw_host(np.zeros((2, 9000), dtype=np.uint16), np.zeros(2, dtype=np.int32), 9000, 9000)
    with pytest.raises(ValueError, match='non-decreasing'):
        align.dtw_host(np.zeros((3, 2), dtype=np.uint16), np.array([0, 2, 1]), 2, 4)
    with pytest.raises(ValueError, match='more than 1024 samples'):
        align.logmel_host(np.zeros(1000, dtype=np.int16))


def test_features():
    rng = np.random.RandomState(2)
    lm = rng.uniform(align.FLOOR - 2.0, 3.0, size=(21, 229))
    f = align.features(lm)
    assert f.shape == (21, 230) and np.allclose((f * f).sum(1), 1.0) and (f >= 0).all()
    raw = np.clip(lm - align.FLOOR, 0, None)
    assert np.allclose(f[:, -1], align.KAPPA / np.sqrt((raw * raw).sum(1) + align.KAPPA ** 2))
    c = align.features(lm, 4)                                               # 5 coarse frames, the tail frame dropped
    pooled = raw[:20].reshape(5, 4, 229).mean(1)
    assert c.shape == (5, 230) and np.allclose(c[:, :-1] * np.sqrt((pooled * pooled).sum(1) + 64.0)[:, None], pooled)
    t = align.features(torch.from_numpy(lm), 4)
    assert torch.is_tensor(t) and np.allclose(t.numpy(), c)
    silence = align.features(align.logmel_host(np.zeros(4096, dtype=np.int16)))
    assert silence.shape == (9, 230) and np.allclose(silence[:, -1], 1.0)    # silence matches silence at cost 0
    assert (align.cost_host(silence, silence, np.zeros(9, dtype=np.int32), 9) == 0).all()


def test_logmel_host_is_the_front_end():
    """The float64 restatement against the oracle's float32 front end (conv1d with the windowed kernels) on one second of noise."""
    from oracle import frontend as of
    rng = np.random.RandomState(3)
    pcm = (rng.randn(16000) * 3000).astype(np.int16)
    want = torch.log(of.melspec_power(torch.from_numpy(pcm.astype(np.float32) / 32768.0)[None], of.frontend_buffers()) + 1e-5)[0].T.numpy()
    got = align.logmel_host(pcm)
    assert got.shape == want.shape == (32, 229) and np.abs(got - want).max() < 2e-3


def test_end_to_end_on_the_host():
    """The 12 s case (seed 3: 60 notes; score in Timbre('struck', 0), recording in Timbre('struck', 7) through
    t' = 0.4 + 1.15 t + 0.5 sin(2 pi t / 7) with white noise at -66 dBFS).  Coarse-to-fine gives the full matrix's total and path.
    Measured on the host definition: 58 of 60 onsets (0.967) within 50 ms of the truth, median error 13.6 ms; the floor is 0.90."""
    notes, rec, truth = ac.e2e_case()
    assert len(notes) == 60
    from reconvat_amd import synth
    score = synth.render(notes, align.score_length(notes), synth.Timbre('struck', 0), out_dtype=torch.int16).numpy()
    X, Y = align.logmel_host(rec), align.logmel_host(score)
    two = align.align_frames(X, Y, coarse=8, radius=48)
    assert two['S'] == 8 and two['W'] == 2 * 48 + 8 + 1 < two['M'] and two['coarse_inside']
    full = align.dtw_pairs([(align.features(X), align.features(Y))], [np.zeros(len(X), dtype=np.int32)], [len(Y)])[0]
    ac.same_result(two, full)
    aligned, report = align.align_score(rec, notes)
    assert report['total'] == full['total'] and report['length'] == full['length'] and 0.0 < report['mean_cost'] < 0.25
    assert (report['N'], report['M'], report['S']) == (len(X), len(Y), 8)
    share = ac.onset_share(aligned, truth)
    print(f'host: {share:.3f} of {len(notes)} onsets within 50 ms, median |error| {np.median(np.abs(aligned[:, 0] - truth)) * 1e3:.1f} ms')
    assert share >= 0.90
    assert np.array_equal(aligned[:, 2:], notes[:, 2:])                     # pitches and velocities untouched
    assert (aligned[:, 1] >= aligned[:, 0] + align.FRAME_S - 1e-12).all() and aligned.min() >= 0 and aligned[:, :2].max() <= len(rec) / 16000


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    path = tmp_path_factory.mktemp('scores')
    return str(path), ac.make_folder(str(path))


def test_align_scores_cli_on_the_host(folder, capsys):
    import align_scores
    from reconvat_amd.dataset import ingest_track, read_audio_int16
    path, scores = folder
    out = os.path.join(path, 'aligned')
    done = align_scores.main(['with', f'input={path}', f'output={out}', 'device=cpu'])
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith('piece')]
    assert [d[0] for d in done] == sorted(scores) == [f'piece{i}' for i in range(5)] and len(lines) == 5
    assert all(re.match(r'piece\d: N=\d+ M=\d+ S=\d+ W=\d+ total=\d+ length=\d+ mean_cost=0\.\d+', l) for l in lines)
    assert sorted(os.listdir(out)) == [f'piece{i}.tsv' for i in range(5)]
    for name, target, report in done:
        assert open(target).readline().strip() == '# onset,offset,note,velocity'
        rows = np.loadtxt(target, delimiter='\t', skiprows=1, ndmin=2)
        direct, _ = align.align_score(read_audio_int16(os.path.join(path, name + '.wav')), scores[name])
        assert np.allclose(rows, direct, atol=1e-6) and np.array_equal(rows[:, 2:], scores[name][:, 2:])
    # ingest_track loads a written file with its recording
    import shutil
    shutil.copy(os.path.join(path, 'piece0.wav'), os.path.join(out, 'piece0.wav'))
    track = ingest_track(os.path.join(out, 'piece0.wav'), os.path.join(out, 'piece0.tsv'))
    assert track['label'].shape == ((len(track['audio']) - 1) // 512 + 1, 88) and int((track['label'] == 3).sum()) > 0
    with pytest.raises(FileExistsError, match='overwrite=True'):
        align_scores.main(['with', f'input={path}', f'output={out}', 'device=cpu'])
    align_scores.main(['with', f'input={path}', f'output={out}', 'device=cpu', 'overwrite=True'])
    with pytest.raises(SystemExit):
        align_scores.main(['with', 'device=cpu'])
    os.makedirs(os.path.join(out, 'nothing'))
    with pytest.raises(ValueError, match='no name.wav'):
        align_scores.main(['with', f'input={out}/nothing', 'device=cpu'])


def test_train_on_scores_folder(folder, tmp_path):
    import shutil
    from reconvat_amd.dataset import prepare_VAT_dataset
    path, scores = folder
    work = str(tmp_path / 'corpus')
    shutil.copytree(path, work, ignore=shutil.ignore_patterns('aligned', '*.tsv.*'))
    for f in os.listdir(work):                                              # (a copy without the tsv files another test may have written)
        if re.fullmatch(r'piece\d\.tsv', f):
            os.remove(os.path.join(work, f))
    seq = 32768
    l_set, ul_set, val, full = prepare_VAT_dataset(sequence_length=seq, validation_length=seq, refresh=False, device='cpu', dataset=f'Scores:{work}')
    assert sorted(f for f in os.listdir(work) if re.fullmatch(r'piece\d\.tsv', f)) == [f'piece{i}.tsv' for i in range(5)]
    name = lambda t: os.path.basename(t['path'])
    assert [name(t) for t in l_set.data] == [f'piece{i}.wav' for i in (1, 2, 3, 4)]
    assert [name(t) for t in ul_set.data] == ['piece5.wav'] and int(ul_set.data[0]['label'].sum()) == 0
    assert [name(t) for t in val.data] == [name(t) for t in full.data] == ['piece0.wav']
    for t in l_set.data + val.data:
        assert t['audio'].dtype == torch.int16 and t['label'].dtype == torch.uint8 and t['label'].shape == ((len(t['audio']) - 1) // 512 + 1, 88)
        assert int((t['label'] == 3).sum()) > 0 and t['velocity'].shape == t['label'].shape
    item = l_set[0]
    assert item['audio'].shape == (seq,) and item['onset'].shape == (seq // 512, 88) and full[0]['audio'].shape == full.data[0]['audio'].shape
    # an existing name.tsv is used as it is
    marker = np.array([[0.5, 1.0, 60.0, 77.0]])
    align.write_tsv(os.path.join(work, 'piece1.tsv'), marker)
    again = prepare_VAT_dataset(sequence_length=seq, validation_length=seq, refresh=False, device='cpu', dataset=f'Scores:{work}')[0]
    assert int(again.data[0]['velocity'].max()) == 77 and int((again.data[0]['label'] > 0).any(0).sum()) == 1
    # the two error cases
    os.remove(os.path.join(work, 'piece5.wav'))
    with pytest.raises(ValueError, match='without a score'):
        prepare_VAT_dataset(sequence_length=seq, validation_length=seq, refresh=False, device='cpu', dataset=f'Scores:{work}')
    shutil.copy(os.path.join(path, 'piece5.wav'), os.path.join(work, 'piece5.wav'))
    os.remove(os.path.join(work, 'piece4.score.tsv'))
    with pytest.raises(ValueError, match='at least five recordings'):
        prepare_VAT_dataset(sequence_length=seq, validation_length=seq, refresh=False, device='cpu', dataset=f'Scores:{work}')
    with pytest.raises(ValueError, match=r'Scores:<folder>'):
        prepare_VAT_dataset(sequence_length=seq, validation_length=seq, refresh=False, device='cpu', dataset='Nothing')


def test_abi_has_the_two_entry_points():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read(), flags=re.S)
    for name, n_args in (('rv_align_cost', 12), ('rv_align_dtw', 13)):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S)
        assert m and len(m.group(1).split(',')) == n_args == len(_lib.SIGNATURES[name][1])
    source = open(os.path.join(build.CSRC, 'align.hip')).read()
    assert 'align.hip' in build.SOURCES and 'align.hip' not in build.VARIANT_SOURCES and 'getenv' not in source
    assert align.DESC == int(re.search(r'#define ALIGN_DESC (\d+)', source).group(1))
    assert align.HEAD == int(re.search(r'#define ALIGN_HEAD (\d+)', source).group(1))
    assert align.MAX_W == int(re.search(r'#define ALIGN_MAX_W (\d+)', source).group(1))
