"""The synthesiser's definition on the host (reconvat_amd/synth.py): known answers of the float64 yardstick, the partial
table, the tile lists, the seeded scores and the rendered corpus.  No GPU: `render` on device='cpu' is `render_host`."""
import os

import numpy as np
import pytest
import torch

from reconvat_amd import synth
from reconvat_amd.constants import HOP_LENGTH
from reconvat_amd.dataset import RenderedScores, paint_roll, prepare_VAT_dataset

U32 = 1 << 32


def row(s, e, inc, ph, amp, dec, A, R):
    r = np.zeros(8, dtype=np.uint32)
    r[[0, 1, 6, 7]] = np.array([s, e, A, R], dtype=np.int32).view(np.uint32)
    r[2], r[3] = inc % U32, ph % U32
    r[4:6] = np.array([amp, dec], dtype=np.float32).view(np.uint32)
    return r


def envelope(n, s, e, amp, dec, A, R):
    t = n - s
    att = np.minimum(t + 1, A) / A
    rel = np.where(n < e, 1.0, ((e + R - n) / R) ** 2)
    return np.where((n >= s) & (n < e + R), float(np.float32(amp)) * att * np.exp(-float(np.float32(dec)) * t) * rel, 0.0)


def test_dc_row_is_its_envelope_and_silence_outside():
    s, e, amp, dec, A, R = 100, 700, 0.25, 3e-3, 48, 160
    rows = row(s, e, 0, 1 << 30, amp, dec, A, R)[None]
    n = np.arange(1000)
    y = synth.render_host(rows, 0, 1000)
    np.testing.assert_allclose(y, envelope(n, s, e, amp, dec, A, R), rtol=1e-15, atol=0)
    assert np.all(y[:s] == 0) and np.all(y[e + R:] == 0) and y[s] > 0 and y[e + R - 1] > 0
    S, E = synth.render_host(rows, 0, 1000, magnitude=True)
    np.testing.assert_allclose(S, y, rtol=1e-15)
    np.testing.assert_allclose(E, envelope(n, s, e, amp, 0.0, A, R), rtol=1e-15)


def test_half_turn_step_alternates_in_sign():
    ph = 123456789
    rows = row(0, 64, 1 << 31, ph, 1.0, 0.0, 1, 1)[None]
    y = synth.render_host(rows, 0, 64)
    want = np.sin(2 * np.pi * ph / U32) * (-1.0) ** np.arange(64)
    np.testing.assert_allclose(y, want, rtol=0, atol=1e-12)


def test_phase_wraps_without_a_jump():
    inc, ph = 3 << 20, U32 - (1 << 22) + 12345                       # wraps at t = 2 and every 1365.3 samples after
    rows = row(0, 4000, inc, ph, 1.0, 0.0, 1, 1)[None]
    y = synth.render_host(rows, 0, 4000)
    t = np.arange(4000, dtype=np.float64)
    np.testing.assert_allclose(y, np.sin(2 * np.pi * (ph + inc * t) / U32), rtol=0, atol=1e-9)
    assert np.abs(np.diff(y)).max() <= 2 * np.pi * inc / U32 * 1.0001                  # no step larger than the phase step allows
    r2 = row(0, 4, U32 - 1, 5, 1.0, 0.0, 1, 1)[None]                                  # inc = 2^32 - 1: the phase steps back by one unit
    np.testing.assert_allclose(synth.render_host(r2, 0, 4), np.sin(2 * np.pi * (5 - np.arange(4)) / U32), rtol=0, atol=1e-15)


def test_render_host_in_chunks_is_render_host_whole():
    rs = np.random.RandomState(3)
    rows = synth.partials(synth.random_score(rs, 5.0), synth.Timbre('struck', 4))
    n = 5 * 16000
    whole = synth.render_host(rows, 0, n)
    cuts = [0, 1, 1023, 1024, 30000, 30001, n]
    parts = np.concatenate([synth.render_host(rows, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])])
    assert np.array_equal(parts, whole) and np.abs(whole).max() > 0.01


@pytest.mark.parametrize('voice', ['struck', 'sustained'])
def test_partials_properties(voice):
    timbre = synth.Timbre(voice, 11)
    notes = synth.random_score(np.random.RandomState(5), 8.0)
    rows = synth.partials(notes, timbre)
    s = rows[:, 0].view(np.int32)
    assert rows.dtype == np.uint32 and rows.shape[1] == 8 and len(rows) > len(notes) and np.all(np.diff(s) >= 0)
    f, valid = synth.partial_frequencies(notes, timbre)
    assert np.all(f[valid] <= 7200.0) and valid.sum() == len(rows) and valid[:, 0].all()
    assert np.all(valid[:, :-1] >= valid[:, 1:])                                       # k = 1 .. K: a prefix
    order = np.argsort(np.repeat(np.rint(16000 * notes[:, 0]).astype(np.int64), valid.sum(axis=1)), kind='stable')
    inc = (np.rint(f[valid] / 16000 * 2.0 ** 32).astype(np.int64) % U32)[order]
    assert np.array_equal(rows[:, 2].astype(np.int64), inc)
    e = rows[:, 1].view(np.int32)
    assert np.all(e > s) and np.all(rows[:, 6] == synth.VOICES[voice]['A']) and np.all(rows[:, 7] == synth.VOICES[voice]['R'])
    dec = rows[:, 5].view(np.float32)
    assert np.all(dec > 0) if voice == 'struck' else np.all(dec == 0)
    assert len(np.unique(rows[:, 3])) > 0.99 * len(rows)                               # the start phases are spread
    assert np.array_equal(rows, synth.partials(notes, synth.Timbre(voice, 11)))
    with pytest.raises(ValueError, match='2\\^24'):
        synth.partials([[1.0, 1.0 + (2 ** 24) / 16000.0, 60, 80]], timbre)
    with pytest.raises(ValueError, match='2\\^31'):
        synth.partials([[2 ** 31 / 16000.0 - 1.0, 2 ** 31 / 16000.0, 60, 80]], timbre)
    assert synth.partials(np.zeros((0, 4)), timbre).shape == (0, 8)


def test_timbre_draws_in_the_documented_order():
    rs = np.random.RandomState(9)
    t = synth.Timbre('sustained', 9)
    assert (t.p, t.even, t.scale, t.cents) == (rs.uniform(1, 2), rs.uniform(0.3, 1), rs.uniform(0.6, 1.4), rs.uniform(-10, 10))
    with pytest.raises(ValueError, match='voice'):
        synth.Timbre('plucked', 0)


def test_a4_peaks_at_440_hz():
    timbre = synth.Timbre('sustained', 2)
    n = 16000
    y = synth.render([[0.0, 1.5, 69, 100]], n, timbre, device='cpu', out_dtype=torch.float32).numpy()
    spectrum = np.abs(np.fft.rfft(y * np.hanning(n)))
    f = 440.0 * 2.0 ** (timbre.cents / 1200.0)
    assert int(np.argmax(spectrum)) == int(np.rint(f * n / 16000))                      # bins of 1 Hz
    assert abs(f - 440.0) < 440.0 * (2 ** (10 / 1200) - 1) + 1e-9


def test_tile_lists_against_the_double_loop():
    rs = np.random.RandomState(8)
    n_tiles = 12
    rows = []
    for i in range(200):
        s = int(rs.randint(0, n_tiles * 1024 + 600))
        span, R = int(rs.randint(1, 4000)), int(rs.randint(1, 1500))
        if i % 10 == 0:
            s = 1024 * int(rs.randint(0, n_tiles))                                     # starts on a tile boundary
        if i % 10 == 1:
            span = 1024 * int(rs.randint(1, 4)) - (s % 1024) - R                      # e + R falls on a tile boundary
            if span < 1:
                span, R = 1024 - (s % 1024) - 1, 1
                if span < 1:
                    s, span = s - 5, 4
        rows.append(row(s, s + span, 1, 2, 0.1, 0.0, 3, R))
    rows = np.stack(rows)
    s, end = rows[:, 0].view(np.int32).astype(np.int64), rows[:, 1].view(np.int32).astype(np.int64) + rows[:, 7]
    assert np.any(s % 1024 == 0) and np.any(end % 1024 == 0) and np.any(s >= n_tiles * 1024)
    tile_ptr, tile_rows = synth.tile_lists(rows, n_tiles)
    assert tile_ptr.dtype == np.int32 and tile_rows.dtype == np.int32 and tile_ptr.shape == (n_tiles + 1,) and tile_ptr[0] == 0
    for j in range(n_tiles):
        want = [i for i in range(len(rows)) if s[i] < 1024 * (j + 1) and end[i] > 1024 * j]
        assert list(tile_rows[tile_ptr[j]:tile_ptr[j + 1]]) == want, j
    assert tile_ptr[-1] == len(tile_rows)
    empty_ptr, empty_rows = synth.tile_lists(np.zeros((0, 8), dtype=np.uint32), 3)
    assert list(empty_ptr) == [0, 0, 0, 0] and len(empty_rows) == 0


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_random_score(seed):
    seconds = 12.0
    notes = synth.random_score(np.random.RandomState(seed), seconds)
    assert np.array_equal(notes, synth.random_score(np.random.RandomState(seed), seconds)) and len(notes) > 10
    on, off, key, vel = notes.T
    assert np.all(on >= 0.5) and np.all(off > on) and np.all(off + 1600 / 16000 <= seconds)
    assert np.all((key >= 21) & (key <= 108)) and np.all((vel >= 30) & (vel <= 120))
    assert np.all((off - on >= 0.08 - 1e-12) & (off - on <= 2.0 + 1e-12))
    for k in np.unique(key):
        mine = notes[key == k]
        mine = mine[np.argsort(mine[:, 0])]
        assert np.all(mine[1:, 0] - mine[:-1, 1] >= 0.2), k                            # no key carries two notes closer than 0.2 s
    n_steps = (int(seconds * 16000) - 1) // HOP_LENGTH + 1
    label, _ = paint_roll(notes, n_steps)
    head = np.rint(on * 31.25).astype(np.int64)
    assert np.all(label[head, key.astype(np.int64) - 21] == 3)


@pytest.fixture(scope='module')
def corpus():
    return prepare_VAT_dataset(sequence_length=32768, validation_length=32768, refresh=False, device='cpu', small=True, supersmall=True,
                               dataset='Rendered')


def test_rendered_corpus(corpus):
    l_set, ul_set, val, full = corpus
    seq = 32768
    assert [len(d.data) for d in corpus] == [4, 16, 4, 4]
    paths = [set(t['path'] for t in d.data) for d in (l_set, ul_set, val)]
    assert all(len(p) == len(d.data) for p, d in zip(paths, (l_set, ul_set, val)))
    assert not (paths[0] & paths[1]) and not (paths[0] & paths[2]) and not (paths[1] & paths[2])
    assert all(p.startswith('rendered/struck/') for p in paths[0])
    for p in paths[1:]:
        assert {q.split('/')[1] for q in p} == {'struck', 'sustained'}
    assert [t['path'] for t in full.data] == [t['path'] for t in val.data]
    assert l_set.sequence_length == seq and val.sequence_length == seq and full.sequence_length is None
    for d in corpus:
        for t in d.data:
            n = len(t['audio'])
            assert n == 2 * seq + 16 * HOP_LENGTH and n > seq and t['audio'].dtype == torch.int16
            assert t['label'].shape == ((n - 1) // HOP_LENGTH + 1, 88) == t['velocity'].shape and t['label'].dtype == torch.uint8
            assert int(t['label'].max()) == 3
    item = l_set[0]
    assert set(item) == {'path', 'audio', 'label', 'onset', 'offset', 'frame', 'velocity', 'start_idx'}
    assert item['audio'].shape == (seq,) and item['audio'].dtype == torch.float32
    for k in ('label', 'onset', 'offset', 'frame', 'velocity'):
        assert item[k].shape == (seq // HOP_LENGTH, 88), k
    assert full[0]['audio'].shape == (2 * seq + 16 * HOP_LENGTH,)


def test_rendered_corpus_is_clip_free_and_within_one_lsb(corpus):
    """On the definition alone: no sample of the corpus reaches full scale, and 32768 times the error bound of the device path stays
    below 1 everywhere -- the precondition of the 1-LSB agreement of the two paths."""
    peaks = []
    for d in corpus[:3]:
        for t, notes in zip(d.data, d.scores):
            voice, seed = t['path'].split('/')[1:]
            rows = synth.partials(notes, synth.Timbre(voice, int(seed)))
            n = len(t['audio'])
            y = synth.render_host(rows, 0, n)
            assert np.array_equal(synth.to_int16(y), t['audio'].numpy())
            assert np.abs(y).max() * 32768 < 32767 and int(t['audio'].abs().max()) < 32767
            assert 32768 * synth.error_bound(rows, 0, n).max() < 1
            peaks.append(np.abs(y).max())
    assert max(peaks) > 0.05                                                           # and it is not silence


def test_rendered_scores_takes_scores_and_voices():
    notes = np.array([[0.1, 0.4, 60, 90], [0.3, 0.5, 64, 70]])
    d = RenderedScores(2, 16000, ('sustained', 'struck'), seed=5, scores=[notes, ('tune.mid', notes)])
    assert [t['path'] for t in d.data] == ['rendered/sustained/5', 'rendered/struck/tune.mid'] and len(d) == 2
    assert not torch.equal(d.data[0]['audio'], d.data[1]['audio']) and torch.equal(d.data[0]['label'], d.data[1]['label'])
    long = RenderedScores(1, 1000, 'struck', scores=[notes])
    assert len(long.data[0]['audio']) == 8000 + 16000
    with pytest.raises(ValueError, match='scores'):
        RenderedScores(3, 16000, scores=[notes])


def test_folder_mode(tmp_path):
    rs = np.random.RandomState(0)
    for i in range(5):
        np.savetxt(tmp_path / f'score{i}.tsv', synth.random_score(rs, 5.0), fmt='%.6f', delimiter='\t', header='onset,offset,note,velocity')
    (tmp_path / 'notes.txt').write_text('not a score')
    sets = prepare_VAT_dataset(sequence_length=16384, validation_length=16384, refresh=False, device='cpu', dataset=f'Rendered:{tmp_path}')
    names = [[os.path.basename(t['path']) for t in d.data] for d in sets]
    assert names == [['score1.tsv'], ['score2.tsv', 'score3.tsv', 'score4.tsv'], ['score0.tsv'], ['score0.tsv']]
    assert all(len(t['audio']) > 16384 for d in sets for t in d.data)
    os.remove(tmp_path / 'score4.tsv')
    with pytest.raises(ValueError, match='at least five'):
        prepare_VAT_dataset(sequence_length=16384, validation_length=16384, refresh=False, device='cpu', dataset=f'Rendered:{tmp_path}')


def test_unknown_corpus_names_the_new_value():
    with pytest.raises(ValueError, match='Rendered'):
        prepare_VAT_dataset(32768, 32768, False, 'cpu', dataset='Nothing')
    from reconvat_amd.cli import base_config
    assert os.sep not in base_config({'train_on': 'Rendered:/some/folder', 'root': 'runs'}, True)['logdir'][len('runs/'):]
