"""Pitch-shift augmentation on the device (rv_crop_segments_shift) against the float64 yardstick `augment.shift_item`.

Audio bound, derived and not measured (tests/test_resample.py::f32_bound): for every output sample |y - y64| <= (K + 8) 2^-24 S_m,
K = taps per output, S_m = sum_n |x[n]| 2^-15 |h[m M - n L]| -- a length-K float32 dot product in any order plus the float32 rounding
of the coefficients.  No sample is excluded.  Labels, k = 0 audio, batch-independence and repeatability are checked with ==.

Corpus: five tracks of 40 001 .. 70 001 samples, none a multiple of 8 long, so that they lie back to back with only the padding
between them.  Tracks 1 and 3 are full scale with dense labels, track 2 and 4 are quiet: a read that leaks from a neighbour is
thousands of times the bound."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from reconvat_amd import augment
from reconvat_amd.constants import HOP_LENGTH
from test_pitch_shift import SHIFTS, note_track
from test_resample import f32_bound

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [52003, 40001, 61111, 45679, 70001]
NAMES = ('audio', 'onset', 'offset', 'frame', 'velocity')


@functools.lru_cache(maxsize=None)
def tracks():
    rng = np.random.RandomState(2024)
    out = []
    for i, T in enumerate(LENGTHS):
        assert T % 8
        rows = (T - 1) // HOP_LENGTH + 1
        if i in (1, 3):                                                            # the loud neighbours
            audio = np.where(rng.randint(0, 2, T) > 0, 32767, -32768).astype(np.int16)
            label = rng.randint(0, 4, (rows, 88)).astype(np.uint8)
            velocity = rng.randint(1, 128, (rows, 88)).astype(np.uint8)
        else:
            audio = rng.randint(-200 if i in (2, 4) else -32768, 201 if i in (2, 4) else 32768, T).astype(np.int16)
            label, velocity = note_track(50 + i, n_steps=rows, n_notes=50)
            label[-1, ::3], velocity[-1, ::3] = 2, 99                               # something sounding in the very last row
        out.append({'path': f'track{i}.flac', 'audio': audio, 'label': label, 'velocity': velocity})
    return out


@functools.lru_cache(maxsize=None)
def want(idx, j0, k, seq):
    """The yardstick item plus (S, K) of the audio bound; computed once per case and shared."""
    t = tracks()[idx]
    item = augment.shift_item(t, j0, k, seq)
    item['S'] = augment.shift_audio(t['audio'], j0 * HOP_LENGTH, k, seq, magnitude=True)
    item['K'] = augment.taps(k)
    return item


@functools.lru_cache(maxsize=None)
def corpus(seq, batch, pitch_shift=6):
    from reconvat_amd.feed import DeviceCorpus
    return DeviceCorpus(tracks(), seq, batch, torch.device('cuda:0'), seed=42, pitch_shift=pitch_shift, aug_seed=5)


def positions(seq):
    """(track, source row) of the five places every shift is tried at."""
    rows = [t['label'].shape[0] for t in tracks()]
    last_drawn = (LENGTHS[2] - augment.span(6, seq) - 1) // HOP_LENGTH              # the last row a draw can give (for k = +6)
    return [(0, 37),                                                                # the middle of a track
            (2, 0),                                                                 # the filter reaches before the track: into track 1?
            (2, last_drawn),
            (2, rows[2] - 2),                                                       # audio and rows run out inside the item; track 3 follows
            (4, 0)]                                                                 # first sample of the track behind the loud track 3


def batches(seq):
    """13 batches of 5 items: position p of batch n is shifted by SHIFTS[(n + 3 p) % 13] -- every shift at every position, and every
    batch mixes ratios (so L, M and Kp differ between the workgroups of one launch)."""
    pos = positions(seq)
    return [[(idx, j0, SHIFTS[(n + 3 * p) % 13]) for p, (idx, j0) in enumerate(pos)] for n in range(13)]


def crop(dc, items):
    out = dc.crop([i for i, _, _ in items], [j for _, j, _ in items], [k for _, _, k in items])
    assert out['shift'].tolist() == [k for _, _, k in items] and out['shift'].dtype == torch.int64
    return {n: out[n].cpu().numpy() for n in NAMES}


def check_item(got, b, idx, j0, k, seq, tag):
    w = want(idx, j0, k, seq)
    y = got['audio'][b].astype(np.float64)
    err, bound = np.abs(y - w['audio']), f32_bound(w['S'], w['K'])
    worst = int(np.argmax(err - bound))
    print(f'{tag}: worst |y - y64| {err.max():.3e}; tightest sample {worst}: {err[worst]:.3e} of {bound[worst]:.3e}')
    assert np.all(err <= bound), tag
    if k == 0:
        assert np.array_equal(y, w['audio']), tag                                  # int16 * 2^-15: exact in float32
    for n in NAMES[1:]:
        assert np.array_equal(got[n][b], w[n]), (tag, n)


@pytest.mark.parametrize('seq', [2048, 512])
def test_every_shift_at_every_edge(dev, seq):
    dc = corpus(seq, 5)
    assert positions(seq)[2][1] > 0
    for n, items in enumerate(batches(seq)):
        got = crop(dc, items)
        assert got['audio'].shape == (5, seq) and got['frame'].shape == (5, seq // HOP_LENGTH, 88)
        for b, (idx, j0, k) in enumerate(items):
            check_item(got, b, idx, j0, k, seq, f'seq {seq} batch {n} item {b} (track {idx} row {j0} k {k:+d})')
    # the quiet track next to the loud ones stays quiet: nothing of a neighbour came through
    quiet = crop(dc, [(2, 0, 6), (2, positions(seq)[3][1], 6), (4, 0, -6)])
    assert np.abs(quiet['audio']).max() < 0.05


@pytest.mark.parametrize('seq', [2048, 512])
def test_items_do_not_depend_on_the_batch(dev, seq):
    """Each item of a batch equals the same item cropped alone, in a batch of three at another place, and a second run."""
    dc = corpus(seq, 5)
    for items in batches(seq):
        got = crop(dc, items)
        again = crop(dc, items)
        three = crop(dc, [items[4], items[0], items[2]])
        four = crop(dc, items[1:])
        for n in NAMES:
            assert np.array_equal(got[n], again[n]), n
            assert np.array_equal(three[n], got[n][[4, 0, 2]]) and np.array_equal(four[n], got[n][1:]), n
        for b, item in enumerate(items):
            alone = crop(dc, [item])
            for n in NAMES:
                assert np.array_equal(alone[n][0], got[n][b]), (item, n)


@pytest.mark.parametrize('seq', [2048, 512])
def test_unshifted_items_are_the_plain_crop(dev, seq):
    """k = 0 next to +-6 in one batch: bit-identical to rv_crop_segments at the same rows."""
    plain = corpus(seq, 5, pitch_shift=0)
    dc = corpus(seq, 5)
    rows = [(0, 37), (2, 0), (4, 0), (1, 5)]
    mixed = crop(dc, [(0, 37, 0), (2, 0, 6), (2, 0, 0), (4, 0, -6), (4, 0, 0)])
    alone = crop(dc, [(i, j, 0) for i, j in rows])
    ref = crop(plain, [(i, j, 0) for i, j in rows])
    for n in NAMES:
        assert np.array_equal(alone[n], ref[n]), n
        assert np.array_equal(mixed[n][[0, 2, 4]], ref[n][:3]), n
    check_item(mixed, 1, 2, 0, 6, seq, 'k +6 next to k 0')
    check_item(mixed, 3, 4, 0, -6, seq, 'k -6 next to k 0')
    with pytest.raises(ValueError, match='pitch_shift > 0'):
        plain.crop([0], [3], [1])


def test_pitch_shift_off_is_the_feed_as_it_was(dev):
    """DeviceCorpus(pitch_shift=0) and DeviceCorpus() draw and crop what the host item rule gives for the same seed."""
    from reconvat_amd.dataset import crop_item
    from reconvat_amd.feed import DeviceCorpus
    seq, order = 2048, [4, 0, 3, 3, 1]
    outs = [DeviceCorpus(tracks(), seq, 5, dev, seed=42, **kw).batch(order) for kw in ({}, {'pitch_shift': 0, 'aug_seed': 9})]
    rs = np.random.RandomState(42)
    for b, idx in enumerate(order):
        t = tracks()[idx]
        step = int(rs.randint(len(t['audio']) - seq)) // HOP_LENGTH
        item = crop_item({k: (torch.from_numpy(v) if k != 'path' else v) for k, v in t.items()}, step, seq)
        for out in outs:
            assert int(out['start_idx'][b]) == step * HOP_LENGTH and int(out['shift'][b]) == 0
            for n in NAMES:
                assert torch.equal(out[n][b].cpu(), item[n]), (b, n)
    assert outs[0]['path'] == [tracks()[i]['path'] for i in order]


def test_drawn_batches(dev):
    """batch(): k from the second stream, the crop from the first over T - span(k); the items are the yardstick's."""
    from reconvat_amd.feed import DeviceCorpus
    seq, order = 2048, [4, 0, 2, 2]
    dc = DeviceCorpus(tracks(), seq, 4, dev, seed=42, pitch_shift=6, aug_seed=5)
    seen = set()
    rs, aug = np.random.RandomState(42), np.random.RandomState(5)
    for _ in range(3):
        out = dc.batch(order)
        got = {n: out[n].cpu().numpy() for n in NAMES}
        steps, shifts = augment.draw_items(rs, aug, np.array(LENGTHS), order, seq, 6)
        assert out['shift'].tolist() == shifts.tolist() and out['start_idx'].tolist() == (steps * HOP_LENGTH).tolist()
        for b, idx in enumerate(order):
            check_item(got, b, idx, int(steps[b]), int(shifts[b]), seq, f'drawn item {b}')
        seen |= set(shifts.tolist())
    assert len(seen) > 3


def test_short_tracks_and_bad_arguments_are_refused(dev):
    from reconvat_amd import _lib
    from reconvat_amd._lib import ptr
    from reconvat_amd.feed import DeviceCorpus
    seq = 32768
    assert augment.span(6, seq) > LENGTHS[1] > augment.span(2, seq) > seq
    with pytest.raises(ValueError, match='pitch_shift=6'):
        DeviceCorpus(tracks(), seq, 2, dev, pitch_shift=6)
    DeviceCorpus(tracks(), seq, 2, dev, pitch_shift=2)
    with pytest.raises(ValueError, match='pitch_shift'):
        DeviceCorpus(tracks(), 2048, 2, dev, pitch_shift=7)
    dc = corpus(2048, 5)
    with pytest.raises(ValueError):
        dc.crop([0], [0], [7])
    with pytest.raises(ValueError):
        dc.crop([0], [tracks()[0]['label'].shape[0]], [1])
    with pytest.raises(ValueError):
        dc.crop([0], [-1], [1])
    # the entry point itself: bad arguments fail before any launch, and a table row outside the limits yields NaN, not a wild read
    lib = _lib.load()
    S = 4
    outs = [torch.zeros(1, 2048, device=dev)] + [torch.zeros(1, S, 88, device=dev) for _ in range(4)]
    row = np.zeros((1, 12), dtype=np.int64)
    row[0, :11] = [dc.a_off[0], dc.a_off[0], dc.a_off[0] + LENGTHS[0], *dc._banks[3], dc.l_off[0], dc.n_rows[0], 3]
    items = torch.from_numpy(row).to(dev)
    good = [ptr(dc.audio), dc.audio.numel(), ptr(dc.label), ptr(dc.velocity), dc.label.numel(), ptr(dc.banks), dc.banks.numel(), ptr(items),
            1, 2048, S, 88] + [ptr(o) for o in outs] + [None]
    assert lib.rv_crop_segments_shift(*good) == 0
    torch.cuda.synchronize()
    w = want(0, 0, 3, 2048)
    assert np.array_equal(outs[1][0].cpu().numpy(), w['onset']) and np.all(np.abs(outs[0][0].cpu().numpy() - w['audio']) <= f32_bound(w['S'], w['K']))
    for at, value in ((8, 0), (9, 0), (11, 86), (2, None), (7, None), (12, None), (5, ptr(dc.banks) + 4)):
        args = list(good)
        args[at] = value
        assert lib.rv_crop_segments_shift(*args) == -1, at
        assert 'rv_crop_segments_shift' in _lib.last_error()
    for col, value in ((3, 200), (6, 260), (7, dc.banks.numel())):
        bad = row.copy()
        bad[0, col] = value
        args = list(good)
        args[7] = ptr(torch.from_numpy(bad).to(dev))
        assert lib.rv_crop_segments_shift(*args) == 0
        torch.cuda.synchronize()
        assert bool(torch.isnan(outs[0]).all()), col
        if col == 3:
            assert all(bool(torch.isnan(o).all()) for o in outs[1:])


def test_command_line_run_with_pitch_shift(dev, tmp_path):
    """`train_UNet_VAT.py with ... pitch_shift=2`: two steps on the tiny synthetic corpus, labelled and unlabelled loader augmented."""
    logdir = str(tmp_path / 'shift')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_UNet_VAT.py'), 'with', 'train_on=Synthetic', 'small=True', 'supersmall=True',
                        'sequence_length=32768', 'batch_size=2', 'train_batch_size=2', 'iteration=2', 'VAT=True', 'reconstruction=False',
                        'epoches=1', 'pitch_shift=2', f'logdir={logdir}'], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout and 'transposed by a random k in [-2, 2] semitones' in p.stdout
    with open(os.path.join(logdir, 'scalars.jsonl')) as fh:
        rows = [json.loads(line) for line in fh]
    losses = [r['value'] for r in rows if r['tag'].startswith('loss/train_')]
    assert len(losses) >= 3 and np.all(np.isfinite(losses)), losses
    # the loader that run built: its batches carry the shifts
    from reconvat_amd.dataset import SyntheticSegments
    from reconvat_amd.feed import device_loader
    batch = next(iter(device_loader(SyntheticSegments(4, 32768, seed=1), 2, dev, seed=42, pitch_shift=2)))
    assert batch['shift'].dtype == torch.int64 and batch['shift'].shape == (2,) and int(batch['shift'].abs().max()) <= 2
    assert batch['audio'].shape == (2, 32768) and bool(torch.isfinite(batch['audio']).all())
