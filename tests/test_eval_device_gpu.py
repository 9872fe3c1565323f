"""Whole-song evaluation on the device (csrc/eval.hip and the device functions of reconvat_amd/decoding.py and
reconvat_amd/evaluate.py) against the host code it stands in for: the decoder against the reference's own golden and against
extract_notes_wo_velocity, the frame counters against evaluate_frames, AP against scikit-learn, and evaluate_wo_velocity end to
end with device_metrics on and off.  Everything but AP is compared exactly."""
import os

import numpy as np
import pytest
import torch

from test_decoding import decoding_rolls

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')


def painted_by_host(pitches, intervals, shape):
    """The roll notes_to_frames paints, rebuilt from the per-frame lists it returns."""
    from reconvat_amd import decoding as md
    _, freqs = md.notes_to_frames(pitches, intervals, shape)
    roll = np.zeros(shape, np.uint8)
    for t, f in enumerate(freqs):
        roll[t, f] = 1
    return roll


def check_against_host(on, fr, dev, thresholds, rule):
    from reconvat_amd import decoding as md
    on_t, fr_t = torch.from_numpy(on), torch.from_numpy(fr)
    want_p, want_i = md.extract_notes_wo_velocity(on_t, fr_t, *thresholds, rule=rule)
    p, i, roll = md.extract_notes_wo_velocity_device(on_t.to(dev), fr_t.to(dev), *thresholds, rule=rule)
    assert isinstance(p, np.ndarray) and isinstance(i, np.ndarray)
    assert p.shape == want_p.shape and i.shape == want_i.shape
    assert np.array_equal(p, want_p) and np.array_equal(i, want_i)
    assert roll.is_cuda and roll.dtype == torch.uint8 and tuple(roll.shape) == on.shape
    assert np.array_equal(roll.cpu().numpy(), painted_by_host(want_p, want_i, on.shape))
    return want_p, want_i


def test_decoder_matches_reference_golden(dev):
    from reconvat_amd import decoding as md
    g = np.load(os.path.join(G, 'decoding.npz'))
    for seed in (0, 1, 2):
        on, fr, _ = decoding_rolls(seed)
        for rule in ('rule1', 'rule2'):
            p, i, roll = md.extract_notes_wo_velocity_device(torch.from_numpy(on).to(dev), torch.from_numpy(fr).to(dev), 0.5, 0.5, rule=rule)
            assert np.array_equal(p, g[f'{seed}_{rule}_p']) and np.array_equal(i, g[f'{seed}_{rule}_i'])
            assert np.array_equal(roll.cpu().numpy(), painted_by_host(g[f'{seed}_{rule}_p'], g[f'{seed}_{rule}_i'], on.shape))


def tile_edge_rolls():
    """Three tiles of the kernel plus 7 frames, with everything that has to cross a tile edge."""
    from reconvat_amd.decoding import DEVICE_TILE_FRAMES as tile
    T = 3 * tile + 7
    on, fr = np.zeros((T, 88), np.float32), np.zeros((T, 88), np.float32)
    on[0, 5] = 1; fr[:, 5] = 1                                         # one pitch active throughout: the carry crosses whole tiles
    on[tile - 1, 10] = 1; fr[tile - 1:tile + 9, 10] = 1                # a note starting on the last frame of a tile
    on[tile + 30, 11] = 1; fr[tile + 30:2 * tile + 1, 11] = 1          # one ending on the first frame of the next tile
    fr[20:3 * tile - 10, 12] = 1                                       # a sustained frame run with the onset rising again and again,
    for t in (30, 31, tile - 1, tile + 1, 2 * tile, 2 * tile + 5):           # next to and on the tile edges
        on[t, 12] = 1
    fr[10:, 13] = 1                                                    # frames without any onset: no note, nothing painted
    on[2 * tile, 14] = 1                                               # onset without frames, first frame of a tile
    on[T - 1, 15] = 1                                                  # a note on the very last frame
    fr[0:tile, 16] = 1; on[tile, 16] = 1                               # a run that ends exactly with its tile, a note right after
    on += 0.05; fr += 0.05                                             # off the exact zeros, below both threshold pairs
    return on, fr


def scaled_random_rolls(T, seed):
    """The decoding_rolls recipe at T frames with proportionally more notes."""
    rng = np.random.RandomState(seed)
    frames = np.zeros((T, 88), np.float32)
    onsets = np.zeros((T, 88), np.float32)
    for _ in range(120 * T // 300):
        t0, p, ln = rng.randint(0, T), rng.randint(0, 88), rng.randint(1, 40)
        frames[t0:t0 + ln, p] = rng.uniform(0.3, 1.0)
        if rng.rand() < 0.8:
            onsets[t0:min(T, t0 + rng.randint(1, 4)), p] = rng.uniform(0.3, 1.0)
    onsets += rng.uniform(0, 0.2, size=onsets.shape).astype(np.float32)
    frames += rng.uniform(0, 0.2, size=frames.shape).astype(np.float32)
    return onsets, frames


def host_cases():
    one = np.zeros((1, 88), np.float32)
    one_on = one.copy(); one_on[0, 40] = 1
    last_on, last_fr = np.zeros((10, 88), np.float32), np.zeros((10, 88), np.float32)
    last_on[7, 3] = 1; last_fr[7:, 3] = 1
    return {
        'T1_empty': (one, one),
        'T1_note': (one_on, one_on),
        'T10_zeros': (np.zeros((10, 88), np.float32), np.zeros((10, 88), np.float32)),
        'T10_to_the_end': (last_on, last_fr),
        'all_ones': (np.ones((130, 88), np.float32), np.ones((130, 88), np.float32)),
        'tile_edges': tile_edge_rolls(),
        'random_2077': scaled_random_rolls(2077, 3),
    }


@pytest.mark.parametrize('case', ['T1_empty', 'T1_note', 'T10_zeros', 'T10_to_the_end', 'all_ones', 'tile_edges', 'random_2077'])
def test_decoder_matches_host_function(dev, case):
    on, fr = host_cases()[case]
    for rule in ('rule1', 'rule2'):
        for thresholds in ((0.5, 0.5), (0.4, 0.6)):
            p, i = check_against_host(on, fr, dev, thresholds, rule)
            if case in ('T1_empty', 'T10_zeros'):
                assert p.shape == (0,) and i.shape == (0,)              # np.array([]) twice, like the host
            if case == 'T10_to_the_end':
                assert p.tolist() == [3] and i.tolist() == [[7, 10]]
            if case == 'all_ones':
                assert p.tolist() == list(range(88)) and i.tolist() == [[0, 130]] * 88
            if case == 'tile_edges':
                assert len(p) >= 8 and [5, [0, on.shape[0]]] in [[a, b] for a, b in zip(p.tolist(), i.tolist())]


def roll_pair(T, density, seed):
    """A reference roll of the given density and an estimate: part of it kept, part of it moved up or down an octave (a chroma
    match that is no plain match), plus unrelated false alarms."""
    rng = np.random.RandomState(seed)
    ref = rng.rand(T, 88) < density
    keep = rng.rand(T, 88) < 0.6
    est = ref & keep
    octave = ref & ~keep & (rng.rand(T, 88) < 0.5)
    est[:, 12:] |= octave[:, :-12]
    est[:, :-12] |= octave[:, 12:] & (rng.rand(T, 76) < 0.5)
    est |= rng.rand(T, 88) < density * 0.1
    return ref.astype(np.uint8), est.astype(np.uint8)


def frames_by_host(ref, est):
    from reconvat_amd import evaluate as ev
    T = ref.shape[0]
    units = lambda roll: ev._frames_to_eval_units(np.arange(T), [roll[t].nonzero()[0] for t in range(T)])
    return ev.evaluate_frames(*units(ref), *units(est))


@pytest.mark.parametrize('T', [257, 2077])
@pytest.mark.parametrize('density', [0.02, 0.2, 0.9])
def test_frame_counters_equal_host_metrics(dev, T, density):
    from reconvat_amd import evaluate as ev
    ref, est = roll_pair(T, density, seed=int(density * 100) + T)
    want = frames_by_host(ref, est)
    got = ev.evaluate_frames_device(torch.from_numpy(ref).to(dev), torch.from_numpy(est).to(dev))
    assert list(got) == list(want) and len(got) == 14
    for k in want:
        assert got[k] == want[k], (k, got[k], want[k])
    assert want['Chroma Precision'] > want['Precision'] > 0            # the octave errors are in there


def test_frame_counters_empty_rolls(dev):
    from reconvat_amd import evaluate as ev
    ref, est = roll_pair(257, 0.2, seed=5)
    zero = np.zeros_like(ref)
    for a, b in ((zero, est), (ref, zero), (zero, zero)):
        want = frames_by_host(a, b)
        got = ev.evaluate_frames_device(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
        assert list(got) == list(want)
        for k in want:
            assert got[k] == want[k], (k, got[k], want[k])
    assert all(v == 0.0 for v in got.values())


@pytest.mark.parametrize('T', [300, 2077])
@pytest.mark.parametrize('scores', ['continuous', 'sixteenths'])
def test_average_precision_vs_sklearn(dev, T, scores):
    """|AP_device - AP_sklearn| <= 1e-9, derived: the counts behind every precision and recall value are exact integers in float64,
    each term of the sum costs one division and one product (a few 1.1e-16 relative), and at most 2e6 terms add up to a summation
    error below 2e6 * 1.1e-16 = 2.2e-10."""
    from sklearn.metrics import average_precision_score
    from reconvat_amd import evaluate as ev
    rng = np.random.RandomState(T)
    y = (rng.rand(T, 88) < 0.08).astype(np.float32)
    s = rng.rand(T, 88)
    s = np.where(y > 0, np.minimum(s + 0.3 * rng.rand(T, 88), 1.0), s)  # informative, far from perfect
    if scores == 'sixteenths':
        s = np.floor(s * 16) / 16
    s = s.astype(np.float32)
    assert 0 < y.sum() < y.size
    want = average_precision_score(y.flatten(), s.flatten())
    got = ev.average_precision_device(torch.from_numpy(y).to(dev), torch.from_numpy(s).to(dev))
    assert isinstance(got, float) and 0.05 < want < 0.95
    assert abs(got - want) <= 1e-9, (got, want)


def test_evaluate_wo_velocity_device_metrics_equal_host_metrics(dev, monkeypatch):
    """The whole loop, reconstruction block included, on a 1 111-frame song with the fixture UNet_Onset: the same keys in the same
    order and the same values (the two AP keys within the bound of the AP test), and no call of notes_to_frames on the device path."""
    from test_eval_gpu import build, song
    from reconvat_amd import decoding, evaluate
    s = song(1111, 'song_1111')
    m = build('onset', True, dev)
    item = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in s.items()}
    with torch.no_grad():
        want = evaluate.evaluate_wo_velocity([item], m, reconstruction=True, onset=True, VAT=True, device_metrics=False)
    calls = []
    real = decoding.notes_to_frames

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)
    monkeypatch.setattr(decoding, 'notes_to_frames', counted)
    monkeypatch.setattr(evaluate, 'notes_to_frames', counted)
    with torch.no_grad():
        got = evaluate.evaluate_wo_velocity([item], m, reconstruction=True, onset=True, VAT=True, device_metrics=True)
    assert not calls
    assert list(got) == list(want)
    assert 'metric/note/overlap_2' in want and 'metric/frame/chroma_total_error' in want and 'metric/MusicNet/micro_avg_P2' in want
    for k in want:
        assert len(got[k]) == len(want[k]) == 1
        if k.startswith('metric/MusicNet/micro_avg_P'):
            assert abs(got[k][0] - want[k][0]) <= 1e-9, (k, got[k], want[k])
        else:
            assert got[k][0] == want[k][0], (k, got[k], want[k])
