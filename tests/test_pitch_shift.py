"""Pitch-shift augmentation of the device feed, host side: the ratio table, the float64 yardstick `augment.shift_item`
against the resampler's own host path and against properties of the label rule, the draws, and the config surface.
tests/test_pitch_shift_gpu.py compares the device path with the yardstick."""
import math
import os
import re

import numpy as np
import pytest

from reconvat_amd import augment
from reconvat_amd.constants import HOP_LENGTH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIFTS = list(range(-6, 7))


def note_track(seed, n_steps=400, n_notes=50):
    """A roll painted by `paint_roll` from about `n_notes` random notes that do not overlap on their key, with velocities."""
    from reconvat_amd.dataset import paint_roll
    rng = np.random.RandomState(seed)
    hop = HOP_LENGTH / 16000.0
    notes, busy = [], {}
    while len(notes) < n_notes:
        key = int(rng.randint(0, 88))
        head = int(rng.randint(0, n_steps - 12))
        tail = head + int(rng.randint(3, 30))
        if any(head <= b + 3 and a <= tail + 3 for a, b in busy.get(key, [])):
            continue
        busy.setdefault(key, []).append((head, tail))
        notes.append((head * hop, tail * hop, key + 21, int(rng.randint(1, 128))))
    label, velocity = paint_roll(np.array(notes), n_steps)
    return label, velocity


def test_ratio_table():
    assert sorted(augment.RATIOS) == SHIFTS and augment.RATIOS[0] == (1, 1) and augment.MAX_SHIFT == 6
    for k in SHIFTS:
        L, M = augment.RATIOS[k]
        assert 1 <= L <= 128 and 1 <= M <= 128 and math.gcd(L, M) == 1
        cents = 1200.0 * math.log2(M / L) - 100.0 * k
        assert abs(cents) < 2.0, (k, cents)
        assert abs(cents - augment.CENTS[k]) <= 1e-3, (k, cents)              # the committed error column is the true one
        assert augment.RATIOS[-k] == (M, L)
    assert max(abs(augment.CENTS[k]) for k in SHIFTS if abs(k) != 5) < 0.11


@pytest.mark.parametrize('k', SHIFTS)
def test_host_audio_is_the_resampler_definition(k):
    """Cropped at the track's first sample, the item is the head of resample_host(track, M, L): same filter, same sum."""
    from reconvat_amd.resample import resample_host
    L, M = augment.RATIOS[k]
    T = 30000
    track = np.random.RandomState(100 + k).randint(-32768, 32768, T).astype(np.int16)
    seq = -(-T * L // M) // HOP_LENGTH * HOP_LENGTH
    want = resample_host(track, M, L)[:seq]
    got = augment.shift_audio(track, 0, k, seq)
    assert got.dtype == np.float64 and got.shape == (seq,) == want.shape
    assert np.max(np.abs(got - want)) <= 1e-12


def test_host_audio_reads_the_track_around_the_crop_and_zero_beyond_it():
    """A crop in the middle equals the head-of-track result of the same track cut at the crop (plus what lies before it)."""
    k, seq, j0 = 3, 1024, 7
    L, M = augment.RATIOS[k]
    track = np.random.RandomState(3).randint(-32768, 32768, 20000).astype(np.int16)
    y = augment.shift_audio(track, j0 * HOP_LENGTH, k, seq)
    head_only = augment.shift_audio(track[j0 * HOP_LENGTH:], 0, k, seq)           # zero before the crop instead of the real samples
    assert np.max(np.abs(y[200:] - head_only[200:])) == 0 and np.max(np.abs(y[:50] - head_only[:50])) > 1e-4
    short = track[:j0 * HOP_LENGTH + 900]                                          # the track ends inside the crop's source span
    tail = augment.shift_audio(short, j0 * HOP_LENGTH, k, seq)
    reach = augment.filter64(k)[2] // L + 1                                        # source samples an output sees on either side
    assert np.all(tail[(900 + reach) * L // M + 1:] == 0) and np.any(tail[700:] != 0)
    assert np.max(np.abs(tail[:(900 - reach) * L // M] - y[:(900 - reach) * L // M])) == 0


@pytest.mark.parametrize('k', SHIFTS)
def test_host_labels(k):
    label, velocity = note_track(7)
    L, M = augment.RATIOS[k]
    j0, S = 11, 128
    assert j0 + augment.near(S - 1, L, M) + 3 < label.shape[0]
    item = augment.shift_item({'audio': np.zeros(300000, np.int16), 'label': label, 'velocity': velocity}, j0, k, S * HOP_LENGTH)
    code = item['label']
    assert code.shape == (S, 88) and code.dtype == np.uint8 and set(np.unique(code)) <= {0, 1, 2, 3}
    if k == 0:
        assert np.array_equal(code, label[j0:j0 + S])
        assert np.array_equal(item['velocity'], velocity[j0:j0 + S].astype(np.float32) / np.float32(128.0))
    # onsets: as many as there are source onset cells whose target frame and key land inside the item (none lost, none doubled)
    u, key = np.nonzero(label[j0:] == 3)
    t = (2 * u * L + M) // (2 * M)
    inside = (t < S) & (key + k >= 0) & (key + k < 88)
    cells = set(zip(t[inside].tolist(), (key[inside] + k).tolist()))
    assert {tuple(c) for c in np.argwhere(code == 3).tolist()} == cells
    assert int((code == 3).sum()) == int(inside.sum()) == len(cells) >= 10       # (onsets are one row long and never adjacent)
    assert int(item['onset'].sum()) == len(cells)
    assert np.all(item['frame'][code == 3] == 1)
    assert np.array_equal(item['onset'], (code == 3).astype(np.float32)) and np.array_equal(item['offset'], (code == 1).astype(np.float32))
    assert np.array_equal(item['frame'], (code > 1).astype(np.float32))
    # nothing outside the keys the keyboard maps to
    out_of_range = np.ones(88, dtype=bool)
    out_of_range[max(0, k):min(88, 88 + k)] = False
    for name in ('onset', 'offset', 'frame', 'velocity'):
        assert not item[name][:, out_of_range].any(), name
    assert not code[:, out_of_range].any()
    # the sounding state and the velocity are those of the nearest source row
    s = np.arange(S)
    at = j0 + (2 * s * M + L) // (2 * L)
    lo, hi = max(0, k), min(88, 88 + k)
    assert np.array_equal(item['velocity'][:, lo:hi], velocity[at, lo - k:hi - k].astype(np.float32) / np.float32(128.0))
    assert np.all(code[:, lo:hi][label[at, lo - k:hi - k] > 1] >= 2)


def test_host_labels_past_the_last_row_are_empty():
    label, velocity = note_track(9, n_steps=60, n_notes=30)
    label[-1, 40], velocity[-1, 40] = 2, 77
    item = augment.shift_item({'audio': np.zeros(60 * 512, np.int16), 'label': label, 'velocity': velocity}, 50, 0, 16 * HOP_LENGTH)
    assert np.array_equal(item['label'][:10], label[50:]) and not item['label'][10:].any() and not item['velocity'][10:].any()


def test_draws():
    lengths = np.array([70001, 90000, 81234, 65537], dtype=np.int64)
    order = [0, 3, 1, 1, 2, 0, 3, 2]
    seq = 16384
    # pitch_shift = 0: the crop stream exactly as the plain feed uses it, nothing drawn from the second stream
    steps, shifts = augment.draw_items(np.random.RandomState(42), None, lengths, order, seq, 0)
    rs = np.random.RandomState(42)
    want = [int(rs.randint(lengths[i] - seq)) // HOP_LENGTH for i in order]
    assert steps.tolist() == want and not shifts.any() and steps.dtype == np.int64
    # pitch_shift = p: k from the second stream, then the crop from the first over T - span(k)
    p = 6
    steps, shifts = augment.draw_items(np.random.RandomState(42), np.random.RandomState(5), lengths, order, seq, p)
    rs, aug = np.random.RandomState(42), np.random.RandomState(5)
    for n, i in enumerate(order):
        k = int(aug.randint(-p, p + 1))
        L, M = augment.RATIOS[k]
        span = -(-(-(-seq * M // L)) // HOP_LENGTH) * HOP_LENGTH + HOP_LENGTH
        assert span == augment.span(k, seq)
        assert (int(shifts[n]), int(steps[n])) == (k, int(rs.randint(lengths[i] - span)) // HOP_LENGTH)
        assert steps[n] * HOP_LENGTH + span < lengths[i]
    assert set(shifts.tolist()) <= set(SHIFTS) and len(set(shifts.tolist())) > 3
    assert augment.span(0, seq) == seq + HOP_LENGTH and augment.span(6, 2048) == 3584 and augment.span(-6, 2048) == 2048
    for bad in (-1, 7, 1.5):
        with pytest.raises(ValueError, match='pitch_shift'):
            augment.check_shift(bad)


def test_banks_are_the_resampler_banks():
    from reconvat_amd.resample import design_filter, polyphase_bank
    for k in SHIFTS:
        L, M, F, Kp, bank = augment.bank32(k)
        assert (L, M) == augment.RATIOS[k] and bank.shape == (L, Kp) and bank.dtype == np.float32 and Kp % 4 == 0 and Kp <= 256
        if k == 0:
            assert (F, Kp) == (0, 4) and bank.tolist() == [[1.0, 0.0, 0.0, 0.0]] and augment.taps(0) == 1
            continue
        gL, gM, half, h = design_filter(M, L)
        assert (gL, gM) == (L, M)
        assert np.array_equal(polyphase_bank(L, half, h)[2], bank)
        assert augment.taps(k) == -(-(2 * half + 1) // L)


def test_config_default_override_and_refusal():
    from reconvat_amd import cli
    for c in (cli.base_config({}, True), cli.base_config({}, False), cli.baseline_config({}), cli.thickstun_config({})):
        assert c['pitch_shift'] == 0 and type(c['pitch_shift']) is int and c['device_feed'] is True
    assert cli.base_config({'pitch_shift': 3}, True)['pitch_shift'] == 3
    for kw in ({'device_feed': False}, {'device': 'cpu'}):
        c = cli.base_config(dict(kw, pitch_shift=2, logdir='unused'), True)
        with pytest.raises(SystemExit, match='pitch_shift is an option of the device feed'):
            cli.run_training(True, **c)
    c = cli.base_config(dict(pitch_shift=7, logdir='unused'), True)
    with pytest.raises(SystemExit, match='pitch_shift must be a whole number of semitones in 0..6'):
        cli.run_training(True, **c)


@pytest.mark.parametrize('script', ['train_UNet_Onset_VAT.py', 'train_UNet_VAT.py', 'train_baseline_onset_frame_VAT.py',
                                    'train_baseline_Thickstun.py'])
def test_scripts_hand_the_key_to_run_training(script):
    src = open(os.path.join(ROOT, script)).read()
    sig = re.search(r'def train\((.*?)\):', src, flags=re.S).group(1)
    assert 'pitch_shift' in {a.strip() for a in sig.split(',')}


def test_header_and_ctypes_agree_on_the_entry_point():
    from reconvat_amd import _lib, feed
    text = open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+rv_crop_segments_shift\s*\(([^;]*?)\)\s*;', text, flags=re.S)
    assert m, 'rv_crop_segments_shift is not declared in include/reconvat_hip.h'
    ctype = {'float': _lib.F, 'long': _lib.L, 'int': _lib.I}
    want = [_lib.P if '*' in a else ctype[a.replace('const ', '').split()[0]] for a in (x.strip() for x in m.group(1).split(','))]
    assert _lib.SIGNATURES['rv_crop_segments_shift'] == (_lib.I, want)
    src = open(os.path.join(ROOT, 'reconvat_amd', 'csrc', 'data.hip')).read()
    assert int(re.search(r'#define RV_SHIFT_FIELDS (\d+)', src).group(1)) == feed.ITEM_FIELDS
