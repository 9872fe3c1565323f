"""Inputs shared by tests/test_threshold_sweep.py (no GPU) and tests/test_threshold_sweep_gpu.py: label rolls, "posteriorgrams"
and stub models for the threshold sweep.  Every function returns float32 [T, 88] arrays (onset_ref, frame_ref,
onset_pred, frame_pred)."""
import numpy as np
import torch

TILE = 64


def blank(T):
    return [np.zeros((T, 88), np.float32) for _ in range(4)]


def paint(onset, frame, pitch, start, end, level=1.0):
    """A note of the given level: the onset roll on its first frame, the frame roll on [start, end)."""
    onset[start, pitch] = level
    frame[start:end, pitch] = level


def random_rolls(T, seed, thresholds=(0.3, 0.5, 0.7), density=0.06):
    """Label notes; estimates derived from them (kept, moved by -1 .. 2 frames, ends moved by up to 6 frames, at a random level so
    that the thresholds cut some) plus false alarms, on noise in [0, 1] smoothed in time; a share of the values is then set EXACTLY
    to one of the thresholds, which `>` must leave off and `>=` would switch on."""
    rng = np.random.RandomState(seed)
    on_r, fr_r, on_p, fr_p = blank(T)
    for _ in range(max(2, int(T * 88 * density / 8))):
        t0, p, ln = rng.randint(0, T), rng.randint(0, 88), rng.randint(1, 25)
        paint(on_r, fr_r, p, t0, min(T, t0 + ln))
        if rng.rand() < 0.75:
            s = min(T - 1, max(0, t0 + rng.randint(-1, 3)))
            e = min(T, max(s + 1, t0 + ln + rng.randint(-6, 7)))
            paint(on_p, fr_p, p, s, e, rng.uniform(0.25, 1.0))
    for _ in range(max(1, int(T * 88 * density / 40))):
        t0, p = rng.randint(0, T), rng.randint(0, 88)
        paint(on_p, fr_p, p, t0, min(T, t0 + rng.randint(1, 12)), rng.uniform(0.25, 1.0))
    for roll in (on_p, fr_p):
        noise = rng.uniform(0, 0.6, size=(T + 2, 88)).astype(np.float32)
        roll[:] = np.clip(np.maximum(roll, 0.25 * noise[:-2] + 0.5 * noise[1:-1] + 0.25 * noise[2:]), 0, 1)
        exact = rng.rand(T, 88) < 0.03
        roll[exact] = rng.choice(np.asarray(thresholds, np.float32), size=int(exact.sum()))
    return on_r, fr_r, on_p, fr_p


def chain_rolls(T=200, seed=7):
    """Pitch 30: reference notes start on even frames and estimates on odd frames (every start within one frame of two starts of
    the other side: one long path per stretch); the frame rolls switch off at pseudo-random frames in between, which varies the note
    lengths so that the offset test removes a pseudo-random subset of the edges; a few starts are left out, which cuts the path
    into pieces of either parity.  Pitch 50: the same with the two sides swapped.  Three tiles and a bit."""
    rng = np.random.RandomState(seed)
    on_r, fr_r, on_p, fr_p = blank(T)
    for pitch, (on_even, fr_even, on_odd, fr_odd) in ((30, (on_r, fr_r, on_p, fr_p)), (50, (on_p, fr_p, on_r, fr_r))):
        for on, fr, first in ((on_even, fr_even, 2), (on_odd, fr_odd, 3)):
            for t in range(first, T - 2, 2):
                if rng.rand() < 0.93:
                    on[t, pitch] = 1
            fr[:, pitch] = (rng.rand(T) < 0.7).astype(np.float32)
    return on_r, fr_r, on_p, fr_p


def long_run_rolls(T):
    """Notes active across three whole tiles on both sides: one to the very end (T), one ending a frame before a tile edge."""
    on_r, fr_r, on_p, fr_p = blank(T)
    paint(on_r, fr_r, 10, 3, T)
    paint(on_p, fr_p, 10, 4, T)
    paint(on_r, fr_r, 11, 5, 4 * TILE - 1)
    paint(on_p, fr_p, 11, 5, 4 * TILE - 1)
    paint(on_r, fr_r, 12, TILE - 1, 4 * TILE - 1)                       # estimate one frame longer: up to the edge itself
    paint(on_p, fr_p, 12, TILE, 4 * TILE)
    return on_r, fr_r, on_p, fr_p


def offset_boundary_rolls(duration, delta, start=50, T=100):
    """One reference note of `duration` frames next to (or across) the first tile edge, and one estimate starting with it that ends `delta`
    frames later."""
    on_r, fr_r, on_p, fr_p = blank(T)
    paint(on_r, fr_r, 40, start, start + duration)
    paint(on_p, fr_p, 40, start, start + duration + delta)
    return on_r, fr_r, on_p, fr_p


class StubModel:
    """run_on_batch returns the fixed "posteriorgrams" stored with the song (and no losses)."""

    def run_on_batch(self, label, *args):
        return {'onset': label['pred_onset'].unsqueeze(0), 'frame': label['pred_frame'].unsqueeze(0)}, {}, None


def stub_songs(T, seeds, device='cpu'):
    songs = []
    for seed in seeds:
        on_r, fr_r, on_p, fr_p = (torch.from_numpy(x).to(device) for x in random_rolls(T, seed))
        songs.append({'path': f'stub/{seed}', 'onset': on_r, 'frame': fr_r, 'pred_onset': on_p, 'pred_frame': fr_p})
    return songs
