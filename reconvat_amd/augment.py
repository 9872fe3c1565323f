"""Pitch-shift augmentation of the device feed: every training item is its crop transposed by a whole number of
semitones k, |k| <= 6 -- the audio resampled, the labels moved k keys and rescaled in time by the same rational factor.

Definition (everything here, `rv_crop_segments_shift` in csrc/data.hip and reconvat_amd/feed.py implement exactly this):

  ratio    a shift by k semitones plays the source faster by M/L ~ 2^(k/12): output sample m sits at source position m M / L.
           RATIOS[k] = (L, M), both terms <= 128 (table below); -k swaps the two numbers, 0 is 1/1.
  audio    resample.py's filter unchanged, h = design_filter(M, L) (ZEROS, ROLLOFF, BETA of that module), and for an item cropped at
           track sample a0 = j0 * 512:   y[m] = sum_n x[a0 + n] 2^-15 h[m M - n L],   m = 0 .. seq_len - 1.
           The sum runs over every n with a0 + n inside the track: samples before a0 and after the crop are the track's own,
           samples beyond the track's two ends are zero.  k = 0 is the one-tap filter [1.0]: the plain crop, bit for bit.
  labels   S = seq_len / 512 output frames, source rows counted from j0 (a row past the track's last one is empty):
               near(s) = (2 s M + L) // (2 L)      the source row nearest to output frame s
               tgt(u)  = (2 u L + M) // (2 M)      the output frame nearest to source row u
           output key c reads source key c - k (outside [0, 88): 0).  The code at (s, c) is the first that applies of
               3  if some u with tgt(u) == s holds 3          (onset:  a one-frame event, carried FORWARD to its nearest frame)
               2  if roll[j0 + near(s)] > 1                   (sounding: a state, looked up BACKWARD at the nearest row)
               1  if some u with tgt(u) == s holds 1          (offset: an event, carried forward)
               0  otherwise
           so that events are neither lost when M > L (several rows per frame) nor doubled when M < L (several frames per row).
           velocity[s][c] = velocity[j0 + near(s)][c - k].  onset / offset / frame are code == 3 / == 1 / > 1 as in the plain crop.
  draws    a second stream RandomState(aug_seed): per item, in item order, k = aug.randint(-p, p + 1), then the crop from the crop
           stream as randint(T - span(k)) // 512, span(k) = ceil(seq_len M / L) rounded up to whole hops, plus one hop.

`shift_item` is the host yardstick (float64, unrounded filter): the only path without a GPU, and what the tests compare with.
"""
import math

import numpy as np

from .constants import HOP_LENGTH
from . import resample

MAX_SHIFT = 6
# k: (L, M, error in cents of M/L against 2^(k/12)); the best approximations with both terms <= 128
_UP = {
    1: (101, 107, -0.093),
    2: (49, 55, -0.020),
    3: (37, 44, -0.026),
    4: (50, 63, +0.108),
    5: (3, 4, -1.955),
    6: (70, 99, +0.088),
}
RATIOS = {0: (1, 1)}
CENTS = {0: 0.0}
for _k, (_l, _m, _c) in _UP.items():
    RATIOS[_k], RATIOS[-_k] = (_l, _m), (_m, _l)
    CENTS[_k], CENTS[-_k] = _c, -_c


def check_shift(pitch_shift):
    p = int(pitch_shift)
    if p != pitch_shift or not 0 <= p <= MAX_SHIFT:
        raise ValueError(f'pitch_shift must be a whole number of semitones in 0..{MAX_SHIFT} (got {pitch_shift!r})')
    return p


def span(k, sequence_length):
    """Source samples a draw reserves for an item shifted by k: ceil(seq_len M / L) rounded up to whole hops, plus one hop."""
    L, M = RATIOS[k]
    need = -(-int(sequence_length) * M // L)
    return -(-need // HOP_LENGTH) * HOP_LENGTH + HOP_LENGTH


def near(s, L, M):
    return (2 * s * M + L) // (2 * L)


def tgt(u, L, M):
    return (2 * u * L + M) // (2 * M)


def filter64(k):
    """(L, M, half, h float64): the unrounded filter of shift k; k = 0 is the single tap 1.0."""
    L, M = RATIOS[k]
    if k == 0:
        return 1, 1, 0, np.ones(1)
    return resample._design64(M, L, resample.ZEROS, resample.ROLLOFF, resample.BETA)


def bank32(k):
    """(L, M, F, Kp, bank float32 [L, Kp]) in the layout of resample.polyphase_bank; k = 0: F = 0 and the row [1, 0, 0, 0]."""
    L, M = RATIOS[k]
    if k == 0:
        return 1, 1, 0, 4, np.array([[1.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    L, M, half, h = resample.design_filter(M, L)
    F, Kp, bank = resample.polyphase_bank(L, half, h)
    return L, M, F, Kp, bank


def taps(k):
    """Non-zero taps of one output, at most: the K of the float32 error bound (K + 8) 2^-24 sum |x| |h|."""
    L, _, half, _ = filter64(k)
    return -(-(2 * half + 1) // L)


def shift_audio(audio, a0, k, sequence_length, magnitude=False):
    """y[m] = sum_n x[a0 + n] 2^-15 h[m M - n L] in float64 over the whole track `audio` (int16 [T]); `magnitude`: sum |x| |h|."""
    L, M, half, h = filter64(k)
    x = np.asarray(audio).astype(np.float64) * 2.0 ** -15
    if magnitude:
        x, h = np.abs(x), np.abs(h)
    T, a0, n_out = len(x), int(a0), int(sequence_length)
    y = np.zeros(n_out)
    reach = half // L + 1
    for m0 in range(0, n_out, 8192):
        m = np.arange(m0, min(n_out, m0 + 8192), dtype=np.int64)
        # every n with |m M - n L| <= half lies in [m M // L - reach, m M // L + reach]
        n = (m * M // L)[:, None] + np.arange(-reach, reach + 1, dtype=np.int64)[None, :]
        lag = m[:, None] * M - n * L
        ok = (np.abs(lag) <= half) & (a0 + n >= 0) & (a0 + n < T)
        c = np.where(ok, h[np.clip(lag + half, 0, 2 * half)], 0.0)
        y[m0:m0 + len(m)] = np.sum(c * x[np.clip(a0 + n, 0, T - 1)], axis=1)
    return y


def shift_labels(label, velocity, j0, k, n_steps):
    """(code uint8 [n_steps, keys], velocity uint8 [n_steps, keys]) of the item that starts at source row j0, by the rule above."""
    L, M = RATIOS[k]
    label, velocity = np.asarray(label), np.asarray(velocity)
    rows, keys = label.shape[0] - int(j0), label.shape[1]
    # the source window of the item, moved k keys (columns shifted in from outside the keyboard are empty)
    n_src = near(n_steps - 1, L, M) + 2 + M // L
    src = np.zeros((n_src, keys), dtype=np.uint8)
    vel = np.zeros((n_src, keys), dtype=np.uint8)
    have = max(0, min(n_src, rows))
    lo, hi = max(0, k), min(keys, keys + k)
    src[:have, lo:hi] = label[j0:j0 + have, lo - k:hi - k]
    vel[:have, lo:hi] = velocity[j0:j0 + have, lo - k:hi - k]
    u = np.arange(n_src)
    t = tgt(u, L, M)
    keep = t < n_steps
    onset = np.zeros((n_steps, keys), dtype=bool)
    offset = np.zeros((n_steps, keys), dtype=bool)
    np.logical_or.at(onset, t[keep], src[keep] == 3)
    np.logical_or.at(offset, t[keep], src[keep] == 1)
    at = near(np.arange(n_steps), L, M)
    code = np.where(onset, 3, np.where(src[at] > 1, 2, np.where(offset, 1, 0))).astype(np.uint8)
    return code, vel[at]


def shift_item(track, j0, k, sequence_length):
    """The host yardstick: the item of `track` (dict with int16 'audio' [T], uint8 'label' / 'velocity' [rows, 88]) that starts at
    source row j0, transposed by k semitones -- float64 audio with the unrounded filter, float32 label tensors."""
    if sequence_length % HOP_LENGTH:
        raise ValueError('sequence_length must be a multiple of HOP_LENGTH (512)')
    n_steps = sequence_length // HOP_LENGTH
    code, vel = shift_labels(track['label'], track['velocity'], j0, k, n_steps)
    return {'audio': shift_audio(track['audio'], int(j0) * HOP_LENGTH, k, sequence_length), 'label': code,
            'onset': (code == 3).astype(np.float32), 'offset': (code == 1).astype(np.float32),
            'frame': (code > 1).astype(np.float32), 'velocity': vel.astype(np.float32) * np.float32(1.0 / 128.0), 'shift': int(k)}


def draw_items(random, aug, lengths, indices, sequence_length, pitch_shift):
    """Crop rows and shifts of the given items, in item order: (steps [B], shifts [B]) int64.  pitch_shift = 0 draws nothing from
    `aug` and the crop exactly as the plain feed does (randint(T - seq_len) // 512)."""
    steps, shifts = [], []
    for i in indices:
        k = int(aug.randint(-pitch_shift, pitch_shift + 1)) if pitch_shift else 0
        reserve = span(k, sequence_length) if pitch_shift else sequence_length
        steps.append(int(random.randint(lengths[i] - reserve)) // HOP_LENGTH)
        shifts.append(k)
    return np.array(steps, dtype=np.int64), np.array(shifts, dtype=np.int64)


def table_cents():
    """{k: error in cents of M/L against 2^(k/12)} computed from RATIOS (the committed CENTS are these, rounded)."""
    return {k: 1200.0 * math.log2(M / L) - 100.0 * k for k, (L, M) in RATIOS.items()}
