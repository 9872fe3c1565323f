"""Additive synthesiser: a note list rendered to audio, so that a corpus with true labels exists wherever this package
runs -- `train_on=Rendered` -- and a MIDI file can be listened to.  Sample rate 16 000 Hz.

Definition (everything here, `rv_synth_render` in csrc/synth.hip and the tests implement exactly this):

  row      a render is a sum of PARTIAL ROWS of eight 32-bit words, in this order:
               s, e      int      first sample and end sample of the note, e > s
               inc, ph   uint32   phase step per sample and start phase, in units of 2^-32 turn
               amp, dec  float32  amplitude and decay rate per sample, dec >= 0
               A, R      int      attack and release lengths in samples, both >= 1
           With t = n - s, for s <= n < e + R the row contributes  amp * att * decay * rel * osc:
               att   = min(t + 1, A) / A                    decay = exp(-dec t)
               rel   = 1 for n < e, else ((e + R - n) / R)^2
               osc   = sin(2 pi theta / 2^32),  theta = (ph + inc t) mod 2^32 in exact uint32 wrap-around arithmetic
           and nothing outside [s, e + R).
  output   y[n] = the sum over all rows in ascending row order; float32, or int16 = round-half-even of 32768 y, saturated.
  limits   `partials` enforces e + R - s <= 2^24 (t is exact in float32), 0 <= s and e + R < 2^31; anything else is a ValueError.
  timbre   Timbre(voice, seed): four draws from RandomState(seed), in this order:
               p = uniform(1, 2) spectral slope      even = uniform(0.3, 1) weight of the even partials
               scale = uniform(0.6, 1.4) decay scale cents = uniform(-10, 10) tuning offset
           voices:  'struck'    (piano, guqin)  A = 48, R = 1600, inharmonicity B = 2e-4 2^((m - 48) / 12),
                                dec_k = (1 + 0.3 (k - 1)) / (tau 16000), tau = scale 2.5 2^(-(m - 21) / 29) seconds, weight 1
                    'sustained' (bowed, blown)  A = 640, R = 1280, dec = 0, B = 0, weight `even` for even k, else 1
  partials note i = tsv row (onset s, offset s, MIDI note m, velocity):  s = rint(16000 onset), e = max(s + 1, rint(16000 offset)),
           f0 = 440 2^((m - 69) / 12 + cents / 1200); partials k = 1 .. K: f_k = k f0 sqrt(1 + B k^2) <= 7200 Hz and K <= 24;
               inc = rint(f_k / 16000 2^32) mod 2^32
               ph  = lowbias32(lowbias32(seed + 0x9E3779B9) ^ lowbias32(32 i + k)), all uint32 (lowbias32: reconvat_amd/acoustics.py)
               amp = float32(0.12 (velocity / 127) k^-p weight),   dec = float32(dec_k)
           rows in note order, k ascending, then sorted by s (stable).
  tiles    tile j = the absolute samples [1024 j, 1024 (j + 1)); `tile_lists` gives, per tile, the ascending list of the rows whose
           [s, e + R) meets it (CSR) -- what the kernel walks.

Not modelled: vibrato, noise components (hammer, bow, breath), the soundboard and any resonance between strings, the pedal, and
velocity-dependent timbre (velocity scales the amplitude alone).  This is audio with exact labels and pitched, decaying or
sustained partials -- not a piano.

`render_host` is the yardstick: the definition in float64.  `render` runs the kernel on a HIP device and the yardstick anywhere
else.  The kernel evaluates every term in float32 and sums in float64; with S[n] = sum amp att decay rel and E[n] = sum amp att rel
    |y - y64| <= 32 2^-24 S[n] + 2^-24 E[n]
(derived in tests/test_synth_gpu.py), so where 32768 times that bound is below 1 -- every corpus `prepare_VAT_dataset('Rendered')`
builds, tests/test_synth.py checks it -- the two paths agree to within 1 LSB as int16 (a sample whose exact value lies next to a
rounding boundary may fall on either side), the contract of the resampler.
"""
import numpy as np
import torch

from .acoustics import _lowbias32

SAMPLE_RATE = 16000
TILE = 1024
MAX_PARTIALS = 24
MAX_HZ = 7200.0
GAIN = 0.12
MAX_SPAN = 1 << 24
CHUNK = 1 << 22               # samples per kernel call, at most
VOICES = {'struck': dict(A=48, R=1600), 'sustained': dict(A=640, R=1280)}
OUT_DTYPES = {torch.float32: 0, torch.int16: 1}
# the columns of a row
S_, E_, INC, PH, AMP, DEC, A_, R_ = range(8)


class Timbre:
    """The per-track draws of a voice, from RandomState(seed) in the documented order."""

    def __init__(self, voice='struck', seed=0):
        if voice not in VOICES:
            raise ValueError(f'voice must be one of {", ".join(sorted(VOICES))} (got {voice!r})')
        self.voice, self.seed = voice, int(seed)
        rs = np.random.RandomState(self.seed)
        self.p = float(rs.uniform(1.0, 2.0))
        self.even = float(rs.uniform(0.3, 1.0))
        self.scale = float(rs.uniform(0.6, 1.4))
        self.cents = float(rs.uniform(-10.0, 10.0))

    def __repr__(self):
        return f'Timbre({self.voice!r}, {self.seed}: p={self.p:.3f}, even={self.even:.3f}, scale={self.scale:.3f}, cents={self.cents:+.2f})'


def partial_frequencies(notes, timbre):
    """(f [N, 24] float64, valid [N, 24] bool): f_k of every note and which of them are rendered (f_k <= 7200 Hz)."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    m = notes[:, 2:3]
    k = np.arange(1, MAX_PARTIALS + 1, dtype=np.float64)[None, :]
    f0 = 440.0 * 2.0 ** ((m - 69.0) / 12.0 + timbre.cents / 1200.0)
    B = 2e-4 * 2.0 ** ((m - 48.0) / 12.0) if timbre.voice == 'struck' else np.zeros_like(m)
    f = k * f0 * np.sqrt(1.0 + B * k * k)
    return f, f <= MAX_HZ


def partials(notes, timbre):
    """tsv rows (onset s, offset s, MIDI note, velocity) -> the partial rows uint32 [n_rows, 8], sorted by s."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    N = len(notes)
    voice = VOICES[timbre.voice]
    A, R = voice['A'], voice['R']
    s = np.rint(SAMPLE_RATE * notes[:, 0]).astype(np.int64)
    e = np.maximum(s + 1, np.rint(SAMPLE_RATE * notes[:, 1]).astype(np.int64))
    if N and (s.min() < 0 or (e + R).max() >= 1 << 31):
        raise ValueError(f'notes must start at or after 0 s and end (release included) before sample 2^31 (got samples {int(s.min())} .. {int((e + R).max())})')
    if N and (e + R - s).max() > MAX_SPAN:
        raise ValueError(f'a note of {int((e + R - s).max())} samples (release included): at most 2^24 = {MAX_SPAN}, about 17 minutes')
    f, valid = partial_frequencies(notes, timbre)
    k = np.arange(1, MAX_PARTIALS + 1, dtype=np.float64)[None, :]
    m, vel = notes[:, 2:3], notes[:, 3:4]
    if timbre.voice == 'struck':
        tau = timbre.scale * 2.5 * 2.0 ** (-(m - 21.0) / 29.0)
        dec = (1.0 + 0.3 * (k - 1.0)) / (tau * SAMPLE_RATE)
        weight = np.ones_like(k)
    else:
        dec = np.zeros_like(f)
        weight = np.where(k % 2 == 0, timbre.even, 1.0)
    amp = GAIN * (vel / 127.0) * k ** -timbre.p * weight
    inc = (np.rint(f / SAMPLE_RATE * 2.0 ** 32).astype(np.int64) % (1 << 32)).astype(np.uint32)
    with np.errstate(over='ignore'):
        i = np.arange(N, dtype=np.uint32)[:, None]
        ki = np.arange(1, MAX_PARTIALS + 1, dtype=np.uint32)[None, :]
        ph = _lowbias32(_lowbias32(np.uint32(timbre.seed & 0xFFFFFFFF) + np.uint32(0x9E3779B9)) ^ _lowbias32(np.uint32(32) * i + ki))
    rows = np.empty((N, MAX_PARTIALS, 8), dtype=np.uint32)
    rows[:, :, S_] = s[:, None].astype(np.int32).view(np.uint32)
    rows[:, :, E_] = e[:, None].astype(np.int32).view(np.uint32)
    rows[:, :, INC] = inc
    rows[:, :, PH] = ph
    rows[:, :, AMP] = (amp + np.zeros_like(f)).astype(np.float32).view(np.uint32)
    rows[:, :, DEC] = (dec + np.zeros_like(f)).astype(np.float32).view(np.uint32)
    rows[:, :, A_] = A
    rows[:, :, R_] = R
    rows = rows[valid]                                       # note order, k ascending
    return np.ascontiguousarray(rows[np.argsort(rows[:, S_].view(np.int32), kind='stable')])


def _fields(rows):
    rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1, 8)
    return (rows[:, S_].view(np.int32).astype(np.int64), rows[:, E_].view(np.int32).astype(np.int64), rows[:, INC].astype(np.int64),
            rows[:, PH].astype(np.int64), rows[:, AMP].view(np.float32).astype(np.float64), rows[:, DEC].view(np.float32).astype(np.float64),
            rows[:, A_].view(np.int32).astype(np.int64), rows[:, R_].view(np.int32).astype(np.int64))


def tile_lists(rows, n_tiles):
    """(tile_ptr int32 [n_tiles + 1], tile_rows int32 [nnz]): tile j lists, ascending, the rows whose [s, e + R) meets the samples
    [1024 j, 1024 (j + 1))."""
    s, e, _, _, _, _, _, R = _fields(rows)
    n_tiles = int(n_tiles)
    first = np.maximum(s, 0) // TILE
    last = np.minimum((e + R - 1) // TILE, n_tiles - 1)
    count = np.maximum(last - first + 1, 0)
    count[e + R <= 0] = 0
    row = np.repeat(np.arange(len(s), dtype=np.int64), count)
    start = np.cumsum(count) - count
    tile = np.arange(len(row), dtype=np.int64) - np.repeat(start, count) + np.repeat(first, count)
    order = np.argsort(tile, kind='stable')                  # `row` ascends already: it still does inside every tile
    tile_ptr = np.zeros(n_tiles + 1, dtype=np.int64)
    np.cumsum(np.bincount(tile, minlength=n_tiles)[:n_tiles], out=tile_ptr[1:])
    return tile_ptr.astype(np.int32), row[order].astype(np.int32)


def render_host(rows, n0, n_out, magnitude=False):
    """The yardstick: y[n0 .. n0 + n_out) of the definition in float64, the rows summed in ascending order.  `magnitude`: (S, E) with
    S[n] = sum amp att decay rel and E[n] = sum amp att rel, what the error bound is stated in."""
    n0, n_out = int(n0), int(n_out)
    y, E = np.zeros(n_out), np.zeros(n_out)
    for s, e, inc, ph, amp, dec, A, R in zip(*_fields(rows)):
        lo, hi = max(s, n0), min(e + R, n0 + n_out)
        if hi <= lo:
            continue
        n = np.arange(lo, hi, dtype=np.int64)
        t = n - s
        att = np.minimum(t + 1, A) / float(A)
        rel = np.where(n < e, 1.0, ((e + R - n) / float(R)) ** 2)
        env = amp * att * rel
        if magnitude:
            y[lo - n0:hi - n0] += env * np.exp(-dec * t)
            E[lo - n0:hi - n0] += env
        else:
            theta = (ph + inc * t) % (1 << 32)
            y[lo - n0:hi - n0] += env * np.exp(-dec * t) * np.sin(2.0 * np.pi * (theta / 2.0 ** 32))
    return (y, E) if magnitude else y


def to_int16(y):
    """round-half-even of 32768 y, saturated."""
    return np.clip(np.rint(np.asarray(y, dtype=np.float64) * 32768.0), -32768, 32767).astype(np.int16)


def error_bound(rows, n0, n_out):
    """32 2^-24 S[n] + 2^-24 E[n]: what the kernel's float32 output may differ from `render_host` by."""
    S, E = render_host(rows, n0, n_out, magnitude=True)
    return (32.0 * S + E) * 2.0 ** -24


def random_score(rng, seconds):
    """A seeded polyphonic note list, float64 [N, 4] tsv rows.  Events with exponential gaps of mean 0.25 s from 0.5 s up to
    `seconds` - 3; an event has 1 .. 4 notes (probabilities .5, .25, .15, .1) stacked by intervals from {3, 4, 5, 7, 8, 9, 12} on a
    root that follows a random walk (steps uniform in +-7) clipped to 33 .. 96; durations log-uniform in 0.08 .. 2 s, velocities in
    30 .. 120.  A note on a key that still sounds or releases (until its offset + 0.2 s) is dropped: no key carries overlapping notes."""
    notes, t, centre, busy = [], 0.5, 60.0, {}
    while True:
        t += rng.exponential(0.25)
        if t > seconds - 3.0:
            break
        n = int(rng.choice([1, 2, 3, 4], p=[.5, .25, .15, .1]))
        centre = float(np.clip(centre + rng.uniform(-7, 7), 33, 96))
        keys = [int(round(centre))]
        for _ in range(n - 1):
            keys.append(keys[-1] + int(rng.choice([3, 4, 5, 7, 8, 9, 12])))
        for m in keys:
            if not 21 <= m <= 108:
                continue
            d = float(np.exp(rng.uniform(np.log(0.08), np.log(2.0))))
            v = int(rng.randint(30, 121))
            if busy.get(m, -1.0) > t:
                continue
            busy[m] = t + d + 0.2
            notes.append((t, t + d, m, v))
    return np.array(notes, dtype=np.float64).reshape(-1, 4)


def _as_rows(notes_or_rows, timbre):
    a = np.asarray(notes_or_rows)
    if a.dtype == np.uint32 and a.ndim == 2 and a.shape[1] == 8:
        return np.ascontiguousarray(a)
    if timbre is None:
        raise ValueError('a note list needs a Timbre to become partial rows')
    return partials(a, timbre)


def render(notes_or_rows, n_samples, timbre=None, device='cpu', out_dtype=torch.int16):
    """Samples [0, n_samples) of a note list (tsv rows, with `timbre`) or of a table of partial rows (uint32 [n, 8]) as a tensor of
    `out_dtype` (torch.float32 or torch.int16) on `device`: `rv_synth_render` on a HIP device, in calls of at most 2^22 samples
    (the bits do not depend on the cuts), `render_host` on any other device."""
    if out_dtype not in OUT_DTYPES:
        raise ValueError(f'out_dtype {out_dtype}: expected torch.float32 or torch.int16')
    rows = _as_rows(notes_or_rows, timbre)
    n_samples = int(n_samples)
    if not 0 <= n_samples < (1 << 31) - TILE:
        raise ValueError(f'n_samples must lie in [0, 2^31 - {TILE}) (got {n_samples})')
    device = torch.device(device)
    if device.type != 'cuda':
        y = render_host(rows, 0, n_samples)
        return torch.from_numpy(to_int16(y) if out_dtype == torch.int16 else y.astype(np.float32)).to(device)
    from ._lib import call, ptr, stream
    n_tiles = -(-n_samples // TILE)
    tile_ptr, tile_rows = tile_lists(rows, n_tiles)
    y = torch.empty(n_samples, dtype=out_dtype, device=device)
    with torch.cuda.device(device):
        d_rows = torch.from_numpy(rows.view(np.int32).reshape(-1)).to(device)
        d_ptr, d_list = torch.from_numpy(tile_ptr).to(device), torch.from_numpy(tile_rows).to(device)
        for n0 in range(0, n_samples, CHUNK):
            call('rv_synth_render', ptr(d_rows) if len(rows) else None, len(rows), ptr(d_ptr), ptr(d_list) if len(tile_rows) else None,
                 n_tiles, n0, min(CHUNK, n_samples - n0), y.data_ptr() + n0 * y.element_size(), OUT_DTYPES[out_dtype], stream())
    return y
