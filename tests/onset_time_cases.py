"""Inputs and bounds shared by tests/test_onset_time.py and tests/test_onset_time_gpu.py (reconvat_amd/onset_time.py).

The error bound of the kernel's amplitudes, derived from the definition and from how the kernel adds (u = 2^-24, S = sum_n |tab| |x| of a
component), in the way tests/test_synth_gpu.py derives its bound -- terms in float32, their sum in float64:

  * a component (re or im) is 128 groups of four products; a group is added in float32 from zero, each step one rounding (fused) or two
    (unfused), in any order of the four, and the 128 group values are added in float64:
        |re' - re| <= (g + 2^-45) S_re,   g = 4 u / (1 - 4 u);
    the host's own float64 sum of the 512 exact products is within 512 2^-53 S = 2^-44 S of the true value: (g + 2^-43) S covers both;
  * A' = fl32(sqrt(re'^2 + im'^2)) with the squares, their sum and the root in float64 (relative 2^-50 at most) and ONE rounding to
    float32: |A' - hypot(re', im')| <= (u + 2^-50) hypot(re', im'), and |hypot(re', im') - hypot(re, im)| <= |re' - re| + |im' - im|;
    a float32 product that falls below the normal range adds at most 2^-149 per step: 2^-70 covers all of them;
  * the rise d = A[m + 1] - A[m - 1] is rounded once more in float32, by at most u max(A[m + 1], A[m - 1]): one more u A in each
    amplitude's bound covers it, so that two rises compare as in the definition whenever they differ by more than FOUR bounds.

        bound[m, q] = (1 + 2 u) (g + 2^-43) (S_re + S_im) + (2 u + 2^-50) A + 2^-70
"""
import functools

import numpy as np

from reconvat_amd import onset_time as ot, synth

U = 2.0 ** -24
G = 4 * U / (1 - 4 * U)
SR, HOP = 16000, 512


@functools.lru_cache(maxsize=None)
def rendered(voice, seed, seconds):
    """(audio float32 [seconds * 16000] from the int16 render of `render_host`, the score's tsv rows) -- read-only."""
    notes = synth.random_score(np.random.RandomState(seed), seconds)
    pcm = synth.to_int16(synth.render_host(synth.partials(notes, synth.Timbre(voice, seed)), 0, seconds * SR))
    audio = pcm.astype(np.float32) / np.float32(32768.0)
    audio.setflags(write=False)
    notes.setflags(write=False)
    return audio, notes


def true_notes(notes, shift=0):
    """(keys, onset frames of a perfect decoder, moved by `shift` frames)"""
    return notes[:, 2].astype(np.int64) - 21, np.maximum(np.rint(notes[:, 0] * SR / HOP).astype(np.int64) + shift, 0)


def onset_errors_ms(audio, notes, shift=0, lead=0):
    """(|grid onset - true onset|, |refined onset - true onset|) per note, in ms"""
    keys, frames = true_notes(notes, shift)
    refined = ot.refine_host(audio, keys, frames, lead)
    return np.abs(frames * HOP / SR - notes[:, 0]) * 1e3, np.abs(refined / SR - notes[:, 0]) * 1e3


def amp_bound(audio, keys, frames):
    """(A float64 [n, 49, 8] of the definition, bound [n, 49, 8]) -- see the module docstring."""
    A = ot.amplitudes(audio, keys, frames)
    s_re, s_im = ot._products(audio, keys, frames, magnitude=True)
    return A, (1 + 2 * U) * (G + 2.0 ** -43) * (s_re + s_im) + (2 * U + 2.0 ** -50) * A + 2.0 ** -70


def safe_notes(A, bound, keys):
    """bool [n]: for every valid harmonic the largest rise exceeds every other rise by more than four times the harmonic's largest bound."""
    d = ot.rises(A)                                                     # [n, 47, 8]
    top2 = np.sort(d, axis=1)[:, -2:, :]                                # second largest, largest
    margin = top2[:, 1, :] - top2[:, 0, :]
    ok = margin > 4.0 * bound.max(axis=1)
    valid = np.arange(8)[None, :] < ot.valid_harmonics()[np.asarray(keys)][:, None]
    return np.all(ok | ~valid, axis=1)


PARITY_SEED = 0


@functools.lru_cache(maxsize=None)
def parity_input():
    """The input of the parity test: the 8 s 'struck' seed-0 render with its true notes, then hand-placed notes: frame 0, the last
    frame (249: the one frame of the track whose windows pass T = 128000), keys 0 and 87.  -> (audio, keys, frames)
    Frame 0 and the last frame lie in silence: every rise is 0 there, a tie that no bound can make safe."""
    audio, notes = rendered('struck', PARITY_SEED, 8)
    keys, frames = true_notes(notes)
    last = (len(audio) - 1) // HOP
    mid = int(frames[len(frames) // 2])
    hand = [(int(keys[0]), 0), (int(keys[-1]), last), (0, mid), (87, mid)]
    keys = np.concatenate([keys, [k for k, _ in hand]]).astype(np.int64)
    frames = np.concatenate([frames, [t for _, t in hand]]).astype(np.int64)
    return audio, keys, frames


@functools.lru_cache(maxsize=None)
def parity_reference():
    """(A, bound, safe, samples at lead 0) of `parity_input`, computed once"""
    audio, keys, frames = parity_input()
    A, bound = amp_bound(audio, keys, frames)
    return A, bound, safe_notes(A, bound, keys), ot.refine_host(audio, keys, frames)
