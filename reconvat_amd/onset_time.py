"""Sub-frame note onsets: the decoders return onsets on the 32 ms frame grid; this module moves each one to the sample at
which the note's own harmonics rise most steeply in the audio.

This module is the definition and runs without a GPU; csrc/onset_time.hip (`rv_onset_refine`) computes the same on the device and the
tests hold the kernel to what is written here.  Sample rate 16 000 Hz, HOP = 512.

    inputs     audio float32 [T], zero outside [0, T); per note a key p in 0..87 and an onset frame t >= 0
    harmonics  f0(p) = 440 * 2^((p + 21 - 69) / 12) (velocity.key_frequencies); q = 1..8, valid iff q f0 <= 7200; V(p) >= 1 of them
    window     w[n] = 0.5 - 0.5 cos(2 pi (n + 0.5) / 512),  n = 0..511
    table      tab[p, q, 0, n] = w[n] cos(2 pi q f0 n / 16000),  tab[p, q, 1, n] = -w[n] sin(2 pi q f0 n / 16000): float64, rounded ONCE
               to float32.  The rounded values are the definition; the host path uses them in float64 arithmetic.
    search     c = 512 t;  positions u_m = c - 768 + 32 m, m = 0..48;  window m covers the samples u_m - 256 + n
    amplitude  A[m, q] = sqrt(re^2 + im^2),  re = sum_n tab[p, q, 0, n] x[u_m - 256 + n],  im likewise with tab[p, q, 1, n]
    rise       d[m, q] = A[m + 1, q] - A[m - 1, q],  m = 1..47
    vote       k_q = the first m that maximises d[., q];  k = the lower median of k_q over the valid harmonics (sorted, index (V - 1) // 2)
    onset      sample clamp(u_k - lead, 0, T - 1); `lead` >= 0 samples, default 0

u_k is the time of steepest rise.  For a percussive attack that is the onset to within a few milliseconds; for a slow attack it is the
middle of the attack, which is what `lead` is for.  The audio is taken to be finite.
"""
import numpy as np
import torch

from .constants import HOP_LENGTH, SAMPLE_RATE
from .velocity import N_HARMONICS, N_KEYS, key_frequencies

WINDOW = 512
STEP = 32
N_POS = 49                                  # search positions: +-768 samples around the frame's first sample
SPAN = WINDOW + STEP * (N_POS - 1)          # 2048: the samples one note looks at, from c - 1024
BACK = SPAN // 2                            # the first of them is c - 1024
MAX_HZ = 7200.0
MAX_FRAME = (1 << 22) - 1                   # 512 t + 1024 stays far inside int32
assert HOP_LENGTH == 512 and SAMPLE_RATE == 16000

_TABLE = []
_DEVICE_TABLES = {}


def valid_harmonics():
    """int64 [88]: V(p), the number of harmonics q = 1..V with q f0(p) <= 7200 Hz (they are a prefix)."""
    f = key_frequencies()[:, None] * np.arange(1, N_HARMONICS + 1, dtype=np.float64)[None, :]
    return (f <= MAX_HZ).sum(axis=1).astype(np.int64)


def window():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(WINDOW, dtype=np.float64) + 0.5) / WINDOW)


def basis_table():
    """float32 [88, 8, 2, 512], built once."""
    if not _TABLE:
        n = np.arange(WINDOW, dtype=np.float64)
        f = key_frequencies()[:, None] * np.arange(1, N_HARMONICS + 1, dtype=np.float64)[None, :]
        arg = 2.0 * np.pi * f[:, :, None] * n[None, None, :] / SAMPLE_RATE
        tab = np.stack([window() * np.cos(arg), -window() * np.sin(arg)], axis=2)
        tab = tab.astype(np.float32)
        tab.setflags(write=False)
        _TABLE.append(tab)
    return _TABLE[0]


def _host_audio(audio):
    if torch.is_tensor(audio):
        audio = audio.detach().cpu().numpy()
    audio = np.asarray(audio)
    if audio.ndim != 1 or audio.dtype != np.float32:
        raise ValueError(f'audio must be float32 [T], got {audio.dtype} {audio.shape}')
    if not 1 <= len(audio) < (1 << 31):
        raise ValueError(f'audio of {len(audio)} samples: 1 .. 2^31 - 1 expected')
    return audio


def _notes(keys, frames):
    keys, frames = np.asarray(keys, dtype=np.int64).reshape(-1), np.asarray(frames, dtype=np.int64).reshape(-1)
    if keys.shape != frames.shape:
        raise ValueError(f'{len(keys)} keys for {len(frames)} onset frames')
    if len(keys) and not (0 <= keys.min() and keys.max() < N_KEYS):
        raise ValueError(f'keys must lie in 0..{N_KEYS - 1} (got {int(keys.min())} .. {int(keys.max())})')
    if len(frames) and not (0 <= frames.min() and frames.max() <= MAX_FRAME):
        raise ValueError(f'onset frames must lie in 0..{MAX_FRAME} (got {int(frames.min())} .. {int(frames.max())})')
    return keys, frames


def _lead(lead):
    if int(lead) != lead or not 0 <= int(lead) < (1 << 30):
        raise ValueError(f'lead must be an int number of samples in [0, 2^30), got {lead!r}')
    return int(lead)


def windows(audio, frames):
    """float64 [n, 2048]: the samples c - 1024 .. c + 1023 of every note, zero outside [0, T)."""
    audio = _host_audio(audio)
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    idx = (HOP_LENGTH * frames - BACK)[:, None] + np.arange(SPAN, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < len(audio))
    return np.where(inside, audio[np.where(inside, idx, 0)].astype(np.float64), 0.0)


def _products(audio, keys, frames, magnitude=False):
    """(re, im) float64 [n, 49, 8] each; `magnitude`: sum_n |tab| |x| in their place, what the device's error bound is stated in."""
    keys, frames = _notes(keys, frames)
    tab = basis_table()
    win = windows(audio, frames)
    out = np.zeros((2, len(keys), N_POS, N_HARMONICS))
    for i, p in enumerate(keys):
        X = np.lib.stride_tricks.sliding_window_view(win[i], WINDOW)[::STEP]                # [49, 512]
        B = tab[p].reshape(2 * N_HARMONICS, WINDOW).astype(np.float64)                      # rows: (q, re / im)
        D = (np.abs(X) @ np.abs(B).T) if magnitude else (X @ B.T)
        out[:, i] = D.reshape(N_POS, N_HARMONICS, 2).transpose(2, 0, 1)
    return out[0], out[1]


def amplitudes(audio, keys, frames):
    """A float64 [n, 49, 8]; 0 for the invalid harmonics of a key."""
    keys, frames = _notes(keys, frames)
    re, im = _products(audio, keys, frames)
    A = np.sqrt(re * re + im * im)
    A[np.broadcast_to((np.arange(N_HARMONICS)[None, :] >= valid_harmonics()[keys][:, None])[:, None, :], A.shape)] = 0.0
    return A


def rises(A):
    """d [n, 47, 8]: row i is m = i + 1."""
    return A[:, 2:, :] - A[:, :-2, :]


def pick(A, keys):
    """k int64 [n]: per harmonic the first m in 1..47 with the largest rise, then the lower median over the key's valid harmonics."""
    A = np.asarray(A)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1)
    if A.shape != (len(keys), N_POS, N_HARMONICS):
        raise ValueError(f'A of shape {A.shape} for {len(keys)} notes')
    kq = rises(A).argmax(axis=1) + 1                                                        # argmax: the first of equal values
    V = valid_harmonics()[keys]
    kq = np.where(np.arange(N_HARMONICS)[None, :] < V[:, None], kq, N_POS)                  # the invalid ones sort to the end
    return np.take_along_axis(np.sort(kq, axis=1), ((V - 1) // 2)[:, None], axis=1).reshape(-1) if len(keys) else np.zeros(0, np.int64)


def _samples(k, frames, lead, T):
    return np.clip(HOP_LENGTH * frames - (WINDOW + WINDOW // 2) + STEP * k - lead, 0, T - 1).astype(np.int64)


def refine_host(audio, keys, frames, lead=0):
    """int64 [n]: the refined onset samples, by the definition in float64."""
    audio, lead = _host_audio(audio), _lead(lead)
    keys, frames = _notes(keys, frames)
    return _samples(pick(amplitudes(audio, keys, frames), keys), frames, lead, len(audio))


def device_table(device):
    """The basis table on a HIP device, uploaded once per device."""
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('reconvat_amd ops run on a HIP device only; there is no CPU fallback')
    index = device.index if device.index is not None else torch.cuda.current_device()
    if index not in _DEVICE_TABLES:
        _DEVICE_TABLES[index] = torch.from_numpy(np.array(basis_table())).to(torch.device('cuda', index))
    return _DEVICE_TABLES[index]


def refine_device(audio, keys, frames, lead=0, return_amplitudes=False):
    """`rv_onset_refine` on a float32 [T] tensor on a HIP device: the refined samples as an int32 [n] tensor on that device (and, with
    `return_amplitudes`, the kernel's A as float32 [n, 49, 8]).  One launch per 2^20 notes, no synchronisation; the keys and frames
    are checked here and uploaded."""
    from . import _lib
    if not torch.is_tensor(audio):
        raise TypeError('refine_device: a tensor on a HIP device expected')
    _lib.need_gpu(audio)
    if audio.dim() != 1 or audio.dtype != torch.float32:
        raise ValueError(f'audio must be float32 [T], got {audio.dtype} {tuple(audio.shape)}')
    if not 1 <= audio.numel() < (1 << 31):
        raise ValueError(f'audio of {audio.numel()} samples: 1 .. 2^31 - 1 expected')
    lead = _lead(lead)
    keys, frames = _notes(keys, frames)
    n, dev = len(keys), audio.device
    audio = audio if audio.is_contiguous() else audio.contiguous()
    with torch.cuda.device(dev):
        out = torch.empty(n, dtype=torch.int32, device=dev)
        amp = torch.empty((n, N_POS, N_HARMONICS), dtype=torch.float32, device=dev) if return_amplitudes else None
        if n:
            notes = torch.from_numpy(np.stack([keys, frames], axis=1).astype(np.int32)).to(dev)
            _lib.call('rv_onset_refine', audio.data_ptr(), audio.numel(), device_table(dev).data_ptr(), notes.data_ptr(), n, lead,
                      out.data_ptr(), _lib.ptr(amp), _lib.stream())
    return (out, amp) if return_amplitudes else out


def refine(audio, keys, frames, lead=0):
    """int64 [n] (NumPy): the kernel for a tensor on a HIP device, the host path for anything else."""
    if torch.is_tensor(audio) and audio.is_cuda:
        return refine_device(audio, keys, frames, lead).cpu().numpy().astype(np.int64)
    return refine_host(audio, keys, frames, lead)


def refine_intervals(audio, pitches, intervals, lead=0, device=False):
    """A decoder's (pitches 0..87, intervals in frames [n, 2]) -> intervals in SECONDS, float64 [n, 2], in the same order.

    onset    the refined sample / 16000 (`device`: by the kernel, `audio` on a HIP device; else by the host path)
    offset   frame * 512 / 16000, raised to onset + 512 / 16000 where the refined onset would reach it
    per key  in onset order, an onset is never earlier than the previous note's offset on that key
    The post-processing is host NumPy on either path."""
    pitches = np.asarray(pitches, dtype=np.int64).reshape(-1)
    intervals = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    if len(pitches) != len(intervals):
        raise ValueError(f'{len(pitches)} pitches for {len(intervals)} intervals')
    if device:
        samples = refine_device(audio, pitches, intervals[:, 0], lead).cpu().numpy().astype(np.int64)
    else:
        samples = refine_host(audio, pitches, intervals[:, 0], lead)
    hop = HOP_LENGTH / SAMPLE_RATE
    out = np.stack([samples / float(SAMPLE_RATE), intervals[:, 1] * hop], axis=1).reshape(-1, 2)
    for p in np.unique(pitches):
        idx = np.flatnonzero(pitches == p)
        idx = idx[np.argsort(intervals[idx, 0], kind='stable')]
        end = 0.0
        for i in idx:
            out[i, 0] = max(out[i, 0], end)
            if out[i, 1] <= out[i, 0]:
                out[i, 1] = out[i, 0] + hop
            end = out[i, 1]
    return out
