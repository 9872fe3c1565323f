"""Sample-rate conversion on ingest, host side: the filter design, the float64 host path and the dataset entry points
against an oracle written HERE from the definition -- it shares no code with reconvat_amd/resample.py:

    g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, q = max(L, M), half = 64 q
    h[i] = L (rho / q) sinc(rho i / q) kaiser(2 half + 1, beta)[i + half]
    y[m] = sum_n x[n] h[m M - n L] = upfirdn(h, x, L, 1)[half::M][:ceil(T L / M)]          (float64)

tests/test_resample_gpu.py imports the oracle and the error bound from this file.
"""
import functools
import math
import os
import wave

import numpy as np
import pytest
import torch
from scipy.signal import upfirdn

RATES = [44100, 48000, 22050, 32000, 8000, 96000, 11025, 44056]
SR_OUT = 16000
Z, RHO, BETA = 64, 0.9475937167399596, 14.769656459379492


@functools.lru_cache(maxsize=None)
def oracle_filter(sr_in, sr_out=SR_OUT):
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    q = max(L, M)
    half = Z * q
    i = np.arange(-half, half + 1, dtype=np.float64)
    h = L * (RHO / q) * np.sinc(RHO * i / q) * np.kaiser(2 * half + 1, BETA)
    return L, M, half, h


def mono64(x):
    """Interleaved frames [T] / [T, C] of int16, int32 or float -> float64 mono in [-1, 1)."""
    x = np.asarray(x)
    scale = {np.dtype(np.int16): 2.0 ** -15, np.dtype(np.int32): 2.0 ** -31}.get(x.dtype, 1.0)
    x = x.astype(np.float64) * scale
    return x if x.ndim == 1 else x.mean(axis=1)


def oracle(x, sr_in, sr_out=SR_OUT, bound=True):
    """(y64, S, K): the definition in float64, S[m] = sum_n |x[n]| |h[m M - n L]| (None without `bound`) and the taps per output K."""
    L, M, half, h = oracle_filter(sr_in, sr_out)
    x = mono64(x)
    n_out = -(-len(x) * L // M)
    y = upfirdn(h, x, L, 1)[half::M][:n_out]
    S = upfirdn(np.abs(h), np.abs(x), L, 1)[half::M][:n_out] if bound else None
    assert len(y) == n_out
    return y, S, -(-(2 * half + 1) // L)


def f32_bound(S, K):
    """|y - y64| of a length-K float32 dot product summed in any order, with or without FMA, plus the float32 rounding of the
    coefficients and of the downmix: (K + 8) 2^-24 S."""
    return (K + 8) * 2.0 ** -24 * S


def int16_bound(S, K):
    return 0.5 + 32768.0 * f32_bound(S, K)


def signal(kind, T, sr, seed=0):
    """Float64 mono test signals in [-1, 1]."""
    t = np.arange(T) / sr
    if kind == 'noise':
        return np.random.RandomState(seed).uniform(-1.0, 1.0, T)
    if kind == 'tones':
        return 0.45 * np.sin(2 * np.pi * 440.0 * t) + 0.45 * np.sin(2 * np.pi * 3520.0 * t + 0.3)
    if kind == 'square':
        return np.where(np.sin(2 * np.pi * 220.0 * t) >= 0, 1.0, -1.0)
    raise KeyError(kind)


def as_dtype(x, dtype, channels):
    """Mono float64 signal -> [T] / [T, C] frames of `dtype` whose channel mean is (close to) the signal: channel c carries the
    signal times a gain, the gains average to one."""
    if channels > 1:
        gains = np.linspace(0.5, 1.5, channels)
        x = np.clip(x[:, None] * gains[None, :], -1.0, 1.0)
    if dtype == np.int16:
        return np.clip(np.rint(x * 32767.0), -32768, 32767).astype(np.int16)
    if dtype == np.int32:
        return (np.clip(np.rint(x * 8388607.0), -8388608, 8388607).astype(np.int64) << 8).astype(np.int32)       # 24-bit, left justified
    return x.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sr', RATES)
def test_design_filter_matches_the_formula(sr):
    from reconvat_amd.resample import design_filter
    L, M, half, h = oracle_filter(sr)
    gL, gM, ghalf, gh = design_filter(sr, SR_OUT)
    assert (gL, gM, ghalf) == (L, M, half)
    assert gh.dtype == np.float32 and gh.shape == (2 * half + 1,)
    assert np.all(np.abs(gh.astype(np.float64) - h) <= 2.0 ** -24 * np.abs(h))            # half an ulp of float32
    d = design_filter(sr, SR_OUT, zeros=Z, rolloff=RHO, beta=BETA)
    assert np.array_equal(d[3], gh)


@pytest.mark.parametrize('sr', RATES)
def test_filter_response(sr):
    """Passband within 1e-4 dB up to 0.875 of the lower Nyquist, stopband at most -120 dB from 1.0625 of it up to the Nyquist of the
    common rate sr_in L (everything that can alias).  Measured on this design (float32-stored h, float64 arithmetic; the test
    prints them, DESIGN 3.8 has the table): passband 6.6e-7 .. 3.5e-6 dB, stopband -144.8 .. -145.9 dB over the eight rates."""
    from reconvat_amd.resample import design_filter
    L, M, half, h = design_filter(sr, SR_OUT)
    q = max(L, M)
    n = 1 << int(np.ceil(np.log2(8 * len(h))))
    H = np.abs(np.fft.rfft(h.astype(np.float64), n)) / L
    f = np.arange(len(H)) / n * 2 * q                        # in units of the lower Nyquist: the common rate is 2 q of them
    with np.errstate(divide='ignore'):
        db = 20 * np.log10(H)
    passband = np.max(np.abs(db[f <= 0.875]))
    stopband = np.max(db[f >= 1.0625])
    print(f'{sr} -> {SR_OUT}: L/M = {L}/{M}, passband deviation {passband:.3e} dB, stopband {stopband:.1f} dB')
    assert passband <= 1e-4
    assert stopband <= -120.0


def test_over_the_cap_is_a_value_error():
    from reconvat_amd import resample
    resample.design_filter(44056, SR_OUT)                                        # 0.71 M coefficients: accepted
    with pytest.raises(ValueError, match='cap'):
        resample.design_filter(44101, SR_OUT)                                    # L = 16000: 5.7 M
    with pytest.raises(ValueError):
        resample.design_filter(0, SR_OUT)
    with pytest.raises(ValueError):
        resample.resample_host(np.zeros((0,), np.int16), 44100, SR_OUT)
    with pytest.raises(ValueError):
        resample.resample_host(np.zeros((10,), np.uint8), 44100, SR_OUT)
    from reconvat_amd import _lib
    assert _lib.load().rv_resample_max_coeffs() == resample.MAX_COEFFS


def test_polyphase_bank_holds_every_coefficient_once():
    from reconvat_amd.resample import design_filter, polyphase_bank
    for sr in (44100, 8000, 11025, 96000):
        L, M, half, h = design_filter(sr, SR_OUT)
        F, Kp, bank = polyphase_bank(L, half, h)
        assert bank.shape == (L, Kp) and Kp % 4 == 0 and bank.dtype == np.float32
        for p in (0, L // 2, L - 1):
            for u in (0, 1, F, Kp - 1):
                k = p + (F - u) * L
                assert bank[p, u] == (h[k + half] if abs(k) <= half else 0.0)
        assert np.count_nonzero(bank) == np.count_nonzero(h)


@pytest.mark.parametrize('sr', RATES)
def test_resample_host_matches_the_oracle(sr):
    from reconvat_amd.resample import resample_host
    L, M, half, _ = oracle_filter(sr)
    longest = 1500 if L > 1000 else 6000
    for T in (1, 2, 7, M, M + 1, 2 * half // L // 3 + 1, longest):              # shorter than one filter length .. several of them
        for kind in ('noise', 'zero', 'impulse'):
            if kind == 'noise':
                x = np.random.RandomState(T).uniform(-1, 1, T)
            else:
                x = np.zeros(T)
                if kind == 'impulse':
                    x[T // 2] = 1.0
            y64, _, _ = oracle(x, sr, bound=False)
            got = resample_host(x, sr, SR_OUT)
            assert got.dtype == np.float64 and got.shape == (-(-T * L // M),) == y64.shape
            assert np.max(np.abs(got - y64)) <= 1e-12, (sr, T, kind)
            # chunks and threads do not change the result
            assert np.max(np.abs(resample_host(x, sr, SR_OUT, chunk_outputs=97, workers=3) - y64)) <= 1e-12
    # stereo int16 and 24-bit-in-int32 input, int16 output
    x = as_dtype(signal('noise', 4000, sr, seed=5), np.int16, 2)
    y64, S, K = oracle(x, sr)
    assert np.max(np.abs(resample_host(x, sr, SR_OUT) - y64)) <= 1e-12
    q = resample_host(x, sr, SR_OUT, out_dtype=np.int16)
    assert q.dtype == np.int16 and np.all(np.abs(q - np.clip(32768.0 * y64, -32768, 32767)) <= 0.5 + 1e-9)
    x = as_dtype(signal('tones', 4000, sr), np.int32, 2)
    assert np.max(np.abs(resample_host(x, sr, SR_OUT) - oracle(x, sr, bound=False)[0])) <= 1e-12


def test_host_identity_passthrough():
    from reconvat_amd.resample import resample_host
    x = np.random.RandomState(0).randint(-32768, 32768, 5000).astype(np.int16)
    y = resample_host(x, SR_OUT, SR_OUT, out_dtype=np.int16)
    assert y.dtype == np.int16 and np.shares_memory(y, x) and np.array_equal(y, x)


# ---------------------------------------------------------------------------------------------------------------------------
def write_wav(path, sr, frames, sampwidth):
    """PCM wav of int16 frames (sampwidth 2) or of left-justified 24-bit-in-int32 frames (sampwidth 3)."""
    frames = np.asarray(frames)
    channels = 1 if frames.ndim == 1 else frames.shape[1]
    if sampwidth == 2:
        raw = frames.astype('<i2').tobytes()
    else:
        b = (frames.astype(np.int64) >> 8).astype('<i4').reshape(-1, 1).view(np.uint8).reshape(-1, 4)
        raw = np.ascontiguousarray(b[:, :3]).tobytes()
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(sampwidth)
        w.setframerate(sr)
        w.writeframes(raw)


NOTES = np.array([[0.10, 0.50, 60, 80], [0.30, 0.90, 64, 100], [0.55, 1.20, 72, 64], [1.00, 1.35, 45, 90]])


def write_tsv(path):
    np.savetxt(str(path), NOTES, fmt='%.6f', delimiter='\t', header='onset,offset,note,velocity')


def check_track(track, frames, sr, path):
    from reconvat_amd.constants import HOP_LENGTH
    from reconvat_amd.dataset import paint_roll
    L, M, _, _ = oracle_filter(sr)
    y64, S, K = oracle(frames, sr)
    audio = track['audio'].numpy()
    assert track['audio'].dtype == torch.int16 and audio.shape == (-(-len(frames) * L // M),)
    n_steps = (len(audio) - 1) // HOP_LENGTH + 1
    assert track['label'].shape == track['velocity'].shape == (n_steps, 88)
    err = np.abs(audio.astype(np.float64) - 32768.0 * y64)
    print(f'{path}: worst |q - 32768 y64| = {err.max():.4f} (bound at that sample {int16_bound(S, K)[err.argmax()]:.4f})')
    assert np.all(err <= int16_bound(S, K))
    label, velocity = paint_roll(NOTES, n_steps)
    assert np.array_equal(track['label'].numpy(), label) and np.array_equal(track['velocity'].numpy(), velocity)
    assert label.any()
    assert track['source_rate'] == sr and track['path'] == path


def make_recordings(tmp_path):
    """A 44.1 kHz stereo 16-bit wav and a 48 kHz mono 24-bit wav (1.5 s each, amplitude 0.8) with their tsv."""
    out = []
    for name, sr, dtype, channels, width in (('stereo44', 44100, np.int16, 2, 2), ('mono48', 48000, np.int32, 1, 3)):
        frames = as_dtype(0.8 * signal('tones', int(1.5 * sr), sr) + 0.1 * signal('noise', int(1.5 * sr), sr, seed=3), dtype, channels)
        path = str(tmp_path / (name + '.wav'))
        write_wav(path, sr, frames, width)
        write_tsv(tmp_path / (name + '.tsv'))
        out.append((path, str(tmp_path / (name + '.tsv')), sr, frames))
    return out


def test_ingest_any_rate_wav_on_the_host(tmp_path):
    from scipy.io import wavfile
    from reconvat_amd.dataset import ingest_track, read_audio_int16
    for path, tsv, sr, frames in make_recordings(tmp_path):
        got_sr, stored = wavfile.read(path)
        assert got_sr == sr and np.array_equal(stored, frames)                  # the file holds what the oracle is given
        track = ingest_track(path, tsv)
        check_track(track, frames, sr, path)
        assert np.array_equal(read_audio_int16(path), track['audio'].numpy())
        cached = ingest_track(path, tsv)                                        # second call: the .pt cache
        assert os.path.exists(os.path.splitext(path)[0] + '.pt')
        assert torch.equal(cached['audio'], track['audio']) and cached['source_rate'] == sr


def test_16k_mono_file_is_ingested_as_before(tmp_path):
    """The parent's path: scipy's samples as they are, n_steps from their count, no extra key in the track."""
    from scipy.io import wavfile
    from reconvat_amd.constants import HOP_LENGTH
    from reconvat_amd.dataset import ingest_track, paint_roll, read_audio_int16
    pcm = np.random.RandomState(7).randint(-32768, 32768, 16000 + 123).astype(np.int16)
    path, tsv = str(tmp_path / 'a.wav'), str(tmp_path / 'a.tsv')
    wavfile.write(path, 16000, pcm)
    write_tsv(tsv)
    assert np.array_equal(read_audio_int16(path), pcm) and read_audio_int16(path).dtype == np.int16
    track = ingest_track(path, tsv)
    assert sorted(track) == ['audio', 'label', 'path', 'velocity']
    assert track['audio'].dtype == torch.int16 and np.array_equal(track['audio'].numpy(), pcm)
    label, velocity = paint_roll(NOTES, (len(pcm) - 1) // HOP_LENGTH + 1)
    assert np.array_equal(track['label'].numpy(), label) and np.array_equal(track['velocity'].numpy(), velocity)


def test_load_audio_16k_path_unchanged_and_host_resampling(tmp_path):
    import transcribe_files
    pcm = np.random.RandomState(8).randint(-32768, 32768, (4000, 2)).astype(np.int16)
    path = str(tmp_path / 's16.wav')
    write_wav(path, 16000, pcm, 2)
    want = torch.from_numpy(pcm.mean(axis=1).astype(np.float32) / 32768.0)
    assert torch.equal(transcribe_files.load_audio(path), want)
    (path, _, sr, frames), _ = make_recordings(tmp_path)
    y64, S, K = oracle(frames, sr)
    got = transcribe_files.load_audio(path, 'cpu')
    assert got.dtype == torch.float32 and np.all(np.abs(got.numpy().astype(np.float64) * 32768.0 - 32768.0 * y64) <= int16_bound(S, K))


def test_resampler_needs_a_hip_device():
    from reconvat_amd.resample import Resampler
    with pytest.raises(RuntimeError, match='HIP device only'):
        Resampler(44100, SR_OUT, 'cpu')
