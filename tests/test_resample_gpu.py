"""The polyphase resampler on the device (csrc/resample.hip) against the float64 oracle of tests/test_resample.py.

Error bound, derived and not measured: for every output sample |y - y64| <= (K + 8) 2^-24 S_m, K = taps per output,
S_m = sum_n |x[n]| |h[m M - n L]| in float64 -- the bound of a length-K float32 dot product in any order, with or without FMA, plus
the float32 rounding of coefficients and downmix.  As int16: |q - clip(32768 y64)| <= 0.5 + 32768 bound.  No sample is excluded.
"""
import os

import numpy as np
import pytest
import torch

import test_resample as tr
from test_resample import RATES, SR_OUT, as_dtype, f32_bound, int16_bound, oracle, oracle_filter, signal

pytestmark = pytest.mark.gpu

TORCH = {np.int16: torch.int16, np.int32: torch.int32, np.float32: torch.float32}


def run(dev, frames, sr, out_dtype=torch.float32, chunk_outputs=None, on_device=True):
    from reconvat_amd.resample import Resampler
    x = torch.from_numpy(frames)
    rs = Resampler(sr, SR_OUT, dev, out_dtype=out_dtype)
    y = rs(x.to(dev) if on_device else x, chunk_outputs=chunk_outputs)
    torch.cuda.synchronize()
    assert y.dtype == out_dtype and y.device.type == 'cuda'
    return y.cpu().numpy()


def check_float(y, y64, S, K, tag):
    assert y.shape == y64.shape, tag
    err, bound = np.abs(y.astype(np.float64) - y64), f32_bound(S, K)
    worst = int(np.argmax(err - bound))
    print(f'{tag}: worst |y - y64| = {err.max():.3e}, tightest sample {worst}: err {err[worst]:.3e} of bound {bound[worst]:.3e}')
    assert np.all(err <= bound), tag


def check_int16(q, y64, S, K, tag):
    assert q.shape == y64.shape and q.dtype == np.int16, tag
    err = np.abs(q.astype(np.float64) - np.clip(32768.0 * y64, -32768.0, 32767.0))
    print(f'{tag}: worst |q - 32768 y64| = {err.max():.4f}')
    assert np.all(err <= int16_bound(S, K)), tag
    over = 32768.0 * f32_bound(S, K) + 0.5
    assert np.all(q[32768.0 * y64 >= 32767.0 + over] == 32767) and np.all(q[32768.0 * y64 <= -32768.0 - over] == -32768), tag


@pytest.mark.parametrize('sr', RATES)
def test_every_rate_edges_chunks_repeatability(dev, sr):
    """Full-scale noise, int16 stereo in: float32 and int16 out; output 0 and the last output sit on the signal's edges; a prime
    chunk size (at least three chunks, a host-resident source) and a second run reproduce the single launch bit for bit."""
    L, M, _, _ = oracle_filter(sr)
    T = 12000 if L > 1000 else 30011
    frames = as_dtype(signal('noise', T, sr, seed=sr), np.int16, 2)
    y64, S, K = oracle(frames, sr)
    y = run(dev, frames, sr)
    check_float(y, y64, S, K, f'{sr} float32')
    q = run(dev, frames, sr, torch.int16)
    check_int16(q, y64, S, K, f'{sr} int16')
    chunk = 1009
    assert len(y64) >= 3 * chunk
    for out_dtype, whole in ((torch.float32, y), (torch.int16, q)):
        assert np.array_equal(run(dev, frames, sr, out_dtype), whole)
        assert np.array_equal(run(dev, frames, sr, out_dtype, chunk_outputs=chunk), whole)
        assert np.array_equal(run(dev, frames, sr, out_dtype, chunk_outputs=chunk, on_device=False), whole)


@pytest.mark.parametrize('dtype,channels', [(np.int16, 1), (np.int16, 2), (np.int32, 2), (np.float32, 1), (np.float32, 3)])
@pytest.mark.parametrize('kind', ['noise', 'tones', 'square'])
def test_signals_and_sample_types(dev, kind, dtype, channels):
    sr, T = 44100, 12007
    frames = as_dtype(signal(kind, T, sr, seed=11), dtype, channels)
    y64, S, K = oracle(frames, sr)
    tag = f'{kind} {np.dtype(dtype).name} x{channels}'
    check_float(run(dev, frames, sr), y64, S, K, tag)
    q = run(dev, frames, sr, torch.int16, chunk_outputs=997)
    check_int16(q, y64, S, K, tag)
    if kind == 'square' and channels == 1:
        assert np.any(32768.0 * y64 > 32767.5) and np.any(q == 32767) and np.any(q == -32768)         # the overshoot saturates


def test_short_signals(dev):
    """T shorter than one filter length, down to one frame."""
    for sr in (44100, 8000, 96000):
        for T in (1, 2, 5, 177, 1000):
            frames = as_dtype(signal('noise', T, sr, seed=T), np.int16, 1)
            y64, S, K = oracle(frames, sr)
            check_float(run(dev, frames, sr), y64, S, K, f'{sr} T={T}')
            check_int16(run(dev, frames, sr, torch.int16), y64, S, K, f'{sr} T={T}')


def test_same_rate_mono_int16_is_untouched(dev):
    frames = np.random.RandomState(0).randint(-32768, 32768, 5000).astype(np.int16)
    assert np.array_equal(run(dev, frames, SR_OUT, torch.int16), frames)
    assert np.array_equal(run(dev, frames, SR_OUT), frames.astype(np.float32) / 32768.0)


def test_aliasing_and_passband(dev):
    """A 10 kHz sine at 44.1 kHz (faded in and out, so that the signal itself is band limited) lies above the 8 kHz output Nyquist:
    what comes out is below the float32 noise floor the error bound implies.  A 1 kHz sine keeps its amplitude within that bound."""
    sr, T, A = 44100, 30000, 0.9
    t = np.arange(T) / sr
    fade = np.ones(T)
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(4000) / 4000)
    fade[:4000], fade[-4000:] = ramp, ramp[::-1]
    x = (A * np.sin(2 * np.pi * 10000.0 * t) * fade).astype(np.float32)
    y64, S, K = oracle(x, sr)
    y = run(dev, x, sr)
    check_float(y, y64, S, K, '10 kHz')
    rms, floor = np.sqrt(np.mean(y.astype(np.float64) ** 2)), np.sqrt(np.mean(f32_bound(S, K) ** 2))
    print(f'10 kHz in: output rms {rms:.3e} (oracle {np.sqrt(np.mean(y64 ** 2)):.3e}), float32 floor of the bound {floor:.3e}')
    assert rms <= floor
    x = (A * np.sin(2 * np.pi * 1000.0 * t)).astype(np.float32)
    y64, S, K = oracle(x, sr)
    y = run(dev, x, sr).astype(np.float64)
    check_float(y, y64, S, K, '1 kHz')
    mid = slice(2000, 2000 + 16 * 300)                                          # 300 whole periods of 1 kHz at 16 kHz, clear of the edges
    amp = 2 * np.abs(np.mean(y[mid] * np.exp(-2j * np.pi * 1000.0 * np.arange(len(y))[mid] / SR_OUT)))
    slack = f32_bound(S, K)[mid].max() + A * (10 ** (1e-4 / 20) - 1) + A * 2.0 ** -24
    print(f'1 kHz in: amplitude {amp:.8f} for {A} (slack {slack:.2e})')
    assert abs(amp - A) <= slack


def test_dataset_and_transcription_on_the_device(dev, tmp_path):
    """ingest_track / read_audio_int16 / transcribe_files.load_audio resample on the device; transcribe2midi takes the file."""
    import reconvat_amd as ra
    import transcribe_files
    from reconvat_amd.dataset import ingest_track, read_audio_int16
    for path, tsv, sr, frames in tr.make_recordings(tmp_path):
        track = ingest_track(path, tsv, device=dev)
        tr.check_track(track, frames, sr, path)
        host = read_audio_int16(path, 'cpu').astype(np.int64)
        assert np.max(np.abs(track['audio'].numpy().astype(np.int64) - host)) <= 1                     # the two paths: within 1 LSB
    path, _, sr, frames = tr.make_recordings(tmp_path)[0]
    y64, S, K = oracle(frames, sr)
    audio = transcribe_files.load_audio(path, dev)
    assert audio.dtype == torch.float32 and audio.shape == y64.shape
    assert np.all(np.abs(audio.numpy().astype(np.float64) * 32768.0 - np.clip(32768.0 * y64, -32768, 32767)) <= int16_bound(S, K))
    torch.manual_seed(0)
    model = ra.UNet((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel', device=str(dev)).to(dev).eval()
    out = str(tmp_path / 'midi')
    transcribe_files.transcribe2midi([path], model, dev, out)
    midi = os.path.join(out, 'ReconVAT-stereo44.mid')
    assert os.path.exists(midi) and os.path.getsize(midi) > 0


def test_bad_arguments_are_refused_before_any_launch(dev):
    from reconvat_amd import _lib, resample
    from reconvat_amd._lib import ptr
    lib = _lib.load()
    rs = resample.Resampler(44100, SR_OUT, dev)
    x = torch.zeros(1000, 2, dtype=torch.int16, device=dev)
    y = torch.zeros(363, dtype=torch.float32, device=dev)
    L, M, F, Kp = rs.L, rs.M, rs.F, rs.Kp
    good = [ptr(x), 0, 1000, 2, 0, ptr(rs.bank), L, M, F, Kp, ptr(y), 0, 0, 363, None]

    def status(**change):
        names = ['x', 'in_dtype', 'T_in', 'C', 'in_offset', 'bank', 'L', 'M', 'F', 'Kp', 'y', 'out_dtype', 'm_start', 'n_out', 'stream']
        args = list(good)
        for k, v in change.items():
            args[names.index(k)] = v
        return lib.rv_resample(*args)
    assert status() == 0
    torch.cuda.synchronize()
    for change in (dict(T_in=0), dict(n_out=0), dict(C=0), dict(C=65), dict(x=None), dict(bank=None), dict(y=None), dict(in_dtype=3),
                   dict(out_dtype=2), dict(L=0), dict(M=0), dict(Kp=Kp + 1), dict(Kp=0), dict(L=1 << 20), dict(L=50000, Kp=Kp),
                   dict(in_offset=-1), dict(m_start=-1), dict(bank=ptr(rs.bank) + 4)):
        assert status(**change) == -1, change
        assert 'rv_resample' in _lib.last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='cap'):
        resample.Resampler(44101, SR_OUT, dev)
    with pytest.raises(ValueError):
        rs(torch.zeros(0, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError):
        rs(torch.zeros(10, 0, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError):
        rs(torch.zeros(10, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        rs(torch.zeros(10, dtype=torch.int16, device=dev), chunk_outputs=0)
    with pytest.raises(ValueError):
        resample.Resampler(44100, SR_OUT, dev, out_dtype=torch.float64)
