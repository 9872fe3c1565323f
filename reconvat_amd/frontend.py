"""Log-Mel front-end modules with the reference's attribute / state_dict layout.

``MelSpectrogram`` mirrors nnAudio's class as the reference uses it (model/UNet_onset.py:354-356,
model/Spectrogram.py:396-461): buffers ``mel_basis [229,1025]`` and ``stft.{wsin,wcos} [1025,1,2048]``,
``stft.window_mask [1,2048,1]`` are kept so a reference checkpoint loads with ``load_state_dict`` -- but
the computation is the fused FFT kernel (csrc/mel.hip), driven by small derived tables (window, FFT
twiddles, the sparse rows of ``mel_basis``) that are rebuilt whenever the buffers are (re)loaded.

The three helpers nnAudio 0.2.0 provides (not vendored in the reference) are restated here from their
published definitions: periodic Hann window, windowed DFT kernels, librosa-0.7 Slaney mel filterbank.

``CQT1992v2`` mirrors the reference's constant-Q front end (model/Spectrogram.py:1241-1326, the ``spec='CQT'`` default of
both ReconVAT models): buffers ``lenghts [n_bins]``, ``cqt_kernels_real`` / ``cqt_kernels_imag [n_bins, 1, 32768]``.  Its
computation is the banded MFMA kernel of csrc/cqt.hip over packed tap windows derived from those buffers.
"""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from .constants import SAMPLE_RATE, HOP_LENGTH, N_BINS, MEL_FMIN, MEL_FMAX, WINDOW_LENGTH


def _hann(n):
    k = np.arange(n, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * k / n)


def _slaney_hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-12) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def _slaney_mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    lin = m * (200.0 / 3.0)
    log = 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0))
    return np.where(m >= 15.0, log, lin)


def slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax):
    nf = n_fft // 2 + 1
    freqs = np.linspace(0.0, sr / 2.0, nf)
    edges = _slaney_mel_to_hz(np.linspace(_slaney_hz_to_mel(fmin), _slaney_hz_to_mel(fmax), n_mels + 2))
    width = np.diff(edges)
    ramps = edges[:, None] - freqs[None, :]
    lower = -ramps[:-2] / width[:-1, None]
    upper = ramps[2:] / width[1:, None]
    basis = np.maximum(0.0, np.minimum(lower, upper))
    basis *= (2.0 / (edges[2:] - edges[:-2]))[:, None]
    return basis.astype(np.float32)


class STFT(nn.Module):
    """Holds the reference's STFT buffers (state_dict compatibility only)."""

    def __init__(self, n_fft=WINDOW_LENGTH):
        super().__init__()
        n = np.arange(n_fft, dtype=np.float64)
        k = np.arange(n_fft // 2 + 1, dtype=np.float64)
        ang = 2.0 * np.pi * k[:, None] * n[None, :] / n_fft
        win = torch.from_numpy(_hann(n_fft).astype(np.float32))
        self.register_buffer('wsin', (torch.from_numpy(np.sin(ang).astype(np.float32)) * win).unsqueeze(1))
        self.register_buffer('wcos', (torch.from_numpy(np.cos(ang).astype(np.float32)) * win).unsqueeze(1))
        self.register_buffer('window_mask', win.view(1, -1, 1))


class MelSpectrogram(nn.Module):
    def __init__(self, sr=SAMPLE_RATE, n_fft=WINDOW_LENGTH, n_mels=N_BINS, hop_length=HOP_LENGTH, fmin=MEL_FMIN,
                 fmax=MEL_FMAX):
        super().__init__()
        if n_fft != 2048 or hop_length != 512 or n_mels > 256:
            raise ValueError('the fused front-end kernel (csrc/mel.hip: four frames per workgroup sharing one audio chunk, one thread '
                             f'per mel band) is built for n_fft = 2048, hop_length = 512, n_mels <= 256; got n_fft={n_fft}, '
                             f'hop_length={hop_length}, n_mels={n_mels} (the reference scripts use 2048 / 512 / 229)')
        self.n_fft, self.hop, self.n_mels = n_fft, hop_length, n_mels
        self.stft = STFT(n_fft)
        self.register_buffer('mel_basis', torch.from_numpy(slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax)))
        self._tables = None
        self._tables_key = None

    def tables(self):
        """Derived kernel tables on the buffers' device (rebuilt if the buffers changed)."""
        mb, wm = self.mel_basis, self.stft.window_mask
        key = (mb.device, mb._version, wm._version, mb.data_ptr())
        if self._tables is not None and self._tables_key == key:
            return self._tables
        basis = mb.detach().cpu().numpy()
        nz = basis != 0
        start = nz.argmax(1).astype(np.int32)
        last = (basis.shape[1] - 1 - nz[:, ::-1].argmax(1)).astype(np.int32)
        length = np.where(nz.any(1), last - start + 1, 0).astype(np.int32)
        if int(length.max()) > 32:
            raise ValueError(f'the fused front-end kernel keeps 32 filter taps per mel band in registers; the widest band of this '
                             f'filterbank spans {int(length.max())} FFT bins (fewer mel bands / a higher fmax than the reference '
                             "scripts' 229 bands over 30 .. 8000 Hz widen the bands)")
        # taps past a band's end are stored as zeros and still multiplied: like the reference's dense `mel_basis @ spec`
        # (0 * inf = nan there poisons EVERY band), a non-finite power bin is not contained to its own bands -- finite audio assumed
        ld = 32
        w = np.zeros((basis.shape[0], ld), dtype=np.float32)
        for i in range(basis.shape[0]):
            w[i, :length[i]] = basis[i, start[i]:start[i] + length[i]]
        k = np.arange(self.n_fft // 2, dtype=np.float64)
        tw = np.stack([np.cos(2 * np.pi * k / self.n_fft), -np.sin(2 * np.pi * k / self.n_fft)], 1).astype(np.float32)
        dev = mb.device
        self._tables = {
            'window': wm.detach().reshape(-1).contiguous().float(),
            'twiddle': torch.from_numpy(tw).to(dev),
            'mel_start': torch.from_numpy(start).to(dev),
            'mel_len': torch.from_numpy(length).to(dev),
            'mel_w': torch.from_numpy(w).to(dev),
        }
        self._tables_key = key
        return self._tables

    @staticmethod
    def _as_batch(x):
        if x.dim() == 1:
            return x[None, :]
        if x.dim() == 3 and x.shape[1] == 1:
            return x[:, 0, :]
        if x.dim() == 2:
            return x
        raise ValueError("Only support input with shape = (batch, len) or shape = (len)")

    def forward(self, x):
        """Mel power spectrogram [B, n_mels, T] like nnAudio's MelSpectrogram.forward."""
        x = self._as_batch(x)
        if x.shape[-1] < self.n_fft // 2:
            raise AssertionError("Signal length shorter than reflect padding length (n_fft // 2).")
        return ops.melspec(x, self.tables(), do_log=False, normalise=False, hop=self.hop).transpose(1, 2)

    def lognorm(self, x, log=True, normalise=True):
        """Fused path: (log-)mel, per-clip min-max normalised, time-major [B, 1, T, n_mels]."""
        x = self._as_batch(x)
        return ops.melspec(x, self.tables(), do_log=log, normalise=normalise, hop=self.hop).unsqueeze(1)


def create_cqt_kernels(Q, fs, fmin, n_bins=84, bins_per_octave=12, norm=1, window='hann', fmax=None, topbin_check=True):
    """nnAudio 0.2.0 ``utils.create_cqt_kernels`` restated from its published definition (parity unpinned: nnAudio is
    not vendored in the reference).  Returns (complex64 [n_bins, fftLen] kernels, fftLen, float32 tensor of the lengths).

    Points where another version could differ, written down as restated here:
    * centre frequencies f_k = fmin * 2^(k / bins_per_octave) (fmax given: n_bins = ceil(bins_per_octave * log2(fmax/fmin)));
    * lengths l_k = ceil(Q * fs / f_k) in float64; fftLen = 2^ceil(log2(ceil(Q * fs / fmin)));
    * window: scipy ``get_window('hann', l, fftbins=True)``, i.e. the PERIODIC Hann 0.5 - 0.5 cos(2 pi n / l) (only 'hann');
    * row k = window * exp(i 2 pi f_k n / fs) / l for n in np.r_[-l//2 : l//2] (float l: n runs from floor(-l/2));
    * normalisation: the row is divided by its L``norm`` norm (norm=1: L1, as librosa) in complex128, then cast to complex64;
    * centring: the row starts at ceil(fftLen/2 - l/2), one sample earlier when l is odd."""
    if window != 'hann':
        raise ValueError(f"only window='hann' is restated (got {window!r})")
    fft_len = 2 ** int(np.ceil(np.log2(np.ceil(Q * fs / fmin))))
    if fmax is not None:
        n_bins = np.ceil(bins_per_octave * np.log2(fmax / fmin))
    freqs = fmin * 2.0 ** (np.r_[0:n_bins] / float(bins_per_octave))
    if np.max(freqs) > fs / 2 and topbin_check:
        raise ValueError(f'The top bin {np.max(freqs)}Hz has exceeded the Nyquist frequency, please reduce the n_bins')
    kernels = np.zeros((int(n_bins), int(fft_len)), dtype=np.complex64)
    lengths = np.ceil(Q * fs / freqs)
    for k in range(int(n_bins)):
        freq = freqs[k]
        l = np.ceil(Q * fs / freq)
        start = int(np.ceil(fft_len / 2.0 - l / 2.0)) - (1 if l % 2 == 1 else 0)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(int(l), dtype=np.float64) / l)
        sig = win * np.exp(np.r_[-l // 2:l // 2] * 1j * 2 * np.pi * freq / fs) / l
        if norm:
            kernels[k, start:start + int(l)] = sig / np.linalg.norm(sig, norm)
        else:
            kernels[k, start:start + int(l)] = sig
    return kernels, fft_len, torch.tensor(lengths).float()


# split-K slice of the CQT kernel: every workgroup multiplies at most this many taps of one 16-bin group (a multiple of 64:
# four waves x 16-tap blocks); the low groups (up to 19 856 taps) split into several slices, the high ones (127 taps) take one
CQT_SLICE = 2048


class CQT1992v2(nn.Module):
    """Constant-Q magnitude spectrogram with nnAudio's ``CQT1992v2`` constructor and buffers (model/Spectrogram.py:1241-1326),
    computed by the banded kernel of csrc/cqt.hip: per 16-bin group only the union of its rows' non-zero taps is multiplied
    (853 280 of 176 x 32 768 taps per frame in the reference configuration).  ``trainable=True`` and the 'Complex' / 'Phase'
    outputs are not provided; ``n_bins`` is this instance's own (the reference's module-global N_BINS is not reproduced)."""

    def __init__(self, sr=22050, hop_length=512, fmin=32.70, fmax=None, n_bins=84, bins_per_octave=12, norm=1, window='hann',
                 center=True, pad_mode='reflect', trainable=False, output_format='Magnitude', verbose=True):
        super().__init__()
        if trainable:
            raise NotImplementedError('CQT1992v2(trainable=True) is not provided: the kernel bank is a fixed buffer here')
        if output_format != 'Magnitude':
            raise NotImplementedError(f"CQT1992v2 provides output_format='Magnitude' only (got {output_format!r})")
        if not center or pad_mode != 'reflect':
            raise NotImplementedError('CQT1992v2 provides center=True with reflect padding only (the reference configuration)')
        if hop_length % 4 != 0:
            raise ValueError(f'the CQT kernel reads frames with 16-byte loads: hop_length must be a multiple of 4 (got {hop_length})')
        self.trainable, self.hop_length, self.center, self.pad_mode, self.output_format = False, hop_length, True, 'reflect', output_format
        Q = 1 / (2 ** (1 / bins_per_octave) - 1)
        kernels, self.kernel_width, lenghts = create_cqt_kernels(Q, sr, fmin, n_bins, bins_per_octave, norm, window, fmax)
        self.n_bins = kernels.shape[0]
        self.fmin, self.bins_per_octave = float(fmin), int(bins_per_octave)      # the bins' centre frequencies: fmin 2^(k / bins_per_octave)
        self.register_buffer('lenghts', lenghts)
        self.register_buffer('cqt_kernels_real', torch.tensor(kernels.real).unsqueeze(1))
        self.register_buffer('cqt_kernels_imag', torch.tensor(kernels.imag).unsqueeze(1))
        self._tables = None
        self._tables_key = None

    def _key(self):
        bufs = (self.lenghts, self.cqt_kernels_real, self.cqt_kernels_imag)
        return (self.lenghts.device,) + tuple((b._version, b.data_ptr()) for b in bufs)

    def tables(self):
        """Packed kernel tables on the buffers' device, rebuilt whenever a buffer changed (load_state_dict, .to()):
        * ``w``: per 16-bin group g a [32][K_g] block -- rows 0..15 the real taps of bins 16g.., rows 16..31 the imaginary
          taps, over the group's tap window [tw_g, tw_g + K_g) (the union of its rows' non-zero supports, widened to 16);
          the taps are the buffers' values unchanged: sqrt(lenghts) is applied in the epilogue (after the sum, as the
          reference multiplies the conv1d output), and the sign of the imaginary part is dropped (|.| only: exact);
        * ``items`` [n_items][8] int32: split-K work items (group, first tap, taps, weight offset, K_g, 0, 0, 0), slices of
          at most CQT_SLICE taps; ``groups`` [n_groups][2]: (first item, item count), summed in that order;
        * ``scale`` [n_bins]: sqrt(lenghts) in float32."""
        key = self._key()
        if self._tables is not None and self._tables_key == key:
            return self._tables
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError('CQT1992v2: the kernel tables are stale (buffers changed) inside a graph capture; call tables() '
                               'once before capturing')
        re = self.cqt_kernels_real.detach().float().cpu().numpy()[:, 0, :]
        im = self.cqt_kernels_imag.detach().float().cpu().numpy()[:, 0, :]
        nb, width = re.shape
        nz = (re != 0) | (im != 0)
        if not nz.any(1).all():
            raise ValueError('CQT1992v2: a kernel row is all zeros')
        first = nz.argmax(1)
        last = width - 1 - nz[:, ::-1].argmax(1)
        n_groups = (nb + 15) // 16
        blocks, items, groups, woff = [], [], [], 0
        for g in range(n_groups):
            rows = slice(16 * g, min(16 * g + 16, nb))
            tw = int(first[rows].min()) // 16 * 16
            k = (int(last[rows].max()) + 1 + 15) // 16 * 16 - tw
            blk = np.zeros((32, k), dtype=np.float32)
            n = rows.stop - rows.start
            blk[:n] = re[rows, tw:tw + k]
            blk[16:16 + n] = im[rows, tw:tw + k]
            blocks.append(blk.reshape(-1))
            groups.append((len(items), (k + CQT_SLICE - 1) // CQT_SLICE))
            for s in range(0, k, CQT_SLICE):
                items.append((g, tw + s, min(CQT_SLICE, k - s), woff + s, k, 0, 0, 0))
            woff += 32 * k
        dev = self.lenghts.device
        self._tables = {
            'w': torch.from_numpy(np.concatenate(blocks)).to(dev),
            'items': torch.tensor(items, dtype=torch.int32, device=dev),
            'groups': torch.tensor(groups, dtype=torch.int32, device=dev),
            'scale': torch.sqrt(self.lenghts.detach().float()).contiguous(),
            'kernel_width': width,
            'taps_exact': int((last - first + 1).sum()),
            'taps_tiled': int(sum(16 * (it[2]) for it in items)),
        }
        self._tables_key = key
        return self._tables

    def _as_batch(self, x):
        x = MelSpectrogram._as_batch(x)
        if x.shape[-1] <= self.kernel_width // 2:
            raise ValueError(f'CQT1992v2: the signal ({x.shape[-1]} samples) must be longer than the reflect padding '
                             f'(kernel_width // 2 = {self.kernel_width // 2} samples), as torch.nn.ReflectionPad1d requires')
        return x

    def forward(self, x):
        """Constant-Q magnitudes [B, n_bins, T] like nnAudio's CQT1992v2.forward (output_format='Magnitude')."""
        x = self._as_batch(x)
        return ops.cqtspec(x, self.tables(), do_log=False, normalise=False, hop=self.hop_length).transpose(1, 2)

    def lognorm(self, x, log=True, normalise=True):
        """Fused path: (log-)CQT magnitude, per-clip min-max normalised, time-major [B, 1, T, n_bins]."""
        x = self._as_batch(x)
        return ops.cqtspec(x, self.tables(), do_log=log, normalise=normalise, hop=self.hop_length).unsqueeze(1)


def cqt_gflop(tables, batch, frames):
    """(exact-support, group-tiled) GFLOP of the CQT front end: 2 flop per tap, real and imaginary, per frame and clip."""
    f = 2.0 * 2.0 * batch * frames / 1e9
    return tables['taps_exact'] * f, tables['taps_tiled'] * f


class Normalization:
    """model/utils.py:82-106 ('imagewise' and 'framewise' min-max) for callers that use
    ``model.normalize.transform`` directly; the hot path uses the fused kernel instead."""

    def __init__(self, mode='framewise'):
        if mode not in ('framewise', 'imagewise'):
            print('please choose the correct mode')
        self.mode = mode

    def transform(self, x):
        if self.mode == 'framewise':
            x_max = x.max(1, keepdim=True)[0]
            x_min = x.min(1, keepdim=True)[0]
            out = (x - x_min) / (x_max - x_min)
            out[torch.isnan(out)] = 0
            return out
        flat = x.reshape(x.shape[0], -1)
        x_max = flat.max(1, keepdim=True)[0].unsqueeze(1)
        x_min = flat.min(1, keepdim=True)[0].unsqueeze(1)
        return (x - x_min) / (x_max - x_min)
