"""Sample-rate conversion for audio ingest: rational-ratio polyphase FIR resampling with the channel downmix fused in.

Definition (everything here and `csrc/resample.hip` implement exactly this):

    g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, q = max(L, M), half = zeros * q
    h[i] = L * (rolloff / q) * sinc(rolloff * i / q) * kaiser(2 half + 1, beta)[i + half],   i = -half .. half
    y[m] = sum_n x[n] h[m M - n L],   m = 0 .. ceil(T L / M) - 1,   x[n] = mean over channels of frame n, zero outside [0, T)

No delay: output m sits at time m / sr_out.  int16 input is scaled by 2^-15, int32 by 2^-31 (how `scipy.io.wavfile` delivers 24-
and 32-bit PCM); int16 output is round-half-even of 32768 y, saturated.

  design_filter    the filter (float64 design, float32 storage)
  Resampler        the device path: `rv_resample` on a HIP device, long signals in bounded chunks (bit-identical to one call)
  resample_host    the same definition in float64 with scipy's upfirdn, for machines without a GPU

The device path sums in float32, the host path in float64: as int16 the two agree to within 1 LSB (a sample whose exact value
lies next to a rounding boundary may fall on either side), as float32 to within the float32 dot-product bound
(K + 8) 2^-24 sum |x| |h| that tests/test_resample_gpu.py checks.
"""
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ZEROS = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
# Coefficient cap of one polyphase bank (L * padded taps per phase; 16 MiB of float32): mirrors RV_RESAMPLE_MAX_COEFFS in
# csrc/resample.hip (tests/test_resample.py compares the two).  44056 -> 16000 (L = 2000) needs 0.71 M, 44100 -> 16000 57 k.
MAX_COEFFS = 1 << 22
MAX_RATIO = 65536
MAX_SPAN = 12288          # input frames (float32, 48 KiB of LDS) one workgroup stages: RV_RESAMPLE_MAX_SPAN
MAX_CHANNELS = 64
IN_DTYPES = {torch.int16: (0, 2.0 ** -15), torch.int32: (1, 2.0 ** -31), torch.float32: (2, 1.0)}
OUT_DTYPES = {torch.float32: 0, torch.int16: 1}


def ratio(sr_in, sr_out):
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f'sample rates must be positive (got {sr_in} -> {sr_out})')
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def output_length(T, L, M):
    return -(-T * L // M)


def _design64(sr_in, sr_out, zeros, rolloff, beta):
    L, M = ratio(sr_in, sr_out)
    q = max(L, M)
    half = int(zeros) * q
    if int(zeros) < 1:
        raise ValueError(f'zeros must be positive (got {zeros})')
    bank = L * 4 * -(-(half // L + -(-half // L) + 1) // 4)                     # L * Kp of polyphase_bank
    if L > MAX_RATIO or M > MAX_RATIO or bank > MAX_COEFFS:
        raise ValueError(f'{sr_in} -> {sr_out} Hz reduces to {L}/{M}: a polyphase bank of {bank} coefficients, over the cap of '
                         f'{MAX_COEFFS} coefficients (or a ratio term over {MAX_RATIO}); resample to a rate with a larger common divisor')
    rows = -(-256 // L) * L                                                     # outputs of the kernel's smallest tile (resample.hip)
    span = (L - 1 + (rows - 1) * M) // L + bank // L
    if span > MAX_SPAN:
        raise ValueError(f'{sr_in} -> {sr_out} Hz reduces to {L}/{M}: one tile of {rows} outputs reads {span} input frames, over the '
                         f'{MAX_SPAN} the kernel stages per workgroup')
    i = np.arange(-half, half + 1, dtype=np.float64)
    h = L * (rolloff / q) * np.sinc(rolloff * i / q) * np.kaiser(2 * half + 1, beta)
    return L, M, half, h


def design_filter(sr_in, sr_out, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA):
    """(L, M, half, h): h float32 [2 half + 1], h[half + i] = the coefficient at lag i.  ValueError over the bank cap."""
    L, M, half, h = _design64(sr_in, sr_out, zeros, rolloff, beta)
    return L, M, half, h.astype(np.float32)


def polyphase_bank(L, half, h):
    """(F, Kp, bank [L, Kp] float32): bank[p][u] = h[p + (F - u) L] (zero beyond the filter), F = half // L, Kp = taps per phase
    rounded up to a multiple of 4 -- the layout `rv_resample` reads: y[m] = sum_u bank[p][u] x[n0 - F + u], (n0, p) = divmod(m M, L)."""
    F = half // L
    K = F + -(-half // L) + 1
    Kp = 4 * -(-K // 4)
    k = np.arange(L)[:, None] + (F - np.arange(Kp))[None, :] * L
    inside = np.abs(k) <= half
    bank = np.where(inside, np.asarray(h)[np.clip(k + half, 0, 2 * half)], 0).astype(np.float32)
    return F, Kp, np.ascontiguousarray(bank)


def _frames(x):
    if x.dim() == 1:
        x = x.unsqueeze(1)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'expected a non-empty [T] or [T, C] signal, got shape {tuple(x.shape)}')
    if x.shape[1] > MAX_CHANNELS:
        raise ValueError(f'{x.shape[1]} channels: at most {MAX_CHANNELS} (is the signal [T, C], frames first?)')
    if x.dtype not in IN_DTYPES:
        raise ValueError(f'sample type {x.dtype}: expected int16, int32 or float32')
    return x.contiguous()


class Resampler:
    """`Resampler(sr_in, sr_out, device)(x)`: x an int16 / int32 / float32 tensor [T] or [T, C] (frames first, on the host or on the
    device) -> [ceil(T L / M)] of `out_dtype` (float32 or int16) on `device`.  The coefficient bank is built once and kept on the
    device.  A signal longer than `chunk_outputs` outputs runs as several launches, each on the slice of the input its outputs touch
    (a host tensor is uploaded slice by slice, so the source never has to fit in HBM next to the corpus); the result is bit-identical
    to a single launch.  sr_in == sr_out on mono int16 input returns the samples as they are, without a launch."""

    def __init__(self, sr_in, sr_out, device, out_dtype=torch.float32, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA, chunk_outputs=1 << 22):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'Resampler runs on a HIP device only (got {self.device}); resample_host is the host path')
        if out_dtype not in OUT_DTYPES:
            raise ValueError(f'out_dtype {out_dtype}: expected torch.float32 or torch.int16')
        self.sr_in, self.sr_out, self.out_dtype = int(sr_in), int(sr_out), out_dtype
        self.L, self.M, self.half, h = design_filter(sr_in, sr_out, zeros, rolloff, beta)
        self.F, self.Kp, bank = polyphase_bank(self.L, self.half, h)
        self.taps = -(-(2 * self.half + 1) // self.L)           # non-zero taps of an output, at most
        self.bank = torch.from_numpy(bank).to(self.device)
        self.chunk_outputs = int(chunk_outputs)

    def __call__(self, x, chunk_outputs=None):
        from ._lib import call, ptr, stream
        x = _frames(x)
        T, C = x.shape
        if self.L == self.M and C == 1 and x.dtype == torch.int16:
            x = x.reshape(-1).to(self.device)
            return x if self.out_dtype == torch.int16 else x.to(torch.float32) * (1.0 / 32768.0)
        chunk = int(chunk_outputs if chunk_outputs is not None else self.chunk_outputs)
        if chunk < 1:
            raise ValueError(f'chunk_outputs must be positive (got {chunk})')
        L, M, F, Kp = self.L, self.M, self.F, self.Kp
        n_out = output_length(T, L, M)
        y = torch.empty(n_out, dtype=self.out_dtype, device=self.device)
        with torch.cuda.device(self.device):
            for m0 in range(0, n_out, chunk):
                m1 = min(n_out, m0 + chunk)
                lo = max(0, m0 * M // L - F)
                hi = min(T, (m1 - 1) * M // L - F + Kp)
                part = x[lo:hi].to(self.device, non_blocking=True)
                call('rv_resample', ptr(part), IN_DTYPES[x.dtype][0], hi - lo, C, lo, ptr(self.bank), L, M, F, Kp,
                     y.data_ptr() + m0 * y.element_size(), OUT_DTYPES[self.out_dtype], m0, m1 - m0, stream())
                part.record_stream(torch.cuda.current_stream())
        return y


def _mono64(x):
    x = np.asarray(x)
    if x.dtype == np.int16:
        scale = 2.0 ** -15
    elif x.dtype == np.int32:
        scale = 2.0 ** -31
    elif x.dtype in (np.float32, np.float64):
        scale = 1.0
    else:
        raise ValueError(f'sample type {x.dtype}: expected int16, int32 or float32')
    if x.ndim == 1:
        x = x[:, None]
    if x.ndim != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f'expected a non-empty [T] or [T, C] signal, got shape {x.shape}')
    return x.astype(np.float64).mean(axis=1) * scale


def resample_host(x, sr_in, sr_out, out_dtype=np.float64, zeros=ZEROS, rolloff=ROLLOFF, beta=BETA, workers=None, chunk_outputs=1 << 20):
    """The definition above in float64 on the host: x a numpy array [T] or [T, C] (int16, int32, float32 or float64) ->
    [ceil(T L / M)] float64 / float32, or int16 with the device path's rounding.  The float64 filter is used unrounded.
    Output chunks run on `workers` threads (default: OMP_NUM_THREADS, else the CPU count, at most 16)."""
    from scipy.signal import upfirdn
    x = np.asarray(x)
    out_dtype = np.dtype(out_dtype)
    if x.dtype == np.int16 and (x.ndim == 1 or x.shape[1] == 1) and int(sr_in) == int(sr_out):
        x = x.reshape(-1)
        return x if out_dtype == np.int16 else (x.astype(np.float64) * 2.0 ** -15).astype(out_dtype)
    L, M, half, h = _design64(sr_in, sr_out, zeros, rolloff, beta)
    if x.ndim == 1:
        x = x[:, None]
    T = x.shape[0]
    _mono64(x[:1])                                                              # argument checks before any work
    n_out = output_length(T, L, M)
    reach = half // L + 1                                                       # input frames an output can see on either side

    def piece(m0):
        m1 = min(n_out, m0 + chunk_outputs)
        lo, hi = max(0, m0 * M // L - reach), min(T, (m1 - 1) * M // L + reach + 1)
        # the full convolution of the slice holds output m at index half + m M - lo L; upfirdn(.., L, M) keeps every M-th index
        # from 0 on, so delay the filter until output m0 lands on a multiple of M
        s0 = half + m0 * M - lo * L
        lead = (-s0) % M
        full = upfirdn(np.concatenate([np.zeros(lead), h]), _mono64(x[lo:hi]), L, M)
        j0 = (s0 + lead) // M
        out = np.zeros(m1 - m0)
        got = full[j0:j0 + m1 - m0]
        out[:len(got)] = got
        return out
    starts = list(range(0, n_out, chunk_outputs))
    if workers is None:
        workers = min(16, int(os.environ.get('OMP_NUM_THREADS') or os.cpu_count() or 1))
    if len(starts) == 1 or workers <= 1:
        parts = [piece(m0) for m0 in starts]
    else:
        with ThreadPoolExecutor(max_workers=workers) as ex:
            parts = list(ex.map(piece, starts))
    y = np.concatenate(parts)
    if out_dtype == np.int16:
        return np.clip(np.rint(y * 32768.0), -32768, 32767).astype(np.int16)
    return y.astype(out_dtype, copy=False)
