"""Score-to-recording alignment: a recording and a score of the same piece that is NOT time-aligned to it become aligned
labels, by dynamic time warping between the recording's features and those of the score rendered by reconvat_amd/synth.py.

Definition (everything here, `rv_align_cost` / `rv_align_dtw` in csrc/align.hip and the tests implement exactly this):

  features   per frame (hop 512, 1 + nsamp // 512 frames, the front end's log-Mel over 229 bands): f = max(log(mel + 1e-5) - log(1e-5), 0);
             one constant component KAPPA = 8 is appended (D = 230) and the row is scaled to unit L2 norm -- the constant makes silence
             match silence at cost 0 instead of 0/0.  Coarse features: the un-normalised f averaged over S consecutive frames (tail
             dropped), then constant and norm.
  band       rows i = recording frames (N), columns j = score frames (M); row i owns the columns lo[i] .. lo[i] + W - 1, cut off at M;
             lo is non-decreasing, lo[0] = 0; the full matrix is lo = 0, W = M.
  cost       c[i, k] = rint(clip(1 - <x_i, y_(lo[i] + k)>, 0, 1) * 4095), uint16 [N][W]; 0xFFFF where lo[i] + k >= M (never read).
  recurrence D[0, 0] = 2 c;  D[i, j] = min(D[i-1, j-1] + 2 c, D[i-1, j] + c, D[i, j-1] + c) over the cells of the band, in uint32; a
             predecessor outside the band or the matrix is +inf.  Direction code per cell, uint8 [N][W]: 0 diagonal, 1 from (i-1, j),
             2 from (i, j-1), 3 unreachable / start; TIES GO TO THE LOWEST CODE.  Twelve-bit costs and N + M <= 2^18 keep every sum
             below 2^30; a larger pair is refused, not wrapped.
  path       walked back from (N-1, M-1) to (0, 0); reported as row_lo / row_hi [N] (lowest / highest column of the path per row),
             col_lo / col_hi [M] (lowest / highest row per column), its length and total = D[N-1, M-1].  A band that does not connect
             the corners: total = 0xFFFFFFFF, length 0, the four arrays -1; the Python layer raises a ValueError.
  two passes full DTW on the coarse features (S = `coarse`, doubled until the coarse score has at most 8192 frames), then with R = radius
             W = min(2 R + S + 1, M),  lo[i] = clip(S row_lo_c[min(i // S, N_c - 1)] - R, 0, max(M - W, 0)), made non-decreasing by a
             running maximum, lo[0] = 0 -- and banded DTW at full resolution.  A pair with fewer than two coarse frames on a side is
             aligned on the full matrix directly.
  time map   score time t (s) -> interp(t 16000 / 512, arange(M), col_lo) 512 / 16000: onsets and offsets both, an offset at least one
             frame after its onset, times clipped to the recording; pitches and velocities untouched.

`dtw_host` and `cost_host` are the yardstick (NumPy float64 and integers; they run where there is no GPU).  On a HIP device the log-Mel
comes from the fused front end, the cost matrix from rv_align_cost (f32 matrix pipe: a cell may differ from the yardstick's by 1) and
recurrence and backtrack from rv_align_dtw, whose integers equal dtw_host's on the same cost matrix.  A folder goes through one batched
launch per stage.  No accuracy on real recordings is claimed anywhere: only rendered pairs exist where this was written.
"""
import os

import numpy as np
import torch

from .constants import HOP_LENGTH, SAMPLE_RATE, N_BINS, MEL_FMIN, MEL_FMAX, WINDOW_LENGTH

KAPPA = 8.0
QUANT = 4095
DEAD = 0xFFFF
SENTINEL = 0xFFFFFFFF
MAX_W = 8192
MAX_NM = 1 << 18
FLOOR = float(np.log(1e-5))
FRAME_S = HOP_LENGTH / SAMPLE_RATE
DESC = 9                    # int64 words per pair in the device table
HEAD = 4                    # int32 words before the path arrays of a pair's output


# ------------------------------------------------------------------------------------------------------------------
# features
# ------------------------------------------------------------------------------------------------------------------
_MEL_BASIS = []


def logmel_host(audio):
    """int16 (or float in [-1, 1)) samples [n] -> log(mel + 1e-5) float64 [1 + n // 512, 229]: the front end restated in float64
    (reflect padding, periodic Hann, 2048-point DFT, power, Slaney filterbank)."""
    from .frontend import _hann, slaney_mel_basis
    x = np.asarray(audio)
    x = x.astype(np.float64) / 32768.0 if x.dtype.kind in 'iu' else x.astype(np.float64)
    if x.ndim != 1 or len(x) <= WINDOW_LENGTH // 2:
        raise ValueError(f'align: a signal of more than {WINDOW_LENGTH // 2} samples is needed (got shape {x.shape})')
    if not _MEL_BASIS:
        _MEL_BASIS.append(slaney_mel_basis(SAMPLE_RATE, WINDOW_LENGTH, N_BINS, MEL_FMIN, MEL_FMAX).astype(np.float64))
    T = 1 + len(x) // HOP_LENGTH
    xp = np.pad(x, WINDOW_LENGTH // 2, mode='reflect')
    win = _hann(WINDOW_LENGTH)
    out = np.empty((T, N_BINS))
    for t0 in range(0, T, 1024):
        idx = (np.arange(t0, min(t0 + 1024, T)) * HOP_LENGTH)[:, None] + np.arange(WINDOW_LENGTH)[None, :]
        power = np.abs(np.fft.rfft(xp[idx] * win, axis=1)) ** 2
        out[t0:t0 + len(idx)] = np.log(power @ _MEL_BASIS[0].T + 1e-5)
    return out


def features(logmel, S=1):
    """log(mel + 1e-5) [T, 229] (NumPy or torch, any float type) -> unit rows [T // S, 230] of the same kind."""
    lib = torch if torch.is_tensor(logmel) else np
    f = lib.clip(logmel - FLOOR, 0.0, None)
    if S > 1:
        T = f.shape[0] // S
        f = f[:T * S].reshape(T, S, f.shape[1]).mean(1)
    if torch.is_tensor(f):
        f = torch.cat([f, torch.full((f.shape[0], 1), KAPPA, dtype=f.dtype, device=f.device)], 1)
        return f / torch.linalg.vector_norm(f, dim=1, keepdim=True)
    f = np.concatenate([f, np.full((f.shape[0], 1), KAPPA, dtype=f.dtype)], 1)
    return f / np.sqrt((f * f).sum(1, keepdims=True))


_MELS = {}


def logmel(audio, device='cpu'):
    """log(mel + 1e-5) [T, 229] of int16 samples: the fused front end on a HIP device (float32 tensor), `logmel_host` elsewhere."""
    device = torch.device(device)
    if device.type != 'cuda':
        return logmel_host(audio)
    from .frontend import MelSpectrogram
    key = str(device)
    if key not in _MELS:
        _MELS[key] = MelSpectrogram().to(device)
    a = audio if torch.is_tensor(audio) else torch.from_numpy(np.ascontiguousarray(audio))
    a = a.to(device)
    a = a.to(torch.float32) * (1.0 / 32768.0) if not a.is_floating_point() else a.to(torch.float32)
    if a.dim() != 1 or a.numel() <= WINDOW_LENGTH // 2:
        raise ValueError(f'align: a signal of more than {WINDOW_LENGTH // 2} samples is needed (got shape {tuple(a.shape)})')
    with torch.cuda.device(device), torch.no_grad():
        return _MELS[key].lognorm(a[None, :], log=True, normalise=False)[0, 0]


# ------------------------------------------------------------------------------------------------------------------
# the yardstick
# ------------------------------------------------------------------------------------------------------------------
def _check_band(N, M, lo, W, name='pair'):
    lo = np.asarray(lo, dtype=np.int64).reshape(-1)
    if N < 1 or M < 1:
        raise ValueError(f'align: {name}: an empty side ({N} x {M} frames)')
    if N + M > MAX_NM:
        raise ValueError(f'align: {name}: {N} + {M} frames; N + M is at most 2^18 = {MAX_NM} (sums of twelve-bit costs must stay below '
                         '2^30), about 70 minutes a side: cut the piece into movements')
    if not 1 <= W <= min(M, MAX_W):
        raise ValueError(f'align: {name}: a band of {W} columns; 1 .. min(M = {M}, {MAX_W}) are possible')
    if len(lo) != N or lo[0] != 0 or (np.diff(lo) < 0).any() or lo[-1] >= M:
        raise ValueError(f'align: {name}: lo must hold {N} non-decreasing columns below {M}, the first 0')
    return lo


def cost_host(X, Y, lo, W, dtype=np.float64):
    """The banded cost matrix uint16 [N][W] of unit rows X [N, D], Y [M, D], evaluated in `dtype` (float64: the yardstick)."""
    X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
    N, M = len(X), len(Y)
    lo = _check_band(N, M, lo, W)
    cols = lo[:, None] + np.arange(W)[None, :]
    live = cols < M
    out = np.full((N, W), DEAD, dtype=np.uint16)
    for i0 in range(0, N, 64):                                # dense products over the columns a block of rows spans, then the band's cells
        sl = slice(i0, min(i0 + 64, N))
        c0, c1 = int(lo[sl.start]), int(min(lo[sl.stop - 1] + W, M))
        dot = np.take_along_axis(X[sl] @ Y[c0:c1].T, np.minimum(cols[sl], M - 1) - c0, axis=1)
        q = np.rint(np.clip(dtype(1.0) - dot, dtype(0.0), dtype(1.0)) * dtype(QUANT)).astype(np.uint16)
        out[sl][live[sl]] = q[live[sl]]
    return out


def _infer_M(cost, lo):
    return int(lo[-1]) + int((np.asarray(cost)[-1] != DEAD).sum())


def dtw_host(cost, lo, W, M=None):
    """Recurrence and backtrack of the definition over a cost matrix uint16 [N][W], vectorised over anti-diagonals.  `M`: the number
    of columns (default: where the last row's live cells end).  Returns a dict: total, length, row_lo, row_hi, col_lo, col_hi (int32)
    and dirs uint8 [N][W] (3 in every cell that is unreachable or outside the matrix)."""
    cost = np.asarray(cost)
    N = cost.shape[0]
    lo64 = np.asarray(lo, dtype=np.int64).reshape(-1)
    M = _infer_M(cost, lo64) if M is None else int(M)
    if cost.shape != (N, W):
        raise ValueError(f'align: a cost matrix of shape {cost.shape} for W = {W}')
    lo = _check_band(N, M, lo64, W)
    INF = np.int64(SENTINEL)
    hi = np.minimum(lo + W, M)
    rows = np.arange(N, dtype=np.int64)
    a, b = rows + lo, rows + hi                               # row i is on the diagonals a[i] <= d < b[i]: both strictly increasing
    ds = np.arange(N + M - 1, dtype=np.int64)
    imax = np.searchsorted(a, ds, side='right') - 1
    imin = np.searchsorted(b, ds, side='right')
    Dm = np.full((N, W), INF, dtype=np.int64)
    dirs = np.full((N, W), 3, dtype=np.uint8)
    c64 = cost.astype(np.int64)
    lo_p = np.concatenate([[0], lo[:-1]])
    hi_p = np.concatenate([[0], hi[:-1]])                      # row -1 owns no column
    Dm[0, 0] = 2 * c64[0, 0]
    for d in range(1, N + M - 1):
        i = rows[imin[d]:imax[d] + 1]
        if not len(i):
            continue
        j = d - i
        k = j - lo[i]
        c = c64[i, k]
        ip = np.maximum(i - 1, 0)
        kp = j - lo_p[i]                                      # column j in the previous row's band
        in_up = (j >= lo_p[i]) & (j < hi_p[i])
        in_dg = (j - 1 >= lo_p[i]) & (j - 1 < hi_p[i])
        up = np.where(in_up, Dm[ip, np.clip(kp, 0, W - 1)], INF)
        dg = np.where(in_dg, Dm[ip, np.clip(kp - 1, 0, W - 1)], INF)
        lf = np.where(k >= 1, Dm[i, np.maximum(k - 1, 0)], INF)
        best = np.where(dg == INF, INF, dg + 2 * c)
        code = np.where(dg == INF, 3, 0)
        vu = np.where(up == INF, INF, up + c)
        t = vu < best
        best, code = np.where(t, vu, best), np.where(t, 1, code)
        vl = np.where(lf == INF, INF, lf + c)
        t = vl < best
        best, code = np.where(t, vl, best), np.where(t, 2, code)
        Dm[i, k] = best
        dirs[i, k] = code
    res = dict(N=N, M=M, W=int(W), dirs=dirs)
    k_last = M - 1 - lo[-1]
    total = int(Dm[N - 1, k_last]) if k_last < W else SENTINEL
    arrays = [np.full(n, -1, dtype=np.int32) for n in (N, N, M, M)]
    length = 0
    if total != SENTINEL:
        row_lo, row_hi, col_lo, col_hi = arrays
        i, j = N - 1, M - 1
        row_hi[i], col_hi[j] = j, i
        while True:
            row_lo[i], col_lo[j] = j, i
            length += 1
            if i == 0 and j == 0:
                break
            code = int(dirs[i, j - lo[i]])
            assert code < 3 and (code == 2 or i > 0) and (code == 1 or j > 0)
            if code != 2:
                i -= 1
            if code != 1:
                j -= 1
            if code != 2:
                row_hi[i] = j
            if code != 1:
                col_hi[j] = i
    res.update(total=total, length=length, row_lo=arrays[0], row_hi=arrays[1], col_lo=arrays[2], col_hi=arrays[3])
    return res


# ------------------------------------------------------------------------------------------------------------------
# the device path: one launch per stage for a batch of pairs
# ------------------------------------------------------------------------------------------------------------------
class _Layout:
    """Offsets of a batch of pairs in the shared buffers, and the int64 table the kernels read."""

    def __init__(self, Ns, Ms, Ws, D=0):
        self.Ns, self.Ms, self.Ws, self.D = [int(n) for n in Ns], [int(m) for m in Ms], [int(w) for w in Ws], int(D)
        self.P = len(self.Ns)
        table = np.zeros((self.P, DESC), dtype=np.int64)
        feat = row = cell = out = 0
        for p, (N, M, W) in enumerate(zip(self.Ns, self.Ms, self.Ws)):
            table[p] = (N, M, W, feat, feat + N * self.D, row, cell, cell, out)
            feat += (N + M) * self.D
            row += N
            cell += N * W
            out += HEAD + 2 * (N + M)
        self.table, self.n_feats, self.n_lo, self.n_cells, self.n_out = table, feat, row, cell, out
        self.max_n, self.max_w, self.max_nm = max(self.Ns), max(self.Ws), max(n + m for n, m in zip(self.Ns, self.Ms))

    def split_cells(self, flat):
        """The per-pair [N, W] views of a flat cost or direction buffer."""
        at, parts = 0, []
        for N, W in zip(self.Ns, self.Ws):
            parts.append(flat[at:at + N * W].reshape(N, W))
            at += N * W
        return parts


def _lo_tensor(los, device):
    return torch.from_numpy(np.concatenate([np.asarray(l, dtype=np.int32).reshape(-1) for l in los])).to(device)


def cost_device(pairs, los, Ws, device):
    """rv_align_cost over a batch: pairs = [(X [N, D], Y [M, D])] (float tensors on `device`, or arrays), los / Ws the bands.
    Returns (flat uint16 cost tensor on the device, layout)."""
    from ._lib import call, ptr, stream
    device = torch.device(device)
    as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(device=device, dtype=torch.float32)
    pairs = [(as_t(x), as_t(y)) for x, y in pairs]
    D = pairs[0][0].shape[1]
    if any(x.dim() != 2 or y.dim() != 2 or x.shape[1] != D or y.shape[1] != D for x, y in pairs):
        raise ValueError('align: every feature matrix of a batch must be [frames, D] with one D')
    lay = _Layout([len(x) for x, _ in pairs], [len(y) for _, y in pairs], Ws, D)
    for p, l in enumerate(los):
        _check_band(lay.Ns[p], lay.Ms[p], l, lay.Ws[p], f'pair {p}')
    with torch.cuda.device(device):
        feats = torch.cat([t.reshape(-1) for x, y in pairs for t in (x, y)])
        lo = _lo_tensor(los, device)
        desc = torch.from_numpy(lay.table).to(device)
        cost = torch.empty(lay.n_cells, dtype=torch.int16, device=device)              # the bits of uint16
        call('rv_align_cost', ptr(desc), lay.P, D, lay.max_n, lay.max_w, ptr(feats), feats.numel(), ptr(lo), lo.numel(),
             ptr(cost), cost.numel(), stream())
    return cost, lay


def dtw_device(cost, los, Ws, Ms, device, keep_dirs=False):
    """rv_align_dtw over a batch.  cost: the flat tensor of `cost_device`, or a list of uint16 arrays [N][W].  Returns one dict per
    pair (total, length, the four path arrays; dirs uint8 [N][W] -- cells the kernel did not write hold 3 -- with `keep_dirs`)."""
    from ._lib import call, ptr, stream
    device = torch.device(device)
    if not torch.is_tensor(cost):
        Ns = [np.asarray(c).shape[0] for c in cost]
        cost = torch.from_numpy(np.concatenate([np.ascontiguousarray(c, dtype=np.uint16).reshape(-1) for c in cost]).view(np.int16))
    else:
        Ns = [len(l) for l in los]
    lay = _Layout(Ns, Ms, Ws)
    for p, l in enumerate(los):
        _check_band(lay.Ns[p], lay.Ms[p], l, lay.Ws[p], f'pair {p}')
    if cost.numel() != lay.n_cells:
        raise ValueError(f'align: {cost.numel()} cost cells for bands of {lay.n_cells}')
    with torch.cuda.device(device):
        cost = cost.to(device)
        lo = _lo_tensor(los, device)
        desc = torch.from_numpy(lay.table).to(device)
        dirs = torch.full((lay.n_cells,), 3, dtype=torch.uint8, device=device)
        out = torch.zeros(lay.n_out, dtype=torch.int32, device=device)
        call('rv_align_dtw', ptr(desc), lay.P, lay.max_nm, lay.max_w, ptr(lo), lo.numel(), ptr(cost), cost.numel(), ptr(dirs),
             dirs.numel(), ptr(out), out.numel(), stream())
        out = out.cpu().numpy()
        dirs = lay.split_cells(dirs.cpu().numpy()) if keep_dirs else None
    results, at = [], 0
    for p, (N, M, W) in enumerate(zip(lay.Ns, lay.Ms, lay.Ws)):
        head, body = out[at:at + HEAD], out[at + HEAD:at + HEAD + 2 * (N + M)]
        at += HEAD + 2 * (N + M)
        if head[2] != 0:
            raise RuntimeError(f'rv_align_dtw: pair {p} ({N} x {M}, W = {W}) was refused by the kernel (status {int(head[2])})')
        res = dict(N=N, M=M, W=W, total=int(np.uint32(head[0])), length=int(head[1]), row_lo=body[:N].copy(), row_hi=body[N:2 * N].copy(),
                   col_lo=body[2 * N:2 * N + M].copy(), col_hi=body[2 * N + M:].copy())
        if keep_dirs:
            res['dirs'] = dirs[p]
        results.append(res)
    return results


def dtw_pairs(pairs, los, Ws, device='cpu', names=None):
    """Cost matrix and DTW of a batch of feature pairs under the given bands: the kernels on a HIP device, the yardstick elsewhere.
    Raises a ValueError that names the pair if a band does not connect its corners."""
    device = torch.device(device)
    Ms = [len(y) for _, y in pairs]
    if device.type == 'cuda':
        cost, _ = cost_device(pairs, los, Ws, device)
        results = dtw_device(cost, los, Ws, Ms, device)
    else:
        to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else a
        results = [dtw_host(cost_host(to_np(x), to_np(y), l, W), l, W, len(y)) for (x, y), l, W in zip(pairs, los, Ws)]
    for p, r in enumerate(results):
        if r['total'] == SENTINEL:
            name = names[p] if names else f'pair {p}'
            raise ValueError(f'align: {name}: the band of {r["W"]} columns does not connect the first and the last frames of recording '
                             f'({r["N"]} frames) and score ({r["M"]} frames); use a wider radius (radius_s)')
    return results


# ------------------------------------------------------------------------------------------------------------------
# coarse to fine
# ------------------------------------------------------------------------------------------------------------------
def coarse_factor(M, S=8):
    """`S` doubled until the coarse score (M // S frames, the width of the full coarse matrix) has at most 8192 frames."""
    S = max(int(S), 1)
    while M // S > MAX_W:
        S *= 2
    return S


def band_from_coarse(row_lo_c, N, M, S, R):
    """(lo int32 [N], W): the band of radius R frames around a coarse path given by its lowest column per coarse row."""
    row_lo_c = np.asarray(row_lo_c, dtype=np.int64)
    W = min(2 * R + S + 1, M)
    lo = np.clip(S * row_lo_c[np.minimum(np.arange(N) // S, len(row_lo_c) - 1)] - R, 0, max(M - W, 0))
    lo = np.maximum.accumulate(lo)
    lo[0] = 0
    return lo.astype(np.int32), int(W)


def align_logmels(pairs, coarse=8, radius=125, device='cpu', names=None):
    """pairs = [(log-Mel of the recording [N, 229], log-Mel of the score [M, 229])] -> one result dict per pair (`dtw_host`'s keys
    plus S, lo and `coarse_inside`: whether every coarse path cell's fine cells lie inside the band).  Two batched passes."""
    P = len(pairs)
    names = names or [f'pair {p}' for p in range(P)]
    R = int(radius)
    if R < 1:
        raise ValueError(f'align: radius must be at least one frame (got {radius})')
    shapes = [(x.shape[0], y.shape[0]) for x, y in pairs]
    for (N, M), name in zip(shapes, names):
        if N + M > MAX_NM:
            raise ValueError(f'align: {name}: {N} + {M} frames; N + M is at most 2^18 = {MAX_NM}: cut the piece into movements')
    Ss = [coarse_factor(M, coarse) for _, M in shapes]
    two = [N // S >= 2 and M // S >= 2 and min(2 * R + S + 1, M) < M for (N, M), S in zip(shapes, Ss)]
    los, Ws, inside = [None] * P, [None] * P, [True] * P
    idx = [p for p in range(P) if two[p]]
    if idx:
        cpairs = [(features(pairs[p][0], Ss[p]), features(pairs[p][1], Ss[p])) for p in idx]
        cres = dtw_pairs(cpairs, [np.zeros(len(x), dtype=np.int32) for x, _ in cpairs], [len(y) for _, y in cpairs], device,
                         [names[p] + ' (coarse pass)' for p in idx])
        for p, r in zip(idx, cres):
            N, M = shapes[p]
            los[p], Ws[p] = band_from_coarse(r['row_lo'], N, M, Ss[p], R)
            inside[p] = bool((Ss[p] * (r['row_hi'] - r['row_lo']) <= R + 1).all())
    for p in range(P):
        if not two[p]:
            N, M = shapes[p]
            if M > MAX_W:
                raise ValueError(f'align: {names[p]}: a score of {M} frames against a recording of {N}: too short a recording for a coarse pass')
            los[p], Ws[p], Ss[p] = np.zeros(N, dtype=np.int32), M, 1
    results = dtw_pairs([(features(x), features(y)) for x, y in pairs], los, Ws, device, names)
    for p, r in enumerate(results):
        r.update(S=Ss[p], lo=los[p], coarse_inside=inside[p])
    return results


def align_frames(X_logmel, Y_logmel, coarse=8, radius=125, device='cpu'):
    """One pair: see `align_logmels`."""
    return align_logmels([(X_logmel, Y_logmel)], coarse, radius, device)[0]


# ------------------------------------------------------------------------------------------------------------------
# scores
# ------------------------------------------------------------------------------------------------------------------
def map_times(t, col_lo):
    """Score times (s) -> recording times (s) through the path's lowest row per score frame."""
    col_lo = np.asarray(col_lo, dtype=np.float64)
    return np.interp(np.asarray(t, dtype=np.float64) / FRAME_S, np.arange(len(col_lo)), col_lo) * FRAME_S


def map_notes(notes, col_lo, n_samples):
    """tsv rows (onset, offset, note, velocity) in score time -> the same rows in recording time."""
    notes = np.array(notes, dtype=np.float64).reshape(-1, 4)
    end = n_samples / SAMPLE_RATE
    on = np.clip(map_times(notes[:, 0], col_lo), 0.0, end)
    off = np.clip(np.maximum(map_times(notes[:, 1], col_lo), on + FRAME_S), 0.0, end)
    notes[:, 0], notes[:, 1] = on, off
    return notes


def score_length(notes):
    """Samples a score is rendered to: its last offset and a second more."""
    notes = np.asarray(notes, dtype=np.float64).reshape(-1, 4)
    if not len(notes):
        raise ValueError('align: an empty score')
    return int(np.ceil(notes[:, 1].max() * SAMPLE_RATE)) + SAMPLE_RATE


def align_scores(items, timbre=None, device='cpu', radius_s=4.0, coarse=8, names=None):
    """items = [(recording int16 [n], score tsv rows)] -> [(aligned tsv rows, report)], every stage batched over the items.
    report: N, M, S, W, total, length, mean_cost (per path step, in [0, 1]) and coarse_inside."""
    from . import synth
    timbre = timbre or synth.Timbre('struck', 0)
    device = torch.device(device)
    radius = int(round(radius_s / FRAME_S))
    pairs = []
    for rec, notes in items:
        rec = rec.cpu().numpy() if torch.is_tensor(rec) else np.asarray(rec)
        audio = synth.render(np.asarray(notes, dtype=np.float64).reshape(-1, 4), score_length(notes), timbre, device=device, out_dtype=torch.int16)
        pairs.append((logmel(rec, device), logmel(audio if device.type == 'cuda' else audio.numpy(), device)))
    results = align_logmels(pairs, coarse, radius, device, names)
    out = []
    for (rec, notes), r in zip(items, results):
        # a cell costs c (a side step) or 2 c (a diagonal step and the start cell): the weights of a path add up to N + M
        report = dict(N=r['N'], M=r['M'], S=r['S'], W=r['W'], total=r['total'], length=r['length'],
                      mean_cost=r['total'] / (QUANT * float(r['N'] + r['M'])), coarse_inside=r['coarse_inside'])
        out.append((map_notes(notes, r['col_lo'], len(rec)), report))
    return out


def align_score(recording_int16, score_rows, timbre=None, device='cpu', radius_s=4.0, coarse=8):
    """One recording (16 kHz mono int16) and its score (tsv rows in score time) -> (aligned tsv rows, report).  The score is rendered
    by synth.render (default timbre: Timbre('struck', 0)) to its last offset + 1 s."""
    return align_scores([(recording_int16, score_rows)], timbre, device, radius_s, coarse)[0]


# ------------------------------------------------------------------------------------------------------------------
# folders
# ------------------------------------------------------------------------------------------------------------------
SCORE_SUFFIXES = ('.mid', '.midi', '.score.tsv')
TSV_HEADER = 'onset,offset,note,velocity'


def read_score(path):
    if path.endswith('.tsv'):
        return np.loadtxt(path, delimiter='\t', skiprows=1, ndmin=2).reshape(-1, 4)
    from .midi import parse_midi
    return np.asarray(parse_midi(path), dtype=np.float64).reshape(-1, 4)


def folder_pairs(folder):
    """(scored, unscored): [(name, wav path, score path)] for every name.wav with name.mid / .midi / .score.tsv beside it, and the
    wav paths that have none; both sorted."""
    scored, unscored = [], []
    for f in sorted(os.listdir(folder)):
        if not f.endswith('.wav'):
            continue
        stem = os.path.join(folder, f[:-4])
        score = next((stem + s for s in SCORE_SUFFIXES if os.path.exists(stem + s)), None)
        if score is None:
            unscored.append(stem + '.wav')
        else:
            scored.append((f[:-4], stem + '.wav', score))
    return scored, unscored


def write_tsv(path, notes):
    """tsv rows with the corpora's header line; the file appears in one step (written beside itself, then renamed)."""
    part = f'{path}.{os.getpid()}.part'
    np.savetxt(part, np.asarray(notes, dtype=np.float64).reshape(-1, 4), fmt='%.6f', delimiter='\t', header=TSV_HEADER)
    os.replace(part, path)


def align_folder(input, output=None, radius_s=4.0, coarse=8, device='cpu', overwrite=False, timbre=None, log=print):
    """Every scored recording of `input` aligned in one batch; writes `output`/name.tsv (default: beside the recording) and returns
    [(name, tsv path, report)].  An existing name.tsv is an error unless `overwrite`."""
    from .dataset import read_audio_int16
    scored, _ = folder_pairs(input)
    if not scored:
        raise ValueError(f'{input}: no name.wav with a name.mid, name.midi or name.score.tsv beside it')
    output = output or input
    os.makedirs(output, exist_ok=True)
    targets = [os.path.join(output, name + '.tsv') for name, _, _ in scored]
    taken = [t for t in targets if os.path.exists(t)]
    if taken and not overwrite:
        raise FileExistsError(f'{taken[0]} exists ({len(taken)} of {len(targets)} do); pass overwrite=True to replace them')
    items = [(read_audio_int16(wav, device), read_score(score)) for _, wav, score in scored]
    done = align_scores(items, timbre, device, radius_s, coarse, [name for name, _, _ in scored])
    out = []
    for (name, _, _), target, (notes, report) in zip(scored, targets, done):
        write_tsv(target, notes)
        log(f'{name}: N={report["N"]} M={report["M"]} S={report["S"]} W={report["W"]} total={report["total"]} '
            f'length={report["length"]} mean_cost={report["mean_cost"]:.4f}' + ('' if report['coarse_inside'] else ' (coarse path left the band)'))
        out.append((name, target, report))
    return out
