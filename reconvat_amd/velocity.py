"""Note velocities from the spectrogram: a small head that shares its weights across the 88 keys and looks, for the
cell (frame t, key p), at the spectrogram bins nearest to the first eight harmonics of the key over four frames around the onset.

This module is the definition and runs without a GPU; csrc/velocity.hip computes the same on the device (ops.velocity_roll,
ops.velocity_loss) and the tests hold the kernels to what is written here.

    f0(p)      = 440 * 2^((p + 21 - 69) / 12)                                        p = 0..87
    tab[p, k]  = argmin_i |centres[i] - (k + 1) f0(p)|  (first index on ties),  -1 where (k + 1) f0(p) > max(centres)     k = 0..7
    x[8 j + k] = spec[b, clamp(t - 1 + j, 0, T - 1), tab[p, k]]  (0 where tab[p, k] = -1),  j = 0..3;     x[32] = p / 88
    v^         = sigmoid(b2 + sum_h w2[h] sigmoid(b1[h] + sum_i w1[h, i] x[i]))        in the corpus's unit, velocity / 128
    loss       = sum m (v^ - target)^2 / sum m  over all B T 88 cells;  0 with zero gradient when sum m = 0

The flat parameter vector is w1 [32, 33] row-major, b1 [32], w2 [32], b2: 1121 floats.  The spectrogram gets no gradient."""
import numpy as np
import torch
from torch import nn

from .constants import MIN_MIDI, SAMPLE_RATE, WINDOW_LENGTH

N_KEYS, N_HARMONICS, N_CONTEXT, N_HIDDEN = 88, 8, 4, 32
N_INPUTS = N_CONTEXT * N_HARMONICS + 1                       # 33
N_PARAMS = N_HIDDEN * N_INPUTS + N_HIDDEN + N_HIDDEN + 1     # 1121
SPEC_KINDS = ('Mel', 'CQT')


def key_frequencies():
    return 440.0 * 2.0 ** ((np.arange(N_KEYS, dtype=np.float64) + MIN_MIDI - 69.0) / 12.0)


def harmonic_bins(centres):
    """float64 [n_bins] centre frequencies -> int32 [88, 8]: the bin nearest to harmonic k + 1 of key p, -1 above the highest centre."""
    centres = np.asarray(centres, dtype=np.float64).reshape(-1)
    if centres.size < 1:
        raise ValueError('harmonic_bins: no centre frequencies')
    target = key_frequencies()[:, None] * np.arange(1, N_HARMONICS + 1, dtype=np.float64)[None, :]
    tab = np.abs(centres[None, None, :] - target[:, :, None]).argmin(axis=2).astype(np.int32)        # argmin: first index on ties
    tab[target > centres.max()] = -1
    return tab


def mel_centres(mel_basis):
    """The FFT bin at which each row of a mel filterbank [n_mels, n_fft / 2 + 1] peaks, in Hz."""
    basis = torch.as_tensor(mel_basis).detach().cpu().numpy()
    return basis.argmax(axis=1).astype(np.float64) * (SAMPLE_RATE / WINDOW_LENGTH)


def cqt_centres(fmin, bins_per_octave, n_bins):
    """Centre frequencies of CQT1992v2's bins (frontend.create_cqt_kernels: fmin 2^(k / bins_per_octave))."""
    return float(fmin) * 2.0 ** (np.arange(int(n_bins), dtype=np.float64) / float(bins_per_octave))


def front_end_centres(model):
    """(spec kind, centres) of a model's front end: its `mel_basis` buffer, or the parameters its CQT1992v2 was built with."""
    sg = model.spectrogram
    if hasattr(sg, 'mel_basis'):
        return 'Mel', mel_centres(sg.mel_basis)
    return 'CQT', cqt_centres(sg.fmin, sg.bins_per_octave, sg.n_bins)


def features(spec, tab):
    """x [B, T, 88, 33] of a spectrogram [B, T, n_bins] (torch, in the dtype and on the device of `spec`)."""
    if spec.dim() != 3:
        raise ValueError(f'expected a [B, T, n_bins] spectrogram, got {tuple(spec.shape)}')
    B, T, _ = spec.shape
    tab_t = torch.as_tensor(np.asarray(tab), dtype=torch.long, device=spec.device)
    frames = (torch.arange(T, device=spec.device)[:, None] - 1 + torch.arange(N_CONTEXT, device=spec.device)[None, :]).clamp(0, T - 1)
    g = spec[:, frames][..., tab_t.clamp_min(0).reshape(-1)]                                         # [B, T, 4, 704]
    g = g.reshape(B, T, N_CONTEXT, N_KEYS, N_HARMONICS) * (tab_t >= 0).to(spec.dtype)
    g = g.permute(0, 1, 3, 2, 4).reshape(B, T, N_KEYS, N_CONTEXT * N_HARMONICS)
    key = (torch.arange(N_KEYS, device=spec.device, dtype=torch.float64) / N_KEYS).to(spec.dtype)
    return torch.cat([g, key.expand(B, T, N_KEYS)[..., None]], dim=-1)


def unpack(params):
    """flat [1121] -> (w1 [32, 33], b1 [32], w2 [32], b2 [])"""
    a, b = N_HIDDEN * N_INPUTS, N_HIDDEN * N_INPUTS + N_HIDDEN
    return params[:a].reshape(N_HIDDEN, N_INPUTS), params[a:b], params[b:b + N_HIDDEN], params[b + N_HIDDEN]


def roll_torch(spec, tab, params):
    """v^ [B, T, 88]: the definition composed from torch ops, differentiable in `params`."""
    w1, b1, w2, b2 = unpack(params)
    a = torch.sigmoid(features(spec, tab) @ w1.t() + b1)
    return torch.sigmoid(a @ w2 + b2)


def loss_torch(spec, tab, params, target, mask):
    v = roll_torch(spec, tab, params)
    total = mask.sum()
    if float(total) == 0.0:
        return (params * 0.0).sum()
    return (mask * (v - target) ** 2).sum() / total


def roll_host(spec, tab, params):
    """v^ [B, T, 88] in float64 NumPy."""
    spec = torch.as_tensor(np.asarray(spec, dtype=np.float64))
    return roll_torch(spec, tab, torch.as_tensor(np.asarray(params, dtype=np.float64))).numpy()


def _sig(z):
    return 1.0 / (1.0 + np.exp(-z))


def _dsig(z):
    """sigmoid'(z) as e / (1 + e)^2 with e = exp(-|z|): s (1 - s) loses all its digits in float64 once 1 - s falls below 2^-53."""
    e = np.exp(-np.abs(z))
    return e / ((1.0 + e) * (1.0 + e))


def loss_and_grad_host(spec, tab, params, target, mask):
    """(loss, gradient [1121]) in float64 NumPy, written out by hand (the tests compare it with autograd of `loss_torch`).  Only the
    cells with a non-zero mask are evaluated."""
    spec = np.asarray(torch.as_tensor(spec).detach().cpu().numpy() if torch.is_tensor(spec) else spec, dtype=np.float64)
    as64 = lambda a: np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    params, target, mask = as64(params).reshape(-1), as64(target), as64(mask)
    if params.size != N_PARAMS or target.shape != spec.shape[:2] + (N_KEYS,) or mask.shape != target.shape:
        raise ValueError('loss_and_grad_host: shapes do not match')
    total = mask.sum()
    grad = np.zeros(N_PARAMS)
    b, t, p = np.nonzero(mask)
    if total == 0.0 or b.size == 0:
        return 0.0, grad
    x = masked_features_host(spec, tab, b, t, p)
    w1, b1, w2, b2 = unpack(params)
    m, tg = mask[b, t, p], target[b, t, p]
    z1 = x @ w1.T + b1
    a = _sig(z1)
    z2 = a @ w2 + b2
    r = _sig(z2) - tg
    loss = float((m * r * r).sum() / total)
    d2 = 2.0 * m * r * _dsig(z2) / total
    dz1 = d2[:, None] * w2[None, :] * _dsig(z1)
    grad[:N_HIDDEN * N_INPUTS] = (dz1.T @ x).reshape(-1)
    grad[N_HIDDEN * N_INPUTS:N_HIDDEN * N_INPUTS + N_HIDDEN] = dz1.sum(axis=0)
    grad[N_HIDDEN * N_INPUTS + N_HIDDEN:N_PARAMS - 1] = a.T @ d2
    grad[N_PARAMS - 1] = d2.sum()
    return loss, grad


def masked_features_host(spec, tab, b, t, p):
    """x [n, 33] (float64) of the cells (b[i], t[i], p[i])."""
    spec, tab = np.asarray(spec, dtype=np.float64), np.asarray(tab)
    T = spec.shape[1]
    x = np.zeros((len(b), N_INPUTS))
    bins = tab[p]                                                                                    # [n, 8]
    for j in range(N_CONTEXT):
        row = np.clip(t - 1 + j, 0, T - 1)
        x[:, N_HARMONICS * j:N_HARMONICS * (j + 1)] = np.where(bins >= 0, spec[b[:, None], row[:, None], np.maximum(bins, 0)], 0.0)
    x[:, N_INPUTS - 1] = p / float(N_KEYS)
    return x


class VelocityHead(nn.Module):
    """The head and the front end it was trained on.  ``forward(spec)`` is rv_velocity_roll and ``loss(spec, target, mask)`` is
    rv_velocity_loss_grad (HIP device only); ``definition(spec)`` is the torch definition on any device."""

    def __init__(self, spec='Mel', centres=None, seed=0):
        super().__init__()
        if spec not in SPEC_KINDS:
            raise ValueError(f'spec={spec!r}: expected one of {SPEC_KINDS}')
        if centres is None:
            raise ValueError('VelocityHead needs the centre frequencies of its front end (velocity.front_end_centres(model))')
        g = torch.Generator().manual_seed(int(seed))
        u = lambda shape, fan_in: (torch.rand(shape, generator=g) * 2 - 1) / fan_in ** 0.5
        self.w1 = nn.Parameter(u((N_HIDDEN, N_INPUTS), N_INPUTS))
        self.b1 = nn.Parameter(u((N_HIDDEN,), N_INPUTS))
        self.w2 = nn.Parameter(u((N_HIDDEN,), N_HIDDEN))
        self.b2 = nn.Parameter(u((), N_HIDDEN))
        self.register_buffer('spec_kind', torch.tensor(SPEC_KINDS.index(spec), dtype=torch.int64))
        self.register_buffer('centres', torch.as_tensor(np.asarray(centres, dtype=np.float64).reshape(-1)).clone())
        self._table = None

    @classmethod
    def for_model(cls, model, seed=0):
        kind, centres = front_end_centres(model)
        return cls(kind, centres, seed)

    @classmethod
    def from_state_dict(cls, state):
        """The head of a checkpoint: its front end is read from the checkpoint's own `spec_kind` and `centres`."""
        head = cls(SPEC_KINDS[int(state['spec_kind'])], state['centres'].cpu().numpy())
        head.load_state_dict(state)
        return head

    @property
    def spec(self):
        return SPEC_KINDS[int(self.spec_kind)]

    @property
    def table(self):
        """int32 [88, 8] (NumPy), rebuilt when `centres` changed."""
        key = (self.centres._version, self.centres.data_ptr())
        if self._table is None or self._table[0] != key:
            self._table = (key, harmonic_bins(self.centres.detach().cpu().numpy()))
        return self._table[1]

    def packed(self):
        """The flat parameter vector [1121] (differentiable)."""
        return torch.cat([self.w1.reshape(-1), self.b1, self.w2, self.b2.reshape(1)])

    def check_front_end(self, model):
        kind, centres = front_end_centres(model)
        own = self.centres.detach().cpu().numpy()
        if kind != self.spec or centres.shape != own.shape or not np.array_equal(centres, own):
            raise ValueError(f'this velocity head was trained on a {self.spec} front end with {own.size} bins; the model has {kind} with '
                             f'{centres.size} bins (or other centre frequencies)')

    def definition(self, spec):
        return roll_torch(spec, self.table, self.packed())

    def definition_loss(self, spec, target, mask):
        return loss_torch(spec, self.table, self.packed(), target, mask)

    def forward(self, spec):
        from . import ops
        return ops.velocity_roll(spec, self.table, self.packed().detach())

    def loss(self, spec, target, mask):
        from . import ops
        return ops.velocity_loss(spec, self.table, self.packed(), target, mask)


def velocity_loss(head, spec, target, mask):
    """The masked mean squared error of `head` on a batch (`mask = batch['onset']`, `target = batch['velocity']`): the fused kernel on a
    HIP device.  `head.definition_loss` is the same from torch ops."""
    return head.loss(spec, target, mask)


def midi_velocities(v):
    """Roll units (velocity / 128) -> MIDI velocities: clamp(rint(128 v), 1, 127) as int64."""
    return np.clip(np.rint(128.0 * np.asarray(v, dtype=np.float64)), 1, 127).astype(np.int64)


# ---- training and held-out error (train_velocity.py; HIP device only) ---------------------------------------------------------------
def front_end(model, audio):
    """The normalised spectrogram [B, T, n_bins] of audio [B, L] (or [L]) as the transcriber sees it: the model's own `_front`."""
    audio = audio.reshape(-1, audio.shape[-1])
    with torch.no_grad():
        return model._front(audio, audio.shape[-1]).squeeze(1)


def fit(head, model, batches, steps, lr=3e-3, on_step=None):
    """`steps` Adam steps on the head's 1121 parameters: per batch the front end of `model` (no transcriber pass), then the fused loss
    and gradient (rv_velocity_loss_grad) at the label onset cells.  Eager: no graph capture, one device.  `batches` is any iterable of
    feed batches (dicts with 'audio', 'onset', 'velocity'); it is cycled."""
    opt = torch.optim.Adam(head.parameters(), lr=lr)
    step = 0
    while step < steps:
        seen = 0
        for batch in batches:
            seen += 1
            spec = front_end(model, batch['audio'])
            shape = (spec.shape[0], spec.shape[1], N_KEYS)
            loss = head.loss(spec, batch['velocity'].reshape(shape), batch['onset'].reshape(shape))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            step += 1
            if on_step is not None:
                on_step(step, loss)
            if step >= steps:
                break
        if not seen:
            raise ValueError('velocity.fit: no batches')
    return head


def onset_velocity_mean(tracks):
    """Mean of velocity / 128 over the label onset cells (label == 3) of a list of tracks: the constant predictor."""
    total, count = 0.0, 0
    for t in tracks:
        on = torch.as_tensor(t['label']) == 3
        total += float(torch.as_tensor(t['velocity'])[on].double().sum()) / 128.0
        count += int(on.sum())
    return total / max(count, 1)


def heldout_error(head, model, items, constant):
    """(head error, constant-prediction error): mean |v^ - v| over the label onset cells of whole-track `items`, in units of 1 / 128."""
    err = const = 0.0
    count = 0
    for item in items:
        dev = head.w1.device
        roll = head(front_end(model, item['audio'].to(dev))).squeeze(0)
        on = item['onset'].to(dev).reshape(roll.shape) > 0
        target = item['velocity'].to(dev).reshape(roll.shape)[on].double()
        err += float((roll[on].double() - target).abs().sum())
        const += float((constant - target).abs().sum())
        count += int(on.sum())
    return 128.0 * err / max(count, 1), 128.0 * const / max(count, 1)
