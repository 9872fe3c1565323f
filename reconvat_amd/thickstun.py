"""Drop-in surface of the reference's Thickstun CNN baseline (model/Thickstun_model.py) on MI355X.

Same constructor (no arguments), attributes (``normalize``, ``CNN_freq``, ``CNN_time``, ``linear``, ``spectrogram``), ``state_dict``
keys / order / shapes, ``forward`` signature and ``run_on_batch`` contract.  The ``nn`` modules are parameter containers only; every
numeric step goes through ``reconvat_amd.ops`` (csrc/thickstun.hip, rv_gemm).

The reference turns each of the T frames of a segment into its own 229 x 25 window and pushes a batch of T windows through the
three layers.  The windows overlap by 24 frames and ``CNN_freq`` is one frame wide, so here ``relu(CNN_freq)`` is computed once per
frame of the zero-padded spectrogram and ``CNN_time`` runs as a 25-tap convolution along time over that shared tensor -- the same
sums, 25 times less work in the first layer and no unfolded copy of the input (ops.ThickFreqFn / ThickTconvFn / ThickLinearFn).
"""
import torch
import torch.nn as nn

from . import ops
from .frontend import MelSpectrogram, Normalization
from .ops import ThickFreqFn, ThickLinearFn, ThickTconvFn, bce_mean

PAD = 12                   # F.pad(spec, (12, 12)): half of the 25-frame window on either side
EVAL_CHUNK = 512           # frames per pass of a no_grad evaluation (z3 is 835 KB per frame)


class Thickstun(nn.Module):
    def __init__(self):
        super().__init__()
        self.normalize = Normalization('imagewise')
        k_out, k2_out = 128, 4096
        self.CNN_freq = nn.Conv2d(1, k_out, kernel_size=(128, 1), stride=(2, 1))
        self.CNN_time = nn.Conv2d(k_out, k2_out, kernel_size=(1, 25), stride=(1, 1))
        self.linear = nn.Linear(k2_out * 51, 88, bias=False)
        self.spectrogram = MelSpectrogram()

    def __del__(self):
        try:
            ops.drop_packs_of_params(list(self.parameters()))     # the packed-weight cache holds its source weights
        except Exception:  # noqa: BLE001 -- interpreter shutdown
            pass

    def _layers(self, x, pad):
        """x [B, Tin, 229] time-major -> probabilities [B * (Tin + 2*pad - 24), 88]."""
        z2 = ThickFreqFn.apply(x, self.CNN_freq.weight, self.CNN_freq.bias, pad)
        z3 = ThickTconvFn.apply(z2, self.CNN_time.weight, self.CNN_time.bias)
        bb, t, rows, n = z3.shape
        return ThickLinearFn.apply(z3.view(bb * t, rows * n), self.linear.weight, n)

    def forward(self, x):
        """x [N, 229, 25] ready-made windows -> [N, 88] (the reference signature): each window is a clip of 25 frames with one output frame."""
        if x.dim() != 3 or x.shape[1] != 229 or x.shape[2] != 25:
            raise ValueError(f'expected windows of shape [N, 229, 25], got {tuple(x.shape)}')
        return self._layers(x.transpose(1, 2).contiguous(), 0)

    def frames(self, spec):
        """Normalised spectrogram [B, T, 229] (time-major) -> [B*T, 88], every frame seeing its zero-padded 25-frame window.  In eval mode
        under no_grad time is processed in chunks of EVAL_CHUNK frames with a 12-frame halo, so memory stays bounded for whole songs;
        each output frame sees the same 25 inputs in the same order, so the result equals the unchunked one bit for bit."""
        bb, t, _ = spec.shape
        if self.training or torch.is_grad_enabled() or t <= EVAL_CHUNK:
            return self._layers(spec, PAD)
        padded = torch.nn.functional.pad(spec, (0, 0, PAD, PAD))
        out = torch.empty((bb, t, 88), device=spec.device, dtype=torch.float32)
        for s in range(0, t, EVAL_CHUNK):
            e = min(t, s + EVAL_CHUNK)
            out[:, s:e] = self._layers(padded[:, s:e + 2 * PAD].contiguous(), 0).view(bb, e - s, 88)
        return out.view(bb * t, 88)

    def run_on_batch(self, batch, batch_ul=None, VAT=False):
        audio_label = batch['audio']
        frame_label = batch['frame']
        if frame_label.dim() == 2:
            frame_label = frame_label.unsqueeze(0)
        audio = audio_label.reshape(-1, audio_label.shape[-1])[:, :-1]
        spec = self.spectrogram.lognorm(audio, log=True, normalise=True).squeeze(1)        # [B, T, 229], log + image-wise min-max
        frame_pred = self.frames(spec)
        predictions = {'onset': frame_pred, 'frame': frame_pred, 'r_adv': None}
        losses = {'loss/train_frame': bce_mean(frame_pred, frame_label.reshape(-1, 88))}
        return predictions, losses, spec.transpose(1, 2)
