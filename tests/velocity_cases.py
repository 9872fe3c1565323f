"""The rendered mini-corpus and the training loop that tests/test_velocity.py (float32 torch definition, host renderer, oracle front
end) and tests/test_velocity_gpu.py (fused kernel, device renderer, device front end) share.

Corpus: `N_TRAIN + N_HELD` tracks of `SECONDS` s from `synth.random_score`, both voices, timbre seed = track index; the last
`N_HELD` are held out.  Every track is one clip (the front end normalises per clip).  Loss: masked MSE at label onset cells; error:
mean |v^ - v| at held-out onset cells in units of 1 / 128, next to that of predicting the training mean velocity."""
import numpy as np
import torch

from reconvat_amd import velocity as V
from reconvat_amd.constants import SAMPLE_RATE
from reconvat_amd.dataset import RenderedScores

N_TRAIN, N_HELD, SECONDS = 12, 4, 16
STEPS, LR = 2000, 3e-3
VOICES = ('struck', 'sustained')


def corpus(device='cpu'):
    """[(audio float32 [L] on `device`, onset mask [T, 88], velocity / 128 [T, 88]), ...] for the N_TRAIN + N_HELD tracks."""
    data = RenderedScores(N_TRAIN + N_HELD, SECONDS * SAMPLE_RATE, VOICES, seed=0, device=device)
    out = []
    for tr in data.data:
        audio = tr['audio'].to(device).to(torch.float32) * (1.0 / 32768.0)
        onset = (tr['label'] == 3).to(torch.float32).to(device)
        out.append((audio, onset, tr['velocity'].to(torch.float32).to(device) * (1.0 / 128.0)))
    return out


def stack(tracks, front):
    """(spec [n, T, n_bins], mask [n, T, 88], target [n, T, 88]); `front(audio [n, L])` -> [n, 1, T, n_bins] as `_front` returns it."""
    audio = torch.stack([a for a, _, _ in tracks])
    spec = front(audio).squeeze(1)
    return spec, torch.stack([m for _, m, _ in tracks]), torch.stack([v for _, _, v in tracks])


def errors(v_hat, mask, target, train_mask, train_target):
    """(mean |v^ - v| at the masked cells, the same for the constant = mean training velocity), in units of 1 / 128."""
    on = mask > 0
    const = float(train_target[train_mask > 0].double().mean())
    err = float((v_hat[on].double() - target[on].double()).abs().mean()) * 128.0
    return err, float((const - target[on].double()).abs().mean()) * 128.0


def train(head, loss_fn, steps=STEPS, lr=LR):
    """Full-batch Adam on the head's parameters; `loss_fn()` -> the scalar loss with a graph to them."""
    opt = torch.optim.Adam(head.parameters(), lr=lr)
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss_fn().backward()
        opt.step()
    return head
