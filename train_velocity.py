#!/usr/bin/env python
"""Train the note-velocity head (reconvat_amd/velocity.py) beside a transcriber, not inside it.

    python train_velocity.py with train_on=Rendered [weight=runs/.../model-final.pt spec=Mel steps=3000 pitch_shift=2 reverb_rt60=0.4]

The corpus is fed from HBM (reconvat_amd/feed.py, with its pitch-shift and acoustic augmentation); a step is the front end alone
(no transcriber pass), the fused loss and gradient at the label onset cells (rv_velocity_loss_grad) and Adam on the 1121 parameters.
Eager, one device.  ``velocity-{step}.pt`` is saved every ``saving_freq`` steps and at the end; the checkpoint names its front end.
At the end the held-out error at label onset cells is printed next to that of predicting the mean training velocity, and, when
``weight=`` names a transcriber, the note-with-velocity metrics of that transcriber with this head."""
import os
from datetime import datetime

import numpy as np
import torch

from reconvat_amd import velocity
from reconvat_amd.sacred_lite import Experiment

ex = Experiment('train_velocity')


@ex.config
def config(o):
    cfg = dict(train_on='Rendered', weight=None, spec='Mel', steps=3000, batch_size=8, sequence_length=327680, validation_length=327680,
               learning_rate=3e-3, small=False, supersmall=False, refresh=False, device='cuda:0', saving_freq=1000, logging_freq=100,
               pitch_shift=0, reverb_rt60=0.0, eq_db=0.0, noise_db=None, reverb_taps=None, seed=0, logdir=None)
    cfg.update(o)
    if cfg['logdir'] is None:
        cfg['logdir'] = f"runs/velocity-{cfg['spec']}-{cfg['train_on'].split(':')[0]}-" + datetime.now().strftime('%y%m%d-%H%M%S')
    return cfg


@ex.automain
def train(train_on, weight, spec, steps, batch_size, sequence_length, validation_length, learning_rate, small, supersmall, refresh, device,
          saving_freq, logging_freq, pitch_shift, reverb_rt60, eq_db, noise_db, reverb_taps, seed, logdir):
    from reconvat_amd.dataset import prepare_VAT_dataset
    from reconvat_amd.feed import device_loader
    from transcribe_files import load_model
    if not str(device).startswith('cuda') or not torch.cuda.is_available():
        raise SystemExit(f'device={device!r}: the velocity head trains on an MI355X only (HIP kernels, no CPU fallback); use device=cuda:0')
    torch.cuda.set_device(torch.device(device))
    acoustics = None
    if reverb_rt60 or eq_db or noise_db is not None:
        from reconvat_amd.acoustics import Acoustics
        from reconvat_amd.cli import FEED_OPTIONS
        acoustics = Acoustics(rt60=reverb_rt60, eq_db=eq_db, noise_db=noise_db, taps=reverb_taps or FEED_OPTIONS['reverb_taps'])
    l_set, _, _, full = prepare_VAT_dataset(sequence_length=sequence_length, validation_length=validation_length, refresh=refresh,
                                            device=device, small=small, supersmall=supersmall, dataset=train_on, rank=0)
    if not hasattr(l_set, 'data'):
        raise SystemExit(f'train_on={train_on}: the velocity head trains from the device feed, which needs in-memory tracks')
    loader = device_loader(l_set, batch_size, device, seed=42, pitch_shift=pitch_shift, acoustics=acoustics)
    model = load_model(weight, spec, device)
    torch.manual_seed(seed)
    head = velocity.VelocityHead.for_model(model, seed=seed).to(device)
    os.makedirs(logdir, exist_ok=True)

    def on_step(step, loss):
        if step % logging_freq == 0:
            print(f'step {step}: loss {loss.item():.6f}')
        if step % saving_freq == 0 or step == steps:
            torch.save(head.state_dict(), os.path.join(logdir, f'velocity-{step}.pt'))

    velocity.fit(head, model, loader, steps, lr=learning_rate, on_step=on_step)
    constant = velocity.onset_velocity_mean(l_set.data)
    with torch.no_grad():
        err, const = velocity.heldout_error(head, model, full, constant)
    print(f'held-out error at label onset cells: {err:.2f} / 128 (constant prediction {const:.2f} / 128, ratio {err / max(const, 1e-12):.3f})')
    result = {'heldout_error': err, 'constant_error': const}
    if weight:
        from reconvat_amd.evaluate import evaluate_with_velocity
        with torch.no_grad():
            metrics = evaluate_with_velocity(full, model, head, reconstruction=False)
        for key in sorted(metrics):
            if 'velocity' in key:
                print(f'{key:52s} {np.mean(metrics[key]):.4f}')
                result[key] = float(np.mean(metrics[key]))
    return result
