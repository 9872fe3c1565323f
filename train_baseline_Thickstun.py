#!/usr/bin/env python
"""Drop-in entry point: `python train_baseline_Thickstun.py with key=value ...` (keys/defaults of the reference script of this
name: the Thickstun CNN baseline, one pass over the whole labelled loader per epoch, no VAT).  One process per GPU under
torch.distributed.run trains data-parallel, as for the other scripts."""
from reconvat_amd.cli import thickstun_config, run_training
from reconvat_amd.sacred_lite import Experiment

ex = Experiment('train_original')


@ex.config
def config(overrides):
    return thickstun_config(overrides)


@ex.automain
def train(spec, resume_iteration, train_on, batch_size, sequence_length, small, supersmall, train_batch_size, learning_rate,
          learning_rate_decay_steps, learning_rate_decay_rate, alpha, clip_gradient_norm, validation_length, refresh, device,
          epoches, logdir, log, iteration, VAT_start, VAT, XI, eps, reconstruction, graph, fused_optimizer, saving_freq,
          device_feed, logging_freq, device_metrics, tune_thresholds, weight_decay,
          ema_decay, clip_before_step, pitch_shift, reverb_rt60, eq_db, noise_db, reverb_taps):
    return run_training('thickstun', **locals())
