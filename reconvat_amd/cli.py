"""Shared body of the drop-in training entry points (train_UNet_Onset_VAT.py / train_UNet_VAT.py /
train_baseline_onset_frame_VAT.py / train_baseline_Thickstun.py).

Keeps the reference CLI (`python train_UNet_Onset_VAT.py with key=value ...`, keys and defaults of
train_UNet_Onset_VAT.py:28-78 / train_UNet_VAT.py:26-79) and loop semantics (:128-154): epochs of
`iteration` optimiser steps through train_VAT_model, a checkpoint every `saving_freq` epochs
(model-{ep}.pt + last-optimizer-state.pt), scalar logging of every loss key per epoch.
MI355X-side additions: one process per GPU under torch.distributed.run (data-parallel, ONE flat RCCL
gradient all-reduce per step), the fused FlatAdam, optional whole-step hipGraph replay (`graph=True`) and
`train_on=Synthetic`, and `train_on=Rendered` / `train_on=Rendered:<folder>`: a corpus of note lists rendered to audio when the script
starts (reconvat_amd/synth.py) -- seeded random scores, or the .tsv / .mid / .midi files of a folder; and
`train_on=Scores:<folder>`: recordings with scores that are not aligned to them, aligned when the script starts (reconvat_amd/align.py,
DESIGN 3.16), the recordings without a score as the unlabelled set.
"""
import contextlib
import json
import os
import time
from datetime import datetime

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import UNet_Onset, UNet, dp
from .dataset import prepare_VAT_dataset
from .train import FlatAdam, TrainStep, train_VAT_model, train_model, cycle

ds_ksize, ds_stride = (2, 2), (2, 2)
mode = 'imagewise'
logging_freq = 100
saving_freq = 200
# optimiser options of the fused step (fused_optimizer=True only), all off by default: decoupled weight decay, an
# exponential moving average of the weights (checkpointed as model-{ep}.ema.pt, used for every validation), and
# clip_before_step=True: `clip_gradient_norm` limits the update (the reference clips after the step, which limits nothing)
OPTIM_OPTIONS = dict(weight_decay=0.0, ema_decay=0.0, clip_before_step=False)
# augmentation of the device feed (device_feed=True only), off by default: every training item -- labelled and
# unlabelled -- is transposed by a random whole number of semitones in [-pitch_shift, pitch_shift] (at most 6) while it is cropped
# -- and, with reverb_rt60 / eq_db / noise_db, recorded in a random room (RT60 up to reverb_rt60 seconds, an impulse
# response of reverb_taps taps), through a random five-band equaliser of at most +-eq_db dB and over white noise between
# noise_db - 20 and noise_db dBFS.  The labels are untouched.
# reverb_taps: the largest of 1024 / 2048 / 4096 / 8192 whose two launches per step (labelled + unlabelled batch) measured under 5 % of
# the training step (profiles/feed_acoustics.txt: 2 x 434 us of 19.75 ms = 4.4 % at 8192; 2.0 % at 4096)
FEED_OPTIONS = dict(pitch_shift=0, reverb_rt60=0.0, eq_db=0.0, noise_db=None, reverb_taps=8192)


def base_config(o, onset_script):
    """Config scope shared by both scripts; `o` holds CLI overrides (needed for the derived entries)."""
    c = dict(
        root='runs', device='cuda:0', log=True, w_size=31, spec='Mel', resume_iteration=None,
        train_on='MAPS' if onset_script else 'Wind', n_heads=4, position=True, iteration=10, VAT_start=0, alpha=1,
        VAT=True, XI=1e-6, eps=2, small=False, supersmall=False, onset_stack=True,
        KL_Div=False, reconstruction=False, batch_size=8,
        train_batch_size=8 if onset_script else 1, sequence_length=327680, epoches=20000,
        step_size_up=100, max_lr=1e-4, learning_rate=1e-3, learning_rate_decay_steps=1000,
        learning_rate_decay_rate=0.98, leave_one_out=None, clip_gradient_norm=3, refresh=False,
        # MI355X-side extras (not in the reference)
        graph=True, fused_optimizer=True, saving_freq=saving_freq, logging_freq=logging_freq, device_feed=True,
        device_metrics=True,   # validation: note decoding, frame counters and AP on the device; False = the host metric code
        tune_thresholds=False,  # True: choose onset / frame threshold on the validation set before the final evaluation
        dtype='fp32',          # 'bf16': opt-in experiment -- bf16-operand backward convs of the final graphs (forward stays fp32)
        **OPTIM_OPTIONS, **FEED_OPTIONS,
    )
    c.update(o)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory < 10e9:
        if 'batch_size' not in o:
            c['batch_size'] //= 2
        if 'sequence_length' not in o:
            c['sequence_length'] //= 2
        print(f"Reducing batch size to {c['batch_size']} and sequence_length to {c['sequence_length']} to save memory")
    c.setdefault('validation_length', c['sequence_length'])
    if 'validation_length' not in o:
        c['validation_length'] = c['sequence_length']
    stamp = datetime.now().strftime('%y%m%d-%H%M%S')
    if 'logdir' not in o:
        corpus = str(c['train_on']).replace(os.sep, '_')    # train_on=Rendered:<folder> names a path
        if onset_script:
            c['logdir'] = (f"{c['root']}/Unet_Onset-recons={c['reconstruction']}-XI={c['XI']}-eps={c['eps']}-alpha={c['alpha']}"
                           f"-train_on=small_{c['small']}_{corpus}-w_size={c['w_size']}-n_heads={c['n_heads']}"
                           f"-lr={c['learning_rate']}-" + stamp)
        else:
            c['logdir'] = (f"{c['root']}/Unet-recons={c['reconstruction']}-XI={c['XI']}-eps={c['eps']}-alpha={c['alpha']}"
                           f"-train_on=small_{c['small']}_{corpus}-w_size={c['w_size']}-n_heads={c['n_heads']}"
                           f"-lr={c['learning_rate']}-" + stamp)
    return c


def baseline_config(o):
    """Config scope of train_baseline_onset_frame_VAT.py:25-73 (model_name='onset_frame' is the one on the MI355X path)."""
    c = dict(
        root='runs', onset_stack=True, device='cuda:0', log=True, w_size=31, model_complexity=48, spec='Mel',
        resume_iteration=None, train_on='String', iteration=10, alpha=1, VAT=False, XI=1e-6, eps=1e-1, VAT_mode='all',
        model_name='onset_frame', VAT_start=0, small=True, supersmall=False, batch_size=8, train_batch_size=8,
        sequence_length=327680, epoches=20000, learning_rate=5e-4, learning_rate_decay_steps=10000,
        learning_rate_decay_rate=0.98, leave_one_out=None, clip_gradient_norm=3, refresh=False, reconstruction=False,
        graph=True, fused_optimizer=True, saving_freq=saving_freq, logging_freq=logging_freq, device_feed=True,
        device_metrics=True, tune_thresholds=False, **OPTIM_OPTIONS, **FEED_OPTIONS,
    )
    c.update(o)
    if c['model_name'] not in ('onset_frame', 'frame', 'onset'):
        raise NotImplementedError("model_name must be 'onset_frame', 'frame' or 'onset' (the 'attention' variant is not built)")
    if 'validation_length' not in o:
        c['validation_length'] = c['sequence_length']
    if 'logdir' not in o:
        c['logdir'] = f"{c['root']}/baseline_Onset_Frame-" + datetime.now().strftime('%y%m%d-%H%M%S')
    return c


def thickstun_config(o):
    """Config scope of train_baseline_Thickstun.py:25-78 (the VAT keys are set and never used there; kept so the reference's
    command lines parse)."""
    c = dict(
        root='runs', onset_stack=True, device='cuda:0', log=True, w_size=31, spec='Mel', resume_iteration=None, train_on='String',
        n_heads=4, position=True, iteration=10, VAT_start=0, alpha=1, VAT=True, XI=1e-6, eps=1.3, small=True, supersmall=True,
        KL_Div=False, reconstruction=False, batch_size=1, train_batch_size=1, sequence_length=327680, epoches=20000,
        step_size_up=100, max_lr=1e-4, learning_rate=1e-4, learning_rate_decay_steps=1000, learning_rate_decay_rate=0.98,
        leave_one_out=None, clip_gradient_norm=3, refresh=False,
        graph=True, fused_optimizer=True, saving_freq=10, logging_freq=10, device_feed=True,
        device_metrics=True, tune_thresholds=False, **OPTIM_OPTIONS, **FEED_OPTIONS,
    )
    c.update(o)
    if torch.cuda.is_available() and torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory < 10e9:
        if 'batch_size' not in o:
            c['batch_size'] //= 2
        if 'sequence_length' not in o:
            c['sequence_length'] //= 2
        print(f"Reducing batch size to {c['batch_size']} and sequence_length to {c['sequence_length']} to save memory")
    if 'validation_length' not in o:
        c['validation_length'] = c['sequence_length']
    if 'logdir' not in o:
        c['logdir'] = f"{c['root']}/baseline_ThickStun-lr={c['learning_rate']}" + datetime.now().strftime('%y%m%d-%H%M%S')
    return c


class ScalarLog:
    """TensorBoard SummaryWriter when available, else one JSON line per (tag, step)."""

    def __init__(self, logdir):
        os.makedirs(logdir, exist_ok=True)
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.tb = SummaryWriter(logdir)
        except Exception:  # noqa: BLE001 -- tensorboard is optional
            self.tb = None
        self.f = open(os.path.join(logdir, 'scalars.jsonl'), 'a')

    def add_scalar(self, tag, value, global_step):
        if self.tb is not None:
            self.tb.add_scalar(tag, value, global_step=global_step)
        self.f.write(json.dumps({'tag': tag, 'value': value, 'step': global_step}) + '\n')
        self.f.flush()


def log_validation(model, val_set, l_loader, ep, writer, reconstruction, onset_script, VAT, VAT_start, device_metrics=False):
    """The scalar half of tensorboard_log (model/helper_functions.py:120-141): `evaluate_wo_velocity(validation_dataset, model,
    reconstruction=reconstruction, VAT=False)` -- precision / recall / f1 of every non-chroma metric logged under its key -- then
    `eval_model(model, ep, supervised_loader, VAT_start, VAT)` -- the mean of every eval-mode loss key."""
    from .evaluate import evaluate_wo_velocity
    from .train import eval_model
    was_training = model.training
    model.eval()
    with torch.no_grad():
        metrics = evaluate_wo_velocity(val_set, model, reconstruction=reconstruction, VAT=False, device_metrics=device_metrics)
    for key, values in metrics.items():
        if key.startswith('metric/') and values:
            _, category, name = key.split('/')
            print(f'{category:>32} {name:25}: {np.mean(values):.3f} \u00b1 {np.std(values):.3f}')
            if ('precision' in name or 'recall' in name or 'f1' in name) and 'chroma' not in name:
                writer.add_scalar(key, float(np.mean(values)), ep)
    test_losses = eval_model(model, ep, l_loader, VAT_start, VAT)
    for key, values in test_losses.items():
        if key.startswith('loss/') and values:
            writer.add_scalar(key, float(np.mean(values)), ep)
    model.train(was_training)


def run_training(onset_script, spec, resume_iteration, train_on, batch_size, sequence_length, small, supersmall,
                 train_batch_size, learning_rate, learning_rate_decay_steps, learning_rate_decay_rate, alpha,
                 clip_gradient_norm, validation_length, refresh, device, epoches, logdir, log, iteration, VAT_start, VAT,
                 XI, eps, reconstruction, graph, fused_optimizer, saving_freq, device_feed=True, model_complexity=48, model_name='onset_frame', VAT_mode='all',
                 logging_freq=logging_freq, dtype='fp32', device_metrics=True, tune_thresholds=False, weight_decay=0.0, ema_decay=0.0,
                 clip_before_step=False, pitch_shift=0, reverb_rt60=0.0, eq_db=0.0, noise_db=None, reverb_taps=FEED_OPTIONS['reverb_taps'], **_unused):
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    if not fused_optimizer and (weight_decay or ema_decay or clip_before_step):
        raise SystemExit('weight_decay, ema_decay and clip_before_step are options of the fused optimiser step: they need '
                         'fused_optimizer=True (the torch optimiser path stays the reference loop).')
    if pitch_shift:
        from .augment import check_shift
        try:
            check_shift(pitch_shift)
        except ValueError as e:
            raise SystemExit(str(e))
        if not device_feed or not str(device).startswith('cuda'):
            raise SystemExit('pitch_shift is an option of the device feed (the batch is resampled while it is cropped in HBM): it needs '
                             'device_feed=True and device=cuda:N (the host DataLoader path stays the reference loop).')
    acoustics = None
    if reverb_rt60 or eq_db or noise_db is not None:
        from .acoustics import Acoustics
        try:
            acoustics = Acoustics(rt60=reverb_rt60, eq_db=eq_db, noise_db=noise_db, taps=reverb_taps)
        except ValueError as e:
            raise SystemExit(str(e))
        if not device_feed or not str(device).startswith('cuda'):
            raise SystemExit('reverb_rt60, eq_db and noise_db are options of the device feed (the batch is filtered in HBM after it is '
                             'cropped): they need device_feed=True and device=cuda:N (the host DataLoader path stays the reference loop).')
    if onset_script == 'thickstun':
        VAT = False                                        # train_baseline_Thickstun.py sets the VAT keys and never uses them
    if not str(device).startswith('cuda') or not torch.cuda.is_available():
        raise SystemExit(f"device={device!r}: this build runs the training path on an MI355X only (hand-written HIP kernels, no CPU "
                         "fallback); use device=cuda:0.  The reference's CPU plumbing run maps to the same command with device=cuda:0.")
    if world > 1:
        # one process per GPU (RV_DP_BACKEND=nccl: RCCL; gloo + RV_DP_SAME_GPU=1: every rank on cuda:0, for one-GPU boxes).  The
        # training group keeps the default collective timeout; rank 0 alone runs the validation passes (whole songs can take
        # minutes) while its peers wait in dp.wait_for_rank0() on a separate long-timeout gloo group
        dev_ = dp.local_device()
        device = f'cuda:{dev_.index}'
        torch.cuda.set_device(dev_)
        dp.init(dev_, long_wait_group=True)
    elif str(device).startswith('cuda'):
        torch.cuda.set_device(torch.device(device))

    l_set, ul_set, val_set, full_validation = prepare_VAT_dataset(sequence_length=sequence_length, validation_length=validation_length,
                                                        refresh=refresh, device=device, small=small, supersmall=supersmall,
                                                        dataset=train_on, rank=rank)
    if device_feed and hasattr(l_set, 'data') and str(device).startswith('cuda'):
        # corpus resident in HBM, batches cropped/decoded by rv_crop_segments (reconvat_amd/feed.py); the training loaders alone
        # are augmented: validation, test and threshold-tuning sets never are
        from .feed import device_loader
        l_loader = device_loader(l_set, train_batch_size, device, rank=rank, world=world, seed=42 + rank, pitch_shift=pitch_shift,
                                 acoustics=acoustics)
        ul_loader = device_loader(ul_set, batch_size, device, rank=rank, world=world, seed=43 + rank, pitch_shift=pitch_shift,
                                  acoustics=acoustics) if VAT else None
        if pitch_shift and rank == 0:
            print(f'Pitch-shift augmentation: every training item transposed by a random k in [-{pitch_shift}, {pitch_shift}] semitones')
        if acoustics is not None and rank == 0:
            print(f'Acoustic augmentation: every training item in a room of RT60 in [{0.25 * acoustics.rt60:g}, {acoustics.rt60:g}] s '
                  f'({acoustics.taps} taps), equalised by up to +-{acoustics.eq_db:g} dB, noise floor '
                  + ('off' if acoustics.noise_db is None else f'in [{acoustics.noise_db - 20:g}, {acoustics.noise_db:g}] dBFS'))
    else:
        if acoustics is not None:
            raise SystemExit(f'reverb_rt60, eq_db and noise_db need the device feed, and the {train_on} training set has no in-memory '
                             'tracks to keep in HBM.')
        if pitch_shift:
            raise SystemExit(f'pitch_shift needs the device feed, and the {train_on} training set has no in-memory tracks to keep in HBM.')
        ul_loader = DataLoader(ul_set, batch_size, shuffle=True, drop_last=True) if VAT else None
        l_loader = DataLoader(l_set, train_batch_size, shuffle=True, drop_last=True)

    # which recordings this rank trains on (labelled / unlabelled corpus and this rank's shard of each)
    os.makedirs(logdir, exist_ok=True)
    with open(os.path.join(logdir, f'corpus_rank{rank}.json'), 'w') as fh:
        paths = lambda ds: [str(d['path']) for d in getattr(ds, 'data', [])]
        json.dump({'train_on': train_on, 'rank': rank, 'world': world, 'labelled': paths(l_set), 'unlabelled': paths(ul_set),
                   'labelled_shard': list(getattr(l_loader, 'paths', [])), 'unlabelled_shard': list(getattr(ul_loader, 'paths', [])),
                   'validation': paths(val_set), 'full_validation': paths(full_validation)}, fh, indent=0)

    torch.manual_seed(0)                                   # identical initial weights on every rank
    if onset_script == 'thickstun':
        from .thickstun import Thickstun
        cls = Thickstun
        model = cls()
    elif onset_script == 'baseline':
        from . import onset_frames as onf
        from .constants import N_BINS, MAX_MIDI, MIN_MIDI
        cls = {'onset_frame': onf.OnsetsAndFrames_VAT_full, 'frame': onf.Frame_stack_VAT, 'onset': onf.Onset_stack_VAT}[model_name]
        model = cls(N_BINS, MAX_MIDI - MIN_MIDI + 1, model_complexity=model_complexity, log=log, mode=mode, spec=spec, XI=XI, eps=eps,
                    VAT_mode=VAT_mode)
    else:
        cls = UNet_Onset if onset_script else UNet
        model = cls(ds_ksize, ds_stride, log=log, reconstruction=reconstruction, mode=mode, spec=spec, device=device, XI=XI, eps=eps)
    if resume_iteration is not None:
        sd = torch.load(os.path.join(logdir, f'model-{resume_iteration}.pt'), map_location='cpu')
        model.load_state_dict(sd)
    model.to(device)
    torch.manual_seed(1 + rank)
    scheduler = None
    if fused_optimizer:
        optimizer = FlatAdam(model.parameters(), lr=learning_rate, step_size=learning_rate_decay_steps,
                             gamma=learning_rate_decay_rate, data_parallel=world > 1,
                             sync_error_word=bool(getattr(model, 'has_recurrence', False)), weight_decay=weight_decay,
                             max_grad_norm=float(clip_gradient_norm or 0) if clip_before_step else 0.0, ema_decay=ema_decay)
    else:
        optimizer = torch.optim.Adam(model.parameters(), learning_rate)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=learning_rate_decay_steps, gamma=learning_rate_decay_rate)
    first_epoch = 1
    if resume_iteration is not None:
        optimizer.load_state_dict(torch.load(os.path.join(logdir, 'last-optimizer-state.pt'), map_location=device))
        first_epoch = int(resume_iteration) + 1
        if scheduler is not None:                          # StepLR is not checkpointed by the reference: rebuild its position
            steps_done = max((int(float(st['step'])) for st in optimizer.state_dict()['state'].values()), default=0)
            scheduler.last_epoch = steps_done
        if rank == 0:
            if fused_optimizer:
                print(f'Resumed from model-{resume_iteration}.pt: optimiser step {int(optimizer.step_count.item())}, '
                      f'lr {optimizer.current_lr():.6e}')
            else:
                print(f'Resumed from model-{resume_iteration}.pt')
        if ema_decay:
            ema_file = os.path.join(logdir, f'model-{resume_iteration}.ema.pt')
            if os.path.exists(ema_file):
                optimizer.load_ema(torch.load(ema_file, map_location=device), model)
                if rank == 0:
                    print(f'Resumed the averaged weights from model-{resume_iteration}.ema.pt')
            elif rank == 0:
                print(f'No model-{resume_iteration}.ema.pt: the average starts from the resumed weights')
    # validation, threshold tuning and the final evaluation run on the averaged weights when there are any
    averaged = (lambda: optimizer.ema_weights()) if ema_decay else contextlib.nullcontext
    n_params = sum(p.numel() for p in model.parameters())
    if rank == 0:
        print(f'{cls.__name__}: {n_params} parameters, world size {world}, device {device}')
    writer = ScalarLog(logdir) if rank == 0 else None

    step_runner = None
    for ep in range(first_epoch, epoches + 1):
        use_vat = VAT and ep >= VAT_start
        if graph and fused_optimizer:
            # whole-step hipGraph replay on static buffers (same loop semantics as train_VAT_model)
            model.train()
            # (train_model, the Thickstun script's loop: one pass over the WHOLE loader per epoch instead of `iteration` steps)
            whole = onset_script == 'thickstun'
            li, ui = (iter(l_loader) if whole else cycle(l_loader)), (cycle(ul_loader) if use_vat else None)
            iteration = len(l_loader) if whole else iteration
            total = 0.0
            t_epoch = time.perf_counter()
            for _ in range(iteration):
                bl = next(li)
                bul = next(ui) if use_vat else None
                if step_runner is None or step_runner.VAT != use_vat:
                    step_runner = TrainStep(model, optimizer, bl, bul, alpha=alpha, VAT=use_vat, clip=clip_gradient_norm, graph=True,
                                            bf16_backward=str(dtype).lower() in ('bf16', 'bfloat16'))
                else:
                    step_runner.load(bl, bul)
                total += float(step_runner())
                step_runner.check()                # VAT NaN assert + BiLSTM time-out flag (the loss read-back just synchronised)
            losses = step_runner.losses
            if rank == 0:
                print(f'Train Epoch: {ep}\tLoss: {total / iteration:.6f}\t({(time.perf_counter() - t_epoch) / iteration * 1e3:.1f} ms/step)')
        elif onset_script == 'thickstun':
            _, losses, optimizer = train_model(model, ep, l_loader, optimizer, scheduler, clip_gradient_norm)
        else:
            _, losses, optimizer = train_VAT_model(model, iteration, ep, l_loader, ul_loader if VAT else None, optimizer,
                                                   scheduler, clip_gradient_norm, alpha, VAT, VAT_start)
        if onset_script == 'baseline' and str(device).startswith('cuda'):
            from . import ops
            ops.lstm_check(torch.device(device))          # eager loop: a timed-out recurrence launch fails the epoch loudly
        if rank == 0:
            # the scalar part of the reference's tensorboard_log (model/helper_functions.py:120-141; the figures are out of scope):
            # every `logging_freq` epochs (and after the first) note / frame metrics on the validation segments and the eval-mode
            # loss terms over the labelled loader
            if ep % logging_freq == 0 or ep == 1:
                if ema_decay:
                    print(f'Validation of epoch {ep} on the averaged weights (ema_decay={ema_decay})')
                with averaged():
                    log_validation(model, val_set, l_loader, ep, writer, reconstruction, onset_script, VAT and ep >= VAT_start, VAT_start,
                                   device_metrics=device_metrics)
            for key, value in losses.items():
                writer.add_scalar(key, float(value), ep)
            if ep % saving_freq == 0:
                torch.save(model.state_dict(), os.path.join(logdir, f'model-{ep}.pt'))
                if ema_decay:
                    torch.save(optimizer.ema_state_dict(model), os.path.join(logdir, f'model-{ep}.ema.pt'))
                torch.save(optimizer.state_dict(), os.path.join(logdir, 'last-optimizer-state.pt'))
        if world > 1 and (ep % logging_freq == 0 or ep == 1):
            dp.wait_for_rank0()                            # the other ranks wait for rank 0's validation pass
    if rank == 0:
        torch.save(model.state_dict(), os.path.join(logdir, 'model-final.pt'))
        if ema_decay:
            torch.save(optimizer.ema_state_dict(model), os.path.join(logdir, 'model-final.ema.pt'))
        # final evaluation exactly as the reference scripts end (train_UNet_Onset_VAT.py:156-170): WHOLE songs of the test split
        # (`full_validation`, sequence_length=None), transcriptions written to <logdir>/MIDI_results, metrics pickled to
        # <logdir>/result_dict
        import pickle
        from .evaluate import evaluate_wo_velocity
        print('Training finished, now evaluating on the test split (full songs)')
        model.eval()
        chosen = {}
        if ema_decay:
            print(f'Threshold tuning and the final evaluation run on the averaged weights (ema_decay={ema_decay})')
        with averaged():
            if tune_thresholds:
                # thresholds chosen on the validation split, the test songs then evaluated at the chosen pair
                from .evaluate import tune_thresholds as sweep_validation
                grid = [round(0.1 * k, 1) for k in range(1, 10)]
                with torch.no_grad():
                    tuned = sweep_validation(val_set, model, grid, grid, device_metrics=device_metrics)
                chosen = {'onset_threshold': tuned['onset_threshold'], 'frame_threshold': tuned['frame_threshold']}
                print(f"Thresholds chosen on {tuned['songs']} validation items: onset {chosen['onset_threshold']:.2f}, frame "
                      f"{chosen['frame_threshold']:.2f} (mean note F1 {tuned['best_value']:.4f})")
            with torch.no_grad():
                metrics = evaluate_wo_velocity(full_validation, model, reconstruction=False, save_path=os.path.join(logdir, 'MIDI_results'),
                                               device_metrics=device_metrics, **chosen)
        for key, values in metrics.items():
            if key.startswith('metric/'):
                _, category, name = key.split('/')
                print(f'{category:>32} {name:25}: {np.mean(values):.3f} \u00b1 {np.std(values):.3f}')
                writer.add_scalar('validation/' + key, float(np.mean(values)), epoches)
        with open(os.path.join(logdir, 'result_dict'), 'wb') as fh:
            pickle.dump(dict(metrics, **{'threshold/' + k.split('_')[0]: [v] for k, v in chosen.items()}), fh)
        f1 = float(np.mean(metrics['metric/frame/f1'])) if metrics['metric/frame/f1'] else float('nan')
        print(f'Training finished.  validation frame F1 {f1:.4f}, note F1 '
              f"{float(np.mean(metrics['metric/note/f1'])) if metrics['metric/note/f1'] else float('nan'):.4f}")
    if world > 1:
        dp.wait_for_rank0()                                # nobody tears the process group down while rank 0 still evaluates
        dp.shutdown()
    return model
