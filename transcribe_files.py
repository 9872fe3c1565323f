#!/usr/bin/env python
"""Transcribe audio files to MIDI with a trained model (reference transcribe_files.py:12-69).

    python transcribe_files.py with device=cuda:0 weight=runs/.../model-final.pt input=Application/Input output=Application/Output

``onset_threshold=`` / ``frame_threshold=`` (default 0.5 each) set the decoding thresholds -- tune_thresholds.py chooses a pair on
the validation split.  ``min_frames=`` / ``bridge_gap=`` (default 1 / 0: off) clean the decoded notes up: gaps of at most
``bridge_gap`` frames inside a note are bridged, notes shorter than ``min_frames`` frames are dropped.
A checkpoint with an onset head (``transcriber.linear_onset.weight``) is loaded into ``UNet_Onset`` and decoded with its onset
posteriorgram; any other checkpoint, and a run without ``weight=``, builds ``UNet``, whose frame roll serves as onset roll too.
``spec=CQT`` selects the constant-Q front end; with ``weight=`` the front end follows the checkpoint's keys.
``render=True`` writes ``<tag>-<name>.wav`` next to each MIDI file: the decoded notes rendered by the synthesiser (DESIGN 3.15:
the 'struck' voice, timbre seed 0; 16 kHz, 16 bit, as long as the input) -- the transcription as something to listen to.
``velocity=<checkpoint>`` (a ``velocity-*.pt`` of train_velocity.py) gives every note its dynamics: the velocity roll of
the head on the spectrogram of the same audio, averaged per note on the device, as MIDI velocity clamp(rint(128 v), 1, 127) -- in the
MIDI file and in the rendering.  Without it every note has velocity 127, as before.
``decoder=hmm`` decodes the notes by Viterbi with a per-key onset / sustain / off model in place of thresholding: its
tables come from ``onset_threshold=`` / ``frame_threshold=``, ``note_on=`` / ``note_off=`` / ``restrike=`` (default 2.0 nats each) are
the costs of switching -- tune_hmm.py chooses all five on the validation split -- and the onset roll counts as evidence iff the
checkpoint has an onset head.  ``min_frames=`` / ``bridge_gap=`` and ``velocity=`` work on its notes as on the threshold decoder's.
``refine_onsets=True`` moves every decoded onset off the 32 ms frame grid to the sample at which the note's own harmonics rise most
steeply in the audio (after either decoder and after clean-up); ``onset_lead=<samples>`` (default 0) places it that much
earlier, for voices with a slow attack.  Without it the onsets are frame times, as before.

Inputs: ``.wav`` files of any sample rate and channel count (16 / 24 / 32-bit PCM or float; anything but 16 kHz 16-bit is
resampled to 16 kHz mono on the model's device) or ``.pt`` track caches (dict with an int16 ``audio`` tensor).
"""
import os
import sys
import wave

import numpy as np
import torch

import reconvat_amd as ra
from reconvat_amd.constants import HOP_LENGTH, SAMPLE_RATE, MIN_MIDI
from reconvat_amd import velocity
from reconvat_amd.decoding import NoteDecoder
from reconvat_amd.evaluate import midi_to_hz
from reconvat_amd.midi import save_midi
from reconvat_amd.sacred_lite import parse_cli


def load_audio(path, device='cpu'):
    """float32 [T] at 16 kHz.  A 16 kHz 16-bit wav is read as before; any other PCM / float wav (rate, channel count, 16 / 24 / 32
    bit) is resampled and downmixed on `device` (reconvat_amd/resample.py: the kernel on a HIP device, else the host path)."""
    if path.endswith('.pt'):
        return torch.load(path)['audio'].float().div(32768.0)
    try:
        with wave.open(path, 'rb') as w:
            if w.getframerate() == SAMPLE_RATE and w.getsampwidth() == 2:
                x = np.frombuffer(w.readframes(w.getnframes()), dtype=np.int16).reshape(-1, w.getnchannels()).mean(axis=1)
                return torch.from_numpy(x.astype(np.float32) / 32768.0)
    except wave.Error:                          # float and extensible-format wav: not for the `wave` module
        pass
    from reconvat_amd.dataset import read_audio_int16
    return torch.from_numpy(read_audio_int16(path, device)).float().div(32768.0)


def write_rendering(path, notes, n_samples, device):
    """The audible rendering of decoded notes (reconvat_amd/synth.py: 'struck' voice, timbre seed 0) as a 16 kHz 16-bit mono wav of
    `n_samples` frames -- on a HIP device by rv_synth_render."""
    from reconvat_amd import synth
    pcm = synth.render(np.asarray(notes, dtype=np.float64).reshape(-1, 4), n_samples, synth.Timbre('struck', 0), device=device,
                       out_dtype=torch.int16).cpu().numpy()
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(SAMPLE_RATE)
        w.writeframes(pcm.astype('<i2').tobytes())


def transcribe2midi(files, model, device, out_dir, onset_threshold=0.5, frame_threshold=0.5, rule='rule2', tag='ReconVAT', min_frames=1,
                    bridge_gap=0, render=False, head=None, hmm=None, refine_onsets=False, onset_lead=0):
    """``hmm``: a ``reconvat_amd.NoteHMM``.  The notes are then those of its Viterbi path (the two thresholds are unused:
    the model carries its own), found where the posteriorgrams are; the path's ONSET roll and ONSET-or-SUSTAIN roll take the place of
    the posteriorgrams in everything after the decode, so a note's velocity is the mean over its ONSET frames.
    ``refine_onsets``: the decoded notes (either decoder, after clean-up) go through ``onset_time.refine_intervals`` on the audio, where it
    is: onsets at the sample of steepest harmonic rise, ``onset_lead`` samples earlier, in place of the 32 ms frame grid."""
    from reconvat_amd import onset_time
    onset_lead = onset_time._lead(onset_lead)
    decode = NoteDecoder(onset_threshold, frame_threshold, rule, min_frames, bridge_gap, hmm)
    os.makedirs(out_dir, exist_ok=True)
    for path in files:
        audio = load_audio(path, device).to(device)
        with torch.no_grad():
            pred = model.transcribe({'audio': audio.unsqueeze(0)})
            # the head's roll on the spectrogram of the same audio, read per note by the decoder
            roll = None if head is None else head(velocity.front_end(model, audio.unsqueeze(0))).squeeze(0)
        onset, frame = pred['onset'].squeeze(0).relu(), pred['frame'].squeeze(0).relu()
        # decode where the posteriorgrams are (csrc/eval.hip, csrc/hmm.hip); same notes as the host decoder
        p_est, i_est, v_est, _ = decode(onset, frame, roll, device=frame.is_cuda)
        midi_vel = None if v_est is None else velocity.midi_velocities(v_est)
        scaling = HOP_LENGTH / SAMPLE_RATE
        if refine_onsets:                       # sub-frame onsets from the audio itself (csrc/onset_time.hip on a HIP device)
            i_est = onset_time.refine_intervals(audio, p_est, i_est, onset_lead, device=audio.is_cuda)
        else:
            i_est = (np.asarray(i_est) * scaling).reshape(-1, 2)
        keys = MIN_MIDI + np.asarray(p_est, dtype=np.float64).reshape(-1)
        p_est = np.array([midi_to_hz(MIN_MIDI + m) for m in p_est])
        midi_path = os.path.join(out_dir, tag + '-' + os.path.splitext(os.path.basename(path))[0] + '.mid')
        save_midi(midi_path, p_est, i_est, [127] * len(p_est) if midi_vel is None else [int(v) / 127 for v in midi_vel])
        print(f'midi_path = {midi_path}  ({len(p_est)} notes)')
        if render:                              # what the MIDI file says, to listen to: the same notes at the same velocity
            loud = np.full(len(keys), 127.0) if midi_vel is None else midi_vel.astype(np.float64)
            write_rendering(midi_path[:-len('.mid')] + '.wav', np.column_stack([i_est, keys, loud]), len(audio), device)


def load_model(weight, spec, device):
    """The model of a checkpoint, in eval mode on `device`: ``UNet_Onset`` if the state dict has an onset head, else ``UNet`` -- and
    ``UNet`` with fresh weights without a checkpoint.  The checkpoint's front-end buffers name its spectrogram."""
    state = torch.load(weight, map_location='cpu') if weight else None
    cls = ra.UNet
    if state is not None:
        spec = 'CQT' if 'spectrogram.cqt_kernels_real' in state else 'Mel'
        if 'transcriber.linear_onset.weight' in state:
            cls = ra.UNet_Onset
    # a checkpoint trained with reconstruction=False has no reconstructor to load
    recon = state is None or any(k.startswith('reconstructor.') for k in state)
    model = cls((2, 2), (2, 2), log=True, reconstruction=recon, mode='imagewise', spec=spec, device=device)
    if state is not None:
        model.load_state_dict(state)
    model.to(device).eval()
    model.has_onset_head = cls is ra.UNet_Onset         # decoder=hmm: whether the onset roll is evidence of its own
    return model


def load_head(path, model, device):
    """The velocity head of a checkpoint on `device`; it must have been trained on the model's front end."""
    from reconvat_amd.velocity import VelocityHead
    head = VelocityHead.from_state_dict(torch.load(path, map_location='cpu'))
    head.check_front_end(model)
    return head.to(device).eval()


def main(argv):
    cfg = dict(device='cuda:0', weight=None, input='Application/Input', output='Application/Output', spec='Mel', onset_threshold=0.5,
               frame_threshold=0.5, render=False, velocity=None, decoder='threshold', note_on=2.0, note_off=2.0, restrike=2.0)
    given = parse_cli(argv)
    cfg.update(given)
    if cfg['decoder'] not in ('threshold', 'hmm'):
        raise SystemExit(f"decoder must be 'threshold' or 'hmm', got {cfg['decoder']!r}")
    model = load_model(cfg['weight'], cfg['spec'], cfg['device'])
    files = sorted(os.path.join(cfg['input'], f) for f in os.listdir(cfg['input']) if f.endswith(('.wav', '.pt')))
    cleanup = {k: given[k] for k in ('min_frames', 'bridge_gap', 'render', 'refine_onsets', 'onset_lead') if k in given}     # handed on only when given
    if cfg['velocity']:
        cleanup['head'] = load_head(cfg['velocity'], model, cfg['device'])
    if cfg['decoder'] == 'hmm':                 # the tables come from the two thresholds; onsets count iff the checkpoint has an onset head
        cleanup['hmm'] = ra.NoteHMM(cfg['onset_threshold'], cfg['frame_threshold'], cfg['note_on'], cfg['note_off'], cfg['restrike'],
                                    use_onsets=model.has_onset_head)
    transcribe2midi(files, model, cfg['device'], cfg['output'], onset_threshold=cfg['onset_threshold'],
                    frame_threshold=cfg['frame_threshold'], **cleanup)


if __name__ == '__main__':
    main(sys.argv[1:])
