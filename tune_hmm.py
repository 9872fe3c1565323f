#!/usr/bin/env python
"""Choose the parameters of the Viterbi note decoder of a trained model on the validation split.

    python tune_hmm.py with weight=runs/.../model-final.pt train_on=MAPS device=cuda:0 \\
        onset_thresholds=[0.3,0.5,0.7] frame_thresholds=[0.3,0.5,0.7] note_on=[0,1,2,4] note_off=[0,1,2,4] restrike=[2] criterion=note_f1

The five lists span a grid of ``NoteHMM`` parameter sets (their product, at most 256 sets per run; the thresholds default to
0.3 / 0.5 / 0.7, the three penalties -- in nats -- to 0 / 1 / 2 / 4, 2 and 2); ``criterion`` is ``note_f1``, ``note_with_offsets_f1`` or
``frame_f1``.  ``min_frames=`` / ``bridge_gap=`` (default 1 / 0) add one note clean-up pair to every decode.
The checkpoint and the validation split are loaded as tune_thresholds.py loads them; a checkpoint without an onset head gets
``use_onsets=False`` sets, decoded on its frame roll alone.  One forward pass per validation item, then one batched decode per 16 sets
on the device.  Prints the best sets and writes every value to ``<weight>.hmm.json`` (``output=`` overrides the path); hand the choice to
transcribe_files.py as ``decoder=hmm onset_threshold= frame_threshold= note_on= note_off= restrike=``.
"""
import json
import sys

import numpy as np
import torch

from reconvat_amd.dataset import prepare_VAT_dataset
from reconvat_amd.evaluate import tune_hmm
from reconvat_amd.hmm import hmm_grid
from reconvat_amd.sacred_lite import parse_cli
from transcribe_files import load_model


def main(argv):
    cfg = dict(device='cuda:0', weight=None, train_on='MAPS', spec='Mel', onset_thresholds=[0.3, 0.5, 0.7], frame_thresholds=[0.3, 0.5, 0.7],
               note_on=[0.0, 1.0, 2.0, 4.0], note_off=[2.0], restrike=[2.0], criterion='note_f1', validation_length=327680, small=True,
               supersmall=False, device_metrics=None, output=None, min_frames=1, bridge_gap=0)
    given = parse_cli(argv)
    unknown = sorted(set(given) - set(cfg))
    if unknown:
        raise SystemExit(f'unknown keys {unknown}; known: {sorted(cfg)}')
    cfg.update(given)
    on_device = str(cfg['device']).startswith('cuda')
    device_metrics = on_device if cfg['device_metrics'] is None else bool(cfg['device_metrics'])
    model = load_model(cfg['weight'], cfg['spec'], cfg['device'])
    use_onsets = bool(getattr(model, 'has_onset_head', False))
    hmms = hmm_grid(cfg['onset_thresholds'], cfg['frame_thresholds'], cfg['note_on'], cfg['note_off'], cfg['restrike'], use_onsets=use_onsets)
    _, _, val_set, _ = prepare_VAT_dataset(sequence_length=cfg['validation_length'], validation_length=cfg['validation_length'],
                                           refresh=False, device=cfg['device'], small=cfg['small'], supersmall=cfg['supersmall'],
                                           dataset=cfg['train_on'])
    with torch.no_grad():
        res = tune_hmm(val_set, model, hmms, criterion=cfg['criterion'], onset=use_onsets, device_metrics=device_metrics,
                       min_frames=cfg['min_frames'], bridge_gap=cfg['bridge_gap'])
    values = res['values'][cfg['criterion']]
    print(f"mean {cfg['criterion']} over {res['songs']} validation items, {len(hmms)} parameter sets; the best five:")
    for n in np.argsort(-values, kind='stable')[:5]:
        print(f'{values[n]:8.4f}  {res["hmms"][n]!r}')
    best = res['best']
    print(f"best: decoder=hmm onset_threshold={best.onset_threshold} frame_threshold={best.frame_threshold} note_on={best.note_on} "
          f"note_off={best.note_off} restrike={best.restrike}  ({cfg['criterion']} {res['best_value']:.4f})")
    out = cfg['output'] or ((cfg['weight'] or 'untrained') + '.hmm.json')
    with open(out, 'w') as fh:
        json.dump({'weight': cfg['weight'], 'train_on': cfg['train_on'], 'criterion': cfg['criterion'], 'songs': res['songs'],
                   'min_frames': cfg['min_frames'], 'bridge_gap': cfg['bridge_gap'], 'hmms': [h.as_dict() for h in res['hmms']],
                   'values': {k: v.tolist() for k, v in res['values'].items()}, 'best_index': res['best_index'], 'best': best.as_dict(),
                   'best_value': res['best_value']}, fh, indent=1)
    print('wrote', out)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
