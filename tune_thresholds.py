#!/usr/bin/env python
"""Choose the decoding thresholds of a trained model on the validation split.

    python tune_thresholds.py with weight=runs/.../model-final.pt train_on=MAPS device=cuda:0 \\
        onset_thresholds=[0.3,0.4,0.5] frame_thresholds=[0.3,0.4,0.5] criterion=note_f1

Both grids default to 0.1 .. 0.9 in steps of 0.1 (at most 32 values each); ``criterion`` is ``note_f1``, ``note_with_offsets_f1`` or
``frame_f1``.  ``cleanups=[[1,0],[2,0],[2,1],[3,1]]`` adds the note clean-up to the choice: up to 8 pairs
``[min_frames, bridge_gap]``, one sweep per pair on the same forward pass (default ``[[1,0]]``: none).
The checkpoint is loaded as transcribe_files.py loads it (``UNet_Onset`` if it has an onset head), the validation split is the one ``prepare_VAT_dataset``
returns for ``train_on`` (``validation_length`` samples per item, the whole track with ``validation_length=None``).  That function builds
all four splits, so the labelled and unlabelled training sets of the corpus are opened as well and dropped (for MAPS that includes
MAESTRO; ``small=True``, the default here, keeps the labelled set to one piano).  Prints the grid of
the criterion at the chosen clean-up pair, the best thresholds and that pair, and writes every grid to ``<weight>.thresholds.json``
(``output=`` overrides the path); hand the choice to transcribe_files.py as ``onset_threshold=`` / ``frame_threshold=`` /
``min_frames=`` / ``bridge_gap=``.
"""
import json
import sys

import numpy as np
import torch

from reconvat_amd.dataset import prepare_VAT_dataset
from reconvat_amd.evaluate import tune_thresholds
from reconvat_amd.sacred_lite import parse_cli
from transcribe_files import load_model

DEFAULT_GRID = [round(0.1 * k, 1) for k in range(1, 10)]


def main(argv):
    cfg = dict(device='cuda:0', weight=None, train_on='MAPS', spec='Mel', onset_thresholds=DEFAULT_GRID, frame_thresholds=DEFAULT_GRID,
               criterion='note_f1', validation_length=327680, small=True, supersmall=False, rule='rule2', device_metrics=None, output=None,
               cleanups=[[1, 0]])
    given = parse_cli(argv)
    unknown = sorted(set(given) - set(cfg))
    if unknown:
        raise SystemExit(f'unknown keys {unknown}; known: {sorted(cfg)}')
    cfg.update(given)
    on_device = str(cfg['device']).startswith('cuda')
    device_metrics = on_device if cfg['device_metrics'] is None else bool(cfg['device_metrics'])
    model = load_model(cfg['weight'], cfg['spec'], cfg['device'])
    _, _, val_set, _ = prepare_VAT_dataset(sequence_length=cfg['validation_length'], validation_length=cfg['validation_length'],
                                           refresh=False, device=cfg['device'], small=cfg['small'], supersmall=cfg['supersmall'],
                                           dataset=cfg['train_on'])
    with torch.no_grad():
        res = tune_thresholds(val_set, model, cfg['onset_thresholds'], cfg['frame_thresholds'], criterion=cfg['criterion'],
                              rule=cfg['rule'], device_metrics=device_metrics, cleanups=cfg['cleanups'])
    on_thr, fr_thr = np.atleast_1d(cfg['onset_thresholds']), np.atleast_1d(cfg['frame_thresholds'])
    print(f"mean {cfg['criterion']} over {res['songs']} validation items at min_frames={res['min_frames']} bridge_gap={res['bridge_gap']} "
          f"(rows: onset threshold, columns: frame threshold)")
    print(' ' * 6 + ''.join(f'{y:8.2f}' for y in fr_thr))
    for x, row in zip(on_thr, res['grid'][cfg['criterion']]):
        print(f'{x:6.2f}' + ''.join(f'{v:8.4f}' for v in row))
    a, b = res['best_index']
    print(f"best: onset_threshold={float(on_thr[a])} frame_threshold={float(fr_thr[b])} min_frames={res['min_frames']} "
          f"bridge_gap={res['bridge_gap']}  ({cfg['criterion']} {res['best_value']:.4f})")
    out = cfg['output'] or ((cfg['weight'] or 'untrained') + '.thresholds.json')
    with open(out, 'w') as fh:
        json.dump({'weight': cfg['weight'], 'train_on': cfg['train_on'], 'criterion': cfg['criterion'], 'songs': res['songs'],
                   'onset_thresholds': [float(x) for x in on_thr], 'frame_thresholds': [float(y) for y in fr_thr],
                   'onset_threshold': float(on_thr[a]), 'frame_threshold': float(fr_thr[b]), 'best_index': [int(a), int(b)],
                   'best_value': res['best_value'], 'grid': {k: v.tolist() for k, v in res['grid'].items()},
                   'cleanups': [list(c) for c in res['cleanups']], 'best_cleanup': res['best_cleanup'], 'min_frames': res['min_frames'],
                   'bridge_gap': res['bridge_gap'], 'grids': [{k: v.tolist() for k, v in g.items()} for g in res['grids']]}, fh, indent=1)
    print('wrote', out)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
