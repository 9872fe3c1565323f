#!/usr/bin/env python
"""Align scores to recordings: recordings with a score or MIDI file of the piece that is NOT time-aligned to them
become recordings with labels.

    python align_scores.py with input=<folder> [output=<folder>] [radius_s=4.0] [coarse=8] [device=cuda:0] [overwrite=False]

For every ``name.wav`` of ``input`` (any sample rate, channel count and width) that has ``name.mid``, ``name.midi`` or ``name.score.tsv``
beside it, the score is rendered (reconvat_amd/synth.py), recording and rendering are aligned by banded dynamic time warping
(reconvat_amd/align.py: a coarse pass over the full matrix, then a band of ``radius_s`` seconds around its path) and the score's notes,
moved to the recording's time, are written to ``output``/``name.tsv`` (default: beside the recording) with the corpora's four columns
and header line.  All pairs of the folder go through one batched launch per stage on a HIP device; ``device=cpu`` runs the NumPy
definition.  One report line per pair: frames of recording (N) and score (M), coarse factor S, band width W, total cost, path length
and the mean cost per step in [0, 1].  An existing ``name.tsv`` is not overwritten unless ``overwrite=True``.
"""
import sys

from reconvat_amd.align import align_folder
from reconvat_amd.sacred_lite import parse_cli


def main(argv):
    cfg = dict(input=None, output=None, radius_s=4.0, coarse=8, device='cuda:0', overwrite=False)
    given = parse_cli(argv)
    unknown = sorted(set(given) - set(cfg))
    if unknown:
        raise SystemExit(f'unknown keys {unknown}; known: {sorted(cfg)}')
    cfg.update(given)
    if not cfg['input']:
        raise SystemExit('input=<folder> is required')
    return align_folder(str(cfg['input']), None if cfg['output'] is None else str(cfg['output']), float(cfg['radius_s']), int(cfg['coarse']),
                        str(cfg['device']), bool(cfg['overwrite']))


if __name__ == '__main__':
    main(sys.argv[1:])
