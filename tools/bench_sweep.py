"""Threshold sweep of one song: rv_eval_sweep against a loop over the per-pair device path.

    python tools/bench_sweep.py [--frames 18750] [--grid 9] [--repeats 10] [--min-frames 1] [--bridge-gap 0]

The song is the ten-minute synthetic song of tools/bench_eval.py; the grid is 0.1 .. 0.9 on both axes.  Timed are
  sweep: sweep_counts_device -- the labels decoded once, the reference notes handed over, two launches for the whole grid, one
         read-back;
  loop:  what the same counters cost before the sweep existed -- per grid point extract_notes_wo_velocity_device, two
         match_notes_sparse calls (without / with the offset test) and evaluate_frames_device (its integer counters are kept, so the
         loop makes no launch or read-back beyond those calls), the labels decoded once outside the loop.
The counters of the two are compared for equality before any time is printed.  One warm-up run each, then the median of the
repeats with min..max; every run ends in a device synchronise.  --min-frames / --bridge-gap: the note clean-up of the estimate
(DESIGN 3.13), in the sweep and in every decode of the loop."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench_eval import make_song
from reconvat_amd import decoding as md, evaluate as ev


def loop_counts(s, on_thr, fr_thr, clean):
    p_ref, i_ref, roll_ref = md.extract_notes_wo_velocity_device(s['onset'], s['frame'], rule='rule2')
    pr, ir = ev._to_eval_units(p_ref, i_ref)
    out = {k: np.zeros((len(on_thr), len(fr_thr)), np.int64) for k in ev.SWEEP_KEYS}
    for a, x in enumerate(on_thr):
        for b, y in enumerate(fr_thr):
            p_est, i_est, roll_est = md.extract_notes_wo_velocity_device(s['pred_onset'], s['pred_frame'], float(x), float(y), rule='rule2',
                                                                         **clean)
            pe, ie = ev._to_eval_units(p_est, i_est)
            out['n_est'][a, b] = len(pe)
            out['matched'][a, b] = len(ev.match_notes_sparse(ir, pr, ie, pe, offset_ratio=None))
            out['matched_with_offsets'][a, b] = len(ev.match_notes_sparse(ir, pr, ie, pe))
            counts = ev.frame_counts_device(roll_ref, roll_est)       # evaluate_frames_device = this + the ratios; no extra read-back
            ev._frame_metrics_from_counts(counts)
            out['frame_tp'][a, b], out['frame_est'][a, b], frame_ref = counts[0], counts[2], counts[1]
    out['n_ref'], out['frame_ref'] = len(pr), frame_ref
    return out


def timed(name, fn, repeats):
    fn()                                                               # warm-up: code objects, allocator
    times = []
    for run in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        print(f'{name} run {run + 1}/{repeats}: {times[-1]:.4f} s', file=sys.stderr, flush=True)
    return out, statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=18750)
    ap.add_argument('--grid', type=int, default=9)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--min-frames', type=int, default=1)
    ap.add_argument('--bridge-gap', type=int, default=0)
    a = ap.parse_args()
    clean = dict(min_frames=a.min_frames, bridge_gap=a.bridge_gap)
    if not torch.cuda.is_available():
        raise SystemExit('bench_sweep: needs a HIP device (the device path has no CPU fallback)')
    dev = torch.device('cuda:0')
    song = {k: torch.from_numpy(v).to(dev) for k, v in make_song(a.frames).items()}
    thr = np.linspace(0.1, 0.9, a.grid).round(3).astype(np.float32)
    sweep, t_sweep, lo_s, hi_s = timed('sweep', lambda: ev.sweep_counts_device(song['onset'], song['frame'], song['pred_onset'], song['pred_frame'],
                                                                               thr, thr, rule='rule2', **clean), a.repeats)
    loop, t_loop, lo_l, hi_l = timed('loop', lambda: loop_counts(song, thr, thr, clean), a.repeats)
    same = all(np.array_equal(sweep[k], loop[k]) for k in ev.SWEEP_KEYS) and sweep['n_ref'] == loop['n_ref'] and \
        sweep['frame_ref'] == loop['frame_ref']
    if not same:
        raise SystemExit('bench_sweep: the sweep and the loop disagree -- no time is reported')
    mid = a.grid // 2
    print(f"song: {a.frames} frames, {sweep['n_ref']} reference notes; grid {a.grid} x {a.grid}; min_frames {a.min_frames}, bridge_gap "
          f"{a.bridge_gap}; at ({thr[mid]:.1f}, {thr[mid]:.1f}): "
          f"{sweep['n_est'][mid, mid]} estimated notes, {sweep['matched'][mid, mid]} matched, {sweep['matched_with_offsets'][mid, mid]} with offsets")
    print(f'counters identical over the grid (5 x {a.grid * a.grid} integers and the reference totals): {same}')
    print(f'median of {a.repeats} runs after one warm-up each, seconds per song and grid')
    print(f'sweep (rv_eval_sweep_clean) {t_sweep:10.4f}   min..max {lo_s:.4f}..{hi_s:.4f}')
    print(f'loop (per-pair device path) {t_loop:10.4f}   min..max {lo_l:.4f}..{hi_l:.4f}')
    print(f'loop / sweep                {t_loop / t_sweep:10.1f}')
    print(json.dumps({'frames': a.frames, 'grid': a.grid, 'min_frames': a.min_frames, 'bridge_gap': a.bridge_gap, 'ref_notes': sweep['n_ref'], 'identical': bool(same), 'sweep_s': t_sweep,
                      'loop_s': t_loop, 'sweep_min_max_s': [lo_s, hi_s], 'loop_min_max_s': [lo_l, hi_l]}))


if __name__ == '__main__':
    main()
