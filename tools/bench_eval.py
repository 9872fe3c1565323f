"""Whole-song evaluation after the model's forward: the host metric code against the device path, one synthetic song.

    python tools/bench_eval.py [--frames 18750] [--host-repeats 3] [--device-repeats 10] [--min-frames 1] [--bridge-gap 0]

The song: notes painted into label rolls (about one note per 3.2 frames, i.e. ~5 900 at the default ten minutes); the
"posteriorgrams" are the labels shifted by one frame, scaled, plus noise.  Timed are steps 2 to 6 of evaluate_wo_velocity's loop
(decoding, per-frame pitch lists, the two note matchings, frame metrics, AP) with the model excluded; every stage ends in a device
synchronise, one warm-up run per path, then the median of the repeats.  Both paths run in this process on the same inputs and
their results are compared before any time is printed.  --min-frames / --bridge-gap: the note clean-up of the estimate's decode
(DESIGN 3.13), on both paths."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from sklearn.metrics import average_precision_score

from reconvat_amd import decoding as md, evaluate as ev

STAGES = ('decoding', 'per-frame pitch lists', 'note matching (two calls)', 'frame metrics', 'AP')


def make_song(T, seed=0):
    rng = np.random.RandomState(seed)
    onset, frame = np.zeros((T, 88), np.float32), np.zeros((T, 88), np.float32)
    for _ in range(int(T / 3.2)):
        t0, p, ln = rng.randint(0, T), rng.randint(0, 88), rng.randint(3, 40)
        frame[t0:t0 + ln, p] = 1
        onset[t0:t0 + 2, p] = 1
    noise = lambda: rng.uniform(0, 0.45, size=(T, 88)).astype(np.float32)
    shift = lambda roll: np.concatenate([np.zeros((1, 88), np.float32), roll[:-1]])
    return {'onset': onset, 'frame': frame, 'pred_onset': shift(onset) * 0.5 + noise(), 'pred_frame': shift(frame) * 0.5 + noise()}


class Clock:
    def __init__(self):
        self.t = {}

    def stage(self, name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        self.t[name] = self.t.get(name, 0.0) + time.perf_counter() - t0
        return out


def note_metrics(ref, est, match):
    (p_ref, i_ref), (p_est, i_est) = ev._to_eval_units(*ref), ev._to_eval_units(*est)
    return (ev.evaluate_notes(i_ref, p_ref, i_est, p_est, offset_ratio=None, match=match),
            ev.evaluate_notes(i_ref, p_ref, i_est, p_est, match=match))


CLEAN = dict(min_frames=1, bridge_gap=0)                               # set from the command line


def host_path(s):
    c = Clock()
    ref, est = c.stage('decoding', lambda: (md.extract_notes_wo_velocity(s['onset'], s['frame'], rule='rule2'),
                                            md.extract_notes_wo_velocity(s['pred_onset'], s['pred_frame'], rule='rule2', **CLEAN)))
    shape = s['frame'].shape
    lists = c.stage('per-frame pitch lists', lambda: (ev._frames_to_eval_units(*md.notes_to_frames(*ref, shape)),
                                                      ev._frames_to_eval_units(*md.notes_to_frames(*est, shape))))
    notes = c.stage('note matching (two calls)', lambda: note_metrics(ref, est, ev.match_notes))
    frames = c.stage('frame metrics', lambda: ev.evaluate_frames(*lists[0], *lists[1]))
    ap = c.stage('AP', lambda: average_precision_score(s['frame'].cpu().flatten().numpy(), s['pred_frame'].cpu().flatten().numpy()))
    return c.t, (len(ref[0]), len(est[0]), notes, frames, ap)


def device_path(s):
    c = Clock()
    ref, est = c.stage('decoding', lambda: (md.extract_notes_wo_velocity_device(s['onset'], s['frame'], rule='rule2'),
                                            md.extract_notes_wo_velocity_device(s['pred_onset'], s['pred_frame'], rule='rule2', **CLEAN)))
    c.t['per-frame pitch lists'] = 0.0                                 # not built on this path
    notes = c.stage('note matching (two calls)', lambda: note_metrics(ref[:2], est[:2], ev.match_notes_sparse))
    frames = c.stage('frame metrics', lambda: ev.evaluate_frames_device(ref[2], est[2]))
    ap = c.stage('AP', lambda: ev.average_precision_device(s['frame'].flatten(), s['pred_frame'].flatten()))
    return c.t, (len(ref[0]), len(est[0]), notes, frames, ap)


def median_run(path, song, repeats):
    path(song)                                                         # warm-up: code objects, allocator, sort workspace
    runs = [path(song) for _ in range(repeats)]
    times = {k: statistics.median(r[0][k] for r in runs) for k in STAGES}
    totals = [sum(r[0].values()) for r in runs]
    return times, statistics.median(totals), (min(totals), max(totals)), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=18750)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--device-repeats', type=int, default=10)
    ap.add_argument('--min-frames', type=int, default=1)
    ap.add_argument('--bridge-gap', type=int, default=0)
    a = ap.parse_args()
    CLEAN.update(min_frames=a.min_frames, bridge_gap=a.bridge_gap)
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval: needs a HIP device (the device path has no CPU fallback; a CPU timing says nothing about it)')
    dev = torch.device('cuda:0')
    song = {k: torch.from_numpy(v).to(dev) for k, v in make_song(a.frames).items()}
    host_t, host_total, host_span, host_res = median_run(host_path, song, a.host_repeats)
    dev_t, dev_total, dev_span, dev_res = median_run(device_path, song, a.device_repeats)
    same = host_res[:4] == dev_res[:4] and abs(host_res[4] - dev_res[4]) <= 1e-9
    print(f'song: {a.frames} frames, {host_res[0]} reference notes, {host_res[1]} estimated notes; '
          f'note f1 {host_res[2][0][2]:.4f}, frame precision {host_res[3]["Precision"]:.4f}, AP {host_res[4]:.4f}')
    print(f'results identical (notes, note metrics, frame metrics; AP within 1e-9): {same}')
    print(f'median of {a.host_repeats} host / {a.device_repeats} device runs after one warm-up each, seconds per song')
    print(f'{"stage":28s} {"host":>10s} {"device":>10s} {"host/device":>12s}')
    for k in STAGES:
        ratio = f'{host_t[k] / dev_t[k]:12.1f}' if dev_t[k] > 0 else f'{"-":>12s}'
        print(f'{k:28s} {host_t[k]:10.4f} {dev_t[k]:10.4f} {ratio}')
    print(f'{"total":28s} {host_total:10.4f} {dev_total:10.4f} {host_total / dev_total:12.1f}')
    print(f'total, min..max over the runs: host {host_span[0]:.4f}..{host_span[1]:.4f}, device {dev_span[0]:.4f}..{dev_span[1]:.4f}')
    print(json.dumps({'frames': a.frames, 'min_frames': a.min_frames, 'bridge_gap': a.bridge_gap, 'ref_notes': host_res[0], 'est_notes': host_res[1], 'identical': bool(same),
                      'host_total_s': host_total, 'device_total_s': dev_total, 'host_stages_s': host_t, 'device_stages_s': dev_t}))
    if not same:
        raise SystemExit('bench_eval: the two paths disagree')


if __name__ == '__main__':
    main()
