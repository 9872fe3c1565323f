"""The Viterbi note decoder (rv_hmm_decode; profiles/hmm_decode.txt keeps the output) on a ten-minute roll:

    T = 18 750 frames of random "posteriorgrams" (the construction of tests/sweep_cases.py::random_rolls, inline), G = 1 and G = 16
    parameter sets, next to the threshold decoder (rv_eval_decode) on the same roll -- the floor of "read both rolls once and write
    one byte roll" -- and to the host definition (reconvat_amd/hmm.py::viterbi_states, NumPy, wall clock, one set).

Times are HIP-event times on the launch stream around one call (all its launches), warm, the median of REPS windows of INNER calls
each; no clock or device setting is touched.  Before any time is printed the device result is compared with the host definition
(G = 1: states and cost, ==).  `--trace 1|16|eval` only issues CALLS calls of one configuration and prints nothing: run under
`rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/bench_hmm.py --trace 16` it gives the split per launch
(kernel names hmm_*_k), in a run of its own.

`--rendered <checkpoint>` measures accuracy instead (one seed, rendered audio; no pass mark): with a model trained by the command in
profiles/rendered_f1.txt it chooses a decoder on the validation split of train_on=Rendered -- `tune_thresholds` over 0.1 .. 0.9 squared
and the clean-up pairs (1, 0), (2, 0), (2, 1), (3, 1), and `tune_hmm` over thresholds {0.3, 0.5, 0.7}^2 x penalties {0, 1, 2, 4}^3 = 576
sets (three calls of 192, one per onset threshold) -- and evaluates both choices and the plain 0.5 / 0.5 decoder on the held-out whole
songs: frame, note and note-with-offsets F1 as mean +- std over the songs.  (The validation items are crops of those same held-out
tracks: `prepare_VAT_dataset` has no third split for this corpus.)"""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from reconvat_amd import NoteHMM, _lib, decoding, hmm as nh

REPS, INNER, CALLS, T = 21, 10, 20, 18750

if not torch.cuda.is_available():
    raise SystemExit('bench_hmm.py measures on the GPU; there is none')
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)


def rolls(T, seed=3, density=0.06):
    """Two float32 [T, 88] rolls in [0, 1]: notes at random levels with moved ends and false alarms on time-smoothed noise."""
    rng = np.random.RandomState(seed)
    on, fr = np.zeros((T, 88), np.float32), np.zeros((T, 88), np.float32)
    for _ in range(int(T * 88 * density / 8)):
        t0, p, ln, level = rng.randint(0, T), rng.randint(0, 88), rng.randint(1, 25), rng.uniform(0.25, 1.0)
        on[t0, p] = level
        fr[t0:min(T, t0 + ln), p] = level
    for roll in (on, fr):
        noise = rng.uniform(0, 0.6, size=(T + 2, 88)).astype(np.float32)
        roll[:] = np.clip(np.maximum(roll, 0.25 * noise[:-2] + 0.5 * noise[1:-1] + 0.25 * noise[2:]), 0, 1)
    return on, fr


def timed(fn):
    """Median, min and max over REPS windows of the HIP-event time of INNER calls, per call, in microseconds (after a warm-up window)."""
    for _ in range(INNER):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0 / INNER)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def hmm_call(on, fr, hmms):
    """One rv_hmm_decode on preallocated buffers: what the call costs without the allocations of the Python wrapper."""
    G = len(hmms)
    tables = torch.from_numpy(np.stack([h.tables()[0] for h in hmms]).view(np.int16)).to(dev)
    trans = np.ascontiguousarray(np.stack([h.tables()[1] for h in hmms]))
    states = torch.empty((G, T, 88), dtype=torch.uint8, device=dev)
    cost = torch.empty((G, 88), dtype=torch.int64, device=dev)
    ws_bytes = _lib.load().rv_hmm_workspace_bytes(T, G)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    args = (on.data_ptr(), fr.data_ptr(), T, tables.data_ptr(), trans.ctypes.data, G, states.data_ptr(), cost.data_ptr(), ws.data_ptr(),
            ws_bytes, _lib.stream())
    keep = (tables, trans, states, cost, ws)
    return (lambda: _lib.call('rv_hmm_decode', *args)), keep, ws_bytes


def eval_call(on, fr):
    max_notes = 88 * ((T + 1) // 2)
    ws_bytes = _lib.load().rv_eval_workspace_bytes(T)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    notes = torch.empty((max_notes, 3), dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    painted = torch.empty((T, 88), dtype=torch.uint8, device=dev)
    args = (on.data_ptr(), fr.data_ptr(), T, 0.5, 0.5, 2, notes.data_ptr(), max_notes, count.data_ptr(), painted.data_ptr(), ws.data_ptr(),
            ws_bytes, _lib.stream())
    return (lambda: _lib.call('rv_eval_decode', *args)), (ws, notes, count, painted)


def rendered(checkpoint):
    from reconvat_amd import evaluate as ev
    from reconvat_amd.dataset import prepare_VAT_dataset
    from transcribe_files import load_model
    model = load_model(checkpoint, 'Mel', str(dev))
    _, _, val, full = prepare_VAT_dataset(sequence_length=327680, validation_length=327680, refresh=False, device=str(dev), small=True,
                                          dataset='Rendered')
    keys = {'frame': 'metric/frame/f1', 'note': 'metric/note/f1', 'note-with-offsets': 'metric/note-with-offsets/f1'}
    out = {'checkpoint': os.path.basename(checkpoint), 'validation_items': len(val), 'held_out_songs': len(full)}
    with torch.no_grad():
        grid = [round(0.1 * k, 1) for k in range(1, 10)]
        t0 = time.perf_counter()
        thr = ev.tune_thresholds(val, model, grid, grid, cleanups=[[1, 0], [2, 0], [2, 1], [3, 1]])
        out['tune_thresholds_s'] = time.perf_counter() - t0
        t0, best = time.perf_counter(), None
        for on_thr in (0.3, 0.5, 0.7):          # 192 sets per call, under tune_hmm's limit of 256
            res = ev.tune_hmm(val, model, nh.hmm_grid([on_thr], [0.3, 0.5, 0.7], [0, 1, 2, 4], [0, 1, 2, 4], [0, 1, 2, 4]))
            if best is None or res['best_value'] > best['best_value']:
                best = res
        out['tune_hmm_s'] = time.perf_counter() - t0
        default = ev.tune_hmm(val, model, [NoteHMM()])
        out['validation_note_f1'] = {'thresholds': thr['best_value'], 'hmm': best['best_value'], 'hmm_default_2_2_2': default['best_value']}
        choices = {'plain 0.5 / 0.5': {},
                   'tune_thresholds': dict(onset_threshold=thr['onset_threshold'], frame_threshold=thr['frame_threshold'],
                                           min_frames=thr['min_frames'], bridge_gap=thr['bridge_gap']),
                   'tune_hmm': dict(hmm=best['best']), 'hmm default (2, 2, 2)': dict(hmm=NoteHMM())}
        out['chosen'] = {'tune_thresholds': choices['tune_thresholds'], 'tune_hmm': best['best'].as_dict()}
        out['held_out'] = {}
        for name, kw in choices.items():
            m = ev.evaluate_wo_velocity(full, model, reconstruction=False, device_metrics=True, **kw)
            out['held_out'][name] = {k: [float(np.mean(m[key])), float(np.std(m[key]))] for k, key in keys.items()}
    print(f"validation note F1: thresholds {thr['best_value']:.4f} at {out['chosen']['tune_thresholds']}; hmm {best['best_value']:.4f} at "
          f"{best['best']!r}; hmm at the default penalties {default['best_value']:.4f}")
    print(f"tune_thresholds (81 pairs x 4 clean-ups) {out['tune_thresholds_s']:.1f} s, tune_hmm (576 sets) {out['tune_hmm_s']:.1f} s, "
          f"{len(val)} validation items")
    for name, r in out['held_out'].items():
        print(f'{name:24s}' + '   '.join(f'{k} F1 {v[0]:.3f} +- {v[1]:.3f}' for k, v in r.items()))
    print(json.dumps(out))


if '--rendered' in sys.argv:
    rendered(sys.argv[sys.argv.index('--rendered') + 1])
    raise SystemExit(0)

on_h, fr_h = rolls(T)
on, fr = torch.from_numpy(on_h).to(dev), torch.from_numpy(fr_h).to(dev)
grid = nh.hmm_grid([0.3, 0.5], [0.5, 0.7], [0.0, 2.0], [1.0, 2.0], [2.0])
assert len(grid) == 16
one, keep1, ws1 = hmm_call(on, fr, [NoteHMM()])
sixteen, keep16, ws16 = hmm_call(on, fr, grid)
floor, keep0 = eval_call(on, fr)

if '--trace' in sys.argv:
    fn = {'1': one, '16': sixteen, 'eval': floor}[sys.argv[sys.argv.index('--trace') + 1]]
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    raise SystemExit(0)

t0 = time.perf_counter()
want_states, want_cost = nh.viterbi_states(on_h, fr_h, *NoteHMM().tables())
host_s = time.perf_counter() - t0
one()
torch.cuda.synchronize()
assert np.array_equal(keep1[2][0].cpu().numpy(), want_states) and np.array_equal(keep1[3][0].cpu().numpy(), want_cost)
notes = len(nh.extract_notes_hmm_device(on, fr, [NoteHMM()])[0][0])
result = {'T': T, 'reps': REPS, 'inner': INNER, 'host_definition_s': host_s, 'notes_default_model': notes,
          'roll_bytes_read': 2 * T * 88 * 4}
for name, fn, G, ws in (('hmm_G1', one, 1, ws1), ('hmm_G16', sixteen, 16, ws16), ('eval_decode', floor, 0, 0)):
    med, lo, hi = timed(fn)
    result[name] = {'us': med, 'us_min_max': [lo, hi], 'workspace_bytes': ws}
    per_set = f'  ({med / G:8.1f} us per set)' if G > 1 else ''
    print(f'{name:12s} T = {T}  {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}){per_set}')
print(f'host definition (NumPy, one set): {host_s:.2f} s; the device decode equals it (states and cost, ==); {notes} notes at the default model')
print(json.dumps(result))
