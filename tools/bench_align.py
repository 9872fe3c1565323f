"""Score-to-recording alignment (rv_align_cost, rv_align_dtw; profiles/align_dtw.txt keeps the output): one rendered
ten-minute pair, and a batch of 32 one-minute pairs in one launch per stage.  A pair is a `synth.random_score` rendered plainly (the
score) and, through t' = 0.4 + 1.15 t + 0.5 sin(2 pi t / 7), in another timbre with white noise (the recording).  Stage times are
HIP-event times around each launch of the stage (recorded through the _lib.HOOK of every launch the host makes), median of REPS runs
of the whole chain after one warm-up run; the host side of the chain (feature ops, band construction, copies) is in the wall clock
only.  The NumPy yardstick (`cost_host`, `dtw_host`) runs once on the same features on the same box; before any time is printed its
integers are compared: every cost cell within 1, and -- on the device's own cost matrices -- total, path length and the four path
arrays equal."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from reconvat_amd import _lib, align, synth

REPS = 5
STAGES = ('rv_melspec_lognorm_fwd', 'coarse rv_align_cost', 'coarse rv_align_dtw', 'fine rv_align_cost', 'fine rv_align_dtw')

if not torch.cuda.is_available():
    raise SystemExit('bench_align.py measures on the GPU; there is none')
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)
warp = lambda t: 0.4 + 1.15 * t + 0.5 * np.sin(2.0 * np.pi * t / 7.0)


def make_pair(seed, seconds):
    """(recording int16 tensor, score int16 tensor) on the device, both rendered there."""
    notes = synth.random_score(np.random.RandomState(seed), seconds)
    warped = notes.copy()
    warped[:, 0], warped[:, 1] = warp(notes[:, 0]), warp(notes[:, 1])
    score = synth.render(notes, align.score_length(notes), synth.Timbre('struck', 0), device=dev, out_dtype=torch.int16)
    rec = synth.render(warped, align.score_length(warped), synth.Timbre('struck', 7 + seed), device=dev, out_dtype=torch.float32)
    noise = torch.from_numpy(np.random.RandomState(1000 + seed).randn(rec.numel()).astype(np.float32)).to(dev)
    rec = (rec + 5e-4 * noise).mul(32768.0).round().clamp(-32768, 32767).to(torch.int16)
    return rec, score


def chain(audio, radius=125, coarse=8):
    """The stages of align.align_logmels, with everything kept: logmels, bands, the device's cost matrices and the results."""
    tag = ['']

    def hook(name, args, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        events.setdefault(tag[0] + name, []).append((e0, e1))
        return rc
    events = {}
    _lib.HOOK[0] = hook
    try:
        t0 = time.perf_counter()
        lm = [(align.logmel(r, dev), align.logmel(s, dev)) for r, s in audio]
        shapes = [(x.shape[0], y.shape[0]) for x, y in lm]
        Ss = [align.coarse_factor(M, coarse) for _, M in shapes]
        cpairs = [(align.features(x, S), align.features(y, S)) for (x, y), S in zip(lm, Ss)]
        clos, cWs = [np.zeros(len(x), dtype=np.int32) for x, _ in cpairs], [len(y) for _, y in cpairs]
        tag[0] = 'coarse '
        ccost, clay = align.cost_device(cpairs, clos, cWs, dev)
        cres = align.dtw_device(ccost, clos, cWs, cWs, dev)
        bands = [align.band_from_coarse(r['row_lo'], N, M, S, radius) for r, (N, M), S in zip(cres, shapes, Ss)]
        los, Ws = [b[0] for b in bands], [b[1] for b in bands]
        fpairs = [(align.features(x), align.features(y)) for x, y in lm]
        tag[0] = 'fine '
        fcost, flay = align.cost_device(fpairs, los, Ws, dev)
        fres = align.dtw_device(fcost, los, Ws, [M for _, M in shapes], dev)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        _lib.HOOK[0] = None
    ms = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in events.items()}
    return dict(ms=ms, wall=wall, shapes=shapes, Ss=Ss, coarse=(cpairs, clos, cWs, ccost, clay, cres), fine=(fpairs, los, Ws, fcost, flay, fres))


def yardstick(run, label):
    """cost_host / dtw_host on the run's features and on the device's cost matrices; asserts the integers, returns the host seconds."""
    secs = {}
    for name in ('coarse', 'fine'):
        pairs, los, Ws, cost, lay, res = run[name]
        dev_cost = lay.split_cells(cost.cpu().numpy().view(np.uint16))
        t_cost = t_dtw = 0.0
        differ, cells = 0, 0
        for p, ((x, y), lo, W) in enumerate(zip(pairs, los, Ws)):
            x, y = x.cpu().numpy(), y.cpu().numpy()
            t0 = time.perf_counter()
            want = align.cost_host(x, y, lo, W)
            t1 = time.perf_counter()
            host = align.dtw_host(dev_cost[p], lo, W, len(y))
            t2 = time.perf_counter()
            t_cost, t_dtw = t_cost + t1 - t0, t_dtw + t2 - t1
            live = want != align.DEAD
            diff = np.abs(want.astype(np.int64) - dev_cost[p].astype(np.int64))
            assert (dev_cost[p][~live] == align.DEAD).all() and diff[live].max() <= 1, (label, name, p)
            differ, cells = differ + int((diff[live] != 0).sum()), cells + int(live.sum())
            assert host['total'] == res[p]['total'] and host['length'] == res[p]['length'], (label, name, p)
            for key in ('row_lo', 'row_hi', 'col_lo', 'col_hi'):
                assert np.array_equal(host[key], res[p][key]), (label, name, p, key)
        secs[name] = (t_cost, t_dtw, differ, cells)
    return secs


def report(label, audio):
    chain(audio)                                             # warm-up: tables, LDS attribute, allocator
    runs = [chain(audio) for _ in range(REPS)]
    run = runs[-1]
    host = yardstick(run, label)
    med = {k: float(np.median([r['ms'][k] for r in runs])) for k in STAGES}
    wall = float(np.median([r['wall'] for r in runs]))
    shapes, (_, _, cWs, _, clay, _), (_, _, Ws, _, flay, fres) = run['shapes'], run['coarse'], run['fine']
    print(f'{label}: {len(shapes)} pair(s); first pair N = {shapes[0][0]}, M = {shapes[0][1]} frames, S = {run["Ss"][0]}, coarse matrix '
          f'{shapes[0][0] // run["Ss"][0]} x {cWs[0]}, fine band W = {Ws[0]}; {clay.n_cells / 1e6:.2f} M coarse and {flay.n_cells / 1e6:.2f} M fine cells in all; '
          f'path length {fres[0]["length"]}, mean cost {fres[0]["total"] / (align.QUANT * float(sum(shapes[0]))):.4f}')
    print(f'  device, median of {REPS} runs after one warm-up run (HIP events around each launch):')
    for k in STAGES:
        print(f'    {k:24}: {med[k]:9.3f} ms')
    print(f'    whole chain, wall clock : {wall * 1e3:9.1f} ms (features, band construction, uploads and read-backs included)')
    print('  NumPy yardstick on the same features, one run; its integers were compared first (cost cells within 1, DTW outputs equal):')
    for name in ('coarse', 'fine'):
        t_cost, t_dtw, differ, cells = host[name]
        print(f'    {name:6} cost_host {t_cost:7.2f} s   dtw_host {t_dtw:7.2f} s   ({differ} of {cells} cost cells differ by 1)')
    return dict(label=label, pairs=len(shapes), N=shapes[0][0], M=shapes[0][1], W=Ws[0], coarse_cells=clay.n_cells, fine_cells=flay.n_cells,
                device_ms=med, wall_ms=wall * 1e3, host_s={k: v[:2] for k, v in host.items()})


def backtrack_split(n=2048):
    """Recurrence and backtrack apart: two n x n full matrices whose recurrence does the same loads and stores on 2 n - 1 diagonals,
    one with its path on the diagonal (n cells), one with its path along the first row and the last column (2 n - 1 cells).  The
    difference of the launch times over the n - 1 extra cells is the time of one step of the walk back."""
    lo = np.zeros(n, dtype=np.int32)
    straight = np.full((n, n), 4095, dtype=np.uint16)
    straight[np.arange(n), np.arange(n)] = 0
    hooked = np.full((n, n), 4095, dtype=np.uint16)
    hooked[0, :] = 0
    hooked[:, n - 1] = 0
    times, lengths = {}, {}

    def hook(name, args, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        events.append((e0, e1))
        return rc
    for label, cost in (('straight', straight), ('hooked', hooked)):
        want = align.dtw_host(cost, lo, n, n)
        events = []
        _lib.HOOK[0] = hook
        try:
            for _ in range(REPS + 1):
                got = align.dtw_device([cost], [lo], [n], [n], dev)[0]
        finally:
            _lib.HOOK[0] = None
        assert got['total'] == want['total'] and got['length'] == want['length'] and np.array_equal(got['col_lo'], want['col_lo'])
        times[label] = float(np.median([a.elapsed_time(b) for a, b in events[1:]]))
        lengths[label] = got['length']
    step = (times['hooked'] - times['straight']) / (lengths['hooked'] - lengths['straight'])
    diag = (times['straight'] - step * lengths['straight']) / (2 * n - 1)
    print(f'recurrence and backtrack apart: {n} x {n} full matrix, {2 * n - 1} diagonals, block of 1024; path of {lengths["straight"]} cells '
          f'{times["straight"]:.3f} ms, path of {lengths["hooked"]} cells {times["hooked"]:.3f} ms (medians of {REPS})')
    print(f'  one step of the walk back: {step * 1e3:.3f} us; one diagonal of the recurrence (2 rows per work item at most): {diag * 1e3:.3f} us')
    return dict(n=n, ms=times, lengths=lengths, backtrack_step_us=step * 1e3, diagonal_us=diag * 1e3)


res = [report('ten-minute pair', [make_pair(0, 600.0)]), report('32 one-minute pairs', [make_pair(100 + i, 60.0) for i in range(32)]),
       backtrack_split()]
print(json.dumps(res))
