"""Synthesiser throughput (rv_synth_render; profiles/synth_render.txt keeps the output): one 60 s track of
`synth.random_score` in the 'struck' voice, and the default small corpus of `train_on=Rendered` (84 tracks of 41.5 s).  Kernel times
are HIP-event times of single launches after warm-up launches of the same shape (median, min .. max); the host side -- partial table,
tile lists, upload -- is wall clock and reported separately, as is the float64 NumPy yardstick on the same track on the same box.
A TERM is one (row, sample) pair of the definition; the kernel also evaluates, and masks, the rest of every 256-sample wave span a
row touches (`executed`).  The share of the f32 vector rate counts VALU_PER_TERM vector instructions per executed term -- the 382
vector instructions of the compiled row loop's body for four samples -- against one instruction per lane and clock, half the 157.3
TFLOP/s an FMA-only stream would reach."""
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from reconvat_amd import _lib, synth
from reconvat_amd._lib import call, ptr, stream

F32_VECTOR_PEAK = 157.3e12          # FLOP/s, an FMA counted as two
VALU_PER_TERM = 382 / 4

if not torch.cuda.is_available():
    raise SystemExit('bench_synth.py measures on the GPU; there is none')
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)


def term_counts(rows, n):
    s = rows[:, 0].view(np.int32).astype(np.int64)
    end = np.minimum(rows[:, 1].view(np.int32).astype(np.int64) + rows[:, 7].view(np.int32), n)
    live = end > s
    useful = int((end - s)[live].sum())
    executed = int((((end[live] - 1) // 256 - s[live] // 256 + 1) * 256).sum())
    return useful, executed


def one_track(seconds=60.0, reps=20):
    n = int(seconds * 16000)
    notes = synth.random_score(np.random.RandomState(0), seconds)
    timbre = synth.Timbre('struck', 0)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        rows = synth.partials(notes, timbre)
        t1 = time.perf_counter()
        n_tiles = -(-n // synth.TILE)
        tile_ptr, tile_rows = synth.tile_lists(rows, n_tiles)
        t2 = time.perf_counter()
        d_rows = torch.from_numpy(rows.view(np.int32).reshape(-1)).to(dev)
        d_ptr, d_list = torch.from_numpy(tile_ptr).to(dev), torch.from_numpy(tile_rows).to(dev)
        torch.cuda.synchronize()
        host.append((t1 - t0, t2 - t1, time.perf_counter() - t2))
    useful, executed = term_counts(rows, n)
    out = {}
    for name, dtype in (('int16', torch.int16), ('float32', torch.float32)):
        y = torch.empty(n, dtype=dtype, device=dev)
        args = (ptr(d_rows), len(rows), ptr(d_ptr), ptr(d_list), n_tiles, 0, n, ptr(y), synth.OUT_DTYPES[dtype])
        for _ in range(3):
            call('rv_synth_render', *args, stream())
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call('rv_synth_render', *args, stream())
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e-3)
        out[name] = (float(np.median(times)), min(times), max(times))
    t0 = time.perf_counter()
    y64 = synth.render_host(rows, 0, n)
    t_numpy = time.perf_counter() - t0
    diff = np.abs(synth.to_int16(y64).astype(np.int64) - y.mul(32768.0).round().clamp(-32768, 32767).cpu().numpy().astype(np.int64))
    med = out['int16'][0]
    h = np.median(np.array(host), axis=0)
    print(f'one track: {seconds:.0f} s, {len(notes)} notes, {len(rows)} partial rows, {len(tile_rows)} tile-list entries over {n_tiles} tiles; '
          f'{useful / 1e6:.2f} M terms ({executed / 1e6:.2f} M executed)')
    for name in out:
        m, lo, hi = out[name]
        print(f'  rv_synth_render -> {name:8}: {m * 1e3:8.3f} ms per launch [{lo * 1e3:.3f} .. {hi * 1e3:.3f}], median of {reps} after 3 warm-up launches')
    print(f'  terms per second          : {useful / med / 1e9:8.2f} G useful, {executed / med / 1e9:.2f} G executed')
    print(f'  share of the f32 vector rate: {executed / med * VALU_PER_TERM / (F32_VECTOR_PEAK / 2):.1%} '
          f'({VALU_PER_TERM:.1f} vector instructions per executed term against {F32_VECTOR_PEAK / 2e12:.2f} T lane-instructions/s)')
    print(f'  host, median of 5          : partials {h[0] * 1e3:.2f} ms, tile lists {h[1] * 1e3:.2f} ms, upload {h[2] * 1e3:.2f} ms')
    print(f'  NumPy yardstick (float64, render_host, one run): {t_numpy:.2f} s = {useful / t_numpy / 1e6:.1f} M terms/s; '
          f'{t_numpy / med:.0f} x the kernel; int16 of the two differ in {int((diff != 0).sum())} of {n} samples, by at most {int(diff.max())}')
    return dict(seconds=seconds, notes=len(notes), rows=len(rows), terms=useful, executed_terms=executed, kernel_ms_int16=med * 1e3,
                kernel_ms_float32=out['float32'][0] * 1e3, terms_per_s=useful / med, valu_share=executed / med * VALU_PER_TERM / (F32_VECTOR_PEAK / 2),
                host_partials_ms=h[0] * 1e3, host_tiles_ms=h[1] * 1e3, host_upload_ms=h[2] * 1e3, numpy_s=t_numpy)


def small_corpus():
    """prepare_VAT_dataset('Rendered', small=True) at the default sequence length: wall clock of the whole call (scores, tables,
    kernel, copy of the int16 audio back to the host, label rolls) and, inside it, the event time of every rv_synth_render launch."""
    from reconvat_amd.dataset import prepare_VAT_dataset
    events = []

    def hook(name, args, fn):
        if name != 'rv_synth_render':
            return fn(*args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(*args)
        e1.record()
        events.append((e0, e1))
        return rc
    prepare_VAT_dataset(32768, 32768, False, dev, small=True, supersmall=True, dataset='Rendered')          # warm-up
    _lib.HOOK[0] = hook
    t0 = time.perf_counter()
    sets = prepare_VAT_dataset(327680, 327680, False, dev, small=True, dataset='Rendered')
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    _lib.HOOK[0] = None
    kernel = sum(a.elapsed_time(b) for a, b in events) * 1e-3
    tracks = sum(len(d.data) for d in sets[:2]) + len(sets[3].data)
    samples = sum(len(t['audio']) for d in (sets[0], sets[1], sets[3]) for t in d.data)
    peak = max(int(t['audio'].abs().max()) for d in sets for t in d.data)
    print(f'small corpus: {tracks} tracks, {samples / 16000:.0f} s of audio, {len(events)} launches: {wall:.2f} s wall for prepare_VAT_dataset, '
          f'{kernel * 1e3:.1f} ms of it in rv_synth_render; largest |sample| {peak} of 32767')
    return dict(tracks=tracks, audio_s=samples / 16000, wall_s=wall, kernel_ms=kernel * 1e3, peak=peak)


res = {'track': one_track(), 'corpus': small_corpus()}
print(json.dumps(res))
