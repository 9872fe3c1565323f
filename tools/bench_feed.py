"""Data-feed throughput: DeviceCorpus (rv_crop_segments) vs the reference-style host path (per-item slicing, float
conversion, DataLoader collate, host->device copy) on the same synthetic corpus, batch 8 x 327 680 samples -- and, in the same
process, the feed with pitch_shift=6 (rv_crop_segments_shift; profiles/feed_pitch_shift.txt keeps that line).
`--acoustics` runs the acoustic-augmentation leg alone (rv_fir_items; profiles/feed_acoustics.txt keeps its table)."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch.utils.data import DataLoader
from reconvat_amd.feed import DeviceCorpus
from reconvat_amd.dataset import PianoRollAudioDataset

dev = torch.device('cuda:0')
F32_MATRIX_PEAK = 157.3e12          # FLOP/s of the f32 matrix pipe


def acoustics_leg():
    """`--acoustics` (profiles/feed_acoustics.txt keeps the table): rv_fir_items alone on B = 8 items of 327 680 samples
    for taps in {1024, 2048, 4096, 8192}, median of 30 HIP-event times per launch after 5 warm-up launches of the same shape; the
    executed work is 2 W n B FLOP (W = taps + 64, zero taps included) and the share of peak is that over the f32 matrix peak.  Then
    the host side: drawing the parameters, building and uploading one batch's filters (wall clock around a device synchronise)."""
    from reconvat_amd import acoustics
    from reconvat_amd._lib import call, ptr, stream
    if not torch.cuda.is_available():
        raise SystemExit('bench_feed.py --acoustics measures on the GPU; there is none')
    B, n = 8, 327680
    x = torch.rand(B, n, device=dev) * 2 - 1
    y = torch.empty_like(x)
    print(f'rv_fir_items, B = {B} items of {n} samples, noise on; median of 30 launches (HIP events), min .. max in brackets')
    print(f'{"taps":>6} {"W":>6} {"us/launch":>12} {"[min .. max]":>22} {"GFLOP":>8} {"TFLOP/s":>8} {"of f32 matrix peak":>19} {"host build+upload ms":>21}')
    for taps in (1024, 2048, 4096, 8192):
        a = acoustics.Acoustics(rt60=0.5, eq_db=6.0, noise_db=-50.0, taps=taps)
        W = a.width
        rs = np.random.RandomState(taps)
        pinned = torch.empty(B * (W + 2), dtype=torch.float32).pin_memory()

        def build():
            params = [acoustics.draw(rs, a) for _ in range(B)]
            h = np.stack([acoustics.item_filter(p)[0] for p in params]).astype(np.float32)
            pinned[:B * W] = torch.from_numpy(h.reshape(-1))
            pinned[B * W:B * W + B] = torch.from_numpy(np.array([p['seed'] for p in params], dtype=np.uint32).view(np.float32))
            pinned[B * W + B:] = torch.from_numpy(np.array([p['amp'] for p in params], dtype=np.float32))
            return pinned.to(dev, non_blocking=True)
        fir = build()
        torch.cuda.synchronize()
        host = []
        for _ in range(10):
            t0 = time.perf_counter()
            fir = build()
            torch.cuda.synchronize()
            host.append(time.perf_counter() - t0)
        args = (ptr(x), n, ptr(fir), W, acoustics.LEAD, ptr(fir) + 4 * B * W, ptr(fir) + 4 * (B * W + B), B, n, ptr(y), n)
        for _ in range(5):
            call('rv_fir_items', *args, stream())
        torch.cuda.synchronize()
        times = []
        for _ in range(30):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call('rv_fir_items', *args, stream())
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3)
        us, flop = float(np.median(times)), 2.0 * W * n * B
        print(f'{taps:6d} {W:6d} {us:12.1f} {f"[{min(times):.1f} .. {max(times):.1f}]":>22} {flop / 1e9:8.2f} {flop / us / 1e6:8.2f} '
              f'{flop / (us * 1e-6) / F32_MATRIX_PEAK:18.1%} {float(np.median(host)) * 1e3:21.2f}')
    # the feed with the option on, end to end (crop + filter + host side), next to the plain feed
    rs = np.random.RandomState(5)
    tr = []
    for i in range(16):
        t = int(rs.randint(700_000, 900_000))
        steps = (t - 1) // 512 + 1
        tr.append({'path': f'track{i}.flac', 'audio': rs.randint(-32768, 32768, size=t).astype(np.int16),
                   'label': rs.randint(0, 4, size=(steps, 88)).astype(np.uint8), 'velocity': rs.randint(0, 128, size=(steps, 88)).astype(np.uint8)})
    for taps in (None, 4096):
        a = None if taps is None else acoustics.Acoustics(rt60=0.5, eq_db=6.0, noise_db=-50.0, taps=taps)
        dc = DeviceCorpus(tr, n, B, dev, acoustics=a, acoustics_seed=1)
        for _ in range(3):
            dc.batch(range(B))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(20):
            dc.batch([(i * B + j) % 16 for j in range(B)])
        torch.cuda.synchronize()
        print(f'DeviceCorpus.batch, acoustics {"off" if a is None else f"on ({taps} taps)"}: {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms/batch wall')


if '--acoustics' in sys.argv:
    acoustics_leg()
    sys.exit(0)

rng = np.random.RandomState(5)
tracks = []
for i in range(32):
    t = int(rng.randint(2_000_000, 3_000_000))
    steps = (t - 1) // 512 + 1
    tracks.append({'path': f'track{i}.flac', 'audio': rng.randint(-32768, 32768, size=t).astype(np.int16),
                   'label': rng.randint(0, 4, size=(steps, 88)).astype(np.uint8),
                   'velocity': rng.randint(0, 128, size=(steps, 88)).astype(np.uint8)})


class Mem(PianoRollAudioDataset):
    @classmethod
    def available_groups(cls):
        return ['g']

    def files(self, group):
        return [(i, None) for i in range(len(tracks))]

    def load(self, i, _):
        t = tracks[i]
        return dict(path=t['path'], audio=torch.from_numpy(t['audio']), label=torch.from_numpy(t['label']),
                    velocity=torch.from_numpy(t['velocity']))


dc = DeviceCorpus(tracks, 327680, 8, dev)
for _ in range(3):
    dc.batch(range(8))
torch.cuda.synchronize()
t0 = time.perf_counter()
n = 50
for i in range(n):
    b = dc.batch([(i * 8 + j) % 32 for j in range(8)])
torch.cuda.synchronize()
t_dev = (time.perf_counter() - t0) / n
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for i in range(20):
    dc.batch(range(8))
e1.record(); e1.synchronize()

ds = DeviceCorpus(tracks, 327680, 8, dev, pitch_shift=6, aug_seed=1)
for _ in range(3):
    ds.batch(range(8))
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(n):
    b = ds.batch([(i * 8 + j) % 32 for j in range(8)])
torch.cuda.synchronize()
t_shift = (time.perf_counter() - t0) / n
s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s0.record()
for i in range(20):
    ds.batch([(i * 8 + j) % 32 for j in range(8)])
s1.record(); s1.synchronize()
host = Mem('.', sequence_length=327680, device='cpu')
it = iter(DataLoader(host, 8, shuffle=True, drop_last=True))
t0 = time.perf_counter()
m = 0
for batch in it:
    for k in ('audio', 'onset', 'frame'):
        batch[k] = batch[k].to(dev)
    m += 1
torch.cuda.synchronize()
t_host = (time.perf_counter() - t0) / m
sec = 8 * 327680 / 16000
print(f'device feed : {t_dev * 1e3:7.3f} ms/batch wall ({sec / t_dev:9.0f} audio-s/s), {e0.elapsed_time(e1) / 20 * 1e3:.1f} us GPU time per batch')
print(f'pitch_shift=6: {t_shift * 1e3:7.3f} ms/batch wall ({sec / t_shift:9.0f} audio-s/s), {s0.elapsed_time(s1) / 20 * 1e3:.1f} us GPU time per batch '
      f'(k drawn per item from -6..6; the training step this feeds takes about 20 ms)')
print(f'host path   : {t_host * 1e3:7.3f} ms/batch wall ({sec / t_host:9.0f} audio-s/s)')
