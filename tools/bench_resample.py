"""Resampler throughput: one hour of 44.1 kHz stereo int16 -> 16 kHz mono int16 on the device (rv_resample, the source
resident in HBM, the chunked launches of reconvat_amd.resample.Resampler) next to resample_host on this machine's CPUs.

    python tools/bench_resample.py [--seconds 3600] [--runs 20] [--warmup 5] [--host-seconds 600] [--out profiles/NAME.json]

Kernel time = median over `runs` of the HIP-event time of one whole conversion.  Bytes = what the operation must move (every input
sample once, every output sample once); MACs = outputs x non-zero taps per output.  The host path is timed on `host-seconds` of the
same signal (it is linear in the length) with the worker threads resample_host picks (OMP_NUM_THREADS, at most 16).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from reconvat_amd.resample import Resampler, resample_host

ap = argparse.ArgumentParser()
ap.add_argument('--seconds', type=int, default=3600)
ap.add_argument('--runs', type=int, default=20)
ap.add_argument('--warmup', type=int, default=5)
ap.add_argument('--host-seconds', type=int, default=600)
ap.add_argument('--sr-in', type=int, default=44100)
ap.add_argument('--out', default=None)
a = ap.parse_args()
assert a.runs >= 1 and a.warmup >= 0

dev = torch.device('cuda:0')
sr_in, sr_out, C = a.sr_in, 16000, 2
T = a.seconds * sr_in
g = torch.Generator().manual_seed(0)
x = torch.randint(-20000, 20000, (T, C), generator=g, dtype=torch.int16)
rs = Resampler(sr_in, sr_out, dev, out_dtype=torch.int16)
xd = x.to(dev)
for _ in range(a.warmup):
    y = rs(xd)
torch.cuda.synchronize()
times = []
for _ in range(a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    y = rs(xd)
    e1.record()
    e1.synchronize()
    times.append(e0.elapsed_time(e1) * 1e-3)
t_dev = statistics.median(times)
n_out = y.numel()
moved = T * C * 2 + n_out * 2
macs = n_out * rs.taps

Th = min(T, a.host_seconds * sr_in)
xh = x[:Th].numpy()
resample_host(xh[:sr_in], sr_in, sr_out, out_dtype=np.int16)                    # warm-up: imports, filter design
t0 = time.perf_counter()
yh = resample_host(xh, sr_in, sr_out, out_dtype=np.int16)
t_host = (time.perf_counter() - t0) * (T / Th)
n_cmp = len(yh) - 200 if Th < T else len(yh)                                    # the shortened host signal ends early: skip its tail
lsb = int(np.max(np.abs(yh[:n_cmp].astype(np.int64) - y[:n_cmp].cpu().numpy().astype(np.int64))))
line = {
    'tool': 'bench_resample', 'sr_in': sr_in, 'sr_out': sr_out, 'channels': C, 'audio_seconds': a.seconds, 'outputs': n_out,
    'taps_per_output': rs.taps, 'bank_bytes': rs.bank.numel() * 4, 'runs': a.runs, 'warmup': a.warmup,
    'kernel_ms_median': round(t_dev * 1e3, 4), 'kernel_ms_min': round(min(times) * 1e3, 4), 'kernel_ms_max': round(max(times) * 1e3, 4),
    'audio_hours_per_s': round(a.seconds / 3600 / t_dev, 2), 'bytes_moved': moved, 'achieved_GBps': round(moved / t_dev * 1e-9, 2),
    'GMACps': round(macs / t_dev * 1e-9, 2),
    'host_s_per_hour_audio': round(t_host * 3600 / a.seconds, 3), 'host_seconds_timed': Th // sr_in,
    'host_audio_hours_per_s': round(a.seconds / 3600 / t_host, 4), 'device_over_host': round(t_host / t_dev, 1),
    'max_lsb_device_vs_host': lsb,
}
print(json.dumps(line))
if a.out:
    with open(a.out, 'w') as fh:
        fh.write(json.dumps(line) + '\n')
