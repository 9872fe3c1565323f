"""The optimiser kernel with and without the options of DESIGN 3.11, at the flat size of UNet_Onset.

    python tools/bench_optim.py [--rounds 15] [--launches 50]

Timed, alternating in ONE process (round r times one after the other; the medians over the rounds are reported with min..max):
  adam:  rv_adam_step -- the default step: p, m, v read and written, g read = 7 float streams per element;
  adamw: rv_adamw_step with weight decay, the clip coefficient (the norm is in place; its reduction is timed on its own line) and
         the averaged weights = 9 float streams per element;
  norm:  rv_reduce_mean(kind 3) over the gradient bucket -- the launch max_grad_norm adds in front of the kernel (1 read stream).
Each sample is `--launches` launches between two device events.  All streams together (14.6 MB each) fit the 256 MB last-level
cache, so the GB/s column -- bytes the algorithm moves over kernel time -- is not an HBM figure."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from reconvat_amd import UNet_Onset, ops
from reconvat_amd._lib import call, ptr, stream
from reconvat_amd.train import FlatAdam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--launches', type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_optim: needs a HIP device (the optimiser has no CPU fallback)')
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel').to(dev)
    opt = FlatAdam(model.parameters(), lr=1e-3, weight_decay=0.01, max_grad_norm=3.0, ema_decay=0.999, data_parallel=False)
    n = opt.n
    opt.flat_grad.normal_(generator=torch.Generator(device=dev).manual_seed(1))
    word = ptr(ops.step_error_word(dev))
    head = (ptr(opt.flat_param), ptr(opt.flat_grad), ptr(opt.exp_avg), ptr(opt.exp_avg_sq), n, ptr(opt.step_count), opt.lr,
            opt.step_size, opt.gamma, opt.betas[0], opt.betas[1], opt.eps, 1.0, word)
    runs = {
        'adam': (7, lambda: call('rv_adam_step', *head, stream())),
        'adamw': (9, lambda: call('rv_adamw_step', *head, opt.weight_decay, opt.max_grad_norm, ptr(opt.norm_buf), ptr(opt.flat_ema),
                                  opt.ema_decay, stream())),
        'norm': (1, lambda: call('rv_reduce_mean', 3, ptr(opt.flat_grad), None, n, ptr(opt.norm_buf), ptr(opt.norm_ws), None, stream())),
    }
    runs['norm'][1]()                                                  # the clip coefficient reads a real norm
    for _, fn in runs.values():                                        # warm-up: code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(a.rounds):
        for name, (_, fn) in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                fn()
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    assert bool(torch.isfinite(opt.flat_param).all()) and bool(torch.isfinite(opt.flat_ema).all())
    print(f'UNet_Onset flat bucket: n = {n} floats ({4 * n / 1e6:.1f} MB per stream); {a.rounds} rounds x {a.launches} launches, alternating')
    print(f"{'':8}{'streams':>8}{'median us':>12}{'min..max us':>20}{'GB/s':>10}")
    med = {}
    for name, (streams, _) in runs.items():
        med[name] = statistics.median(us[name])
        print(f'{name:8}{streams:8d}{med[name]:12.2f}{min(us[name]):10.2f}..{max(us[name]):<8.2f}{streams * 4 * n / med[name] / 1e3:10.0f}')
    print(f"adamw / adam = {med['adamw'] / med['adam']:.3f} (bytes alone: 9 / 7 = 1.286); with the norm launch "
          f"{(med['adamw'] + med['norm']) / med['adam']:.3f}")
    print(json.dumps({'n': n, 'rounds': a.rounds, 'launches': a.launches, 'median_us': med,
                      'min_max_us': {k: [min(v), max(v)] for k, v in us.items()}}))


if __name__ == '__main__':
    main()
