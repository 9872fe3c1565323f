"""Time the Thickstun baseline at the training script's shape (B = 1, T = 640); prints ONE JSON line.

* per stage: HIP events around every single call, median / min / max of `--reps` (>= 20) calls after `--warmup` (>= 5), the GFLOP of
  the stage and the achieved TFLOP/s and share of the f32 MFMA peak (157.3 TFLOP/s);
* the time convolution's forward GEMM twice in the same process: the dedicated kernel (rv_thick_tconv_fwd, A operand stationary in LDS,
  bias + ReLU fused) and the generic rv_gemm on the same Hankel problem (sam = 128, sak = 1, batch = 51, bsa = (T+24)*128; bias fused, no
  ReLU).  Its input- and weight-gradient GEMMs run on rv_gemm in the product, so their times ARE the generic kernel's;
* the whole optimiser step (hipGraph TrainStep on FlatAdam), audio seconds per second, and the peak device memory of a training step
  and of a 2 000-frame evaluation.

    python tools/bench_thickstun.py [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

PEAK_F32_TFLOPS = 157.3
B, T, N, C, ROWS, TAPS = 1, 640, 4096, 128, 51, 25


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4), 'max_ms': round(max(ms), 4)}


def with_rate(r, gflop):
    r['gflop'] = round(gflop, 1)
    r['tflops'] = round(gflop / r['median_ms'], 1)
    r['frac_f32_mfma_peak'] = round(gflop / r['median_ms'] / PEAK_F32_TFLOPS, 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    reps, warmup = max(20, args.reps), max(5, args.warmup)
    assert torch.cuda.is_available(), 'tools/bench_thickstun.py needs an MI355X'
    import reconvat_amd as ra
    from reconvat_amd import ops
    from reconvat_amd._lib import call, ptr, stream
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = ra.Thickstun().to(dev)
    tp = T + TAPS - 1
    gen = torch.Generator().manual_seed(3)
    x = torch.rand(B, T, 229, generator=gen).to(dev)
    wf, bf, wt, bt, wl = (p.detach() for p in model.parameters())
    out = {'shape': f'B={B} T={T}', 'reps': reps, 'warmup': warmup, 'peak_f32_tflops': PEAK_F32_TFLOPS}

    z2 = ops.ThickFreqFn.apply(x, wf, bf, 12)
    out['freq_fwd'] = with_rate(timed(lambda: ops.ThickFreqFn.apply(x, wf, bf, 12), reps, warmup), 2 * ROWS * tp * C * 128 * B / 1e9)
    wj = ops.thick_wj(wt)
    z3 = torch.empty((B, T, ROWS, N), device=dev)
    g_tconv = 2.0 * B * ROWS * T * N * TAPS * C / 1e9
    out['tconv_fwd_dedicated'] = with_rate(timed(lambda: call('rv_thick_tconv_fwd', ptr(z2), ptr(wj), ptr(bt), ptr(z3), B, T, N, stream()),
                                                 reps, warmup), g_tconv)
    # the same Hankel problem on the generic kernel: A rows overlap by 3072 floats, W flattened as [n][j*128 + c]
    wflat = wt[:, :, 0, :].permute(0, 2, 1).reshape(N, TAPS * C).contiguous()
    hankel = z2.as_strided((T, TAPS * C), (C, 1))
    c_view = z3.as_strided((T, N), (ROWS * N, 1))
    out['tconv_fwd_rv_gemm'] = with_rate(timed(lambda: ops.gemm(hankel, wflat.t(), c_view, bt, 0, splitk=1, batch=ROWS,
                                                                bstrides=(tp * C, 0, N)), reps, warmup), g_tconv)
    call('rv_thick_tconv_fwd', ptr(z2), ptr(wj), ptr(bt), ptr(z3), B, T, N, stream())
    dz3 = torch.rand(z3.shape, generator=gen).to(dev) * (z3 > 0)
    out['tconv_dgrad_rv_gemm'] = with_rate(timed(lambda: ops.thick_tconv_dgrad(dz3, wj, B, T), reps, warmup), g_tconv)
    out['tconv_wgrad_rv_gemm'] = with_rate(timed(lambda: ops.thick_tconv_wgrad(dz3, z2), reps, warmup), g_tconv)
    g_lin = 2.0 * B * T * 88 * ROWS * N / 1e9
    wlt = ops.thick_wlt(wl, N)
    z3m = z3.view(B * T, ROWS * N)
    y = torch.empty((B * T, 88), device=dev)
    dy = torch.rand(B * T, 88, generator=gen).to(dev)
    dz = torch.empty_like(z3m)
    dwlt = torch.empty((ROWS * N, 88), device=dev)
    out['linear_fwd_rv_gemm'] = with_rate(timed(lambda: ops.gemm(z3m, wlt, y, None, 1, splitk=ops.THICK_LINEAR_SPLITK), reps, warmup), g_lin)
    out['linear_dz'] = with_rate(timed(lambda: call('rv_thick_linear_dz', ptr(dy), ptr(wlt), ptr(z3m), ptr(dz), B * T, ROWS * N, 88, stream()),
                                       reps, warmup), g_lin)
    out['linear_wgrad_rv_gemm'] = with_rate(timed(lambda: ops.gemm(z3m.t(), dy, dwlt, splitk=1), reps, warmup), g_lin)
    del z3, z3m, dz3, dz, dwlt, wflat
    torch.cuda.empty_cache()

    # the whole step
    opt = ra.FlatAdam(model.parameters(), lr=1e-4, step_size=1000, gamma=0.98)
    u = torch.rand(B, T, 88, generator=gen)
    batch = {'audio': (torch.rand(B, T * 512, generator=gen) * 0.2 - 0.1).to(dev), 'frame': (u > 0.95).float().to(dev),
             'onset': (u > 0.99).float().to(dev)}
    torch.cuda.reset_peak_memory_stats()
    step = ra.TrainStep(model, opt, batch, None, VAT=False, clip=3.0, graph=True)
    out['step'] = timed(step, reps, warmup)
    out['step']['audio_seconds_per_second'] = round(B * T * 512 / 16000 / (out['step']['median_ms'] / 1e3), 1)
    out['step']['loss'] = round(float(step.loss), 5)
    out['train_step_peak_memory_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    step.release()
    del step, opt
    torch.cuda.empty_cache()
    model.eval()
    torch.cuda.reset_peak_memory_stats()
    with torch.no_grad():
        song = torch.rand(1, 2000, 229, generator=gen).to(dev)
        out['eval_2000_frames'] = timed(lambda: model.frames(song), 3, 1)
    out['eval_2000_frames_peak_memory_mb'] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
