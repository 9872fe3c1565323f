"""Time the constant-Q front end (csrc/cqt.hip) and the spec='CQT' training step; prints ONE JSON line.

* front end: CQT1992v2.lognorm (log + imagewise min-max) on 16 full crops of 327 679 samples (640 frames x 176 bins), HIP events
  around `--reps` calls after a warm-up; its GFLOP at exact support and group-tiled (from the packed bank) and the share of the
  f32 MFMA peak (157.3 TFLOP/s) on the group-tiled count;
* step: UNet_Onset VAT + reconstruction at B_l = B_ul = 8, two-stream hipGraph TrainStep (bench.py's configuration), spec='CQT'
  next to spec='Mel', same build, same synthetic batch.

    python tools/bench_cqt.py [--reps 50] [--steps 10]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

PEAK_F32_TFLOPS = 157.3
SEG = 327680


def _events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def frontend(dev, reps):
    from reconvat_amd.frontend import CQT1992v2, cqt_gflop
    layer = CQT1992v2(sr=16000, hop_length=512, n_bins=176, fmin=27.5, bins_per_octave=24, trainable=False, verbose=False).to(dev)
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand(16, SEG, generator=gen) * 0.2 - 0.1).to(dev)[:, :-1]
    for _ in range(3):
        layer.lognorm(x)
    torch.cuda.synchronize()
    ms = _events(lambda: layer.lognorm(x), reps)
    exact, tiled = cqt_gflop(layer.tables(), 16, 640)
    return {'cqt_frontend_ms': round(ms, 4), 'cqt_gflop_exact': round(exact, 2), 'cqt_gflop_tiled': round(tiled, 2),
            'cqt_gflop_dense_reference': round(2 * 2 * 16 * 640 * 176 * 32768 / 1e9, 1),
            'cqt_tflops_tiled': round(tiled / ms, 1), 'cqt_frac_f32_mfma_peak': round(tiled / ms / PEAK_F32_TFLOPS, 3)}


def step_ms(spec, dev, steps):
    import reconvat_amd as ra
    torch.manual_seed(1234)
    model = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec=spec, XI=1e-6, eps=2).to(dev)
    opt = ra.FlatAdam(model.parameters(), lr=1e-3, step_size=1000, gamma=0.98)
    gen = torch.Generator().manual_seed(1000)

    def batch(b):
        u = torch.rand(b, SEG // 512, 88, generator=gen)
        return {'audio': (torch.rand(b, SEG, generator=gen) * 0.2 - 0.1).to(dev), 'frame': (u > 0.95).float().to(dev),
                'onset': (u > 0.99).float().to(dev)}
    bl, bul = batch(8), batch(8)
    torch.manual_seed(77)
    step = ra.TrainStep(model, opt, bl, bul, alpha=1.0, VAT=True, clip=3.0, graph=True, dual_stream=True)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    ms = _events(step, steps)
    step.check()
    loss = float(step.losses['loss/train_frame'])
    del step, opt, model
    torch.cuda.synchronize()
    return ms, loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--frontend-only', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/bench_cqt.py needs an MI355X'
    dev = torch.device('cuda:0')
    out = frontend(dev, args.reps)
    if not args.frontend_only:
        for spec in ('CQT', 'Mel'):
            ms, loss = step_ms(spec, dev, args.steps)
            out[f'step_ms_{spec.lower()}'] = round(ms, 3)
            out[f'step_loss_frame_{spec.lower()}'] = round(loss, 5)
        out['step_config'] = 'UNet_Onset VAT + reconstruction, B_l = B_ul = 8 x 327 680 samples, two-stream hipGraph TrainStep'
    print(json.dumps(out))


if __name__ == '__main__':
    main()
