"""The velocity kernels (rv_velocity_roll, rv_velocity_loss_grad; profiles/velocity_head.txt keeps the output) next to the
same definition composed from torch-eager ops (velocity.roll_torch / loss_torch with autograd) on the same device:

    roll        one ten-minute spectrogram, [1, 18750, 229] (the head on a rendered track's log-mel)
    loss+grad   a corpus batch, B = 8, T = 640 (8 x 327680 samples from the device feed of rendered tracks)

Times are HIP-event times around one call (the kernels' launches, or the eager chain with its backward), warm, the median of REPS
calls, each window holding INNER calls.  Before any time is printed the two are compared: the roll within 2^-18 per cell, loss and
gradient within 2^-18 of the gradient's largest entry (float32 against float32 in another order; the derived bounds against float64
are tests/test_velocity_gpu.py's).  These launches are short: the figures are call times, no share of any peak is claimed."""
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import reconvat_amd as ra
from reconvat_amd import ops, synth, velocity
from reconvat_amd.dataset import RenderedScores
from reconvat_amd.feed import DeviceCorpus

REPS, INNER = 21, 20

if not torch.cuda.is_available():
    raise SystemExit('bench_velocity.py measures on the GPU; there is none')
dev = torch.device('cuda:0')
torch.cuda.set_device(dev)


def timed(fn):
    """Median over REPS windows of the HIP-event time of INNER calls, per call, in microseconds (after a warm-up window)."""
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


model = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=False, mode='imagewise', spec='Mel').to(dev).eval()
head = velocity.VelocityHead.for_model(model, seed=0).to(dev)
table, params = head.table, head.packed().detach()
result = {}

# ---- the roll of one ten-minute track
notes = synth.random_score(np.random.RandomState(1), 600.0)
audio = synth.render(notes, 600 * 16000, synth.Timbre('struck', 1), device=dev, out_dtype=torch.float32)
spec = velocity.front_end(model, audio)
got, want = ops.velocity_roll(spec, table, params), velocity.roll_torch(spec, table, params)
err = float((got - want).abs().max())
assert got.shape == want.shape == (1, spec.shape[1], 88) and err <= 2.0 ** -18, err
k = timed(lambda: ops.velocity_roll(spec, table, params))
e = timed(lambda: velocity.roll_torch(spec, table, params))
result['roll'] = {'shape': list(spec.shape), 'max_abs_diff': err, 'kernel_us': k[0], 'kernel_us_min_max': k[1:], 'eager_us': e[0],
                  'eager_us_min_max': e[1:], 'eager_over_kernel': e[0] / k[0]}

# ---- loss and gradient of a corpus batch
tracks = RenderedScores(16, 2 * 327680 + 8192, ('struck', 'sustained'), seed=1000, device=dev).data
batch = next(iter(DeviceCorpus(tracks, 327680, 8, dev, seed=42)))
spec = velocity.front_end(model, batch['audio'])
target, mask = batch['velocity'].reshape(8, -1, 88), batch['onset'].reshape(8, -1, 88)


def eager():
    p = params.clone().requires_grad_(True)
    loss = velocity.loss_torch(spec, table, p, target, mask)
    loss.backward()
    return loss.detach(), p.grad


loss_k, grad_k = ops.velocity_loss_grad(spec, table, params, target, mask)
loss_e, grad_e = eager()
scale = float(grad_e.abs().max())
err_l, err_g = abs(float(loss_k) - float(loss_e)), float((grad_k - grad_e).abs().max())
assert int(mask.sum()) > 0 and scale > 0 and err_l <= 2.0 ** -18 * max(float(loss_e), 1.0) and err_g <= 2.0 ** -18 * scale, (err_l, err_g, scale)
k = timed(lambda: ops.velocity_loss_grad(spec, table, params, target, mask))
e = timed(eager)
result['loss_grad'] = {'shape': list(spec.shape), 'onset_cells': int(mask.sum()), 'loss': float(loss_k), 'loss_abs_diff': err_l,
                       'grad_max_abs_diff': err_g, 'grad_max_abs': scale, 'kernel_us': k[0], 'kernel_us_min_max': k[1:], 'eager_us': e[0],
                       'eager_us_min_max': e[1:], 'eager_over_kernel': e[0] / k[0]}
for name, r in result.items():
    print(f"{name:10s} {str(r['shape']):18s} kernel {r['kernel_us']:9.1f} us   torch eager {r['eager_us']:9.1f} us   ratio {r['eager_over_kernel']:.1f}")
print(json.dumps(result))
