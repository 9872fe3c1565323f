"""Generate tests/golden/thickstun_{c1,c1_step,c2,c2_grad}.npz by RUNNING THE REFERENCE's Thickstun class (model/Thickstun_model.py, imported unmodified
through ``_refload``) and its ``train_model`` loop:

    python tests/golden/make_golden_thickstun.py

Inputs and weights are closed-form (tests/thickstun_fixture.py), so no weight file is stored.  For every quantity the reference's
float32 result AND its float64 result are stored (``*_f32`` / ``*_f64``): the tests accept |hip - f32| <= 2 x |f32 - f64|.
* c1 (B = 2, 16 frames): frame prediction, loss, returned spec, all five parameter gradients; loss and parameters after two
  train_model steps (Adam 1e-4, StepLR 1000 / 0.98, clip 3) on the same batch;
* c2 (B = 1, 640 frames): prediction, loss, gradients.
The two large tensors (CNN_time.weight, linear.weight; gradients and stepped parameters) are stored as every 997th element of the
flattened tensor plus the L2 norm per output channel.  ``*_stats``: share of positive z2 / z3 pre-activations, share of them within
1e-5 of zero (fp64), min / max of the sigmoid outputs, and the share of z2 / z3 ReLU decisions on which the fp32 run disagrees with fp64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refload  # noqa: E402
import thickstun_fixture as tf  # noqa: E402

torch.set_num_threads(8)
ref = _refload.load_reference()
BIG = ('CNN_time.weight', 'linear.weight')


def build(dtype):
    net = ref.Thickstun()
    sd = net.state_dict()
    sd.update(tf.params())
    net.load_state_dict(sd, strict=True)
    net.train(True)
    return net.double() if dtype == torch.float64 else net


def cast(batch, dtype):
    return {k: v.to(dtype) if v.is_floating_point() else v for k, v in batch.items()}


def store(out, key, name, t):
    t = t.detach()
    if name in BIG:
        out[key + '_sample'] = t.flatten()[::tf.SAMPLE].numpy()
        out[key + '_norms'] = t.flatten(1).double().norm(dim=1).numpy()
    else:
        out[key] = t.numpy()


def run_case(case, out, steps):
    acts = {}
    for tag, dtype in (('f32', torch.float32), ('f64', torch.float64)):
        net = build(dtype)
        keep = {}
        hooks = [net.CNN_freq.register_forward_hook(lambda m, i, o: keep.__setitem__('z2', o.detach())),
                 net.CNN_time.register_forward_hook(lambda m, i, o: keep.__setitem__('z3', o.detach()))]
        b = cast(tf.batch(case), dtype)
        pred, losses, spec = net.run_on_batch(b)
        loss = sum(losses.values())
        loss.backward()
        for h in hooks:
            h.remove()
        acts[tag] = keep
        out[f'{case}_loss_keys'] = np.array(list(losses.keys()))
        out[f'{case}_frame_{tag}'] = pred['frame'].detach().numpy()
        out[f'{case}_loss_{tag}'] = np.float64(loss.item())
        if case == 'c1':
            out[f'{case}_spec_{tag}'] = spec.detach().numpy()
        for name, p in net.named_parameters():
            store(out, f'{case}_grad_{name}_{tag}', name, p.grad)
        print(case, tag, 'loss', loss.item(), 'pred range', pred['frame'].min().item(), pred['frame'].max().item(), flush=True)
        if tag == 'f64':
            z2, z3, p = keep['z2'], keep['z3'], pred['frame'].detach()
            out[f'{case}_stats'] = np.array([(z2 > 0).double().mean().item(), (z3 > 0).double().mean().item(),
                                             (z2.abs() < 1e-5).double().mean().item(), (z3.abs() < 1e-5).double().mean().item(),
                                             p.min().item(), p.max().item(),
                                             ((acts['f32']['z2'] > 0) != (z2 > 0)).double().mean().item(),
                                             ((acts['f32']['z3'] > 0) != (z3 > 0)).double().mean().item()])
            print(case, 'stats [z2>0, z3>0, |z2|<1e-5, |z3|<1e-5, pmin, pmax, flips z2, flips z3]', out[f'{case}_stats'], flush=True)
        del keep, hooks
        if steps:
            net = build(dtype)
            opt = torch.optim.Adam(net.parameters(), 1e-4)
            sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1000, gamma=0.98)

            class Loader(list):
                batch_size = tf.CASES[case][0]
                dataset = [0] * (steps * tf.CASES[case][0])
            _, losses, _ = ref.train_model(net, 1, Loader([b] * steps), opt, sched, 3)
            out[f'{case}_step_loss_{tag}'] = np.float64(sum(losses.values()).item())
            for name, p in net.named_parameters():
                store(out, f'{case}_step_{name}_{tag}', name, p)


def main():
    out = {}
    sd = ref.Thickstun().state_dict()
    out['sd_keys'] = np.array(list(sd.keys()))
    out['sd_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    out['n_params'] = np.int64(sum(p.numel() for p in ref.Thickstun().parameters()))
    run_case('c1', out, steps=2)
    if '--short' not in sys.argv:
        run_case('c2', out, steps=0)
    # four files, each below the 1 MiB limit for a committed file (tests/thickstun_fixture.py::golden merges them)
    part = lambda k: ('c1_step' if k.startswith('c1_step_') else 'c2_grad' if k.startswith('c2_grad_') else 'c2' if k.startswith('c2_') else 'c1')
    for name in ('c1', 'c1_step', 'c2', 'c2_grad'):
        sel = {k: v for k, v in out.items() if part(k) == name}
        if sel:
            path = os.path.join(HERE, f'thickstun_{name}.npz')
            np.savez_compressed(path, **sel)
            print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
