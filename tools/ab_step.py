"""What a batch becomes in a training step, as bits and launches, for one checkout: the A/B record of a refactoring of the Python
layer (model.py / onset_frames.py / vat.py / train.py) that must change neither.

    python tools/ab_step.py --out a.json [--package-root DIR] [--deterministic]
    python tools/ab_step.py --compare parent.json branch.json          # CPU only; prints the launch counts per configuration

For every configuration at the fixture shape of the goldens (B = 2, T = 64, oracle.fixture parameters, batches and injected
noise) it records the raw bits of every loss, SHA-256 of every prediction, of every BatchNorm running statistic and
`num_batches_tracked` and -- with --deterministic (ops.DETERMINISTIC: no fp32 atomics in the parameter gradients) -- of every
`param.grad`, and the ordered list of library entry points with the stream each was launched on and a hash of its arguments -- every
non-pointer value, and which pointers are NULL -- (through `_lib.HOOK`).
`--package-root` names the directory that holds the `reconvat_amd` package to import (default: this checkout), e.g. the parent
exported by `git archive <parent> | tar -x -C <dir>` (or a `git worktree`) with this checkout's `libreconvat_hip.so` copied next to
its sources, so that both runs load the same library.  Results: profiles/step_plan_ab.txt, profiles/conv_backward_ab.txt.
"""
import argparse
import hashlib
import itertools
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DS = ((2, 2), (2, 2))


def compare(a_path, b_path):
    with open(a_path) as fh:
        a = json.load(fh)
    with open(b_path) as fh:
        b = json.load(fh)
    bad = sorted(set(a) ^ set(b))
    for name in sorted(set(a) & set(b)):
        diff = [k for k in sorted(set(a[name]) | set(b[name])) if a[name].get(k) != b[name].get(k)]
        bad += [f'{name}: {k}' for k in diff]
        print(f"{name:58s} launches {len(a[name]['launches']):5d} {len(b[name]['launches']):5d}  {'DIFFERS: ' + ', '.join(diff) if diff else 'identical'}")
    print(f'{len(a)} / {len(b)} configurations; ' + ('ALL IDENTICAL' if not bad else f'{len(bad)} DIFFERENCES: {bad}'))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--package-root', default=ROOT)
    ap.add_argument('--deterministic', action='store_true')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    sys.path.insert(0, ROOT)                              # oracle.fixture
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    import reconvat_amd as ra
    from oracle import fixture as fx, onset_frames as oo
    from reconvat_amd import _lib, ops
    assert os.path.dirname(os.path.dirname(os.path.abspath(ra.__file__))) == os.path.abspath(args.package_root)
    ops.DETERMINISTIC[0] = args.deterministic
    dev = torch.device('cuda:0')
    sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    bits = lambda v: struct.pack('<f', float(v.detach())).hex()
    launches = []

    def hook(name, a, fn):
        # the arguments as far as they repeat from run to run: every non-pointer value (pointers vary with allocation: only whether one is NULL)
        types = _lib.SIGNATURES[name][1]
        assert len(a) == len(types), name
        what = repr([(v is not None and v != 0) if t is _lib.P else v for v, t in zip(a, types)])
        launches.append((name, torch.cuda.current_stream().cuda_stream, hashlib.sha256(what.encode()).hexdigest()[:16]))
        return fn(*a)

    def batch(tag, T=64):
        onset, frame = fx.fixture_labels(2, T, tag)
        return {'audio': fx.fixture_audio(2, T * 512, tag).to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev)}

    def inject(m, shape, tags):
        """Noise in call order: the tags cycle (unlabelled first where there is an unlabelled batch)."""
        if m.vat_loss is not None:
            d = itertools.cycle([fx.fixture_noise(shape, t).to(dev) for t in tags])
            m.vat_loss.noise = lambda t: next(d).clone()

    def unet(kind, recon, training):
        m = (ra.UNet_Onset if kind == 'onset' else ra.UNet)(*DS, log=True, reconstruction=recon, mode='imagewise', spec='Mel', XI=1e-6, eps=2.0)
        m.load_state_dict(fx.fixture_params(kind, recon))
        return m.to(dev).train(training)

    def onf(cls, kind, training, **kw):
        m = cls(229, 88, model_complexity=48, log=True, mode='imagewise', spec='Mel', **kw)
        m.load_state_dict(oo.fixture_params(kind=kind) if kind else oo.fixture_params())
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        return m.to(dev).train(training)

    def record(m, losses, preds, grads):
        main = torch.cuda.current_stream().cuda_stream
        sides = {ops.side_stream(dev, i).cuda_stream: f'side{i}' for i in range(2)}
        rec = {'losses': {k: bits(v) for k, v in losses.items()},
               'predictions': {k: None if v is None else sha(v) for k, v in preds.items()},
               'bn': {k: sha(v) for k, v in m.state_dict().items() if k.endswith(('running_mean', 'running_var', 'num_batches_tracked'))},
               'launches': [[n, 'main' if s == main else sides.get(s, 'other'), h] for n, s, h in launches]}
        if args.deterministic:
            rec['grads'] = grads
        return rec

    def one_call(m, fn, *a):
        """One run_on_batch-like call (+ backward of the plain sum in training mode) with the launches recorded."""
        del launches[:]
        _lib.HOOK[0] = hook
        try:
            preds, losses, _ = fn(*a)
            if m.training:
                sum(losses.values()).backward()
            torch.cuda.synchronize()
        finally:
            _lib.HOOK[0] = None
        return record(m, losses, preds, {k: sha(p.grad) for k, p in m.named_parameters() if p.grad is not None})

    def train_step(m, bl, bul, graph, dual):
        """One TrainStep forward + backward as tests/test_model_gpu.py::test_train_step_two_streams_equals_single_stream runs it."""
        opt = ra.FlatAdam(m.parameters(), lr=1e-3)
        del launches[:]
        _lib.HOOK[0] = hook
        try:
            step = ra.TrainStep(m, opt, bl, bul, VAT=True, graph=graph, dual_stream=dual)
            if graph:
                step.capture()
                step.graph.replay()
            else:
                step._fwd_bwd()
                step._dual_ready = True
                step._fwd_bwd()
            torch.cuda.synchronize()
        finally:
            _lib.HOOK[0] = None
        return record(m, step.losses, {}, {'flat_grad': sha(opt.flat_grad)})

    out = {}
    bl, bul = batch('L'), batch('UL')
    unet_noise = ((2, 1, 64, 229), ('d0_ul', 'd0_l'))
    onf_noise = ((2, 64, 229), ('onf_d0_ul', 'onf_d0_l'))
    for kind, recon, vat, training in itertools.product(('onset', 'frame'), (False, True), (False, True), (True, False)):
        for ul in (False, True) if training else (False,):
            m = unet(kind, recon, training)
            inject(m, unet_noise[0], unet_noise[1] if ul else unet_noise[1][1:])
            out[f'{kind} recon={int(recon)} VAT={int(vat)} train={int(training)} ul={int(ul)}'] = one_call(m, m.run_on_batch, bl, bul if ul else None, vat)
    for training in (True, False):
        m = unet('frame', True, training)
        inject(m, *unet_noise)
        out[f'application train={int(training)}'] = one_call(m, m.run_on_batch_application, bl, bul, True)
    for vat, training in itertools.product((False, True), (True, False)):
        for ul in (False, True) if training else (False,):
            m = onf(ra.OnsetsAndFrames_VAT_full, None, training, XI=1e-6, eps=1e-1)
            inject(m, onf_noise[0], onf_noise[1] if ul else onf_noise[1][1:])
            out[f'onf VAT={int(vat)} train={int(training)} ul={int(ul)}'] = one_call(m, m.run_on_batch, bl, bul if ul else None, vat)
    for vat in (False, True):
        m = onf(ra.Frame_stack_VAT, 'frame', True, XI=1e-1, eps=2.0, VAT_mode='all')
        inject(m, onf_noise[0], ('onf_fs_d0',))
        out[f'frame_stack VAT={int(vat)}'] = one_call(m, m.run_on_batch, bl, None, vat)
    m = onf(ra.Onset_stack_VAT, 'onset', True)
    out['onset_stack'] = one_call(m, m.run_on_batch, bl, None, False)
    for name in ('onset', 'frame', 'onf'):            # the two- / three-chain schedule of one run_on_batch + backward, outside TrainStep
        m = onf(ra.OnsetsAndFrames_VAT_full, None, True, XI=1e-6, eps=1e-1) if name == 'onf' else unet(name, True, True)
        inject(m, *(onf_noise if name == 'onf' else unet_noise))
        ops.DUAL_STREAM[0] = True
        try:
            out[f'{name} recon=1 VAT=1 train=1 ul=1 dual=1'] = one_call(m, m.run_on_batch, bl, bul, True)
        finally:
            ops.DUAL_STREAM[0] = False
    for name, graph, dual in itertools.product(('onset', 'frame', 'onf'), (False, True), (False, True)):
        m = onf(ra.OnsetsAndFrames_VAT_full, None, True, XI=1e-6, eps=1e-1) if name == 'onf' else unet(name, True, True)
        inject(m, *(onf_noise if name == 'onf' else unet_noise))
        out[f'TrainStep {name} graph={int(graph)} dual={int(dual)}'] = train_step(m, bl, bul, graph, dual)
    with open(args.out, 'w') as fh:
        json.dump(out, fh, indent=0, sort_keys=True)
    print(f'{len(out)} configurations -> {args.out}')


if __name__ == '__main__':
    main()
