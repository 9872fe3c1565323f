"""GPU tests of the Thickstun baseline (reconvat_amd/thickstun.py, csrc/thickstun.hip): each kernel alone against torch on the device,
run_on_batch / gradients / optimiser steps against the reference's own values (tests/golden/thickstun_*.npz,
make_golden_thickstun.py), graph replay, chunked evaluation and the training script.

Tolerance, for every quantity:  |hip - reference_fp32| <= 2 x |reference_fp32 - reference_fp64|, both sides the maximum over the
tensor, with a floor of 1e-6 x the tensor's largest magnitude where the reference's own spread is below fp32 resolution.  Every
measured error is appended to the parity log that tests/parity_tol.py writes (the table of DESIGN.md section 4 is made from it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thickstun_fixture as tf  # noqa: E402
from parity_tol import _OUT  # noqa: E402 -- the parity log of the other GPU tests

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = ('CNN_time.weight', 'linear.weight')


def check(where, got, f32, f64):
    got, f32, f64 = (np.asarray(a, dtype=np.float64) for a in (got, f32, f64))
    assert got.shape == f32.shape == f64.shape, (where, got.shape, f32.shape, f64.shape)
    err = float(np.abs(got - f32).max())
    spread = float(np.abs(f32 - f64).max())
    tol = max(2.0 * spread, 1e-6 * float(np.abs(f32).max()))
    print(f'[parity] {where}: err {err:.3e} tol {tol:.3e} (reference f32-f64 spread {spread:.3e}, max |ref| {np.abs(f32).max():.3e})')
    try:
        os.makedirs(os.path.dirname(_OUT), exist_ok=True)
        with open(_OUT, 'a') as fh:
            fh.write(json.dumps({'where': where, 'abs_err': err, 'tol': tol, 'ref_spread': spread, 'ref_max': float(np.abs(f32).max())}) + '\n')
    except OSError:
        pass
    assert err <= tol, (where, err, tol)


def check_t(where, got, ref32, ref64):
    check(where, got.detach().cpu().numpy(), ref32.detach().cpu().numpy(), ref64.detach().cpu().numpy())


def model(dev, training=True):
    import reconvat_amd as ra
    m = ra.Thickstun()
    missing, unexpected = m.load_state_dict(tf.params(), strict=False)
    assert not unexpected and all(k.startswith('spectrogram.') for k in missing)
    return m.to(dev).train(training)


def to_dev(batch, dev):
    return {k: v.to(dev) for k, v in batch.items()}


def sampled(name, t):
    """What the golden stores of a tensor: everything, or (every 997th element, per-output-channel L2 norms) of the two large ones."""
    t = t.detach()
    if name in BIG:
        return {'_sample': t.flatten()[::tf.SAMPLE].cpu().numpy(), '_norms': t.flatten(1).double().norm(dim=1).cpu().numpy()}
    return {'': t.cpu().numpy()}


def rand(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * 2 - 1).to(dev)


SIZES = [(1, 1), (3, 37), (2, 130)]          # (clips, frames): one frame, odd sizes, more than one 128-frame tile


@pytest.mark.parametrize('bb,t', SIZES)
def test_freq_kernels(dev, bb, t):
    """rv_thick_freq_fwd / rv_thick_freq_bwd against conv2d and its autograd on the device, the padded frames included."""
    from reconvat_amd.ops import ThickFreqFn
    x = rand((bb, t, 229), dev, 1).abs()
    w = (rand((128, 1, 128, 1), dev, 2) * 0.3).requires_grad_(True)
    b = (rand((128,), dev, 3) * 0.3).requires_grad_(True)
    z2 = ThickFreqFn.apply(x, w, b, 12)
    assert z2.shape == (bb, 51, t + 24, 128)
    dz2 = rand(z2.shape, dev, 4)
    z2.backward(dz2)
    refs = []
    for dt in (torch.float32, torch.float64):
        wr, br = w.detach().to(dt).requires_grad_(True), b.detach().to(dt).requires_grad_(True)
        img = F.pad(x.to(dt).transpose(1, 2), (12, 12)).unsqueeze(1)                       # [B, 1, 229, T+24]
        r = torch.relu(F.conv2d(img, wr, br, stride=(2, 1)))                                # [B, 128, 51, T+24]
        r.backward(dz2.to(dt).permute(0, 3, 1, 2))
        refs.append((r.permute(0, 2, 3, 1), wr.grad, br.grad))
    check_t(f'freq_fwd B{bb} T{t}', z2, refs[0][0], refs[1][0])
    edge = torch.relu(b.detach()).expand(bb, 51, 12, 128)
    assert torch.equal(z2[:, :, :12], edge) and torch.equal(z2[:, :, t + 12:], edge)
    check_t(f'freq_wgrad B{bb} T{t}', w.grad, refs[0][1], refs[1][1])
    check_t(f'freq_bgrad B{bb} T{t}', b.grad, refs[0][2], refs[1][2])


@pytest.mark.parametrize('bb,t', SIZES)
def test_tconv_kernels(dev, bb, t):
    """rv_thick_tconv_fwd and the rv_gemm-based input / weight / bias gradients against conv2d and its autograd (N = 256 channels)."""
    from reconvat_amd.ops import ThickTconvFn
    n = 256
    z2 = rand((bb, 51, t + 24, 128), dev, 5).requires_grad_(True)
    w = (rand((n, 128, 1, 25), dev, 6) * 0.03).requires_grad_(True)
    b = (rand((n,), dev, 7) * 0.1).requires_grad_(True)
    z3 = ThickTconvFn.apply(z2, w, b)
    assert z3.shape == (bb, t, 51, n)
    dz3 = rand(z3.shape, dev, 8) * (z3.detach() > 0)          # the function's contract: the incoming gradient carries z3's ReLU mask
    z3.backward(dz3)
    refs = []
    for dt in (torch.float32, torch.float64):
        zr, wr, br = (v.detach().to(dt).requires_grad_(True) for v in (z2, w, b))
        pre = F.conv2d(zr.permute(0, 3, 1, 2), wr, br)                                      # [B, N, 51, T]
        pre.backward(dz3.to(dt).permute(0, 3, 2, 1))
        refs.append((torch.relu(pre).permute(0, 3, 2, 1), zr.grad, wr.grad, br.grad))
    check_t(f'tconv_fwd B{bb} T{t}', z3, refs[0][0], refs[1][0])
    check_t(f'tconv_dgrad B{bb} T{t}', z2.grad, refs[0][1], refs[1][1])
    check_t(f'tconv_wgrad B{bb} T{t}', w.grad, refs[0][2], refs[1][2])
    check_t(f'tconv_bgrad B{bb} T{t}', b.grad, refs[0][3], refs[1][3])


@pytest.mark.parametrize('m', [1, 37, 130])
def test_linear_kernels(dev, m):
    """The linear stage (rv_gemm forward with fused sigmoid, rv_thick_linear_dz with z3's ReLU mask, rv_gemm weight gradient, the
    c*51+f <-> f*C+c re-indexing both ways) against torch, C = 128 channels."""
    from reconvat_amd.ops import ThickLinearFn
    c = 128
    z3 = torch.relu(rand((m, 51, c), dev, 9)).requires_grad_(True)                          # z3's layout: [M, f, c]
    w = (rand((88, c * 51), dev, 10) * 0.05).requires_grad_(True)                            # checkpoint layout: feature c*51 + f
    p = ThickLinearFn.apply(z3.view(m, 51 * c), w, c)
    dp = rand(p.shape, dev, 11)
    p.backward(dp)
    refs = []
    for dt in (torch.float32, torch.float64):
        zr, wr = z3.detach().to(dt).requires_grad_(True), w.detach().to(dt).requires_grad_(True)
        pr = torch.sigmoid(torch.relu(zr).permute(0, 2, 1).reshape(m, c * 51) @ wr.t())
        pr.backward(dp.to(dt))
        refs.append((pr, zr.grad * (zr.detach() > 0), wr.grad))
    check_t(f'linear_fwd M{m}', p, refs[0][0], refs[1][0])
    check_t(f'linear_dz M{m}', z3.grad, refs[0][1], refs[1][1])
    check_t(f'linear_wgrad M{m}', w.grad, refs[0][2], refs[1][2])


def test_tconv_wgrad_reproducible(dev):
    """The weight gradient of the time convolution adds its partial products in stream order, no float atomics: identical bits twice."""
    from reconvat_amd import ops
    z2, dz3 = rand((2, 51, 40 + 24, 128), dev, 12), rand((2, 40, 51, 256), dev, 13)
    a, b = ops.thick_tconv_wgrad(dz3, z2), ops.thick_tconv_wgrad(dz3, z2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _forward_backward(case, dev):
    g = tf.golden()
    m = model(dev)
    pred, losses, spec = m.run_on_batch(to_dev(tf.batch(case), dev))
    assert list(losses) == [str(k) for k in g[case + '_loss_keys']] == ['loss/train_frame']
    assert pred['onset'] is pred['frame'] and pred['r_adv'] is None
    b, t = tf.CASES[case]
    assert pred['frame'].shape == (b * t, 88) and spec.shape == (b, 229, t)
    sum(losses.values()).backward()
    check(f'{case} frame', pred['frame'].detach().cpu().numpy(), g[f'{case}_frame_f32'], g[f'{case}_frame_f64'])
    check(f'{case} loss', losses['loss/train_frame'].item(), g[f'{case}_loss_f32'], g[f'{case}_loss_f64'])
    if case == 'c1':
        check(f'{case} spec', spec.cpu().numpy(), g[f'{case}_spec_f32'], g[f'{case}_spec_f64'])
    for name, p in m.named_parameters():
        for suffix, got in sampled(name, p.grad).items():
            key = f'{case}_grad_{name}'
            check(f'{case} grad {name}{suffix}', got, g[f'{key}_f32{suffix}'], g[f'{key}_f64{suffix}'])


def test_run_on_batch_golden_short(dev):
    """Case 1 (B = 2, 16 frames): prediction, loss, spec and all five parameter gradients against the reference."""
    _forward_backward('c1', dev)


def test_run_on_batch_golden_full(dev):
    """Case 2 (B = 1, the full 640-frame segment of the training script): prediction, loss and gradients against the reference."""
    _forward_backward('c2', dev)


def test_two_steps_golden(dev):
    """Two train_model steps (Adam 1e-4, StepLR 1000 / 0.98, clip 3) on case 1: last loss and the parameters against the reference."""
    from reconvat_amd import train_model
    g = tf.golden()
    m = model(dev)
    opt = torch.optim.Adam(m.parameters(), 1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1000, gamma=0.98)

    class Loader(list):
        batch_size = 2
        dataset = [0] * 4
    _, losses, _ = train_model(m, 1, Loader([to_dev(tf.batch('c1'), dev)] * 2), opt, sched, 3)
    check('c1 step loss', sum(losses.values()).item(), g['c1_step_loss_f32'], g['c1_step_loss_f64'])
    for name, p in m.named_parameters():
        for suffix, got in sampled(name, p).items():
            key = f'c1_step_{name}'
            check(f'c1 step {name}{suffix}', got, g[f'{key}_f32{suffix}'], g[f'{key}_f64{suffix}'])


def test_graph_replay_equals_eager(dev):
    """TrainStep on FlatAdam: two captured-and-replayed steps give the bits of two eager steps."""
    from reconvat_amd import FlatAdam, TrainStep
    res = []
    for graph in (False, True):
        m = model(dev)
        opt = FlatAdam(m.parameters(), lr=1e-4, step_size=1000, gamma=0.98)
        step = TrainStep(m, opt, to_dev(tf.batch('c1'), dev), None, VAT=False, clip=3, graph=graph)
        losses = [float(step()), float(step())]
        res.append((losses, opt.flat_param.clone()))
        step.release()
    assert res[0][0] == res[1][0], (res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])


def test_chunked_evaluation(dev, tmp_path):
    """eval() under no_grad processes time in chunks with a 12-frame halo: bit-identical to the unchunked pass on 2 000 frames (B = 1,
    chunk boundaries at 512, 1024, 1536), with the peak memory bounded by the chunk; evaluate_wo_velocity runs on such a song."""
    from oracle import fixture as fx
    from reconvat_amd import thickstun
    from reconvat_amd.evaluate import evaluate_wo_velocity
    m = model(dev, training=False)
    t = 2000
    spec = rand((1, t, 229), dev, 14).abs()
    with torch.no_grad():
        assert t > thickstun.EVAL_CHUNK
        chunked = m.frames(spec)
        whole = m._layers(spec, thickstun.PAD)
        assert chunked.shape == whole.shape == (t, 88)
        assert torch.equal(chunked, whole)
        onset, frame = fx.fixture_labels(1, t, 'thick_song')
        song = {'audio': fx.fixture_audio(1, t * 512, 'thick_song').to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev),
                'path': 'song.flac'}
        metrics = evaluate_wo_velocity([song], m, reconstruction=False)
    assert len(metrics['metric/frame/f1']) == 1 and np.isfinite(metrics['loss/train_frame'][0])


def test_window_forward(dev):
    """forward(x) keeps the reference signature ([N, 229, 25] windows -> [N, 88]) and equals run_on_batch's frames on the same windows."""
    m = model(dev, training=False)
    spec = rand((1, 20, 229), dev, 15).abs()
    with torch.no_grad():
        frames = m.frames(spec)
        windows = F.pad(spec.transpose(1, 2), (12, 12)).unfold(2, 25, 1).transpose(1, 2).reshape(-1, 229, 25)
        out = m(windows)
    assert out.shape == (20, 88)
    assert torch.equal(out, frames)


def test_training_script(tmp_path):
    """train_baseline_Thickstun.py as a fresh process on the synthetic corpus: trains two epochs, saves, evaluates whole songs; the
    checkpoint has the reference's keys and loads into a new Thickstun with strict=True."""
    import reconvat_amd as ra
    logdir = str(tmp_path / 'run')
    args = ['train_on=Synthetic', 'epoches=2', f'logdir={logdir}']
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_baseline_Thickstun.py'), 'with', *args], capture_output=True,
                       text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout
    assert os.path.exists(os.path.join(logdir, 'result_dict'))
    sd = torch.load(os.path.join(logdir, 'model-final.pt'), map_location='cpu')
    assert list(sd) == [str(k) for k in tf.golden()['sd_keys']]
    ra.Thickstun().load_state_dict(sd, strict=True)
