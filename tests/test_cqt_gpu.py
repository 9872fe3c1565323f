"""GPU parity of the constant-Q front end (spec='CQT', csrc/cqt.hip) and of the CQT models against the reference's own values
(tests/golden/cqt_frontend.npz, cqt_models.npz; make_golden_cqt.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
DS = ((2, 2), (2, 2))
FLOOR = 2e-5          # the relative floor of the existing front-end / op tests (test_ops_gpu.TOL)


def gold(name):
    return np.load(os.path.join(G, name + '.npz'), allow_pickle=False)


def cqt_layer(dev):
    from reconvat_amd.frontend import CQT1992v2
    return CQT1992v2(sr=16000, hop_length=512, n_bins=176, fmin=27.5, bins_per_octave=24, trainable=False).to(dev)


def params176(kind, recon, monkeypatch):
    from oracle import fixture as fx
    monkeypatch.setattr(fx, 'N_BINS', 176)
    return fx.fixture_params(kind, recon, with_frontend=False)


def build(kind, recon, dev, monkeypatch, training=True):
    import reconvat_amd as ra
    cls = ra.UNet_Onset if kind == 'onset' else ra.UNet
    m = cls(*DS, log=True, reconstruction=recon, mode='imagewise', spec='CQT', XI=1e-6, eps=2.0)
    missing, unexpected = m.load_state_dict(params176(kind, recon, monkeypatch), strict=False)
    assert not unexpected and all(k.startswith('spectrogram.') for k in missing)
    return m.to(dev).train(training)


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_cqt_frontend_golden(dev):
    """Magnitude and log + imagewise normalisation against the reference in fp64: two short clips (one just above the reflect
    pad, both with a length that is not a multiple of 512, so both reflected ends matter), one full training crop at B = 1,
    the same three clips as ONE batch of rows (row stride 327 679), and a whole-song length."""
    from oracle import fixture as fx
    g = gold('cqt_frontend')
    layer = cqt_layer(dev)
    for name, n in (('short_a', 17385), ('short_b', 41234), ('full', 327679)):
        audio = fx.fixture_audio(1, n, 'cqt_' + name).to(dev)
        sel = g['full_frames'] if name == 'full' else slice(None)
        mag = layer(audio).transpose(1, 2)[0, sel].cpu().numpy()
        ln = layer.lognorm(audio)[0, 0, sel].cpu().numpy()
        assert mag.shape == g[name + '_mag_f64'].shape
        for what, got in (('mag', mag), ('lognorm', ln)):
            bound = max(FLOOR, 2.0 * float(g[f'{name}_{what}_dev']))
            err = rel(got, g[f'{name}_{what}_f64'])
            print(name, what, f'rel err {err:.2e} bound {bound:.2e}')
            assert err <= bound, (name, what, err, bound)
    # a batch: each row equals its B = 1 result bit for bit (rows are independent: same kernels, same order of sums)
    rows = torch.zeros(3, 327679)
    for i, (name, n) in enumerate((('short_a', 17385), ('short_b', 41234), ('full', 327679))):
        rows[i, :n] = fx.fixture_audio(1, n, 'cqt_' + name)[0]
    full = layer(rows.to(dev))
    one = layer(rows[2:3].to(dev))
    assert torch.equal(full[2:3], one)
    # whole song: 3 minutes, magnitude against a float64 conv1d of the layer's own buffers on four frames at both ends
    n = 16000 * 180 + 123
    song = fx.fixture_audio(1, n, 'cqt_song')
    mag = layer(song.to(dev)).cpu()
    assert mag.shape == (1, 176, 1 + n // 512)
    pad = torch.nn.functional.pad(song.double()[:, None], (16384, 16384), mode='reflect')
    kr, ki = layer.cqt_kernels_real.double().cpu(), layer.cqt_kernels_imag.double().cpu()
    sl = torch.sqrt(layer.lenghts.double().cpu())[:, None]
    for f0 in (0, mag.shape[-1] - 4):
        seg = pad[:, :, f0 * 512:(f0 + 3) * 512 + 32768]
        re = torch.nn.functional.conv1d(seg, kr, stride=512) * sl
        im = torch.nn.functional.conv1d(seg, ki, stride=512) * sl
        want = torch.sqrt(re ** 2 + im ** 2)
        assert rel(mag[:, :, f0:f0 + 4].numpy(), want.numpy()) <= 5 * FLOOR


def test_cqt_frontend_deterministic_and_refuses_short(dev):
    from oracle import fixture as fx
    layer = cqt_layer(dev)
    audio = fx.fixture_audio(4, 327679, 'cqt_det').to(dev)
    a, b = layer.lognorm(audio), layer.lognorm(audio)
    assert torch.equal(a, b)
    assert torch.equal(layer(audio), layer(audio))
    with pytest.raises(ValueError, match='longer than the reflect padding'):
        layer(torch.zeros(1, 16384, device=dev))
    layer(torch.zeros(1, 16385, device=dev))                      # one sample more is accepted


@pytest.mark.parametrize('kind', ['onset', 'frame'])
def test_cqt_run_on_batch_golden(dev, kind, monkeypatch):
    import parity_tol
    from oracle import fixture as fx
    from test_model_gpu import close_digest
    g = gold('cqt_models')

    def batch(tag):
        onset, frame = fx.fixture_labels(2, 64, tag)
        return {'audio': fx.fixture_audio(2, 64 * 512, tag).to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev)}
    bl, bul = batch('L'), batch('UL')
    n_ul, n_l = fx.fixture_noise((2, 1, 64, 176), 'd0_ul').to(dev), fx.fixture_noise((2, 1, 64, 176), 'd0_l').to(dev)
    for recon in (False, True):
        for vat in (False, True):
            key = f'{kind}_r{int(recon)}_v{int(vat)}_T64'
            m = build(kind, recon, dev, monkeypatch)
            seq = [n_ul, n_l] if vat else [n_l]
            m.vat_loss.noise = lambda t, seq=seq: seq.pop(0).clone()
            pred, losses, spec = m.run_on_batch(bl, bul if vat else None, vat)
            keys = [str(k) for k in g[key + '_keys']]
            assert list(losses.keys()) == keys, key
            sp = max([s for k, s in zip(keys, g[key + '_spread']) if parity_tol.is_vat_key(k)] or [0.0])
            for k, ref in zip(keys, g[key + '_f32_8t']):
                tol = max(1e-3, 2.0 * sp) if parity_tol.is_vat_key(k) else 1e-3
                err = abs(float(losses[k]) - float(ref)) / max(abs(float(ref)), 1e-6)
                assert err <= tol, (key, k, float(losses[k]), float(ref), err, tol)
            close_digest(pred['frame'], g[key + '_frame'], 1e-3, 256)
            if recon:
                close_digest(pred['reconstruction'], g[key + '_rec'], 1e-3, 256)
            assert spec.shape == (2, 64, 176)


def test_cqt_full_length_graph_step(dev, monkeypatch):
    """UNet_Onset, spec='CQT', VAT + reconstruction, B = 2 + 2 full crops: the two-stream TrainStep replayed from a captured
    graph gives the losses of the eager TrainStep, and both are within tolerance of the reference's full-length losses."""
    import reconvat_amd as ra
    from oracle import fixture as fx
    g = gold('cqt_models')
    key = 'onset_r1_v1_T640'

    def batch(tag):
        onset, frame = fx.fixture_labels(2, 640, tag)
        return {'audio': fx.fixture_audio(2, 640 * 512, tag).to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev)}
    bl, bul = batch('L'), batch('UL')
    noise = [fx.fixture_noise((2, 1, 640, 176), 'd0_ul').to(dev), fx.fixture_noise((2, 1, 640, 176), 'd0_l').to(dev)]
    keys = [str(k) for k in g[key + '_keys']]
    sp = max(s for k, s in zip(keys, g[key + '_spread']) if 'LDS' in k or 'r_norm' in k)
    results = {}
    for graph in (False, True):
        m = build('onset', True, dev, monkeypatch)
        opt = ra.FlatAdam(m.parameters(), lr=0.0)
        state = {'i': 0}

        def draw(t, state=state):
            state['i'] += 1
            return noise[(state['i'] - 1) % 2].clone()
        m.vat_loss.noise = draw
        step = ra.TrainStep(m, opt, bl, bul, alpha=1.0, VAT=True, clip=3.0, graph=graph, dual_stream=True)
        step()
        step()
        torch.cuda.synchronize()
        step.check()
        assert list(step.losses.keys()) == keys
        results[graph] = {k: float(v) for k, v in step.losses.items()}
        for k, ref in zip(keys, g[key + '_f32_8t']):
            vat = 'LDS' in k or 'r_norm' in k
            tol = max(1e-3, 2.0 * sp) if vat else 1e-3
            err = abs(results[graph][k] - float(ref)) / max(abs(float(ref)), 1e-6)
            assert err <= tol, (graph, k, results[graph][k], float(ref), err, tol)
    for k in keys:
        assert abs(results[True][k] - results[False][k]) <= 1e-5 * max(abs(results[False][k]), 1e-6), \
            (k, results[True][k], results[False][k])


def test_cqt_onset_script_checkpoint(dev, tmp_path):
    """train_UNet_Onset_VAT.py with spec=CQT as a fresh child process: a few iterations, a checkpoint with the CQT buffers
    that a fresh CQT model loads with strict=True."""
    import reconvat_amd as ra
    logdir = str(tmp_path / 'run')
    args = ['train_on=Synthetic', 'small=True', 'supersmall=True', 'sequence_length=32768', 'batch_size=2', 'train_batch_size=2',
            'iteration=2', 'spec=CQT', 'reconstruction=True', 'epoches=1', 'saving_freq=1', f'logdir={logdir}']
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_UNet_Onset_VAT.py'), 'with', *args], capture_output=True,
                       text=True, cwd=ROOT, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout
    sd = torch.load(os.path.join(logdir, 'model-final.pt'), map_location='cpu')
    assert list(sd)[:3] == ['spectrogram.lenghts', 'spectrogram.cqt_kernels_real', 'spectrogram.cqt_kernels_imag']
    assert tuple(sd['spectrogram.cqt_kernels_real'].shape) == (176, 1, 32768)
    m = ra.UNet_Onset(*DS, log=True, reconstruction=True, mode='imagewise', spec='CQT')
    m.load_state_dict(sd, strict=True)
