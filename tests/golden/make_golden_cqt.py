"""Generate tests/golden/cqt_*.npz by RUNNING THE REFERENCE with spec='CQT'.

Run where the reference checkout that _refload imports is available, in a process of its own -- the reference's CQT constructor sets
its module-global N_BINS to 176, so no Mel model may be built after it in the same process:

    python tests/golden/make_golden_cqt.py

The reference (imported unmodified through ``_refload``) takes its kernel bank from ``nnAudio.Spectrogram
.create_cqt_kernels``, looked up at construction time; nnAudio is not vendored, so that name is set to the product's
restatement (reconvat_amd.frontend.create_cqt_kernels, "parity unpinned").  The 176-bin fixture weights are
``oracle.fixture.fixture_params(with_frontend=False)`` with ``fixture.N_BINS`` set to 176 at run time.
Written (no kernel banks inside):
* cqt_frontend.npz: front-end outputs (magnitude, log + imagewise normalised) in float64 and the reference's own float32
  deviation from them, for two short clips and one full 327 679-sample clip (strided frame subset), and digests of the
  three buffers;
* cqt_models.npz: state_dict keys and shapes of the four model variants; run_on_batch losses (fp32 8 / 1 threads, fp64) and
  prediction digests for onset / frame x recon on / off x VAT on / off at B = 2, T = 64; one full-length (T = 640,
  B = 2 + 2) UNet_Onset VAT + reconstruction step's losses at fp32 8 / 1 threads and fp64.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refload  # noqa: E402
from oracle import fixture as fx  # noqa: E402
from reconvat_amd import frontend as rfe  # noqa: E402

torch.set_num_threads(8)
ref = _refload.load_reference()
sys.modules['nnAudio.Spectrogram'].create_cqt_kernels = rfe.create_cqt_kernels
fx.N_BINS = 176
DS = ((2, 2), (2, 2))

# (name, clip lengths): short clips just above the reflect pad and not a multiple of 512, one full training crop
SHORT = (('short_a', 16385 + 1000), ('short_b', 41234))
FULL = ('full', 327679)
FULL_FRAMES = np.r_[0:40, 40:600:8, 600:640]


def digest(t, n=96):
    f = t.detach().double().flatten()
    stride = max(1, f.numel() // n)
    return np.concatenate([[f.norm().item()], f[::stride][:n].numpy()]).astype(np.float64)


def ref_cqt():
    return sys.modules['nnAudio.Spectrogram'].CQT1992v2(sr=16000, hop_length=512, n_bins=176, fmin=27.5, bins_per_octave=24,
                                                        trainable=False, verbose=False)


def lognorm(mag):
    x = torch.log(mag + 1e-5)
    flat = x.reshape(x.shape[0], -1)
    mn, mx = flat.min(1, keepdim=True)[0].unsqueeze(1), flat.max(1, keepdim=True)[0].unsqueeze(1)
    return ((x - mn) / (mx - mn)).transpose(1, 2)          # [B, T, n_bins]


def g_frontend():
    out = {}
    spec = ref_cqt()
    for name in ('lenghts', 'cqt_kernels_real', 'cqt_kernels_imag'):
        out['buf_' + name] = digest(getattr(spec, name), 512)
    for name, n in SHORT + (FULL,):
        audio = fx.fixture_audio(1, n, 'cqt_' + name)
        res = {}
        for dt in ('f32', 'f64'):
            s = spec if dt == 'f32' else ref_cqt().double()
            mag = s(audio if dt == 'f32' else audio.double()).transpose(1, 2)        # [1, T, n_bins]
            res[dt] = (mag, lognorm(s(audio if dt == 'f32' else audio.double())))
        sel = FULL_FRAMES if name == 'full' else slice(None)
        for i, what in enumerate(('mag', 'lognorm')):
            a32, a64 = res['f32'][i].double(), res['f64'][i]
            out[f'{name}_{what}_f64'] = a64[0, sel].numpy()
            out[f'{name}_{what}_dev'] = float((a32 - a64).abs().max() / a64.abs().max())
            print(name, what, tuple(a64.shape), 'f32 vs f64 max rel dev', f"{out[f'{name}_{what}_dev']:.2e}")
    out['full_frames'] = FULL_FRAMES
    np.savez_compressed(os.path.join(HERE, 'cqt_frontend.npz'), **out)


def _batch(b, t, tag):
    onset, frame = fx.fixture_labels(b, t, tag)
    return {'audio': fx.fixture_audio(b, t * 512, tag), 'onset': onset, 'frame': frame}


def build_ref(kind, recon, dtype=torch.float32):
    cls = ref.UNet_Onset if kind == 'onset' else ref.UNet
    net = cls(*DS, log=True, reconstruction=recon, mode='imagewise', spec='CQT', XI=1e-6, eps=2.0)
    params = fx.fixture_params(kind, recon, with_frontend=False)
    params = {**{k: v for k, v in net.state_dict().items() if k.startswith('spectrogram.')}, **params}
    net.load_state_dict(params, strict=True)
    net.train(True)
    return net.double() if dtype == torch.float64 else net


def ref_losses(kind, recon, vat, bl, bul, noises, dtype, threads):
    real = torch.randn_like
    prev = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        net = build_ref(kind, recon, dtype)
        cast = lambda d: {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}
        seq = [n.to(dtype) for n in (noises if vat else noises[1:])]

        def fake(t, **kw):
            d = seq.pop(0).clone()
            return d.requires_grad_(True) if kw.get('requires_grad') else d
        torch.randn_like = fake
        pr, lr, sr = net.run_on_batch(cast(bl), cast(bul) if vat else None, vat)
    finally:
        torch.randn_like = real
        torch.set_num_threads(prev)
    return pr, lr


def g_models():
    out = {}
    for kind in ('onset', 'frame'):
        for recon in (False, True):
            net = build_ref(kind, recon)
            sd = net.state_dict()
            tag = f'{kind}_r{int(recon)}'
            out[tag + '_sd_keys'] = np.array(list(sd.keys()))
            out[tag + '_sd_shapes'] = np.array([','.join(map(str, v.shape)) for v in sd.values()])
    cases = [(kind, recon, vat, 64) for kind in ('onset', 'frame') for recon in (False, True) for vat in (False, True)]
    cases.append(('onset', True, True, 640))
    for kind, recon, vat, T in cases:
        bl, bul = _batch(2, T, 'L'), _batch(2, T, 'UL')
        noises = [fx.fixture_noise((2, 1, T, 176), 'd0_ul'), fx.fixture_noise((2, 1, T, 176), 'd0_l')]
        key = f'{kind}_r{int(recon)}_v{int(vat)}_T{T}'
        runs = {}
        for name, dtype, threads in (('f32_8t', torch.float32, 8), ('f32_1t', torch.float32, 1), ('f64', torch.float64, 8)):
            pr, lr = ref_losses(kind, recon, vat, bl, bul, noises, dtype, threads)
            runs[name] = pr
            out[f'{key}_{name}'] = np.array([float(v) for v in lr.values()], dtype=np.float64)
        out[key + '_keys'] = np.array(list(lr.keys()))
        base = out[key + '_f32_8t']
        den = np.maximum(np.abs(base), 1e-12)
        out[key + '_spread'] = np.max([np.abs(out[f'{key}_{n}'] - base) for n in ('f32_1t', 'f64')], axis=0) / den
        out[key + '_frame'] = digest(runs['f32_8t']['frame'], 256)
        if recon:
            out[key + '_rec'] = digest(runs['f32_8t']['reconstruction'], 256)
        print(key, {k.split('/')[-1]: f'{v:.5f}' for k, v in zip(out[key + '_keys'], base)})
    np.savez_compressed(os.path.join(HERE, 'cqt_models.npz'), **out)


if __name__ == '__main__':
    g_frontend()
    g_models()
