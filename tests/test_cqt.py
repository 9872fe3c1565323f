"""CPU checks of the constant-Q front end's kernel bank and of the spec='CQT' model surface (no GPU needed)."""
import os

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(__file__), 'golden')
DS = ((2, 2), (2, 2))


@pytest.fixture(scope='module')
def layer():
    from reconvat_amd.frontend import CQT1992v2
    return CQT1992v2(sr=16000, hop_length=512, n_bins=176, fmin=27.5, bins_per_octave=24, trainable=False)


def gold(name):
    return np.load(os.path.join(G, name + '.npz'), allow_pickle=False)


def test_bank_closed_form(layer):
    Q = 1 / (2 ** (1 / 24) - 1)
    k = np.arange(176)
    f = 27.5 * 2.0 ** (k / 24)
    l = np.ceil(Q * 16000 / f)
    assert layer.kernel_width == 32768 and layer.n_bins == 176
    assert np.array_equal(layer.lenghts.numpy(), l.astype(np.float32))
    assert l[0] == 19856 and l[-1] == 127
    re = layer.cqt_kernels_real[:, 0].double().numpy()
    im = layer.cqt_kernels_imag[:, 0].double().numpy()
    z = re + 1j * im
    # every row: L1 norm 1, support exactly l_k taps, centred (odd l: one sample earlier)
    np.testing.assert_allclose(np.abs(z).sum(1), 1.0, rtol=2e-5)
    nz = np.abs(z) > 0
    first, last = nz.argmax(1), 32767 - nz[:, ::-1].argmax(1)
    start = np.ceil(16384 - l / 2).astype(int) - (l % 2 == 1)
    # the periodic Hann window is zero at n = 0: the first stored tap of a row is exactly zero
    assert np.array_equal(first, start + 1) and np.array_equal(last, start + l.astype(int) - 1)
    # spectral peak at f_k (the kernel is a windowed complex exponential at f_k)
    for kk in (0, 40, 100, 175):
        freqs = f[kk] * np.array([0.97, 1.0, 1.03])
        n = np.arange(32768)
        resp = np.abs(z[kk] @ np.exp(-2j * np.pi * freqs[:, None] * n[None, :] / 16000).T)
        assert resp.argmax() == 1, (kk, resp)


def test_bank_matches_golden_digests(layer):
    g = gold('cqt_frontend')
    for name in ('lenghts', 'cqt_kernels_real', 'cqt_kernels_imag'):
        f = getattr(layer, name).double().flatten()
        stride = max(1, f.numel() // 512)
        d = np.concatenate([[f.norm().item()], f[::stride][:512].numpy()])
        np.testing.assert_array_equal(d, g['buf_' + name])


def test_tables_are_banded_and_cover_every_tap(layer):
    from reconvat_amd.frontend import CQT_SLICE, cqt_gflop
    t = layer.tables()
    items, groups = t['items'].numpy(), t['groups'].numpy()
    assert groups.shape == (11, 2) and items.shape[1] == 8
    exact, tiled = cqt_gflop(t, 16, 640)
    assert abs(exact - 28.39) < 0.01 and abs(tiled - 35.06) < 0.01
    re, im = layer.cqt_kernels_real[:, 0].numpy(), layer.cqt_kernels_imag[:, 0].numpy()
    w = t['w'].numpy()
    for gi, (i0, ni) in enumerate(groups):
        its = items[i0:i0 + ni]
        assert (its[:, 0] == gi).all() and (its[:, 2] <= CQT_SLICE).all() and (its[:, 2] % 16 == 0).all()
        tw, kg, woff = its[0, 1], its[0, 4], its[0, 3]
        assert its[:, 2].sum() == kg and 0 <= tw and tw + kg <= 32768
        blk = w[woff:woff + 32 * kg].reshape(32, kg)
        rows = slice(16 * gi, 16 * gi + 16)
        assert np.array_equal(blk[:16], re[rows, tw:tw + kg]) and np.array_equal(blk[16:], im[rows, tw:tw + kg])
        # nothing outside the window
        assert not re[rows, :tw].any() and not re[rows, tw + kg:].any() and not im[rows, tw + kg:].any()
    assert t['scale'].dtype == torch.float32
    # the tables follow the buffers
    layer.lenghts.mul_(1.0)
    assert layer.tables() is not t
    t2 = layer.tables()
    assert layer.tables() is t2


@pytest.mark.parametrize('kind', ['onset', 'frame'])
@pytest.mark.parametrize('recon', [False, True])
def test_cqt_state_dict_is_the_reference_layout(kind, recon):
    """UNet_Onset((2, 2), (2, 2)) -- the reference's default constructor call, spec='CQT' -- constructs, and its state_dict has
    the reference's keys, order and shapes (176-wide layers); a reference-shaped state_dict loads with strict=True."""
    import reconvat_amd as ra
    g = gold('cqt_models')
    cls = ra.UNet_Onset if kind == 'onset' else ra.UNet
    m = cls(*DS) if recon else cls(*DS, reconstruction=False)
    sd = m.state_dict()
    tag = f'{kind}_r{int(recon)}'
    assert list(sd.keys()) == [str(k) for k in g[tag + '_sd_keys']]
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[tag + '_sd_shapes']]
    other = cls(*DS, reconstruction=recon)
    other.load_state_dict({k: v.clone() + (0.5 if v.is_floating_point() and not k.startswith('spectrogram.') else 0)
                           for k, v in sd.items()}, strict=True)


def test_cqt_then_mel_keeps_mel_229_wide():
    import reconvat_amd as ra
    c = ra.UNet_Onset(*DS, spec='CQT')
    m = ra.UNet_Onset(*DS, spec='Mel')
    u = ra.UNet(*DS, spec='Mel')
    assert c.reconstructor.linear2.weight.shape == (176, 704) and c.transcriber.lstm1.W_k.weight.shape == (704, 264)
    assert m.reconstructor.linear2.weight.shape == (229, 916) and m.transcriber.linear_onset.weight.shape == (88, 229)
    assert u.transcriber.lstm1.W_k.weight.shape == (916, 229)
    assert m.spectrogram.mel_basis.shape == (229, 1025)


def test_cqt_unsupported_options_raise():
    import reconvat_amd as ra
    from reconvat_amd.frontend import CQT1992v2
    from reconvat_amd.onset_frames import OnsetsAndFrames_VAT_full
    with pytest.raises(NotImplementedError, match='trainable'):
        CQT1992v2(sr=16000, n_bins=176, fmin=27.5, bins_per_octave=24, trainable=True)
    for fmt in ('Complex', 'Phase'):
        with pytest.raises(NotImplementedError, match='Magnitude'):
            CQT1992v2(sr=16000, n_bins=176, fmin=27.5, bins_per_octave=24, output_format=fmt)
    layer = CQT1992v2(sr=16000, hop_length=512, n_bins=176, fmin=27.5, bins_per_octave=24)
    with pytest.raises(ValueError, match='longer than the reflect padding'):
        layer(torch.zeros(1, 16384))
    with pytest.raises(NotImplementedError, match='CFP'):
        ra.UNet_Onset(*DS, spec='CFP')
    with pytest.raises(NotImplementedError):
        OnsetsAndFrames_VAT_full(229, 88, spec='CQT')
