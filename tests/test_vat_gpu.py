"""vat.VAT -- the one power iteration behind UNet_VAT, stepwise_VAT and stepwise_VAT_frame_stack -- on the B = 2, T = 64 fixtures:
the power_iteration / final_loss split and `refs=` for all three classes, the random direction of n_power = 0 and the
`d = g * scale` branch of n_power = 2."""
import pytest
import torch

import test_model_gpu as tm
import test_onset_frames as to

pytestmark = pytest.mark.gpu
KINDS = ['unet_onset', 'unet', 'stepwise', 'frame_stack']      # UNet_VAT with two heads and with one, and the two stepwise classes


def _case(kind, dev):
    """(model in training mode with XI = 0.1, eps = 2 and dropout off, its VAT object with injected noise, x, d0)."""
    from oracle import fixture as fx, onset_frames as oo
    if kind in ('unet_onset', 'unet'):
        m = tm.build('onset' if kind == 'unet_onset' else 'frame', False, dev, xi=1e-1, eps=2.0)
        x = fx.fixture_spec(2, 64, 'spec_vat').to(dev)
    else:
        if kind == 'stepwise':
            m = to.build(dev, True, 1e-1, 2.0)
        else:
            from reconvat_amd import Frame_stack_VAT
            m = Frame_stack_VAT(229, 88, model_complexity=48, log=True, mode='imagewise', spec='Mel', XI=1e-1, eps=2.0, VAT_mode='all')
            m.load_state_dict(oo.fixture_params(kind='frame'))
            for mod in m.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.p = 0.0
            m.to(dev).train()
        x = fx.fixture_spec(2, 64, 'onf_spec').squeeze(1).to(dev)
    d0 = fx.fixture_noise(x.shape, 'd0_' + kind).to(dev)
    m.vat_loss.noise = lambda t: d0.clone()
    return m, m.vat_loss, x, d0


def _flat(result):
    """Every tensor of a VAT result, the per-head dictionary flattened in key order."""
    out = []
    for r in result:
        out += list(r.values()) if isinstance(r, dict) else [r]
    return out


def _same_bits(a, b):
    a, b = _flat(a), _flat(b)
    assert len(a) == len(b)
    for i, (s, t) in enumerate(zip(a, b)):
        assert s.shape == t.shape and torch.equal(s.detach(), t.detach()), i


@pytest.mark.parametrize('kind', KINDS)
def test_forward_is_power_iteration_then_final_loss(dev, kind):
    m, vat, x, _ = _case(kind, dev)
    stats = {k: v.clone() for k, v in m.state_dict().items() if 'running' in k or 'num_batches' in k}

    def restore():
        for k, v in m.state_dict().items():
            if k in stats:
                v.copy_(stats[k])
    whole = vat(m, x)
    assert len(whole) == (2 if kind == 'frame_stack' else 3)
    restore()
    x_adv, r_adv, d_norm, refs = vat.power_iteration(m, x)
    vat.check_nan()
    _same_bits(whole, (vat.final_loss(m, x_adv, refs), r_adv, d_norm)[:len(whole)])
    # the target predictions handed in: a forward pass with the same weights and the same running statistics
    restore()
    given = vat.outputs(m, x)
    restore()
    _same_bits(whole, vat(m, x, refs=given))
    x_adv2, _, _, refs2 = vat.power_iteration(m, x, refs=given)
    assert torch.equal(x_adv2, x_adv) and all(not r.requires_grad for r in refs2)
    assert int(vat.nan_flag.item()) == 0


@pytest.mark.parametrize('kind', KINDS)
def test_n_power_0_is_the_random_direction(dev, kind):
    """No power iteration: r_adv = eps * d0 / ||d0|| row by row (tolerances: float32 rounding of one normalisation)."""
    m, vat, x, d0 = _case(kind, dev)
    vat.n_power = 0
    r_adv = vat(m, x)[1]
    rn = r_adv.norm(dim=-1)
    assert torch.allclose(rn, torch.full_like(rn, 2.0), rtol=1e-5)
    cos = torch.nn.functional.cosine_similarity(r_adv.double(), d0.double(), dim=-1)
    assert float(cos.min()) >= 1 - 1e-6, float(cos.min())
    assert int(vat.nan_flag.item()) == 0
    assert all(p.grad is None for p in m.parameters())


@pytest.mark.parametrize('kind', KINDS)
def test_n_power_2_rescales_the_gradient(dev, kind):
    """Two power iterations: the second starts from d = g * scale (1e10; 1e20 in the frame-stack class)."""
    m, vat, x, _ = _case(kind, dev)
    vat.n_power = 2
    result = vat(m, x)
    assert int(vat.nan_flag.item()) == 0
    assert all(torch.isfinite(t).all() for t in _flat(result))
    rn = result[1].norm(dim=-1)
    assert torch.allclose(rn, torch.full_like(rn, 2.0), rtol=1e-5)
    assert all(p.grad is None for p in m.parameters())
