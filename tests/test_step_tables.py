"""model.step_tables / model.vat_terms (the one place that builds the `predictions` and `losses` of run_on_batch) on CPU tensors, with
the loss kernels substituted by torch.nn.functional: keys and key order against the goldens recorded from the reference, values against
the substituted functions; and the placeholder of a branch that did not run."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

G = os.path.join(os.path.dirname(__file__), 'golden')
B, T = 2, 64


def gold(name):
    return np.load(os.path.join(G, name + '.npz'), allow_pickle=False)


@pytest.fixture
def model(monkeypatch):
    from reconvat_amd import model
    calls = []

    def sub(name, fn):
        def f(p, t):
            calls.append(name)
            return fn(p, t)
        return f
    monkeypatch.setattr(model, 'bce_mean', sub('bce', F.binary_cross_entropy))
    monkeypatch.setattr(model, 'mse_mean', sub('mse', F.mse_loss))
    model.calls = calls
    return model


def _inputs(model, heads, recon, vat, training, seed):
    g = torch.Generator().manual_seed(seed)
    roll = lambda: torch.rand(B, T, 88, generator=g)
    out = {h: roll() for h in heads}
    out['attention'] = torch.rand(B, T, 6, 31, generator=g)
    if recon:
        out['reconstruction'] = torch.rand(B, 1, T, 229, generator=g)
        out.update({h + '2': roll() for h in heads})
    labels = {h: (roll() > 0.9).float() for h in heads}
    if not training:                       # eval mode: the frame heads (only they) are reshaped to the frame label's shape
        labels['frame'] = labels['frame'].reshape(1, B * T, 88)
    term = lambda: torch.rand((), generator=g) if vat else model.zero_loss()
    lds = lambda: {h: term() for h in heads} if len(heads) == 2 else term()
    plan = model.StepPlan(spec=torch.rand(B, 1, T, 229, generator=g), lds_l=lds(), lds_ul=lds(), r_norm_l=term(), r_norm_ul=term(),
                          r_adv=torch.rand(B, T, 229, generator=g) if vat else None)
    return out, labels, plan


def _check_values(losses, preds, out, labels, plan, heads, recon, tag):
    if recon:
        assert torch.equal(losses[f'loss/{tag}_reconstruction'], F.mse_loss(out['reconstruction'].squeeze(1), plan.spec.squeeze(1)))
    for h in heads:
        for s in ('', '2') if recon else ('',):
            assert torch.equal(losses[f'loss/{tag}_{h}{s}'], F.binary_cross_entropy(out[h + s].reshape(labels[h].shape), labels[h])), h + s
    lds = plan.lds_l if len(heads) == 2 else {None: plan.lds_l}
    for h, v in lds.items():
        assert losses[f'loss/{tag}_LDS_l' + (f'_{h}' if h else '')] is v
    assert losses[f'loss/{tag}_r_norm_l'] is plan.r_norm_l
    assert preds['r_adv'] is plan.r_adv and preds['attention'] is out['attention']


@pytest.mark.parametrize('kind', ['onset', 'frame'])
@pytest.mark.parametrize('recon', [False, True])
@pytest.mark.parametrize('vat', [False, True])
@pytest.mark.parametrize('training', [True, False])
def test_run_on_batch_tables(model, kind, recon, vat, training):
    g = gold('run_on_batch')
    heads = model.UNet_Onset.heads if kind == 'onset' else model.UNet.heads
    out, labels, plan = _inputs(model, heads, recon, vat, training, 7)
    preds, losses = model.step_tables(heads, training, labels, plan, out)
    assert list(losses) == list(g[f'{kind}_r{int(recon)}_v{int(vat)}_t{int(training)}_keys'])
    tag = 'train' if training else 'test'
    _check_values(losses, preds, out, labels, plan, heads, recon, tag)
    # launched in key order: the reconstruction MSE, then per head the first and the second transcriber pass
    assert model.calls == (['mse'] if recon else []) + ['bce'] * (len(heads) * (2 if recon else 1))
    want = (['frame', 'onset'] if kind == 'onset' else ['onset', 'frame']) + ['frame2', 'onset2', 'attention', 'r_adv', 'reconstruction'] \
        if recon else ['onset', 'frame', 'r_adv', 'attention']
    assert list(preds) == want
    assert preds['frame'].shape == labels['frame'].shape
    if kind == 'frame':
        assert preds['onset'] is preds['frame'] and (not recon or preds['onset2'] is preds['frame2'])
    else:
        assert preds['onset'] is out['onset']                # the onset head is not reshaped in eval mode
    if training:
        assert losses['loss/train_r_norm_ul'] is plan.r_norm_ul
        for h, v in (plan.lds_ul if kind == 'onset' else {None: plan.lds_ul}).items():
            assert losses['loss/train_LDS_ul' + (f'_{h}' if h else '')] is v


def test_two_stream_pack_launches_only_the_first_pass_losses(model):
    """The reconstruction branch's three losses arrive from the side stream; only BCE(frame), BCE(onset) are launched here."""
    g = gold('run_on_batch')
    heads = model.UNet_Onset.heads
    out, labels, plan = _inputs(model, heads, True, True, True, 11)
    side = {k: torch.rand(()) for k in ('reconstruction', 'frame2', 'onset2')}
    plan.pack = ({k: out[k] for k in side}, side)
    preds, losses = model.step_tables(heads, True, labels, plan, out)
    assert list(losses) == list(g['onset_r1_v1_t1_keys'])
    assert model.calls == ['bce', 'bce']
    for k, v in side.items():
        assert losses[f'loss/train_{k}'] is v
    for h in heads:
        assert torch.equal(losses[f'loss/train_{h}'], F.binary_cross_entropy(out[h], labels[h]))
    assert list(preds) == ['frame', 'onset', 'frame2', 'onset2', 'attention', 'r_adv', 'reconstruction']


@pytest.mark.parametrize('training', [True, False])
def test_application_tables(model, training):
    g = gold('application')
    heads = model.UNet.heads
    out, labels, plan = _inputs(model, heads, True, True, training, 13)
    ul = (torch.rand(B, T, 88), torch.rand(B, T, 88))
    preds, losses = model.step_tables(heads, training, labels, plan, out, ul=ul)
    t = f't{int(training)}'
    assert list(losses) == list(g[t + '_keys'])
    assert list(preds) == list(g[t + '_pred_keys'])
    _check_values(losses, preds, out, labels, plan, heads, True, 'train' if training else 'test')
    if training:
        assert torch.equal(losses['loss/ul_consistency_wrt1'], F.binary_cross_entropy(ul[1], ul[0]))
        assert preds['ul_frame'] is ul[0] and preds['ul_frame2'] is ul[1]
        assert model.calls == ['mse', 'bce', 'bce', 'bce']


@pytest.mark.parametrize('vat', [False, True])
@pytest.mark.parametrize('training', [True, False])
def test_onsets_and_frames_vat_keys(model, vat, training):
    """OnsetsAndFrames_VAT_full appends the shared VAT keys to its two head losses."""
    g = gold('onset_frames')
    _, _, plan = _inputs(model, ('frame',), False, vat, training, 17)
    tag = 'train' if training else 'test'
    losses = model.vat_terms({f'loss/{tag}_frame': torch.tensor(1.), f'loss/{tag}_onset': torch.tensor(2.)}, training, plan)
    assert list(losses) == list(g[f'rob_v{int(vat)}_t{int(training)}_keys'])
    assert losses[f'loss/{tag}_LDS_l'] is plan.lds_l


def test_placeholders_are_cpu_zeros():
    """A branch that did not run contributes a CPU zero, as in the reference; weighted_loss adds such terms on the host."""
    import reconvat_amd as ra
    from reconvat_amd import model
    z = model.zero_loss()
    assert z.device.type == 'cpu' and z.dtype == torch.float32 and z.dim() == 0 and float(z) == 0.0 and not z.requires_grad
    assert model.zero_loss() is not z
    m = ra.UNet_Onset(((2, 2), (2, 2))[0], (2, 2), reconstruction=False, spec='Mel')
    lds, r_norm = m._no_vat()
    assert list(lds) == ['frame', 'onset'] and all(v.device.type == 'cpu' and float(v) == 0.0 for v in lds.values()) and float(r_norm) == 0.0
    lds, r_norm = ra.UNet((2, 2), (2, 2), reconstruction=False, spec='Mel')._no_vat()
    assert lds.device.type == 'cpu' and float(lds) == 0.0 and float(r_norm) == 0.0
    x = torch.tensor(3.0, requires_grad=True)
    total = ra.weighted_loss({'loss/train_frame': x * 2, 'loss/train_LDS_l': model.zero_loss(), 'loss/train_r_norm_l': model.zero_loss()}, 1.0)
    assert float(total.detach()) == 6.0
    total.backward()
    assert float(x.grad) == 2.0
