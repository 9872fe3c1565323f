"""The optimiser options of the fused step on the GPU: clip before the update, decoupled weight decay and the
exponential moving average of the weights -- rv_adamw_step / rv_swap_floats, FlatAdam, TrainStep and the command line."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 7                      # optimiser steps of the torch comparison
MAX_NORM = 3.0
# 1 090 dense Gaussian gradient elements have a norm of ~33: these factors put it at ~0.7 16 1.6 33 1.0 6.6 2.0 (and half of
# that with grad_scale = 0.5), i.e. on both sides of MAX_NORM
GRAD_FACTORS = (0.02, 0.5, 0.05, 1.0, 0.03, 0.2, 0.06)
SHAPES = ((7, 5), (33,), (4, 3, 2), (1031,))     # test_adam's set (the 33 never receive a gradient) + one with a 4-float tail
NEVER = 1
EMA_DECAY = 0.9


def uniform(*shape, seed):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def gauss(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


@pytest.fixture(scope='module', params=[1.0, 0.5], ids=['grad_scale=1', 'grad_scale=0.5'])
def trajectory(request, dev):
    """K steps of FlatAdam with all three options on, and of torch.optim.AdamW + StepLR with clip_grad_norm_ BEFORE each step on the
    CPU, on the same gradients (torch gets them times grad_scale).  Run once per grad_scale, shared by the tests below."""
    from reconvat_amd.train import FlatAdam
    grad_scale = request.param
    init = [uniform(*s, seed=1 + i) for i, s in enumerate(SHAPES)]
    ref = [torch.nn.Parameter(p.clone()) for p in init]
    gp = [torch.nn.Parameter(p.clone().to(dev)) for p in init]
    o_ref = torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.01)
    sch = torch.optim.lr_scheduler.StepLR(o_ref, step_size=3, gamma=0.5)
    o = FlatAdam(gp, lr=1e-3, step_size=3, gamma=0.5, data_parallel=False, weight_decay=0.01, max_grad_norm=MAX_NORM,
                 ema_decay=EMA_DECAY)
    o.grad_scale = grad_scale
    ema0 = o.flat_ema.cpu().clone()
    assert torch.equal(ema0, o.flat_param.cpu())                 # the average starts as a copy of the weights
    norms, flats = [], []
    for it in range(K):
        o.zero_grad()
        o_ref.zero_grad()
        for i, (a, r) in enumerate(zip(gp, ref)):
            if i == NEVER:
                continue
            g = gauss(*a.shape, seed=10 * it + i) * GRAD_FACTORS[it]
            r.grad = g * grad_scale
            a.grad.copy_(g.to(dev))
        norms.append(float(torch.nn.utils.clip_grad_norm_([r for r in ref if r.grad is not None], MAX_NORM)))
        o.step()
        o_ref.step()
        sch.step()
        flats.append(o.flat_param.cpu().clone())
    return {'opt': o, 'gpu': gp, 'ref': ref, 'init': init, 'norms': norms, 'flats': flats, 'ema0': ema0,
            'lr_ref': o_ref.param_groups[0]['lr']}


def test_clip_decay_against_torch_adamw(trajectory):
    """rel_err < 1e-5 per tensor: test_adam's bar for the same recursion (decay and clip add one rounding each per step); the
    tensor that never received a gradient does not move, weight decay or not."""
    t = trajectory
    clipped = [n > MAX_NORM for n in t['norms']]
    print('gradient norms', t['norms'])
    assert any(clipped) and not all(clipped), t['norms']
    for i, (a, r) in enumerate(zip(t['gpu'], t['ref'])):
        err = rel_err(a, r)
        print('tensor', i, tuple(a.shape), 'rel_err', err)
        assert err < 1e-5, (i, err)
    assert torch.equal(t['gpu'][NEVER].detach().cpu(), t['init'][NEVER])
    assert torch.equal(t['ref'][NEVER].detach(), t['init'][NEVER])          # ... like torch, which skips it
    o = t['opt']
    assert abs(o.current_lr() - t['lr_ref']) < 1e-12
    assert int(o.step_count.item()) == K
    # the pad elements of the flat buffers stay zero
    used = torch.zeros(o.n, dtype=torch.bool)
    for p, off in zip(o.params, o.offsets):
        used[off:off + p.numel()] = True
    assert int((~used).sum()) == 1 + 3 + 0 + 1
    for buf in (o.flat_param, o.flat_ema, o.exp_avg, o.exp_avg_sq):
        assert float(buf.cpu()[~used].abs().max()) == 0.0
    # checkpoint layout: torch's, with the real weight decay in the param group and no averaged weights in the file
    sd = o.state_dict()
    assert set(sd) == {'state', 'param_groups'} and sd['param_groups'][0]['weight_decay'] == 0.01
    assert set(sd['state']) == {0, 2, 3} and all(set(v) == {'step', 'exp_avg', 'exp_avg_sq'} for v in sd['state'].values())


def test_ema_recursion(trajectory):
    """e <- d e + (1 - d) p_k in float64 on the parameters read back after every step.  Each device step rounds at most three times
    (two products, one sum), each by at most half an ulp of max(|e|, |p|) <= 2^-24 max|p|, and earlier errors shrink by d: the
    final error is below 3 K 2^-24 max|p| / 2 < 2 K 2^-24 max|p|."""
    t = trajectory
    e = t['ema0'].double()
    for p in t['flats']:
        e = EMA_DECAY * e + (1 - EMA_DECAY) * p.double()
    got = t['opt'].flat_ema.cpu().double()
    bound = 2 * K * 2.0 ** -24 * float(t['flats'][-1].abs().max())
    err = float((got - e).abs().max())
    print('ema error', err, 'bound', bound)
    assert err <= bound, (err, bound)
    assert float((got - t['flats'][-1].double()).abs().max()) > 100 * bound          # ... and it is an average, not a copy


def _adam_buffers(dev, n, offset):
    """p, g (three steps of them), m, v of n floats starting `offset` floats into 16-byte aligned allocations."""
    mk = lambda seed, f: torch.cat([torch.zeros(offset), f(n, seed=seed)]).to(dev)
    p, m, v = mk(1, uniform), torch.zeros(offset + n, device=dev), torch.zeros(offset + n, device=dev)
    gs = []
    for it in range(3):
        g = gauss(n, seed=20 + it)
        g[:5] = 0.0                      # elements whose gradient is zero from the first step on
        g[7 + it] = 0.0                  # ... and ones that see a zero gradient later
        gs.append(torch.cat([torch.zeros(offset), g]).to(dev))
    return p, gs, m, v


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset_by_one_float'])
def test_neutral_options_are_the_old_kernel(dev, offset):
    """rv_adamw_step(weight_decay = 0, max_grad_norm = 0, total_norm = NULL, ema = NULL) against rv_adam_step on identical copies:
    n = 1 031 (16-byte path + scalar tail) and the same buffers one float further (scalar path); bit-equal after 3 steps."""
    from reconvat_amd._lib import call, stream
    n = 1031
    p0, gs, m0, v0 = _adam_buffers(dev, n, offset)
    assert p0.data_ptr() % 16 == 0 and p0[offset:].data_ptr() % 16 == 4 * offset
    res = []
    for new in (False, True):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        step = torch.zeros((), device=dev, dtype=torch.int64)
        for g in gs:
            head = (p[offset:].data_ptr(), g[offset:].data_ptr(), m[offset:].data_ptr(), v[offset:].data_ptr(), n, step.data_ptr(),
                    1e-3, 2, 0.5, 0.9, 0.999, 1e-8, 0.5, None)
            if new:
                call('rv_adamw_step', *head, 0.0, 0.0, None, None, 0.0, stream())
            else:
                call('rv_adam_step', *head, stream())
            call('rv_counter_add', step.data_ptr(), 1, None, stream())
        torch.cuda.synchronize()
        assert int(step.item()) == 3
        res.append((p.cpu(), m.cpu(), v.cpu()))
    (p_a, m_a, v_a), (p_b, m_b, v_b) = res
    assert not torch.equal(p_a, p0.cpu())
    assert torch.equal(p_a, p_b) and torch.equal(m_a, m_b) and torch.equal(v_a, v_b)


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset_by_one_float'])
def test_swap_floats(dev, offset):
    from reconvat_amd._lib import call, stream
    n = 1031
    a0, b0 = uniform(n + offset + 3, seed=5), uniform(n + offset + 3, seed=6)
    a, b = a0.to(dev), b0.to(dev)
    call('rv_swap_floats', a[offset:].data_ptr(), b[offset:].data_ptr(), n, stream())
    ea, eb = a0.clone(), b0.clone()
    ea[offset:offset + n], eb[offset:offset + n] = b0[offset:offset + n], a0[offset:offset + n]
    assert torch.equal(a.cpu(), ea) and torch.equal(b.cpu(), eb)          # the floats around the range are untouched


def test_skip_word_leaves_everything_untouched(dev):
    """With the per-device error word set, one step() writes nothing: p, m, v, the averaged weights and the step counter."""
    from reconvat_amd import ops
    from reconvat_amd.train import FlatAdam
    gp = [torch.nn.Parameter(uniform(*s, seed=1 + i).to(dev)) for i, s in enumerate(SHAPES)]
    o = FlatAdam(gp, lr=1e-3, step_size=3, gamma=0.5, data_parallel=False, weight_decay=0.01, max_grad_norm=MAX_NORM, ema_decay=EMA_DECAY)
    for it in range(2):
        o.flat_grad.copy_(gauss(o.n, seed=it).to(dev))
        o.step()
    names = ('flat_param', 'exp_avg', 'exp_avg_sq', 'flat_ema', 'step_count')
    before = {k: getattr(o, k).clone() for k in names}
    assert int(before['step_count']) == 2 and not torch.equal(before['flat_ema'], before['flat_param'])
    word = ops.step_error_word(dev)
    assert int(word.item()) == 0
    word.fill_(1)
    try:
        o.flat_grad.copy_(gauss(o.n, seed=9).to(dev))
        o.step()
        torch.cuda.synchronize()
    finally:
        word.zero_()
    for k in names:
        assert torch.equal(getattr(o, k), before[k]), k
    o.step()                                                     # the word is clear again: the same gradient now applies
    assert int(o.step_count.item()) == 3 and not torch.equal(o.flat_param, before['flat_param'])


# ---- the model fixture (UNet_Onset, T = 64, B = 2: the smallest one the suite runs) ---------------------------------------------
def _model(dev, training=True):
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel')
    m.load_state_dict(fx.fixture_params('onset', True))
    m.to(dev)
    m.train(training)
    return m


def _batch(dev, tag):
    from oracle import fixture as fx
    onset, frame = fx.fixture_labels(2, 64, tag)
    return {'audio': fx.fixture_audio(2, 64 * 512, tag).to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev)}


def _eval_forward(m, x):
    m.eval()
    with torch.no_grad():
        return [t.clone() for t in m(x)]


def test_ema_weights_context(dev, monkeypatch):
    """Inside ema_weights() the model IS the averaged model -- parameters and, through the invalidated packed-weight cache, its
    forward --; after it, the raw model again, bit for bit."""
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = _model(dev)
    opt = ra.FlatAdam(m.parameters(), lr=1e-3, ema_decay=0.5)
    step = ra.TrainStep(m, opt, _batch(dev, 'L'), None, VAT=False, graph=False)
    for _ in range(2):
        step()
    x = fx.fixture_spec(2, 64).to(dev)
    raw = {k: v.clone() for k, v in m.state_dict().items()}
    y_raw = _eval_forward(m, x)
    ema_sd = opt.ema_state_dict(m)
    assert list(ema_sd) == list(raw)
    params = {n for n, _ in m.named_parameters()}
    assert any(not torch.equal(ema_sd[k], raw[k]) for k in params)
    assert all(torch.equal(ema_sd[k], raw[k]) for k in raw if k not in params)            # buffers: the live ones
    other = _model(dev, training=False)
    other.load_state_dict(ema_sd, strict=True)
    y_other = _eval_forward(other, x)
    with monkeypatch.context() as mp:                            # (no real capture needed to see the refusal)
        mp.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        with pytest.raises(RuntimeError, match='capturing'):
            with opt.ema_weights():
                pass
    assert torch.equal(m.state_dict()[next(iter(params))], raw[next(iter(params))])
    with opt.ema_weights():
        inside = m.state_dict()
        for k in raw:
            assert torch.equal(inside[k], ema_sd[k]), k
        assert all(torch.equal(v, ema_sd[k]) for k, v in opt.ema_state_dict(m).items())   # the same dict from inside the context
        y_in = _eval_forward(m, x)
        with pytest.raises(RuntimeError, match='inside ema_weights'):
            opt.step()
    assert len(y_in) == len(y_other) == len(y_raw)
    for a, b in zip(y_in, y_other):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(y_in, y_raw))
    after = m.state_dict()
    for k in raw:
        assert torch.equal(after[k], raw[k]), k
    for a, b in zip(_eval_forward(m, x), y_raw):
        assert torch.equal(a, b)
    # load_ema round trip
    opt.flat_ema.zero_()
    opt.load_ema(ema_sd, m)
    assert all(torch.equal(v, ema_sd[k]) for k, v in opt.ema_state_dict(m).items())


def test_graph_and_eager_steps_agree_bitwise(dev, monkeypatch):
    """Three steps with all three options on, RV_DETERMINISTIC reductions: the hipGraph TrainStep (the norm reduction, the optimiser
    kernel and the average run after every replay) and the eager one leave the same bits."""
    import reconvat_amd as ra
    from reconvat_amd import ops
    monkeypatch.setattr(ops, 'DETERMINISTIC', [True])
    batches = [_batch(dev, f'R{i}') for i in range(3)]
    res = []
    for graph in (False, True):
        m = _model(dev)
        opt = ra.FlatAdam(m.parameters(), lr=1e-3, step_size=2, gamma=0.5, weight_decay=0.01, max_grad_norm=3.0, ema_decay=0.9)
        step = ra.TrainStep(m, opt, batches[0], None, VAT=False, clip=3.0, graph=graph)
        for b in batches:
            step.load(b, None)
            step()
        torch.cuda.synchronize()
        step.check()
        assert int(opt.step_count.item()) == 3
        res.append({k: getattr(opt, k).clone() for k in ('flat_param', 'flat_ema', 'exp_avg', 'exp_avg_sq')})
        print('graph' if graph else 'eager', 'gradient norm of the last step', float(opt.norm_buf))
    for k in res[0]:
        diff = float((res[0][k].double() - res[1][k].double()).abs().max())
        print(k, 'max |eager - graph|', diff)
        assert torch.equal(res[0][k], res[1][k]), (k, diff)
    assert not torch.equal(res[0]['flat_ema'], res[0]['flat_param'])


# ---- the command line ------------------------------------------------------------------------------------------------------------
SMALL = ['train_on=Synthetic', 'small=True', 'supersmall=True', 'sequence_length=32768', 'batch_size=2', 'train_batch_size=2',
         'iteration=2']


def _run(*args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'train_UNet_Onset_VAT.py'), 'with', *args], capture_output=True,
                          text=True, cwd=ROOT, env=env, timeout=timeout)


def test_command_line(dev, tmp_path):
    import reconvat_amd as ra
    logdir = str(tmp_path / 'run')
    opts = ['ema_decay=0.9', 'weight_decay=0.01', 'clip_before_step=True']
    p = _run(*SMALL, *opts, 'epoches=2', 'saving_freq=1', f'logdir={logdir}')
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout
    assert 'Validation of epoch 1 on the averaged weights' in p.stdout
    assert 'the final evaluation run on the averaged weights' in p.stdout
    for f in ('model-1.pt', 'model-1.ema.pt', 'model-2.pt', 'model-2.ema.pt', 'model-final.pt', 'model-final.ema.pt'):
        assert os.path.exists(os.path.join(logdir, f)), f
    sd = torch.load(os.path.join(logdir, 'model-2.pt'), map_location='cpu')
    ema = torch.load(os.path.join(logdir, 'model-2.ema.pt'), map_location='cpu')
    assert list(ema) == list(sd)
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=False, mode='imagewise', spec='Mel')
    m.load_state_dict(ema, strict=True)
    params = {n for n, _ in m.named_parameters()}
    assert any(not torch.equal(ema[k], sd[k]) for k in params)
    for k in sd:
        if k not in params:
            assert torch.equal(ema[k], sd[k]), k
    osd = torch.load(os.path.join(logdir, 'last-optimizer-state.pt'), map_location='cpu')
    assert set(osd) == {'state', 'param_groups'} and osd['param_groups'][0]['weight_decay'] == 0.01
    p = _run(*SMALL, *opts, 'epoches=3', 'saving_freq=1', f'logdir={logdir}', 'resume_iteration=2')
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Resumed the averaged weights from model-2.ema.pt' in p.stdout and 'Train Epoch: 3' in p.stdout
    assert os.path.exists(os.path.join(logdir, 'model-3.ema.pt'))
    p = _run(*SMALL, 'fused_optimizer=False', 'ema_decay=0.9', 'epoches=1', f'logdir={tmp_path / "torch"}')
    assert p.returncode != 0 and 'need fused_optimizer=True' in (p.stderr + p.stdout) and 'Traceback' not in p.stderr
