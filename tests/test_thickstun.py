"""CPU tests of the Thickstun baseline's host side: public surface, state_dict layout, feature re-indexing, the training script's
config, the C ABI declarations, and a pure-torch restatement of the window-sharing algorithm against the reference's golden."""
import os
import re
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thickstun_fixture as tf  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_state_dict_layout():
    """Same keys, order and shapes as the reference class (recorded in the golden), 31 510 656 parameters, no load_my_state_dict."""
    from reconvat_amd import Thickstun
    g = tf.golden()
    m = Thickstun()
    sd = m.state_dict()
    assert list(sd) == [str(k) for k in g['sd_keys']]
    assert [','.join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g['sd_shapes']]
    n = sum(p.numel() for p in m.parameters())
    assert n == 31510656 == int(g['n_params'])
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in tf.SHAPES]
    assert not hasattr(m, 'load_my_state_dict')
    for attr in ('normalize', 'CNN_freq', 'CNN_time', 'linear', 'spectrogram'):
        assert hasattr(m, attr)
    m.load_state_dict({**sd, **tf.params()}, strict=True)


def test_feature_reindex_round_trip():
    """linear.weight's feature c*51 + f is z3's feature f*4096 + c; the gradient mapping back is the inverse permutation."""
    from reconvat_amd import ops
    seen = set()
    for c in (0, 1, 77, 4095):
        for f in (0, 1, 50):
            ck, z = ops.thick_feature_index(c, f)
            assert ck == c * 51 + f and z == f * 4096 + c
            seen.add((ck, z))
    assert len({a for a, _ in seen}) == len({b for _, b in seen}) == len(seen)
    channels, rows, n = 8, 51, 4
    w = torch.arange(n * channels * rows, dtype=torch.float32).view(n, channels * rows)
    wlt = w.view(n, channels, rows).permute(2, 1, 0).reshape(rows * channels, n)            # what thick_wlt packs on the device
    for c, f, o in ((0, 0, 0), (3, 17, 2), (7, 50, 3)):
        ck, z = ops.thick_feature_index(c, f, channels, rows)
        assert wlt[z, o] == w[o, ck]
    assert torch.equal(ops.thick_wlt_grad_to_checkpoint(wlt.contiguous(), channels), w)


def test_script_config_defaults():
    """train_baseline_Thickstun.py parses `with k=v` and reports the reference's defaults."""
    from reconvat_amd.cli import thickstun_config
    from reconvat_amd.sacred_lite import parse_cli
    c = thickstun_config({})
    want = dict(train_on='String', small=True, supersmall=True, batch_size=1, train_batch_size=1, learning_rate=1e-4,
                learning_rate_decay_steps=1000, learning_rate_decay_rate=0.98, clip_gradient_norm=3, logging_freq=10, saving_freq=10,
                sequence_length=327680, epoches=20000, spec='Mel', eps=1.3, XI=1e-6, root='runs')
    for k, v in want.items():
        assert c[k] == v, (k, c[k], v)
    assert c['logdir'].startswith('runs/baseline_ThickStun-lr=0.0001')
    c = thickstun_config(parse_cli(['with', 'train_on=Synthetic', 'epoches=2', 'learning_rate=0.001']))
    assert c['train_on'] == 'Synthetic' and c['epoches'] == 2 and 'lr=0.001' in c['logdir']
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_baseline_Thickstun.py'), 'with', 'no_such_key=1'], capture_output=True,
                       text=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert p.returncode != 0 and 'no_such_key' in p.stderr


def test_train_model_loop_order():
    """train_model: one pass over the WHOLE loader, run_on_batch -> zero_grad -> backward -> step -> scheduler.step -> clip."""
    from reconvat_amd import train_model
    log = []

    class M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(3))

        def run_on_batch(self, batch):
            log.append('run')
            return {'frame': self.w}, {'loss/train_frame': (self.w * batch).sum()}, None

    class Opt(torch.optim.SGD):
        def zero_grad(self, *a, **k):
            log.append('zero')
            return super().zero_grad(*a, **k)

        def step(self, *a, **k):
            log.append('step')
            return super().step(*a, **k)

    m = M()
    opt = Opt(m.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.5)

    class Loader(list):
        batch_size = 1
        dataset = [0] * 5
    pred, losses, o = train_model(m, 1, Loader([torch.full((3,), float(i)) for i in range(5)]), opt, sched, 3)
    assert log == ['run', 'zero', 'step'] * 5 and o is opt
    assert abs(opt.param_groups[0]['lr'] - 0.1 * 0.5 ** 2) < 1e-12          # five scheduler steps
    assert float(m.w.grad.norm()) <= 3 + 1e-5                               # clipped after the step
    assert set(losses) == {'loss/train_frame'}


def test_header_declares_every_prototype():
    """include/reconvat_hip.h declares every rv_thick_* symbol that _lib.py prototypes, with the same number of arguments."""
    from reconvat_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read()
    names = [n for n in _lib.SIGNATURES if n.startswith('rv_thick_')]
    assert set(names) >= {'rv_thick_freq_fwd', 'rv_thick_freq_bwd', 'rv_thick_tconv_fwd', 'rv_thick_linear_dz'}
    source = open(os.path.join(ROOT, 'reconvat_amd', 'csrc', 'thickstun.hip')).read()
    for n in names:
        decl = re.search(r'\b(?:int|long)\s+' + n + r'\s*\(([^;]*?)\)\s*;', header, re.S)
        assert decl, f'{n} is not declared in reconvat_hip.h'
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[n][1]), n
        assert re.search(r'\b(?:int|long)\s+' + n + r'\s*\(', source), f'{n} is not defined in thickstun.hip'
    from reconvat_amd import build
    assert 'thickstun.hip' in build.SOURCES


def shared_window_form(spec, p, labels):
    """The algorithm of csrc/thickstun.hip restated in torch: relu(CNN_freq) ONCE over the zero-padded spectrogram, kept channels-last
    [B, 51, T+24, 128]; CNN_time as a GEMM over the Hankel view (25*128 contiguous values per output row) with the weight flattened
    as W[n, j*128 + c]; the linear layer on z3 [B*T, 51*4096] with its weight re-indexed from c*51+f to f*4096+c."""
    b, bins, t = spec.shape
    img = F.pad(spec, (12, 12)).unsqueeze(1)                                                   # [B, 1, 229, T+24]
    z2 = torch.relu(F.conv2d(img, p['CNN_freq.weight'], p['CNN_freq.bias'], stride=(2, 1)))      # [B, 128, 51, T+24]
    z2 = z2.permute(0, 2, 3, 1).contiguous()                                                   # [B, 51, T+24, 128]
    hankel = z2.as_strided((b, 51, t, 25 * 128), ((51 * (t + 24)) * 128, (t + 24) * 128, 128, 1))
    wflat = p['CNN_time.weight'][:, :, 0, :].permute(0, 2, 1).reshape(4096, 25 * 128)
    z3 = torch.relu(hankel @ wflat.t() + p['CNN_time.bias'])                                    # [B, 51, T, 4096]
    z3 = z3.permute(0, 2, 1, 3).reshape(b * t, 51 * 4096)                                       # rows (b, t), features f*4096 + c
    wl = p['linear.weight'].view(88, 4096, 51).permute(0, 2, 1).reshape(88, 51 * 4096)
    pred = torch.sigmoid(z3 @ wl.t())
    return pred, F.binary_cross_entropy(pred, labels.reshape(-1, 88))


def test_shared_window_form_reproduces_reference():
    """Golden case 1 from the reference's windowed class equals the shared-window restatement (fp64 on the golden's fp64 spec: the two
    forms are the same sums, so they agree to fp64 rounding; fp32 within the reference's own fp32-fp64 spread)."""
    g = tf.golden()
    batch = tf.batch('c1')
    p64 = {k: v.double() for k, v in tf.params().items()}
    pred, loss = shared_window_form(torch.from_numpy(g['c1_spec_f64']), p64, batch['frame'].double())
    assert pred.shape == g['c1_frame_f64'].shape
    assert np.abs(pred.numpy() - g['c1_frame_f64']).max() < 1e-12
    assert abs(loss.item() - float(g['c1_loss_f64'])) < 1e-12
    pred32, loss32 = shared_window_form(torch.from_numpy(g['c1_spec_f32']), tf.params(), batch['frame'])
    spread = np.abs(g['c1_frame_f32'].astype(np.float64) - g['c1_frame_f64']).max()
    assert np.abs(pred32.numpy().astype(np.float64) - g['c1_frame_f32']).max() <= max(2 * spread, 1e-6)
    stats = g['c1_stats']
    assert 0.3 < stats[0] < 0.7 and 0.3 < stats[1] < 0.7 and stats[4] > 1e-3 and stats[5] < 1 - 1e-3       # not saturated, half active
    assert stats[6] < 1e-3 and stats[7] < 1e-3                                                             # fp32 ReLU flips below 0.1 %
