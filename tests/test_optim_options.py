"""CPU checks of the optimiser options of the fused step: the three config keys are off by default in every
training script's config scope, FlatAdam validates its arguments before it asks for a HIP device, and the header and the ctypes
table agree on the two new entry points."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = {'weight_decay': 0.0, 'ema_decay': 0.0, 'clip_before_step': False}


def test_keys_default_to_off_in_all_four_config_scopes():
    from reconvat_amd import cli
    scopes = [cli.base_config({}, True), cli.base_config({}, False), cli.baseline_config({}), cli.thickstun_config({})]
    for c in scopes:
        for k, v in OFF.items():
            assert k in c and c[k] == v and type(c[k]) is type(v), (k, c.get(k))
        assert c['fused_optimizer'] is True and c['clip_gradient_norm'] == 3
    c = cli.base_config({'ema_decay': 0.9, 'weight_decay': 0.01, 'clip_before_step': True}, True)
    assert (c['ema_decay'], c['weight_decay'], c['clip_before_step']) == (0.9, 0.01, True)


@pytest.mark.parametrize('script', ['train_UNet_Onset_VAT.py', 'train_UNet_VAT.py', 'train_baseline_onset_frame_VAT.py',
                                    'train_baseline_Thickstun.py'])
def test_scripts_hand_the_keys_to_run_training(script):
    """The entry points inject config entries by parameter name: a key missing from `train(...)` would never reach run_training."""
    src = open(os.path.join(ROOT, script)).read()
    sig = re.search(r'def train\((.*?)\):', src, flags=re.S).group(1)
    names = {a.strip() for a in sig.split(',')}
    assert set(OFF) <= names, set(OFF) - names


@pytest.mark.parametrize('kw', [{'weight_decay': -0.01}, {'max_grad_norm': -1.0}, {'ema_decay': -0.5}, {'ema_decay': 1.0},
                                {'ema_decay': 1.5}])
def test_flat_adam_rejects_bad_options(kw):
    from reconvat_amd.train import FlatAdam
    p = [torch.nn.Parameter(torch.zeros(3))]                   # a CPU parameter: the argument check comes first
    with pytest.raises(ValueError):
        FlatAdam(p, **kw)


def test_flat_adam_valid_options_reach_the_device_check():
    from reconvat_amd.train import FlatAdam
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(RuntimeError, match='HIP device only'):
        FlatAdam(p, weight_decay=0.01, max_grad_norm=3.0, ema_decay=0.999)


def test_torch_optimizer_path_refuses_the_options():
    """fused_optimizer=False with any of the three set: one sentence, before anything else is looked at."""
    from reconvat_amd import cli
    for kw in ({'ema_decay': 0.9}, {'weight_decay': 0.01}, {'clip_before_step': True}):
        c = cli.base_config(dict(kw, fused_optimizer=False, logdir='unused'), True)
        with pytest.raises(SystemExit, match='need fused_optimizer=True'):
            cli.run_training(True, **c)


def test_header_and_ctypes_agree_on_the_new_prototypes():
    from reconvat_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    ctype = {'float': _lib.F, 'long': _lib.L, 'int': _lib.I}
    for name in ('rv_adamw_step', 'rv_swap_floats'):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', text, flags=re.S)
        assert m, name + ' is not declared in include/reconvat_hip.h'
        want = []
        for arg in m.group(1).split(','):
            arg = arg.strip()
            want.append(_lib.P if '*' in arg else ctype[arg.replace('const ', '').split()[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.I and args == want, name
    # the new call is rv_adam_step's argument list plus (weight_decay, max_grad_norm, total_norm, ema, ema_decay) before the stream
    old, new = _lib.SIGNATURES['rv_adam_step'][1], _lib.SIGNATURES['rv_adamw_step'][1]
    assert new == old[:-1] + [_lib.F, _lib.F, _lib.P, _lib.P, _lib.F] + old[-1:]
