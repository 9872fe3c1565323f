"""Closed-form inputs of the Thickstun goldens, shared by tests/golden/make_golden_thickstun.py and the two test files.

Weights are ``oracle.fixture.hashed`` uniforms (zero mean, so about half of every pre-activation is positive); the scales keep the
activations of order one through the three layers and the logits of order one, so the sigmoid outputs are not saturated (the measured
fractions and the output range are recorded in the golden, keys ``*_stats``)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import fixture as fx  # noqa: E402

SHAPES = (('CNN_freq.weight', (128, 1, 128, 1)), ('CNN_freq.bias', (128,)), ('CNN_time.weight', (4096, 128, 1, 25)),
          ('CNN_time.bias', (4096,)), ('linear.weight', (88, 4096 * 51)))
# uniform half-widths: sqrt(3 / fan_in) is unit gain; the ReLUs halve the power, hence the factors above one
SCALES = {'CNN_freq.weight': 0.30, 'CNN_freq.bias': 0.05, 'CNN_time.weight': 0.045, 'CNN_time.bias': 0.05, 'linear.weight': 0.008}
SAMPLE = 997               # stride of the stored samples of the two large gradients / parameters
CASES = {'c1': (2, 16), 'c2': (1, 640)}          # case -> (clips, frames); audio is frames * 512 samples


def params():
    return {k: fx.hashed('thickstun.' + k, shape, SCALES[k]) for k, shape in SHAPES}


def batch(case):
    b, t = CASES[case]
    onset, frame = fx.fixture_labels(b, t, 'thick_' + case)
    return {'audio': fx.fixture_audio(b, t * 512, 'thick_' + case), 'onset': onset, 'frame': frame}


def golden():
    """The four golden files as one dict."""
    import numpy as np
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    out = {}
    for name in ('c1', 'c1_step', 'c2', 'c2_grad'):
        with np.load(os.path.join(here, f'thickstun_{name}.npz')) as g:
            out.update({k: g[k] for k in g.files})
    return out
