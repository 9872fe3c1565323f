"""The launches of one training step's run_on_batch + backward -- every library entry point in host order, with the chain (main or side
stream) it went to -- for the three models with a multi-stream schedule, single- and multi-stream.  tests/step_launches.txt holds
what the commit before the step-plan refactoring launched; Python-layer changes must reproduce it, and a kernel change that alters the
schedule on purpose regenerates the file in its own diff (the command is in the file's header)."""
import collections
import hashlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, 'step_launches.txt')
CONFIGS = [(model, dual) for model in ('onset', 'frame', 'onf') for dual in (False, True)]
HEADER = """# Launches of one run_on_batch(labelled, unlabelled, VAT=True) + backward at the B = 2, T = 64 fixtures (tests/test_step_launches_gpu.py).
# Regenerate on an MI355X, from the repository root:    python tests/test_step_launches_gpu.py > tests/step_launches.txt
# <model> <streams>: sha256 of the ordered "name stream" lines, then the launch count of every entry point
"""


def measure(model, dual, dev):
    """(digest of the ordered (entry point, main / side<i>) sequence, {entry point: launches})."""
    import test_model_gpu as tm
    import test_onset_frames as to
    from oracle import fixture as fx
    from reconvat_amd import _lib, ops
    if model == 'onf':
        m = to.build(dev, True)
        bl, bul = ({k: v.to(dev) for k, v in to._batch(2, 64, tag).items()} for tag in ('L', 'UL'))
        noise = [fx.fixture_noise((2, 64, 229), t).to(dev) for t in ('onf_d0_ul', 'onf_d0_l')]
    else:
        m = tm.build(model, True, dev)
        bl, bul = tm._batches(dev)
        noise = [fx.fixture_noise((2, 1, 64, 229), t).to(dev) for t in ('d0_ul', 'd0_l')]
    m.vat_loss.noise = lambda t: noise.pop(0).clone()
    main = torch.cuda.current_stream().cuda_stream
    sides = {ops.side_stream(dev, i).cuda_stream: f'side{i}' for i in range(2)}
    seq = []

    def hook(name, args, fn):
        s = torch.cuda.current_stream().cuda_stream
        seq.append(f"{name} {'main' if s == main else sides[s]}")
        return fn(*args)
    ops.DUAL_STREAM[0], _lib.HOOK[0] = dual, hook
    try:
        _, losses, _ = m.run_on_batch(bl, bul, True)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        ops.DUAL_STREAM[0], _lib.HOOK[0] = False, None
    return hashlib.sha256('\n'.join(seq).encode()).hexdigest(), dict(collections.Counter(s.split()[0] for s in seq))


def recorded():
    out = {}
    with open(DATA) as fh:
        for line in fh:
            if line.strip() and not line.startswith('#'):
                model, streams, digest, *counts = line.split()
                out[(model, streams == 'multi')] = (digest, {c.split('=')[0]: int(c.split('=')[1]) for c in counts})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('model,dual', CONFIGS)
def test_launches_are_those_recorded(dev, model, dual):
    want_digest, want_counts = recorded()[(model, dual)]
    digest, counts = measure(model, dual, dev)
    assert counts == want_counts
    assert digest == want_digest


if __name__ == '__main__':
    # (an argument names another checkout's root, whose reconvat_amd package is measured instead of this one's)
    sys.path[:0] = [os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(HERE), HERE]
    import reconvat_amd  # noqa: F401 -- before conftest puts this checkout's root in front
    sys.stdout.write(HEADER)
    for model, dual in CONFIGS:
        digest, counts = measure(model, dual, torch.device('cuda:0'))
        print(model, 'multi' if dual else 'single', digest, *(f'{k}={v}' for k, v in sorted(counts.items())))
