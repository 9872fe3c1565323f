"""Acoustic augmentation on the device (rv_fir_items) against the float64 definition y[m] = sum_j h[j] x[m + lead - j] +
noise[m] (`acoustics.apply_item` for the feed, np.convolve for the raw entry point).

Bound, derived and not measured: |y - y64| <= (W + 9) 2^-24 (S[m] + |noise[m]|), S[m] = sum_j |h[j]| |x[m + lead - j]| -- a length-W
float32 dot product in any order (W 2^-24 S to first order), the float32 rounding of the coefficients (2^-24 S), one rounding for the
final add (2^-24 (|sum| + |noise|)), and the rest of the 9 for the second-order terms.  No sample is excluded.  The integer case, the
identities and batch-independence are checked with ==.

Every raw call passes rows n + 37 apart: the gaps of x hold +-1e6 (a read that leaves its row is a million times any bound) and the
gaps of y a sentinel that must survive."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from reconvat_amd import acoustics
from reconvat_amd.acoustics import Acoustics
from reconvat_amd.constants import HOP_LENGTH
from test_pitch_shift_gpu import LENGTHS, NAMES, tracks, want

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = [(512, 80), (2048, 80), (1037, 272), (2048, 4160), (512, 4160), (300, 8256), (5000, 1040)]
LEADS = [0, 31]
B, GAP, SENTINEL = 3, 37, -12345.5
U = 2.0 ** -24


def fir(x, h, lead, seeds=None, amps=None):
    """rv_fir_items on x [b, n], h [b, W] (float32 numpy) through rows n + GAP apart; returns y [b, n] after checking y's gaps."""
    from reconvat_amd import _lib
    from reconvat_amd._lib import ptr
    dev = torch.device('cuda:0')
    b, n = x.shape
    W = h.shape[1]
    xb = np.empty((b, n + GAP), dtype=np.float32)
    xb[:, :n] = x
    xb[:, n:] = np.where(np.arange(GAP) % 2, 1e6, -1e6)
    # the first row is preceded by a loud margin too (leads < W reach before the row)
    xd = torch.from_numpy(np.concatenate([np.full(64, 1e6, dtype=np.float32), xb.reshape(-1)])).to(dev)
    yd = torch.full((b, n + GAP), SENTINEL, device=dev, dtype=torch.float32)
    hd = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev)
    sd = None if seeds is None else torch.from_numpy(np.asarray(seeds, dtype=np.uint32).view(np.int32)).to(dev)
    ad = None if amps is None else torch.from_numpy(np.asarray(amps, dtype=np.float32)).to(dev)
    rc = _lib.load().rv_fir_items(ptr(xd) + 256, n + GAP, ptr(hd), W, lead, ptr(sd), ptr(ad), b, n, ptr(yd), n + GAP, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    y = yd.cpu().numpy()
    assert np.all(y[:, n:] == SENTINEL), 'a store left its row'
    return y[:, :n].copy()


def conv64(x, h, lead):
    """The definition without the noise, in float64 (int64 for integer inputs): row by row."""
    n = x.shape[1]
    return np.stack([np.convolve(xr, hr)[lead:lead + n] for xr, hr in zip(x, h)])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def realistic(W, b, seed):
    """b parameter sets with every part the tap count allows switched on, and their filters (float64 [b, W])."""
    taps = W - 64
    a = Acoustics(rt60=0.5 if taps >= 256 else 0.0, eq_db=9.0, noise_db=-30.0, taps=taps)
    rs = np.random.RandomState(seed)
    params = [acoustics.draw(rs, a) for _ in range(b)]
    return params, np.stack([acoustics.item_filter(p)[0] for p in params])


def check_bound(y, x, h64, lead, params, tag):
    n, W = x.shape[1], h64.shape[1]
    worst = 0.0
    for i, p in enumerate(params):
        nz = acoustics.noise(p['seed'], n, p['amp']).astype(np.float64)
        y64 = np.convolve(x[i].astype(np.float64), h64[i])[lead:lead + n] + nz
        S = np.convolve(np.abs(x[i]).astype(np.float64), np.abs(h64[i]))[lead:lead + n]
        bound = (W + 9) * U * (S + np.abs(nz))
        err = np.abs(y[i].astype(np.float64) - y64)
        ratio = np.max(err / np.maximum(bound, 1e-300))
        worst = max(worst, ratio)
        assert np.all(err <= bound), (tag, i, int(np.argmax(err - bound)), ratio)
    print(f'{tag}: worst |y - y64| / bound {worst:.4f}')


@pytest.mark.parametrize('lead', LEADS)
@pytest.mark.parametrize('n,W', REGIMES)
def test_integer_inputs_are_exact(dev, n, W, lead):
    """x in [-8, 8], h in [-4, 4]: every partial sum is an integer below 2^24 (8256 * 32 < 2^19), so any summation order gives the
    integer convolution exactly -- one missing, doubled or misplaced tap changes it."""
    rs = np.random.RandomState(1000 * W + n + lead)
    x = rs.randint(-8, 9, (B, n))
    h = rs.randint(-4, 5, (B, W))
    h[:, 0], h[:, W - 1] = 3, -4                                                    # the two end taps are never zero
    y = fir(x.astype(np.float32), h.astype(np.float32), lead)
    assert np.array_equal(y.astype(np.int64), conv64(x, h, lead)) and np.array_equal(y, np.rint(y))


@pytest.mark.parametrize('lead', LEADS)
@pytest.mark.parametrize('n,W', REGIMES)
def test_realistic_filters_stay_within_the_bound(dev, n, W, lead):
    params, h64 = realistic(W, B, 7 * W + n)
    x = np.random.RandomState(n + W).uniform(-1, 1, (B, n)).astype(np.float32)
    y = fir(x, h64.astype(np.float32), lead, [p['seed'] for p in params], [p['amp'] for p in params])
    check_bound(y, x, h64, lead, params, f'n {n} W {W} lead {lead}')
    assert all(p['amp'] > 0 for p in params)


@pytest.mark.parametrize('lead', LEADS)
@pytest.mark.parametrize('n,W', REGIMES)
def test_identities(dev, n, W, lead):
    rs = np.random.RandomState(n * 31 + W)
    x = rs.uniform(-1, 1, (B, n)).astype(np.float32)
    h = np.zeros((B, W), dtype=np.float32)
    h[:, lead] = 1.0
    assert np.array_equal(bits(fir(x, h, lead)), bits(x))                           # the unit impulse at `lead`, no noise: y == x
    seeds, amps = rs.randint(0, 2 ** 31, B), rs.uniform(1e-4, 1e-2, B).astype(np.float32)
    hr = rs.uniform(-1, 1, (B, W)).astype(np.float32)
    y = fir(np.zeros((B, n), dtype=np.float32), hr, lead, seeds, amps)              # silence: y == noise
    for i in range(B):
        assert np.array_equal(bits(y[i]), bits(acoustics.noise(int(seeds[i]), n, amps[i]))), i


@pytest.mark.parametrize('n,W', REGIMES)
def test_items_do_not_depend_on_the_batch(dev, n, W):
    lead = 31
    params, h64 = realistic(W, B, 5 * W + n)
    h = h64.astype(np.float32)
    rs = np.random.RandomState(n)
    x = rs.uniform(-1, 1, (B, n)).astype(np.float32)
    x[1] *= np.float32(1e-4)                                                        # a quiet item between two full-scale ones
    seeds, amps = [p['seed'] for p in params], np.array([p['amp'] for p in params], dtype=np.float32)
    amps[1] *= np.float32(1e-4)
    quiet = [dict(p, amp=a) for p, a in zip(params, amps)]
    y = fir(x, h, lead, seeds, amps)
    check_bound(y, x, h64, lead, quiet, f'n {n} W {W} quiet item in the middle')
    assert np.abs(y[1]).max() < 1e-2
    assert np.array_equal(bits(fir(x, h, lead, seeds, amps)), bits(y))              # a second run
    order = [2, 0, 1]
    moved = fir(x[order], h[order], lead, [seeds[i] for i in order], amps[order])    # a batch of three, every item at another place
    assert np.array_equal(bits(moved), bits(y[order]))
    for i in range(B):
        alone = fir(x[i:i + 1], h[i:i + 1], lead, seeds[i:i + 1], amps[i:i + 1])
        assert np.array_equal(bits(alone[0]), bits(y[i])), i


def test_bad_arguments_are_refused(dev):
    from reconvat_amd import _lib
    from reconvat_amd._lib import ptr
    lib = _lib.load()
    n, W = 512, 80
    x = torch.zeros(2, n + 8, device=dev)
    y = torch.zeros(2, n + 8, device=dev)
    h = torch.zeros(2 * W + 4, device=dev)
    seed = torch.zeros(2, device=dev, dtype=torch.int32)
    amp = torch.zeros(2, device=dev)
    good = [ptr(x), n + 8, ptr(h), W, 31, ptr(seed), ptr(amp), 2, n, ptr(y), n + 8, None]
    assert lib.rv_fir_items(*good) == 0
    quiet = list(good)
    quiet[5] = quiet[6] = None
    assert lib.rv_fir_items(*quiet) == 0
    torch.cuda.synchronize()
    bad = [(3, 0), (3, 8), (3, 72), (3, 8272), (3, -16), (4, -1), (4, W), (8, 0), (8, -5), (8, 2 ** 31), (1, n - 1), (10, n - 1), (7, 0), (7, -2),
           (0, None), (2, None), (9, None), (2, ptr(h) + 4), (5, None), (6, None)]
    for at, value in bad:
        args = list(good)
        args[at] = value
        if (at, value) == (8, 2 ** 31):
            args[1] = args[10] = 2 ** 31 + 8                                         # the strides are not what is wrong here
        assert lib.rv_fir_items(*args) == -1, (at, value)
        assert 'rv_fir_items' in _lib.last_error(), (at, value)


# ---- the feed --------------------------------------------------------------------------------------------------------------------
ROOM = dict(rt60=0.3, eq_db=6.0, noise_db=-50.0, taps=1024)


def feed_corpus(seq, batch, pitch_shift, on=True):
    from reconvat_amd.feed import DeviceCorpus
    return DeviceCorpus(tracks(), seq, batch, torch.device('cuda:0'), seed=42, pitch_shift=pitch_shift, aug_seed=5,
                        acoustics=Acoustics(**ROOM) if on else None, acoustics_seed=77)


@pytest.mark.parametrize('pitch_shift', [0, 6])
@pytest.mark.parametrize('seq', [2048, 512])
def test_feed_items_stay_within_the_bound(dev, seq, pitch_shift):
    """Explicit parameters.  The device filters its own float32 crop x32; the yardstick filters the yardstick crop x64.  Unshifted,
    x32 == x64 (int16 2^-15 is exact).  Shifted, |x32 - x64| <= e = (K + 8) 2^-24 S_shift sample by sample (the bound of
    test_pitch_shift_gpu.py), so with E[m] = sum_j |h[j]| e[m + lead - j]:
        |y - y64| <= |fir32(x32) - fir64(x32)| + |fir64(x32 - x64)| <= (W + 9) 2^-24 (S64[m] + E[m] + |noise[m]|) + E[m],
    since sum |h| |x32| <= S64 + E."""
    a = Acoustics(**ROOM)
    dc, plain = feed_corpus(seq, 3, pitch_shift), feed_corpus(seq, 3, pitch_shift, on=False)
    rs = np.random.RandomState(seq + pitch_shift)
    items = [(0, 37, pitch_shift), (2, 0, -pitch_shift), (4, 0, pitch_shift // 2)]
    params = [acoustics.draw(rs, a) for _ in items]
    idx, rows, ks = [i for i, _, _ in items], [j for _, j, _ in items], [k for _, _, k in items]
    out = dc.crop(idx, rows, ks if pitch_shift else None, params)
    ref = plain.crop(idx, rows, ks if pitch_shift else None)
    assert out['acoustics'] is not None and len(out['acoustics']) == 3 and 'acoustics' not in ref
    for name in NAMES[1:]:
        assert torch.equal(out[name], ref[name]), name
    assert torch.equal(out['shift'], ref['shift']) and torch.equal(out['start_idx'], ref['start_idx']) and out['path'] == ref['path']
    y = out['audio'].cpu().numpy().astype(np.float64)
    assert y.shape == (3, seq)
    for b, (i, j0, k) in enumerate(items):
        w = want(i, j0, k, seq)
        y64 = acoustics.apply_item(w['audio'], params[b])
        S = acoustics.apply_item(w['audio'], params[b], magnitude=True)
        e = np.zeros(seq) if k == 0 else (w['K'] + 8) * U * w['S']
        E = acoustics.apply_item(e, params[b], magnitude=True)
        nz = np.abs(acoustics.noise(params[b]['seed'], seq, params[b]['amp'])).astype(np.float64)
        bound = (a.width + 9) * U * (S + E + nz) + E
        err = np.abs(y[b] - y64)
        print(f'seq {seq} p {pitch_shift} item {b} (k {k:+d}): worst |y - y64| / bound {np.max(err / bound):.4f}')
        assert np.all(err <= bound), (b, int(np.argmax(err - bound)))
        assert np.abs(y[b] - w['audio']).max() > 1e-4                               # and it is not the dry crop
    with pytest.raises(ValueError, match='acoustic parameters need'):
        plain.crop(idx, rows, ks if pitch_shift else None, params)
    with pytest.raises(ValueError, match='taps'):
        dc.crop(idx, rows, ks if pitch_shift else None, [dict(p, taps=512) for p in params])
    with pytest.raises(ValueError, match='one set'):
        dc.crop(idx, rows, ks if pitch_shift else None, params[:2])


@pytest.mark.parametrize('pitch_shift', [0, 6])
def test_drawn_batches_leave_the_other_streams_alone(dev, pitch_shift):
    """batch(): the parameters are acoustics.draw's for the same seed, and start_idx, shift and the labels are those of the same
    corpus without acoustics."""
    seq, order = 2048, [4, 0, 2, 2]
    a = Acoustics(**ROOM)
    dc, plain = feed_corpus(seq, 4, pitch_shift), feed_corpus(seq, 4, pitch_shift, on=False)
    rs = np.random.RandomState(77)
    for _ in range(3):
        out, ref = dc.batch(order), plain.batch(order)
        assert torch.equal(out['start_idx'], ref['start_idx']) and torch.equal(out['shift'], ref['shift'])
        for name in NAMES[1:]:
            assert torch.equal(out[name], ref[name]), name
        assert not torch.equal(out['audio'], ref['audio']) and bool(torch.isfinite(out['audio']).all())
        for p in out['acoustics']:
            d = acoustics.draw(rs, a)
            assert set(p) == set(d)
            for key in d:
                assert np.array_equal(p[key], d[key]), key
        # the batch is what crop() gives for those parameters
        again = dc.crop(order, (ref['start_idx'] // HOP_LENGTH).numpy(), ref['shift'].numpy() if pitch_shift else None, out['acoustics'])
        assert torch.equal(again['audio'], out['audio'])


def test_acoustics_off_is_the_feed_as_it_was(dev):
    """DeviceCorpus(), DeviceCorpus(acoustics=None) and an Acoustics() with nothing on draw and crop what the host item rule gives."""
    from reconvat_amd.dataset import crop_item
    from reconvat_amd.feed import DeviceCorpus
    seq, order = 2048, [4, 0, 3, 3, 1]
    outs = [DeviceCorpus(tracks(), seq, 5, dev, seed=42, **kw).batch(order)
            for kw in ({}, {'acoustics': None, 'acoustics_seed': 9}, {'acoustics': Acoustics(taps=512), 'acoustics_seed': 3})]
    rs = np.random.RandomState(42)
    for b, idx in enumerate(order):
        t = tracks()[idx]
        step = int(rs.randint(len(t['audio']) - seq)) // HOP_LENGTH
        item = crop_item({k: (torch.from_numpy(v) if k != 'path' else v) for k, v in t.items()}, step, seq)
        for out in outs:
            assert int(out['start_idx'][b]) == step * HOP_LENGTH and int(out['shift'][b]) == 0 and 'acoustics' not in out
            for n in NAMES:
                assert torch.equal(out[n][b].cpu(), item[n]), (b, n)
    with pytest.raises(ValueError, match='Acoustics'):
        DeviceCorpus(tracks(), seq, 5, dev, acoustics={'rt60': 0.3})
    assert LENGTHS[order[0]] == len(tracks()[order[0]]['audio'])


def test_command_line_run_with_acoustics(dev, tmp_path):
    """`train_UNet_VAT.py with ... reverb_rt60=0.3 eq_db=6 noise_db=-50 reverb_taps=1024`: two steps on the tiny synthetic corpus."""
    logdir = str(tmp_path / 'room')
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'train_UNet_VAT.py'), 'with', 'train_on=Synthetic', 'small=True', 'supersmall=True',
                        'sequence_length=32768', 'batch_size=2', 'train_batch_size=2', 'iteration=2', 'epoches=1', 'reverb_rt60=0.3',
                        'eq_db=6', 'noise_db=-50', 'reverb_taps=1024', f'logdir={logdir}'], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + '\n---\n' + p.stderr[-3000:]
    assert 'Training finished.' in p.stdout
    assert ('Acoustic augmentation: every training item in a room of RT60 in [0.075, 0.3] s (1024 taps), equalised by up to +-6 dB, '
            'noise floor in [-70, -50] dBFS') in p.stdout
    with open(os.path.join(logdir, 'scalars.jsonl')) as fh:
        rows = [json.loads(line) for line in fh]
    losses = [r['value'] for r in rows if r['tag'].startswith('loss/train_')]
    assert len(losses) >= 3 and np.all(np.isfinite(losses)), losses
    from reconvat_amd import cli
    c = cli.base_config(dict(device_feed=False, reverb_rt60=0.3, logdir='unused'), False)
    with pytest.raises(SystemExit, match='reverb_rt60, eq_db and noise_db are options of the device feed'):
        cli.run_training(False, **c)
