"""The acoustic augmentation's definition (reconvat_amd/acoustics.py) against a restatement written from the text of
the definition alone: this file shares no code with the module.  tests/test_acoustics_gpu.py compares the device path with
`acoustics.apply_item`."""
import inspect
import math
import os
import re

import numpy as np
import pytest

from reconvat_amd import acoustics
from reconvat_amd.acoustics import Acoustics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def ref_draws(rs, R):
    return {'u': rs.uniform(0.25, 1.0), 'drr': rs.uniform(0.0, 12.0), 'n0': rs.randint(16, 161), 'w': rs.standard_normal(R),
            'g': rs.uniform(-1.0, 1.0, 5), 'un': rs.uniform(0.0, 1.0), 'seed': rs.randint(0, 2 ** 31)}


def ref_room(R, rt, drr, n0, w):
    room = [0.0] * R
    if rt > 0:
        t = [w[n] * 10.0 ** (-3.0 * (n - n0) / (rt * 16000.0)) if n >= n0 else 0.0 for n in range(R)]
        scale = math.sqrt(10.0 ** (-drr / 10.0) / math.fsum(v * v for v in t))
        room = [v * scale for v in t]
    room[0] += 1.0
    return np.array(room)


def ref_eq(eq_db, g):
    if eq_db == 0:
        return np.array([1.0 if j == 31 else 0.0 for j in range(63)])
    anchors = [0.0, 250.0, 1000.0, 4000.0, 8000.0]
    G = []
    for i in range(33):
        f = 250.0 * i
        k = max(q for q in range(4) if anchors[q] <= f)
        frac = (f - anchors[k]) / (anchors[k + 1] - anchors[k])
        G.append(10.0 ** ((eq_db * g[k] + frac * (eq_db * g[k + 1] - eq_db * g[k])) / 20.0))
    # the inverse real FFT of 33 real bins, length 64, spelled out
    e = [(G[0] + G[32] * (-1) ** n + 2.0 * math.fsum(G[k] * math.cos(2.0 * math.pi * k * n / 64.0) for k in range(1, 32))) / 64.0
         for n in range(64)]
    return np.array([e[(j - 31) % 64] * (0.5 - 0.5 * math.cos(2.0 * math.pi * j / 62.0)) for j in range(63)])


def ref_filter(R, rt, drr, n0, w, eq_db, g):
    room, eq = ref_room(R, rt, drr, n0, w), ref_eq(eq_db, g)
    h = np.zeros(R + 64)
    for j in range(63):
        h[j:j + R] += eq[j] * room
    return h


def ref_lowbias32(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    x ^= x >> 16
    return x


def ref_noise(seed, n, amp):
    out = np.empty(n, dtype=np.float32)
    for m in range(n):
        v = ref_lowbias32(seed ^ ref_lowbias32((m + 0x9E3779B9) & M32))
        out[m] = np.float32((v & 0xFFFF) + (v >> 16) - 65535) * np.float32(amp)
    return out


def rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


CASES = [dict(rt60=0.5, eq_db=6.0, noise_db=-50.0, taps=1024), dict(rt60=1.0, eq_db=12.0, noise_db=-20.0, taps=256),
         dict(rt60=0.05, eq_db=3.0, noise_db=-90.0, taps=4096), dict(rt60=0.3, taps=8192), dict(eq_db=9.0, taps=16)]


# ---- tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', CASES)
def test_filters_agree_with_the_restatement(kw):
    a = Acoustics(**kw)
    p = acoustics.draw(np.random.RandomState(7), a)
    d = ref_draws(np.random.RandomState(7), a.taps)
    rt = a.rt60 * d['u']
    assert rel(acoustics.room_filter(p), ref_room(a.taps, rt, d['drr'], d['n0'], d['w'])) <= 1e-12
    assert rel(acoustics.eq_filter(p), ref_eq(a.eq_db, d['g'])) <= 1e-12
    h, lead = acoustics.item_filter(p)
    assert lead == 31 and h.shape == (a.taps + 64,) and h.dtype == np.float64 and a.width == a.taps + 64
    assert rel(h, ref_filter(a.taps, rt, d['drr'], d['n0'], d['w'], a.eq_db, d['g'])) <= 1e-12
    assert h[-2] == 0 and h[-1] == 0


def test_noise_agrees_with_the_restatement():
    for seed, amp in ((0, 1.0), (12345, 3.7e-5), (2 ** 31 - 1, 0.25), (0xDEADBEEF, 1e-3)):
        got = acoustics.noise(seed, 3000, np.float32(amp))
        assert got.dtype == np.float32 and np.array_equal(got, ref_noise(seed, 3000, amp)), seed
    # the counter wraps in uint32: sample m = 2^32 - 0x9E3779B9 hashes counter 0
    v = ref_lowbias32(99 ^ ref_lowbias32(0))
    m = (1 << 32) - 0x9E3779B9
    assert ((m + 0x9E3779B9) & M32) == 0 and v == ref_lowbias32(99 ^ ref_lowbias32((m + 0x9E3779B9) & M32))


def test_parts_that_are_off():
    rs = np.random.RandomState(3)
    p = acoustics.draw(rs, Acoustics(noise_db=-40.0, taps=512))
    room, eq = acoustics.room_filter(p), acoustics.eq_filter(p)
    assert room[0] == 1.0 and not room[1:].any() and room.shape == (512,)
    assert eq[31] == 1.0 and not np.delete(eq, 31).any() and eq.shape == (63,)
    h, lead = acoustics.item_filter(p)
    assert h[31] == 1.0 and not np.delete(h, 31).any() and lead == 31
    assert p['amp'] > 0 and p['amp'].dtype == np.float32
    q = acoustics.draw(rs, Acoustics(rt60=0.2, taps=512))
    assert q['amp'] == 0 and q['amp'].dtype == np.float32
    assert not acoustics.noise(q['seed'], 100, q['amp']).any()
    eq = acoustics.eq_filter(q)
    assert eq[31] == 1.0 and not np.delete(eq, 31).any()
    assert Acoustics().off and Acoustics(taps=16).off
    assert not Acoustics(rt60=0.1).off and not Acoustics(eq_db=1).off and not Acoustics(noise_db=-60).off


def test_room_properties():
    a = Acoustics(rt60=0.4, taps=2048)
    rs = np.random.RandomState(11)
    for _ in range(4):
        p = acoustics.draw(rs, a)
        room = acoustics.room_filter(p)
        t = room.copy()
        t[0] -= 1.0
        assert abs(np.sum(t ** 2) / 10.0 ** (-p['drr'] / 10.0) - 1.0) <= 1e-12
        n0 = p['n0']
        assert 16 <= n0 <= 160 and not room[1:n0].any() and room[n0] != 0
        # |t| / |w| is the envelope up to one scale: log10 of it is a line of slope -3 / (rt 16000)
        n = np.arange(n0, 2048)
        logenv = np.log10(np.abs(t[n] / p['w'][n]))
        slope = -3.0 / (p['rt'] * 16000.0)
        assert np.abs(np.diff(logenv) - slope).max() <= 1e-9
        assert 0.25 * 0.4 <= p['rt'] <= 0.4


def test_eq_properties():
    a = Acoustics(eq_db=12.0, taps=16)
    p = acoustics.draw(np.random.RandomState(5), a)
    eq = acoustics.eq_filter(p)
    assert np.abs(eq - eq[::-1]).max() <= 1e-15 and eq[0] == 0 and eq[62] == 0
    for c in (-7.5, 0.0, 4.0):
        flat = dict(p, eq_db=1.0, g=np.full(5, c))
        want = np.zeros(63)
        want[31] = 10.0 ** (c / 20.0)
        assert np.abs(acoustics.eq_filter(flat) - want).max() <= 1e-12 * want[31]


def test_noise_statistics():
    n = 327680
    a = Acoustics(noise_db=-40.0, taps=16)
    rs = np.random.RandomState(1)
    p, q = acoustics.draw(rs, a), acoustics.draw(rs, a)
    for d in (p, q):
        sigma = 10.0 ** ((-40.0 - 20.0 * d['un']) / 20.0)
        assert d['amp'] == np.float32(sigma * math.sqrt(6.0) / 65536.0)
        x = acoustics.noise(d['seed'], n, d['amp']).astype(np.float64)
        print(f"sigma {sigma:.4e}: mean {x.mean():+.3e}, rms / sigma {np.sqrt(np.mean(x * x)) / sigma:.5f}")
        assert abs(x.mean()) < 1e-4 * sigma / 0.01
        assert abs(np.sqrt(np.mean(x * x)) / sigma - 1.0) < 0.01
    assert p['seed'] != q['seed']
    assert not np.array_equal(acoustics.noise(p['seed'], 4096, np.float32(1)), acoustics.noise(q['seed'], 4096, np.float32(1)))


def test_draws_come_in_order_whatever_is_on():
    R = 512
    ends = []
    for kw in ({'rt60': 0.3, 'eq_db': 4.0, 'noise_db': -30.0}, {'rt60': 0.3}, {'eq_db': 4.0}, {'noise_db': -30.0}, {}):
        a = Acoustics(taps=R, **kw)
        rs, ref = np.random.RandomState(21), np.random.RandomState(21)
        for _ in range(3):
            p, d = acoustics.draw(rs, a), ref_draws(ref, R)
            assert p['rt'] == a.rt60 * d['u'] and p['drr'] == d['drr'] and p['n0'] == d['n0'] and p['un'] == d['un']
            assert np.array_equal(p['w'], d['w']) and np.array_equal(p['g'], d['g']) and p['seed'] == d['seed']
            assert p['taps'] == R and p['eq_db'] == a.eq_db and 0 <= p['seed'] < 2 ** 31
        ends.append(rs.randint(0, 2 ** 31))
    assert len(set(ends)) == 1                                                      # the stream stands at the same place after an item


def test_apply_item_is_the_definition():
    a = Acoustics(rt60=0.2, eq_db=6.0, noise_db=-30.0, taps=256)
    p = acoustics.draw(np.random.RandomState(2), a)
    x = np.random.RandomState(3).uniform(-1, 1, 700)
    h, lead = acoustics.item_filter(p)
    nz = acoustics.noise(p['seed'], 700, p['amp']).astype(np.float64)
    y, S = acoustics.apply_item(x, p), acoustics.apply_item(x, p, magnitude=True)
    for m in (0, 1, 30, 31, 32, 350, 698, 699):
        j = np.arange(len(h))
        k = m + lead - j
        ok = (k >= 0) & (k < 700)
        assert abs(y[m] - (np.sum(h[j[ok]] * x[k[ok]]) + nz[m])) <= 1e-12
        assert abs(S[m] - np.sum(np.abs(h[j[ok]]) * np.abs(x[k[ok]]))) <= 1e-12
    assert y.shape == (700,) and y.dtype == np.float64


@pytest.mark.parametrize('kw', [dict(rt60=-0.1), dict(rt60=1.01), dict(rt60='0.3'), dict(eq_db=-1), dict(eq_db=12.5), dict(noise_db=-91),
                                dict(noise_db=-19.9), dict(noise_db='quiet'), dict(taps=0), dict(taps=8), dict(taps=100), dict(taps=8208),
                                dict(taps=1024.0), dict(rt60=0.2, taps=240), dict(rt60=float('nan')), dict(eq_db=float('nan')),
                                dict(noise_db=float('nan')), dict(rt60=True)])
def test_illegal_options_raise(kw):
    with pytest.raises(ValueError):
        Acoustics(**kw)


def test_legal_options_at_their_limits():
    Acoustics(rt60=1.0, eq_db=12, noise_db=-20, taps=8192)
    Acoustics(rt60=0.0, eq_db=0, noise_db=-90, taps=16)
    Acoustics(rt60=0.01, taps=256)


def test_config_default_override_and_refusal():
    from reconvat_amd import cli
    for c in (cli.base_config({}, True), cli.base_config({}, False), cli.baseline_config({}), cli.thickstun_config({})):
        assert (c['reverb_rt60'], c['eq_db'], c['noise_db'], c['reverb_taps']) == (0.0, 0.0, None, cli.FEED_OPTIONS['reverb_taps'])
        assert c['reverb_taps'] in (1024, 2048, 4096, 8192)
    assert inspect.signature(cli.run_training).parameters['reverb_taps'].default == cli.FEED_OPTIONS['reverb_taps']
    for key, value in (('reverb_rt60', 0.3), ('eq_db', 6), ('noise_db', -50)):
        for kw in ({'device_feed': False}, {'device': 'cpu'}):
            c = cli.base_config(dict(kw, logdir='unused', **{key: value}), True)
            with pytest.raises(SystemExit, match='reverb_rt60, eq_db and noise_db are options of the device feed'):
                cli.run_training(True, **c)
    c = cli.base_config(dict(reverb_rt60=2.0, logdir='unused'), True)
    with pytest.raises(SystemExit, match='rt60 must lie in'):
        cli.run_training(True, **c)


@pytest.mark.parametrize('script', ['train_UNet_Onset_VAT.py', 'train_UNet_VAT.py', 'train_baseline_onset_frame_VAT.py',
                                    'train_baseline_Thickstun.py'])
def test_scripts_hand_the_keys_to_run_training(script):
    src = open(os.path.join(ROOT, script)).read()
    sig = re.search(r'def train\((.*?)\):', src, flags=re.S).group(1)
    assert {'reverb_rt60', 'eq_db', 'noise_db', 'reverb_taps'} <= {a.strip() for a in sig.split(',')}


def test_header_and_ctypes_agree_on_the_entry_point():
    from reconvat_amd import _lib, build
    text = open(os.path.join(ROOT, 'include', 'reconvat_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\bint\s+rv_fir_items\s*\(([^;]*?)\)\s*;', text, flags=re.S)
    assert m, 'rv_fir_items is not declared in include/reconvat_hip.h'
    ctype = {'float': _lib.F, 'long': _lib.L, 'int': _lib.I}
    want = [_lib.P if '*' in a else ctype[a.replace('const ', '').split()[0]] for a in (x.strip() for x in m.group(1).split(','))]
    assert len(want) == 12 and _lib.SIGNATURES['rv_fir_items'] == (_lib.I, want)
    source = open(os.path.join(ROOT, 'reconvat_amd', 'csrc', 'acoustics.hip')).read()
    assert re.search(r'\bint\s+rv_fir_items\s*\(', source) and 'acoustics.hip' in build.SOURCES
