"""The velocity kernels (csrc/velocity.hip) against the float64 definition in reconvat_amd/velocity.py.

Bounds, derived and not measured.  u = 2^-24 is the relative cost of one rounding to float32, g(n) = n u / (1 - n u) the bound of a
float32 sum of n terms relative to the sum of their absolute values (any order; an fma chain of n terms has n roundings).  The
spectrogram and the parameters are float32 on both sides, so the inputs are exact.

rv_velocity_roll, per cell:
    x[32]      p / 88, one correctly rounded division: u of itself -- counted as a 34th term of the sum below
    z1[h]      b1 + sum of 33 products in one fma chain:                  dz1 = g(34) A1,   A1 = |b1[h]| + sum_i |w1[h][i] x[i]|
    sigmoid    s = 1 / (1 + e), e = expf(-z).  expf: 3 ulp (the OpenCL limit; the device library documents 1), an ulp at most 2 u
               of the value: 6 u of e, which moves s by s (1 - s) 6 u <= 1.5 u; the addition and the correctly rounded division u of
               s <= 1 each: 3.5 u, taken as eps = 4 u.  An e beyond the float32 range gives s = 0 where the exact s < 2^-126.
    a[h]       sigmoid is 1/4-Lipschitz:                                  da = dz1 / 4 + eps
    z2         b2 + 32 products:                                          dz2 = g(33) A2 + sum_h |w2[h]| da[h],   A2 = |b2| + sum_h |w2[h] a[h]|
    v                                                                     dv = dz2 / 4 + eps
rv_velocity_loss_grad evaluates the same forward, then, per masked cell (r = v - target, s'(z) = e / (1 + e)^2 with e = expf(-|z|)):
    s'(z)      e: 6 u; d = 1 + e: u and at most half of e's error; d d: twice that and u; the division u: below eps' = 16 u of
               s'; |d ln s' / dz| <= 1, so an error dz of its argument costs s' dz:       ds' = s' (dz + eps')
    d2         2 m r s'(z2): the subtraction and two products:            dd2 = 2 m (dv s'2 + |r| ds'2) + 3 u |d2|
    d2 a[h]                                                               |d2| da + a dd2 + u |d2 a|
    dz1[h]     (w2 s'(z1)) d2:                                            |w2 d2| ds'1 + |w2| s'1 dd2 + 2 u |dz1|
    terms      dz1[h] x[i] inside the fma (x[32]: u more), m r^2: 2 m |r| dv + 3 u m r^2
    sums       the cells of a workgroup in float32 (g(n), n = all masked cells: an upper bound), the workgroups in float64; sum m
               the same way; one float64 division and one rounding:      g(n) S + (g(n) + 2 u) |result|,   S = sum |terms| / sum m
    underflow  a float32 result below 2^-126 may be flushed to zero or rounded as a subnormal: an absolute f = 2^-126 in place of the
               relative u, carried through the factors that follow.  e of s' -> f of s'; d2: f (2 m |r| + 2); d2 a: f (|d2| + 1);
               dz1: f ((|w2| + 1) |d2| + 1); m r^2: 2 f; a sum of n terms n f, the division f.  (Saturated sigmoids get there:
               s'(z1) of an |z1| beyond 87 is below 2^-126 and w2 s'(z1) d2 is its multiple.)
Each entry's bound is the sum of its terms' errors over sum m plus that; nothing is excluded.  Two runs must agree bit for bit.

rv_eval_note_velocity states the arithmetic of decoding.note_velocities (float64 sum in ascending frames, one rounding): equal bits."""
import os
import sys

import numpy as np
import pytest
import torch

import velocity_cases as vc
from reconvat_amd import decoding as md
from reconvat_amd import velocity as V
from test_decoding import decoding_rolls
from test_note_cleanup_gpu import CLEANUPS, RULES
from test_velocity import CENTRES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
EPS, EPS_D = 4 * U, 16 * U
UF = 2.0 ** -126
GAP, SENTINEL = 37, -12345.5
SHAPES = [(2, 70, 'Mel'), (1, 3, 'Mel'), (1, 1, 'forty'), (3, 129, 'CQT84')]          # 229, 229, 40 (with -1 entries) and 84 bins
SCALES = [1.0, 8.0]


def gam(n):
    return n * U / (1 - n * U)


def inputs(B, T, kind, scale, seed=5):
    """float32 spectrogram and parameters (as float64 arrays holding float32 values), the table"""
    rs = np.random.RandomState([seed, B, T, int(scale)])
    centres = CENTRES[kind]()
    spec = rs.rand(B, T, len(centres)).astype(np.float32).astype(np.float64)
    params = (scale * rs.randn(V.N_PARAMS)).astype(np.float32).astype(np.float64)
    target = rs.rand(B, T, 88).astype(np.float32).astype(np.float64)
    return spec, V.harmonic_bins(centres), params, target


def forward_errors(x, params):
    """Per cell of x [n, 33]: the float64 forward and the error bounds of the docstring."""
    w1, b1, w2, b2 = V.unpack(params)
    z1 = x @ w1.T + b1
    dz1 = gam(34) * (np.abs(b1) + np.abs(x) @ np.abs(w1).T)
    a = 1 / (1 + np.exp(-z1))
    da = dz1 / 4 + EPS
    z2 = a @ w2 + b2
    dz2 = gam(33) * (np.abs(b2) + a @ np.abs(w2)) + da @ np.abs(w2)
    v = 1 / (1 + np.exp(-z2))
    return dict(z1=z1, dz1=dz1, a=a, da=da, z2=z2, dz2=dz2, v=v, dv=dz2 / 4 + EPS)


def dsig(z):
    e = np.exp(-np.abs(z))
    return e / (1 + e) ** 2


def loss_grad_bounds(spec, tab, params, target, mask):
    """(bound of the loss, bound of every gradient entry [1121]) as derived in the docstring."""
    b, t, p = np.nonzero(mask)
    if b.size == 0:
        return 0.0, np.zeros(V.N_PARAMS)
    x = V.masked_features_host(spec, tab, b, t, p)
    w1, b1, w2, b2 = V.unpack(params)
    f = forward_errors(x, params)
    m, r, n, total = mask[b, t, p], f['v'] - target[b, t, p], b.size, mask.sum()
    s1, s2 = dsig(f['z1']), dsig(f['z2'])
    ds1, ds2 = s1 * (f['dz1'] + EPS_D), s2 * (f['dz2'] + EPS_D)
    d2 = 2 * m * r * s2
    dd2 = 2 * m * (f['dv'] * s2 + np.abs(r) * ds2) + 3 * U * np.abs(d2) + UF * (2 * m * np.abs(r) + 2)
    e_terms, de = f['a'] * d2[:, None], np.abs(d2)[:, None] * f['da'] + f['a'] * dd2[:, None] + U * np.abs(f['a'] * d2[:, None]) + UF * (np.abs(d2)[:, None] + 1)
    dz = w2 * s1 * d2[:, None]
    ddz = np.abs(w2 * d2[:, None]) * ds1 + np.abs(w2) * s1 * dd2[:, None] + 2 * U * np.abs(dz) + UF * ((np.abs(w2) + 1) * np.abs(d2)[:, None] + 1)
    w_terms = dz[:, :, None] * x[:, None, :]                                         # [n, 32, 33]
    dw = ddz[:, :, None] * np.abs(x)[:, None, :] + U * np.abs(w_terms)
    l_terms = m * r * r
    dl = 2 * m * np.abs(r) * f['dv'] + 3 * U * l_terms + 2 * UF

    def entry(terms, dterms):
        s_abs = np.abs(terms).sum(axis=0) / total
        return dterms.sum(axis=0) / total + gam(n) * s_abs + (gam(n) + 2 * U) * np.abs(terms.sum(axis=0) / total) + (n / total + 1) * UF

    grad = np.concatenate([entry(w_terms, dw).reshape(-1), entry(dz, ddz), entry(e_terms, de), [entry(d2, dd2)]])
    return float(entry(l_terms, dl)), grad


def guarded(n, dev):
    buf = torch.full((n + 2 * GAP,), SENTINEL, device=dev, dtype=torch.float32)
    return buf, buf.data_ptr() + 4 * GAP


def check_guards(buf, n, written=True):
    out = buf.cpu().numpy()
    assert np.all(out[:GAP] == SENTINEL) and np.all(out[GAP + n:] == SENTINEL), 'a store left the output'
    if not written:
        assert np.all(out == SENTINEL), 'a refused call wrote'
    return out[GAP:GAP + n].copy()


def raw_roll(dev, spec, tab, params, B, T, n_bins, expect=0, spec_ptr=None, n_spec=None, n_out=None, n_params=None):
    from reconvat_amd import _lib
    d_spec = torch.from_numpy(spec.astype(np.float32)).to(dev)
    d_par = torch.from_numpy(params.astype(np.float32)).to(dev)
    tab = np.ascontiguousarray(tab, dtype=np.int32)
    n = B * T * 88
    buf, out_ptr = guarded(n, dev)
    rc = _lib.load().rv_velocity_roll(d_spec.data_ptr() if spec_ptr is None else spec_ptr(d_spec), d_spec.numel() if n_spec is None else n_spec,
                                      B, T, n_bins, tab.ctypes.data, d_par.data_ptr(), d_par.numel() if n_params is None else n_params,
                                      out_ptr, n if n_out is None else n_out, None)
    torch.cuda.synchronize()
    if expect != 0:
        assert rc == expect and 'rv_velocity_roll' in _lib.last_error(), (rc, _lib.last_error())
        check_guards(buf, n, written=False)
        return None
    assert rc == 0, _lib.last_error()
    return check_guards(buf, n).reshape(B, T, 88)


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('B,T,kind', SHAPES)
def test_roll_stays_within_the_bound(dev, B, T, kind, scale):
    spec, tab, params, _ = inputs(B, T, kind, scale)
    if kind != 'Mel':
        assert (tab == -1).any()
    got = raw_roll(dev, spec, tab, params, B, T, spec.shape[2])
    want = V.roll_host(spec, tab, params)
    b, t, p = np.nonzero(np.ones((B, T, 88)))
    bound = forward_errors(V.masked_features_host(spec, tab, b, t, p), params)['dv'].reshape(B, T, 88)
    err = np.abs(got.astype(np.float64) - want)
    print(f'({B}, {T}, {kind}) scale {scale}: worst |v - v64| / bound {np.max(err / bound):.4f}, worst bound {bound.max():.3e}')
    assert np.all(err <= bound), int(np.argmax(err - bound))
    # the wrapper and the module give the same bits
    from reconvat_amd import ops
    d_spec, d_par = torch.from_numpy(spec.astype(np.float32)).to(dev), torch.from_numpy(params.astype(np.float32)).to(dev)
    assert np.array_equal(ops.velocity_roll(d_spec, tab, d_par).cpu().numpy(), got)


def masks_for(B, T):
    rs = np.random.RandomState([B, T])
    out = {'empty': np.zeros((B, T, 88))}
    one = np.zeros((B, T, 88))
    one[B - 1, T // 2, 41] = 1
    out['one'] = one
    corners = np.zeros((B, T, 88))
    for t0 in range(0, T, 32):
        for t in (t0, min(t0 + 31, T - 1)):
            corners[:, t, 0] = corners[:, t, 87] = 1
    out['corners'] = corners
    if T <= 3:
        out['all'] = np.ones((B, T, 88))
    else:
        out['corpus'] = (rs.rand(B, T, 88) < 1e-3).astype(np.float64)
        assert out['corpus'].sum() >= 3
        out['weights'] = out['corpus'] * rs.choice([0.5, 1.0, 2.0], size=(B, T, 88))       # m is a weight, not only a flag
    return out


def run_loss_grad(dev, spec, tab, params, target, mask):
    from reconvat_amd import ops
    up = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    loss, grad = ops.velocity_loss_grad(up(spec), tab, up(params), up(target), up(mask))
    return loss.cpu().numpy().copy(), grad.cpu().numpy().copy()


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('B,T,kind', SHAPES)
def test_loss_and_gradient_stay_within_the_bound(dev, B, T, kind, scale):
    spec, tab, params, target = inputs(B, T, kind, scale)
    for name, mask in masks_for(B, T).items():
        loss, grad = run_loss_grad(dev, spec, tab, params, target, mask)
        again = run_loss_grad(dev, spec, tab, params, target, mask)
        assert loss.tobytes() == again[0].tobytes() and grad.tobytes() == again[1].tobytes(), name      # the same bits on every run
        want_loss, want_grad = V.loss_and_grad_host(spec, tab, params, target, mask)
        b_loss, b_grad = loss_grad_bounds(spec, tab, params, target, mask)
        if name == 'empty':
            assert loss == 0.0 and not grad.any()
            continue
        e_loss, e_grad = abs(float(loss) - want_loss), np.abs(grad.astype(np.float64) - want_grad)
        print(f'({B}, {T}, {kind}) scale {scale} {name}: {int((mask != 0).sum())} cells, loss err / bound {e_loss / b_loss:.4f}, '
              f'worst gradient err / bound {np.max(e_grad / b_grad):.4f}')
        assert e_loss <= b_loss, name
        assert np.all(e_grad <= b_grad), (name, int(np.argmax(e_grad - b_grad)))
        assert np.abs(want_grad).max() > 0


def test_autograd_wrapper(dev):
    spec, tab, params, target = inputs(2, 70, 'Mel', 1.0)
    mask = masks_for(2, 70)['corpus']
    loss, grad = run_loss_grad(dev, spec, tab, params, target, mask)
    head = V.VelocityHead('Mel', CENTRES['Mel']()).to(dev)
    with torch.no_grad():
        for dst, src in zip((head.w1, head.b1, head.w2, head.b2), V.unpack(torch.from_numpy(params.astype(np.float32)))):
            dst.copy_(src)
    up = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    out = V.velocity_loss(head, up(spec), up(target), up(mask))
    assert out.shape == () and out.detach().cpu().numpy().tobytes() == loss.tobytes()
    (3.0 * out).backward()                                                         # a non-unit grad_output
    got = torch.cat([head.w1.grad.reshape(-1), head.b1.grad, head.w2.grad, head.b2.grad.reshape(1)]).cpu().numpy()
    assert np.array_equal(got, 3.0 * grad)
    assert np.array_equal(head(up(spec)).cpu().numpy(), raw_roll(dev, spec, tab, params, 2, 70, 229))
    with pytest.raises(RuntimeError, match='HIP device only'):
        V.velocity_loss(head, up(spec).cpu(), up(target), up(mask))


def test_argument_checks(dev):
    from reconvat_amd import _lib, ops
    spec, tab, params, target = inputs(1, 3, 'Mel', 1.0)
    bad = tab.copy()
    bad[87, 7] = 229                                                               # one past the last bin
    raw_roll(dev, spec, bad, params, 1, 3, 229, expect=-1)
    bad[87, 7] = -2
    raw_roll(dev, spec, bad, params, 1, 3, 229, expect=-1)
    raw_roll(dev, spec, tab, params, 1, 3, 229, expect=-1, n_spec=3 * 229 - 1)     # short buffers
    raw_roll(dev, spec, tab, params, 1, 3, 229, expect=-1, n_out=3 * 88 - 1)
    raw_roll(dev, spec, tab, params, 1, 3, 229, expect=-1, n_params=1120)
    raw_roll(dev, spec, tab, params, 1, 3, 229, expect=-1, spec_ptr=lambda s: s.data_ptr() + 2)       # a misaligned pointer
    raw_roll(dev, spec, tab, params, 1, 3, 385, expect=-1)                         # more bins than the tile holds
    # the loss entry point: the same checks, and nothing written to loss or gradient
    lib = _lib.load()
    up = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dev)
    d_spec, d_par, d_t, d_m = up(spec), up(params), up(target), up(np.ones((1, 3, 88)))
    ws_bytes = lib.rv_velocity_workspace_bytes(1, 3)
    assert ws_bytes == 1124 * 4 and lib.rv_velocity_workspace_bytes(0, 3) == 0 and lib.rv_velocity_workspace_bytes(2, 70) == 2 * 3 * 1124 * 4
    ws = torch.empty(ws_bytes // 4, device=dev)
    tab32 = np.ascontiguousarray(tab, dtype=np.int32)

    def call(table=tab32, n_spec=d_spec.numel(), n_cells=264, n_grad=1121, ws_b=ws_bytes, spec_ptr=d_spec.data_ptr(), expect=-1):
        buf, out_ptr = guarded(1122, dev)
        rc = lib.rv_velocity_loss_grad(spec_ptr, n_spec, 1, 3, 229, table.ctypes.data, d_par.data_ptr(), 1121, d_t.data_ptr(), d_m.data_ptr(),
                                       n_cells, out_ptr, out_ptr + 4, n_grad, ws.data_ptr(), ws_b, None)
        torch.cuda.synchronize()
        assert rc == expect, (rc, _lib.last_error())
        if expect:
            assert 'rv_velocity_loss_grad' in _lib.last_error()
        return check_guards(buf, 1122, written=expect == 0)

    good = call(expect=0)
    loss, grad = ops.velocity_loss_grad(d_spec, tab, d_par, d_t, d_m)
    assert good[0] == float(loss) and np.array_equal(good[1:], grad.cpu().numpy())
    bad32 = tab32.copy()
    bad32[0, 0] = 229
    call(table=bad32)
    call(n_spec=3 * 229 - 1)
    call(n_cells=263)
    call(n_grad=1120)
    call(ws_b=ws_bytes - 4)
    call(spec_ptr=d_spec.data_ptr() + 2)
    # the note velocities: a short output buffer and a misaligned pointer
    on = torch.rand(10, 88, device=dev)
    notes = torch.tensor([[0, 5, 4]], dtype=torch.int32, device=dev)
    buf, out_ptr = guarded(1, dev)
    assert lib.rv_eval_note_velocity(on.data_ptr(), on.data_ptr(), 10, 0.5, notes.data_ptr(), 1, out_ptr, 0, None) == -1
    assert lib.rv_eval_note_velocity(on.data_ptr() + 2, on.data_ptr(), 10, 0.5, notes.data_ptr(), 1, out_ptr, 1, None) == -1
    assert lib.rv_eval_note_velocity(on.data_ptr(), on.data_ptr(), 0, 0.5, notes.data_ptr(), 1, out_ptr, 1, None) == -1
    torch.cuda.synchronize()
    check_guards(buf, 1, written=False)
    with pytest.raises(ValueError):
        ops.velocity_roll(d_spec, tab[:80], d_par)


@pytest.mark.parametrize('T', [70, 200])
def test_note_velocities_equal_the_host_twin(dev, T):
    from reconvat_amd import _lib
    checked = 0
    for seed in (0, 1):
        on, fr, vel = (torch.from_numpy(a) for a in decoding_rolls(seed, T=T))
        for thr in ((0.5, 0.5), (0.3, 0.6)):
            for rule in RULES:
                for m, g in CLEANUPS:
                    p, i, v = md.extract_notes_with_velocity(on, fr, vel, *thr, rule=rule, min_frames=m, bridge_gap=g)
                    if len(p) == 0:
                        continue
                    gp, gi, gv, painted = md.extract_notes_device(on.to(dev), fr.to(dev), vel.to(dev), *thr, rule=rule, min_frames=m, bridge_gap=g)
                    assert np.array_equal(gp, p) and np.array_equal(gi, i), (seed, thr, rule, m, g)
                    assert gv.dtype == np.float32 and gv.tobytes() == v.tobytes(), (seed, thr, rule, m, g)
                    p0, i0, painted0 = md.extract_notes_wo_velocity_device(on.to(dev), fr.to(dev), *thr, rule=rule, min_frames=m, bridge_gap=g)
                    assert np.array_equal(gp, p0) and np.array_equal(gi, i0) and torch.equal(painted, painted0)
                    checked += 1
    assert checked >= 2 * 2 * 2 * 3
    # no notes: nothing is launched, empty arrays come back
    z = torch.zeros(T, 88, device=dev)
    p, i, v, _ = md.extract_notes_device(z, z, z, 0.5, 0.5)
    assert len(p) == 0 and len(i) == 0 and v.shape == (0,) and v.dtype == np.float32
    assert _lib.load().rv_eval_note_velocity(None, None, T, 0.5, None, 0, None, 0, None) == 0
    # a note without an onset-active frame (a row handed in by hand) gives 0; a row that ends past the roll is cut at T
    on = torch.zeros(T, 88)
    on[3:6, 10] = 1
    vel = torch.rand(T, 88)
    rows = torch.tensor([[3, 10, 6], [8, 10, 12], [4, 10, T + 50]], dtype=torch.int32, device=dev)
    out = torch.empty(3, device=dev)
    assert _lib.load().rv_eval_note_velocity(on.to(dev).data_ptr(), vel.to(dev).data_ptr(), T, 0.5, rows.data_ptr(), 3, out.data_ptr(), 3, None) == 0
    want = md.note_velocities(on, vel, 0.5, [10, 10, 10], [[3, 6], [8, 12], [4, T + 50]])
    assert out.cpu().numpy().tobytes() == want.tobytes() and want[1] == 0 and want[0] > 0


@pytest.fixture(scope='module')
def onset_model(dev):
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel')
    m.load_state_dict(fx.fixture_params('onset', True))
    return m.to(dev).eval()


@pytest.fixture(scope='module')
def trained(dev, onset_model):
    """train_velocity's loop (velocity.fit) on the mini-corpus rendered on the device: (head, tracks, held-out error, constant error)"""
    tracks = vc.corpus(dev)
    batch = {'audio': torch.stack([a for a, _, _ in tracks[:vc.N_TRAIN]]), 'onset': torch.stack([m for _, m, _ in tracks[:vc.N_TRAIN]]),
             'velocity': torch.stack([v for _, _, v in tracks[:vc.N_TRAIN]])}
    torch.manual_seed(0)
    head = V.VelocityHead.for_model(onset_model, seed=0).to(dev)
    V.fit(head, onset_model, [batch], vc.STEPS, lr=vc.LR)
    with torch.no_grad():
        held = tracks[vc.N_TRAIN:]
        v_hat = head(V.front_end(onset_model, torch.stack([a for a, _, _ in held])))
    err, const = vc.errors(v_hat, torch.stack([m for _, m, _ in held]), torch.stack([v for _, _, v in held]), batch['onset'], batch['velocity'])
    return head, tracks, err, const


def test_training_run_learns_dynamics(trained):
    """The definition reaches a ratio of 0.633 on this corpus (tests/test_velocity.py); 0.85 leaves room for float32 ordering and the
    device renderer's 1-LSB freedom."""
    head, _, err, const = trained
    print(f'held-out error {err:.2f} / 128, constant {const:.2f} / 128, ratio {err / const:.3f}')
    assert err <= 0.85 * const
    assert head.spec == 'Mel' and all(torch.isfinite(p).all() for p in head.parameters())


def test_transcribe_files_with_and_without_a_head(dev, onset_model, trained, tmp_path):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    from reconvat_amd.evaluate import midi_to_hz
    from reconvat_amd.midi import parse_midi, save_midi
    head, tracks, _, _ = trained
    audio = tracks[-1][0]
    clip = tmp_path / 'clip.pt'
    torch.save({'audio': (audio.cpu() * 32768.0).round().clamp(-32768, 32767).to(torch.int16)}, str(clip))
    ckpt = tmp_path / 'velocity-1.pt'
    torch.save(head.state_dict(), str(ckpt))
    with torch.no_grad():
        pred = onset_model.transcribe({'audio': tf.load_audio(str(clip)).to(dev).unsqueeze(0)})
    onset, frame = pred['onset'].squeeze(0).relu(), pred['frame'].squeeze(0).relu()
    # the transcriber's weights are a fixture, not a trained model: thresholds from the posteriorgrams themselves, so that there are notes
    thr_on, thr_fr = float(onset.flatten().quantile(0.98)), float(frame.flatten().quantile(0.9))
    p_est, i_est, _ = md.extract_notes_wo_velocity_device(onset, frame, thr_on, thr_fr, rule='rule2')
    assert len(p_est) > 4
    hz = np.array([midi_to_hz(21 + q) for q in p_est])
    # without velocity=: the bytes of the code path as it was (every note at 127)
    tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / 'plain'), onset_threshold=thr_on, frame_threshold=thr_fr)
    save_midi(str(tmp_path / 'want.mid'), hz, np.asarray(i_est) * (512 / 16000), [127] * len(p_est))
    plain = open(tmp_path / 'plain' / 'ReconVAT-clip.mid', 'rb').read()
    assert plain == open(tmp_path / 'want.mid', 'rb').read()
    assert set(parse_midi(str(tmp_path / 'plain' / 'ReconVAT-clip.mid'))[:, 3]) == {127}
    # with it: the same notes, velocities of the head
    loaded = tf.load_head(str(ckpt), onset_model, dev)
    tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / 'dyn'), onset_threshold=thr_on, frame_threshold=thr_fr, head=loaded,
                       render=True)
    got, want = parse_midi(str(tmp_path / 'dyn' / 'ReconVAT-clip.mid')), parse_midi(str(tmp_path / 'plain' / 'ReconVAT-clip.mid'))
    assert got.shape == want.shape and np.array_equal(got[:, :3], want[:, :3])
    vel = got[:, 3]
    assert vel.min() >= 1 and vel.max() <= 127 and len(set(vel.tolist())) > 1
    with torch.no_grad():
        roll = loaded(V.front_end(onset_model, tf.load_audio(str(clip)).to(dev).unsqueeze(0))).squeeze(0)
    _, _, v_est, _ = md.extract_notes_device(onset, frame, roll, thr_on, thr_fr, rule='rule2')
    assert sorted(vel.tolist()) == sorted(V.midi_velocities(v_est).tolist())
    assert os.path.getsize(tmp_path / 'dyn' / 'ReconVAT-clip.wav') == 44 + 2 * len(audio)
    # a head of another front end is refused
    other = V.VelocityHead('CQT', CENTRES['CQT']())
    torch.save(other.state_dict(), str(tmp_path / 'cqt.pt'))
    with pytest.raises(ValueError, match='front end'):
        tf.load_head(str(tmp_path / 'cqt.pt'), onset_model, dev)


def as_track(audio, onset, velocity):
    """A corpus track (uint8 rolls) from one tuple of velocity_cases.corpus"""
    return {'label': (onset * 3).to(torch.uint8).cpu(), 'velocity': (velocity * 128).round().to(torch.uint8).cpu()}


def test_heldout_error_is_the_error_of_the_training_run(dev, onset_model, trained):
    head, tracks, err, const = trained
    constant = V.onset_velocity_mean([as_track(*t) for t in tracks[:vc.N_TRAIN]])
    on = torch.stack([m for _, m, _ in tracks[:vc.N_TRAIN]]) > 0
    assert abs(constant - float(torch.stack([v for _, _, v in tracks[:vc.N_TRAIN]])[on].double().mean())) < 1e-12
    items = [{'audio': a, 'onset': m, 'velocity': v} for a, m, v in tracks[vc.N_TRAIN:]]
    with torch.no_grad():
        got_err, got_const = V.heldout_error(head, onset_model, items, constant)
    assert abs(got_err - err) <= 1e-6 * err and abs(got_const - const) <= 1e-9 * const
    assert V.onset_velocity_mean([]) == 0.0


class LabelHead(V.VelocityHead):
    """A head that answers with a given roll: the labels' own velocities."""

    def forward(self, spec):
        assert spec.dim() == 3 and spec.shape[0] == 1 and spec.shape[1:] == (self.roll.shape[0], 229)
        return self.roll[None]


def test_evaluate_with_velocity(dev, onset_model, trained):
    from reconvat_amd import evaluate as ev
    from reconvat_amd.dataset import RenderedScores, crop_item
    data = RenderedScores(2, 256 * 512, ('struck', 'sustained'), seed=70, device=dev)
    songs = [crop_item(t, None, None, dev) for t in data.data]
    n_ref = [len(md.extract_notes_wo_velocity(s['onset'].cpu(), s['frame'].cpu(), rule='rule2')[0]) for s in songs]
    assert min(n_ref) > 5
    # 1. the trained head: evaluate_wo_velocity's dictionary plus the two new blocks, one value per song
    head = trained[0]
    with torch.no_grad():
        plain = ev.evaluate_wo_velocity(songs, onset_model, reconstruction=False, device_metrics=True)
        got = ev.evaluate_with_velocity(songs, onset_model, head, reconstruction=False)
    new = {f'metric/{tag}/{k}' for tag in ('note-with-velocity', 'note-with-offsets-and-velocity') for k in ('precision', 'recall', 'f1', 'overlap')}
    assert set(got) == set(plain) | new and not new & set(plain)
    for key in plain:
        assert got[key] == plain[key], key
    for key in new:
        assert len(got[key]) == len(songs) and all(0.0 <= v <= 1.0 for v in got[key]), key
    for a, b in (('note-with-velocity', 'note'), ('note-with-offsets-and-velocity', 'note-with-offsets')):      # survivors are a subset
        assert all(x <= y + 1e-12 for x, y in zip(got[f'metric/{a}/recall'], got[f'metric/{b}/recall']))
    # 2. velocities equal to the labels': every matched pair survives.  With the label onsets as the estimate's onsets and a frame threshold
    # no posteriorgram reaches, the estimate's notes are the label's onset frames, and each reads its own label velocity
    for song in songs:
        oracle = LabelHead.for_model(onset_model).to(dev)
        oracle.roll = song['velocity']
        with torch.no_grad():
            m = ev.evaluate_with_velocity([song], onset_model, oracle, frame_threshold=2.0, pseudo_onset=True, reconstruction=False)
        assert m['metric/note/f1'] == [1.0] and m['metric/note/precision'] == [1.0]
        for k in ('precision', 'recall', 'f1', 'overlap'):
            assert m[f'metric/note-with-velocity/{k}'] == m[f'metric/note/{k}'], k
            assert m[f'metric/note-with-offsets-and-velocity/{k}'] == m[f'metric/note-with-offsets/{k}'], k
        # ... and a head that is wrong about every second note loses those pairs: loud where the label is soft
        wrong = LabelHead.for_model(onset_model).to(dev)
        wrong.roll = torch.where((torch.arange(88, device=dev) % 2 == 0)[None, :], song['velocity'], 1.0 - song['velocity'])
        with torch.no_grad():
            w = ev.evaluate_with_velocity([song], onset_model, wrong, frame_threshold=2.0, pseudo_onset=True, reconstruction=False)
        assert w['metric/note/f1'] == [1.0] and w['metric/note-with-velocity/f1'][0] < 1.0
    # a head of another front end is refused before anything runs
    with pytest.raises(ValueError, match='front end'):
        ev.evaluate_with_velocity(songs, onset_model, V.VelocityHead('CQT', CENTRES['CQT']()).to(dev), reconstruction=False)


class CountingModel:
    """The model, counting its ``run_on_batch`` calls."""

    def __init__(self, model):
        self.model, self.calls = model, 0

    def __getattr__(self, name):
        return getattr(self.model, name)

    def run_on_batch(self, *args, **kwargs):
        self.calls += 1
        return self.model.run_on_batch(*args, **kwargs)


def test_evaluate_with_velocity_is_one_pass(dev, onset_model, trained):
    from reconvat_amd import NoteHMM, evaluate as ev
    from reconvat_amd.dataset import RenderedScores, crop_item
    data = RenderedScores(2, 256 * 512, ('struck', 'sustained'), seed=70, device=dev)
    songs = [crop_item(t, None, None, dev) for t in data.data]
    head, counting = trained[0], CountingModel(onset_model)
    with torch.no_grad():
        ev.evaluate_with_velocity(songs, counting, head, reconstruction=False)
        assert counting.calls == len(songs)                             # one forward per song for both halves of the dictionary
    # with a model both halves describe the notes of its Viterbi path.  At the default penalties this model's posteriorgrams decode to no
    # matching note (recall 0, printed); the second set switches for free, so that there are pairs for the velocity test to thin out
    recalls = []
    for h in (NoteHMM(), NoteHMM(note_on=0.0, note_off=0.0, restrike=0.0)):
        with torch.no_grad():
            got = ev.evaluate_with_velocity(songs, onset_model, head, reconstruction=False, hmm=h)
            plain = ev.evaluate_wo_velocity(songs, onset_model, reconstruction=False, hmm=h, device_metrics=True)
        for k in ('precision', 'recall', 'f1', 'overlap'):
            assert got[f'metric/note/{k}'] == plain[f'metric/note/{k}'] and len(got[f'metric/note/{k}']) == len(songs), (h, k)
        print(h, 'note recall:', plain['metric/note/recall'], ' with velocity:', got['metric/note-with-velocity/recall'])
        for a, b in (('note-with-velocity', 'note'), ('note-with-offsets-and-velocity', 'note-with-offsets')):      # survivors are a subset
            assert all(x <= y for x, y in zip(got[f'metric/{a}/recall'], got[f'metric/{b}/recall'])), (h, a)
        recalls.append(min(plain['metric/note/recall']))
    assert recalls[1] > 0
    # a head of another front end is refused before the model runs at all
    counting.calls = 0
    with pytest.raises(ValueError, match='front end'):
        ev.evaluate_with_velocity(songs, counting, V.VelocityHead('CQT', CENTRES['CQT']()).to(dev), reconstruction=False)
    assert counting.calls == 0
