"""The velocity head's definition (reconvat_amd/velocity.py) on the CPU: the bin table, the hand-written gradient against
autograd, velocity decoding against the reference's golden, the note-with-velocity metric on hand-made cases, and that the head can
learn dynamics at all on the rendered mini-corpus (tests/velocity_cases.py)."""
import os

import numpy as np
import pytest
import torch

import velocity_cases as vc
from reconvat_amd import decoding as md
from reconvat_amd import evaluate as ev
from reconvat_amd import velocity as V
from test_decoding import decoding_rolls

G = os.path.join(os.path.dirname(__file__), 'golden')


def mel_centres():
    from reconvat_amd.frontend import slaney_mel_basis
    from reconvat_amd.constants import SAMPLE_RATE, WINDOW_LENGTH, N_BINS, MEL_FMIN, MEL_FMAX
    return V.mel_centres(slaney_mel_basis(SAMPLE_RATE, WINDOW_LENGTH, N_BINS, MEL_FMIN, MEL_FMAX))


CENTRES = {'Mel': mel_centres, 'CQT': lambda: V.cqt_centres(27.5, 24, 176), 'CQT84': lambda: V.cqt_centres(27.5, 12, 84),
           'forty': lambda: np.linspace(50.0, 2000.0, 40)}


@pytest.mark.parametrize('kind', sorted(CENTRES))
def test_bin_table(kind):
    centres = CENTRES[kind]()
    tab = V.harmonic_bins(centres)
    assert tab.shape == (88, 8) and tab.dtype == np.int32
    f0 = 440.0 * 2.0 ** ((np.arange(88) + 21 - 69) / 12.0)
    target = f0[:, None] * np.arange(1, 9)[None, :]
    assert np.array_equal(tab == -1, target > centres.max())                       # -1 exactly where stated
    assert tab[tab >= 0].max() < len(centres) and tab.min() >= -1
    for p in range(88):
        for k in range(8):
            if tab[p, k] >= 0:
                d = np.abs(centres - target[p, k])
                assert d[tab[p, k]] == d.min() and not (d[:tab[p, k]] == d.min()).any()        # nearest; the first of equals
    # monotone in k and in p where defined (the centres ascend)
    for a, b in ((tab[:, :-1], tab[:, 1:]), (tab[:-1], tab[1:])):
        both = (a >= 0) & (b >= 0)
        assert (a[both] <= b[both]).all()
    if kind in ('forty', 'CQT84'):
        assert (tab == -1).any() and (tab >= 0).any()
    if kind == 'Mel':
        assert (tab == -1).sum() == 112 and tab[0, 0] == 0


def test_bin_table_ties_go_to_the_lower_index():
    f0 = 27.5
    tab = V.harmonic_bins(np.array([f0 - 2.0, f0 + 2.0, 20000.0]))                 # key 0's fundamental lies exactly between bins 0 and 1
    assert tab[0, 0] == 0
    assert V.harmonic_bins(np.array([f0, f0, 20000.0]))[0, 0] == 0                 # two equal centres


def case(B, T, centres, density, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    tab = V.harmonic_bins(centres)
    spec, params = rs.rand(B, T, len(centres)), scale * rs.randn(V.N_PARAMS)
    target = rs.rand(B, T, 88)
    mask = (rs.rand(B, T, 88) < density).astype(np.float64)
    return spec, tab, params, target, mask


def autograd(spec, tab, params, target, mask):
    p = torch.tensor(params, dtype=torch.float64, requires_grad=True)
    loss = V.loss_torch(torch.tensor(spec), tab, p, torch.tensor(target), torch.tensor(mask))
    loss.backward()
    return float(loss.detach()), p.grad.numpy()


@pytest.mark.parametrize('kind,B,T,density,scale', [('Mel', 2, 9, 0.05, 1.0), ('Mel', 1, 3, 1.0, 1.0), ('forty', 1, 1, 1.0, 1.0),
                                                    ('CQT84', 3, 17, 0.01, 1.0), ('Mel', 2, 9, 0.05, 8.0)])
def test_gradient_equals_autograd(kind, B, T, density, scale):
    spec, tab, params, target, mask = case(B, T, CENTRES[kind](), density, 7, scale)
    mask[0, 0, 0] = 1.0
    loss, grad = V.loss_and_grad_host(spec, tab, params, target, mask)
    want_loss, want_grad = autograd(spec, tab, params, target, mask)
    assert abs(loss - want_loss) <= 1e-12 and np.abs(grad - want_grad).max() <= 1e-12
    assert np.abs(grad).max() > 0


def test_gradient_of_an_empty_mask_and_of_single_cells():
    spec, tab, params, target, mask = case(2, 6, CENTRES['Mel'](), 0.0, 3)
    loss, grad = V.loss_and_grad_host(spec, tab, params, target, mask)
    assert loss == 0.0 and not grad.any()
    want_loss, want_grad = autograd(spec, tab, params, target, mask)
    assert want_loss == 0.0 and not want_grad.any()
    for t in (0, 5):                                                               # the frame clamp at either end
        one = np.zeros_like(mask)
        one[1, t, 40] = 1.0
        loss, grad = V.loss_and_grad_host(spec, tab, params, target, one)
        want_loss, want_grad = autograd(spec, tab, params, target, one)
        assert abs(loss - want_loss) <= 1e-12 and np.abs(grad - want_grad).max() <= 1e-12
        x = V.masked_features_host(spec, tab, np.array([1]), np.array([t]), np.array([40]))[0]
        rows = np.clip(np.arange(t - 1, t + 3), 0, 5)
        assert np.array_equal(x[:32].reshape(4, 8), spec[1][rows][:, tab[40]]) and x[32] == 40 / 88
    # features() and masked_features_host() are the same numbers
    full = V.features(torch.tensor(spec), tab).numpy()
    b, t, p = np.nonzero(np.ones_like(mask))
    assert np.array_equal(full.reshape(-1, 33), V.masked_features_host(spec, tab, b, t, p))


def test_head_checkpoint_names_its_front_end():
    head = V.VelocityHead('CQT', CENTRES['CQT'](), seed=3)
    state = head.state_dict()
    assert set(state) == {'w1', 'b1', 'w2', 'b2', 'spec_kind', 'centres'} and head.packed().numel() == 1121
    again = V.VelocityHead.from_state_dict(state)
    assert again.spec == 'CQT' and np.array_equal(again.table, head.table) and torch.equal(again.packed(), head.packed())
    x = torch.rand(1, 4, 176)
    assert torch.equal(again.definition(x), head.definition(x)) and again.definition(x).shape == (1, 4, 88)
    with pytest.raises(RuntimeError, match='HIP device only'):
        head(x)                                                                    # no CPU fallback for the product path


def test_front_end_centres_of_both_front_ends():
    """The centres come from the model's own front end: its `mel_basis` buffer, or the parameters its CQT1992v2 was built with."""
    import reconvat_amd as ra
    mel = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=False, mode='imagewise', spec='Mel')
    kind, centres = V.front_end_centres(mel)
    assert kind == 'Mel' and np.array_equal(centres, CENTRES['Mel']())
    cqt = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=False, mode='imagewise', spec='CQT')
    kind, centres = V.front_end_centres(cqt)
    assert kind == 'CQT' and centres.shape == (176,) and np.array_equal(centres, CENTRES['CQT']())
    assert cqt.spectrogram.fmin == 27.5 and cqt.spectrogram.bins_per_octave == 24
    # the centres agree with the kernel bank itself: a bin's kernel has Q fs / f samples
    q = 1 / (2 ** (1 / 24) - 1)
    assert np.array_equal(np.ceil(q * 16000 / centres), cqt.spectrogram.lenghts.numpy().astype(np.float64))
    head = V.VelocityHead.for_model(cqt)
    assert head.spec == 'CQT' and np.array_equal(head.table, V.harmonic_bins(centres))
    head.check_front_end(cqt)
    with pytest.raises(ValueError, match='front end'):
        head.check_front_end(mel)


def test_velocity_decode_against_the_golden():
    g = np.load(os.path.join(G, 'decoding.npz'))
    for seed in (0, 1, 2):
        on, fr, vel = (torch.from_numpy(a) for a in decoding_rolls(seed))
        p, i, v = md.extract_notes_with_velocity(on, fr, vel, 0.4, 0.6, rule='rule2', min_frames=1, bridge_gap=0)
        assert np.array_equal(p, g[f'{seed}_v_p']) and np.array_equal(i, g[f'{seed}_v_i'])
        assert v.dtype == np.float32 and np.abs(v - g[f'{seed}_v_v']).max() <= 1e-6
        p0, i0 = md.extract_notes_wo_velocity(on, fr, 0.4, 0.6, rule='rule2')
        assert np.array_equal(p, p0) and np.array_equal(i, i0)


def test_note_velocities_of_a_bridged_note():
    """Onset on at frames 2, 3 and 9; frames on over [2, 5) and [8, 12): bridge_gap = 3 makes one note [2, 12) (and a second start
    at 9) whose interior [5, 8) is inactive; the mean runs over the onset-active frames alone."""
    on, fr, vel = np.zeros((14, 88), np.float32), np.zeros((14, 88), np.float32), np.zeros((14, 88), np.float32)
    on[[2, 3, 9], 30] = 1
    fr[2:5, 30] = fr[8:12, 30] = 1
    vel[:, 30] = np.arange(14, dtype=np.float32) / 16
    vel[5:8, 30] = 100.0                                                           # must not be looked at
    p, i, v = md.extract_notes_with_velocity(on, fr, vel, 0.5, 0.5, bridge_gap=3)
    assert p.tolist() == [30, 30] and i.tolist() == [[2, 12], [9, 12]]
    assert v.tolist() == [np.float32((2 + 3 + 9) / 16 / 3), np.float32(9 / 16)]
    assert md.note_velocities(on, vel, 0.5, [30, 31], [[5, 8], [0, 14]]).tolist() == [0.0, 0.0]      # no onset-active frame
    assert md.note_velocities(on, vel, 0.5, [], []).shape == (0,)


def test_note_with_velocity_metric():
    hz = ev.midi_to_hz
    ref_i = np.array([[0.0, 1.0], [1.0, 2.0], [2.0, 3.0], [3.0, 4.0]])
    ref_p = hz(np.array([60, 62, 64, 65]))
    ref_v = np.array([30.0, 60.0, 90.0, 120.0])
    # a perfect affine relation: all pairs kept
    est_v = 0.002 * ref_v + 0.3
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, ref_v, ref_i, ref_p, est_v) == (1.0, 1.0, 1.0, 1.0)
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, ref_v, ref_i, ref_p, est_v, offset_ratio=None) == (1.0, 1.0, 1.0, 1.0)
    # one outlier among ten: the line stays with the nine, the outlier is more than 0.1 off and is dropped
    n = 10
    ri = np.stack([np.arange(n, dtype=np.float64), np.arange(n) + 0.5], axis=1)
    rp = hz(np.full(n, 60))
    rv = np.linspace(20, 110, n)
    evel = (rv - 20) / 90
    evel[4] += 0.3
    p, r, f, o = ev.evaluate_notes_with_velocity(ri, rp, rv, ri, rp, evel)
    assert (p, r) == (0.9, 0.9) and abs(f - 0.9) < 1e-12 and o == 1.0
    # constant reference velocities: max(1, max - min) = 1, every mapped velocity 0; a constant estimate fits exactly
    const = np.full(4, 64.0)
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, const, ref_i, ref_p, np.full(4, 0.5))[:3] == (1.0, 1.0, 1.0)
    # ... and a range below 1 is not stretched: references 0 and 0.5 against estimates that cannot be fitted closer than 0.25
    half = np.array([0.0, 0.5, 0.0, 0.5])
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, half, ref_i, ref_p, np.array([0.0, 0.0, 1.0, 1.0]))[:3] == (0.0, 0.0, 0.0)
    # an unmatched estimate counts against precision only; an empty matching and empty sides give zeros
    est_i = np.vstack([ref_i, [[10.0, 11.0]]])
    est_p = np.append(ref_p, hz(70))
    p, r, _, _ = ev.evaluate_notes_with_velocity(ref_i, ref_p, ref_v, est_i, est_p, np.append(est_v, 0.9))
    assert (p, r) == (0.8, 1.0)
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, ref_v, ref_i + 10.0, ref_p, est_v) == (0.0, 0.0, 0.0, 0.0)
    assert ev.evaluate_notes_with_velocity(ref_i, ref_p, ref_v, np.zeros((0, 2)), np.array([]), np.array([])) == (0.0, 0.0, 0.0, 0.0)


def test_midi_velocities():
    assert V.midi_velocities([0.0, 0.001, 0.5, 64.4 / 128, 0.999, 1.0]).tolist() == [1, 1, 64, 64, 127, 127]


def test_the_definition_learns_dynamics():
    """Full-batch Adam (lr 3e-3, 2000 steps) on the float32 torch definition at the 941 onset cells of the 12 training tracks (host
    renderer, oracle front end); the error at the 312 onset cells of the 4 held-out tracks must be below 0.8 of the constant
    predictor's.  Reached: 14.06 / 128 against 22.21 / 128, ratio 0.633 (0.707 after 1000 steps, 0.621 after 3000)."""
    from oracle import frontend as of
    bufs = of.frontend_buffers()
    front = lambda audio: of.frontend(audio[:, :-1], bufs)
    tracks = vc.corpus('cpu')
    head = V.VelocityHead('Mel', V.mel_centres(bufs['spectrogram.mel_basis']), seed=0)

    def cells(part):
        spec, mask, target = vc.stack(part, front)
        b, t, p = np.nonzero(mask.numpy())
        x = torch.tensor(V.masked_features_host(spec.numpy(), head.table, b, t, p), dtype=torch.float32)
        return x, target[mask > 0], mask, target

    def forward(x):
        w1, b1, w2, b2 = V.unpack(head.packed())
        return torch.sigmoid(torch.sigmoid(x @ w1.t() + b1) @ w2 + b2)

    x_tr, y_tr, m_tr, t_tr = cells(tracks[:vc.N_TRAIN])
    x_he, y_he, m_he, t_he = cells(tracks[vc.N_TRAIN:])
    # the loss over the masked cells alone is the definition's loss over all of them
    with torch.no_grad():
        spec8 = vc.stack(tracks[:1], front)[0]
        whole = head.definition_loss(spec8, t_tr[:1], m_tr[:1])
        n0 = int(m_tr[0].sum())
        assert abs(float(whole) - float(((forward(x_tr[:n0]) - y_tr[:n0]) ** 2).mean())) < 1e-6
    vc.train(head, lambda: ((forward(x_tr) - y_tr) ** 2).mean())
    with torch.no_grad():
        v_hat = torch.zeros_like(t_he)
        v_hat[m_he > 0] = forward(x_he)
    err, const = vc.errors(v_hat, m_he, t_he, m_tr, t_tr)
    print(f'held-out error {err:.2f} / 128, constant {const:.2f} / 128, ratio {err / const:.3f}')
    assert err / const < 0.8
