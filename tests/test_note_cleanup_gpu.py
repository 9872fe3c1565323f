"""Note clean-up on the device (csrc/eval.hip): rv_eval_decode_clean and rv_eval_sweep_clean against the host
definition (reconvat_amd/decoding.py), every comparison == on integers.  Hand-made rolls aim at what the kernels have to carry over
the 64-frame tile edges (bridged gaps, run ends, the painting carry, note ranks); then sizes around the tile, the (1, 0) case against
the old entry point, the sweep, the argument checks, evaluate_wo_velocity and UNet_Onset.transcribe / transcribe2midi."""
import os
import sys

import numpy as np
import pytest
import torch

import sweep_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RULES = ['rule1', 'rule2']
CLEANUPS = [(1, 0), (2, 0), (1, 2), (3, 1), (5, 3), (32, 31)]
ON_THR, FR_THR = [0.3, 0.5, 0.7], [0.5, 0.3]


def rolls_of(T, *pitches):
    """Per pitch (pitch, [active [a, b) ...], [frames where the onset roll rises]): the frame roll is on over the active stretches,
    the onset roll for the one frame of each rise."""
    onset, frame = np.zeros((T, 88), np.float32), np.zeros((T, 88), np.float32)
    for pitch, active, rises in pitches:
        for a, b in active:
            frame[a:b, pitch] = 1
        for r in rises:
            onset[r, pitch] = 1
    return onset, frame


def decode(dev, onset, frame, m, g, rule='rule2', thr=(0.5, 0.5)):
    """Device and host decode; asserts that they agree in the notes and in the painted roll, returns (notes, roll)."""
    from reconvat_amd import decoding as md
    on, fr = torch.from_numpy(onset), torch.from_numpy(frame)
    p, i = md.extract_notes_wo_velocity(on, fr, *thr, rule=rule, min_frames=m, bridge_gap=g)
    _, freqs = md.notes_to_frames(p, i, frame.shape)
    want_roll = np.zeros(frame.shape, np.uint8)
    for t, f in enumerate(freqs):
        want_roll[t, f] = 1
    gp, gi, painted = md.extract_notes_wo_velocity_device(on.to(dev), fr.to(dev), *thr, rule=rule, min_frames=m, bridge_gap=g)
    assert gp.shape == p.shape and gi.shape == i.shape, (gp.shape, p.shape, m, g, rule)
    assert np.array_equal(gp, p) and np.array_equal(gi, i), (m, g, rule)
    got_roll = painted.cpu().numpy()
    assert got_roll.dtype == np.uint8 and np.array_equal(got_roll, want_roll), (m, g, rule)
    return [(int(s), int(q), int(e)) for q, (s, e) in zip(p, np.asarray(i).reshape(-1, 2))], want_roll


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('first, second', [((50, 60), (68, 80)),         # the gap lies over the tile edge
                                           ((50, 64), (72, 80)),         # ... begins at it
                                           ((40, 56), (64, 80))])        # ... ends at it
def test_gap_at_a_tile_edge(dev, rule, first, second):
    """A gap of 8 frames: bridged at g = 8, not at g = 7; pitch 70 holds the same one tile later."""
    shift = lambda ab: (ab[0] + 64, ab[1] + 64)
    rolls = rolls_of(200, (20, [first, second], [first[0], second[0]]), (70, [shift(first), shift(second)], [first[0] + 64, second[0] + 64]))
    notes, roll = decode(dev, *rolls, 1, 8, rule)
    assert notes == [(first[0], 20, second[1]), (second[0], 20, second[1]), (first[0] + 64, 70, second[1] + 64), (second[0] + 64, 70, second[1] + 64)]
    assert roll[first[0]:second[1], 20].all() and roll[:, 20].sum() == second[1] - first[0]
    notes, roll = decode(dev, *rolls, 1, 7, rule)
    assert notes[:2] == [(first[0], 20, first[1]), (second[0], 20, second[1])] and not roll[first[1]:second[0], 20].any()
    # m = 20: only the bridged stretch (30 or 40 frames) makes the first note long enough; no part is (at most 16 frames)
    notes, _ = decode(dev, *rolls, 20, 8, rule)
    assert notes == [(first[0], 20, second[1]), (first[0] + 64, 70, second[1] + 64)]
    assert decode(dev, *rolls, 20, 7, rule)[0] == []


@pytest.mark.parametrize('rule', RULES)
def test_runs_at_the_ends_of_the_roll_are_not_bridged(dev, rule):
    rolls = rolls_of(67, (20, [(3, 10), (35, 40), (60, 64)], [3, 60]), (70, [(1, 2), (30, 36), (66, 67)], [1, 66]))
    notes, roll = decode(dev, *rolls, 1, 31, rule)
    assert notes == [(1, 70, 67), (3, 20, 64), (60, 20, 64), (66, 70, 67)]         # the gaps in between are bridged ...
    assert not roll[:3, 20].any() and not roll[64:, 20].any() and not roll[0, 70]      # ... [0, 3), [64, 67) and [0, 1) are not
    assert roll[3:64, 20].all() and roll[1:, 70].all()


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('m', [2, 5, 32])
def test_boundary_of_the_minimum_length(dev, rule, m):
    T = 200
    rolls = rolls_of(T, (20, [(60, 60 + m - 1), (T - 1, T)], [60, T - 1]), (70, [(60, 60 + m)], [60]))
    notes, roll = decode(dev, *rolls, m, 0, rule)
    assert notes == [(60, 70, 60 + m)] and roll.sum() == m and not roll[:, 20].any()
    notes, _ = decode(dev, *rolls, m - 1, 0, rule)
    assert (60, 20, 60 + m - 1) in notes and ((T - 1, 20, T) in notes) == (m == 2)


@pytest.mark.parametrize('rule', RULES)
def test_painting_carry_over_a_tile_edge(dev, rule):
    """A dropped note that starts at frame 62 must not be painted in tile 1 either; one frame longer it is kept."""
    rolls = rolls_of(200, (20, [(62, 66)], [62]), (70, [(62, 67)], [62]))
    notes, roll = decode(dev, *rolls, 5, 0, rule)
    assert notes == [(62, 70, 67)] and not roll[:, 20].any() and roll[:, 70].sum() == 5 and roll[64:67, 70].all()
    # a kept run that covers a whole tile is painted through it; and the first case again at the third tile edge
    rolls = rolls_of(300, (20, [(126, 194)], [126]), (70, [(126, 195)], [126, 192]))
    notes, roll = decode(dev, *rolls, 32, 0, rule)
    assert notes == [(126, 20, 194), (126, 70, 195)] and roll[:, 20].sum() == 68 and roll[:, 70].sum() == 69
    rolls = rolls_of(300, (20, [(190, 194)], [190]), (70, [(190, 195)], [190]))
    notes, roll = decode(dev, *rolls, 5, 0, rule)
    assert notes == [(190, 70, 195)] and not roll[:, 20].any()


@pytest.mark.parametrize('rule', RULES)
def test_long_run_is_kept(dev, rule):
    T = 300
    rolls = rolls_of(T, (20, [(63, 257)], [63]), (70, [(63, T)], [63]))
    notes, roll = decode(dev, *rolls, 32, 0, rule)
    assert notes == [(63, 20, 257), (63, 70, T)] and roll[:, 20].sum() == 194 and roll[:, 70].sum() == T - 63


@pytest.mark.parametrize('rule', RULES)
def test_two_starts_in_one_run(dev, rule):
    rolls = rolls_of(200, (20, [(10, 20)], [10, 17]), (70, [(60, 70)], [60, 67]))
    notes, roll = decode(dev, *rolls, 5, 0, rule)
    assert notes == [(10, 20, 20), (60, 70, 70)] and roll[10:20, 20].all() and roll[60:70, 70].all() and roll.sum() == 20
    assert len(decode(dev, *rolls, 3, 0, rule)[0]) == 4


@pytest.mark.parametrize('rule', RULES)
def test_bridging_lengthens_a_note(dev, rule):
    rolls = rolls_of(200, (20, [(62, 64), (66, 70)], [62]), (70, [(126, 128), (130, 134)], [126]))
    notes, roll = decode(dev, *rolls, 6, 2, rule)
    assert notes == [(62, 20, 70), (126, 70, 134)] and roll[62:70, 20].all() and roll.sum() == 16
    assert decode(dev, *rolls, 6, 1, rule)[0] == []


@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 129, 257])
def test_sizes_at_the_edges(dev, T):
    _, _, on_p, fr_p = sc.random_rolls(T, seed=200 + T, density=0.12)
    for rule in RULES:
        for m, g in ((1, 0), (3, 1), (32, 31)):
            decode(dev, on_p, fr_p, m, g, rule)
            decode(dev, on_p, fr_p, m, g, rule, thr=(0.3, 0.3))


def raw_decode(dev, name, on, fr, extra, T=None, ws_bytes=None, null=None):
    """rv_eval_decode / rv_eval_decode_clean called directly; returns (status, notes, count, painted)."""
    from reconvat_amd import _lib
    T = on.shape[0] if T is None else T
    need = _lib.load().rv_eval_workspace_bytes(on.shape[0])
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    max_notes = 88 * ((on.shape[0] + 1) // 2)
    notes = torch.full((max_notes, 3), -7, dtype=torch.int32, device=dev)
    count = torch.full((1,), -7, dtype=torch.int32, device=dev)
    painted = torch.full(tuple(on.shape), 7, dtype=torch.uint8, device=dev)
    ptr = {'onsets': on.data_ptr(), 'notes': notes.data_ptr(), 'workspace': ws.data_ptr()}
    if null:
        ptr[null] = None
    rc = _lib.invoke(name, ptr['onsets'], fr.data_ptr(), T, 0.5, 0.5, 2, *extra, ptr['notes'], max_notes, count.data_ptr(), painted.data_ptr(),
                     ptr['workspace'], need if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, notes.cpu().numpy(), int(count.item()), painted.cpu().numpy()


def test_clean_entry_point_at_1_0_is_the_old_one(dev):
    _, _, on_p, fr_p = sc.random_rolls(200, 3)
    on, fr = torch.from_numpy(on_p).to(dev), torch.from_numpy(fr_p).to(dev)
    old = raw_decode(dev, 'rv_eval_decode', on, fr, ())
    new = raw_decode(dev, 'rv_eval_decode_clean', on, fr, (1, 0))
    assert old[0] == new[0] == 0 and old[2] == new[2] > 50
    assert np.array_equal(old[1], new[1]) and np.all(new[1][:new[2]] >= 0) and np.all(new[1][new[2]:] == -7)
    assert np.array_equal(old[3], new[3]) and set(np.unique(new[3])) == {0, 1}
    cleaned = raw_decode(dev, 'rv_eval_decode_clean', on, fr, (3, 1))
    assert cleaned[0] == 0 and 0 < cleaned[2] < new[2] and np.all(cleaned[1][cleaned[2]:] == -7)


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('case', ['random40', 'random200', 'chain', 'long_runs'])
def test_sweep_equals_host(dev, case, rule):
    from reconvat_amd import evaluate as ev
    rolls = {'random40': lambda: sc.random_rolls(40, 11, density=0.12), 'random200': lambda: sc.random_rolls(200, 3),
             'chain': sc.chain_rolls, 'long_runs': lambda: sc.long_run_rolls(200)}[case]()
    cpu = [torch.from_numpy(r) for r in rolls]
    gpu = [x.to(dev) for x in cpu]
    plain = ev.sweep_counts_device(*gpu, ON_THR, FR_THR, rule=rule)
    differs = 0
    for m, g in CLEANUPS:
        want = ev.sweep_counts_host(*cpu, ON_THR, FR_THR, rule=rule, min_frames=m, bridge_gap=g)
        got = ev.sweep_counts_device(*gpu, ON_THR, FR_THR, rule=rule, min_frames=m, bridge_gap=g)
        assert set(got) == set(want)
        for k in ev.SWEEP_KEYS:
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want[k]), (k, m, g, got[k], want[k])
        assert got['n_ref'] == want['n_ref'] and got['frame_ref'] == want['frame_ref']
        if (m, g) == (1, 0):
            assert all(np.array_equal(got[k], plain[k]) for k in ev.SWEEP_KEYS)
        differs += any(not np.array_equal(got[k], plain[k]) for k in ev.SWEEP_KEYS)
    assert differs == (0 if case == 'long_runs' else 5)                # (no clean-up setting touches the long runs: nothing may change)


def raw_sweep(dev, rolls, extra, ws_bytes=None, null=None):
    """rv_eval_sweep_clean called directly on valid buffers (3 x 2 grid); returns (status, counts)."""
    from reconvat_amd import _lib
    T = rolls[2].shape[0]
    on, fr = torch.from_numpy(rolls[2]).to(dev), torch.from_numpy(rolls[3]).to(dev)
    thr = torch.tensor([0.3, 0.5, 0.7, 0.0, 0.5, 0.3], dtype=torch.float32, device=dev)
    ref = torch.zeros((1, 5), dtype=torch.int32, device=dev)
    roll = torch.zeros((T, 88), dtype=torch.uint8, device=dev)
    need = _lib.load().rv_eval_sweep_workspace_bytes(T, 3, 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    counts = torch.full((3 * 2 * 5 + 5,), -7, dtype=torch.int64, device=dev)
    totals = torch.full((2,), -7, dtype=torch.int64, device=dev)
    ptr = {'onsets': on.data_ptr(), 'counts': counts.data_ptr(), 'workspace': ws.data_ptr()}
    if null:
        ptr[null] = None
    rc = _lib.invoke('rv_eval_sweep_clean', ptr['onsets'], fr.data_ptr(), T, thr.data_ptr(), 3, thr.data_ptr() + 16, 2, 2, *extra,
                     ref.data_ptr(), 0, roll.data_ptr(), ptr['counts'], totals.data_ptr(), ptr['workspace'],
                     need if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy()


def test_argument_errors(dev):
    from reconvat_amd import _lib, decoding as md, evaluate as ev
    rolls = sc.random_rolls(200, 3)
    on, fr = torch.from_numpy(rolls[2]).to(dev), torch.from_numpy(rolls[3]).to(dev)
    need = _lib.load().rv_eval_workspace_bytes(200)
    assert need == _lib.load().rv_eval_workspace_bytes(200) > 0 and _lib.load().rv_abi_version() == 1
    for kw in (dict(extra=(0, 0)), dict(extra=(33, 0)), dict(extra=(1, -1)), dict(extra=(1, 32)), dict(extra=(2, 1), ws_bytes=need - 16),
               dict(extra=(2, 1), null='onsets'), dict(extra=(2, 1), null='notes'), dict(extra=(2, 1), null='workspace')):
        rc, notes, count, painted = raw_decode(dev, 'rv_eval_decode_clean', on, fr, **kw)
        assert rc != 0, kw
        assert np.all(notes == -7) and count == -7 and np.all(painted == 7), kw       # nothing was launched
        assert 'rv_eval_decode_clean' in _lib.last_error(), (kw, _lib.last_error())
    assert raw_decode(dev, 'rv_eval_decode_clean', on, fr, (2, 1))[0] == 0
    need = _lib.load().rv_eval_sweep_workspace_bytes(200, 3, 2)
    for kw in (dict(extra=(0, 0)), dict(extra=(33, 0)), dict(extra=(1, -1)), dict(extra=(1, 32)), dict(extra=(2, 1), ws_bytes=need - 16),
               dict(extra=(2, 1), null='onsets'), dict(extra=(2, 1), null='counts'), dict(extra=(2, 1), null='workspace')):
        rc, counts = raw_sweep(dev, rolls, **kw)
        assert rc != 0, kw
        assert np.all(counts == -7), kw
        assert 'rv_eval_sweep_clean' in _lib.last_error(), (kw, _lib.last_error())
    rc, counts = raw_sweep(dev, rolls, (2, 1))
    assert rc == 0 and counts[:30].min() >= 0 and counts[:30].max() > 0 and np.all(counts[30:] == -7)
    gpu = [torch.from_numpy(r).to(dev) for r in rolls]
    for bad in (dict(min_frames=0), dict(min_frames=33), dict(bridge_gap=-1), dict(bridge_gap=32), dict(min_frames=2.5)):
        with pytest.raises(ValueError):
            md.extract_notes_wo_velocity_device(gpu[2], gpu[3], **bad)
        with pytest.raises(ValueError):
            ev.sweep_counts_device(*gpu, [0.5], [0.5], **bad)


def test_evaluate_wo_velocity_device_equals_host(dev):
    from reconvat_amd import evaluate as ev
    model = sc.StubModel()
    want = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4)), model, reconstruction=False, device_metrics=False, min_frames=3, bridge_gap=1)
    got = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4), device=dev), model, reconstruction=False, device_metrics=True, min_frames=3,
                                  bridge_gap=1)
    plain = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4), device=dev), model, reconstruction=False, device_metrics=True)
    assert list(got) == list(want) and 'metric/note/f1' in want and 'metric/frame/chroma_total_error' in want
    for k in want:
        assert len(got[k]) == len(want[k]) == 2
        for a, b in zip(got[k], want[k]):
            if k.startswith('metric/MusicNet/micro_avg_P'):
                assert abs(a - b) <= 1e-9, (k, a, b)
            else:
                assert a == b, (k, a, b)
    assert got['metric/note/precision'] != plain['metric/note/precision'] and got['metric/frame/precision'] != plain['metric/frame/precision']


@pytest.fixture(scope='module')
def onset_model(dev):
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel')
    m.load_state_dict(fx.fixture_params('onset', True))
    return m.to(dev).eval()


def test_unet_onset_transcribe_is_the_first_pass_of_run_on_batch(dev, onset_model, monkeypatch):
    from oracle import fixture as fx
    onset, frame = fx.fixture_labels(2, 64, 'L')
    batch = {'audio': fx.fixture_audio(2, 64 * 512, 'L').to(dev), 'onset': onset.to(dev), 'frame': frame.to(dev)}
    with torch.no_grad():
        want, _, _ = onset_model.run_on_batch(batch)
    passes = []
    transcriber, reconstructor = onset_model.transcriber.forward, onset_model.reconstructor.forward
    monkeypatch.setattr(onset_model.transcriber, 'forward', lambda *a, **k: passes.append('transcriber') or transcriber(*a, **k))
    monkeypatch.setattr(onset_model.reconstructor, 'forward', lambda *a, **k: passes.append('reconstructor') or reconstructor(*a, **k))
    with torch.no_grad():
        got = onset_model.transcribe({'audio': batch['audio']})
    assert passes == ['transcriber']
    assert list(got) == ['onset', 'frame'] and got['frame'].shape == (2, 64, 88)
    assert torch.equal(got['onset'], want['onset']) and torch.equal(got['frame'], want['frame'])
    assert not torch.equal(got['onset'], got['frame'])


def test_transcribe2midi_with_the_onset_model_and_cleanup(dev, onset_model, tmp_path):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    from oracle import fixture as fx
    from reconvat_amd import decoding as md
    from reconvat_amd.midi import parse_midi, save_midi
    audio = fx.fixture_audio(1, 64 * 512, 'L')[0]
    clip = tmp_path / 'clip.pt'
    torch.save({'audio': (audio * 32768.0).round().clamp(-32768, 32767).to(torch.int16)}, str(clip))
    with torch.no_grad():
        pred = onset_model.transcribe({'audio': tf.load_audio(str(clip)).to(dev).unsqueeze(0)})
    onset, frame = pred['onset'].squeeze(0).relu().cpu(), pred['frame'].squeeze(0).relu().cpu()
    # the weights are a fixture, not a trained model: thresholds from the posteriorgrams themselves, so that there are notes to clean up
    thr_on, thr_fr = float(onset.flatten().quantile(0.8)), float(frame.flatten().quantile(0.8))
    p_all, _ = md.extract_notes_wo_velocity(onset, frame, thr_on, thr_fr, rule='rule2')
    p_est, i_est = md.extract_notes_wo_velocity(onset, frame, thr_on, thr_fr, rule='rule2', min_frames=2, bridge_gap=1)
    assert 0 < len(p_est) < len(p_all)
    tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / 'out'), onset_threshold=thr_on, frame_threshold=thr_fr, min_frames=2,
                       bridge_gap=1)
    scaling = 512 / 16000
    from reconvat_amd.evaluate import midi_to_hz
    save_midi(str(tmp_path / 'want.mid'), np.array([midi_to_hz(21 + q) for q in p_est]), np.asarray(i_est) * scaling, [127] * len(p_est))
    got, want = parse_midi(str(tmp_path / 'out' / 'ReconVAT-clip.mid')), parse_midi(str(tmp_path / 'want.mid'))
    assert got.shape == want.shape == (len(p_est), 4) and np.array_equal(got, want)
