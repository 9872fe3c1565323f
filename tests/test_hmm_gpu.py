"""Viterbi note decoding on the device (csrc/hmm.hip): rv_hmm_decode against the host definition
(reconvat_amd/hmm.py), every comparison == on integers.  Sizes aim at the edges of the 64-frame chunks the kernels cut the time axis
into; then the number of parameter sets, aliasing rolls, non-finite values, a path cost beyond 2^31, run-to-run bits, the argument
checks, and the layers above: extract_notes_hmm_device, evaluate_wo_velocity(hmm=), tune_hmm and transcribe2midi(hmm=)."""
import os
import sys

import numpy as np
import pytest
import torch

import sweep_cases as sc
from reconvat_amd.hmm import DEVICE_CHUNK_FRAMES
from test_hmm import NAMES, random_set

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_decode(dev, onsets, frames, sets):
    from reconvat_amd import hmm as nh
    on = torch.from_numpy(onsets).to(dev)
    fr = on if frames is onsets else torch.from_numpy(frames).to(dev)
    states, cost = nh.viterbi_states_device(on, fr, sets)
    assert states.dtype == torch.uint8 and states.shape == (len(sets), onsets.shape[0], 88) and states.device == on.device
    assert cost.dtype == torch.int64 and cost.shape == (len(sets), 88)
    return states.cpu().numpy(), cost.cpu().numpy()


def assert_equals_host(dev, onsets, frames, sets):
    from reconvat_amd import hmm as nh
    states, cost = device_decode(dev, onsets, frames, sets)
    for g, s in enumerate(sets):
        want_states, want_cost = nh.viterbi_states(onsets, frames, *nh._as_set(s))
        assert np.array_equal(cost[g], want_cost), (g, np.flatnonzero(cost[g] != want_cost)[:5])
        bad = np.argwhere(states[g] != want_states)
        assert len(bad) == 0, (g, len(bad), bad[:5])
    return states, cost


def mixed_sets(n, seed=0):
    """NoteHMM objects and raw (tables, trans) pairs in turn: defaults, free switching, random sets with forbidden entries, sets with
    many exact ties."""
    from reconvat_amd import NoteHMM
    rng = np.random.RandomState(seed)
    kinds = [lambda: NoteHMM(), lambda: random_set(rng, quanta=[1000, 3000]), lambda: NoteHMM(0.3, 0.7, 0.0, 0.0, 0.0),
             lambda: random_set(rng), lambda: NoteHMM(0.6, 0.4, 4.0, 1.0, 0.5, use_onsets=False), lambda: random_set(rng, quanta=[500, 20000])]
    return [kinds[i % len(kinds)]() for i in range(n)]


L = DEVICE_CHUNK_FRAMES                                                # the tests aim at the edges of the kernels' chunks
SIZES = [1, 2, L - 1, L, L + 1, 2 * L, 2 * L + 1, 5 * L + 3]


def test_chunk_length_is_the_kernels():
    """One chunk up to L frames -- the workspace grows by the 176 bytes of a quantised row per frame -- and a second one at L + 1."""
    from reconvat_amd import _lib
    need = _lib.load().rv_hmm_workspace_bytes
    assert L >= 2 and need(L, 1) == need(1, 1) + (L - 1) * 176 and need(L + 1, 1) > need(L, 1) + 176 + 88 * 60


@pytest.mark.parametrize('T', SIZES)
def test_default_model_equals_host(dev, T):
    from reconvat_amd import NoteHMM
    _, _, on_p, fr_p = sc.random_rolls(T, 3)
    states, _ = assert_equals_host(dev, on_p, fr_p, [NoteHMM()])
    if T >= 2 * L:
        assert set(np.unique(states)) == {0, 1, 2}


@pytest.mark.parametrize('T', SIZES)
def test_random_tables_with_ties_equal_host(dev, T):
    rng = np.random.RandomState(T)
    _, _, on_p, fr_p = sc.random_rolls(T, 5)
    sets = [random_set(rng, quanta=[1000, 3000]), random_set(rng, quanta=[500, 20000]), random_set(rng)]
    states, _ = assert_equals_host(dev, on_p, fr_p, sets)
    if T >= 2 * L:
        assert all(len(np.unique(states[g])) == 3 for g in range(2))


@pytest.mark.parametrize('G', [1, 3, 16])
def test_mixed_sets(dev, G):
    _, _, on_p, fr_p = sc.random_rolls(3 * L + 5, 7)
    sets = mixed_sets(G)
    if G > 1:
        sets[-1] = sets[0]                                              # the same set in two slots
    states, cost = assert_equals_host(dev, on_p, fr_p, sets)
    if G > 1:
        assert np.array_equal(states[0], states[-1]) and np.array_equal(cost[0], cost[-1])
        assert not np.array_equal(states[0], states[1])


def test_seventeen_sets_take_two_batches(dev):
    from reconvat_amd import _lib
    _, _, on_p, fr_p = sc.random_rolls(L + 9, 8)
    launches = []
    hook = lambda name, args, fn: (launches.append((name, args[5])), fn(*args))[1]
    _lib.HOOK[0] = hook
    try:
        assert_equals_host(dev, on_p, fr_p, mixed_sets(17, seed=1))
    finally:
        _lib.HOOK[0] = None
    assert launches == [('rv_hmm_decode', 16), ('rv_hmm_decode', 1)]


def test_aliasing_rolls(dev):
    from reconvat_amd import NoteHMM
    _, _, _, fr_p = sc.random_rolls(2 * L + 7, 9)
    assert_equals_host(dev, fr_p, fr_p, [NoteHMM(use_onsets=False), NoteHMM(), random_set(np.random.RandomState(2), quanta=[1000, 3000])])


def test_non_finite_and_out_of_range_values(dev):
    from reconvat_amd import NoteHMM
    rng = np.random.RandomState(4)
    _, _, on_p, fr_p = sc.random_rolls(2 * L + 3, 10)
    for roll in (on_p, fr_p):
        for value in (np.nan, -0.5, -0.0, 1.0, 1.5, np.inf, -np.inf, np.float32(1) / np.float32(256), np.nextafter(np.float32(1), np.float32(0))):
            roll[rng.rand(*roll.shape) < 0.02] = value
    with np.errstate(invalid='ignore'):
        assert_equals_host(dev, on_p, fr_p, [NoteHMM(), random_set(rng), random_set(rng, quanta=[1000, 3000])])


@pytest.fixture(scope='module')
def overflow_case():
    """T = 40 000, uniform random q, every allowed transition and init entry of the default model raised by 60 000: the path cost
    passes 2^31, which int32 accumulators cannot follow."""
    from reconvat_amd import NoteHMM, hmm as nh
    rng = np.random.RandomState(12)
    on = ((rng.randint(0, 256, size=(40000, 88)) + 0.5) / 256).astype(np.float32)
    fr = ((rng.randint(0, 256, size=(40000, 88)) + 0.5) / 256).astype(np.float32)
    tables, trans = NoteHMM().tables()
    trans = np.where(trans >= 0, trans + 60000, trans).astype(np.int32)
    return on, fr, (tables, trans), nh.viterbi_states(on, fr, tables, trans)


def test_path_cost_beyond_int32(dev, overflow_case):
    on, fr, one_set, (want_states, want_cost) = overflow_case
    assert want_cost.min() > 2 ** 31
    states, cost = device_decode(dev, on, fr, [one_set])
    assert cost.min() > 2 ** 31 and np.array_equal(cost[0], want_cost)
    assert np.array_equal(states[0], want_states) and set(np.unique(want_states)) == {0, 1, 2}


def test_two_runs_give_the_same_bytes(dev):
    _, _, on_p, fr_p = sc.random_rolls(5 * L + 3, 11)
    sets = mixed_sets(5, seed=3)
    a, b = device_decode(dev, on_p, fr_p, sets), device_decode(dev, on_p, fr_p, sets)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def raw_decode(dev, on, fr, T=None, G=2, trans=None, ws_bytes=None, null=None):
    """rv_hmm_decode called directly on canary-filled outputs; returns (status, states, cost)."""
    from reconvat_amd import NoteHMM, _lib
    T = on.shape[0] if T is None else T
    need = _lib.load().rv_hmm_workspace_bytes(on.shape[0], 2)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    tables_h, trans_h = NoteHMM().tables()
    tables = torch.from_numpy(np.stack([tables_h, tables_h]).view(np.int16)).to(dev)
    trans_h = np.ascontiguousarray(np.stack([trans_h, trans_h]) if trans is None else np.asarray(trans, np.int32))
    states = torch.full((2, on.shape[0], 88), 7, dtype=torch.uint8, device=dev)
    cost = torch.full((2, 88), -7, dtype=torch.int64, device=dev)
    ptr = {'onsets': on.data_ptr(), 'frames': fr.data_ptr(), 'tables': tables.data_ptr(), 'trans': trans_h.ctypes.data,
           'states': states.data_ptr(), 'cost': cost.data_ptr(), 'workspace': ws.data_ptr()}
    if null:
        ptr[null] = None
    rc = _lib.invoke('rv_hmm_decode', ptr['onsets'], ptr['frames'], T, ptr['tables'], ptr['trans'], G, ptr['states'], ptr['cost'],
                     ptr['workspace'], need if ws_bytes is None else ws_bytes, _lib.stream())
    torch.cuda.synchronize()
    return rc, states.cpu().numpy(), cost.cpu().numpy()


def test_argument_errors(dev):
    from reconvat_amd import NoteHMM, _lib, hmm as nh
    lib = _lib.load()
    assert lib.rv_hmm_workspace_bytes(200, 2) > 0 and lib.rv_hmm_workspace_bytes(1 << 20, 16) > lib.rv_hmm_workspace_bytes(1 << 20, 15) > 0
    for T, G in ((0, 1), (-1, 1), ((1 << 20) + 1, 1), (200, 0), (200, 17), (200, -1)):
        assert lib.rv_hmm_workspace_bytes(T, G) == 0, (T, G)
    _, _, on_p, fr_p = sc.random_rolls(200, 3)
    on, fr = torch.from_numpy(on_p).to(dev), torch.from_numpy(fr_p).to(dev)
    need = lib.rv_hmm_workspace_bytes(200, 2)
    good = np.stack([NoteHMM().tables()[1]] * 2)

    def with_entry(g, j, v):
        bad = good.copy()
        bad[g, j] = v
        return bad
    cases = [dict(null=name) for name in ('onsets', 'frames', 'tables', 'trans', 'states', 'cost', 'workspace')]
    cases += [dict(T=0), dict(T=(1 << 20) + 1), dict(G=0), dict(G=17), dict(ws_bytes=need - 16), dict(ws_bytes=0)]
    cases += [dict(trans=with_entry(1, 7, -2)), dict(trans=with_entry(0, 11, 65536)), dict(trans=with_entry(1, 0, -1)),
              dict(trans=with_entry(0, 3, -1))]
    for kw in cases:
        rc, states, cost = raw_decode(dev, on, fr, **kw)
        assert rc != 0, kw
        assert np.all(states == 7) and np.all(cost == -7), kw           # nothing was launched
        assert 'rv_hmm_decode' in _lib.last_error(), (kw, _lib.last_error())
    rc, states, cost = raw_decode(dev, on, fr)
    assert rc == 0 and states.max() == 2 and cost.min() > 0 and np.array_equal(states[0], states[1])
    rc, states, cost = raw_decode(dev, on, fr, trans=with_entry(1, 4, 65535))      # the ends of the range are in
    assert rc == 0 and not np.array_equal(states[0], states[1])
    # the Python layer raises before it launches
    for bad in ([], [(NoteHMM().tables()[0], with_entry(0, 3, -1)[0])], [(NoteHMM().tables()[0][:5], good[0])]):
        with pytest.raises(ValueError):
            nh.viterbi_states_device(on, fr, bad)
    with pytest.raises(ValueError):
        nh.viterbi_states_device(on, fr[:100], [NoteHMM()])
    with pytest.raises(RuntimeError, match='HIP device only'):
        nh.viterbi_states_device(on.cpu(), fr, [NoteHMM()])


@pytest.mark.parametrize('m, g', [(1, 0), (3, 1)])
def test_extract_notes_hmm_device_equals_host(dev, m, g):
    from reconvat_amd import NoteHMM, decoding as md, hmm as nh
    _, _, on_p, fr_p = sc.random_rolls(3 * L + 11, 3)
    hmms = [NoteHMM(), NoteHMM(0.3, 0.5, 0.0, 0.0, 0.0), NoteHMM(0.5, 0.3, 1.0, 4.0, 2.0)]
    got = nh.extract_notes_hmm_device(torch.from_numpy(on_p).to(dev), torch.from_numpy(fr_p).to(dev), hmms, min_frames=m, bridge_gap=g)
    assert len(got) == len(hmms)
    counts = []
    for h, (gp, gi, painted) in zip(hmms, got):
        p, i = nh.extract_notes_hmm(on_p, fr_p, h, min_frames=m, bridge_gap=g)
        assert gp.shape == p.shape and gi.shape == i.shape and np.array_equal(gp, p) and np.array_equal(gi, i)
        want_roll = np.zeros(fr_p.shape, np.uint8)
        for t, f in enumerate(md.notes_to_frames(p, i, fr_p.shape)[1]):
            want_roll[t, f] = 1
        got_roll = painted.cpu().numpy()
        assert got_roll.dtype == np.uint8 and np.array_equal(got_roll, want_roll)
        counts.append(len(p))
    assert counts[0] > 20 and counts[1] > counts[0]


def test_evaluate_wo_velocity_device_equals_host(dev):
    from reconvat_amd import NoteHMM, evaluate as ev
    model, h = sc.StubModel(), NoteHMM(0.4, 0.5, 1.0, 2.0, 2.0)
    want = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4)), model, reconstruction=False, device_metrics=False, min_frames=2, hmm=h)
    got = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4), device=dev), model, reconstruction=False, device_metrics=True, min_frames=2, hmm=h)
    plain = ev.evaluate_wo_velocity(sc.stub_songs(130, (3, 4), device=dev), model, reconstruction=False, device_metrics=True, min_frames=2)
    assert list(got) == list(want) and 'metric/note/f1' in want and 'metric/frame/chroma_total_error' in want
    for k in want:
        assert len(got[k]) == len(want[k]) == 2
        for a, b in zip(got[k], want[k]):
            if k.startswith('metric/MusicNet/micro_avg_P'):
                assert abs(a - b) <= 1e-9, (k, a, b)
            else:
                assert a == b, (k, a, b)
    assert got['metric/note/precision'] != plain['metric/note/precision'] and got['metric/frame/precision'] != plain['metric/frame/precision']


def test_tune_hmm_device_equals_host(dev):
    from reconvat_amd import evaluate as ev, hmm as nh
    hmms = nh.hmm_grid([0.3, 0.5], [0.5], [0.0, 2.0], [0.0, 2.0], [1.0, 2.0, 4.0]) [:18]       # two device batches
    want = ev.tune_hmm(sc.stub_songs(130, (3, 4)), sc.StubModel(), hmms, device_metrics=False, bridge_gap=1)
    got = ev.tune_hmm(sc.stub_songs(130, (3, 4), device=dev), sc.StubModel(), hmms, device_metrics=True, bridge_gap=1)
    assert set(got['values']) == set(want['values']) == set(NAMES)
    for k in want['values']:
        assert np.array_equal(got['values'][k], want['values'][k]), k
    assert got['best_index'] == want['best_index'] and got['best_value'] == want['best_value'] > 0 and got['songs'] == 2
    assert len(np.unique(want['values']['note_f1'])) > 4


@pytest.fixture(scope='module')
def onset_model(dev):
    import reconvat_amd as ra
    from oracle import fixture as fx
    m = ra.UNet_Onset((2, 2), (2, 2), log=True, reconstruction=True, mode='imagewise', spec='Mel')
    m.load_state_dict(fx.fixture_params('onset', True))
    return m.to(dev).eval()


def test_transcribe2midi_with_the_hmm(dev, onset_model, tmp_path):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    from oracle import fixture as fx
    from reconvat_amd import NoteHMM, hmm as nh
    from reconvat_amd.evaluate import midi_to_hz
    from reconvat_amd.midi import parse_midi, save_midi
    audio = fx.fixture_audio(1, 64 * 512, 'L')[0]
    clip = tmp_path / 'clip.pt'
    torch.save({'audio': (audio * 32768.0).round().clamp(-32768, 32767).to(torch.int16)}, str(clip))
    with torch.no_grad():
        pred = onset_model.transcribe({'audio': tf.load_audio(str(clip)).to(dev).unsqueeze(0)})
    onset, frame = pred['onset'].squeeze(0).relu().cpu(), pred['frame'].squeeze(0).relu().cpu()
    # the weights are a fixture, not a trained model: thresholds from the posteriorgrams themselves, so that there are notes to decode
    thr_on, thr_fr = float(onset.flatten().quantile(0.8)), float(frame.flatten().quantile(0.8))
    # ... and switching at a small price: at 0.5 nats and above these 64 frames decode to notes that last to the end of the clip, and
    # the clean-up would have nothing to drop
    h = NoteHMM(thr_on, thr_fr, 0.0, 0.0, 0.125)
    p_all, i_all = nh.extract_notes_hmm(onset, frame, h)
    print('notes:', len(p_all), 'lengths:', np.diff(np.asarray(i_all).reshape(-1, 2), axis=1).ravel().tolist())
    p_est, i_est = nh.extract_notes_hmm(onset, frame, h, min_frames=2, bridge_gap=1)
    assert 0 < len(p_est) < len(p_all)
    tf.transcribe2midi([str(clip)], onset_model, dev, str(tmp_path / 'out'), min_frames=2, bridge_gap=1, hmm=h)
    scaling = 512 / 16000
    save_midi(str(tmp_path / 'want.mid'), np.array([midi_to_hz(21 + q) for q in p_est]), np.asarray(i_est) * scaling, [127] * len(p_est))
    got, want = parse_midi(str(tmp_path / 'out' / 'ReconVAT-clip.mid')), parse_midi(str(tmp_path / 'want.mid'))
    assert got.shape == want.shape == (len(p_est), 4) and np.array_equal(got, want)
