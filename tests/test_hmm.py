"""Viterbi note decoding, the host side: the definition in reconvat_amd/hmm.py against a brute force over all paths, its
tie rule, the chunked evaluation that csrc/hmm.hip implements restated in NumPy (matrix products in the (min, +) semiring, an int64
carry, back-pointers from the carried alpha, the map-composition backtrack) against the sequential one, NoteHMM's tables, hand-made
rolls, evaluate_wo_velocity(hmm=) / tune_hmm on stub songs, and the keys of the two scripts.  Every comparison is == on integers."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

import sweep_cases as sc
from reconvat_amd import NoteHMM, decoding as md, evaluate as ev, hmm as nh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = nh.INF


def random_set(rng, quanta=None, forbid=0.25):
    """Random tables and trans, forbidden entries included (init[0] and A[0][0] stay allowed).  ``quanta``: emissions are multiples of
    a few large values and trans comes from {-1, 0, 1000, 2000} -- many exact ties."""
    if quanta is None:
        tables = rng.randint(0, 65536, size=(6, 256)).astype(np.uint16)
        trans = rng.randint(0, 65536, size=12).astype(np.int32)
        trans[rng.rand(12) < forbid] = -1
    else:
        tables = (rng.randint(0, 4, size=(6, 256)) * rng.choice(quanta, size=(6, 256))).astype(np.uint16)
        trans = rng.choice([-1, 0, 1000, 2000], size=12).astype(np.int32)
    trans[0], trans[3] = max(trans[0], 0), max(trans[3], 0)
    return tables, trans


def path_cost(path, E, init, A):
    """Cost of one path of one key (E [3, T] int), INF if it takes a forbidden step."""
    c = init[path[0]] + E[path[0], 0]
    for t in range(1, len(path)):
        c = min(INF, c + A[path[t - 1], path[t]]) + E[path[t], t]
    return min(INF, c)


def emissions(onsets, frames, tables):
    wide = tables.astype(np.int64)
    return wide[:3][:, nh.quantise(onsets)] + wide[3:][:, nh.quantise(frames)]          # [3, T, 88]


def viterbi_chunked(onsets, frames, tables, trans, L):
    """The algorithm of csrc/hmm.hip in NumPy: chunk matrices in saturating int32 arithmetic, alpha carried in int64, every chunk run
    again from its true incoming alpha for the back-pointers, the chunk maps composed and walked backwards."""
    tables, init, A = nh._check_set(tables, trans)
    E = emissions(onsets, frames, tables)
    T, keys, S32 = E.shape[1], np.arange(88), 1 << 29
    first = np.full((3, 3), INF, np.int64)
    first[0] = init                                                     # frame 0: a step from a virtual OFF frame under init
    nc = -(-T // L)
    sat = lambda M: np.where(M >= INF, S32, M).astype(np.int64)
    mats = []
    for c in range(nc):
        M = np.where(np.eye(3, dtype=bool), 0, S32)[:, :, None].repeat(88, axis=2).astype(np.int64)
        for t in range(c * L, min(T, (c + 1) * L)):
            F = sat(first if t == 0 else A)
            M = np.minimum(S32, (M[:, :, None, :] + F[None, :, :, None]).min(axis=1) + E[None, :, t, :])
            assert M.max() < 2 ** 31
        mats.append(M)
    alpha = np.stack([np.zeros(88, np.int64), np.full(88, INF), np.full(88, INF)])
    entering = []
    for M in mats:                                                      # the int64 carry
        entering.append(alpha)
        cand = np.where(M >= S32, INF, np.minimum(INF, alpha[:, None, :] + M))
        alpha = cand.min(axis=0)
    cost, last = alpha.min(axis=0), alpha.argmin(axis=0)
    bp, maps = np.zeros((T, 3, 88), np.int64), []
    for c in range(nc):
        a, m = entering[c], np.arange(3)[:, None].repeat(88, axis=1)
        for t in range(c * L, min(T, (c + 1) * L)):
            cand = a[:, None, :] + (first if t == 0 else A)[:, :, None]          # unclamped, as on the device
            bp[t] = cand.argmin(axis=0)
            a = np.minimum(INF, cand.min(axis=0) + E[:, t])
            m = m[bp[t], keys[None, :]]
        maps.append(m)
    ends, s = [None] * nc, last
    for c in range(nc - 1, -1, -1):
        ends[c] = s
        s = maps[c][s, keys]
    states = np.zeros((T, 88), np.uint8)
    for c in range(nc):
        s = ends[c]
        for t in range(min(T, (c + 1) * L) - 1, c * L - 1, -1):
            states[t] = s
            s = bp[t, s, keys]
    return states, cost


def test_quantise_edges():
    one, tiny = np.float32(1), np.float32(1) / np.float32(256)
    x = np.array([-1, -0.0, 0, np.nextafter(tiny, np.float32(0)), tiny, 0.5, np.nextafter(one, np.float32(0)), 1, 2, np.inf, np.nan],
                 dtype=np.float32)
    with np.errstate(invalid='ignore'):
        q = nh.quantise(x)
    assert q.dtype == np.uint8 and q.tolist() == [0, 0, 0, 0, 1, 128, 255, 255, 255, 255, 0]
    assert nh.quantise(np.float32(0.7)) == int(np.floor(np.float32(0.7) * np.float32(256)))
    assert nh.quantise(np.zeros((4, 88), np.float32)).shape == (4, 88)


def test_tables_and_trans_layout():
    tables, trans = NoteHMM().tables()
    assert tables.dtype == np.uint16 and tables.shape == (6, 256) and trans.dtype == np.int32 and trans.shape == (12,)
    on, off = tables[1], tables[0]
    assert (on[0], on[127], on[255]) == (200, 22, 0)
    assert np.array_equal(off, on[::-1])                                # theta = 0.5: the two costs mirror each other
    assert np.array_equal(tables[2], off) and np.array_equal(tables[3], off) and np.array_equal(tables[4], on) and np.array_equal(tables[5], on)
    assert trans.tolist() == [0, 64, -1, 0, 64, -1, 64, 0, 0, 64, 64, 0]
    tables, trans = NoteHMM(0.3, 0.7, note_on=1.0, note_off=0.25, restrike=2047, use_onsets=False).tables()
    assert not tables[:3].any() and trans.tolist() == [0, 32, -1, 0, 32, -1, 8, 0, 0, 8, 65504, 0]
    assert tables[4][int(0.7 * 256)] in (22, 23) and tables.max() <= 4095 and np.all(np.diff(tables[4].astype(int)) <= 0)
    assert NoteHMM(0.01, 0.99).tables()[0].max() <= 4095
    for bad in (dict(onset_threshold=0.0), dict(frame_threshold=1.0), dict(onset_threshold=float('nan')), dict(note_on=-0.5),
                dict(note_off=2048), dict(restrike=float('inf')), dict(use_onsets=1), dict(frame_threshold='0.5'), dict(note_on=True)):
        with pytest.raises(ValueError):
            NoteHMM(**bad)
    grid = nh.hmm_grid([0.3, 0.5], 0.5, [0, 1, 2], [2], [2, 4])
    assert len(grid) == 12 and grid[0] == NoteHMM(0.3, 0.5, 0, 2, 2) and grid[1] == NoteHMM(0.3, 0.5, 0, 2, 4) and grid[-1] == NoteHMM(0.5, 0.5, 2, 2, 4)


def test_bad_sets_raise():
    tables, trans = NoteHMM().tables()
    z = np.zeros((3, 88), np.float32)
    for j, v in ((0, -1), (3, -1), (5, -2), (7, 65536)):
        bad = trans.copy()
        bad[j] = v
        with pytest.raises(ValueError):
            nh.viterbi_states(z, z, tables, bad)
    with pytest.raises(ValueError):
        nh.viterbi_states(z, z, tables[:5], trans)
    with pytest.raises(ValueError):
        nh.viterbi_states(z, z[:2], tables, trans)
    with pytest.raises(ValueError):
        nh.viterbi_states(z[:0], z[:0], tables, trans)


@pytest.mark.parametrize('T', [1, 2, 3, 6])
def test_definition_equals_brute_force(T):
    rng = np.random.RandomState(100 + T)
    finite_costs = 0
    for case in range(6):
        tables, trans = random_set(rng, quanta=None if case % 2 == 0 else [1000, 3000])
        onsets, frames = rng.rand(T, 88).astype(np.float32), rng.rand(T, 88).astype(np.float32)
        states, cost = nh.viterbi_states(onsets, frames, tables, trans)
        assert states.dtype == np.uint8 and states.shape == (T, 88) and cost.dtype == np.int64 and cost.shape == (88,)
        _, init, A = nh._check_set(tables, trans)
        E = emissions(onsets, frames, tables)
        for key in (0, 17, 40, 63, 87):
            costs = {path: path_cost(path, E[:, :, key], init, A) for path in itertools.product(range(3), repeat=T)}
            got = tuple(int(s) for s in states[:, key])
            assert cost[key] == min(costs.values()) < INF                     # the minimum ...
            assert costs[got] == cost[key]                                      # ... attained by the returned path, which therefore
            assert init[got[0]] < INF and all(A[a, b] < INF for a, b in zip(got, got[1:]))      # takes no forbidden step
            finite_costs += sum(c < INF for c in costs.values())
    assert finite_costs > 30


def test_tie_rule():
    rng = np.random.RandomState(5)
    onsets, frames = rng.rand(50, 88).astype(np.float32), rng.rand(50, 88).astype(np.float32)
    states, cost = nh.viterbi_states(onsets, frames, np.zeros((6, 256), np.uint16), np.zeros(12, np.int32))
    assert not states.any() and not cost.any()                          # everything ties: the lowest state everywhere
    tables = rng.randint(0, 3, size=(6, 256)).astype(np.uint16) * 100
    tables[2], tables[5] = tables[1], tables[4]                         # states 1 and 2 cost the same everywhere ...
    trans = np.array([0, 50, 50, 0, 50, 50, 50, 0, 0, 50, 0, 0], np.int32)      # ... and are entered and left at the same price
    states, _ = nh.viterbi_states(onsets, frames, tables, trans)
    assert (states == 1).any() and not (states == 2).any()
    for L in (1, 7):
        assert np.array_equal(viterbi_chunked(onsets, frames, tables, trans, L)[0], states)


@pytest.mark.parametrize('L', [1, 7, 64])
def test_chunked_evaluation_equals_the_sequential_one(L):
    rng = np.random.RandomState(L)
    for case, T in enumerate((1, 2, L, L + 1, 3 * L + 2, 150)):
        quanta = [[1000, 3000], None, [500, 20000]][case % 3]
        tables, trans = random_set(rng, quanta=quanta)
        _, _, on_p, fr_p = sc.random_rolls(T, 20 + case)
        want = nh.viterbi_states(on_p, fr_p, tables, trans)
        got = viterbi_chunked(on_p, fr_p, tables, trans, L)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (L, T)
    _, _, on_p, fr_p = sc.random_rolls(150, 3)
    want = nh.viterbi_states(on_p, fr_p, *NoteHMM().tables())
    got = viterbi_chunked(on_p, fr_p, *NoteHMM().tables(), L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def notes_of(onset, frame, model, **kw):
    p, i = nh.extract_notes_hmm(onset, frame, model, **kw)
    return [(int(s), int(q), int(e)) for q, (s, e) in zip(p, np.asarray(i).reshape(-1, 2))]


def test_hand_made_rolls():
    free = dict(note_on=0.0, note_off=0.0, restrike=0.0)
    # a two-frame dropout to 0.3 inside a note on the frame roll alone: bridged at the default penalties, not at penalty 0
    frame = np.zeros((40, 88), np.float32)
    frame[5:30, 40] = 1.0
    frame[14:16, 40] = 0.3
    assert notes_of(frame, frame, NoteHMM(use_onsets=False)) == [(5, 40, 30)]
    assert notes_of(frame, frame, NoteHMM(use_onsets=False, **free)) == [(5, 40, 14), (16, 40, 30)]
    # a one-frame blip at 0.7: dropped at the default penalties, kept at penalty 0
    frame = np.zeros((40, 88), np.float32)
    frame[20, 33] = 0.7
    assert notes_of(frame, frame, NoteHMM(use_onsets=False)) == []
    assert notes_of(frame, frame, NoteHMM(use_onsets=False, **free)) == [(20, 33, 21)]
    # a second onset peak inside a held note: a re-strike, two notes that share their end
    onset, frame = np.zeros((40, 88), np.float32), np.zeros((40, 88), np.float32)
    frame[5:30, 60] = 1.0
    onset[5, 60] = onset[15, 60] = 1.0
    assert notes_of(onset, frame, NoteHMM()) == [(5, 60, 30), (15, 60, 30)]
    states, _ = nh.viterbi_states(onset, frame, *NoteHMM().tables())
    assert states[:, 60].tolist() == [0] * 5 + [1] + [2] * 9 + [1] + [2] * 14 + [0] * 10
    on_roll, fr_roll = nh.states_to_rolls(states)
    assert on_roll.dtype == fr_roll.dtype == np.float32 and on_roll.sum() == 2 and fr_roll.sum() == 25


def test_random_rolls_use_all_states():
    _, _, on_p, fr_p = sc.random_rolls(200, 3)
    states, cost = nh.viterbi_states(on_p, fr_p, *NoteHMM().tables())
    assert set(np.unique(states)) == {0, 1, 2} and cost.min() > 0
    default = notes_of(on_p, fr_p, NoteHMM())
    free = notes_of(on_p, fr_p, NoteHMM(note_on=0.0, note_off=0.0, restrike=0.0))
    print('notes at the default penalties:', len(default), ' at penalty 0:', len(free))
    assert len(default) >= 40 and default != free
    cleaned = notes_of(on_p, fr_p, NoteHMM(note_on=0.0, note_off=0.0, restrike=0.0), min_frames=3, bridge_gap=1)
    assert 0 < len(cleaned) < len(free)
    # tensors are taken as arrays are
    assert notes_of(torch.from_numpy(on_p), torch.from_numpy(fr_p), NoteHMM()) == default


NAMES = {'note_precision': 'metric/note/precision', 'note_recall': 'metric/note/recall', 'note_f1': 'metric/note/f1',
         'note_with_offsets_precision': 'metric/note-with-offsets/precision', 'note_with_offsets_recall': 'metric/note-with-offsets/recall',
         'note_with_offsets_f1': 'metric/note-with-offsets/f1', 'frame_precision': 'metric/frame/precision',
         'frame_recall': 'metric/frame/recall', 'frame_f1': 'metric/frame/f1'}


def test_evaluate_and_tune_hmm_on_stub_songs():
    songs, model = sc.stub_songs(40, seeds=(3, 4)), sc.StubModel()
    calls = []

    class Counting(sc.StubModel):
        def run_on_batch(self, label, *args):
            calls.append(label['path'])
            return super().run_on_batch(label, *args)
    hmms = [NoteHMM(), NoteHMM(0.3, 0.5, 0.0, 0.0, 0.0), NoteHMM(0.5, 0.3, 1.0, 4.0, 2.0)]
    res = ev.tune_hmm(songs, Counting(), hmms, device_metrics=False, min_frames=2, bridge_gap=1)
    assert calls == ['stub/3', 'stub/4']                                # one forward per song, however many sets
    assert set(res) == {'hmms', 'values', 'criterion', 'best_index', 'best', 'best_value', 'songs'}
    assert set(res['values']) == set(NAMES) and res['songs'] == 2 and res['hmms'] == hmms and res['criterion'] == 'note_f1'
    plain = ev.evaluate_wo_velocity(songs, model, reconstruction=False, device_metrics=False, min_frames=2, bridge_gap=1)
    differs = 0
    for n, h in enumerate(hmms):
        # the two thresholds are unused: the model carries its own
        want = ev.evaluate_wo_velocity(songs, model, 0.9, 0.1, reconstruction=False, device_metrics=False, min_frames=2, bridge_gap=1, hmm=h)
        assert set(want) == set(plain)
        for k, key in NAMES.items():
            assert res['values'][k].dtype == np.float64 and res['values'][k][n] == np.mean(want[key]), (n, k)
        differs += want['metric/note/precision'] != plain['metric/note/precision']
    assert differs == len(hmms)
    best = int(np.argmax(res['values']['note_f1']))
    assert res['best_index'] == best and res['best'] is hmms[best] and res['best_value'] == res['values']['note_f1'][best] > 0
    # ties go to the lowest index
    top = int(np.argmax(res['values']['frame_f1']))
    twice = ev.tune_hmm(songs, model, [hmms[top - 1], hmms[top], hmms[top]], criterion='frame_f1', device_metrics=False)
    assert twice['best_index'] == 1 and twice['values']['frame_f1'][1] == twice['values']['frame_f1'][2] > twice['values']['frame_f1'][0]
    # frame-only decoding
    frame_only = NoteHMM(use_onsets=False)
    got = ev.tune_hmm(songs, model, [frame_only], onset=False, device_metrics=False)
    want = ev.evaluate_wo_velocity(songs, model, reconstruction=False, onset=False, device_metrics=False, hmm=frame_only)
    for k, key in NAMES.items():
        assert got['values'][k][0] == np.mean(want[key]), k


def test_argument_errors():
    songs, model = sc.stub_songs(40, seeds=(3,)), sc.StubModel()
    with pytest.raises(ValueError):
        ev.evaluate_wo_velocity([], None, reconstruction=False, onset=False, hmm=NoteHMM())       # before any song is touched
    with pytest.raises(TypeError):
        ev.evaluate_wo_velocity([], None, reconstruction=False, hmm=(0.5, 0.5))
    with pytest.raises(ValueError):
        ev.evaluate_wo_velocity(songs, model, reconstruction=False, hmm=NoteHMM(), min_frames=0)
    for bad in (dict(hmms=[]), dict(hmms=[NoteHMM()] * 257), dict(hmms=[NoteHMM()], criterion='loss'), dict(hmms=[NoteHMM()], onset=False),
                dict(hmms=[NoteHMM()], bridge_gap=32)):
        with pytest.raises(ValueError):
            ev.tune_hmm(songs, model, device_metrics=False, **bad)
    with pytest.raises(TypeError):
        ev.tune_hmm(songs, model, [NoteHMM().tables()], device_metrics=False)
    with pytest.raises(ValueError):
        ev.tune_hmm([], model, [NoteHMM()], device_metrics=False)
    z = torch.zeros(8, 88)
    with pytest.raises(RuntimeError, match='HIP device only'):          # no fallback
        nh.viterbi_states_device(z, z, [NoteHMM()])
    with pytest.raises(RuntimeError, match='HIP device only'):
        nh.extract_notes_hmm_device(z, z, [NoteHMM()])
    assert nh.DEVICE_CHUNK_FRAMES == 64 and md.DEVICE_TILE_FRAMES == 64


class FakeModel:
    def __init__(self, name):
        self.name, self.loaded = name, None

    def load_state_dict(self, state):
        self.loaded = state

    def to(self, device):
        return self

    def eval(self):
        return self


def fake_models(monkeypatch, tf):
    states = {'onset.pt': {'transcriber.linear_onset.weight': 0, 'transcriber.linear_feature.weight': 0},
              'frame.pt': {'transcriber.linear_feature.weight': 0}}
    monkeypatch.setattr(tf.ra, 'UNet', lambda *a, **k: FakeModel('UNet'))
    monkeypatch.setattr(tf.ra, 'UNet_Onset', lambda *a, **k: FakeModel('UNet_Onset'))
    monkeypatch.setattr(tf.torch, 'load', lambda path, **k: states[path])


def test_transcribe_files_decoder_keys(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    (tmp_path / 'a.wav').write_bytes(b'')
    calls = []
    fake_models(monkeypatch, tf)
    monkeypatch.setattr(tf, 'transcribe2midi', lambda files, model, device, out, **kw: calls.append((model, kw)))
    base = ['with', 'device=cpu', f'input={tmp_path}', f'output={tmp_path}']
    tf.main(base + ['weight=onset.pt'])
    tf.main(base + ['weight=onset.pt', 'decoder=threshold', 'note_on=3.0'])
    tf.main(base + ['weight=onset.pt', 'decoder=hmm', 'onset_threshold=0.3', 'note_off=1.5', 'min_frames=2'])
    tf.main(base + ['weight=frame.pt', 'decoder=hmm'])
    thr = {'onset_threshold': 0.5, 'frame_threshold': 0.5}
    assert calls[0][1] == thr and calls[1][1] == thr                    # the new keyword goes on only with decoder=hmm
    assert calls[2][1] == dict(onset_threshold=0.3, frame_threshold=0.5, min_frames=2, hmm=NoteHMM(0.3, 0.5, 2.0, 1.5, 2.0, use_onsets=True))
    assert calls[3][1] == dict(thr, hmm=NoteHMM(use_onsets=False))
    with pytest.raises(SystemExit, match='decoder'):
        tf.main(base + ['decoder=viterbi'])


def test_tune_hmm_script_keys(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    import tune_hmm as th
    with pytest.raises(SystemExit, match='unknown keys'):
        th.main(['with', 'device=cpu', 'cleanups=[[1,0]]'])
    seen = {}

    def fake_tune(data, model, hmms, **kw):
        seen.update(kw, hmms=hmms)
        return ev.tune_hmm(sc.stub_songs(40, seeds=(3,)), sc.StubModel(), hmms, criterion=kw['criterion'], device_metrics=False,
                           min_frames=kw['min_frames'], bridge_gap=kw['bridge_gap'])
    fake_models(monkeypatch, tf)
    monkeypatch.setattr(th, 'prepare_VAT_dataset', lambda **kw: (None, None, [], None))
    monkeypatch.setattr(th, 'tune_hmm', fake_tune)
    out = tmp_path / 'hmm.json'
    res = th.main(['with', 'device=cpu', 'weight=onset.pt', 'onset_thresholds=[0.3,0.5]', 'frame_thresholds=[0.5]', 'note_on=[0,2]',
                   'note_off=[1]', 'restrike=[2,4]', 'criterion=frame_f1', 'bridge_gap=1', f'output={out}'])
    assert seen['hmms'] == nh.hmm_grid([0.3, 0.5], [0.5], [0, 2], [1], [2, 4]) and len(seen['hmms']) == 8
    assert seen['onset'] is True and seen['device_metrics'] is False and (seen['min_frames'], seen['bridge_gap']) == (1, 1)
    saved = json.loads(out.read_text())
    assert saved['best_index'] == res['best_index'] and saved['best'] == res['best'].as_dict() and saved['criterion'] == 'frame_f1'
    assert saved['values']['frame_f1'] == res['values']['frame_f1'].tolist() and len(saved['hmms']) == 8
    assert NoteHMM(**saved['best']) == res['best']
    # a checkpoint without an onset head: frame-only sets; the default output path
    monkeypatch.chdir(tmp_path)
    th.main(['with', 'device=cpu', 'weight=frame.pt', 'onset_thresholds=[0.5]', 'frame_thresholds=[0.5]', 'note_on=[2]'])
    assert seen['onset'] is False and all(not h.use_onsets for h in seen['hmms']) and (tmp_path / 'frame.pt.hmm.json').exists()
