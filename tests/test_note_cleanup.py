"""Note clean-up in the decoder, the host side: extract_notes_wo_velocity with min_frames / bridge_gap against a
frame-by-frame restatement of the definition, the two properties the device kernels rely on, sweep_counts_host against a brute-force
count with scipy's maximum matching (and "candidates in time order" against that matching), tune_thresholds over several clean-up
pairs against evaluate_wo_velocity called pair by pair, the argument ranges, and the new keys of the two scripts."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import sweep_cases as sc
from test_threshold_sweep import ON_THR, FR_THR, assert_same_counts, hits_brute, in_time_order, max_matching, t
from reconvat_amd import decoding as md, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEANUPS = [(1, 0), (2, 0), (1, 2), (3, 1), (5, 3), (32, 31)]
RULES = ['rule1', 'rule2']


def bridge_brute(act, g):
    """One pitch: every maximal inactive run of at most g frames with an active frame directly before and after it becomes active."""
    out, T, s = act.copy(), len(act), 0
    while s < T:
        if act[s]:
            s += 1
            continue
        e = s
        while e < T and not act[e]:
            e += 1
        if s > 0 and e < T and e - s <= g:
            out[s:e] = True
        s = e
    return out


def decode_brute(onset, frame, thr_on, thr_fr, rule, m=1, g=0):
    """Kept notes [(start, pitch, end)] in (start, pitch) order, the painted roll, and the bridged activity, from the definition."""
    T = onset.shape[0]
    on, fr = onset > np.float32(thr_on), frame > np.float32(thr_fr)
    notes, roll, bridged = [], np.zeros((T, 88), bool), np.zeros((T, 88), bool)
    for p in range(88):
        act = bridge_brute(on[:, p] | fr[:, p], g)
        bridged[:, p] = act
        for s in range(T):
            if on[s, p] and not (s > 0 and on[s - 1, p]) and (rule == 'rule2' or fr[s, p]):     # the unbridged rolls decide a start
                e = s
                while e < T and act[e]:
                    e += 1
                if e - s >= m:
                    notes.append((s, p, e))
                    roll[s:e, p] = True
    return sorted(notes), roll, bridged


def decode_host(onset, frame, thr_on, thr_fr, rule, **kw):
    pitches, intervals = md.extract_notes_wo_velocity(*t(onset, frame), thr_on, thr_fr, rule=rule, **kw)
    _, freqs = md.notes_to_frames(pitches, intervals, frame.shape)
    roll = np.zeros(frame.shape, bool)
    for i, f in enumerate(freqs):
        roll[i, f] = True
    return [(int(s), int(p), int(e)) for p, (s, e) in zip(pitches, np.asarray(intervals).reshape(-1, 2))], roll


@pytest.fixture(scope='module')
def inputs():
    return {40: sc.random_rolls(40, 11, density=0.12), 200: sc.random_rolls(200, 3)}


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('T', [40, 200])
def test_definition_equals_brute_force(inputs, T, rule):
    _, _, on_p, fr_p = inputs[T]
    kept_somewhere = dropped_somewhere = 0
    for x in ON_THR:
        for y in FR_THR:
            plain = decode_host(on_p, fr_p, x, y, rule)
            for m, g in CLEANUPS:
                got_notes, got_roll = decode_host(on_p, fr_p, x, y, rule, min_frames=m, bridge_gap=g)
                want_notes, want_roll, _ = decode_brute(on_p, fr_p, x, y, rule, m, g)
                assert got_notes == want_notes, (x, y, m, g)
                assert np.array_equal(got_roll, want_roll), (x, y, m, g)
                if (m, g) == (1, 0):
                    assert got_notes == plain[0] and np.array_equal(got_roll, plain[1])
                kept_somewhere += len(got_notes) > 0
                dropped_somewhere += len(got_notes) < len(plain[0])
    assert kept_somewhere and dropped_somewhere


def test_defaults_are_the_old_function_bit_for_bit(inputs):
    _, _, on_p, fr_p = inputs[200]
    for rule in RULES:
        a = md.extract_notes_wo_velocity(*t(on_p, fr_p), 0.5, 0.5, rule=rule)
        b = md.extract_notes_wo_velocity(*t(on_p, fr_p), 0.5, 0.5, rule=rule, min_frames=1, bridge_gap=0)
        for u, v in zip(a, b):
            assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)
    z = np.zeros((5, 88), np.float32)                                   # no note at all: the two empty arrays, as before
    p, i = md.extract_notes_wo_velocity(*t(z, z), min_frames=2, bridge_gap=1)
    assert p.shape == (0,) and i.shape == (0,)


def test_inputs_exercise_both_options(inputs):
    """Values of the CPU prototype at T = 40, rule2: a test that compares nothing cannot pass."""
    _, _, on_p, fr_p = inputs[40]
    n_est, frame_est = {}, {}
    for mg in [(1, 0), (2, 0), (1, 2)]:
        for x in ON_THR:
            for y in FR_THR:
                notes, roll = decode_host(on_p, fr_p, x, y, 'rule2', min_frames=mg[0], bridge_gap=mg[1])
                n_est[mg, x, y], frame_est[mg, x, y] = len(notes), int(roll.sum())
    grid = [(x, y) for x in ON_THR for y in FR_THR]
    assert sum(n_est[(2, 0), x, y] != n_est[(1, 0), x, y] for x, y in grid) >= 4
    assert (n_est[(1, 0), 0.5, 0.5], n_est[(2, 0), 0.5, 0.5]) == (131, 57)
    assert all(frame_est[(1, 2), x, y] > frame_est[(1, 0), x, y] for x, y in grid)
    assert (frame_est[(1, 0), 0.5, 0.5], frame_est[(1, 2), 0.5, 0.5]) == (353, 412)
    assert all(n_est[(1, 2), x, y] == n_est[(1, 0), x, y] for x, y in grid)    # bridging never adds or removes a start


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('T', [40, 200])
def test_the_two_properties_the_kernels_rely_on(inputs, T, rule):
    _, _, on_p, fr_p = inputs[T]
    runs_seen = dropped_runs = 0
    for x, y in ((0.5, 0.5), (0.3, 0.3)):
        for m, g in CLEANUPS:
            kept, roll = decode_host(on_p, fr_p, x, y, rule, min_frames=m, bridge_gap=g)
            every, _, act = decode_brute(on_p, fr_p, x, y, rule, 1, g)             # all starts, ends in the bridged activity
            kept = set(kept)
            for p in range(88):
                starts = [n for n in every if n[1] == p]
                s = 0
                while s < T:
                    if not act[s, p]:
                        assert not roll[s, p]
                        s += 1
                        continue
                    e = s
                    while e < T and act[e, p]:
                        e += 1
                    inside = [n for n in starts if s <= n[0] < e]
                    # 1. all notes of one active run end with the run; the run is painted, from its first start, iff that first note is kept
                    assert all(n[2] == e for n in inside)
                    want = np.zeros(e - s, bool)
                    if inside and inside[0] in kept:
                        want[inside[0][0] - s:] = True
                    assert np.array_equal(roll[s:e, p], want), (p, s, e, m, g)
                    assert all(n not in kept for n in inside) or inside[0] in kept
                    runs_seen += bool(inside)
                    dropped_runs += bool(inside) and inside[0] not in kept
                    # 2. a start at least m - 1 frames behind a frame that is still active is kept, whatever comes later -- and only such a start
                    for n in inside:
                        assert (n in kept) == (n[0] + m - 1 < e), (n, m, e)
                    s = e
    assert runs_seen > 20 and dropped_runs > 5


def counts_brute(rolls, on_thr, fr_thr, rule, m, g):
    """The sweep counters from the definition: the labels decoded without clean-up, the estimate with it; maximum matchings by scipy on
    the float64 candidate graph.  Also checks that candidates taken in time order reach the maximum."""
    on_r, fr_r, on_p, fr_p = rolls
    ref, ref_roll, _ = decode_brute(on_r, fr_r, 0.5, 0.5, rule)
    out = {k: np.zeros((len(on_thr), len(fr_thr)), np.int64) for k in ev.SWEEP_KEYS}
    for a, x in enumerate(on_thr):
        for b, y in enumerate(fr_thr):
            est, est_roll, _ = decode_brute(on_p, fr_p, x, y, rule, m, g)
            for key, offsets in (('matched', False), ('matched_with_offsets', True)):
                edges = hits_brute(ref, est, offsets)
                out[key][a, b] = max_matching(edges, len(ref), len(est))
                assert in_time_order(ref, est, edges) == out[key][a, b], (key, x, y, m, g)
            out['n_est'][a, b] = len(est)
            out['frame_tp'][a, b] = int((ref_roll & est_roll).sum())
            out['frame_est'][a, b] = int(est_roll.sum())
    out['n_ref'], out['frame_ref'] = len(ref), int(ref_roll.sum())
    return out


@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('T', [40, 200])
def test_host_sweep_equals_brute_force(inputs, T, rule):
    plain = ev.sweep_counts_host(*t(*inputs[T]), ON_THR, FR_THR, rule=rule)
    differs = 0
    for m, g in CLEANUPS:
        got = ev.sweep_counts_host(*t(*inputs[T]), ON_THR, FR_THR, rule=rule, min_frames=m, bridge_gap=g)
        assert_same_counts(got, counts_brute(inputs[T], ON_THR, FR_THR, rule, m, g))
        assert got['n_ref'] == plain['n_ref'] and got['frame_ref'] == plain['frame_ref']     # the labels are never cleaned up
        if (m, g) == (1, 0):
            assert_same_counts(got, plain)
        differs += any(not np.array_equal(got[k], plain[k]) for k in ev.SWEEP_KEYS)
    assert differs == len(CLEANUPS) - 1
    if T == 40 and rule == 'rule2':                                     # the issue's figures at 0.5 / 0.5
        got = ev.sweep_counts_host(*t(*inputs[T]), [0.5], [0.5], rule=rule, min_frames=2)
        assert (plain['n_est'][1, 0], plain['matched'][1, 0]) == (131, 22) and (got['n_est'][0, 0], got['matched'][0, 0]) == (57, 17)


@pytest.mark.parametrize('mg', [(2, 1), (3, 2), (4, 0)])
def test_in_time_order_is_maximum_on_the_chain(mg):
    rolls = sc.chain_rolls()
    want = counts_brute(rolls, [0.5], [0.5], 'rule2', *mg)              # asserts time order == maximum, with and without offsets
    got = ev.sweep_counts_host(*t(*rolls), [0.5], [0.5], rule='rule2', min_frames=mg[0], bridge_gap=mg[1])
    assert_same_counts(got, want)
    assert want['matched'][0, 0] > 10 and want['n_est'][0, 0] > 10


NAMES = {'note_precision': 'metric/note/precision', 'note_recall': 'metric/note/recall', 'note_f1': 'metric/note/f1',
         'note_with_offsets_precision': 'metric/note-with-offsets/precision', 'note_with_offsets_recall': 'metric/note-with-offsets/recall',
         'note_with_offsets_f1': 'metric/note-with-offsets/f1', 'frame_precision': 'metric/frame/precision',
         'frame_recall': 'metric/frame/recall', 'frame_f1': 'metric/frame/f1'}
OLD_KEYS = {'onset_thresholds', 'frame_thresholds', 'grid', 'criterion', 'best_index', 'onset_threshold', 'frame_threshold', 'best_value',
            'songs'}


def test_tune_thresholds_over_cleanups():
    songs, model = sc.stub_songs(40, seeds=(3, 4)), sc.StubModel()
    cleanups = [(2, 1), (1, 0), (3, 1)]
    calls = []

    class Counting(sc.StubModel):
        def run_on_batch(self, label, *args):
            calls.append(label['path'])
            return super().run_on_batch(label, *args)
    res = ev.tune_thresholds(songs, Counting(), ON_THR, FR_THR, device_metrics=False, cleanups=cleanups)
    assert calls == ['stub/3', 'stub/4']                                # one forward per song, however many pairs
    assert set(res) == OLD_KEYS | {'cleanups', 'grids', 'best_cleanup', 'min_frames', 'bridge_gap'}
    assert res['cleanups'] == cleanups and len(res['grids']) == 3
    for (m, g), grid in zip(cleanups, res['grids']):
        assert set(grid) == set(NAMES)
        for a, x in enumerate(ON_THR):
            for b, y in enumerate(FR_THR):
                want = ev.evaluate_wo_velocity(songs, model, x, y, reconstruction=False, device_metrics=False, min_frames=m, bridge_gap=g)
                for k, key in NAMES.items():
                    assert grid[k][a, b] == np.mean(want[key]), (m, g, k, a, b)
    assert not np.array_equal(res['grids'][0]['note_f1'], res['grids'][1]['note_f1'])
    c, (a, b) = res['best_cleanup'], res['best_index']
    tops = [grid['note_f1'].max() for grid in res['grids']]
    assert c == int(np.argmax(tops)) and res['best_value'] == max(tops) == res['grids'][c]['note_f1'][a, b] > 0
    assert res['grid'] is res['grids'][c] and (res['min_frames'], res['bridge_gap']) == cleanups[c]
    assert (a, b) == ev.best_threshold_index(res['grid']['note_f1'], ON_THR, FR_THR)
    # the default: today's dictionary under today's keys
    old = ev.tune_thresholds(songs, model, ON_THR, FR_THR, device_metrics=False)
    assert (old['cleanups'], old['best_cleanup'], old['min_frames'], old['bridge_gap']) == ([(1, 0)], 0, 1, 0)
    for k, v in res['grids'][1].items():
        assert np.array_equal(old['grid'][k], v)
    want = ev.evaluate_wo_velocity(songs, model, ON_THR[0], FR_THR[1], reconstruction=False, device_metrics=False)
    assert old['grid']['note_f1'][0, 1] == np.mean(want['metric/note/f1']) and old['songs'] == 2
    assert old['best_index'] == ev.best_threshold_index(old['grid']['note_f1'], ON_THR, FR_THR)
    assert old['best_value'] == old['grid']['note_f1'].max()


def test_tie_goes_to_the_earliest_cleanup_then_to_the_threshold_rule():
    """Estimate = labels, every note 3 frames or longer and no gap: (1, 0), (3, 0) and (2, 5) all decode the labels at every pair;
    (4, 0) loses the 3-frame note."""
    on_r, fr_r, _, _ = sc.blank(40)
    for pitch, start, end in ((30, 2, 5), (40, 10, 20), (50, 30, 40)):
        sc.paint(on_r, fr_r, pitch, start, end)
    song = {'path': 'x', 'onset': torch.from_numpy(on_r), 'frame': torch.from_numpy(fr_r), 'pred_onset': torch.from_numpy(on_r),
            'pred_frame': torch.from_numpy(fr_r)}
    res = ev.tune_thresholds([song], sc.StubModel(), [0.2, 0.6, 0.4], [0.8, 0.5], device_metrics=False,
                             cleanups=[(4, 0), (3, 0), (1, 0), (2, 5)])
    assert np.all(res['grids'][0]['note_f1'] < 1.0) and all(np.all(g['note_f1'] == 1.0) for g in res['grids'][1:])
    assert res['best_cleanup'] == 1 and (res['min_frames'], res['bridge_gap']) == (3, 0)
    assert res['best_index'] == (1, 1)                                 # as without clean-up: nearest (0.5, 0.5), then the lower index


def test_argument_ranges_raise(inputs):
    rolls = t(*inputs[40])
    songs, model = sc.stub_songs(40, seeds=(3,)), sc.StubModel()
    for bad in (dict(min_frames=0), dict(min_frames=33), dict(bridge_gap=-1), dict(bridge_gap=32), dict(min_frames=1.5),
                dict(bridge_gap=2.0), dict(min_frames=True)):
        with pytest.raises(ValueError):
            md.extract_notes_wo_velocity(rolls[2], rolls[3], **bad)
        with pytest.raises(ValueError):
            ev.sweep_counts_host(*rolls, [0.5], [0.5], **bad)
        with pytest.raises(ValueError):
            ev.evaluate_wo_velocity(songs, model, reconstruction=False, **bad)
        with pytest.raises(ValueError):
            ev.evaluate_wo_velocity([], None, reconstruction=False, **bad)                # checked before any song is touched
        with pytest.raises(ValueError):
            ev.tune_thresholds(songs, model, [0.5], [0.5], device_metrics=False, cleanups=[(bad.get('min_frames', 1), bad.get('bridge_gap', 0))])
    for cleanups in ([], [(1, 0)] * 9, [(1,)], [(1, 0, 0)]):
        with pytest.raises(ValueError):
            ev.tune_thresholds(songs, model, [0.5], [0.5], device_metrics=False, cleanups=cleanups)
    md.extract_notes_wo_velocity(rolls[2], rolls[3], min_frames=32, bridge_gap=31)        # the ends of both ranges are in
    md.extract_notes_wo_velocity(rolls[2], rolls[3], min_frames=np.int64(2), bridge_gap=np.int32(1))


class FakeModel:
    def __init__(self, name):
        self.name, self.loaded = name, None

    def load_state_dict(self, state):
        self.loaded = state

    def to(self, device):
        return self

    def eval(self):
        return self


def test_transcribe_files_cleanup_keys_and_model_choice(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    (tmp_path / 'a.wav').write_bytes(b'')
    calls, states = [], {'onset.pt': {'transcriber.linear_onset.weight': 0, 'transcriber.linear_feature.weight': 0},
                         'frame.pt': {'transcriber.linear_feature.weight': 0}}
    monkeypatch.setattr(tf.ra, 'UNet', lambda *a, **k: FakeModel('UNet'))
    monkeypatch.setattr(tf.ra, 'UNet_Onset', lambda *a, **k: FakeModel('UNet_Onset'))
    monkeypatch.setattr(tf.torch, 'load', lambda path, **k: states[path])
    monkeypatch.setattr(tf, 'transcribe2midi', lambda files, model, device, out, **kw: calls.append((model, kw)))
    base = ['with', 'device=cpu', f'input={tmp_path}', f'output={tmp_path}']
    tf.main(base + ['min_frames=3', 'bridge_gap=1'])
    tf.main(base + ['bridge_gap=2', 'weight=onset.pt'])
    tf.main(base + ['weight=frame.pt'])
    thr = {'onset_threshold': 0.5, 'frame_threshold': 0.5}
    assert [c[1] for c in calls] == [dict(thr, min_frames=3, bridge_gap=1), dict(thr, bridge_gap=2), thr]
    assert [c[0].name for c in calls] == ['UNet', 'UNet_Onset', 'UNet']
    assert calls[0][0].loaded is None and calls[1][0].loaded is states['onset.pt'] and calls[2][0].loaded is states['frame.pt']


def test_tune_thresholds_script_keys(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import tune_thresholds as tt
    with pytest.raises(SystemExit, match='unknown keys'):
        tt.main(['with', 'device=cpu', 'min_frames=2'])
    seen = {}

    def fake_tune(data, model, on_thr, fr_thr, **kw):
        seen.update(kw)
        return ev.tune_thresholds(sc.stub_songs(40, seeds=(3,)), sc.StubModel(), on_thr, fr_thr, device_metrics=False,
                                  cleanups=kw['cleanups'])
    monkeypatch.setattr(tt, 'load_model', lambda weight, spec, device: FakeModel('UNet'))
    monkeypatch.setattr(tt, 'prepare_VAT_dataset', lambda **kw: (None, None, [], None))
    monkeypatch.setattr(tt, 'tune_thresholds', fake_tune)
    out = tmp_path / 'thr.json'
    res = tt.main(['with', 'device=cpu', 'onset_thresholds=[0.3,0.5]', 'frame_thresholds=[0.5]', 'cleanups=[[1,0],[2,0],[2,1],[3,1]]',
                   f'output={out}'])
    assert seen['cleanups'] == [[1, 0], [2, 0], [2, 1], [3, 1]]
    saved = json.loads(out.read_text())
    c = res['best_cleanup']
    assert saved['cleanups'] == [[1, 0], [2, 0], [2, 1], [3, 1]] and saved['best_cleanup'] == c and len(saved['grids']) == 4
    assert [saved['min_frames'], saved['bridge_gap']] == saved['cleanups'][c]
    assert saved['grid'] == saved['grids'][c] and saved['grids'][1]['note_f1'] == res['grids'][1]['note_f1'].tolist()
