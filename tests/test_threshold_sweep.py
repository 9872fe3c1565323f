"""Decoding thresholds chosen on a validation set, the host side: sweep_counts_host against a brute-force restatement,
the metrics formed from its counters against evaluate_notes / evaluate_frames, tune_thresholds against evaluate_wo_velocity called
pair by pair, the tie rule, the new keys of transcribe_files, and -- without a GPU -- the two things the device kernel relies on:
the integer offset slack the host hands it, and that taking candidates in time order is a maximum matching where "every note
takes its first candidate at once" is not."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import maximum_bipartite_matching

import sweep_cases as sc
from reconvat_amd import decoding as md, evaluate as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON_THR, FR_THR = [0.3, 0.5, 0.7], [0.5, 0.3]
HOP = 512 / 16000


def t(*rolls):
    return [torch.from_numpy(r) for r in rolls]


def decode_brute(onset, frame, thr_on, thr_fr, rule):
    """Notes [(start, pitch, end)] and the painted roll, frame by frame from the decoding rule's definition."""
    T = onset.shape[0]
    on, fr = onset > np.float32(thr_on), frame > np.float32(thr_fr)
    notes, roll = [], np.zeros((T, 88), bool)
    for p in range(88):
        for s in range(T):
            if on[s, p] and not (s > 0 and on[s - 1, p]) and (rule == 'rule2' or fr[s, p]):
                e = s
                while e < T and (on[e, p] or fr[e, p]):
                    e += 1
                notes.append((s, p, e))
                roll[s:e, p] = True
    return notes, roll


def hits_brute(ref, est, offsets):
    """Edge list of the candidate graph with the float64 tests of mir_eval on times frame * 0.032."""
    edges = []
    for i, (rs, rp, re_) in enumerate(ref):
        for j, (es, ep, ee) in enumerate(est):
            if rp != ep or np.around(abs(rs * HOP - es * HOP), 4) > 0.05:
                continue
            if offsets and np.around(abs(re_ * HOP - ee * HOP), 4) > max(0.2 * (re_ * HOP - rs * HOP), 0.05):
                continue
            edges.append((i, j))
    return edges


def max_matching(edges, n_ref, n_est):
    if not edges:
        return 0
    r, c = zip(*edges)
    g = csr_matrix((np.ones(len(edges), bool), (r, c)), shape=(n_ref, n_est))
    return int((maximum_bipartite_matching(g, perm_type='column') >= 0).sum())


def counts_brute(rolls, on_thr, fr_thr, rule):
    on_r, fr_r, on_p, fr_p = rolls
    ref, ref_roll = decode_brute(on_r, fr_r, 0.5, 0.5, rule)
    out = {k: np.zeros((len(on_thr), len(fr_thr)), np.int64) for k in ev.SWEEP_KEYS}
    for a, x in enumerate(on_thr):
        for b, y in enumerate(fr_thr):
            est, est_roll = decode_brute(on_p, fr_p, x, y, rule)
            out['n_est'][a, b] = len(est)
            out['matched'][a, b] = max_matching(hits_brute(ref, est, False), len(ref), len(est))
            out['matched_with_offsets'][a, b] = max_matching(hits_brute(ref, est, True), len(ref), len(est))
            out['frame_tp'][a, b] = int((ref_roll & est_roll).sum())
            out['frame_est'][a, b] = int(est_roll.sum())
    out['n_ref'], out['frame_ref'] = len(ref), int(ref_roll.sum())
    return out


def assert_same_counts(got, want):
    assert set(got) == set(want) == set(ev.SWEEP_KEYS) | {'n_ref', 'frame_ref'}
    for k in ev.SWEEP_KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape
        assert np.array_equal(got[k], want[k]), (k, got[k], want[k])
    assert got['n_ref'] == want['n_ref'] and got['frame_ref'] == want['frame_ref']


@pytest.fixture(scope='module')
def rolls40():
    return sc.random_rolls(40, seed=11, density=0.12)


@pytest.mark.parametrize('rule', ['rule1', 'rule2'])
def test_host_sweep_equals_brute_force(rolls40, rule):
    got = ev.sweep_counts_host(*t(*rolls40), ON_THR, FR_THR, rule=rule)
    want = counts_brute(rolls40, ON_THR, FR_THR, rule)
    assert_same_counts(got, want)
    assert want['n_ref'] > 5 and want['matched'].max() > 0 and len(np.unique(want['n_est'])) > 2


@pytest.mark.parametrize('rule', ['rule1', 'rule2'])
def test_metrics_from_counters_equal_host_metrics(rolls40, rule):
    on_r, fr_r, on_p, fr_p = t(*rolls40)
    counts = ev.sweep_counts_host(on_r, fr_r, on_p, fr_p, ON_THR, FR_THR, rule=rule)
    p_ref, i_ref = md.extract_notes_wo_velocity(on_r, fr_r, rule=rule)
    units = lambda p, i: ev._frames_to_eval_units(*md.notes_to_frames(p, i, fr_r.shape))
    seen = 0
    for a, x in enumerate(ON_THR):
        for b, y in enumerate(FR_THR):
            p_est, i_est = md.extract_notes_wo_velocity(on_p, fr_p, x, y, rule=rule)
            frames = ev.evaluate_frames(*units(p_ref, i_ref), *units(p_est, i_est))
            (pr, ir), (pe, ie) = ev._to_eval_units(p_ref, i_ref), ev._to_eval_units(p_est, i_est)
            m = ev.sweep_metrics(counts, a, b)
            assert (m['note_precision'], m['note_recall'], m['note_f1']) == ev.evaluate_notes(ir, pr, ie, pe, offset_ratio=None)[:3]
            assert (m['note_with_offsets_precision'], m['note_with_offsets_recall'], m['note_with_offsets_f1']) == \
                ev.evaluate_notes(ir, pr, ie, pe)[:3]
            assert m['frame_precision'] == frames['Precision'] and m['frame_recall'] == frames['Recall']
            seen += m['note_f1'] > 0
    assert seen


def test_metrics_zero_guards():
    z = np.zeros((1, 1), np.int64)
    counts = dict(n_est=z, matched=z, matched_with_offsets=z, frame_tp=z, frame_est=z, n_ref=0, frame_ref=0)
    m = ev.sweep_metrics(counts, 0, 0)
    assert all(m[k] == 0.0 for k in m if k != 'frame_f1') and abs(m['frame_f1']) < 1e-15


def test_tune_thresholds_equals_evaluation_pair_by_pair():
    songs = sc.stub_songs(60, seeds=(3, 4))
    model = sc.StubModel()
    for onset in (True, False):
        res = ev.tune_thresholds(songs, model, ON_THR, FR_THR, criterion='note_f1', onset=onset, device_metrics=False)
        names = {'note_precision': 'metric/note/precision', 'note_recall': 'metric/note/recall', 'note_f1': 'metric/note/f1',
                 'note_with_offsets_precision': 'metric/note-with-offsets/precision',
                 'note_with_offsets_recall': 'metric/note-with-offsets/recall', 'note_with_offsets_f1': 'metric/note-with-offsets/f1',
                 'frame_precision': 'metric/frame/precision', 'frame_recall': 'metric/frame/recall', 'frame_f1': 'metric/frame/f1'}
        assert set(res['grid']) == set(names) and res['songs'] == 2
        for a, x in enumerate(ON_THR):
            for b, y in enumerate(FR_THR):
                want = ev.evaluate_wo_velocity(songs, model, x, y, reconstruction=False, onset=onset, device_metrics=False)
                for k, key in names.items():
                    assert res['grid'][k][a, b] == np.mean(want[key]), (k, a, b)
        a, b = res['best_index']
        assert res['grid']['note_f1'][a, b] == res['grid']['note_f1'].max() == res['best_value'] > 0
        assert res['onset_threshold'] == float(np.float32(ON_THR[a])) and res['frame_threshold'] == float(np.float32(FR_THR[b]))
    for criterion in ev.SWEEP_CRITERIA:
        res = ev.tune_thresholds(songs, model, ON_THR, FR_THR, criterion=criterion, device_metrics=False)
        assert res['grid'][criterion][res['best_index']] == res['grid'][criterion].max()
    # VAT=True calls run_on_batch(label, None, False) as evaluate_wo_velocity does, pseudo_onset decodes the label onsets: same as there
    seen = []

    class Recording(sc.StubModel):
        def run_on_batch(self, label, *args):
            seen.append(args)
            return super().run_on_batch(label, *args)
    res = ev.tune_thresholds(songs, Recording(), ON_THR, FR_THR, device_metrics=False, VAT=True, pseudo_onset=True)
    assert seen == [(None, False)] * 2
    want = ev.evaluate_wo_velocity(songs, model, 0.3, 0.5, reconstruction=False, pseudo_onset=True, VAT=True, device_metrics=False)
    assert res['grid']['note_f1'][0, 0] == np.mean(want['metric/note/f1']) and res['grid']['frame_f1'][0, 0] == np.mean(want['metric/frame/f1'])
    with pytest.raises(ValueError):
        ev.tune_thresholds(songs, model, ON_THR, FR_THR, criterion='overlap', device_metrics=False)
    with pytest.raises(ValueError):
        ev.tune_thresholds(songs, model, [], FR_THR, device_metrics=False)
    with pytest.raises(ValueError):
        ev.tune_thresholds(songs, model, [0.5] * 33, FR_THR, device_metrics=False)


def test_tie_rule():
    on, fr = [0.1, 0.3, 0.7, 0.5], [0.9, 0.4, 0.6]
    flat = np.zeros((4, 3))
    assert ev.best_threshold_index(flat, on, fr) == (3, 1)             # all equal: nearest (0.5, 0.5) is (0.5, 0.4) before (0.5, 0.6)
    v = flat.copy(); v[1, 1] = v[2, 2] = v[0, 1] = 1.0                  # (0.3, 0.4) and (0.7, 0.6) are equally far: the lower index
    assert ev.best_threshold_index(v, on, fr) == (1, 1)
    v[0, 0] = 2.0                                                      # a larger value wins wherever it is
    assert ev.best_threshold_index(v, on, fr) == (0, 0)
    # with a model: every pair decodes the same notes from rolls of zeros and ones, so the whole grid ties
    on_r, fr_r, _, _ = sc.random_rolls(40, seed=2)
    song = {'path': 'x', 'onset': torch.from_numpy(on_r), 'frame': torch.from_numpy(fr_r), 'pred_onset': torch.from_numpy(on_r),
            'pred_frame': torch.from_numpy(fr_r)}
    res = ev.tune_thresholds([song], sc.StubModel(), [0.2, 0.6, 0.4], [0.8, 0.5], device_metrics=False)
    assert np.all(res['grid']['note_f1'] == 1.0)
    assert res['best_index'] == (1, 1)                                 # onset 0.6 and 0.4 are equally far from 0.5: the lower index
    assert (res['onset_threshold'], res['frame_threshold']) == (float(np.float32(0.6)), 0.5)


def test_offset_slack_is_the_host_offset_test():
    """The integer interval handed to the kernel admits exactly the end-frame differences that match_notes admits -- at every
    reference duration up to 40 frames, the decisive ones (5, 10, 15: 0.2 * duration is a whole number of hops) included."""
    for start in (0, 7, 1000):
        durations = np.arange(1, 41)
        ref = np.stack([np.full_like(durations, start), start + durations], axis=1)
        slack = ev._offset_slack(ref)
        pr, ir = ev._to_eval_units(np.zeros(len(ref), int), ref)
        for (s, e), (early, late) in zip(ref, slack):
            for d in range(-12, 13):
                if e + d <= s:
                    continue
                pe, ie = ev._to_eval_units([0], np.array([[s, e + d]]))
                hit = len(ev.match_notes(np.array([[s * HOP, e * HOP]]), pr[:1], ie, pe)) == 1
                assert hit == (-early <= d <= late), (s, e, d, early, late)
    # at the decisive durations the host's float64 answer depends on where the note lies, not just on how long it is -- which is why
    # the interval is evaluated per reference note: ten frames from frame 0 admit two frames of difference, from frame 50 only one
    assert ev._offset_slack(np.array([[0, 10], [50, 60]])).tolist() == [[2, 2], [1, 1]]


# The two tests below call no product code: they check the chain INPUT (it separates a wrong matcher from a right one) and the
# ARGUMENT of DESIGN 3.10 (candidates taken in time order are a maximum matching), with `in_time_order` a Python model of the kernel's
# walk, not the kernel.  They pass without the feature; the kernel's own matching is covered by tests/test_threshold_sweep_gpu.py,
# which runs the same inputs through rv_eval_sweep.
def in_time_order(ref, est, edges):
    """Size of the matching the kernel builds: reference notes of a pitch in time order, each takes its earliest free candidate."""
    cand = {}
    for i, j in edges:
        cand.setdefault(i, []).append(j)
    used, n = set(), 0
    for i in sorted(cand, key=lambda i: (ref[i][1], ref[i][0])):
        for j in sorted(cand[i], key=lambda j: est[j][0]):
            if j not in used:
                used.add(j)
                n += 1
                break
    return n


def all_at_once(est, edges):
    """The wrong parallel rule: every reference note claims its first candidate at the same time; an estimate serves one claim."""
    first = {}
    for i, j in edges:
        if i not in first or est[j][0] < est[first[i]][0]:
            first[i] = j
    return len(set(first.values()))


def test_chain_tells_a_wrong_matcher_from_a_right_one():
    rolls = sc.chain_rolls()
    ref, _ = decode_brute(rolls[0], rolls[1], 0.5, 0.5, 'rule2')
    est, _ = decode_brute(rolls[2], rolls[3], 0.5, 0.5, 'rule2')
    assert len(ref) > 100 and len(est) > 100
    for offsets in (False, True):
        edges = hits_brute(ref, est, offsets)
        best = max_matching(edges, len(ref), len(est))
        assert all_at_once(est, edges) < best                          # the input catches "first candidate wins, all notes at once"
        assert in_time_order(ref, est, edges) == best                  # ... and in time order is a maximum matching
    plain, pruned = len(hits_brute(ref, est, False)), len(hits_brute(ref, est, True))
    assert 0.2 * plain < pruned < 0.8 * plain                          # the offset test removes a real share of the edges
    for p in (30, 50):                                                 # both pitches hold long paths: degree 2 on either side
        deg = np.bincount([i for i, j in hits_brute(ref, est, False) if ref[i][1] == p])
        assert deg.max() == 2 and (deg == 2).sum() > 20


def test_in_time_order_is_maximum_on_random_rolls():
    for seed in range(6):
        rolls = sc.random_rolls(130, seed, density=0.15)
        ref, _ = decode_brute(rolls[0], rolls[1], 0.5, 0.5, 'rule2')
        for thr in (0.3, 0.5):
            est, _ = decode_brute(rolls[2], rolls[3], thr, thr, 'rule2')
            for offsets in (False, True):
                edges = hits_brute(ref, est, offsets)
                assert in_time_order(ref, est, edges) == max_matching(edges, len(ref), len(est))


def test_transcribe_files_threshold_keys(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import transcribe_files as tf
    (tmp_path / 'a.wav').write_bytes(b'')
    calls = []

    class Model:
        def to(self, device):
            return self

        def eval(self):
            return self
    monkeypatch.setattr(tf.ra, 'UNet', lambda *a, **k: Model())
    monkeypatch.setattr(tf, 'transcribe2midi', lambda files, model, device, out, **kw: calls.append((files, kw)))
    base = ['with', 'device=cpu', f'input={tmp_path}', f'output={tmp_path}']
    tf.main(base)
    tf.main(base + ['onset_threshold=0.3', 'frame_threshold=0.65'])
    assert [c[1] for c in calls] == [{'onset_threshold': 0.5, 'frame_threshold': 0.5}, {'onset_threshold': 0.3, 'frame_threshold': 0.65}]
    assert calls[0][0] == [str(tmp_path / 'a.wav')]
